"""Multi-process CPU test of the first-order term on the DE-DUPLICATED training exchange (dir_amd.shard.ShardedTables.lookup_train(ids,
with_linear=True, dedup=True); ShardedXDeepFMTrainer, ShardedDeepFMTrainer(dedup=True, linear=)) over the gloo backend, world sizes 2 and 3.

What runs here is what runs under RCCL on a GPU box: the de-duplicating bucket pass, the exchanges with the linear term riding along, ONE
requester-side scatter-sum per micro-batch that gives the gradient slab and the first-order slab on the same sort, the reversed exchanges,
the owner's Adagrad and then FTRL -- on the fixed-capacity path and after a forced overflow (the exact path: one row per entry).  The HIP
steps cannot run without a GPU: tests/shard_standin_dedup_linear.NumpyDedupLinearBackend takes their place (rows_scatter_sum_side defined
through the existing stand-in's scatter_sum: the kernels' order and arithmetic).
Tables, id draws and gradients: tests/test_shard_dedup_train_gloo.py's (VOCAB [50, 400, 1], K = 8; _uniform with ids out of range, _zipf,
_hot with 3000 samples on one row).  Reference: oracle.np_ref.sparse_adagrad_step and sparse_ftrl_step in float64 on the UNSHARDED tables
and weights with the GLOBAL batch.  Error measure and bar: tests/hot_rows_inputs.scaled <= BAR (1e-5)."""
import numpy as np
import pytest
import torch

from tests.hot_rows_inputs import BAR, scaled
from tests.shard_standin import run_ranks
from tests.shard_standin_dedup_linear import NumpyDedupLinearBackend
from tests.test_shard_dedup_train_gloo import F, K, LR, VOCAB, _draw, _grads, _hot, _uniform, _zipf

ACC0 = 0.1
FTRL = dict(lr=0.2, l1=0.01, l2=0.02)


def _draw_w(seed):
    rng = np.random.default_rng(seed + 1)
    return [(0.3 * rng.standard_normal(v)).astype(np.float32) for v in VOCAB]


def _lin_grads(ids_all, seed, scale=1.0):
    return [(scale * np.random.default_rng(seed + 77 + r).standard_normal((a.shape[0], 1))).astype(np.float32) for r, a in enumerate(ids_all)]


def _tables(rank, world, seed, linear=True, **kw):
    from dir_amd.shard import ShardedTables, partition_layout
    full, full_w = _draw(seed), _draw_w(seed)
    parts, first, slices = partition_layout(VOCAB, K, world, rank, None)
    local = [torch.from_numpy(full[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    be = NumpyDedupLinearBackend(local, VOCAB, parts, first, world, K)
    st = ShardedTables(local, VOCAB, backend=be, **kw)
    if linear:
        st.attach_linear([torch.from_numpy(full_w[f][s:e].copy()) for f, (s, e) in enumerate(slices)], initial_accumulator_value=ACC0)
        st.enable_training(LR, ACC0).enable_linear_training(**FTRL)
    return st, be, full, full_w, slices


class Reference:
    """The float64 synchronous step over the FULL tables and first-order weights and the GLOBAL batch."""

    def __init__(self, full, full_w):
        self.T = [t.astype(np.float64) for t in full]
        self.a = [np.full(t.shape, ACC0) for t in full]
        self.w = [w.astype(np.float64).reshape(-1, 1) for w in full_w]
        self.n = [np.full(w.shape, ACC0) for w in self.w]
        self.z = [np.zeros(w.shape) for w in self.w]

    def step(self, ids_all, G_all, g_all):
        from oracle import np_ref as R
        ids = np.concatenate(ids_all)
        ids = np.where((ids >= 0) & (ids < np.array(VOCAB)[None, :]), ids, -1)
        R.sparse_adagrad_step(self.T, self.a, ids, np.concatenate(G_all).astype(np.float64), LR)
        R.sparse_ftrl_step(self.w, self.n, self.z, ids, np.concatenate(g_all).astype(np.float64), FTRL["lr"], FTRL["l1"], FTRL["l2"])

    def compare(self, st, be, slices, what):
        w, n, z = st.linear_state()
        worst = {}
        for f, (s, e) in enumerate(slices):
            if e == s:
                continue
            for name, got, want in (("emb", be.local[f].numpy(), self.T[f][s:e]), ("acc", st.optimizer["acc"][f], self.a[f][s:e]),
                                    ("w", w[f].numpy(), self.w[f][s:e, 0]), ("n", n[f].numpy(), self.n[f][s:e, 0]),
                                    ("z", z[f].numpy(), self.z[f][s:e, 0])):
                worst[name] = max(worst.get(name, 0.0), scaled(got, want))
        assert all(v <= BAR for v in worst.values()), "%s: off the float64 synchronous step: %s" % (what, worst)
        return worst


def _train(st, ids, G, g, dedup=True):
    emb, lin = st.lookup_train(torch.from_numpy(ids), with_linear=True, dedup=dedup)
    ((emb * torch.from_numpy(G)).sum() + (lin * torch.from_numpy(g)).sum()).backward()
    return emb.detach(), lin.detach()


def _nonempty_chunks(st, B):
    plans = [p for (b, slot, cap), p in st._plans.items() if slot == "train_dedup" and b == B]
    assert len(plans) == 1, (B, list(st._plans.keys()), st._use_exact)
    return sum(1 for s, e in plans[0].bounds if e > s), len(plans[0].bounds)


def sc_steps(rank, world):
    """Five steps on the fixed path (uniform with out-of-range ids and an empty rank, Zipf), three pipeline settings: every step against
    the reference; the forward bitwise dedup=False's; ONE fused call per non-empty micro-batch and no linear_grad; capacities apart."""
    for kw in ({}, {"chunks": 1}, {"chunks": 2, "force_collective": True}):
        st, be, full, full_w, slices = _tables(rank, world, 11, **kw)
        twin = _tables(rank, world, 11, **kw)[0]
        ref = Reference(full, full_w)
        for step in range(5):
            sizes = [0 if r == 1 else 24 + 6 * r for r in range(world)]           # uneven, rank 1 empty; the same every step (one capacity)
            ids_all = [(_uniform if step % 2 == 0 else _zipf)(n, 100 + step, r) for r, n in enumerate(sizes)]
            G_all, g_all = _grads(ids_all, 200 + step), _lin_grads(ids_all, 300 + step)
            ids = torch.from_numpy(ids_all[rank])
            with torch.no_grad():
                plain_emb, plain_lin = st.lookup(ids, want_lin=True)
            if step == 0:                                # (twin tables, the same shards: the non-dedup training forward itself)
                e2, l2 = twin.lookup_train(ids, with_linear=True)
            calls, empty, lg = be.side_calls, be.side_calls_empty, be.linear_grad_calls
            emb, lin = _train(st, ids_all[rank], G_all[rank], g_all[rank])
            if step == 0:
                assert torch.equal(emb, e2.detach()) and torch.equal(lin, l2.detach()), "the forward differs from dedup=False's"
            assert torch.equal(emb, plain_emb) and torch.equal(lin, plain_lin), "the training forward differs from the lookup's"
            live, chunks = _nonempty_chunks(st, ids_all[rank].shape[0])
            assert be.side_calls - calls == live, "%d fused calls for %d non-empty micro-batches" % (be.side_calls - calls, live)
            assert be.side_calls_empty - empty == chunks - live, "an empty micro-batch's slabs are zero-filled by the same call"
            assert be.linear_grad_calls == lg, "linear_grad ran on the fixed path of a de-duplicated lookup"
            assert be.scatter_calls == 0, "the scatter-sum without the side ran beside the fused one"
            ref.step(ids_all, G_all, g_all)
            ref.compare(st, be, slices, "%s step %d" % (kw, step))
        assert st.stats["fallbacks"] == 0 and st._updates == 5 and not st._use_exact
        # the one-position-per-entry capacity is what the first lookup agreed on; the de-duplicated one may only have shrunk
        assert st._cap_train == st._cap0 and st._cap_train_dedup <= st._cap0, (st._cap_train, st._cap_train_dedup, st._cap0)
    return "ok"


def sc_mixed(rank, world):
    """dedup=True, dedup=False, dedup=True on ONE set of tables: both routes take the same synchronous step."""
    st, be, full, full_w, slices = _tables(rank, world, 13)
    ref = Reference(full, full_w)
    for step, dedup in enumerate((True, False, True)):
        ids_all = [_zipf(25 + 6 * r, 400 + step, r) for r in range(world)]
        G_all, g_all = _grads(ids_all, 500 + step), _lin_grads(ids_all, 600 + step)
        calls, lg = be.side_calls, be.linear_grad_calls
        _train(st, ids_all[rank], G_all[rank], g_all[rank], dedup)
        assert (be.side_calls > calls) == dedup and (be.linear_grad_calls > lg) == (not dedup)
        ref.step(ids_all, G_all, g_all)
        ref.compare(st, be, slices, "mixed step %d dedup=%s" % (step, dedup))
    assert st._cap_train == st._cap0
    return "ok"


def sc_hot(rank, world):
    """One row hit 3000 times in 4096 samples of rank 0: one run of 3000 entries through both sums' tile cuts and combine."""
    st, be, full, full_w, slices = _tables(rank, world, 19, chunks=1)
    ref = Reference(full, full_w)
    ids_all = [_hot(0, 600, r) for r in range(world)]
    G_all, g_all = _grads(ids_all, 700, 0.5), _lin_grads(ids_all, 800, 0.5)
    _train(st, ids_all[rank], G_all[rank], g_all[rank])
    if rank == 0:
        assert be.longest_run >= 3000, be.longest_run
    assert be.linear_grad_calls == 0
    ref.step(ids_all, G_all, g_all)
    return str(ref.compare(st, be, slices, "hot row"))


def sc_overflow(rank, world):
    """Slabs too small for the first de-duplicated training lookup: it is repaired on the exact path -- one row per entry, where lin
    comes back and d lin goes out as on the non-dedup exact path (linear_grad) -- with the same result; and mode="exact" outright."""
    for kw in (dict(slack=0.05, mode="fixed", chunks=1, force_collective=True), dict(mode="exact")):
        st, be, full, full_w, slices = _tables(rank, world, 23, **kw)
        ref = Reference(full, full_w)
        rng = np.random.default_rng(900)
        ids_all = [np.stack([rng.permutation(400)[:40 + r] % v for v in VOCAB], axis=1).astype(np.int64) for r in range(world)]
        G_all, g_all = _grads(ids_all, 800), _lin_grads(ids_all, 850)
        with torch.no_grad():
            plain_emb, plain_lin = st.lookup(torch.from_numpy(ids_all[rank]), want_lin=True)
        fb = st.stats["fallbacks"]
        emb, lin = _train(st, ids_all[rank], G_all[rank], g_all[rank])
        if "slack" in kw:
            assert st.stats["fallbacks"] > fb, st.stats
        assert torch.equal(emb, plain_emb) and torch.equal(lin, plain_lin)
        assert be.side_calls == 0 and be.linear_grad_calls == 1 and be.scatter_calls == 1 and be.longest_run == 1, \
            (be.side_calls, be.linear_grad_calls, be.scatter_calls, be.longest_run)
        ref.step(ids_all, G_all, g_all)
        ref.compare(st, be, slices, "exact path %s" % kw)
    return "ok"


def sc_refusals(rank, world):
    """What stays refused under dedup: row groups; with_linear under Adam; lookup_rows_train has no linear term."""
    from dir_amd.shard import ShardedTables, partition_layout
    ids = torch.from_numpy(_uniform(4, 31, rank))
    parts, first, sl = partition_layout(VOCAB, K, world, rank, None)
    local2 = [torch.zeros((e - s, 2 * K)) for s, e in sl]
    st2 = ShardedTables(local2, VOCAB, backend=NumpyDedupLinearBackend(local2, VOCAB, parts, first, world, 2 * K), groups=2).enable_training(LR)
    with pytest.raises(NotImplementedError, match="groups"):
        st2.lookup_train(ids, dedup=True)
    st3 = _tables(rank, world, 31, linear=False)[0]
    st3.attach_linear([torch.zeros(t.shape[0]) for t in st3.local_tables])
    st3.enable_training_adam()
    st3.enable_linear_training(0.1)
    with pytest.raises(NotImplementedError, match="enable_training_adam"):
        st3.lookup_train(ids, with_linear=True, dedup=True)
    st4 = _tables(rank, world, 31)[0]
    with pytest.raises(TypeError):
        st4.lookup_rows_train(ids, with_linear=True)
    return "ok"


class _TinyDeepFM(torch.nn.Module):
    """The part of a DeepFM that ShardedDeepFMTrainer.step uses, on CPU tensors: F, K, the tower and the replicated linear bias."""

    def __init__(self):
        super().__init__()
        self.F, self.K, self.units = F, K, 1
        g = torch.Generator().manual_seed(5)
        self.h, self.o = torch.nn.Linear(F * K, 6), torch.nn.Linear(6, 1)
        self.linear_bias = torch.nn.Parameter(torch.zeros(1))
        with torch.no_grad():
            for p in (self.h.weight, self.h.bias, self.o.weight, self.o.bias):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))

    def dnn_logit_fn(self, emb, adds=(), range_ok=None):
        return self.o(torch.relu(self.h(emb)))


def _fm(emb, F_, K_):
    e = emb.view(emb.shape[0], F_, K_)
    return 0.5 * (e.sum(1) ** 2 - (e ** 2).sum(1)).sum(1, keepdim=True)


class _TinyXDeepFM(_TinyDeepFM):
    """The part of an XDeepFM that ShardedXDeepFMTrainer.step uses, on CPU tensors (the model's own CIN and tower kernels are HIP only:
    tests/test_gpu_shard_xdeepfm.py trains the real model): m, D and forward_embedded with one outer-product layer in torch."""

    def __init__(self):
        super().__init__()
        self.m, self.D = F, K
        self.cin_w = torch.nn.Parameter(0.1 * torch.randn((4, F * F), generator=torch.Generator().manual_seed(6)))
        self.cin_o = torch.nn.Linear(4, 1)
        with torch.no_grad():                            # (the same replicated model on every rank)
            self.cin_o.weight.copy_(0.3 * torch.randn((1, 4), generator=torch.Generator().manual_seed(8)))
            self.cin_o.bias.zero_()
        self.seen_range_ok = []

    def forward_embedded(self, emb, linear_logit=None, range_ok=None):
        self.seen_range_ok.append(range_ok)
        x0 = emb.view(-1, F, K)
        z = torch.einsum("bik,bjk->bijk", x0, x0).reshape(-1, F * F, K)
        out = self.cin_o(torch.einsum("hq,bqk->bhk", self.cin_w, z).sum(-1)) + self.dnn_logit_fn(emb)
        return out if linear_logit is None else out + linear_logit


def sc_trainers(rank, world):
    """One SPMD step of ShardedXDeepFMTrainer (dedup is its default; with and without linear=) and of ShardedDeepFMTrainer(dedup=True,
    linear=) on CPU models: runs to completion through the fused scatter-sum, every shard that holds rows moves, the dense parameters and
    the bias's FTRL state are the same on every rank."""
    import dir_amd.autograd as ag
    import torch.distributed as dist
    from dir_amd.shard import ShardedDeepFMTrainer, ShardedXDeepFMTrainer
    ag.fm_logit = _fm                                   # the FM term without a GPU (the trainer resolves it at call time)
    done = []
    for cls, model, linear in ((ShardedXDeepFMTrainer, _TinyXDeepFM(), FTRL), (ShardedXDeepFMTrainer, _TinyXDeepFM(), None),
                               (ShardedDeepFMTrainer, _TinyDeepFM(), FTRL)):
        st, be, full, full_w, slices = _tables(rank, world, 41, linear=False)
        tower = [p for n, p in model.named_parameters() if n != "linear_bias"]
        if linear is not None:
            with pytest.raises(ValueError, match="first-order"):                      # tables without linear rows
                cls(model, st, LR, torch.optim.SGD(tower, lr=0.05), linear=linear)
            st.attach_linear([torch.from_numpy(full_w[f][s:e].copy()) for f, (s, e) in enumerate(slices)], initial_accumulator_value=ACC0)
            with pytest.raises(ValueError, match="linear_bias"):
                cls(model, st, LR, torch.optim.SGD(list(model.parameters()), lr=0.05), linear=linear)
        extra = {} if cls is ShardedXDeepFMTrainer else {"dedup": True}
        tr = cls(model, st, LR, torch.optim.SGD(tower, lr=0.05), initial_accumulator_value=ACC0, linear=linear, **extra)
        assert tr.dedup is True
        ids = _zipf(40 + 8 * rank, 1000, rank)
        ids[:, 0] = (np.arange(ids.shape[0]) + 13 * rank) % VOCAB[0]         # every shard of every slot is named by some rank's batch
        ids[:, 1] = (np.arange(ids.shape[0]) * 37 + 11 * rank) % VOCAB[1]
        y = np.random.default_rng(7 + rank).integers(0, 2, size=(ids.shape[0], 1)).astype(np.float32)
        before = [t.clone() for t in be.local]
        wb = [r.clone() for r in st.lin_rows] if linear is not None else None
        dense0 = [p.detach().clone() for p in tower]
        loss = tr.step(torch.from_numpy(ids), torch.from_numpy(y))
        assert torch.isfinite(loss) and st._updates == 1 and st.stats["fallbacks"] == 0
        if linear is not None:
            assert be.side_calls >= 1 and be.linear_grad_calls == 0 and be.scatter_calls == 0
        else:
            assert be.scatter_calls >= 1 and be.side_calls == 0
        if cls is ShardedXDeepFMTrainer:
            assert model.seen_range_ok == [True], "the range verdict comes from the sharded tables: %s" % model.seen_range_ok
        for f, (s, e) in enumerate(slices):
            if e > s:                                    # every shard that holds rows of slot f was named by some rank's batch
                assert not torch.equal(before[f], be.local[f]), "slot %d's shard did not move" % f
                if linear is not None:
                    assert not torch.equal(wb[f][:, :3], st.lin_rows[f][:, :3]), "slot %d's first-order shard did not move" % f
        assert all(not torch.equal(a, p.detach()) for a, p in zip(dense0, tower))
        mine = torch.cat([p.detach().reshape(-1) for p in model.parameters()] + ([tr.bias_accum, tr.bias_linear] if linear is not None else []))
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, every[0]) for e in every), "the replicated parameters must be identical on every rank"
        if linear is not None:
            assert float(model.linear_bias.detach().abs().sum()) > 0 and float(tr.bias_accum) > ACC0
        else:
            assert float(model.linear_bias.detach().abs().sum()) == 0
        done.append(cls.__name__)
    return done


_FUNCS = dict(steps=sc_steps, mixed=sc_mixed, hot=sc_hot, overflow=sc_overflow, refusals=sc_refusals, trainers=sc_trainers)


def _scenarios(rank, world, names):
    return [(n, _FUNCS[n](rank, world)) for n in names]


def _run(world, names):
    res = run_ranks(world, _scenarios, names, timeout=600)
    for rank, got in sorted(res.items()):
        assert [n for n, _ in got] == list(names), "rank %d ran %s" % (rank, got)
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_dedup_linear_training_matches_float64(world):
    _run(world, ("steps", "mixed", "hot", "overflow"))


@pytest.mark.parametrize("world", [2, 3])
def test_trainers_and_refusals(world):
    _run(world, ("refusals", "trainers"))
