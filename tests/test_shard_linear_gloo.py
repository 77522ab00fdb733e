"""Multi-process CPU test of DeepFM's first-order (linear) term over row-sharded weights (dir_amd.shard.ShardedTables.attach_linear,
lookup(want_lin=), lookup_train(with_linear=), ShardedDeepFMTrainer(linear=)) over the gloo backend, world sizes 1, 2, 3 and 8.

What runs here is what runs under RCCL on a GPU box: the linear term riding on the embedding lookup's id exchange (fixed-capacity and
exact paths, micro-batches, de-duplication, the three check modes), the one autograd node whose backward sends both gradients and applies
both owner-side updates, the overflow fallback, the trainer.  The HIP steps cannot run without a GPU, so NumPy stand-ins take their place
through the `backend` injection point, reading and writing the same buffers (include/dir_hip.h: dir_shard_linear_gather_f32,
dir_shard_linear_finish_f32, dir_shard_linear_grad_f32, dir_sparse_ftrl_rows_sorted_payload_f32).
Reference: the FULL, unsharded weights in float64 on the GLOBAL batch -- oracle.np_ref.sparse_ftrl_step once per step for the first-order
weights, [TF-upstream] Adagrad (duplicates summed before the accumulator moves) for the embedding tables -- the same on every rank.
Error measure (tests/test_gpu_shard_bags_train.py::_close): max |got - ref| / (1 + |ref|) <= 1e-5."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.shard_standin import NumpyBackend, run_ranks

LR, ACC0 = 0.3, 0.1
FTRL = dict(lr=0.2, l1=0.0, l2=0.0)
SCENARIOS = ("forward", "train3", "l1_zero", "partitions", "overflow", "lazy_chunks", "trainer")
TOL = 1e-5


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1 + np.abs(ref)))) if got.size else 0.0


# ---- the float64 reference over the FULL weights and the GLOBAL batch ---------------------------------------------------------------
class Reference:
    def __init__(self, full, full_w):
        self.T = [t.astype(np.float64) for t in full]
        self.acc = [np.full(t.shape, ACC0) for t in full]
        self.w = [w.astype(np.float64).reshape(-1, 1) for w in full_w]
        self.n = [np.full(w.shape, ACC0) for w in self.w]
        self.z = [np.zeros(w.shape) for w in self.w]

    def clean(self, ids):
        return np.stack([np.where((ids[:, f] >= 0) & (ids[:, f] < self.T[f].shape[0]), ids[:, f], -1) for f in range(len(self.T))], axis=1)

    def step(self, ids, G, g, ftrl):
        """ids [Bg, F], G [Bg, F*K] = d loss / d emb, g [Bg, 1] = d loss / d lin, over the global batch: Adagrad on the tables, then
        oracle.np_ref.sparse_ftrl_step on the first-order weights (each from pre-step values: they do not interact)."""
        from oracle import np_ref as R
        ids = self.clean(ids)
        R.sparse_adagrad_step(self.T, self.acc, ids, np.asarray(G, np.float64), LR)
        R.sparse_ftrl_step(self.w, self.n, self.z, ids, np.asarray(g, np.float64), ftrl["lr"], ftrl["l1"], ftrl["l2"])


def _draw(vocab, K, seed):
    rng = np.random.default_rng(seed)
    full = [rng.standard_normal((v, K)).astype(np.float32) for v in vocab]
    full_w = [(0.3 * rng.standard_normal(v)).astype(np.float32) for v in vocab]
    return full, full_w


def _batch(vocab, B, seed, rank, step=0, hot=False):
    """A rank's batch: ids below 0 and past the vocabulary included; hot: id 3 of slot 0 twice in every rank's batch."""
    rng = np.random.default_rng(seed + 1000 * step + 17 * rank + 5)
    ids = np.stack([rng.integers(-2, v + 2, size=B) for v in vocab], axis=1).astype(np.int64).reshape(B, len(vocab))
    if hot and B >= 2:
        ids[0, 0] = ids[1, 0] = 3
    return ids


def _tables(rank, world, vocab, K, seed, **kw):
    from dir_amd.shard import ShardedTables, partition_layout
    full, full_w = _draw(vocab, K, seed)
    parts, first, slices = partition_layout(vocab, K, world, rank, kw.get("partitions"))
    local = [torch.from_numpy(full[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    local_w = [torch.from_numpy(full_w[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    be = NumpyBackend(local, vocab, parts, first, world, K)
    st = ShardedTables(local, vocab, backend=be, **kw)
    st.attach_linear(local_w, initial_accumulator_value=ACC0)
    return st, be, full, full_w, slices


def _compare_shards(st, be, ref, slices, what):
    """Every shard's w, n, z and the embedding rows and accumulators against the reference's slices."""
    w, n, z = st.linear_state()
    worst = {}
    for f, (s, e) in enumerate(slices):
        for name, got, want in (("w", w[f], ref.w[f]), ("n", n[f], ref.n[f]), ("z", z[f], ref.z[f])):
            worst[name] = max(worst.get(name, 0.0), _err(got.numpy(), want[s:e, 0]))
        worst["emb"] = max(worst.get("emb", 0.0), _err(be.local[f].numpy(), ref.T[f][s:e]))
        worst["acc"] = max(worst.get("acc", 0.0), _err(st.optimizer["acc"][f], ref.acc[f][s:e]))
    assert all(v <= TOL for v in worst.values()), "%s: %s" % (what, worst)
    return worst


def _train_steps(rank, world, vocab, K, seed, sizes, steps, ftrl, kw, between=None, check_forward=True):
    """`steps` training steps through ONE node (emb, lin) per step against the reference; -> (st, be, ref, [(emb, lin) bitwise-forward ok])."""
    st, be, full, full_w, slices = _tables(rank, world, vocab, K, seed, **kw)
    st.enable_training(LR, ACC0).enable_linear_training(**ftrl)
    ref = Reference(full, full_w)
    F = len(vocab)
    for step in range(steps):
        ids_all = [_batch(vocab, sizes[r], seed, r, step, hot=True) for r in range(world)]
        rngs = [np.random.default_rng(seed + 31 * step + r) for r in range(world)]
        G_all = [rg.standard_normal((sizes[r], F * K)).astype(np.float32) for r, rg in enumerate(rngs)]
        g_all = [rg.standard_normal((sizes[r], 1)).astype(np.float32) for r, rg in enumerate(rngs)]
        ids = torch.from_numpy(ids_all[rank])
        before = st._updates
        emb, lin = st.lookup_train(ids, with_linear=True)
        assert emb.grad_fn is lin.grad_fn or emb.grad_fn.__class__ is lin.grad_fn.__class__, "one autograd node"
        if check_forward:
            idc = ref.clean(ids_all[rank])
            want_lin = np.zeros(sizes[rank], np.float64)
            want_emb = np.zeros((sizes[rank], F * K))
            for f in range(F):
                ok = idc[:, f] >= 0
                want_lin += np.where(ok, ref.w[f][np.maximum(idc[:, f], 0), 0], 0.0)
                want_emb[:, f * K:(f + 1) * K] = np.where(ok[:, None], ref.T[f][np.maximum(idc[:, f], 0)], 0.0)
            assert _err(lin.detach().numpy().reshape(-1), want_lin) <= TOL and _err(emb.detach().numpy(), want_emb) <= TOL, "forward, step %d" % step
        ((emb * torch.from_numpy(G_all[rank])).sum() + (lin * torch.from_numpy(g_all[rank])).sum()).backward()
        assert st._updates == before + 1, "_updates counts one step, not two"
        ref.step(np.concatenate(ids_all), np.concatenate(G_all), np.concatenate(g_all), ftrl)
        _compare_shards(st, be, ref, slices, "after step %d" % step)
        if between is not None:
            between(st, step)
    return st, be, ref, slices


def _sizes(world, base=6):
    return [base + 3 * r if r != world - 1 or world == 1 else 2 for r in range(world)]


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------
def sc_forward(rank, world):
    """1. forward only: lin equals the unsharded float32 slot-order sum exactly; ids < 0 and >= vocab_f; a table with fewer rows than
    ranks; uneven local batches including an empty one; fixed / exact paths, de-duplication, the check modes, one or two micro-batches."""
    from oracle import oracle as O
    vocab, K, seed = [40, 7, 2, 23], 4, 11
    F = len(vocab)
    bias = torch.tensor([0.37], dtype=torch.float32)
    ran = 0
    for kw in ({}, {"dedup": True}, {"mode": "exact"}, {"check": "lazy"}, {"check": "never", "chunks": 1}, {"chunks": 3, "dedup": True},
               {"force_collective": True}):
        st, be, full, full_w, _ = _tables(rank, world, vocab, K, seed, **kw)
        for it, sizes in enumerate(([4 + 3 * r for r in range(world)], [0 if r == world - 1 else 6 + r for r in range(world)],
                                    [5 if r == world - 1 else 0 for r in range(world)])):
            ids = _batch(vocab, sizes[rank], seed, rank, it)
            b = bias if it != 1 else None
            got = st.lookup(torch.from_numpy(ids), want_fm=(it == 0), want_lin=True, lin_bias=b)
            lin, emb = got[-1], got[0]
            idc = np.stack([np.where((ids[:, f] >= 0) & (ids[:, f] < vocab[f]), ids[:, f], -1) for f in range(F)], axis=1).reshape(-1, F)
            # (the oracle takes no vocabulary: ids past a table are handed to it as pruned ones, which is what they are)
            want = O.linear_sparse_sum(full_w, idc, bias=None if b is None else b.numpy(), B=ids.shape[0]) if ids.shape[0] else np.zeros((0, 1), np.float32)
            assert tuple(lin.shape) == (sizes[rank], 1)
            assert np.array_equal(lin.numpy().reshape(-1), np.asarray(want, np.float32).reshape(-1)), (kw, it, lin.numpy().ravel(), np.asarray(want).ravel())
            for f in range(F):
                assert np.array_equal(emb.numpy()[:, f * K:(f + 1) * K], np.where((idc[:, f] >= 0)[:, None], full[f][np.maximum(idc[:, f], 0)], 0))
            # without want_lin: today's return values
            plain = st.lookup(torch.from_numpy(ids))
            assert isinstance(plain, torch.Tensor) and torch.equal(plain, emb)
            ran += 1
        st.check_overflow()
    return "%d lookups exact" % ran


def sc_train3(rank, world):
    """2. three training steps, one id in every rank's batch and twice inside it: every shard's w, n, z and the embedding tables and their
    accumulators match after each step; one node, both updates, one _updates tick per step."""
    st, be, ref, _ = _train_steps(rank, world, [40, 7, 2, 23], 4, 23, _sizes(world), 3, FTRL, {})
    assert be.ftrl_calls == 3
    return "3 steps"


def sc_l1_zero(rank, world):
    """3. l1 > 0: in the float64 reference itself at least one touched weight lands on exactly 0.0 and at least one does not."""
    ftrl = dict(lr=0.2, l1=0.6, l2=0.05)
    vocab, seed, sizes = [40, 7, 2, 23], 29, _sizes(world)
    st, be, ref, slices = _train_steps(rank, world, vocab, 4, seed, sizes, 2, ftrl, {})
    touched = [np.abs(ref.z[f][:, 0]) > 0 for f in range(len(vocab))]          # z moves off its initial 0 exactly where a row was touched
    zeros = sum(int(((ref.w[f][:, 0] == 0.0) & touched[f]).sum()) for f in range(len(vocab)))
    nonzeros = sum(int(((ref.w[f][:, 0] != 0.0) & touched[f]).sum()) for f in range(len(vocab)))
    assert zeros >= 1 and nonzeros >= 1, "the reference must clip some touched weights to 0.0 and keep others (%d / %d)" % (zeros, nonzeros)
    w = st.linear_weights()
    for f, (s, e) in enumerate(slices):                                        # exact zeros where the reference has them
        assert np.array_equal(w[f].numpy() == 0.0, ref.w[f][s:e, 0] == 0.0), "slot %d: zero pattern" % f
    return "%d zeros, %d non-zeros" % (zeros, nonzeros)


def sc_partitions(rank, world):
    """4. partitions="reference" (one slice per small table, dealt round-robin) and an explicit slice list."""
    vocab = [40, 7, 2, 23]
    explicit = [min(world, p) for p in (2, 1, 2, 3)]
    for part in ("reference", explicit):
        _train_steps(rank, world, vocab, 4, 31, _sizes(world), 2, FTRL, {"partitions": part})
    return "reference + %s" % explicit


def sc_overflow(rank, world):
    """5. a slack so small that the first training lookup overflows: the step is repeated on the exact path (linear term included), the
    result is the same, stats["fallbacks"] moved."""
    seen = {}

    def between(st, step):
        seen[step] = st.stats["fallbacks"]
    st, be, ref, _ = _train_steps(rank, world, [40, 7, 2, 23], 4, 37, [40 + r for r in range(world)], 2, FTRL,
                                  {"slack": 0.1, "mode": "fixed", "chunks": 1, "force_collective": True}, between=between)
    assert seen[0] >= 1, "the first training lookup must have overflowed (fallbacks = %s)" % seen
    return "fallbacks %s" % seen


def sc_lazy_chunks(rank, world):
    """6. chunks = 2 with check="lazy" inference lookups between the training steps: pending verdicts stay pending."""
    vocab, K = [40, 7, 2, 23], 4
    pend = []

    def between(st, step):
        ids = torch.from_numpy(_batch(vocab, 5 + rank, 41, rank, 50 + step))
        emb, lin = st.lookup(ids, want_lin=True)
        assert tuple(lin.shape) == (5 + rank, 1)
        pend.append(len([lk for lk in st._unchecked if not lk.checked]))
    st, be, ref, _ = _train_steps(rank, world, vocab, K, 41, _sizes(world), 3, FTRL,
                                  {"chunks": 2, "check": "lazy", "force_collective": True}, between=between)
    waiting = len([lk for lk in st._unchecked if not lk.checked])
    assert pend == [1, 1, 1] and waiting == 1, "a training step must leave the lazy verdict pending (%s, %d)" % (pend, waiting)
    st.check_overflow()
    return "pending %s" % pend


class _Tiny(torch.nn.Module):
    """The part of a DeepFM that ShardedDeepFMTrainer.step uses: F, K, the tower and the replicated linear bias."""

    def __init__(self, F, K):
        super().__init__()
        self.F, self.K, self.units = F, K, 1
        g = torch.Generator().manual_seed(5)
        self.h = torch.nn.Linear(F * K, 6)
        self.o = torch.nn.Linear(6, 1)
        self.linear_bias = torch.nn.Parameter(torch.zeros(1))
        with torch.no_grad():
            for p in (self.h.weight, self.h.bias, self.o.weight, self.o.bias):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))

    def dnn_logit_fn(self, emb, adds=(), range_ok=None):
        return self.o(torch.relu(self.h(emb)))


def _fm(emb, F, K):
    e = emb.view(emb.shape[0], F, K)
    return 0.5 * (e.sum(1) ** 2 - (e ** 2).sum(1)).sum(1, keepdim=True)


def sc_trainer(rank, world):
    """7. ShardedDeepFMTrainer.step with linear= over two steps: the loss, linear_bias and its FTRL state equal the float64 model's and are
    identical on every rank; step_bags with linear= raises."""
    import dir_amd.autograd as ag
    from dir_amd.shard import ShardedDeepFMTrainer
    from oracle import np_ref as R
    ag.fm_logit = _fm                                   # the FM term without a GPU (the trainer resolves it at call time)
    vocab, K, seed = [40, 7, 2, 23], 4, 43
    F = len(vocab)
    ftrl = dict(lr=0.15, l1=0.01, l2=0.02)
    sizes = _sizes(world, 5)
    st, be, full, full_w, slices = _tables(rank, world, vocab, K, seed)
    model = _Tiny(F, K)
    tower = [p for n, p in model.named_parameters() if n != "linear_bias"]
    with pytest.raises(ValueError):
        ShardedDeepFMTrainer(model, st, LR, torch.optim.SGD(list(model.parameters()), lr=0.05), linear=ftrl)
    tr = ShardedDeepFMTrainer(model, st, LR, torch.optim.SGD(tower, lr=0.05), initial_accumulator_value=ACC0, linear=ftrl)
    with pytest.raises(NotImplementedError, match="multi-hot"):
        tr.step_bags(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros((0, 1)))
    with pytest.raises(NotImplementedError, match="multi-hot"):
        tr.predict_bags(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    # the float64 model
    ref = Reference(full, full_w)
    m64 = _Tiny(F, K).double()
    bn, bz = np.full(1, 0.1), np.zeros(1)
    for step in range(2):
        ids_all = [_batch(vocab, sizes[r], seed, r, step, hot=True) for r in range(world)]
        y_all = [np.random.default_rng(seed + 7 * step + r).integers(0, 2, size=(sizes[r], 1)).astype(np.float32) for r in range(world)]
        loss = tr.step(torch.from_numpy(ids_all[rank]), torch.from_numpy(y_all[rank]))
        # reference: the global batch through the float64 model
        idg, yg = ref.clean(np.concatenate(ids_all)), torch.from_numpy(np.concatenate(y_all)).double()
        T = [torch.from_numpy(t).requires_grad_(True) for t in ref.T]
        W = [torch.from_numpy(w).requires_grad_(True) for w in ref.w]
        it = torch.from_numpy(np.maximum(idg, 0))
        ok = torch.from_numpy(idg >= 0)
        emb = torch.cat([T[f][it[:, f]] * ok[:, f:f + 1] for f in range(F)], dim=1)
        lin = sum(W[f][it[:, f]] * ok[:, f:f + 1] for f in range(F)) + m64.linear_bias
        m64.zero_grad()
        logits = _fm(emb, F, K) + m64.dnn_logit_fn(emb) + lin
        logits.retain_grad()
        per = torch.nn.functional.binary_cross_entropy_with_logits(logits, yg, reduction="none")
        per.sum().backward()
        dlogit = logits.grad.numpy()
        for f in range(F):                                  # Adagrad on the full tables (rows without a gradient do not move)
            g = T[f].grad.numpy()
            ref.acc[f] += g * g
            ref.T[f] -= LR * g / np.sqrt(ref.acc[f])
        R.sparse_ftrl_step(ref.w, ref.n, ref.z, idg, dlogit, ftrl["lr"], ftrl["l1"], ftrl["l2"])
        gb = m64.linear_bias.grad.numpy().astype(np.float64)
        with torch.no_grad():
            for n_, p in m64.named_parameters():
                if n_ != "linear_bias":
                    p -= 0.05 * p.grad
            n_new = bn + gb * gb
            z_new = bz + gb - (np.sqrt(n_new) - np.sqrt(bn)) / ftrl["lr"] * m64.linear_bias.numpy()
            m64.linear_bias.copy_(torch.from_numpy(np.where(np.abs(z_new) > ftrl["l1"], (np.sign(z_new) * ftrl["l1"] - z_new)
                                                            / (np.sqrt(n_new) / ftrl["lr"] + 2 * ftrl["l2"]), 0.0)))
            bn, bz = n_new, z_new
        off = sum(sizes[:rank])
        assert _err(float(loss), float(per[off:off + sizes[rank]].sum())) <= TOL, "loss, step %d" % step
        mine = torch.cat([model.linear_bias.data, tr.bias_accum, tr.bias_linear])
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, every[0]) for e in every), "linear_bias and its FTRL state must be identical on every rank"
        assert _err(mine.numpy(), np.concatenate([m64.linear_bias.detach().numpy(), bn, bz])) <= TOL, "bias / n / z, step %d" % step
        for (n_, p), (_, q) in zip(model.named_parameters(), m64.named_parameters()):
            assert _err(p.detach().numpy(), q.detach().numpy()) <= TOL, n_
        _compare_shards(st, be, ref, slices, "trainer step %d" % step)
    return "2 steps"


_FUNCS = dict(forward=sc_forward, train3=sc_train3, l1_zero=sc_l1_zero, partitions=sc_partitions, overflow=sc_overflow,
              lazy_chunks=sc_lazy_chunks, trainer=sc_trainer)


def _scenarios(rank, world, names):
    return [(n, _FUNCS[n](rank, world)) for n in names]


def _run(world, names):
    res = run_ranks(world, _scenarios, names, timeout=600)
    for rank, got in sorted(res.items()):
        assert [n for n, _ in got] == list(names), "rank %d ran %s" % (rank, got)       # every scenario, on every rank
    return res


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_linear_forward_rides_on_the_lookup(world):
    _run(world, ("forward",))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_linear_training_one_node_owner_side_ftrl(world):
    _run(world, ("train3", "l1_zero", "partitions", "overflow", "lazy_chunks"))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_trainer_with_linear_term(world):
    _run(world, ("trainer",))


def test_every_scenario_is_wired():
    assert set(_FUNCS) == set(SCENARIOS)
