"""Multi-process CPU test of DeepFM's first-order term over row-sharded multi-hot bags (dir_amd.shard.ShardedTables.lookup_bags(want_lin=),
lookup_bags_train(with_linear=), ShardedDeepFMTrainer.step_bags / predict_bags with linear=) over the gloo backend, world sizes 1, 2, 3, 8.

What runs here is what runs under RCCL on a GPU box: the term riding on the bag lookup (the float exchange behind the partial-row
exchange, the plan's float buffers, the overflow repeat), the one autograd node whose backward scatters both gradients, exchanges the
rows and then the floats and applies Adagrad, then FTRL, on the owner; the trainer.  The HIP steps cannot run without a GPU: the NumPy
stand-ins of tests/shard_standin_bags_linear.py take their place through the `backend` injection point, on the kernels' buffers.
Reference: float64 over the FULL weights and the GLOBAL bags -- oracle.np_ref.sparse_ftrl_step on the per-entry gradients w_e * c_bag *
d lin[b] for the first-order weights, tests.test_shard_bags_train_gloo.ref_step for the tables -- the same on every rank.
Error measure (the sibling tests' _close): max |got - ref| / (1 + |ref|) <= 1e-5.  For the forward term that bound has a tenfold margin:
a sample's term is at most ~70 fp32 additions of products of magnitude ~0.3, a rounding error near 1e-6."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.shard_standin import NumpyBackend, run_ranks
from tests.shard_standin_bags_linear import LIN_COMBINERS, BagsLinearBackend, lin_entries, lin_forward64, lin_ftrl64
from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr
from tests.test_shard_bags_train_gloo import _close, bags_forward64, ref_step
from tests.test_shard_linear_gloo import Reference, _Tiny, _fm

LR, ACC0, TOL = 0.3, 0.1, 1e-5
FTRL = dict(lr=0.2, l1=0.01, l2=0.02)
SCENARIOS = ("forward", "train3", "overflow", "trainer")


def _tables(rank, world, vocab, K, linear=True, backend=BagsLinearBackend, **kw):
    from dir_amd.shard import ShardedTables, partition_layout
    rng = np.random.default_rng(7)                                  # the same full tables and weights on every rank
    full = [(rng.standard_normal((v, K)) * 0.5).astype(np.float32) for v in vocab]
    full_w = [(0.3 * rng.standard_normal(v)).astype(np.float32) for v in vocab]
    parts, first, slices = partition_layout(vocab, K, world, rank, kw.get("partitions"))
    local = [torch.from_numpy(full[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    st = ShardedTables(local, vocab, backend=backend(local, vocab, parts, first, world, K), **kw)
    if linear:
        st.attach_linear([torch.from_numpy(full_w[f][s:e].copy()) for f, (s, e) in enumerate(slices)], initial_accumulator_value=ACC0)
    return st, full, full_w, slices


def _csr(bags, F, fmaj):
    v, o, w = to_csr(bags, F, fmaj)
    return torch.from_numpy(v), torch.from_numpy(o), None if w is None else torch.from_numpy(w)


def _compare(st, ref, acc, lref, slices, what):
    """Every shard's w, n, z, embedding rows and Adagrad accumulators against the reference's slices."""
    w, n, z = st.linear_state()
    worst = {}
    for f, (s, e) in enumerate(slices):
        for name, got, want in (("w", w[f], lref.w[f]), ("n", n[f], lref.n[f]), ("z", z[f], lref.z[f])):
            worst[name] = max(worst.get(name, 0.0), _close(got.numpy(), want[s:e, 0]))
        worst["emb"] = max(worst.get("emb", 0.0), _close(st.local_tables[f].numpy(), ref[f][s:e]))
        worst["acc"] = max(worst.get("acc", 0.0), _close(st.optimizer["acc"][f], acc[f][s:e]))
    assert all(v <= TOL for v in worst.values()), "%s: %s" % (what, worst)


def sc_forward(rank, world):
    """1. Every CASES entry under each linear combiner: lin against float64, a bias added once, (emb, fm) untouched by the term; a lookup
    without want_lin on tables WITH first-order weights equals the one on tables without them."""
    vocab, K, max_len = [500, 1000, 7], 8, [1, 60, 4]
    F = len(vocab)
    st, full, full_w, _ = _tables(rank, world, vocab, K)
    plain, _, _, _ = _tables(rank, world, vocab, K, linear=False, backend=NumpyBackend)
    rng = np.random.default_rng(1000 + rank)
    bias = torch.tensor([0.37])
    with pytest.raises(ValueError):
        st.lookup_bags(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), want_lin=True, lin_combiner=["sum"] * F)
    with pytest.raises(RuntimeError, match="attach_linear"):
        plain.lookup_bags(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), want_lin=True)
    for c, (wmode, comb, mn, fmaj, prune) in enumerate(CASES):
        B = (23, 0)[(rank + c) % 2] if world > 1 else 23
        bags = draw_bags(rng, B, vocab, max_len, wmode)
        args = _csr(bags, F, fmaj)
        kw = dict(combiner=comb, max_norm=mn, field_major=fmaj, flags=1 if prune else 0, want_fm=True)
        emb0, fm0 = plain.lookup_bags(*args, **kw)
        emb1, fm1 = st.lookup_bags(*args, **kw)
        assert torch.equal(emb0, emb1) and torch.equal(fm0, fm1), "case %d: attach_linear changed a lookup that did not ask for the term" % c
        for lc in LIN_COMBINERS:
            emb, fm, lin = st.lookup_bags(*args, want_lin=True, lin_combiner=lc, lin_bias=bias if lc == "mean" else None, **kw)
            want = lin_forward64(full_w, lin_entries(bags, vocab, lc, prune), B) + (0.37 if lc == "mean" else 0.0)
            err = _close(lin.numpy().reshape(-1), want)
            assert lin.shape == (B, 1) and err <= TOL, "case %d %s: lin err %.3g" % (c, lc, err)
            assert torch.equal(emb, emb0) and torch.equal(fm, fm0), "case %d %s: the term changed emb / fm" % (c, lc)
    return "forward"


def _train(rank, world, spec):
    """Steps of lookup_bags_train(with_linear=True) -> ONE node (emb, lin) -- against the float64 reference of the global batches."""
    vocab, K, max_len, batch = spec["vocab"], spec["K"], spec["max_len"], spec["batch"]
    F = len(vocab)
    kw = {k: spec[k] for k in ("partitions", "slack") if k in spec}
    st, full, full_w, slices = _tables(rank, world, vocab, K, **kw)
    with pytest.raises(RuntimeError, match="enable_linear_training"):
        st.enable_training(LR, ACC0).lookup_bags_train(torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), with_linear=True)
    st.enable_linear_training(**FTRL)
    ref = [t.astype(np.float64) for t in full]
    acc = [np.full(t.shape, ACC0) for t in full]
    lref = Reference(full, full_w)
    for step, case in enumerate(spec["steps"]):
        wmode, comb, mn, fmaj, prune = CASES[case]
        lc = LIN_COMBINERS[(step + spec.get("lc0", 0)) % 3]
        rng = np.random.default_rng(1000 + step)                    # every rank draws the GLOBAL batch, then takes its own part
        Bs = [batch[(r + step) % len(batch)] for r in range(world)]
        bags_all = [draw_bags(rng, Bs[r], vocab, max_len, wmode) for r in range(world)]
        for bl in bags_all:                                         # one row repeated inside bags, across bags and across ranks
            for row in bl:
                if len(row[1][0]) >= 2:
                    row[1][0][:2] = 3
        G_all = [rng.standard_normal((Bs[r], F * K)).astype(np.float32) for r in range(world)]
        g_all = [rng.standard_normal((Bs[r], 1)).astype(np.float32) for r in range(world)]
        args = _csr(bags_all[rank], F, fmaj)
        kw_b = dict(combiner=comb, max_norm=mn, field_major=fmaj, flags=1 if prune else 0)
        inf = st.lookup_bags(*args, want_lin=True, lin_combiner=lc, **kw_b)
        before, calls = st._updates, st.backend.ftrl_calls
        emb, lin = st.lookup_bags_train(*args, with_linear=True, lin_combiner=lc, **kw_b)
        assert emb.grad_fn is lin.grad_fn or emb.grad_fn.__class__ is lin.grad_fn.__class__, "one autograd node"
        assert torch.equal(emb.detach(), inf[0]) and torch.equal(lin.detach(), inf[2]), "training forward != inference forward, step %d" % step
        want = lin_forward64(lref.w, lin_entries(bags_all[rank], vocab, lc, prune), Bs[rank])
        assert lin.shape == (Bs[rank], 1) and _close(lin.detach().numpy().reshape(-1), want) <= TOL, "forward lin, step %d" % step
        # an inference lookup of OTHER bags between the forward and its backward leaves the backward's buffers alone
        other = draw_bags(np.random.default_rng(5000 + 10 * step + rank), Bs[rank], vocab, max_len, wmode)
        st.lookup_bags(*_csr(other, F, fmaj), want_lin=True, lin_combiner=LIN_COMBINERS[(step + 1) % 3], **kw_b)
        ((emb * torch.from_numpy(G_all[rank])).sum() + (lin * torch.from_numpy(g_all[rank])).sum()).backward()
        assert st._updates == before + 1 and st.backend.ftrl_calls == calls + 1, "one optimiser step: _updates moves once"
        bags_g = [b for bl in bags_all for b in bl]
        ref_step(ref, acc, bags_g, np.concatenate(G_all, axis=0), comb, mn, prune, LR)
        lin_ftrl64(lref.w, lref.n, lref.z, lin_entries(bags_g, vocab, lc, prune), np.concatenate(g_all, axis=0), **FTRL)
        _compare(st, ref, acc, lref, slices, "step %d (case %d, %s)" % (step, case, lc))
    return st


def sc_train3(rank, world):
    """2. Three steps (each linear combiner once): w, n, z of every shard, the tables and their accumulators."""
    batch = [17] if world == 1 else ([23, 0] if world == 2 else [9, 0, 11, 3, 1, 6, 0, 5][:max(3, world)])
    _train(rank, world, dict(vocab=[120, 300, 9], K=4, max_len=[5, 30, 3], batch=batch, steps=[2, 1, 0]))
    if world == 3:                                                  # a table cut fewer ways than there are ranks, dealt round-robin
        _train(rank, world, dict(vocab=[300, 2, 41], K=4, max_len=[12, 3, 1], batch=[9, 17, 4], partitions=[2, 1, 3], steps=[3, 4], lc0=1))
    return "train3"


def sc_overflow(rank, world):
    """3. Tiny first capacities: the inference lookup and the training forward repeat with grown capacities and carry the term."""
    if world == 1:
        return "nothing can overflow on one rank"
    st = _train(rank, world, dict(vocab=[400, 50, 9], K=4, max_len=[40, 3, 5], batch=[40, 31], slack=0.02, steps=[0, 3]))
    assert st.stats.get("bag_fallbacks", 0) >= 1, st.stats
    caps = [None] * world
    dist.all_gather_object(caps, tuple(st._bag_cap))
    assert len(set(caps)) == 1, caps
    return "overflow"


class _Col:
    def __init__(self, combiner):
        self.combiner = combiner


class _TinyBags(_Tiny):
    """tests.test_shard_linear_gloo._Tiny with what step_bags reads off a DeepFM: the columns' combiners, max_norm, the linear combiner."""

    def __init__(self, F, K, combs, lin_comb):
        super().__init__(F, K)
        self.dnn_feature_columns = [_Col(c) for c in combs]
        self.linear_sparse_combiner = lin_comb

    def _max_norm(self):
        return None

    def dnn_logit_fn(self, emb, adds=(), range_ok=None):
        return sum(adds, super().dnn_logit_fn(emb))


def sc_trainer(rank, world):
    """4. ShardedDeepFMTrainer.step_bags with linear= over two steps against the float64 three-term model; the bias and its FTRL state are
    identical on every rank; predict_bags carries the term."""
    import dir_amd.autograd as ag
    from dir_amd.shard import ShardedDeepFMTrainer
    ag.fm_logit = _fm                                   # the FM term without a GPU (the trainer resolves it at call time)
    vocab, K, max_len = [40, 90, 5], 4, [1, 12, 3]
    F = len(vocab)
    combs, lc = ["sum", "mean", "sqrtn"], "sqrtn"
    B = 6
    st, full, full_w, slices = _tables(rank, world, vocab, K)
    model = _TinyBags(F, K, combs, lc)
    tower = [p for n, p in model.named_parameters() if n != "linear_bias"]
    tr = ShardedDeepFMTrainer(model, st, LR, torch.optim.SGD(tower, lr=0.05), initial_accumulator_value=ACC0, linear=FTRL)
    ref = [t.astype(np.float64) for t in full]
    acc = [np.full(t.shape, ACC0) for t in full]
    lref = Reference(full, full_w)
    m64 = _Tiny(F, K).double()
    bn, bz = np.full(1, 0.1), np.zeros(1)

    def logits64(T, W, bags):
        emb = bags_forward64(T, bags, combs, None, False)
        lin = torch.zeros((len(bags), 1), dtype=torch.float64)
        for f, (bi, ids, coef) in enumerate(lin_entries(bags, vocab, lc, False)):
            lin = lin.index_add(0, torch.from_numpy(bi), torch.from_numpy(coef)[:, None] * W[f][torch.from_numpy(ids)])
        return _fm(emb, F, K) + m64.dnn_logit_fn(emb) + lin + m64.linear_bias
    for step in range(2):
        rng = np.random.default_rng(300 + step)
        bags_all = [draw_bags(rng, B + r % 2, vocab, max_len, "pos") for r in range(world)]
        y_all = [rng.integers(0, 2, size=(B + r % 2, 1)).astype(np.float32) for r in range(world)]
        v, o, w = _csr(bags_all[rank], F, step == 1)
        loss = tr.step_bags(v, o, torch.from_numpy(y_all[rank]), weights=w, field_major=step == 1)
        bags_g = [b for bl in bags_all for b in bl]
        T = [torch.from_numpy(t).requires_grad_(True) for t in ref]
        W = [torch.from_numpy(x).requires_grad_(True) for x in lref.w]
        m64.zero_grad()
        logits = logits64(T, W, bags_g)
        logits.retain_grad()
        per = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(np.concatenate(y_all)).double(), reduction="none")
        per.sum().backward()
        for f in range(F):                                  # Adagrad on the full tables (rows without a gradient do not move)
            g = T[f].grad.numpy() if T[f].grad is not None else np.zeros_like(ref[f])
            acc[f] += g * g
            ref[f] -= LR * g / np.sqrt(acc[f])
        lin_ftrl64(lref.w, lref.n, lref.z, lin_entries(bags_g, vocab, lc, False), logits.grad.numpy(), **FTRL)
        gb = m64.linear_bias.grad.numpy().astype(np.float64)
        with torch.no_grad():
            for n_, p in m64.named_parameters():
                if n_ != "linear_bias":
                    p -= 0.05 * p.grad
            new = NumpyBackend._ftrl(m64.linear_bias.detach().numpy().copy(), bn, bz, gb, FTRL["lr"], FTRL["l1"], FTRL["l2"])
            m64.linear_bias.copy_(torch.from_numpy(new[0]))
            bn, bz = new[1], new[2]
        off = sum(B + r % 2 for r in range(rank))
        assert _close(np.array([float(loss)]), np.array([float(per[off:off + B + rank % 2].sum())])) <= TOL, "loss, step %d" % step
        mine = torch.cat([model.linear_bias.data, tr.bias_accum, tr.bias_linear])
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, every[0]) for e in every), "linear_bias and its FTRL state must be identical on every rank"
        assert _close(mine.numpy(), np.concatenate([m64.linear_bias.detach().numpy(), bn, bz])) <= TOL, "bias / n / z, step %d" % step
        for (n_, p), (_, q) in zip(model.named_parameters(), m64.named_parameters()):
            assert _close(p.detach().numpy(), q.detach().numpy()) <= TOL, n_
        _compare(st, ref, acc, lref, slices, "trainer step %d" % step)
    v, o, w = _csr(bags_all[rank], F, False)
    got = tr.predict_bags(v, o, w)
    with torch.no_grad():
        want = logits64([torch.from_numpy(t) for t in ref], [torch.from_numpy(x) for x in lref.w], bags_all[rank]).numpy()
    assert got.shape == (B + rank % 2, 1) and _close(got.numpy(), want) <= 1e-4, "predict_bags"
    return "2 steps"


_FUNCS = dict(forward=sc_forward, train3=sc_train3, overflow=sc_overflow, trainer=sc_trainer)


def _scenarios(rank, world, names):
    return [(n, _FUNCS[n](rank, world)) for n in names]


def _run(world, names):
    res = run_ranks(world, _scenarios, names, timeout=600)
    for rank, got in sorted(res.items()):
        assert [n for n, _ in got] == list(names), "rank %d ran %s" % (rank, got)       # every scenario, on every rank
    return res


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_bags_linear_forward_rides_on_the_bag_lookup(world):
    _run(world, ("forward",))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_bags_linear_training_one_node_owner_side_ftrl(world):
    _run(world, ("train3", "overflow"))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_trainer_step_bags_with_linear_term(world):
    _run(world, ("trainer",))


def test_every_scenario_is_wired():
    assert set(_FUNCS) == set(SCENARIOS)
