"""CPU tests of row groups and units > 1 on the row-sharded tables (dir_amd.shard: ShardedTables(groups=G), attach_linear([rows, U]),
ShardedESMMTrainer) over the gloo backend, world sizes 1, 2 and 3.

What runs here is the exchange logic that runs on a GPU box under RCCL: one id exchange and one owner gather for G groups, U floats per
slab slot behind the rows, the gradient rows interleaved on the way back, the overflow fallback carrying groups and units, and the
trainer's global-mean loss normalisation.  The HIP steps cannot run without a GPU: tests/shard_standin_groups.NumpyGroupsBackend takes
their place (tests/test_gpu_shard_groups.py checks the kernels against the same stand-ins).

Error measure and bar: max |got - ref| / (1 + |ref|) <= 1e-5 against float64, tests/test_shard_linear_gloo.py's for the same kind of
comparison (its trainer scenario included)."""
import copy

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.shard_standin import run_ranks
from tests.shard_standin_groups import NumpyGroupsBackend

LR, ACC0 = 0.3, 0.1
TOL = 1e-5
VOCAB, K, G, U = [40, 7, 2, 23], 4, 2, 2


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else t


def _err(got, ref):
    got, ref = np.asarray(_np(got), np.float64), np.asarray(_np(ref), np.float64)
    return float(np.max(np.abs(got - ref) / (1 + np.abs(ref)))) if got.size else 0.0


def _clean(ids, vocab):
    return np.stack([np.where((ids[:, f] >= 0) & (ids[:, f] < vocab[f]), ids[:, f], -1) for f in range(len(vocab))], axis=1).reshape(-1, len(vocab))


class Reference:
    """float64, over the FULL tables and the GLOBAL batch: G independent Adagrad-trained table sets, U independent FTRL-trained weight sets."""

    def __init__(self, full_g, full_w):
        self.T = [[t.astype(np.float64) for t in full] for full in full_g]
        self.acc = [[np.full(t.shape, ACC0) for t in full] for full in full_g]
        self.w = [[w[:, u:u + 1].astype(np.float64) for w in full_w] for u in range(full_w[0].shape[1])]
        self.n = [[np.full(w.shape, ACC0) for w in ws] for ws in self.w]
        self.z = [[np.zeros(w.shape) for w in ws] for ws in self.w]

    def step(self, ids, Gs, g, ftrl):
        """ids [Bg, F]; Gs[g] [Bg, F*K] = d loss / d group g's emb; g [Bg, U] = d loss / d lin."""
        from oracle import np_ref as R
        ids = _clean(ids, [t.shape[0] for t in self.T[0]])
        for gi in range(len(self.T)):
            R.sparse_adagrad_step(self.T[gi], self.acc[gi], ids, np.asarray(Gs[gi], np.float64), LR)
        for u in range(len(self.w)):
            R.sparse_ftrl_step(self.w[u], self.n[u], self.z[u], ids, np.asarray(g[:, u:u + 1], np.float64), ftrl["lr"], ftrl["l1"], ftrl["l2"])

    def forward(self, ids):
        """-> ([G] emb [B, F*K], lin [B, U]) in float64."""
        F = len(self.T[0])
        idc = _clean(ids, [t.shape[0] for t in self.T[0]])
        embs = [np.concatenate([np.where((idc[:, f] >= 0)[:, None], T[f][np.maximum(idc[:, f], 0)], 0.0) for f in range(F)], axis=1) for T in self.T]
        lin = np.stack([sum(np.where(idc[:, f] >= 0, w[f][np.maximum(idc[:, f], 0), 0], 0.0) for f in range(F)) for w in self.w], axis=1)
        return embs, lin


def _draw(vocab, K, seed, G=G, U=U):
    rng = np.random.default_rng(seed)
    full_g = [[rng.standard_normal((v, K)).astype(np.float32) for v in vocab] for _ in range(G)]
    full_w = [(0.3 * rng.standard_normal((v, U))).astype(np.float32) for v in vocab]
    return full_g, full_w


def _batch(vocab, B, seed, rank, step=0, hot=False):
    """A rank's batch: ids below 0 and past the vocabulary included; hot: id 3 of slot 0 twice in every rank's batch."""
    rng = np.random.default_rng(seed + 1000 * step + 17 * rank + 5)
    ids = np.stack([rng.integers(-2, v + 2, size=B) for v in vocab], axis=1).astype(np.int64).reshape(B, len(vocab))
    if hot and B >= 2:
        ids[0, 0] = ids[1, 0] = 3
    return ids


def _tables(rank, world, vocab, K, seed, G=G, U=U, **kw):
    from dir_amd.shard import ShardedTables, partition_layout
    full_g, full_w = _draw(vocab, K, seed, G, U)
    parts, first, slices = partition_layout(vocab, K, world, rank, kw.get("partitions"))
    local = [torch.from_numpy(np.concatenate([full[f][s:e] for full in full_g], axis=1).copy()) for f, (s, e) in enumerate(slices)]
    be = NumpyGroupsBackend(local, vocab, parts, first, world, K, G)
    st = ShardedTables(local, vocab, backend=be, groups=G, **kw)
    if U:
        st.attach_linear([torch.from_numpy(full_w[f][s:e].copy()) for f, (s, e) in enumerate(slices)], initial_accumulator_value=ACC0)
    return st, be, full_g, full_w, slices


def _compare_shards(st, ref, slices, what):
    """Every group's tables and accumulators and every unit's w, n, z against the reference's slices."""
    worst = {}

    def note(name, got, want):
        worst[name] = max(worst.get(name, 0.0), _err(got, want))
    for g in range(st.G):
        tabs, accs = st.group_tables(g), st.group_accums(g)
        for f, (s, e) in enumerate(slices):
            assert tuple(tabs[f].shape) == (e - s, st.K) and tuple(accs[f].shape) == (e - s, st.K)
            note("emb%d" % g, tabs[f], ref.T[g][f][s:e])
            note("acc%d" % g, accs[f], ref.acc[g][f][s:e])
    if st.lin_rows is not None:
        w, n, z = st.linear_state()
        for f, (s, e) in enumerate(slices):
            assert tuple(w[f].shape) == (e - s, st.U)
            for u in range(st.U):
                note("w%d" % u, w[f][:, u], ref.w[u][f][s:e, 0])
                note("n%d" % u, n[f][:, u], ref.n[u][f][s:e, 0])
                note("z%d" % u, z[f][:, u], ref.z[u][f][s:e, 0])
    assert all(v <= TOL for v in worst.values()), "%s: %s" % (what, worst)


def _sizes(world, base=6):
    return [base + 3 * r if r != world - 1 or world == 1 else 2 for r in range(world)]


def _train_steps(rank, world, seed, sizes, steps, ftrl, kw, between=None, vocab=VOCAB):
    st, be, full_g, full_w, slices = _tables(rank, world, vocab, K, seed, **kw)
    st.enable_training(LR, ACC0).enable_linear_training(**ftrl)
    ref = Reference(full_g, full_w)
    F = len(vocab)
    for step in range(steps):
        ids_all = [_batch(vocab, sizes[r], seed, r, step, hot=True) for r in range(world)]
        rngs = [np.random.default_rng(seed + 31 * step + r) for r in range(world)]
        G_all = [[rg.standard_normal((sizes[r], F * K)).astype(np.float32) for _ in range(G)] for r, rg in enumerate(rngs)]
        g_all = [rg.standard_normal((sizes[r], U)).astype(np.float32) for r, rg in enumerate(rngs)]
        before = st._updates
        embs, lin = st.lookup_train(torch.from_numpy(ids_all[rank]), with_linear=True)
        assert isinstance(embs, tuple) and len(embs) == G and tuple(lin.shape) == (sizes[rank], U)
        want_embs, want_lin = ref.forward(ids_all[rank])
        assert _err(lin.detach().numpy(), want_lin) <= TOL, "lin, step %d" % step
        for g in range(G):
            assert _err(embs[g].detach().numpy(), want_embs[g]) <= TOL, "group %d forward, step %d" % (g, step)
        loss = sum((embs[g] * torch.from_numpy(G_all[rank][g])).sum() for g in range(G)) + (lin * torch.from_numpy(g_all[rank])).sum()
        loss.backward()
        assert st._updates == before + 1, "one owner step per backward"
        ref.step(np.concatenate(ids_all), [np.concatenate([G_all[r][g] for r in range(world)]) for g in range(G)], np.concatenate(g_all), ftrl)
        _compare_shards(st, ref, slices, "after step %d" % step)
        if between is not None:
            between(st, step)
    return st, be, ref, slices


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------
def sc_forward(rank, world):
    """Grouped forward: group g's output is the rows of group g's FULL table bit for bit (a pure copy) and lin[:, u] the float64 sum within
    the bar; ids < 0 and >= vocab_f; a table with fewer rows than ranks; uneven local batches including an empty one; fixed / exact paths,
    de-duplication, the check modes, one to three micro-batches."""
    F = len(VOCAB)
    bias = torch.tensor([0.37, -1.25], dtype=torch.float32)
    ran = 0
    for kw in ({}, {"dedup": True}, {"mode": "exact"}, {"check": "lazy"}, {"check": "never", "chunks": 1}, {"chunks": 3, "dedup": True},
               {"force_collective": True}):
        st, be, full_g, full_w, _ = _tables(rank, world, VOCAB, K, 11, **kw)
        ref = Reference(full_g, full_w)
        for it, sizes in enumerate(([4 + 3 * r for r in range(world)], [0 if r == world - 1 else 6 + r for r in range(world)],
                                    [5 if r == world - 1 else 0 for r in range(world)])):
            ids = _batch(VOCAB, sizes[rank], 11, rank, it)
            b = bias if it != 1 else None
            embs, lin = st.lookup(torch.from_numpy(ids), want_lin=True, lin_bias=b)
            assert isinstance(embs, tuple) and len(embs) == G and tuple(lin.shape) == (sizes[rank], U)
            idc = _clean(ids, VOCAB)
            for g in range(G):
                assert tuple(embs[g].shape) == (sizes[rank], F * K)
                for f in range(F):
                    want = np.where((idc[:, f] >= 0)[:, None], full_g[g][f][np.maximum(idc[:, f], 0)], np.float32(0))
                    assert np.array_equal(embs[g].numpy()[:, f * K:(f + 1) * K], want), (kw, it, g, f)
            want_lin = ref.forward(ids)[1] + (b.numpy().astype(np.float64) if b is not None else 0.0)
            assert _err(lin.numpy(), want_lin) <= TOL, (kw, it)
            plain = st.lookup(torch.from_numpy(ids))                  # without want_lin: the tuple of G alone
            assert isinstance(plain, tuple) and all(torch.equal(p, e) for p, e in zip(plain, embs))
            ran += 1
        st.check_overflow()
    return "%d lookups" % ran


def sc_train3(rank, world):
    """Three training steps, Adagrad at width G*K and FTRL over U units with l1 = l2 = 0, against the float64 reference per group and unit."""
    st, be, ref, _ = _train_steps(rank, world, 23, _sizes(world), 3, dict(lr=0.2, l1=0.0, l2=0.0), {})
    assert be.ftrl_calls == 3 and be.ftrl_widths == [U] * 3            # one FTRL step per backward, U gradient columns per payload word
    return "3 steps"


def sc_train_l1(rank, world):
    """l1, l2 > 0: the float64 reference clips some touched weight of each unit to exactly 0.0, and the shards have the same zero pattern."""
    ftrl = dict(lr=0.2, l1=0.6, l2=0.05)
    st, be, ref, slices = _train_steps(rank, world, 29, _sizes(world), 3, ftrl, {})
    w = st.linear_weights()
    for u in range(U):
        touched = [np.abs(ref.z[u][f][:, 0]) > 0 for f in range(len(VOCAB))]
        zeros = sum(int(((ref.w[u][f][:, 0] == 0.0) & touched[f]).sum()) for f in range(len(VOCAB)))
        nonzeros = sum(int(((ref.w[u][f][:, 0] != 0.0) & touched[f]).sum()) for f in range(len(VOCAB)))
        assert zeros >= 1 and nonzeros >= 1, "unit %d: the reference must clip some touched weights and keep others (%d / %d)" % (u, zeros, nonzeros)
        for f, (s, e) in enumerate(slices):
            assert np.array_equal(w[f][:, u].numpy() == 0.0, ref.w[u][f][s:e, 0] == 0.0), "unit %d slot %d: zero pattern" % (u, f)
    return "zeros in every unit"


def sc_partitions(rank, world):
    """partitions="reference" (one slice per small table, dealt round-robin) and an explicit slice list."""
    explicit = [min(world, p) for p in (2, 1, 2, 3)]
    for part in ("reference", explicit):
        _train_steps(rank, world, 31, _sizes(world), 3, dict(lr=0.2, l1=0.01, l2=0.02), {"partitions": part})
    return "reference + %s" % explicit


def sc_overflow(rank, world):
    """A slack so small that the first training lookup overflows: the step is repeated on the exact path, groups and units included."""
    seen = {}

    def between(st, step):
        seen[step] = st.stats["fallbacks"]
    _train_steps(rank, world, 37, [40 + r for r in range(world)], 3, dict(lr=0.2, l1=0.0, l2=0.0),
                 {"slack": 0.1, "mode": "fixed", "chunks": 1, "force_collective": True}, between=between)
    assert seen[0] >= 1, "the first training lookup must have overflowed (fallbacks = %s)" % seen
    return "fallbacks %s" % seen


def sc_chunks2(rank, world):
    """chunks = 2 (two micro-batches per lookup, one owner step over both) with inference lookups between the steps."""
    def between(st, step):
        ids = torch.from_numpy(_batch(VOCAB, 5 + rank, 41, rank, 50 + step))
        embs, lin = st.lookup(ids, want_lin=True)
        assert len(embs) == G and tuple(lin.shape) == (5 + rank, U)
    _train_steps(rank, world, 41, _sizes(world), 3, dict(lr=0.2, l1=0.01, l2=0.0), {"chunks": 2, "force_collective": True}, between=between)
    return "3 steps"


def sc_errors(rank, world):
    """What grouped tables do not cover raises NotImplementedError, K % 4 != 0 raises ValueError -- before any exchange (no rank hangs)."""
    from dir_amd.shard import ShardedTables
    st, be, _, _, _ = _tables(rank, world, VOCAB, K, 7)
    ids = torch.from_numpy(_batch(VOCAB, 3, 7, rank))
    empty, offs = torch.zeros(0, dtype=torch.int64), torch.zeros(3 * len(VOCAB) + 1, dtype=torch.int64)
    for call in (lambda: st.lookup(ids, want_fm=True), lambda: st.lookup_consume(ids, lambda *a: None), lambda: st.lookup_rows(ids),
                 lambda: st.lookup_rows_async(ids), lambda: st.lookup_bags(empty, offs), lambda: st.lookup_bags_train(empty, offs)):
        with pytest.raises(NotImplementedError, match="grouped"):
            call()
    with pytest.raises(ValueError, match="multiple of 4"):
        _tables(rank, world, VOCAB, 3, 7)
    with pytest.raises(ValueError, match="units"):
        st.attach_linear([torch.zeros(t.shape[0], 9) for t in st.local_tables])
    plain = ShardedTables([t[:, :K].contiguous() for t in st.local_tables], VOCAB, backend=be)          # G = 1: one tensor, as before
    assert plain.G == 1 and plain.KW == K
    return "raised"


def _tiny_model(linear, vocab=VOCAB, K=K, hidden=(6,)):
    from dir_amd import feature_column as fc
    from dir_amd.esmm import ESMM, ESMM_W_D
    torch.manual_seed(5)
    cats = [fc.categorical_column_with_identity("c%d" % i, v) for i, v in enumerate(vocab)]
    dnn = [fc.embedding_column(c, K) for c in cats]
    if linear:
        m = ESMM_W_D(linear_feature_columns=cats, dnn_feature_columns=dnn, dnn_hidden_units=list(hidden))
        with torch.no_grad():
            for sub in (m.ctr_model, m.cvr_model):                    # TF's zeros initialisation would leave the term untested at step 0
                for w in sub.linear.weights:
                    w.copy_(0.3 * torch.randn(w.shape))
    else:
        m = ESMM(columns=dnn, dnn_hidden_units=list(hidden))
    return m


def _trainer(rank, world, linear, dev=None, VOCAB=VOCAB, K=K, hidden=(6,), sizes=None):
    """ShardedESMMTrainer: two steps + predict against a float64 single-process model of the GLOBAL batch (the ranks hold different batch
    sizes, the two weight columns differ: the global-mean normalisation is what makes the two agree); replicated state identical on
    every rank.  dev = None: on the CPU with the NumPy stand-in backend; a CUDA device: the product backend (tests/test_gpu_shard_groups.py)."""
    from dir_amd.shard import ShardedESMMTrainer, ShardedTables
    from oracle import np_ref as R
    ftrl = dict(lr=0.15, l1=0.01, l2=0.02)
    sizes = sizes or _sizes(world, 5)
    F = len(VOCAB)
    model = _tiny_model(linear, VOCAB, K, hidden)
    m64 = copy.deepcopy(model).double()
    on = (lambda a: torch.from_numpy(a)) if dev is None else (lambda a: torch.from_numpy(a).to(dev))
    if dev is not None:
        model = model.to(dev)
    subs = [(s.dnn, s.linear) if linear else (s, None) for s in (model.ctr_model, model.cvr_model)]
    subs64 = [(s.dnn, s.linear) if linear else (s, None) for s in (m64.ctr_model, m64.cvr_model)]
    full_g = [[_np(p.data).copy() for p in t.input_layer.embedding_weights] for t, _ in subs]
    full_w = [np.stack([_np(subs[0][1].weights[f].data), _np(subs[1][1].weights[f].data)], axis=1) for f in range(F)] if linear else None
    # the stand-in backend has to be handed in: tables_from_model's layout, built by hand with it, then compared with tables_from_model's own
    from dir_amd.shard import partition_layout
    parts, first, slices = partition_layout(VOCAB, K, world, rank, None)
    local = [torch.from_numpy(np.concatenate([fg[f][s:e] for fg in full_g], axis=1).copy()) for f, (s, e) in enumerate(slices)]
    if dev is None:
        be = NumpyGroupsBackend(local, VOCAB, parts, first, world, K, 2)
        st = ShardedESMMTrainer.tables_from_model(model, backend=be, linear_initial_accumulator_value=ACC0)
        be.local = st.local_tables                                       # (the stand-in gathers from and updates the tables' own storage)
    else:
        st = ShardedESMMTrainer.tables_from_model(model, linear_initial_accumulator_value=ACC0)
    assert st.G == 2 and st.K == K and (st.U == 2) == linear
    for f in range(F):
        assert torch.equal(st.local_tables[f].cpu(), local[f])
    dense = [p for n, p in model.named_parameters() if "embedding_weights" not in n and ".linear." not in n]
    if linear:
        with pytest.raises(ValueError, match="dense_optimizer"):
            ShardedESMMTrainer(model, st, LR, torch.optim.SGD(dense + [model.ctr_model.linear.bias], lr=0.05), linear=ftrl)
        with pytest.raises(ValueError, match="linear="):
            ShardedESMMTrainer(model, st, LR, torch.optim.SGD(dense, lr=0.05))
    tr = ShardedESMMTrainer(model, st, LR, torch.optim.SGD(dense, lr=0.05), linear=ftrl if linear else None, initial_accumulator_value=ACC0)
    ref = Reference(full_g, full_w if linear else [np.zeros((v, 1), np.float32) for v in VOCAB])
    bn, bz = [np.full(1, 0.1), np.full(1, 0.1)], [np.zeros(1), np.zeros(1)]
    dense64 = [p for n, p in m64.named_parameters() if "embedding_weights" not in n and ".linear." not in n]
    for step in range(2):
        rngs = [np.random.default_rng(43 + 7 * step + r) for r in range(world)]
        ids_all = [_batch(VOCAB, sizes[r], 43, r, step, hot=True) for r in range(world)]
        y_all = [rg.integers(0, 2, size=(sizes[r], 2)).astype(np.float32) for r, rg in enumerate(rngs)]
        wc_all = [rg.uniform(0.5, 2.0, size=(sizes[r], 1)).astype(np.float32) for r, rg in enumerate(rngs)]       # two DIFFERENT weight columns
        wv_all = [rg.uniform(0.1, 3.0, size=(sizes[r], 1)).astype(np.float32) for r, rg in enumerate(rngs)]
        got = tr.step(on(ids_all[rank]), on(y_all[rank]), on(wc_all[rank]), on(wv_all[rank]))
        # the float64 model on the concatenated batch
        idg = _clean(np.concatenate(ids_all), VOCAB)
        yg, wc, wv = (torch.from_numpy(np.concatenate(a)).double() for a in (y_all, wc_all, wv_all))
        it, ok = torch.from_numpy(np.maximum(idg, 0)), torch.from_numpy(idg >= 0)
        T = [[torch.from_numpy(t).requires_grad_(True) for t in ref.T[g]] for g in range(2)]
        embs = [torch.cat([T[g][f][it[:, f]] * ok[:, f:f + 1] for f in range(F)], dim=1) for g in range(2)]
        m64.zero_grad()
        logits = [subs64[g][0].tower(embs[g], True) for g in range(2)]
        if linear:
            W = [[torch.from_numpy(w).requires_grad_(True) for w in ref.w[u]] for u in range(2)]
            lins = [sum(W[u][f][it[:, f]] * ok[:, f:f + 1] for f in range(F)) for u in range(2)]
            for l in lins:
                l.retain_grad()
            logits = [logits[u] + (lins[u] + subs64[u][1].bias) for u in range(2)]
        p = (torch.sigmoid(logits[0]) * torch.sigmoid(logits[1])).clamp(1e-7, 1 - 1e-7)
        ctcvr = torch.log(p / (1 - p))
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        per_ctr = wc * bce(logits[0], yg[:, 0:1], reduction="none") / wc.sum()       # _get_loss: MEAN per task with its weight column
        per_cv = wv * bce(ctcvr, yg[:, 1:2], reduction="none") / wv.sum()
        (per_ctr.sum() + per_cv.sum()).backward()
        for g in range(2):                                    # Adagrad on the full tables (rows without a gradient do not move)
            for f in range(F):
                gr = T[g][f].grad.numpy()
                ref.acc[g][f] += gr * gr
                ref.T[g][f] -= LR * gr / np.sqrt(ref.acc[g][f])
        if linear:
            for u in range(2):
                R.sparse_ftrl_step(ref.w[u], ref.n[u], ref.z[u], idg, lins[u].grad.numpy(), ftrl["lr"], ftrl["l1"], ftrl["l2"])
        with torch.no_grad():
            for q in dense64:
                q -= 0.05 * q.grad
            if linear:
                for u in range(2):
                    b = subs64[u][1].bias
                    gb = b.grad.numpy().astype(np.float64)
                    n_new = bn[u] + gb * gb
                    z_new = bz[u] + gb - (np.sqrt(n_new) - np.sqrt(bn[u])) / ftrl["lr"] * b.numpy()
                    b.copy_(torch.from_numpy(np.where(np.abs(z_new) > ftrl["l1"], (np.sign(z_new) * ftrl["l1"] - z_new)
                                                      / (np.sqrt(n_new) / ftrl["lr"] + 2 * ftrl["l2"]), 0.0)))
                    bn[u], bz[u] = n_new, z_new
        off = sum(sizes[:rank])
        assert _err(float(got[0]), float(per_ctr[off:off + sizes[rank]].sum().detach())) <= TOL, "ctr loss, step %d" % step
        assert _err(float(got[1]), float(per_cv[off:off + sizes[rank]].sum().detach())) <= TOL, "ctcvr loss, step %d" % step
        for p32, q in zip(dense, dense64):
            assert _err(p32, q) <= TOL, "dense parameter, step %d" % step
        if linear:
            mine = torch.cat([b.data for b in tr.biases] + tr.bias_accum + tr.bias_linear)
            mine = mine if dist.get_backend() == "nccl" else mine.cpu()
            every = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            assert all(torch.equal(e, every[0]) for e in every), "the biases and their FTRL state must be identical on every rank"
            want = np.concatenate([subs64[0][1].bias.detach().numpy(), subs64[1][1].bias.detach().numpy(), bn[0], bn[1], bz[0], bz[1]])
            assert _err(mine, want) <= TOL, "biases / n / z, step %d" % step
        if not linear:
            ref.w, ref.n, ref.z = [], [], []
        _compare_shards(st, ref, slices, "trainer step %d" % step)
    # predict on a fresh batch against the float64 model's forward
    ids = _batch(VOCAB, 4 + rank, 43, rank, 9)
    out = tr.predict(on(ids))
    assert sorted(out) == ["ctcvr_logits", "ctr_logits", "cvr_logits"]
    idc = _clean(ids, VOCAB)
    it, ok = torch.from_numpy(np.maximum(idc, 0)), torch.from_numpy(idc >= 0)
    with torch.no_grad():
        want = []
        for g in range(2):
            emb = torch.cat([torch.from_numpy(ref.T[g][f])[it[:, f]] * ok[:, f:f + 1] for f in range(F)], dim=1)
            lg = subs64[g][0].tower(emb, False)
            if linear:
                lg = lg + sum(torch.from_numpy(ref.w[g][f])[it[:, f]] * ok[:, f:f + 1] for f in range(F)) + subs64[g][1].bias
            want.append(lg)
        p = (torch.sigmoid(want[0]) * torch.sigmoid(want[1])).clamp(1e-7, 1 - 1e-7)
        want.append(torch.log(p / (1 - p)))
    for name, w in zip(("ctr_logits", "cvr_logits", "ctcvr_logits"), want):
        assert tuple(out[name].shape) == (4 + rank, 1) and _err(out[name], w) <= TOL, name
    return "2 steps + predict"


def sc_trainer(rank, world):
    return _trainer(rank, world, True)


def sc_trainer_nolinear(rank, world):
    return _trainer(rank, world, False)


_FUNCS = dict(forward=sc_forward, train3=sc_train3, train_l1=sc_train_l1, partitions=sc_partitions, overflow=sc_overflow, chunks2=sc_chunks2,
              errors=sc_errors, trainer=sc_trainer, trainer_nolinear=sc_trainer_nolinear)


def _scenarios(rank, world, names):
    return [(n, _FUNCS[n](rank, world)) for n in names]


def _run(world, names):
    assert set(names) <= set(_FUNCS)
    res = run_ranks(world, _scenarios, names, timeout=600)
    for rank, got in sorted(res.items()):
        assert [n for n, _ in got] == list(names), "rank %d ran %s" % (rank, got)
    return res


@pytest.mark.parametrize("world", [1, 2, 3])
def test_grouped_forward_per_group_and_units(world):
    _run(world, ("forward", "errors"))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_grouped_training_owner_side_adagrad_and_ftrl_units(world):
    _run(world, ("train3", "train_l1", "partitions", "overflow", "chunks2"))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_esmm_trainer_matches_the_global_batch_model(world):
    _run(world, ("trainer", "trainer_nolinear"))
