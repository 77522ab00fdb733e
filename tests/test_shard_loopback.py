"""tests/shard_loopback.py checked on the CPU: P ranks in one process with the NumPy stand-ins on every rank, at every owner count the GPU
test (tests/test_gpu_shard_loopback.py) uses, against the full-table references of the gloo tests -- plain indexing and
oracle.fm_second_order for one-hot, bags_ref / fm_ref for bags, the float64 Adagrad / FTRL restatements for the training steps.  What
this proves is the driver: the emulated exchanges and the order of the backend calls are right before a kernel is put behind them."""
import numpy as np
import pytest
import torch

from tests.shard_loopback import GUARD32, Guards, Loopback, exchange_equal, standin_factory
from tests.shard_standin_bags_linear import lin_entries, lin_forward64, lin_ftrl64
from tests.test_shard_bags_gloo import CASES, bags_ref, draw_bags, fm_ref, to_csr
from tests.test_shard_bags_train_gloo import _close, ref_step
from tests.test_shard_linear_gloo import Reference

OWNERS = [1, 2, 3, 8, 33, 64]
LR, ACC0 = 0.3, 0.1                    # (tests.test_shard_linear_gloo.Reference's constants)
FTRL = (0.2, 0.001, 0.01)
ONEHOT_VOCAB = [300, 2, 641, 37]       # a 2-row table: most ranks hold an empty shard of it at P >= 3
ONEHOT_PARTS = {3: [2, 2, 3, 1], 8: [3, 1, 8, 2]}      # slice counts < P: first = [0, 2, 1, 1] / [0, 3, 4, 4], owners wrap around past P - 1
BAG_VOCAB, BAG_MAXLEN = [300, 2, 641], [12, 3, 1]
BAG_PARTS = {3: [2, 2, 3], 8: [3, 1, 8]}               # first = [0, 2, 1] / [0, 3, 4]
CAP_E, CAP_B = 256, 64


def batch_sizes(P):
    """Uneven local batches, 0..10 samples; rank 2 (and every 11th after it) has none."""
    return [(5 + 3 * r) % 11 for r in range(P)]


def draw_tables(vocab, K, seed=7):
    rng = np.random.default_rng(seed)
    full = [(rng.standard_normal((v, K)) * 0.5).astype(np.float32) for v in vocab]
    lin = [(0.3 * rng.standard_normal(v)).astype(np.float32) for v in vocab]
    return full, lin


def draw_ids(rng, vocab, B, hot=True):
    """[B, F] ids with pruned (< 0) and out-of-vocabulary ids mixed in; hot: row 3 of slot 0 twice in every batch of >= 2 samples."""
    ids = np.stack([rng.integers(-2, v + 2, size=B) for v in vocab], axis=1).astype(np.int64).reshape(B, len(vocab))
    if hot and B >= 2:
        ids[0, 0] = ids[1, 0] = 3
    return ids


def clean(ids, vocab):
    return np.stack([np.where((ids[:, f] >= 0) & (ids[:, f] < v), ids[:, f], -1) for f, v in enumerate(vocab)], axis=1).reshape(ids.shape)


def onehot_rows(full, ids):
    """[B, F*K]: plain indexing, zero rows for pruned / out-of-vocabulary ids."""
    idc = clean(ids, [t.shape[0] for t in full])
    return np.concatenate([np.where((idc[:, f] >= 0)[:, None], t[np.maximum(idc[:, f], 0)], np.float32(0)) for f, t in enumerate(full)],
                          axis=1).astype(np.float32)


def linear_sum32(lin, ids, bias):
    """The first-order term in fp32, slot order, + bias: ops.linear_logit's sum."""
    idc = clean(ids, [w.shape[0] for w in lin])
    acc = np.zeros(ids.shape[0], np.float32)
    for f, w in enumerate(lin):
        acc = acc + np.where(idc[:, f] >= 0, w[np.maximum(idc[:, f], 0)], np.float32(0)).astype(np.float32)
    return (acc + np.float32(bias)).astype(np.float32)


def _loop(full, lin, P, partitions=None):
    return Loopback([torch.from_numpy(t) for t in full], P, standin_factory, partitions=partitions,
                    lin_full=[torch.from_numpy(w) for w in lin], acc0=ACC0)


def _layouts(P, table):
    """The default layout, and at P = 3 and P = 8 a custom one in which some slice's owner first + j reaches P and wraps to first + j - P."""
    from dir_amd.shard import place_slices
    if P in table:
        assert any(f0 + p > P for p, f0 in zip(table[P], place_slices(table[P], P)))
    return [None] + ([table[P]] if P in table else [])


@pytest.mark.parametrize("P", OWNERS)
def test_onehot_lookup_fixed_and_exact(P):
    from oracle import oracle as O
    vocab, K = ONEHOT_VOCAB, 4
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    bias = torch.tensor([0.25])
    rng = np.random.default_rng(100 + P)
    for partitions in _layouts(P, ONEHOT_PARTS):
        lb = _loop(full, lin, P, partitions)
        ids = [draw_ids(rng, vocab, B) for B in batch_sizes(P)]
        tid = [torch.from_numpy(i) for i in ids]
        runs = [lb.onehot_lookup(tid, 48, dedup=d, want_fm=True, want_lin=True, bias=bias) for d in (False, True)]
        runs.append(lb.exact_lookup(tid, want_fm=True, want_lin=True, bias=bias))
        for R in runs:
            for r, s in enumerate(R):
                ref = onehot_rows(full, ids[r])
                assert s.out.shape == (s.B, F * K) and np.array_equal(s.out.numpy(), ref), (P, partitions, r)
                assert np.array_equal(s.fm.numpy()[:, 0], O.fm_second_order(ref, F, K))
                assert np.array_equal(s.lin.numpy()[:, 0], linear_sum32(lin, ids[r], 0.25))
        demand = max(int(s.counts.max()) for s in runs[0])
        for s in runs[0]:
            assert s.stat.tolist() == [0, demand] and int(s.flags) == 0


@pytest.mark.parametrize("P", OWNERS)
def test_onehot_training_step(P):
    vocab, K = ONEHOT_VOCAB, 4
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rng = np.random.default_rng(200 + P)
    for partitions in _layouts(P, ONEHOT_PARTS):
        lb = _loop(full, lin, P, partitions).enable_training(LR, ACC0)
        Bs = batch_sizes(P)
        ids = [draw_ids(rng, vocab, B) for B in Bs]
        G = [rng.standard_normal((B, F * K)).astype(np.float32) for B in Bs]
        g = [rng.standard_normal((B, 1)).astype(np.float32) for B in Bs]
        lb.onehot_train([torch.from_numpy(i) for i in ids], [torch.from_numpy(x) for x in G], 48, [torch.from_numpy(x) for x in g], FTRL)
        ref = Reference(full, lin)
        ref.step(np.concatenate(ids), np.concatenate(G), np.concatenate(g), dict(lr=FTRL[0], l1=FTRL[1], l2=FTRL[2]))
        got, (w, n, z) = lb.assembled(), lb.assembled_linear()
        for f in range(F):
            assert _close(got[f], ref.T[f]) <= 1e-5
            for a, b in ((w, ref.w), (n, ref.n), (z, ref.z)):
                assert _close(a[f], b[f][:, 0]) <= 1e-5, (P, partitions, f)
        untouched = np.ones(vocab[0], bool)
        untouched[np.concatenate(ids)[:, 0].clip(0, vocab[0] - 1)] = False
        assert np.array_equal(got[0][untouched].astype(np.float32), full[0][untouched])


def bag_inputs(P, case, rng, vocab=BAG_VOCAB, max_len=BAG_MAXLEN, sizes=None):
    """-> (bags per rank, csr per rank as torch tensors, batch sizes)."""
    wmode, comb, mn, fmaj, prune = case
    Bs = batch_sizes(P) if sizes is None else sizes
    bags = [draw_bags(rng, B, vocab, max_len, wmode) for B in Bs]
    csr = []
    for b in bags:
        v, o, w = to_csr(b, len(vocab), fmaj)
        csr.append((torch.from_numpy(v), torch.from_numpy(o), None if w is None else torch.from_numpy(w)))
    return bags, csr, Bs


@pytest.mark.parametrize("P", OWNERS)
def test_bags_lookup(P):
    vocab, K = BAG_VOCAB, 4
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rng = np.random.default_rng(300 + P)
    worst, high, top = 0.0, 0, 0
    for partitions in _layouts(P, BAG_PARTS):
        lb = _loop(full, lin, P, partitions)
        for c, case in enumerate(CASES):
            wmode, comb, mn, fmaj, prune = case
            bags, csr, Bs = bag_inputs(P, case, rng)
            lin_comb = ("sum", "mean", "sqrtn")[c % 3]
            R = lb.bags_lookup(csr, Bs, comb, mn, fmaj, 1 if prune else 0, CAP_E, CAP_B, want_fm=True, lin=(lin_comb, torch.tensor([0.5])))
            for r, s in enumerate(R):
                assert s.stat[0] == 0, "a slab overflowed: the capacities of this test are meant to be ample"
                ref, scale = bags_ref(full, bags[r], comb, mn, prune)
                if s.B:
                    worst = max(worst, float((np.abs(s.out.numpy() - ref) / np.maximum(scale, 1e-30)).max()))
                    assert (np.abs(s.out.numpy() - ref) <= 1e-6 + 1e-5 * (scale + 1)).all(), (P, c, r)
                    fr = fm_ref(ref, F, K)
                    assert np.abs(s.fm.numpy()[:, 0] - fr).max() <= 1e-4 * (1 + np.abs(fr).max())
                    lr_ = lin_forward64(lin, lin_entries(bags[r], vocab, lin_comb, prune), s.B) + 0.5
                    assert np.abs(s.lin.numpy()[:, 0] - lr_).max() <= 1e-5 * (1 + np.abs(lr_).max())
                m = s.mask.numpy()[:s.B * F].astype(np.uint64)
                high += int((m >> np.uint64(63)).astype(bool).sum())
                top += int(((m >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(bool).sum())
    assert worst <= (BAG_MAXLEN[0] + min(P, BAG_MAXLEN[0]) + 8) * 2.0 ** -24, worst      # one rounding per accumulated term + clip + division
    if P == 64:
        assert high > 0 and top > 0              # bags owned by rank 63 (the int64 mask's sign bit) and by ranks 32..62 were drawn


@pytest.mark.parametrize("P", OWNERS)
def test_bags_training_step(P):
    vocab, K = BAG_VOCAB, 4
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rng = np.random.default_rng(400 + P)
    for partitions in _layouts(P, BAG_PARTS):
        for c in (1, 2):                             # weights + max_norm + field-major; per-slot combiners + the prune flag
            case = CASES[c]
            wmode, comb, mn, fmaj, prune = case
            lb = _loop(full, lin, P, partitions).enable_training(LR, ACC0)
            bags, csr, Bs = bag_inputs(P, case, rng)
            for bl in bags:                          # a hot row: twice in a bag, on every rank
                for row in bl:
                    if len(row[0][0]) >= 2:
                        row[0][0][:2] = 5
            csr = [(torch.from_numpy(v), torch.from_numpy(o), None if w is None else torch.from_numpy(w))
                   for v, o, w in (to_csr(b, F, fmaj) for b in bags)]
            G = [rng.standard_normal((B, F * K)).astype(np.float32) for B in Bs]
            g = [rng.standard_normal((B, 1)).astype(np.float32) for B in Bs]
            lin_comb = ("mean", "sqrtn", "sum")[c % 3]
            lb.bags_train(csr, Bs, [torch.from_numpy(x) for x in G], comb, mn, fmaj, 1 if prune else 0, CAP_E, CAP_B,
                          g_lin=[torch.from_numpy(x) for x in g], lin_comb=lin_comb, ftrl=FTRL)
            allb = [b for bl in bags for b in bl]
            T, acc = [t.astype(np.float64) for t in full], [np.full(t.shape, ACC0) for t in full]
            ref_step(T, acc, allb, np.concatenate(G), comb, mn, prune, LR)
            w, n, z = ([x.astype(np.float64).reshape(-1, 1) for x in lin], [np.full((v, 1), ACC0) for v in vocab], [np.zeros((v, 1)) for v in vocab])
            lin_ftrl64(w, n, z, lin_entries(allb, vocab, lin_comb, prune), np.concatenate(g), *FTRL)
            got, (gw, gn, gz) = lb.assembled(), lb.assembled_linear()
            for f in range(F):
                assert _close(got[f], T[f]) <= 1e-5, (P, partitions, c, f)
                for a, b in ((gw, w), (gn, n), (gz, z)):
                    assert _close(a[f], b[f][:, 0]) <= 1e-5, (P, partitions, c, f)


def test_exchange_is_the_transpose_of_the_slabs():
    P, w = 5, 3
    send = [torch.arange(P * w) + 100 * s for s in range(P)]
    recv = exchange_equal(send, P)
    for r in range(P):
        for s in range(P):
            assert recv[r].view(P, w)[s].tolist() == [100 * s + r * w + j for j in range(w)]


def test_guard_tail_reports_a_write_past_the_end():
    G = Guards("cpu")
    body = G.alloc("rows", 0, (4, 2), torch.float32, 8)
    G.check("nothing")
    assert int(body.view(torch.int32)[0, 0]) != GUARD32
    body.view(-1).as_strided((9,), (1,))[8] = 1.0            # one element past the body, inside the same allocation
    with pytest.raises(AssertionError, match="rows"):
        G.check("a write past the end")
