"""DeepFM's first-order term over row-sharded multi-hot bags on the GPU (ShardedTables.lookup_bags(want_lin=), lookup_bags_train(with_linear=),
ShardedDeepFMTrainer.step_bags / predict_bags with linear=) with the PRODUCT HIP backend: dir_shard_bags_linear_pool_f32,
dir_shard_bags_linear_combine_f32, dir_shard_bags_linear_grad_f32, dir_sparse_ftrl_rows_sorted_bags_f32.

  1. world 1 forward, bit for bit ops.linear_logit over the unsharded weights (F in {1, 3, 26}; B in (1, 37, 300, 0); runs that cross
     the pool kernel's 8-entry chunk and one bag of more than 256 entries; no weights and weights; every linear combiner; both layouts;
     with and without a bias); emb and fm untouched; PRUNE_NONPOSITIVE_WEIGHTS against float64;
  2. world 1 training against float64 (oracle.np_ref.sparse_ftrl_step on the per-entry gradients), (l1, l2) x every linear combiner;
  3. skewed bags: one row hit > 600 times (its run crosses sort tiles: the carry / fix path of the FTRL bag mode) and a 300-entry bag;
     one row named by more than 3000 entries of a batch of 4096 bags;
  4. the owner's FTRL on its own sort equals the one on the Adagrad step's sort, bit for bit;
  5. one (emb, lin) node leaves the embedding tables and accumulators bit for bit those of a step without the term;
  6. a captured world-1 lookup_bags(want_fm, want_lin) replays to the eager result, also after the first-order rows moved;
  7. step_bags / predict_bags with linear= on a real DeepFM with a history column, against the float64 three-term model;
  8. two ranks on cuda:0 over host-staged gloo (and over RCCL with one rank per GPU; skipped with a reason on a one-GPU box).
  9. payload words at and past 2^31 (F = 2048 slots, a slot of 2^20 + 16 rows): the 64-bit branch of the decode that the one-hot
     gathers, both pools and both key passes share (csrc/shard_wire.hpp), on all four world-1 calls.
Error measure: the sibling tests' _close, max |got - ref| / (1 + |ref|)."""
import os

import numpy as np
import pytest
import torch

from tests.shard_standin_bags_linear import LIN_COMBINERS, lin_entries, lin_forward64, lin_ftrl64
from tests.test_gpu_shard_bags import _one_owner_bags
from tests.test_gpu_shard_bags_train import _close, _dev, _hot_bags, _skewed_bags, _store
from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr
from tests.test_shard_bags_train_gloo import bags_forward64, ref_step
from tests.test_shard_linear_gloo import Reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, ACC0 = 0.3, 0.1


def _draw(vocab, K, seed, dev):
    rng = np.random.default_rng(seed)
    full = [torch.from_numpy((rng.standard_normal((v, K)) * 0.4).astype(np.float32)).to(dev) for v in vocab]
    full_w = [torch.from_numpy((0.3 * rng.standard_normal(v)).astype(np.float32)).to(dev) for v in vocab]
    return full, full_w


def _tables(full, full_w, train=None):
    from dir_amd.shard import ShardedTables
    st = ShardedTables.from_full([t.clone() for t in full]).attach_linear_from_full(full_w, ACC0)
    if train is not None:
        st.enable_training(LR, ACC0).enable_linear_training(**train)
    return st


def _state_err(st, lref, sl=None):
    w, n, z = st.linear_state()
    F = len(w)
    sl = sl or [slice(None)] * F
    return tuple(max(_close(got[f], want[f][sl[f], 0]) for f in range(F)) for got, want in ((w, lref.w), (n, lref.n), (z, lref.z)))


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 26])
def test_world1_forward_bitwise_equals_linear_logit(built_lib, F):
    """linear_csr_k computes v + wt * w[id] as a multiply and an add (the library is built with -ffp-contract=off, so nothing is
    contracted to an fma) and v + w[id] without weights; the pool kernel does acc + w * lw with records that carry 1.0f without weights:
    the same roundings."""
    from dir_amd import ops
    dev = torch.device("cuda", 0)
    vocab = [500, 1000, 7][:F] if F <= 3 else [200 + 37 * i for i in range(F)]
    max_len = ([60, 1, 3] * 9)[:F]
    K = 16
    full, full_w = _draw(vocab, K, 3 + F, dev)
    st = _tables(full, full_w)
    rng = np.random.default_rng(17 + F)
    bias = torch.tensor([0.37], dtype=torch.float32, device=dev)
    bad = []
    for B in (1, 37, 300, 0):
        for wmode in (None, "pos"):
            bags = draw_bags(rng, B, vocab, max_len, wmode)
            if B:                                                      # one bag of more than 256 entries
                L = 300
                bags[0][0] = (rng.integers(0, vocab[0], size=L).astype(np.int64),
                              None if wmode is None else rng.uniform(0.1, 2.0, size=L).astype(np.float32))
            for fmaj in (False, True):
                v, o, w = _dev(*to_csr(bags, F, fmaj), dev)
                kw = dict(combiner="sqrtn", max_norm=0.9, field_major=fmaj, want_fm=True)
                emb0, fm0 = st.lookup_bags(v, o, w, **kw)
                for lc in LIN_COMBINERS:
                    for b in (None, bias):
                        emb, fm, lin = st.lookup_bags(v, o, w, want_lin=True, lin_combiner=lc, lin_bias=b, **kw)
                        ok = lin.shape == (B, 1) and bool(torch.equal(emb, emb0)) and bool(torch.equal(fm, fm0))
                        if B:
                            want = ops.linear_logit(full_w, v, o, w, combiner=lc, bias=b, field_major=fmaj)
                            ok = ok and bool(torch.equal(lin, want))
                        if not ok:
                            bad.append((B, wmode, fmaj, lc, b is not None))
    assert not bad, "lookup_bags(want_lin=True) differs from ops.linear_logit (B, weights, field_major, combiner, bias): %s" % bad


def test_world1_forward_prune_matches_float64(built_lib):
    """PRUNE_NONPOSITIVE_WEIGHTS with signed weights: the term sees the lookup's live entries (the single-GPU linear_csr_k takes no such
    flag).  Within 1e-5 of float64 on the pruned bags: ~60 fp32 additions of terms of magnitude ~0.3 give an error near 1e-6."""
    from dir_amd import ops
    dev = torch.device("cuda", 0)
    vocab, K, B = [500, 1000, 7], 16, 300
    F = len(vocab)
    full, full_w = _draw(vocab, K, 31, dev)
    st = _tables(full, full_w)
    bags = draw_bags(np.random.default_rng(33), B, vocab, [60, 1, 3], "signed")
    W = [w.cpu().numpy() for w in full_w]
    for fmaj in (False, True):
        v, o, w = _dev(*to_csr(bags, F, fmaj), dev)
        for lc in LIN_COMBINERS:
            _, _, lin = st.lookup_bags(v, o, w, combiner="mean", field_major=fmaj, flags=ops.PRUNE_NONPOSITIVE_WEIGHTS, want_lin=True,
                                       lin_combiner=lc)
            err = _close(lin.reshape(-1), lin_forward64(W, lin_entries(bags, vocab, lc, True), B))
            print("prune %s field_major=%s: %.2e" % (lc, fmaj, err))
            assert err <= 1e-5, (lc, fmaj, err)
            unpruned = _close(lin.reshape(-1), lin_forward64(W, lin_entries(bags, vocab, lc, False), B))
            assert unpruned > 1e-3, "the pruned entries must not contribute"


# ---- 2. / 3. training against float64 ----------------------------------------------------------------------------------------------------
def _train_step(st, bags, F, case, lc, G, g, dev):
    from dir_amd import ops
    wmode, comb, mn, fmaj, prune = case
    v, o, w = _dev(*to_csr(bags, F, fmaj), dev)
    kw = dict(combiner=comb, max_norm=mn, field_major=fmaj, flags=ops.PRUNE_NONPOSITIVE_WEIGHTS if prune else 0)
    want = st.lookup_bags(v, o, w, want_lin=True, lin_combiner=lc, **kw)
    before = st._updates
    emb, lin = st.lookup_bags_train(v, o, w, with_linear=True, lin_combiner=lc, **kw)
    same = bool(torch.equal(emb.detach(), want[0])) and bool(torch.equal(lin.detach(), want[2]))
    ((emb * G.to(dev)).sum() + (lin * g.to(dev)).sum()).backward()
    return same and st._updates == before + 1


@pytest.mark.parametrize("lc", LIN_COMBINERS)
@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (0.05, 0.1)])
def test_world1_training_matches_float64(built_lib, l1, l2, lc):
    """Five steps over CASES: w, n, z within 1e-5 of float64 FTRL on the per-entry gradients w_e * c_bag * d lin (the bound
    tests/test_gpu_shard_linear.py holds the same update to); tables and accumulators within 1e-5 of float64 Adagrad."""
    dev = torch.device("cuda", 0)
    vocab, K = [500, 1000, 7], 16
    F = len(vocab)
    ftrl = dict(lr=0.2, l1=l1, l2=l2)
    full, full_w = _draw(vocab, K, 5, dev)
    st = _tables(full, full_w, ftrl)
    ref = [t.double().cpu().numpy() for t in full]
    acc = [np.full(t.shape, ACC0) for t in ref]
    lref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
    rng = np.random.default_rng(23)
    for c, case in enumerate(CASES):
        B = (37, 300, 0, 64, 129)[c]
        bags = draw_bags(rng, B, vocab, [60, 1, 3], case[0])
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32))
        g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32))
        assert _train_step(st, bags, F, case, lc, G, g, dev), "forward / update count, case %d" % c
        ref_step(ref, acc, bags, G.numpy(), case[1], case[2], case[4], LR)
        lin_ftrl64(lref.w, lref.n, lref.z, lin_entries(bags, vocab, lc, case[4]), g.numpy(), **ftrl)
        ew, en, ez = _state_err(st, lref)
        et = max(_close(st.local_tables[f], ref[f]) for f in range(F))
        ea = max(_close(st.optimizer.accums[f], acc[f]) for f in range(F))
        print("case %d %s l1=%g l2=%g: w %.2e n %.2e z %.2e tables %.2e accums %.2e" % (c, lc, l1, l2, ew, en, ez, et, ea))
        assert max(ew, en, ez, et, ea) <= 1e-5, (c, ew, en, ez, et, ea)
    if l1 > 0:
        moved = [(lref.n[f][:, 0] != ACC0) for f in range(F)]
        assert any(bool((w.cpu().numpy()[m] == 0).any()) for w, m in zip(st.linear_weights(), moved)), "l1 leaves some touched weights at 0.0"


def test_world1_training_skewed_bags_match_float64(built_lib):
    """tests/test_gpu_shard_bags_train._skewed_bags: B = 1500, a Zipf(1.3) slot, one row hit more than 600 times, a 300-entry bag.  w, n
    and z within 1e-5: the sorted update compensates its run sums (csrc/backward.hip: run_sum)."""
    dev = torch.device("cuda", 0)
    vocab, K, B = [5000, 2000, 800], 16, 1500
    F = len(vocab)
    ftrl = dict(lr=0.2, l1=0.01, l2=0.02)
    full, full_w = _draw(vocab, K, 7, dev)
    st = _tables(full, full_w, ftrl)
    lref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
    rng = np.random.default_rng(29)
    for step, (case, lc) in enumerate([(("pos", ["mean", "sum", "sqrtn"], [None, 1.2, None], False, False), "sum"),
                                       (("pos", ["sqrtn", "mean", "sum"], None, True, False), "mean")]):
        bags = _skewed_bags(rng, B, vocab, 17, 0, 300)
        hits = sum(int((bg[1][0] == 17).sum()) for bg in bags)
        assert hits > 600, hits
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32))
        g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32))
        assert _train_step(st, bags, F, case, lc, G, g, dev)
        lin_ftrl64(lref.w, lref.n, lref.z, lin_entries(bags, vocab, lc, False), g.numpy(), **ftrl)
        ew, en, ez = _state_err(st, lref)
        print("skewed step %d %s (%d hits): w %.2e n %.2e z %.2e" % (step, lc, hits, ew, en, ez))
        assert ew <= 1e-5 and en <= 1e-5 and ez <= 1e-5, (step, ew, en, ez)


def test_world1_training_hot_row_matches_float64(built_lib):
    """tests/test_gpu_shard_bags_train._hot_bags: 3200 of 4096 bags name one row -- a run over more than twelve sort tiles in the order the
    slab's atomics left, so the bar must hold for any order.  Three steps, every linear combiner: w, n, z within 1e-5; so are the tables
    and accumulators of the same node.  (d lin is drawn at 0.3: the row's summed gradient, sigma ~ 20, stays below 64, where fp32's own
    rounding of the sum is under 4e-6.)"""
    dev = torch.device("cuda", 0)
    vocab, K, B = [5000, 2000, 800], 16, 4096
    F = len(vocab)
    ftrl = dict(lr=0.2, l1=0.01, l2=0.02)
    full, full_w = _draw(vocab, K, 13, dev)
    st = _tables(full, full_w, ftrl)
    ref = [t.double().cpu().numpy() for t in full]
    acc = [np.full(t.shape, ACC0) for t in ref]
    lref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
    rng = np.random.default_rng(43)
    for step, (case, lc) in enumerate([(("pos", ["mean", "sum", "sqrtn"], [None, 1.2, None], False, False), "sum"),
                                       (("pos", ["sqrtn", "mean", "sum"], None, True, False), "mean"),
                                       (("pos", "sum", None, False, False), "sqrtn")]):
        bags = _hot_bags(rng, B, vocab, 17, 3200)
        hits = sum(int((bg[1][0] == 17).sum()) for bg in bags)
        assert hits >= 3000, hits
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32))
        g = torch.from_numpy((rng.standard_normal((B, 1)) * 0.3).astype(np.float32))
        assert _train_step(st, bags, F, case, lc, G, g, dev)
        ref_step(ref, acc, bags, G.numpy(), case[1], case[2], case[4], LR)
        lin_ftrl64(lref.w, lref.n, lref.z, lin_entries(bags, vocab, lc, False), g.numpy(), **ftrl)
        ew, en, ez = _state_err(st, lref)
        et = max(_close(st.local_tables[f], ref[f]) for f in range(F))
        ea = max(_close(st.optimizer.accums[f], acc[f]) for f in range(F))
        print("hot row step %d %s (%d entries): w %.2e n %.2e z %.2e tables %.2e accums %.2e" % (step, lc, hits, ew, en, ez, et, ea))
        assert max(ew, en, ez, et, ea) <= 1e-5, (step, ew, en, ez, et, ea)


# ---- 4. / 5. the two owner updates beside each other -----------------------------------------------------------------------------------
def test_owner_ftrl_on_its_own_sort_equals_on_the_adagrad_sort(built_lib):
    """ONE forward's slabs and gradients (where duplicates sit in the slabs depends on atomic order, so both orders read the same ones):
    FTRL sorting for itself, then -- the first-order rows restored -- Adagrad followed by FTRL on its sorted pairs: the same rows bit for
    bit.  A row repeated inside bags and across bags makes the run sums matter."""
    dev = torch.device("cuda", 0)
    vocab, K, B = [500, 1000, 7], 16, 400
    F = len(vocab)
    hp = (0.2, 0.01, 0.02)
    full, full_w = _draw(vocab, K, 53, dev)
    st = _tables(full, full_w, dict(lr=hp[0], l1=hp[1], l2=hp[2]))
    rng = np.random.default_rng(59)
    bags = draw_bags(rng, B, vocab, [60, 1, 3], "pos")
    for row in bags:
        if len(row[0][0]) >= 2:
            row[0][0][:2] = 5
    comb, mn, lc = ["mean", "sum", "sqrtn"], None, "sqrtn"
    v, o, w = _dev(*to_csr(bags, F, False), dev)
    G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).to(dev)
    _, plan, _ = st._bags_forward_train(v, o, w, comb, mn, False, 0, True, lc)
    be = st.backend
    lrows, lback, lden = plan.lin_buffers()
    be.bags_grad(G, plan.cap_b, plan.pos, plan.mask, plan.denom, B, comb, plan.rows)
    be.bags_linear_grad(g, plan.cap_b, plan.pos, plan.mask, lden, B, lc, lrows)
    rows0 = [r.clone() for r in st.lin_rows]
    be.bags_ftrl(plan.recv, plan.cap_e, plan.cap_b, lback, *hp)                              # its own key pass and sort
    own = [r.clone() for r in st.lin_rows]
    for r, r0 in zip(st.lin_rows, rows0):
        r.copy_(r0)
    be.bags_adagrad(st.optimizer, plan.recv, plan.cap_e, plan.cap_b, plan.back, mn)
    be.bags_ftrl(plan.recv, plan.cap_e, plan.cap_b, lback, *hp, sorted_by=st.optimizer)      # the Adagrad step's sorted pairs
    torch.cuda.synchronize()
    for f in range(F):
        assert torch.equal(st.lin_rows[f], own[f]), f
    assert not torch.equal(own[0][:, 0], rows0[0][:, 0]) and not torch.equal(st.local_tables[0], full[0])


def test_one_node_leaves_the_adagrad_side_bitwise(built_lib):
    """lookup_bags_train(with_linear=True) against a twin trained without the term: tables and accumulators torch.equal.  Every row
    appears at most once per slot (a permutation cut into bags): with one gradient per row there is no summation order (where duplicates
    sit in the slabs depends on atomic order), so any difference would be the term's doing."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, B = [5000, 3000, 1700], 16, 300
    F = len(vocab)
    full, full_w = _draw(vocab, K, 13, dev)
    st = _tables(full, full_w, dict(lr=0.2, l1=0.01, l2=0.02))
    twin = ShardedTables.from_full([t.clone() for t in full]).enable_training(LR, ACC0)
    rng = np.random.default_rng(37)
    comb, mn = ["sqrtn", "mean", "sum"], [None, 1.1, None]
    for step in range(2):
        perms = [rng.permutation(v) for v in vocab]
        bags, used = [], [0] * F
        for b in range(B):
            row = []
            for f, L in enumerate([int(rng.integers(0, 13)), 1, int(rng.integers(0, 6))]):
                row.append((perms[f][used[f]:used[f] + L].astype(np.int64), rng.uniform(0.1, 2.0, size=L).astype(np.float32)))
                used[f] += L
            bags.append(row)
        v, o, w = _dev(*to_csr(bags, F, step == 1), dev)
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).to(dev)
        kw = dict(combiner=comb, max_norm=mn, field_major=step == 1)
        w0 = [x.clone() for x in st.linear_weights()]
        emb, lin = st.lookup_bags_train(v, o, w, with_linear=True, lin_combiner="mean", **kw)
        ((emb * G).sum() + (lin * g).sum()).backward()
        e2 = twin.lookup_bags_train(v, o, w, **kw)
        assert torch.equal(e2.detach(), emb.detach())
        (e2 * G).sum().backward()
        torch.cuda.synchronize()
        for f in range(F):
            assert torch.equal(st.local_tables[f], twin.local_tables[f]), (step, f)
            assert torch.equal(st.optimizer.accums[f], twin.optimizer.accums[f]), (step, f)
            assert not torch.equal(st.linear_weights()[f], w0[f])          # ... while the first-order rows did take their step


# ---- 6. graph capture --------------------------------------------------------------------------------------------------------------------
def test_world1_graph_replay_equals_eager(built_lib):
    from dir_amd import ops
    dev = torch.device("cuda", 0)
    vocab, K = [300, 800, 20], 16
    F = len(vocab)
    full, full_w = _draw(vocab, K, 19, dev)
    st = _tables(full, full_w)
    rng = np.random.default_rng(41)
    bags = draw_bags(rng, 256, vocab, [1, 40, 3], "pos")
    v, o, w = _dev(*to_csr(bags, F, True), dev)
    bias = torch.tensor([-0.21], dtype=torch.float32, device=dev)
    kw = dict(combiner=["sum", "mean", "sqrtn"], max_norm=[None, 0.8, None], field_major=True, want_fm=True, want_lin=True,
              lin_combiner="mean", lin_bias=bias)
    e0, f0, l0 = (t.clone() for t in st.lookup_bags(v, o, w, **kw))               # one eager call: the plan and its float buffers exist
    step = ops.CapturedStep(lambda: st.lookup_bags(v, o, w, **kw))
    step.replay()
    torch.cuda.synchronize()
    assert torch.equal(step.out[0], e0) and torch.equal(step.out[1], f0) and torch.equal(step.out[2], l0)
    for r in st.lin_rows:                                                          # the first-order rows move in place
        r[:, 0].mul_(-1.5).add_(0.01)
    e1, f1, l1 = (t.clone() for t in st.lookup_bags(v, o, w, **kw))
    step.replay()
    torch.cuda.synchronize()
    assert torch.equal(step.out[0], e1) and torch.equal(step.out[1], f1) and torch.equal(step.out[2], l1)
    assert not torch.equal(l1, l0) and torch.equal(e1, e0)


# ---- 9. the 64-bit branch of the payload decode ------------------------------------------------------------------------------------------
def test_world1_wide_payload(built_lib):
    """F = 2048 slots of one row each, except slot 2047 with 2^20 + 16 rows; every id of that slot lies in its last 16 rows, so its
    payload word local_row * F + slot is >= 2^31: lookup(want_lin), lookup_bags(want_lin), one lookup_train(with_linear) step and one
    lookup_bags_train(with_linear) step decode it in 64 bits.  A gather copies rows, so the one-hot emb is the rows themselves; the
    one-hot and the bag term are ops.linear_logit's and the bag rows ops.embedding_bag's bit for bit (the neighbouring world-1 tests'
    contract); both training steps within 1e-5 of the float64 references (theirs too)."""
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    F, K, B, big = 2048, 4, 8, (1 << 20) + 16
    vocab = [1] * (F - 1) + [big]
    rng = np.random.default_rng(71)
    small = torch.from_numpy((rng.standard_normal((F - 1, K)) * 0.4).astype(np.float32)).to(dev)
    wide = torch.from_numpy((rng.standard_normal((big, K)) * 0.4).astype(np.float32)).to(dev)
    small_w = torch.from_numpy((0.3 * rng.standard_normal(F - 1)).astype(np.float32)).to(dev)
    wide_w = torch.from_numpy((0.3 * rng.standard_normal(big)).astype(np.float32)).to(dev)
    views = lambda a, b: [a[f:f + 1] for f in range(F - 1)] + [b]      # noqa: E731   2047 one-row views of one tensor + the wide table
    full, full_w = views(small.clone(), wide.clone()), views(small_w, wide_w)      # `full` stays untouched: st trains its own copy
    ftrl = dict(lr=0.2, l1=0.01, l2=0.02)
    st = ShardedTables.from_full(views(small, wide)).attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(**ftrl)
    lref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
    last = lambda n: rng.integers(big - 16, big, size=n).astype(np.int64)          # noqa: E731
    assert (big - 16) * F + F - 1 >= 1 << 31
    # one-hot
    ids_np = np.zeros((B, F), np.int64)
    ids_np[:, F - 1] = last(B)
    ids = torch.from_numpy(ids_np).to(dev)
    emb, lin = st.lookup(ids, want_lin=True)
    assert torch.equal(emb, torch.cat([small.reshape(1, -1).expand(B, -1), wide[ids[:, F - 1]]], dim=1))
    assert torch.equal(lin, ops.linear_logit(ops.TableSet.ftrl_rows(full_w), ids))
    # bags of 0..3 entries in the wide slot, 0..2 in the others
    bags = []
    for b in range(B):
        row = []
        for f in range(F):
            L = (0, 1, 2, 3, 3, 2, 1, 3)[b] if f == F - 1 else int(rng.integers(0, 3))
            row.append((last(L) if f == F - 1 else np.zeros(L, np.int64), rng.uniform(0.1, 2.0, size=L).astype(np.float32)))
        bags.append(row)
    v, o, w = _dev(*to_csr(bags, F, False), dev)
    kw = dict(combiner="mean", max_norm=0.9)
    embb, _, linb = st.lookup_bags(v, o, w, want_lin=True, lin_combiner="sqrtn", **kw)
    assert torch.equal(embb, ops.embedding_bag(full, v, o, w, **kw))
    assert torch.equal(linb, ops.linear_logit(full_w, v, o, w, combiner="sqrtn"))
    # one one-hot step, then one bag step, against float64
    G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).to(dev)
    e1, l1 = st.lookup_train(ids, with_linear=True)
    assert torch.equal(e1.detach(), emb) and torch.equal(l1.detach(), lin)
    ((e1 * G).sum() + (l1 * g).sum()).backward()
    lref.step(ids_np, G.cpu().numpy(), g.cpu().numpy(), ftrl)

    def errs(what):
        ew, en, ez = _state_err(st, lref)
        et = max(_close(st.local_tables[f], lref.T[f]) for f in range(F))
        ea = max(_close(st.optimizer.accums[f], lref.acc[f]) for f in range(F))
        assert max(ew, en, ez, et, ea) <= 1e-5, "%s: w %.2e n %.2e z %.2e tables %.2e accums %.2e" % (what, ew, en, ez, et, ea)
    errs("one-hot step")
    moved = lref.n[F - 1][:, 0] != ACC0
    assert moved[big - 16:].any() and not moved[:big - 16].any()                   # the rows named by the wide payloads took the step
    e2, l2 = st.lookup_bags_train(v, o, w, with_linear=True, lin_combiner="sqrtn", **kw)
    ((e2 * G).sum() + (l2 * g).sum()).backward()
    ref_step(lref.T, lref.acc, bags, G.cpu().numpy(), "mean", 0.9, False, LR)
    lin_ftrl64(lref.w, lref.n, lref.z, lin_entries(bags, vocab, "sqrtn", False), g.cpu().numpy(), **ftrl)
    errs("bag step")


# ---- 7. / 8. the trainer -----------------------------------------------------------------------------------------------------------------
class _Model64:
    """The float64 three-term DeepFM of the trainer tests: fm + dnn + (lin + bias) over the global bags, Adagrad on tables and dense
    parameters, FTRL on the first-order weights and on the bias."""

    def __init__(self, model, dense, names, full, full_w, vocab, K, combs, mns, lc, ftrl, lr_sparse, lr_dense):
        self.vocab, self.K, self.F, self.combs, self.mns, self.lc, self.ftrl = vocab, K, len(vocab), combs, mns, lc, ftrl
        self.lr_sparse, self.lr_dense = lr_sparse, lr_dense
        self.t64 = [t.double().cpu().numpy().copy() for t in full]
        self.acc64 = [np.full(t.shape, 0.1) for t in self.t64]
        self.lref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
        self.d64 = [p.detach().double().cpu().clone().requires_grad_(True) for p in dense]
        self.dacc = [torch.full_like(p, 0.1) for p in self.d64]
        self.pd = dict(zip(names, self.d64))
        self.b64 = model.linear_bias.detach().double().cpu().clone().requires_grad_(True)
        self.bn, self.bz = np.full(1, 0.1), np.zeros(1)

    def logits(self, T, W, bags):
        F, K, pd = self.F, self.K, self.pd
        emb = bags_forward64(T, bags, self.combs, self.mns, False)
        e3 = emb.view(-1, F, K)
        fm = 0.5 * ((e3.sum(1) ** 2) - (e3 ** 2).sum(1)).sum(1, keepdim=True)
        net = emb
        for i in range(2):
            net = torch.relu(net @ pd["hidden.%d.weight" % i].t() + pd["hidden.%d.bias" % i])
        lin = torch.zeros((len(bags), 1), dtype=torch.float64)
        for f, (bi, ids, coef) in enumerate(lin_entries(bags, self.vocab, self.lc, False)):
            lin = lin.index_add(0, torch.from_numpy(bi), torch.from_numpy(coef)[:, None] * W[f][torch.from_numpy(ids)])
        return fm + net @ pd["logits_layer.weight"].t() + pd["logits_layer.bias"] + lin + self.b64

    def step(self, bags, labels):
        from tests.shard_standin import NumpyBackend
        from tests.test_shard_bags_train_gloo import adagrad64
        F = self.F
        T = [torch.from_numpy(t).requires_grad_(True) for t in self.t64]
        W = [torch.from_numpy(w) for w in self.lref.w]
        logit = self.logits(T, W, bags)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, torch.from_numpy(labels), reduction="sum")
        grads = torch.autograd.grad(loss, T + self.d64 + [self.b64, logit], allow_unused=True)
        adagrad64(self.t64, self.acc64, [None if gr is None else gr.numpy() for gr in grads[:F]], self.lr_sparse)
        lin_ftrl64(self.lref.w, self.lref.n, self.lref.z, lin_entries(bags, self.vocab, self.lc, False), grads[-1].numpy(), **self.ftrl)
        with torch.no_grad():
            for p, a, gr in zip(self.d64, self.dacc, grads[F:F + len(self.d64)]):
                if gr is not None:
                    a += gr ** 2
                    p -= self.lr_dense * gr / a.sqrt()
            new = NumpyBackend._ftrl(self.b64.detach().numpy().copy(), self.bn, self.bz, grads[F + len(self.d64)].numpy(), **self.ftrl)
            self.b64.copy_(torch.from_numpy(new[0]))
            self.bn, self.bz = new[1], new[2]

    def errors(self, stt, dense, model, tr, sl):
        F = self.F
        ew, en, ez = _state_err(stt, self.lref, sl)
        return dict(tables=max(_close(stt.local_tables[f], self.t64[f][sl[f]]) for f in range(F)),
                    accums=max(_close(stt.optimizer.accums[f], self.acc64[f][sl[f]]) for f in range(F)),
                    w=ew, n=en, z=ez, dense=max(_close(p, r.detach().numpy()) for p, r in zip(dense, self.d64)),
                    bias=_close(torch.cat([model.linear_bias.data, tr.bias_accum, tr.bias_linear]),
                                np.concatenate([self.b64.detach().numpy(), self.bn, self.bz])))


def _trainer_run(rank, world, device, B, steps):
    """`steps` ShardedDeepFMTrainer.step_bags steps with linear= on a real DeepFM whose second column is a history column (bags of up to
    12 entries) -> (errors against the float64 three-term model, predict_bags error, the trainer).  Bound for the trained state: 2e-5,
    what tests/test_gpu_shard_bags_train.py holds the same trainer's step_bags to without the term."""
    from dir_amd import feature_column as fc
    from dir_amd.deepfm import DeepFM
    from dir_amd.shard import ShardedDeepFMTrainer, ShardedTables, local_slice
    vocab, K = [700, 2000, 3], 16
    F = len(vocab)
    combs, mns, lc = ["mean", "sqrtn", "sum"], [None, 0.8, None], "sqrtn"
    ftrl = dict(lr=0.15, l1=0.01, l2=0.02)
    cats = [fc.categorical_column_with_identity(n, v) for n, v in zip(("user", "history", "gender"), vocab)]
    torch.manual_seed(7)                                             # the same model on every rank
    cols = [fc.embedding_column(c, K, combiner=cb, max_norm=mn) for c, cb, mn in zip(cats, combs, mns)]
    model = DeepFM(linear_feature_columns=[], linear_sparse_combiner=lc, dnn_feature_columns=cols, dnn_hidden_units=[16, 16],
                   fm_embedding_size=K).to(device)
    with torch.no_grad():
        model.linear_bias.fill_(0.125)
    full = [p.detach().clone() for p in model.embedding_weights]
    full_w = [torch.from_numpy((0.3 * np.random.default_rng(3 + f).standard_normal(v)).astype(np.float32)).to(device) for f, v in enumerate(vocab)]
    stt = ShardedTables.from_full(full).attach_linear_from_full(full_w, 0.1)
    names = [n for n, _ in model.named_parameters() if not n.startswith(("embedding_weights", "linear_weights")) and n != "linear_bias"]
    dense = [p for n, p in model.named_parameters() if n in names]
    opt = torch.optim.Adagrad(dense, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    tr = ShardedDeepFMTrainer(model, stt, lr_sparse=0.05, dense_optimizer=opt, linear=ftrl)
    m64 = _Model64(model, dense, names, full, full_w, vocab, K, combs, mns, lc, ftrl, 0.05, 0.05)
    for s in range(steps):
        g = np.random.default_rng(1000 + s)
        bags_all = [draw_bags(g, B, vocab, [1, 12, 3], "pos") for _ in range(world)]
        lab_all = g.integers(0, 2, size=(world * B, 1)).astype(np.float64)
        v, o, w = _dev(*to_csr(bags_all[rank], F, s % 2 == 1), device)
        tr.step_bags(v, o, torch.from_numpy(lab_all[rank * B:(rank + 1) * B]).float().to(device), weights=w, field_major=s % 2 == 1)
        m64.step([b for bl in bags_all for b in bl], lab_all)
    sl = [slice(*local_slice(v, world, 0, world, rank)) for v in vocab]
    errs = m64.errors(stt, dense, model, tr, sl)
    v, o, w = _dev(*to_csr(bags_all[rank], F, False), device)
    got = tr.predict_bags(v, o, w)
    with torch.no_grad():
        want = m64.logits([torch.from_numpy(t) for t in m64.t64], [torch.from_numpy(x) for x in m64.lref.w], bags_all[rank]).numpy()
    return errs, (got.shape == (B, 1), _close(got, want)), tr


def test_world1_step_bags_and_predict_bags_with_linear(built_lib):
    errs, (shape_ok, ep), _ = _trainer_run(0, 1, torch.device("cuda", 0), 48, 3)
    print(" ".join("%s %.2e" % kv for kv in errs.items()), "predict %.2e" % ep)
    assert all(v <= 2e-5 for v in errs.values()), errs
    assert shape_ok and ep <= 1e-4, ep


def _scenarios(rank, world, device):
    import torch.distributed as dist
    from dir_amd import ops
    from dir_amd.shard import local_slice
    out = []
    vocab, K = [700, 2000, 3], 16
    F = len(vocab)
    ftrl = dict(lr=0.2, l1=0.01, l2=0.02)
    full, full_w = _draw(vocab, K, 77, device)
    st = _tables(full, full_w, ftrl)
    W = [w.cpu().numpy() for w in full_w]
    sl = [slice(*local_slice(v, world, 0, world, rank)) for v in vocab]
    rng = np.random.default_rng(500 + rank)
    bias = torch.tensor([0.37], dtype=torch.float32, device=device)
    # 1. bags whose live entries sit on ONE owner: one partial per bag, so the term is the unsharded ops.linear_logit's bit for bit
    B = 33 + 8 * rank
    bags = _one_owner_bags(rng, B, vocab, world, 20, lambda b, f: (b + f) % world)
    ok = True
    for fmaj, lc in ((False, "sum"), (True, "mean"), (False, "sqrtn")):
        v, o, w = _dev(*to_csr(bags, F, fmaj), device)
        _, _, lin = st.lookup_bags(v, o, w, combiner="mean", field_major=fmaj, want_lin=True, lin_combiner=lc, lin_bias=bias)
        ok = ok and bool(torch.equal(lin, ops.linear_logit(full_w, v, o, w, combiner=lc, bias=bias, field_major=fmaj)))
    out.append(("one_owner_bitwise", ok, "B=%d" % B))
    # 2. mixed-owner bags: the partials are added in owner order -- fp32 rounding only (~40 additions of terms ~0.3: near 1e-6)
    bags = draw_bags(rng, B, vocab, [40, 1, 3], "pos")
    v, o, w = _dev(*to_csr(bags, F, False), device)
    worst = 0.0
    for lc in LIN_COMBINERS:
        _, _, lin = st.lookup_bags(v, o, w, combiner="sqrtn", want_lin=True, lin_combiner=lc)
        worst = max(worst, _close(lin.reshape(-1), lin_forward64(W, lin_entries(bags, vocab, lc, False), B)))
    out.append(("mixed_owner_float64", worst <= 1e-5, "err=%.2e" % worst))
    # 3. one training step, a row hot on every rank, uneven batches
    ref = [t.double().cpu().numpy() for t in full]
    acc = [np.full(t.shape, ACC0) for t in ref]
    lref = Reference([t.cpu().numpy() for t in full], W)
    case, lc = CASES[2], "mean"
    g_ = np.random.default_rng(900)
    Bs = [41 + 17 * r for r in range(world)]
    bags_all = [draw_bags(g_, Bs[r], vocab, [40, 1, 3], case[0]) for r in range(world)]
    for bl in bags_all:
        for row in bl:
            if len(row[0][0]) > 1:
                row[0][0][:2] = 5                                    # row 5 of slot 0: repeated in bags, across bags and ranks
                row[0][1][:2] = np.abs(row[0][1][:2]) + 0.1
    G_all = [g_.standard_normal((Bs[r], F * K)).astype(np.float32) for r in range(world)]
    d_all = [g_.standard_normal((Bs[r], 1)).astype(np.float32) for r in range(world)]
    same = _train_step(st, bags_all[rank], F, case, lc, torch.from_numpy(G_all[rank]), torch.from_numpy(d_all[rank]), device)
    bags_g = [b for bl in bags_all for b in bl]
    ref_step(ref, acc, bags_g, np.concatenate(G_all, axis=0), case[1], case[2], case[4], LR)
    lin_ftrl64(lref.w, lref.n, lref.z, lin_entries(bags_g, vocab, lc, case[4]), np.concatenate(d_all, axis=0), **ftrl)
    ew, en, ez = _state_err(st, lref, sl)
    et = max(_close(st.local_tables[f], ref[f][sl[f]]) for f in range(F))
    ea = max(_close(st.optimizer.accums[f], acc[f][sl[f]]) for f in range(F))
    out.append(("train_step_hot_row", same and max(ew, en, ez, et, ea) <= 1e-5, "w %.2e n %.2e z %.2e tables %.2e accums %.2e" % (ew, en, ez, et, ea)))
    # 4. three step_bags steps against the float64 run of the global batches, predict_bags, and the bias state on every rank
    errs, (shape_ok, ep), tr = _trainer_run(rank, world, device, 48, 3)
    out.append(("step_bags", all(e <= 2e-5 for e in errs.values()), " ".join("%s %.2e" % kv for kv in errs.items())))
    out.append(("predict_bags", shape_ok and ep <= 1e-4, "err=%.2e" % ep))
    mine = torch.cat([tr.model.linear_bias.data, tr.bias_accum, tr.bias_linear])
    nccl = dist.get_backend() == "nccl"
    every = [torch.empty_like(mine) if nccl else torch.empty(3) for _ in range(world)]
    dist.all_gather(every, mine if nccl else mine.cpu())
    out.append(("bias_identical", all(torch.equal(e, every[0]) for e in every), ""))
    return out


def _worker(rank, world, store, transport, q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        import datetime
        import torch.distributed as dist
        if transport == "nccl":
            dev = torch.device("cuda", rank)
            torch.cuda.set_device(dev)
            dist.init_process_group("nccl", init_method="file://" + store, rank=rank, world_size=world, device_id=dev,
                                    timeout=datetime.timedelta(seconds=300))
        else:
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            os.environ["DIR_SHARD_HOST_STAGED"] = "1"                     # several ranks on ONE GPU: exchanges staged through host memory
            dev = torch.device("cuda", 0)
            torch.cuda.set_device(dev)
            dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
        try:
            import dir_amd
            dir_amd.load_library()
            res = _scenarios(rank, world, dev)
            torch.cuda.synchronize()
            q.put((rank, res))
        finally:
            dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


def _run(world, transport, timeout=300):
    """One fresh child process per rank, each under its own time limit: a child that has not reported and exited by then is killed."""
    import queue
    import time
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = _store()
    procs = [ctx.Process(target=_worker, args=(r, world, store, transport, q)) for r in range(world)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + timeout
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=max(1.0, deadline - time.monotonic())))
    except queue.Empty:
        res = None
    for p in procs:
        p.join(timeout=max(1.0, min(30.0, deadline + 30.0 - time.monotonic())))
        if p.is_alive():
            p.kill()                      # the exact processes this test started
    return res


def _check(res, world):
    assert res is not None, "the ranks did not report within the time limit"
    assert sorted(r for r, _ in res) == list(range(world))
    for rank, got in res:
        assert not isinstance(got, str), "rank %d raised:\n%s" % (rank, got)
        print("rank %d: %s" % (rank, got))
        bad = [(n, d) for n, ok, d in got if not ok]
        assert not bad, "rank %d: %s" % (rank, bad)
        assert len(got) == 6


def test_bags_linear_two_ranks_on_one_gpu(built_lib):
    """Two ranks on cuda:0 (gloo, host-staged exchanges)."""
    _check(_run(2, "gloo_same_device"), 2)


def test_bags_linear_over_rccl_one_rank_per_gpu(built_lib):
    """Backend nccl (= RCCL), world = min(8, visible devices), one rank per GPU.  Skipped on a one-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL at world > 1 needs >= 2 visible GPUs (this box shows %d); the same scenarios run on one GPU over gloo" % n)
    world = min(8, n)
    _check(_run(world, "nccl"), world)
