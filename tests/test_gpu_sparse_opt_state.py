"""State that outlives a call on ONE sorted sparse optimiser while the sizes change (dir_amd.sparse_opt): the sort area regrown
between steps, Adam's row marks and norm words across that, the sort an apply half takes from its norm half, the sort FTRL borrows from
the Adagrad step.  The other GPU files run every entry at one size per optimiser instance.

Tables: F = 3, vocab [5, 1, 70] (a one-row table, a table smaller than a tile), K in {4, 16} (the two vector paths); 5 and 700 entries
(700 >= three 256-entry tiles: the carry rows and the fix-up kernel run).

  1. Adam, payload form, four steps of 5, 700, 5 and 0 words on one optimiser, clip idle (0) and active: var, m, v against the float64
     dense Adam of the sharded Adam tests (tests.test_shard_adam_gloo.Reference), measure and bar tests.test_gpu_shard_adam's (_errs, BAR).
  2. No stale sort: twins from one state; A: norm(p1), norm(p2), step(p1); B: norm(p1), step(p1) -- p2 larger (the area is reallocated),
     of p1's size in another tensor, or p1 itself rewritten in place between the halves (B is given the rewritten values): bitwise equal,
     A.sort_reuses == 0, B.sort_reuses == 1.  p1 names distinct rows.
  3. Both through a world-1 ShardedTables under enable_training_adam over bag records, local batches 2, 96 and 2 with one-hot steps in
     between: tests.test_gpu_shard_bags_adam's helpers, BagsAdamReference, the same bar.
  4. SparseAdagrad.step_payload then SparseFtrl.step_payload(sorted_by=adagrad) at 5, 700 and 5 words on one pair against a twin pair
     whose FTRL sorts for itself: weights, n and z bitwise; the same over rows of units = 2 and with step_bags over the
     world-1 bag lookup's slabs."""
import numpy as np
import pytest
import torch

from tests.shard_standin_bags_adam import BagsAdamReference
from tests.test_gpu_shard_adam import BAR, _errs
from tests.test_gpu_shard_bags_adam import _bag_step, _sharded, _state
from tests.test_gpu_sort_plans import _sum_shares
from tests.test_shard_adam_gloo import B1, B2, EPS, LR, Reference, lr_t_of
from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr

pytestmark = pytest.mark.gpu
VOCAB = [5, 1, 70]
F = len(VOCAB)
KS = [4, 16]
GSCALE, CLIP = 5.0, 1.0          # an entry's gradient has norm about 5 sqrt(K) >= 10: every table that is named at all is clipped


def _w0(K, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in VOCAB]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _words(rng, n, K, distinct=False, width=None):
    """-> (slot [n], row [n], payload [n] int64 with a few pruned words, grad [n, K or width]); n >= 3 names every table."""
    if distinct:
        pairs = [(f, r) for f, v in enumerate(VOCAB) for r in range(v)]
        pick = [pairs[i] for i in rng.permutation(len(pairs))[:n]]
        slot, row = np.array([p[0] for p in pick]), np.array([p[1] for p in pick])
    else:
        slot = rng.integers(0, F, size=n)
        slot[:min(n, F)] = np.arange(F)[:min(n, F)]
        row = np.array([rng.integers(0, VOCAB[f]) for f in slot], dtype=np.int64).reshape(n)
    pay = (row * F + slot).astype(np.int64)
    if n > 50:
        pay[F + rng.permutation(n - F)[:n // 20]] = -1      # (the first F words stay: every table is named)
    grad = (rng.standard_normal((n, width or K)) * GSCALE).astype(np.float32)
    return slot, row, pay, grad


def _as_onehot(slot, pay, grad, K):
    """The payload words as the one-hot batch the float64 reference takes: word i is sample i, named in its slot's column only."""
    n = len(pay)
    ids = np.full((n, F), -1, np.int64)
    G = np.zeros((n, F * K), np.float32)
    for i in np.flatnonzero(pay >= 0):
        ids[i, slot[i]] = pay[i] // F
        G[i, slot[i] * K:(slot[i] + 1) * K] = grad[i]
    return ids, G


def _adam(w0, clip):
    from dir_amd import ops
    tabs = [_cuda(w.copy()) for w in w0]
    return tabs, ops.SparseAdam(ops.TableSet(tabs), B1, B2, EPS, clip)


def _halves(opt, pay, grad):
    norms = _sum_shares(opt.norm_payload(pay, grad)) if opt.clip_norm > 0 else None
    opt.step_payload(pay, grad, norms)


# ---- 1. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0.0, CLIP], ids=["noclip", "clip_active"])
@pytest.mark.parametrize("K", KS)
def test_adam_payload_halves_across_a_regrown_sort_area(built_lib, K, clip):
    rng = np.random.default_rng(10 * K + int(clip))
    w0 = _w0(K, K)
    tabs, opt = _adam(w0, clip)
    ref = Reference(w0, clip)
    for t, n in enumerate((5, 700, 5, 0), 1):
        slot, _, pay, grad = _words(rng, n, K)
        opt.lr_t = lr_t_of(t)
        _halves(opt, _cuda(pay), _cuda(grad).reshape(n, K))
        torch.cuda.synchronize()                        # a launch error would surface here
        ref.step(*_as_onehot(slot, pay, grad, K))
        if clip > 0:
            assert (min(ref.norms[-1]) > clip) if n else (max(ref.norms[-1]) == 0.0), "step %d: norms %s" % (t, ref.norms[-1])
        e = _errs(tabs, opt.ms, opt.vs, ref)
        print("K=%d clip=%g step %d (%d words): var %.2e m %.2e v %.2e" % (K, clip, t, n, e["var"], e["m"], e["v"]))
        assert all(x <= BAR for x in e.values()), (t, n, e)
    assert opt.steps == 4 and opt.sort_reuses == (3 if clip > 0 else 0)      # (nothing to sort at n = 0; no norm half without a clip)


# ---- 2. ------------------------------------------------------------------------------------------------------------------------------
def _assert_twins(a, b, what):
    for name, xs, ys in zip(("var", "m", "v"), a, b):
        for f in range(F):
            assert torch.equal(xs[f], ys[f]), "%s: %s of table %d differs" % (what, name, f)


@pytest.mark.parametrize("kind", ["larger", "same_size_other_tensor", "rewritten_in_place"])
@pytest.mark.parametrize("K", KS)
def test_adam_payload_apply_never_runs_on_a_stale_sort(built_lib, K, kind):
    rng = np.random.default_rng(20 * K + len(kind))
    w0 = _w0(K, 2 * K)
    (ta, A), (tb, B) = _adam(w0, CLIP), _adam(w0, CLIP)
    A.lr_t = B.lr_t = lr_t_of(1)
    _, _, p1, g1 = _words(rng, 5, K, distinct=True)
    _, _, p2, g2 = _words(rng, 700 if kind == "larger" else 5, K, distinct=kind != "larger")
    assert len(set(p1.tolist())) == 5 and not np.array_equal(p1, p2)
    g1 = _cuda(g1)
    if kind == "rewritten_in_place":
        pa, pb = _cuda(p1), _cuda(p2)                   # A's tensor holds p1 for the norm half and p2's words for the apply half
        A.norm_payload(pa, g1)
        pa.copy_(pb)
    else:
        pa = pb = _cuda(p1)
        A.norm_payload(pa, g1)
        A.norm_payload(_cuda(p2), _cuda(g2))
    norms = _sum_shares(B.norm_payload(pb, g1))         # the words the apply halves see: one global norm for both twins
    B.step_payload(pb, g1, norms)
    A.step_payload(pa, g1, norms)
    torch.cuda.synchronize()
    assert (A.sort_reuses, B.sort_reuses) == (0, 1)
    _assert_twins((ta, A.ms, A.vs), (tb, B.ms, B.vs), kind)
    assert any(not torch.equal(ta[f].cpu(), torch.from_numpy(w0[f])) for f in range(F)), "the step moved no row"


# ---- 3. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0.0, CLIP], ids=["noclip", "clip_active"])
@pytest.mark.parametrize("K", KS)
def test_adam_bag_halves_across_growth_with_one_hot_steps_between(built_lib, K, clip):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(30 * K + int(clip))
    w0 = _w0(K, 3 * K)
    st = _sharded(w0, clip, dev)
    ref = BagsAdamReference(w0, LR, B1, B2, EPS, clip)
    t = 0
    for B, c in ((2, 0), (96, 3), (2, 4)):
        case = CASES[c]
        t += 1
        bags = draw_bags(rng, B, VOCAB, [6, 6, 6], case[0])
        G = (rng.standard_normal((B, F * K)) * GSCALE).astype(np.float32)
        _bag_step(st, bags, case, G, t, dev)
        ref.step(bags, G, case[1], case[2], case[4])
        t += 1
        ids = np.stack([rng.integers(-1, v + 1, size=B) for v in VOCAB], 1).astype(np.int64)
        G = (rng.standard_normal((B, F * K)) * GSCALE).astype(np.float32)
        st.optimizer.lr_t = lr_t_of(t)
        st.lookup_train(_cuda(ids)).backward(_cuda(G))
        ref.step_onehot(ids, G)
        torch.cuda.synchronize()
        e = _errs(*_state(st), ref)
        print("K=%d clip=%g after %d steps (batch %d): var %.2e m %.2e v %.2e" % (K, clip, t, B, e["var"], e["m"], e["v"]))
        assert all(x <= BAR for x in e.values()), (t, B, e)
    assert st._updates == 6 and st.optimizer.steps == 6
    if clip > 0:
        assert st.optimizer.sort_reuses >= 3            # every bag step's apply half ran on its norm half's sort


def _slabs(st, rng, B, dev):
    """The slabs one forward of B bags leaves on the owner, as a tensor of its own -> (recv, cap_e, cap_b).  Two bags of at most 2
    entries fill at most 12 of the smallest slab's 16 entry slots: every such forward has the same geometry."""
    v, o, w = to_csr(draw_bags(rng, B, VOCAB, [2, 2, 2] if B <= 2 else [6, 6, 6], None), F, False)
    _, plan, _ = st._bags_forward_train(_cuda(v), _cuda(o), None, "mean", None, False, 0, False)
    torch.cuda.synchronize()
    return plan.recv.clone(), plan.cap_e, plan.cap_b


@pytest.mark.parametrize("kind", ["larger", "same_size_other_tensor", "rewritten_in_place"])
@pytest.mark.parametrize("K", KS)
def test_adam_bag_apply_never_runs_on_a_stale_sort(built_lib, K, kind):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(40 * K + len(kind))
    w0 = _w0(K, 4 * K)
    sa, sb = _sharded(w0, CLIP, dev), _sharded(w0, CLIP, dev)
    A, B = sa.optimizer, sb.optimizer
    A.lr_t = B.lr_t = lr_t_of(1)
    r1, cap_e, cap_b = _slabs(sa, rng, 2, dev)
    r2, cap_e2, cap_b2 = _slabs(sa, rng, 96 if kind == "larger" else 2, dev)
    if kind == "larger":
        assert cap_e2 > cap_e
    else:
        assert (cap_e2, cap_b2) == (cap_e, cap_b) and not torch.equal(r1, r2)
    P = sa.backend.P
    g1 = _cuda((rng.standard_normal((P * cap_b, K)) * GSCALE).astype(np.float32))
    g2 = _cuda((rng.standard_normal((P * cap_b2, K)) * GSCALE).astype(np.float32))
    if kind == "rewritten_in_place":
        ra, rb = r1, r2
        A.norm_bags(ra, P, cap_e, cap_b, g1)
        ra.copy_(rb)
    else:
        ra = rb = r1
        A.norm_bags(ra, P, cap_e, cap_b, g1)
        A.norm_bags(r2, P, cap_e2, cap_b2, g2)
    norms = _sum_shares(B.norm_bags(rb, P, cap_e, cap_b, g1))
    B.step_bags(rb, P, cap_e, cap_b, g1, norms)
    A.step_bags(ra, P, cap_e, cap_b, g1, norms)
    torch.cuda.synchronize()
    assert (A.sort_reuses, B.sort_reuses) == (0, 1)
    _assert_twins(_state(sa), _state(sb), kind)
    assert any(not torch.equal(sa.local_tables[f].cpu(), torch.from_numpy(w0[f])) for f in range(F)), "the step moved no row"


# ---- 4. ------------------------------------------------------------------------------------------------------------------------------
HP = (0.2, 0.01, 0.02)           # FTRL lr, l1, l2


def _pair(w0, full_w, dev):
    """-> (ShardedTables with first-order rows, its SparseAdagrad, its SparseFtrl): one pair of owner-side optimisers."""
    from dir_amd.shard import ShardedTables
    st = ShardedTables.from_full([_cuda(w.copy()) for w in w0]).attach_linear_from_full([_cuda(w.copy()) for w in full_w], 0.1)
    st.enable_training(0.3, 0.1).enable_linear_training(*HP)
    return st, st.optimizer, st.backend._ftrl_opt(*HP)


def _assert_pairs(sa, sb, what):
    for f in range(F):
        assert torch.equal(sa.lin_rows[f], sb.lin_rows[f]), "%s: first-order rows [w | n | z] of slot %d differ" % (what, f)
        assert torch.equal(sa.local_tables[f], sb.local_tables[f]), "%s: table %d differs" % (what, f)


@pytest.mark.parametrize("units", [1, 2])
@pytest.mark.parametrize("K", KS)
def test_ftrl_on_a_borrowed_payload_sort_across_growth(built_lib, K, units):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(50 * K + units)
    w0 = _w0(K, 5 * K)
    full_w = [(0.3 * rng.standard_normal((v, units) if units > 1 else v)).astype(np.float32) for v in VOCAB]
    (sa, ada_a, ftrl_a), (sb, ada_b, ftrl_b) = _pair(w0, full_w, dev), _pair(w0, full_w, dev)
    for n in (5, 700, 5):
        _, _, pay, grows = _words(rng, n, K)
        pay, grows = _cuda(pay), _cuda(grows)
        g = _cuda(rng.standard_normal((n, units) if units > 1 else n).astype(np.float32))
        ada_a.step_payload(pay, grows)
        ftrl_a.step_payload(pay, g, sorted_by=ada_a)     # the Adagrad step's sorted pairs
        ada_b.step_payload(pay, grows)
        ftrl_b.step_payload(pay, g)                      # its own key pass and sort
        torch.cuda.synchronize()
        _assert_pairs(sa, sb, "units=%d, %d words" % (units, n))
    assert not torch.equal(sa.lin_rows[2][:, 0].cpu(), torch.from_numpy(full_w[2].reshape(VOCAB[2], -1)[:, 0]))


@pytest.mark.parametrize("K", KS)
def test_ftrl_on_a_borrowed_bag_sort_across_growth(built_lib, K):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(60 * K)
    w0 = _w0(K, 6 * K)
    full_w = [(0.3 * rng.standard_normal(v)).astype(np.float32) for v in VOCAB]
    (sa, ada_a, ftrl_a), (sb, ada_b, ftrl_b) = _pair(w0, full_w, dev), _pair(w0, full_w, dev)
    P = sa.backend.P
    for B in (2, 96, 2):
        recv, cap_e, cap_b = _slabs(sa, rng, B, dev)    # ONE forward's slabs for both pairs (where duplicates sit depends on atomic order)
        grows = _cuda(rng.standard_normal((P * cap_b, K)).astype(np.float32))
        g = _cuda(rng.standard_normal(P * cap_b).astype(np.float32))
        ada_a.step_bags(recv, P, cap_e, cap_b, grows)
        ftrl_a.step_bags(recv, P, cap_e, cap_b, g, sorted_by=ada_a)
        ada_b.step_bags(recv, P, cap_e, cap_b, grows)
        ftrl_b.step_bags(recv, P, cap_e, cap_b, g)
        torch.cuda.synchronize()
        _assert_pairs(sa, sb, "batch %d" % B)
    assert not torch.equal(sa.lin_rows[2][:, 0].cpu(), torch.from_numpy(full_w[2]))
