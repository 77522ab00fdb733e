"""GPU tests of ops.group_rank_stats (csrc/rank_metrics.hip) against the literal NumPy stand-in, and of metrics.GroupedMetrics on the device.
The edge sizes come from the library's own route limits (dir_group_rank_limits), never from numbers written here."""
import math
import os

import numpy as np
import pytest
import torch

from tests import rank_metrics_standin as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu(s, y, w, off):
    from dir_amd import ops
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = ops.group_rank_stats(T(s), T(y), T(w), T(off))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _edge_sizes(built_lib):
    from dir_amd import ops
    W, T = ops.group_rank_limits()
    return [0, 1, 2, 63, 64, 65, 0, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 3, 0]      # an empty group first, in the middle and last


_REF = {}


def _edge_case(built_lib, int_weights):
    """Inputs and the stand-in's statistics at the edge sizes; computed once per kind of weights and shared (never modified)."""
    if int_weights not in _REF:
        inp = S.ragged(31, _edge_sizes(built_lib), score_values=4, pos_rate=0.3, int_weights=int_weights)
        _REF[int_weights] = (inp, S.group_stats(*inp))
    return _REF[int_weights]


def test_edge_sizes_in_one_call_are_exact(built_lib):
    (s, y, w, off), ref = _edge_case(built_lib, True)
    assert np.unique(s).size == 4 and set(np.unique(w)) <= set(range(8))
    got = _gpu(s, y, w, off)
    for k in S.STATS:
        assert got[k].dtype == ref[k].dtype
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])     # integer-valued weights: the float64 sums are exact too
    assert ref["gt"].max() > 0 and ref["eq"].max() > 0 and (ref["n_pos"][[0, 6, 14]] == 0).all()


def test_float_weights(built_lib):
    (s, y, w, off), ref = _edge_case(built_lib, False)
    got = _gpu(s, y, w, off)
    for k in S.INT_STATS:
        assert np.array_equal(got[k], ref[k]), k
    for k in ("mis_w", "tot_w"):
        bound = ref["n_pos"] * 2.0 ** -52 * np.abs(ref[k])           # a reordered sum of n_pos non-negative terms
        err = np.abs(got[k] - ref[k])
        print(k, "largest error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (k, err, bound)


def test_weights_none_equals_ones(built_lib):
    (s, y, _, off), _ = _edge_case(built_lib, True)
    a, b = _gpu(s, y, None, off), _gpu(s, y, np.ones_like(s), off)
    for k in S.STATS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["tot_w"], (a["n_pos"] * a["n_neg"]).astype(np.float64))


def test_packing_and_tails(built_lib):
    sizes = np.random.default_rng(8).integers(0, 41, 1000)
    inp = S.ragged(9, sizes, score_values=6)
    ref, got = S.group_stats(*inp), _gpu(*inp)
    for k in S.STATS:
        assert np.array_equal(got[k], ref[k]), k
    for G in (1, 0):                                                 # one group: a workgroup with three idle waves; none: a no-op
        off = inp[3][:G + 1]
        n = int(off[-1])
        one = (inp[0][:n], inp[1][:n], inp[2][:n], off)
        ref, got = S.group_stats(*one), _gpu(*one)
        for k in S.STATS:
            assert got[k].shape == (G,) and np.array_equal(got[k], ref[k]), (G, k)


def test_single_class_groups(built_lib):
    from dir_amd import ops
    W, T = ops.group_rank_limits()
    sizes = [W, T + 1, W, T + 1]
    s, _, w, off = S.ragged(13, sizes, score_values=4)
    y = np.concatenate([np.ones(W + T + 1, np.float32), np.zeros(W + T + 1, np.float32)])
    ref, got = S.group_stats(s, y, w, off), _gpu(s, y, w, off)
    for k in S.STATS:
        assert np.array_equal(got[k], ref[k]), k
    assert got["n_pos"].tolist() == [W, T + 1, 0, 0] and got["n_neg"].tolist() == [0, 0, W, T + 1]
    for k in ("gt", "eq", "mis_w", "tot_w", "rank"):
        assert not got[k].any(), k


def test_single_positive_rank_among_equal_scores(built_lib):
    from dir_amd import ops
    W, T = ops.group_rank_limits()
    sizes, at = [], []
    for n in (1, 5, 64, 65, W, W + 1, T + 1, 2 * T + 3):
        for i in sorted({0, n // 2, n - 1}):                         # the positive first, in the middle, last
            sizes.append(n)
            at.append(i)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rng = np.random.default_rng(17)
    s = (rng.integers(0, 3, off[-1]) / np.float32(2.0)).astype(np.float32)
    y = np.zeros(off[-1], np.float32)
    for g, i in enumerate(at):
        s[off[g] + i] = 0.5                                          # the middle value: equal scores in front of it and behind it
        y[off[g] + i] = 1.0
    want = [S.stable_rank(s[off[g]:off[g + 1]], at[g]) for g in range(len(at))]
    ref, got = S.group_stats(s, y, None, off), _gpu(s, y, None, off)
    assert ref["rank"].tolist() == want
    for k in S.STATS:
        assert np.array_equal(got[k], ref[k]), k
    # all scores equal: the rank is the position
    s[:] = 0.25
    assert _gpu(s, y, None, off)["rank"].tolist() == [i + 1 for i in at]


def test_two_runs_give_the_same_bits(built_lib):
    (s, y, w, off), _ = _edge_case(built_lib, False)
    a, b = _gpu(s, y, w, off), _gpu(s, y, w, off)
    for k in ("mis_w", "tot_w"):
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k


def test_ops_checks_its_arguments(built_lib):
    from dir_amd import ops
    z = torch.zeros(4, device="cuda")
    off = torch.tensor([0, 4], device="cuda")
    with pytest.raises(TypeError):
        ops.group_rank_stats(z, z.double(), None, off)
    with pytest.raises(TypeError):
        ops.group_rank_stats(z, z, None, off.int())
    with pytest.raises(ValueError):
        ops.group_rank_stats(z, z[:3], None, off)
    with pytest.raises(ValueError):
        ops.group_rank_stats(z, torch.zeros(8, device="cuda")[::2], None, off)
    with pytest.raises(ValueError):
        ops.group_rank_stats(z, z, None, off.reshape(1, 2))


def _close(got, ref, tol):
    assert sorted(got) == sorted(ref)
    for k, r in ref.items():
        g = got[k]
        if isinstance(r, int):
            assert g == r, k
        else:
            assert (math.isnan(g) and math.isnan(r)) or abs(g - r) <= tol * max(1.0, abs(r)), (k, g, r)


def test_grouped_metrics_reproduces_the_reference_fixture(built_lib):
    from dir_amd.metrics import GroupedMetrics
    golden = np.load(os.path.join(ROOT, "tests", "golden", "ref_rank_metrics.npz"))
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    got = GroupedMetrics().update_blocks(T(golden["blk_scores"])).result()
    assert got["ranking_groups"] == got["groups"] == golden["blk_scores"].shape[0]
    # means of at most 48 float64 terms, summed in another order than NumPy's: 48 * 2^-53 relative, far inside 1e-12
    for k, name in (("hr@10", "hr"), ("ndcg@10", "ndcg"), ("mrr@10", "mrr")):
        assert abs(got[k] - float(golden[name])) <= 1e-12 * float(golden[name]), (k, got[k], float(golden[name]))
    m = GroupedMetrics().update(T(golden["wl_uid"]), T(golden["wl_label"]), T(golden["wl_pred"]), T(golden["wl_weight"]))
    assert math.isnan(m.result()["weighted_loss"]) and math.isnan(float(golden["wl_mean"]))         # the user whose pairs weigh nothing
    st = m.group_stats()
    pairs = (st["n_pos"] * st["n_neg"]).cpu().numpy() > 0
    with np.errstate(invalid="ignore"):
        loss = np.where(pairs, (st["mis_w"] / st["tot_w"]).cpu().numpy(), 0.0)
    assert np.array_equal(np.isnan(loss), np.isnan(golden["wl_loss"]))
    assert np.allclose(loss, golden["wl_loss"], rtol=1e-15, atol=0, equal_nan=True)                 # the fixture's weights make both sums exact
    keep = golden["wl_uid"] != golden["wl_users"][2]
    m = GroupedMetrics().update(T(golden["wl_uid"][keep]), T(golden["wl_label"][keep]), T(golden["wl_pred"][keep]), T(golden["wl_weight"][keep]))
    ref = float(golden["wl_mean_ordinary"])
    assert abs(m.result()["weighted_loss"] - ref) <= 1e-12 * ref


def test_grouped_metrics_gpu_equals_cpu_on_ragged_input(built_lib):
    from dir_amd.metrics import GroupedMetrics
    from dir_amd import ops
    W, _ = ops.group_rank_limits()
    rng = np.random.default_rng(41)
    sizes = np.minimum(rng.zipf(1.6, 200), W + 40)                   # about 200 ragged groups, a few on the workgroup route
    assert (sizes > W).any() and (sizes == 1).any()
    s, y, w, _ = S.ragged(42, sizes, score_values=16, int_weights=False)
    gid = np.repeat(rng.permutation(200) + 5, sizes)
    perm = rng.permutation(gid.size)
    cpu, gpu = GroupedMetrics(device="cpu"), GroupedMetrics()
    for part in (slice(0, gid.size // 2), slice(gid.size // 2, None)):
        k = perm[part]
        args = [torch.from_numpy(a[k]) for a in (gid, y, s, w)]
        cpu.update(*args)
        gpu.update(*[a.cuda() for a in args])
    blocks = torch.from_numpy(rng.random((30, 20)).astype(np.float32))
    cpu.update_blocks(blocks, block=20, positive_index=3)
    gpu.update_blocks(blocks.cuda(), block=20, positive_index=3)
    a, b = gpu.result(), cpu.result()
    assert a["groups"] == 230 and a["gauc_groups"] > 50
    _close(a, b, 1e-12)
