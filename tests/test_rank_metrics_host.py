"""CPU tests of the grouped ranking metrics' host logic: the NumPy stand-in against the results recorded from the reference's own functions
(tests/golden/ref_rank_metrics.npz, written by tools/record_rank_metrics.py), and metrics.GroupedMetrics(device="cpu") against the stand-in."""
import math
import os

import numpy as np
import pytest
import torch

from tests import rank_metrics_standin as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K10 = ("hr@10", "ndcg@10", "mrr@10")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_rank_metrics.npz")))


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _block_inputs(blocks, positive_index=0):
    B, n = blocks.shape
    labels = np.zeros((B, n), np.float32)
    labels[:, positive_index] = 1.0
    return blocks.reshape(-1), labels.reshape(-1), None, np.arange(B + 1, dtype=np.int64) * n


def _by_user(golden):
    order = np.argsort(golden["wl_uid"], kind="stable")
    users, counts = np.unique(golden["wl_uid"], return_counts=True)
    assert np.array_equal(users, golden["wl_users"])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return golden["wl_pred"][order], golden["wl_label"][order], golden["wl_weight"][order], offsets


def test_fixture_holds_the_cases_the_reference_leaves_defined(golden):
    blocks = golden["blk_scores"]
    assert blocks.dtype == np.float32 and blocks.shape[1] == 100
    for b in range(blocks.shape[0]):
        assert np.unique(blocks[b]).size == 100, "block %d holds a tie: the reference's quicksort leaves its order undefined" % b
    ranks = [S.stable_rank(blocks[b], 0) for b in range(3)]
    assert ranks == [1, 10, 11]
    assert golden["blk_hit"][:3].tolist() == [1.0, 1.0, 0.0]
    loss = golden["wl_loss"]
    assert loss[0] == 0.0 and loss[1] == 0.0 and math.isnan(loss[2]) and np.isfinite(loss[3:]).all()
    assert math.isnan(float(golden["wl_mean"])) and 0.0 < float(golden["wl_mean_ordinary"]) < 1.0


def test_standin_reproduces_the_reference_blocks(golden):
    st = S.group_stats(*_block_inputs(golden["blk_scores"]))
    assert (st["n_pos"] == 1).all() and (st["n_neg"] == 99).all()
    for b, r in enumerate(st["rank"].tolist()):
        hit = r <= 10
        assert (1.0 if hit else 0.0) == golden["blk_hit"][b]
        assert _rel(1.0 / np.log2(r + 1.0) if hit else 0.0, golden["blk_ndcg"][b]) <= 1e-15
        assert _rel(1.0 / r if hit else 0.0, golden["blk_mrr"][b]) <= 1e-15
    agg = S.aggregate(st, 10)
    assert agg["ranking_groups"] == golden["blk_scores"].shape[0]
    assert agg["hr@10"] == float(golden["hr"])
    assert _rel(agg["ndcg@10"], float(golden["ndcg"])) <= 1e-15
    assert _rel(agg["mrr@10"], float(golden["mrr"])) <= 1e-15


def test_standin_reproduces_the_reference_weighted_loss(golden):
    st = S.group_stats(*_by_user(golden))
    U = golden["wl_users"].size
    for u in range(U):
        pairs = st["n_pos"][u] * st["n_neg"][u]
        with np.errstate(invalid="ignore"):
            got = st["mis_w"][u] / st["tot_w"][u] if pairs else 0.0
        ref = golden["wl_loss"][u]
        assert (math.isnan(got) and math.isnan(ref)) or _rel(got, ref) <= 1e-15, u
    assert math.isnan(S.aggregate(st)["weighted_loss"])
    keep = np.arange(U) != 2
    sub = {k: v[keep] for k, v in st.items()}
    assert _rel(S.aggregate(sub)["weighted_loss"], float(golden["wl_mean_ordinary"])) <= 1e-15


def _same(got, ref, tol=1e-12):
    assert sorted(got) == sorted(ref)
    for k, r in ref.items():
        g = got[k]
        if isinstance(r, int):
            assert g == r, k
        else:
            assert (math.isnan(g) and math.isnan(r)) or abs(g - r) <= tol * max(1.0, abs(r)), (k, g, r)


def _ragged_case(distinct):
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 30, 60)
    sizes[[0, 17, 59]] = 0
    s, y, w, off = S.ragged(12, sizes, score_values=None if distinct else 5, int_weights=False)
    gid = np.repeat(np.arange(60) * 3 + 100, sizes)               # ids with gaps; the empty groups simply never appear
    live = sizes > 0
    off_live = np.concatenate([[0], np.cumsum(sizes[live])]).astype(np.int64)
    return s, y, w, gid, off_live


def _feed(m, gid, y, s, w, parts):
    T = torch.from_numpy
    for k in parts:
        m.update(T(gid[k]), T(y[k]), T(s[k]), None if w is None else T(w[k]))
    return m


def test_grouped_metrics_cpu_one_call_equals_the_standin(built_lib):
    from dir_amd.metrics import GroupedMetrics
    s, y, w, gid, off = _ragged_case(distinct=False)
    ref_st = S.group_stats(s, y, w, off)
    m = _feed(GroupedMetrics(device="cpu"), gid, y, s, w, [slice(None)])
    st = m.group_stats()
    for k in S.INT_STATS:
        assert np.array_equal(st[k].numpy(), ref_st[k]), k
    for k in ("mis_w", "tot_w"):
        # a reordered float64 sum of at most 30 non-negative terms (the groups hold fewer than 30 entries)
        assert np.allclose(st[k].numpy(), ref_st[k], rtol=30 * 2.0 ** -52, atol=0), k
    _same(m.result(), S.aggregate(ref_st))
    assert m.result()["gauc_groups"] > 10 and m.result()["ranking_groups"] > 3


def test_grouped_metrics_cpu_three_calls_split_groups(built_lib):
    from dir_amd.metrics import GroupedMetrics
    s, y, w, gid, off = _ragged_case(distinct=False)
    n = s.size
    cuts = [slice(0, n // 3 + 1), slice(n // 3 + 1, 2 * n // 3 + 2), slice(2 * n // 3 + 2, n)]      # the cuts fall inside groups
    assert gid[cuts[0]][-1] == gid[cuts[1]][0] and gid[cuts[1]][-1] == gid[cuts[2]][0]
    m = _feed(GroupedMetrics(device="cpu"), gid, y, s, w, cuts)
    _same(m.result(), S.aggregate(S.group_stats(s, y, w, off)))


def test_grouped_metrics_cpu_shuffled_samples(built_lib):
    from dir_amd.metrics import GroupedMetrics
    s, y, w, gid, off = _ragged_case(distinct=True)
    assert np.unique(s).size == s.size                            # distinct scores: the order inside a group does not matter
    perm = np.random.default_rng(5).permutation(s.size)
    m = _feed(GroupedMetrics(device="cpu"), gid[perm], y[perm], s[perm], w[perm], [slice(0, 200), slice(200, None)])
    _same(m.result(), S.aggregate(S.group_stats(s, y, w, off)))


def test_grouped_metrics_cpu_default_weights_and_k(built_lib):
    from dir_amd.metrics import GroupedMetrics
    s, y, _, gid, off = _ragged_case(distinct=False)
    m = _feed(GroupedMetrics(k=3, device="cpu"), gid, y, s, None, [slice(None)])
    _same(m.result(), S.aggregate(S.group_stats(s, y, None, off), k=3))


def test_grouped_metrics_cpu_update_blocks(built_lib, golden):
    from dir_amd.metrics import GroupedMetrics
    blocks = golden["blk_scores"]
    m = GroupedMetrics(device="cpu").update_blocks(torch.from_numpy(blocks[:20]))
    m.update_blocks(torch.from_numpy(blocks[20:].reshape(-1)), block=100, positive_index=0)
    got = m.result()
    _same(got, S.aggregate(S.group_stats(*_block_inputs(blocks))))
    for k, name in zip(K10, ("hr", "ndcg", "mrr")):
        assert abs(got[k] - float(golden[name])) <= 1e-12
    # another positive index, beside samples fed by update(): the blocks are groups of their own
    rolled = np.roll(blocks, 7, axis=1).copy()
    s, y, w, gid, off = _ragged_case(distinct=False)
    m = _feed(GroupedMetrics(device="cpu"), gid, y, s, w, [slice(None)]).update_blocks(torch.from_numpy(rolled), positive_index=7)
    bs, by, _, boff = _block_inputs(rolled, 7)
    ref = S.group_stats(np.concatenate([s, bs]), np.concatenate([y, by]), np.concatenate([w, np.ones(bs.size, np.float32)]),
                        np.concatenate([off, boff[1:] + off[-1]]))
    _same(m.result(), S.aggregate(ref))
    with pytest.raises(ValueError):
        GroupedMetrics(device="cpu").update_blocks(torch.zeros(250))


def test_rank_is_the_stable_argsort_position_with_ties(built_lib):
    from dir_amd.metrics import GroupedMetrics
    rng = np.random.default_rng(21)
    sizes = rng.integers(1, 50, 80)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    s = (rng.integers(0, 4, off[-1]) / np.float32(4.0)).astype(np.float32)          # four values: ties on both sides of every positive
    y = np.zeros(off[-1], np.float32)
    at = [int(off[g] + rng.integers(0, sizes[g])) for g in range(80)]
    y[at] = 1.0
    want = [S.stable_rank(s[off[g]:off[g + 1]], at[g] - off[g]) for g in range(80)]
    assert S.group_stats(s, y, None, off)["rank"].tolist() == want
    m = GroupedMetrics(device="cpu").update(torch.from_numpy(np.repeat(np.arange(80), sizes)), torch.from_numpy(y), torch.from_numpy(s))
    assert m.group_stats()["rank"].tolist() == want


def test_empty_accumulator_returns_zeros(built_lib):
    from dir_amd.metrics import GroupedMetrics
    got = GroupedMetrics(device="cpu").result()
    assert got == {"gauc": 0.0, "gauc_groups": 0, "weighted_loss": 0.0, "hr@10": 0.0, "ndcg@10": 0.0, "mrr@10": 0.0, "ranking_groups": 0,
                   "groups": 0}
    assert got == S.aggregate(S.group_stats(np.zeros(0, np.float32), np.zeros(0, np.float32), None, np.zeros(1, np.int64)))


def test_update_refuses_mismatched_arguments(built_lib):
    from dir_amd.metrics import GroupedMetrics
    m = GroupedMetrics(device="cpu")
    with pytest.raises(ValueError):
        m.update(torch.zeros(3, dtype=torch.int64), torch.zeros(3), torch.zeros(4))
    with pytest.raises(TypeError):
        m.update(torch.zeros(3), torch.zeros(3), torch.zeros(3))
    with pytest.raises(RuntimeError):
        GroupedMetrics(device="cuda").update(torch.zeros(3, dtype=torch.int64), torch.zeros(3), torch.zeros(3))
