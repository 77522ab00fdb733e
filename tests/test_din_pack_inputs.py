"""CPU self-checks of tests/din_pack_inputs.py: the restated geometry of csrc/din_pack.hip gives the launches the kernel's text gives, every
case reaches the edge it is named for, and on every case's operands fp32 NumPy stays within a tenth of the GPU tests' bar of float64 -- so
the bar (1e-5 scaled) measures the kernel and not the case's conditioning.  A case that misses the last check is reshaped; the bar stays."""
import numpy as np
import pytest

from oracle import np_ref as R
from tests import din_pack_inputs as D


def _geo(c):
    B, T = c.hist.shape
    return c.hist_len, T, B


def test_geometry_restates_the_launch():
    assert D.chunks(1) == (64, 1) and D.chunks(65536) == (64, 1024) and D.chunks(65537) == (128, 513) and D.chunks(131073) == (256, 513)
    assert D.launch(1) == (1, 8) and D.launch(3) == (1, 8) and D.launch(17) == (2, 16) and D.launch(40) == (3, 24)
    assert D.launch(4096) == (256, 2048) and D.launch(1 << 20) == (256, 2048)
    assert D.covers(64, 65535, 80, 48) and not D.covers(64, 65536, 80, 48) and not D.covers(64, 50, 84, 40) and not D.covers(64, 50, 80, 42)
    # equal lengths: the ranges are the even split
    assert D.partition(np.full(16, 3), 3, 16) == [(2 * g, 2 * g + 2) for g in range(8)]
    # a sample that outweighs several shares leaves the waves whose boundaries fall inside it without samples
    part = D.partition(np.array([2, 0, 100]), 100, 3)
    assert part[0] == (0, 3) and all(lo == hi == 3 for lo, hi in part[1:])


@pytest.mark.parametrize("name", D.NAMES)
def test_partition_covers_the_batch_once(name):
    c = D.case(name)
    hl, T, B = _geo(c)
    part = D.partition(hl, T, B)
    assert len(part) == D.launch(B)[1] and part[0][0] == 0 and part[-1][1] == B
    assert all(lo <= hi for lo, hi in part) and all(a[1] == b[0] for a, b in zip(part, part[1:]))
    bl = D.blocks(hl, T, B)
    assert sum(b.ns for b in bl) == B and sum(b.rows for b in bl) == int(D.clamped(hl, T, B).sum())
    assert sum(D.pass_rows(hl, T, B)) == sum(b.rows for b in bl)
    assert D.covers(D.K, T, c.H1, c.H2) == (name not in D.BEYOND) and D.long_covers(D.K, T, c.H1, c.H2) == (name in D.BEYOND)
    assert c.hist.min() >= -1 and c.hist.max() < D.V and c.cand.min() >= -1 and c.cand.max() < D.V


def test_act_shapes_reach_padded_widths_both_pass_bodies_and_the_small_batches():
    cs = [D.case(n) for n in D.NAMES if n.startswith("act_shapes")]
    assert len(cs) == len(D.ACT_SHAPES) == 12 and all(c.combos == D.PAPER for c in cs)
    assert {(c.H1, c.H2) for c in cs} >= {(80, 40), (16, 4), (48, 48), (72, 36), (4, 4), (80, 48)}
    one_tile = {c.name for c in cs if any(0 < r <= 16 for r in D.pass_rows(*_geo(c)))}          # dp_mlp<1, ACT>
    two_tile = {c.name for c in cs if any(r > 16 for r in D.pass_rows(*_geo(c)))}               # dp_mlp<2, ACT>
    assert {"act_shapes-2x7-80-40-uniform", "act_shapes-9x1-80-40-uniform", "act_shapes-1x1-4-4-uniform"} <= one_tile - two_tile
    assert "act_shapes-1x50-80-40-full" in two_tile and "act_shapes-40x33-16-4-uniform" in one_tile & two_tile
    assert {c.hist.shape for c in cs} >= {(1, 50), (1, 1), (9, 1)}
    assert all(r == 0 for r in D.pass_rows(*_geo(D.case("act_shapes-64x50-80-40-all_empty"))))
    assert all(r == 32 for r in D.pass_rows(*_geo(D.case("act_shapes-96x50-80-40-multiples"))))  # the last pass ends at the block's end
    runs = D.case("act_shapes-1500x50-80-40-empty_runs")
    assert any(b.rows == 0 and b.ns > 1 for b in D.blocks(*_geo(runs))) and not runs.hist_len[:21].any() and not runs.hist_len[-19:].any()
    for c in cs:                                              # alphas of both signs, Dice's scale and shift in their ranges
        for ap, H in ((c.act_params[:3 * c.H1], c.H1), (c.act_params[3 * c.H1:], c.H2)):
            a, s = ap[:H], ap[H:2 * H]
            assert a.min() >= -0.2 and a.max() <= 0.6 and s.min() >= 0.3 and s.max() <= 3.0
    assert min(float(c.act_params[:c.H1].min()) for c in cs) < 0


def test_no_candidate_has_a_block_without_candidates_and_a_part_block():
    small, tiny = D.case("no_candidate-40x20"), D.case("no_candidate-3x20")
    assert small.hist.shape == (40, 20) and tiny.hist.shape == (3, 20)
    assert sorted(np.flatnonzero(small.cand < 0)) == sorted(D.NO_CAND) == [0] + list(range(15, 33)) + [39]
    lens = small.hist_len[small.cand < 0]
    assert (lens == 0).any() and (lens == 20).any()           # some of them empty, some full
    assert max(b.ns for b in D.blocks(*_geo(small))) < 16     # (B = 40, T = 20: no wave holds a whole block)
    # a candidate is missing on the first lane of a block, on a block's last sample, and beside the idle lanes of a short block
    firsts = {b.sb for b in D.blocks(*_geo(small))}
    lasts = {b.sb + b.ns - 1 for b in D.blocks(*_geo(small))}
    miss = set(np.flatnonzero(small.cand < 0).tolist())
    assert firsts & miss and lasts & miss
    dense = D.case("no_candidate-40-dense")
    assert sorted(np.flatnonzero(dense.cand < 0)) == sorted(D.NO_CAND)
    bl = [b for b in D.blocks(*_geo(dense)) if b.wave == 0]
    assert [(b.sb, b.ns) for b in bl] == [(0, 16), (16, 16), (32, 3)]
    assert (dense.cand[16:32] < 0).all() and bl[1].rows > 16                                   # a whole block without candidates, with rows
    assert dense.cand[0] < 0 and dense.cand[15] < 0 and (dense.cand[1:15] >= 0).all()          # first and last lane of a block
    assert dense.cand[32] < 0 and bl[2].ns < 16 and bl[2].passes > 40                          # beside 13 idle lanes, in a block of many passes
    assert dense.cand[39] < 0 and dense.hist_len[39] == dense.T
    dl = dense.hist_len[dense.cand < 0]
    assert (dl == 0).any() and (dl > 0).any()
    three = D.case("no_candidate-3-dense")
    assert [(b.sb, b.ns) for b in D.blocks(*_geo(three))] == [(0, 3)]                          # one wave, one block of three: 13 idle lanes
    assert list(three.cand < 0) == [True, True, False] and list(three.hist_len) == [2, 0, 100]


def test_past_one_chunk_size_has_a_live_carry():
    c = D.case("past_one_chunk_size")
    hl, T, B = _geo(c)
    chunk, nchunk = D.chunks(B)
    assert B == 65536 + 200 and T == 2 and chunk >= 128 and nchunk == 514 and B % chunk != 0      # the last chunk is a part chunk
    late = D.boundaries_in_second_half_of_a_chunk(hl, T, B)
    assert len(late) > 500                                    # about half of the 2048 ranges start on first_at's second trip
    assert set(np.unique(hl)) == {0, 1, 2}
    assert max(b.ns for b in D.blocks(hl, T, B)) == 16 and any(b.ns < 16 and b.sb + b.ns < B for b in D.blocks(hl, T, B))


@pytest.mark.parametrize("form", ["small", "dense"])
def test_lengths_out_of_range_sit_on_both_sides_of_a_block_edge(form):
    c, none = D.case("lengths_out_of_range-" + form), D.case("lengths_out_of_range-%s-none" % form)
    hl, T, B = _geo(c)
    assert B == 70 and none.hist_len is None and np.array_equal(none.hist, c.hist) and np.array_equal(none.cand, c.cand)
    assert {-1, D.I32_MIN, T + 1, D.I32_MAX, 0} <= set(hl.tolist())
    bad = (hl < 0) | (hl > T)
    assert bad[0] and bad[B - 1]                              # the first and the last sample
    edges = [b.sb for b in D.blocks(hl, T, B) if 0 < b.sb]
    both = [e for e in edges if bad[e - 1] and bad[e]]
    assert both, "no block edge with an out-of-range length on either side"
    if form == "small":
        assert T == 9 and len(both) >= 2
    else:                                                     # edges INSIDE a wave's range: the next block's lengths come from the cursor's look-ahead
        inside = [b.sb for b in D.blocks(hl, T, B) if b.wave == 0 and b.sb > 0]
        assert inside[:3] == [16, 32, 48] and all(e in both for e in inside[:3])
        assert hl[69] == D.I32_MAX and hl[67] == D.I32_MAX and hl[66] == T + 1
    # both signs of the violation on a sample whose neighbour ends a block
    assert (hl[bad] < 0).any() and (hl[bad] > T).any()


def test_all_masked_has_a_pass_of_masked_rows_and_lone_valid_rows():
    c = D.case("all_masked")
    hl, T, B = _geo(c)
    assert (B, T) == (50, 40)
    valid = D.valid_mask(c)
    dead = np.flatnonzero((hl > 0) & ~valid.any(1))
    assert len(dead) >= 5 and 0 in dead and B - 1 in dead and {1, 16, 33, 40} <= set(hl[dead].tolist())
    assert list(np.flatnonzero(valid[3])) == [0] and list(np.flatnonzero(valid[12])) == [T - 1]
    assert D.masked_passes(c) >= 1                             # 32 masked rows that are one pass ...
    behind = [b for b in (16, 17, 30, 31) if not valid[b, :32].any() and valid[b, 32:].all()]
    assert len(behind) == 4                                    # ... of a sample with valid rows behind them
    starts = {blk.sb for blk in D.blocks(hl, T, B)}
    assert starts & set(behind)
    # the sample valid at its last position only ends its block: its row is the last row of the block's last pass
    blk = [b for b in D.blocks(hl, T, B) if b.sb <= 12 < b.sb + b.ns][0]
    assert blk.sb + blk.ns - 1 == 12 and blk.ns > 1 and blk.rows % D.PASS != 0


def test_long_history_runs_the_position_field_to_its_top_bit():
    full, sparse, beyond = (D.case("long_history-" + f) for f in ("full", "sparse", "beyond"))
    assert full.hist.shape == sparse.hist.shape == (3, 65535) and beyond.hist.shape == (2, 65536)
    for c in (full, sparse):
        bl = D.blocks(*_geo(c))
        # a block is ONE sample here (see the module's text): 2048 passes, not the 2^15 of a block of 16 such samples
        assert [b.ns for b in bl] == [1, 1, 1] and max(b.passes for b in bl) == 2048 and max(b.rows for b in bl) == 65535
        assert len({b.wave for b in bl}) == 3
    assert (full.hist >= 0).all() and full.combos == (("sigmoid", True), ("dice", True))
    for c in (sparse, beyond):
        T = c.T
        v = D.valid_mask(c)
        n = v.sum(1)
        assert (n >= 10).all() and (n <= 13).all()
        for j in D.LONG_KEPT + (32767, 32768):                 # positions 0, 31, 32 (a pass edge), 2^15 - 1, 2^15 (the field's top bit), 65 533, 65 534
            assert all(v[b, j] for b in range(len(v)) if j < c.hist_len[b])
        assert {a for a, _ in c.combos} == {"sigmoid", "dice"} and {z for _, z in c.combos} == {False, True}
    assert sparse.hist_len[1] == 65534 and sparse.hist[1, 65534] >= 0      # a kept id beyond the length stays out
    assert D.valid_mask(beyond)[:, 65535].all()
    # the widest history the 20-bit field holds: one sample, one block of 2^15 passes, valid rows on both sides of the 16-bit line and at the end
    widest = D.case("long_history-widest")
    assert widest.hist.shape == (1, 1 << 20) and D.long_covers(D.K, widest.T, 80, 40) and not D.long_covers(D.K, widest.T + 1, 80, 40)
    assert not D.long_covers(D.K, 65535, 80, 40) and D.long_covers(D.K, 65536, 80, 40) and not D.long_covers(32, 65536, 80, 40)
    assert [(b.ns, b.passes) for b in D.blocks(*_geo(widest))] == [(1, 1 << 15)]
    vw = D.valid_mask(widest)[0]
    assert all(vw[j] for j in (0, 65535, 65536, 1 << 19, (1 << 20) - 2, (1 << 20) - 1)) and 10 <= vw.sum() <= 14


def test_null_image_case():
    c = D.case("null_image")
    assert c.hist.shape == (257, 30) and c.combos == D.PAPER and (c.cand < 0).any()


# ---- the edges move the answer: a kernel that mishandles one cannot pass for one that does not ----------------------------------------------
def _f64(c, normalize, activation, **repl):
    c = c._replace(**repl)
    return R.din_attention_pool(c.table, D.ids(c, normalize), D.ref_len(c), c.cand, *c.unit, normalize=normalize, activation=activation,
                                act_params=c.act_params)


@pytest.mark.parametrize("activation,normalize", D.ALL)
@pytest.mark.parametrize("form", ["40x20", "40-dense", "3-dense"])
def test_a_missing_candidate_read_as_a_row_moves_the_scores(form, activation, normalize):
    """cand = -1 read as table row 0, or as the neighbouring sample's candidate: the scores of the samples concerned move by more than a
    hundred times the bar (normalize: ten times, a weight being a fraction of 1)."""
    c = D.case("no_candidate-" + form)
    _, s = _f64(c, normalize, activation)
    miss = np.flatnonzero(c.cand < 0)
    rows = D.valid_mask(c, normalize)[miss].any(1)
    assert rows.sum() >= (1 if form == "3-dense" else 2)
    for wrong in (np.where(c.cand < 0, 0, c.cand), np.where(c.cand < 0, np.roll(c.cand, 1).clip(0), c.cand)):
        _, s2 = _f64(c, normalize, activation, cand=wrong)
        moved = np.abs(s2 - s)[miss][rows].max(1) / (1 + np.abs(s[miss][rows]).max(1))
        assert (moved > (10 if normalize else 100) * D.BAR).sum() >= max(1, rows.sum() // 2), moved


@pytest.mark.parametrize("form", ["small", "dense"])
def test_a_length_read_unclamped_moves_the_pooled_rows(form):
    """A negative length read as its magnitude or as T, or one above T read as 0: the pooled rows of those samples move from / to zero by
    more than a hundred times the bar."""
    c = D.case("lengths_out_of_range-" + form)
    hl, T = c.hist_len.astype(np.int64), c.T
    o, _ = _f64(c, False, "dice")
    neg, big = hl < 0, hl > T
    assert not o[neg].any() and (np.abs(o[big]).max(1) > 100 * D.BAR).all()
    as_T, _ = _f64(c, False, "dice", hist_len=np.where(neg, T, hl).clip(-1, T).astype(np.int32))
    assert (np.abs(as_T[neg]).max(1) > 100 * D.BAR).all()


# ---- conditioning: fp32 against float64 on every case's operands, in the GPU tests' norm --------------------------------------------------
STRIDE = {"past_one_chunk_size": 97, "act_shapes-4099x50-80-40-uniform": 9, "act_shapes-1500x50-80-40-empty_runs": 3, "long_history-full": 3}


@pytest.mark.parametrize("name,activation,normalize", D.grid(D.NAMES))
def test_fp32_leaves_room_under_the_bar(name, activation, normalize):
    c = D.case(name)
    if name in STRIDE:                                         # the restatement is a per-sample Python loop: a subsample of the big cases
        c = D.subsample(c, STRIDE[name])
    args = (c.table, D.ids(c, normalize), D.ref_len(c), c.cand) + c.unit
    kw = dict(normalize=normalize, activation=activation, act_params=c.act_params)
    o64, s64 = R.din_attention_pool(*args, dtype=np.float64, **kw)
    o32, s32 = R.din_attention_pool(*args, dtype=np.float32, **kw)
    eo, es = D.scaled(o32, o64), D.scaled(s32, s64)
    print("%s %s normalize=%d: fp32 room out %.2e scores %.2e" % (name, activation, normalize, eo, es))
    assert eo <= D.ROOM and es <= D.ROOM, "fp32 on these operands is %.2e / %.2e off float64: no room under %.0e" % (eo, es, D.BAR)
