"""dir_rows_scatter_sum_side_f32 (csrc/rows_scatter.hip; ops.rows_scatter_sum_side) on the GPU: the sorted scatter-sum of rows with a
SIDE sum on the same sort -- out_side[r] = sum of side[i // side_div] over the entries of row r.

Held to, per case: `out` bitwise ops.rows_scatter_sum on the same input; `out_side` bitwise ops.rows_scatter_sum over the side rows
expanded to one per entry; both bitwise the NumPy stand-in (tests/shard_standin_dedup_linear.scatter_sum_side); both within
tests/hot_rows_inputs.BAR (1e-5, scaled) of the float64 sums; two calls equal in bits; rows nobody names zero; the guard words behind
`out`, `out_side` and a workspace of exactly dir_rows_scatter_sum_side_workspace_bytes intact; a HIP-graph replay equal to the eager call.

Shapes, the smallest at which the kernel can go wrong: K in {4 (one lane per run: it takes every unit), 6 (scalar, a padded group of 8
lanes), 16 (float4s, 4 lanes, none idle), 64, 256 (a whole wave per run)} x U in {1, 2, 4} x side_div in {1, 3, 26}; ld > K and
side_ld > U once each.  One entry list of 9 079 entries (36 sort tiles) over R = 40 rows: runs of 1, 255, 256, 257 and 3000 entries that end
one before, on and one after a 256-entry tile edge (RUNS below gives every run's sorted span), two runs of 3000 -- one from a tile start,
one from mid-tile, each over more than 11 tiles, so the carry of both sums is combined in double -- a row without entries between the
runs, -1, R and R + 5 mixed in, the last entry live (its sample is the last side row).  R = 1 000 003 once: nearly every run is one entry.
n = 0: both outputs zero-filled."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.hot_rows_inputs import BAR, TILE, scaled
from tests.shard_loopback import Guards
from tests.shard_standin_dedup_linear import scatter_sum_side

pytestmark = pytest.mark.gpu
R = 40
# (row, entries), in key order: the run of row r occupies the sorted positions [sum of the counts before it, + its count)
RUNS = ((5, 255),      # [0, 255): ends one before the edge 256
        (6, 1),        # [255, 256): a run of one that ends ON an edge
        (7, 257),      # [256, 513): starts on an edge, ends one after 512
        (8, 255),      # [513, 768): ends on 768
        (9, 256),      # [768, 1024): a whole tile
        (10, 1),       # [1024, 1025): a run of one right after an edge
        (11, 3000),    # [1025, 4025): from mid-tile over 12 tiles
        (12, 70),      # [4025, 4095): ends one before 4096
        (13, 1),       # [4095, 4096): ends on the edge
        (14, 3000),    # [4096, 7096): from a tile start over 12 tiles
        (15, 73),      # [7096, 7169): ends one after 7168
        (16, 256),     # [7169, 7425): 256 entries across an edge, ends one after 7424
        (17, 257),     # [7425, 7682)
        (19, 1277),    # [7682, 8959): ends one before 8960 (row 18 has no entry)
        (20, 1),       # [8959, 8960): ends on the edge
        (21, 1), (22, 30), (25, 7), (33, 22), (34, 40))     # rows 0..4, 18, 23, 24, 26..32 and 35..39 have no entry
DROPPED = (-1,) * 9 + (R,) * 7 + (R + 5,) * 3
U_S, DIV_S = (1, 2, 4), (1, 3, 26)


@functools.lru_cache(maxsize=None)
def entries():
    rng = np.random.default_rng(11)
    live = np.concatenate([np.full(c, r) for r, c in RUNS])
    idx = np.concatenate([live, np.array(DROPPED)]).astype(np.int64)
    rng.shuffle(idx)
    last = int(np.flatnonzero((idx >= 0) & (idx < R))[-1])
    idx[[last, -1]] = idx[[-1, last]]                      # the last entry is live: its sample is the last side row
    ends = np.cumsum([c for _, c in RUNS])
    assert {int(e % TILE) for e in ends} >= {TILE - 1, 0, 1} and idx.size > 35 * TILE and 0 <= idx[-1] < R
    return idx


@functools.lru_cache(maxsize=None)
def vals_of(K, ld):
    full = (np.random.default_rng(100 + K).standard_normal((entries().size, ld)) * 0.5).astype(np.float32)
    full[:, K:] = np.nan                                   # the pad columns are never read
    return full


@functools.lru_cache(maxsize=None)
def side_of(U, div, ld):
    rows = -(-entries().size // div)                       # exactly ceil(n / side_div) rows: entry n - 1 reads the last one
    full = (np.random.default_rng(200 + 10 * U + div).standard_normal((rows, ld)) * 0.5).astype(np.float32)
    full[:, U:] = np.nan
    return full


@functools.lru_cache(maxsize=None)
def reference(K, U, div):
    """The stand-in's two slabs and the float64 sums (computed once per shape; read-only)."""
    idx = entries()
    vals, side = vals_of(K, K)[:, :K], side_of(U, div, U)[:, :U]
    out, out_side, longest = scatter_sum_side(idx, vals, side, div, R)
    assert longest == 3000
    ok = (idx >= 0) & (idx < R)
    w, ws = np.zeros((R, K)), np.zeros((R, U))
    np.add.at(w, idx[ok], vals[ok].astype(np.float64))
    np.add.at(ws, idx[ok], side[np.arange(idx.size) // div][ok].astype(np.float64))
    for a in (out, out_side, w, ws):
        a.setflags(write=False)
    return out, out_side, w, ws


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded_call(lib, idx, vals, K, side, U, div, rows):
    """The C entry on guarded buffers: out and out_side pattern-filled with guard tails, the workspace exactly the size the query reports."""
    n = idx.numel()
    need = int(lib.dir_rows_scatter_sum_side_workspace_bytes(n, K, U, rows))
    assert need >= int(lib.dir_rows_scatter_sum_workspace_bytes(n, K, rows)) >= 0 and need % 4 == 0
    g = Guards("cuda")
    out = g.alloc("out", 0, (rows, K), torch.float32, 256)
    out_side = g.alloc("out_side", 0, (rows, U), torch.float32, 256)
    ws = g.alloc("workspace", 0, (max(need // 4, 1),), torch.int32, 256)
    assert ws.data_ptr() % 256 == 0
    rc = lib.dir_rows_scatter_sum_side_f32(_p(idx), _p(vals), vals.stride(0) if n > 1 else K, _p(side), side.stride(0) if side.shape[0] > 1 else U,
                                           div, n, K, U, rows, _p(out), _p(out_side), _p(ws), need, _stream())
    assert rc == 0, lib.dir_last_error()
    torch.cuda.synchronize()
    g.check("dir_rows_scatter_sum_side_f32 K=%d U=%d side_div=%d" % (K, U, div))
    return out, out_side


def _check(lib, K, U, div, ld, side_ld):
    from dir_amd import ops
    idx = entries()
    n = idx.size
    what = "K=%d ld=%d U=%d side_ld=%d side_div=%d" % (K, ld, U, side_ld, div)
    d_idx = torch.from_numpy(idx).cuda()
    d_vals = torch.from_numpy(vals_of(K, ld)).cuda()[:, :K]
    d_side = torch.from_numpy(side_of(U, div, side_ld)).cuda()[:, :U]
    out, out_side = _guarded_call(lib, d_idx, d_vals, K, d_side, U, div, R)
    again, again_side = ops.rows_scatter_sum_side(d_idx.clone(), d_vals, d_side, div, R)
    assert torch.equal(out, again) and torch.equal(out_side, again_side), "two calls differ: " + what
    assert torch.equal(out, ops.rows_scatter_sum(d_idx, d_vals, R)), "out differs from rows_scatter_sum's: " + what
    expanded = d_side.repeat_interleave(div, 0)[:n].contiguous()
    assert torch.equal(out_side, ops.rows_scatter_sum(d_idx, expanded, R)), "out_side differs from rows_scatter_sum over the expanded side: " + what
    got, got_side = out.cpu().numpy(), out_side.cpu().numpy()
    counts = np.bincount(idx[(idx >= 0) & (idx < R)], minlength=R)
    assert counts[18] == 0 and not got[counts == 0].any() and not got_side[counts == 0].any(), "rows nobody names must be zeros: " + what
    assert np.isfinite(got).all() and np.isfinite(got_side).all(), what
    if ld == K and side_ld == U:                           # (the padded forms hold other values in the same places: compared to the GPU's above)
        ref, ref_side, want, want_side = reference(K, U, div)
        assert np.array_equal(got, ref), "out and the NumPy stand-in differ in bits: %s (%.3e)" % (what, scaled(got, ref))
        assert np.array_equal(got_side, ref_side), "out_side and the NumPy stand-in differ in bits: %s (%.3e)" % (what, scaled(got_side, ref_side))
    else:
        ok = (idx >= 0) & (idx < R)
        want, want_side = np.zeros((R, K)), np.zeros((R, U))
        np.add.at(want, idx[ok], d_vals.cpu().numpy()[ok].astype(np.float64))
        np.add.at(want_side, idx[ok], expanded.cpu().numpy()[ok].astype(np.float64))
    err, err_side = scaled(got, want), scaled(got_side, want_side)
    print("rows_scatter_sum_side %s: scaled error out %.3e out_side %.3e" % (what, err, err_side))
    assert err <= BAR and err_side <= BAR, "%s: out %.3e, out_side %.3e off the float64 sums" % (what, err, err_side)


@pytest.mark.parametrize("K", [4, 6, 16, 64, 256])
def test_side_sum_every_unit_count_and_divisor(built_lib, K):
    for U in U_S:
        for div in DIV_S:
            _check(built_lib, K, U, div, K, U)


@pytest.mark.parametrize("K,ld,U,side_ld", [(16, 20, 2, 5), (6, 9, 1, 1), (4, 4, 4, 7)])
def test_padded_rows(built_lib, K, ld, U, side_ld):
    """ld > K (16-byte path: ld = K + 4; scalar path: ld = K + 3) and side_ld > U."""
    _check(built_lib, K, U, 3, ld, side_ld)


def test_runs_of_one_over_a_million_rows(built_lib):
    """R = 1 000 003, 9 000 entries drawn uniformly (dropped positions mixed in): nearly every run is a single entry, copied bit for bit."""
    from dir_amd import ops
    rows, n, K, U, div = 1_000_003, 9000, 16, 2, 26
    rng = np.random.default_rng(5)
    idx = rng.integers(-3, rows + 3, size=n).astype(np.int64)
    idx[:40] = idx[40:80]                                  # a few runs of two
    vals = (rng.standard_normal((n, K)) * 0.5).astype(np.float32)
    side = (rng.standard_normal((-(-n // div), U)) * 0.5).astype(np.float32)
    d_idx, d_vals, d_side = (torch.from_numpy(a).cuda() for a in (idx, vals, side))
    out, out_side = _guarded_call(built_lib, d_idx, d_vals, K, d_side, U, div, rows)
    assert torch.equal(out, ops.rows_scatter_sum(d_idx, d_vals, rows))
    expanded = d_side.repeat_interleave(div, 0)[:n].contiguous()
    assert torch.equal(out_side, ops.rows_scatter_sum(d_idx, expanded, rows))
    ok = (idx >= 0) & (idx < rows)
    want, want_side = np.zeros((rows, K)), np.zeros((rows, U))
    np.add.at(want, idx[ok], vals[ok].astype(np.float64))
    np.add.at(want_side, idx[ok], side[np.arange(n) // div][ok].astype(np.float64))
    got, got_side = out.cpu().numpy(), out_side.cpu().numpy()
    once = np.flatnonzero(np.bincount(idx[ok], minlength=rows) == 1)
    assert once.size > 8000 and np.array_equal(got[once], want[once].astype(np.float32)) and np.array_equal(got_side[once], want_side[once].astype(np.float32))
    assert scaled(got, want) <= BAR and scaled(got_side, want_side) <= BAR
    touched = np.zeros(rows, bool)
    touched[idx[ok]] = True
    assert not got[~touched].any() and not got_side[~touched].any()


def test_no_entries_zero_fills_both(built_lib):
    from dir_amd import ops
    idx = torch.empty(0, dtype=torch.int64, device="cuda")
    for K, U in ((4, 1), (6, 4), (16, 2)):
        vals, side = torch.empty((0, K), device="cuda"), torch.empty((0, U), device="cuda")
        out, out_side = _guarded_call(built_lib, idx, vals, K, side, U, 26, R)
        assert not out.any() and not out_side.any()
        o2 = torch.full((R, K), float("nan"), device="cuda")
        s2 = torch.full((R, U), float("nan"), device="cuda")
        ops.rows_scatter_sum_side(idx, vals, side, 26, R, out=o2, out_side=s2)
        assert not o2.any() and not s2.any()


def test_graph_replay_equals_eager(built_lib):
    """Captured after one eager call; replayed on new positions, rows and side rows written into the captured buffers."""
    from dir_amd import ops
    K, U, div = 16, 1, 26
    idx0 = entries()
    n = idx0.size
    d_idx = torch.from_numpy(idx0).cuda()
    d_vals = torch.from_numpy(vals_of(K, K)).cuda()
    d_side = torch.from_numpy(side_of(U, div, U)).cuda()
    out, out_side = torch.empty((R, K), device="cuda"), torch.empty((R, U), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.rows_scatter_sum_side(d_idx, d_vals, d_side, div, R, out=out, out_side=out_side)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.rows_scatter_sum_side(d_idx, d_vals, d_side, div, R, out=out, out_side=out_side)
    for r in range(2):
        rng = np.random.default_rng(50 + r)
        idx = idx0.copy()
        rng.shuffle(idx)
        d_idx.copy_(torch.from_numpy(idx).cuda())
        d_vals.copy_(torch.from_numpy((rng.standard_normal((n, K)) * 0.5).astype(np.float32)).cuda())
        d_side.copy_(torch.from_numpy((rng.standard_normal(tuple(d_side.shape)) * 0.5).astype(np.float32)).cuda())
        g.replay()
        eager, eager_side = ops.rows_scatter_sum_side(d_idx.clone(), d_vals.clone(), d_side.clone(), div, R)
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(out_side, eager_side), "replay %d differs from the eager call" % r


def test_argument_errors(built_lib):
    from dir_amd import _lib, ops
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    vals = torch.zeros((4, 8), device="cuda")
    with pytest.raises(ValueError):
        ops.rows_scatter_sum_side(idx, vals, torch.zeros((1, 1), device="cuda"), 3, 5)         # 1 side row x 3 < 4 entries
    with pytest.raises(ValueError):
        ops.rows_scatter_sum_side(idx, vals, torch.zeros((4, 5), device="cuda"), 1, 5)         # U = 5
    with pytest.raises(ValueError):
        ops.rows_scatter_sum_side(idx, vals, torch.zeros((4, 1), device="cuda"), 0, 5)         # side_div = 0
    with pytest.raises(_lib.DirError):
        ops.rows_scatter_sum_side(idx, torch.zeros((4, 300), device="cuda"), torch.zeros((4, 1), device="cuda"), 1, 5)
