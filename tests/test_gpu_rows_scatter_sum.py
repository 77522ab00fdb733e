"""dir_rows_scatter_sum_f32 (csrc/rows_scatter.hip; ops.rows_scatter_sum) on the GPU: sparse rows summed into a dense slab.

Comparand: the float64 sum of every row's entries.  Bar: tests/hot_rows_inputs.scaled <= 1e-5, the bar tests/test_gpu_hot_rows.py holds
the sorted optimiser steps' run sums to (the kernel sums through the same run_sum).  Beside it: a position named once holds its entry's
row bit for bit, rows nobody names are zeros, two calls are bitwise equal, the kernel equals the NumPy stand-in of the CPU tests
(tests/shard_standin_din.scatter_sum: the same stable order and arithmetic) bit for bit, and a HIP-graph replay equals the eager call.

Shapes: K in {4, 16, 64} with ld > K (16-byte path: ld = K + 4; scalar path: ld = K + 3); n in {0, 1, 300, 4096}; runs of 1, 255, 256, 257,
513 and 3000 entries whose ends fall one before, on and one after a 256-entry sort-tile edge, at the lowest and at the highest live key;
two adjacent hot rows that meet inside one tile; negative and too-large positions mixed in; untouched rows at both ends of the slab."""
import functools

import numpy as np
import pytest
import torch

from tests.hot_rows_inputs import BAR, TILE, scaled
from tests.shard_standin_din import scatter_sum

pytestmark = pytest.mark.gpu
R = 40                    # rows 0..4 and 35..39 are never named
LO, HI = 5, 34
RUNS = (1, 255, 256, 257, 513, 3000)
WORST = {}


@functools.lru_cache(maxsize=None)
def case(kind, L, end, seed):
    """-> idx [n] int64 (shuffled entry order, dropped positions mixed in).  kind "low": the run of L entries is the lowest live key (its
    run starts at sorted position 0); "high": the highest live key, with as many filler entries in front that the run ENDS at a multiple
    of 256 plus `end`; "pair": rows LO and LO + 1 with L and L + 100 entries (the first ends and the second starts inside one tile);
    "uniform": L entries drawn from [-2, R + 2)."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        idx = rng.integers(-2, R + 2, size=L)
        idx[(idx >= 0) & (idx < LO)] = LO
        idx[(idx > HI) & (idx < R)] = HI
        return idx.astype(np.int64)
    if kind == "pair":
        live = np.concatenate([np.full(L, LO), np.full(L + 100, LO + 1), rng.integers(LO + 2, HI + 1, size=57)])
    elif kind == "low":
        live = np.concatenate([np.full(L, LO), rng.integers(LO + 1, HI + 1, size=300 + (end % TILE))])
    else:
        fill = (end - L) % TILE + TILE                      # the run starts at sorted position `fill` and ends at fill + L = end (mod 256)
        live = np.concatenate([rng.integers(LO, HI, size=fill), np.full(L, HI)])
    idx = np.concatenate([live, np.full(9, -1), np.full(7, R), np.full(3, R + 5)])
    rng.shuffle(idx)
    return idx.astype(np.int64)


CASES = ([("uniform", n, 0) for n in (0, 1, 300, 4096)] + [("low", L, e) for L in RUNS for e in (0, 1)] +
         [("high", L, e) for L in RUNS for e in (-1, 0, 1)] + [("pair", 300, 0), ("pair", 200, 0)])


def _vals(n, K, ld, seed):
    rng = np.random.default_rng(seed + 7)
    full = (rng.standard_normal((n, ld)) * 0.5).astype(np.float32)
    full[:, K:] = np.nan                                     # the pad columns are never read
    return full


def _run(idx, full, K):
    from dir_amd import ops
    n = idx.size
    d_idx = torch.from_numpy(idx).cuda()
    d_full = torch.from_numpy(full).cuda()
    out = torch.full((R, K), float("nan"), device="cuda")
    ops.rows_scatter_sum(d_idx, d_full[:, :K] if n else d_full[:, :K].contiguous(), R, out=out)
    return out


@pytest.mark.parametrize("pad", [4, 3])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_scatter_sum_against_float64(built_lib, K, pad):
    worst = 0.0
    for ci, (kind, L, end) in enumerate(CASES):
        idx = case(kind, L, end, 100 + ci)
        n = idx.size
        full = _vals(n, K, K + pad, ci)
        got = _run(idx, full, K).cpu().numpy()
        again = _run(idx, full, K).cpu().numpy()
        what = "%s L=%d end=%d K=%d ld=%d" % (kind, L, end, K, K + pad)
        assert np.array_equal(got, again), "two calls differ: " + what
        vals = full[:, :K]
        ok = (idx >= 0) & (idx < R)
        want = np.zeros((R, K))
        np.add.at(want, idx[ok], vals[ok].astype(np.float64))
        counts = np.bincount(idx[ok], minlength=R)
        assert not got[counts == 0].any() and np.isfinite(got).all(), "rows nobody names must be zeros: " + what
        assert not counts[:LO].any() and not counts[HI + 1:].any()
        for r in np.flatnonzero(counts == 1):
            assert np.array_equal(got[r], vals[np.flatnonzero(idx == r)[0]]), "a run of one is a copy: row %d, %s" % (r, what)
        err = scaled(got, want)
        print("rows_scatter_sum %s: scaled error %.3e" % (what, err))
        assert err <= BAR, "%s: %.3e" % (what, err)
        worst = max(worst, err)
        ref, longest = scatter_sum(idx, vals, R)
        assert longest == (int(counts.max()) if n else 0)
        assert np.array_equal(got, ref), "the kernel and the NumPy stand-in differ in bits: %s (%.3e)" % (what, scaled(got, ref))
    print("rows_scatter_sum K=%d ld=K+%d: worst scaled error over %d cases %.3e" % (K, pad, len(CASES), worst))


def test_graph_replay_equals_eager(built_lib):
    """Captured after one eager call; replayed on new positions and rows written into the captured buffers."""
    from dir_amd import ops
    K, n = 64, 4096
    idx0 = case("high", 3000, 1, 5)
    n = idx0.size
    d_idx = torch.from_numpy(idx0).cuda()
    d_vals = torch.from_numpy(_vals(n, K, K, 1)).cuda()
    out = torch.empty((R, K), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.rows_scatter_sum(d_idx, d_vals, R, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.rows_scatter_sum(d_idx, d_vals, R, out=out)
    for r in range(3):
        rng = np.random.default_rng(50 + r)
        idx = idx0.copy()
        rng.shuffle(idx)
        d_idx.copy_(torch.from_numpy(idx).cuda())
        d_vals.copy_(torch.from_numpy(_vals(n, K, K, 20 + r)).cuda())
        g.replay()
        eager = ops.rows_scatter_sum(d_idx.clone(), d_vals.clone(), R)
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "replay %d differs from the eager call" % r


def test_argument_errors(built_lib):
    from dir_amd import _lib, ops
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.rows_scatter_sum(idx, torch.zeros((3, 8), device="cuda"), 5)
    with pytest.raises(_lib.DirError):
        ops.rows_scatter_sum(idx, torch.zeros((4, 300), device="cuda"), 5)            # wider than one wave covers
    lib = _lib.load()
    assert lib.dir_rows_scatter_sum_workspace_bytes(1 << 30, 8, 5) == -1 and lib.dir_rows_scatter_sum_workspace_bytes(4, 8, 1 << 32) == -1
    assert lib.dir_rows_scatter_sum_workspace_bytes(0, 8, 5) >= 0
