"""The NumPy stand-in for the requester-side scatter-sum of dir_amd.shard's de-duplicated training lookup (ShardedTables.lookup_train(dedup=True),
lookup_rows_train): tests/shard_standin_adam.py's backend plus rows_scatter_sum, reading and writing what the HIP entry does
(include/dir_hip.h: dir_rows_scatter_sum_f32).  The same stable order -- (idx, i) pairs, entries that name no row behind every row -- and the
kernels' arithmetic: a run is cut where its sorted position crosses a multiple of 256 (tests/hot_rows_inputs.py: tiled_sum's cuts), each
piece is summed by hot_rows_inputs.kahan_sum in fp32, the pieces are added in float64 and rounded once."""
import numpy as np
import torch

from tests.hot_rows_inputs import TILE, kahan_sum
from tests.shard_standin_adam import NumpyAdamBackend


def scatter_sum(idx, vals, R):
    """out [R, K] fp32 of idx [n] int64, vals [n, K] fp32; -> (out, the longest run)."""
    idx, vals = np.asarray(idx, np.int64), np.asarray(vals, np.float32)
    out = np.zeros((R, vals.shape[1]), np.float32)
    key = np.where((idx >= 0) & (idx < R), idx, R)
    order = np.argsort(key, kind="stable")                # stable: a row's entries stay in ascending entry order
    ks = key[order]
    n = int(np.searchsorted(ks, R))                       # the live entries
    starts = np.flatnonzero(np.concatenate([[True], ks[1:n] != ks[:n - 1]])) if n else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [n]]).astype(np.int64)
    longest = 0
    for s, e in zip(starts, ends):
        rows = vals[order[s:e]]
        longest = max(longest, int(e - s))
        if e - s == 1:
            out[ks[s]] = rows[0]                          # a run of one: bit for bit
            continue
        cuts = [0] + list(range(TILE - s % TILE, e - s, TILE)) + [int(e - s)]
        parts = [kahan_sum(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        wide = parts[0].astype(np.float64)
        for p in parts[1:]:                               # in tile order, in double, rounded once
            wide = wide + p.astype(np.float64)
        out[ks[s]] = parts[0] if len(parts) == 1 else wide.astype(np.float32)
    return out, longest


class NumpyDinBackend(NumpyAdamBackend):
    """+ rows_scatter_sum; counts its calls and remembers the longest run it has summed (the tests read both)."""
    scatter_calls = 0
    longest_run = 0

    def rows_scatter_sum(self, idx, vals, R, out):
        res, longest = scatter_sum(idx.detach().numpy().reshape(-1), vals.detach().numpy().reshape(idx.numel(), out.shape[1]), int(R))
        self.scatter_calls += 1
        self.longest_run = max(self.longest_run, longest)
        out.copy_(torch.from_numpy(res))
