"""The NumPy stand-in for the scatter-sum WITH A SIDE SUM of dir_amd.shard's de-duplicated training lookup with a first-order term
(ShardedTables.lookup_train(ids, with_linear=True, dedup=True)): tests/shard_standin_din.py's backend plus rows_scatter_sum_side, reading
and writing what the HIP entry does (include/dir_hip.h: dir_rows_scatter_sum_side_f32).  Both outputs are DEFINED through the existing
stand-in, which pins the kernel's arithmetic to it: out = scatter_sum(idx, vals, R), out_side = scatter_sum over the side rows expanded to
one per entry (entry i reads side row i // side_div) -- the same stable order, tile cuts, compensated pieces and combine in double."""
import numpy as np
import torch

from tests.shard_standin_din import NumpyDinBackend, scatter_sum


def scatter_sum_side(idx, vals, side, side_div, R):
    """-> (out [R, K], out_side [R, U], the longest run) of idx [n], vals [n, K], side [>= ceil(n / side_div), U]."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    n = idx.size
    side = np.asarray(side, np.float32)
    out, longest = scatter_sum(idx, vals, R)
    out_side, _ = scatter_sum(idx, np.repeat(side, int(side_div), 0)[:n], R)
    return out, out_side, longest


class NumpyDedupLinearBackend(NumpyDinBackend):
    """+ rows_scatter_sum_side; counts its calls that had entries (side_calls), the empty ones apart (side_calls_empty), and the calls of
    the one-writer-per-position linear_grad, which the fixed path of a de-duplicated lookup must not make (the tests read all three)."""
    side_calls = 0
    side_calls_empty = 0
    linear_grad_calls = 0

    def rows_scatter_sum_side(self, idx, vals, side, side_div, R, out, out_side):
        n = idx.numel()
        res, res_side, longest = scatter_sum_side(idx.detach().numpy(), vals.detach().numpy().reshape(n, out.shape[1]),
                                                  side.detach().numpy().reshape(-1, out_side.shape[1]), side_div, int(R))
        if n:
            self.side_calls += 1
        else:
            self.side_calls_empty += 1
        self.longest_run = max(self.longest_run, longest)
        out.copy_(torch.from_numpy(res))
        out_side.copy_(torch.from_numpy(res_side))

    def linear_grad(self, g, inv2d, send):
        self.linear_grad_calls += 1
        return super().linear_grad(g, inv2d, send)
