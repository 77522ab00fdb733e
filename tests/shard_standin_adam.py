"""The NumPy stand-in for the owner-side sparse Adam of dir_amd.shard (ShardedTables.enable_training_adam): tests/shard_standin.py's
NumpyBackend plus make_adam / adam_norm / adam_apply, reading and writing what the HIP entries do (include/dir_hip.h:
dir_sparse_adam_payload_norm_f32 / dir_sparse_adam_payload_apply_f32).  m and v are float64; var lives in the shard's fp32 tensors; the
norm shares are the kernel's two words per table with the carry taken: N = sum over the touched rows of floor(||S_r||^2 * 2^32) handed over
as int64 [2, F], row 0 = N mod 2^32 (the low word), row 1 = N div 2^32 (the high word)."""
import numpy as np
import torch

from tests.shard_standin import NumpyBackend

FX = 1 << 32


class AdamState:
    """What ShardedTables.optimizer is under the stand-in: the hyper-parameters, .lr_t (set by the caller before every backward, as on
    ops.SparseAdam) and this rank's float64 moments."""

    def __init__(self, local, beta1, beta2, eps, clip_norm):
        self.beta1, self.beta2, self.eps, self.clip_norm = beta1, beta2, eps, clip_norm
        self.lr_t = 0.0
        self.ms = [np.zeros(tuple(t.shape), np.float64) for t in local]
        self.vs = [np.zeros(tuple(t.shape), np.float64) for t in local]
        self.norm_calls, self.apply_calls, self.empty_applies = 0, 0, 0


class NumpyAdamBackend(NumpyBackend):
    def make_adam(self, beta1, beta2, eps, clip_norm):
        return AdamState(self.local, beta1, beta2, eps, clip_norm)

    def _row_sums(self, payload, grad_rows):
        """Per table: the summed gradient of every local row (float64 [rows, K]) and which rows the payload touched.  Words < 0 and rows
        outside the slot's local rows carry nothing."""
        p, g = payload.numpy(), grad_rows.numpy().astype(np.float64)
        out = []
        for f in range(self.F):
            rows_f = self.local[f].shape[0]
            sel = (p >= 0) & (p % self.F == f) & (p // self.F < rows_f)
            gsum = np.zeros(tuple(self.local[f].shape))
            np.add.at(gsum, p[sel] // self.F, g[sel])
            out.append((gsum, np.unique(p[sel] // self.F)))
        return out

    def adam_norm(self, opt, payload, grad_rows):
        opt.norm_calls += 1
        words = []
        for gsum, rows in self._row_sums(payload, grad_rows):
            total = sum(int(np.floor(float((gsum[r] * gsum[r]).sum()) * FX)) for r in rows)
            words.append((total % FX, total // FX))
        return torch.tensor(words, dtype=torch.int64).t().contiguous()

    def adam_apply(self, opt, payload, grad_rows, norm2_global):
        opt.apply_calls += 1
        opt.empty_applies += int(not bool((payload >= 0).any()))
        assert (norm2_global is None) == (opt.clip_norm == 0)
        # the hyper-parameters as the fp32 kernels see them (oracle.np_ref.sparse_adam_step)
        lr_t = float(np.float32(opt.lr_t))
        omb1, omb2 = float(np.float32(1) - np.float32(opt.beta1)), float(np.float32(1) - np.float32(opt.beta2))
        b1, b2, eps, clip = (float(np.float32(x)) for x in (opt.beta1, opt.beta2, opt.eps, opt.clip_norm))
        for f, (g, _) in enumerate(self._row_sums(payload, grad_rows)):
            if clip > 0:
                g = g * clip / max(np.sqrt(float(norm2_global[f])), clip)               # the GLOBAL norm of table f's gradient
            m, v = opt.ms[f], opt.vs[f]
            m[:] = m * b1 + g * omb1                                                    # every local row moves, touched or not
            v[:] = v * b2 + g * g * omb2
            w = self.local[f].numpy().astype(np.float64) - lr_t * m / (np.sqrt(v) + eps)
            self.local[f].copy_(torch.from_numpy(w.astype(np.float32)))
