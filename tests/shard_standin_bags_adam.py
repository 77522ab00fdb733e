"""The NumPy stand-in for the owner-side sparse Adam over bag records (dir_amd.shard.ShardedTables.lookup_bags_train under
enable_training_adam): tests/shard_standin_adam.NumpyAdamBackend plus bags_adam_norm / bags_adam_apply, reading what the HIP entries
read (include/dir_hip.h: dir_sparse_adam_bags_norm_f32 / dir_sparse_adam_bags_apply_f32) -- the received slabs of 16-byte records,
decoded as tests/shard_standin.NumpyBackend.bags_adagrad decodes them, and the gradients of the partial rows.  A row's gradient is the
float64 sum of w * grad_rows[src * cap_b + ret] over all its records, through the slot's max_norm clip derivative at the row's current
value; m and v are float64 (AdamState), var lives in the shard's fp32 tensors; the norm share is the two fixed-point rows of
NumpyAdamBackend.adam_norm.  Also here, for the gloo test and the GPU test: the float64 reference of one such step on the FULL tables."""
import numpy as np
import torch

from tests.shard_standin import per_slot
from tests.shard_standin_adam import FX, NumpyAdamBackend


class NumpyBagsAdamBackend(NumpyAdamBackend):
    def _bag_row_grads(self, recv, cap_e, cap_b, grad_rows, max_norm):
        """Per table: (the gradient of every local row, float64 [rows, K], zero where no record points; the touched rows)."""
        F, P = self.F, self.P
        sl = recv.numpy().reshape(P, cap_e + 1, 2)
        gr = grad_rows.numpy().astype(np.float64)
        mn = per_slot(max_norm, F)
        ent = []
        for s in range(P):                                        # (NumpyBackend.bags_adagrad's decoding)
            ne = min(int(sl[s, 0, 0] & 0xffffffff), cap_e)
            rec = sl[s, 1:1 + ne]
            packed = rec[:, 0]
            ret = rec[:, 1] >> 32
            w = (rec[:, 1] & 0xffffffff).astype(np.uint32).view(np.float32).astype(np.float64)
            ok = (packed >= 0) & (ret >= 0) & (ret < cap_b)
            ent.append((packed[ok], ret[ok] + s * cap_b, w[ok]))
        packed, gidx, w = (np.concatenate([e[c] for e in ent]) for c in range(3))
        out = []
        for f in range(F):
            sel = (packed % F == f) & (packed // F < self.local[f].shape[0])
            rows_all = packed[sel] // F
            G = np.zeros(tuple(self.local[f].shape))
            np.add.at(G, rows_all, w[sel][:, None] * gr[gidx[sel]])   # ALL records of a row, of any bag and any rank, before anything moves
            rows = np.unique(rows_all)
            if mn[f] and len(rows):                                   # clip_by_norm's derivative at the pre-update row
                g = G[rows]
                r = self.local[f].numpy().astype(np.float64)[rows]
                n = np.sqrt((r * r).sum(1, keepdims=True))
                gc = mn[f] * (g / np.maximum(n, 1e-30) - r * ((r * g).sum(1, keepdims=True) / np.maximum(n, 1e-30) ** 3))
                G[rows] = np.where(n > mn[f], gc, g)
            out.append((G, rows))
        return out

    def bags_adam_norm(self, opt, recv, cap_e, cap_b, grad_rows, max_norm):
        opt.norm_calls += 1
        words = []
        for G, rows in self._bag_row_grads(recv, cap_e, cap_b, grad_rows, max_norm):
            total = sum(int(np.floor(float((G[r] * G[r]).sum()) * FX)) for r in rows)
            words.append((total % FX, total // FX))
        return torch.tensor(words, dtype=torch.int64).t().contiguous()

    def bags_adam_apply(self, opt, recv, cap_e, cap_b, grad_rows, max_norm, norm2_global):
        opt.apply_calls += 1
        sums = self._bag_row_grads(recv, cap_e, cap_b, grad_rows, max_norm)
        opt.empty_applies += int(not any(len(rows) for _, rows in sums))
        assert (norm2_global is None) == (opt.clip_norm == 0)
        # the hyper-parameters as the fp32 kernels see them (NumpyAdamBackend.adam_apply, oracle.np_ref.sparse_adam_step)
        lr_t = float(np.float32(opt.lr_t))
        omb1, omb2 = float(np.float32(1) - np.float32(opt.beta1)), float(np.float32(1) - np.float32(opt.beta2))
        b1, b2, eps, clip = (float(np.float32(x)) for x in (opt.beta1, opt.beta2, opt.eps, opt.clip_norm))
        for f, (g, _) in enumerate(sums):
            if clip > 0:
                g = g * clip / max(np.sqrt(float(norm2_global[f])), clip)               # the GLOBAL norm of table f's gradient
            m, v = opt.ms[f], opt.vs[f]
            m[:] = m * b1 + g * omb1                                                    # every local row moves, touched or not
            v[:] = v * b2 + g * g * omb2
            w = self.local[f].numpy().astype(np.float64) - lr_t * m / (np.sqrt(v) + eps)
            self.local[f].copy_(torch.from_numpy(w.astype(np.float32)))


class BagsAdamReference:
    """float64 torch autograd of tests.test_shard_bags_train_gloo.bags_forward64 over the FULL tables on the GLOBAL batch, then a float64
    dense Adam with the per-table clip_by_norm in which every row moves ([TF-upstream] AdamOptimizer on the IndexedSlices gradient; the
    hyper-parameters as the fp32 graph sees them, oracle.np_ref.sparse_adam_step)."""

    def __init__(self, full, lr, b1, b2, eps, clip):
        self.T = [np.asarray(t, np.float64).copy() for t in full]
        self.m = [np.zeros(t.shape) for t in full]
        self.v = [np.zeros(t.shape) for t in full]
        self.lr, self.b1, self.b2, self.eps, self.clip, self.t = lr, b1, b2, eps, clip, 0
        self.norms = []                       # per step: ||g|| of every table's gradient (unclipped)
        self.row_clipped = []                 # per step: (rows of a max_norm slot the lookup clipped, rows it left alone) among the touched

    def lr_t(self, t=None):
        t = self.t + 1 if t is None else t
        return self.lr * np.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)

    def grads(self, bags, G, combiner, max_norm, prune):
        from tests.test_shard_bags_train_gloo import bags_forward64
        T = [torch.from_numpy(t.copy()).requires_grad_(True) for t in self.T]
        emb = bags_forward64(T, bags, combiner, max_norm, prune)
        if len(bags) and emb.requires_grad:                       # (no live entry at all: the forward does not read the tables)
            (emb * torch.from_numpy(np.asarray(G, np.float64))).sum().backward()
        return [np.zeros_like(self.T[f]) if t.grad is None else t.grad.numpy() for f, t in enumerate(T)]

    def step_grads(self, gs):
        self.t += 1
        lr_t = float(np.float32(self.lr_t(self.t)))
        omb1, omb2 = float(np.float32(1) - np.float32(self.b1)), float(np.float32(1) - np.float32(self.b2))
        b1, b2, eps, clip = (float(np.float32(x)) for x in (self.b1, self.b2, self.eps, self.clip))
        self.norms.append([float(np.sqrt((g * g).sum())) for g in gs])
        for f, g in enumerate(gs):
            if clip > 0:
                g = g * clip / max(np.sqrt((g * g).sum()), clip)
            self.m[f][:] = self.m[f] * b1 + g * omb1
            self.v[f][:] = self.v[f] * b2 + g * g * omb2
            self.T[f][:] = self.T[f] - lr_t * self.m[f] / (np.sqrt(self.v[f]) + eps)

    def step(self, bags, G, combiner, max_norm, prune):
        F = len(self.T)
        mn = per_slot(max_norm, F)
        gs = self.grads(bags, G, combiner, max_norm, prune)
        cl, un = 0, 0
        for f in range(F):
            if mn[f]:
                touched = np.abs(gs[f]).sum(1) > 0
                nr = np.sqrt((self.T[f] * self.T[f]).sum(1))
                cl += int((touched & (nr > mn[f])).sum())
                un += int((touched & (nr <= mn[f])).sum())
        self.row_clipped.append((cl, un))
        self.step_grads(gs)

    def step_onehot(self, ids, G):
        """A one-hot lookup_train step between bag steps: sum-combined single-entry bags."""
        bags = [[(np.array([i]), None) for i in row] for row in ids]
        self.step(bags, G, "sum", None, False)
