"""NumPy stand-ins of the backend methods that row groups and units > 1 add to dir_amd.shard.HipBackend (finish_groups, grad_groups, the
four *_units steps of the first-order term), on top of tests/shard_standin.NumpyBackend -- whose routing, slabs, owner gather and Adagrad
are width-generic and are reused as they are with K = G * K.  Shared by tests/test_shard_groups_gloo.py (the CPU worlds) and
tests/test_gpu_shard_groups.py (the gradient kernel's expected buffer)."""
import numpy as np
import torch

from tests.shard_standin import NumpyBackend


def finish_groups_np(back, inv2d, G, K):
    """back [n, G*K], inv2d [B, F] -> G arrays [B, F*K]: group g's piece of row inv2d[b, f], zeros where inv2d < 0."""
    B, F = inv2d.shape
    rows = np.where((inv2d >= 0)[:, :, None], back[np.maximum(inv2d, 0)], np.float32(0)).astype(np.float32)       # [B, F, G*K]
    return [np.ascontiguousarray(rows[:, :, g * K:(g + 1) * K]).reshape(B, F * K) for g in range(G)]


def grad_groups_np(grads, inv2d, K, n_send):
    """The transpose: G arrays [B, F*K] -> send [n_send, G*K], zero wherever no entry points."""
    B, F = inv2d.shape
    G = len(grads)
    send = np.zeros((n_send, G * K), np.float32)
    for b in range(B):
        for f in range(F):
            p = inv2d[b, f]
            if 0 <= p < n_send:
                for g in range(G):
                    send[p, g * K:(g + 1) * K] = grads[g][b, f * K:(f + 1) * K]
    return send


class NumpyGroupsBackend(NumpyBackend):
    """NumpyBackend over tables of G*K-float rows (local[f] is [local rows, G*K]) and first-order rows of U units."""

    def __init__(self, local, vocab, parts, first, P, K, G=1):
        super().__init__(local, vocab, parts, first, P, K * G)
        self.G, self.Kg = G, K
        self.units_calls = 0

    # ---- row groups ----
    def finish_groups(self, back, inv2d, K, outs):
        for o, v in zip(outs, finish_groups_np(back.numpy(), inv2d.numpy(), len(outs), K)):
            o.copy_(torch.from_numpy(v))

    def grad_groups(self, grads, inv2d, K, send):
        send.copy_(torch.from_numpy(grad_groups_np([g.detach().numpy() for g in grads], inv2d.numpy(), K, send.shape[0])))

    def accums(self, opt):
        return [torch.from_numpy(a) for a in opt["acc"]]

    # ---- units > 1 ----
    def _unit_weights_of(self, p, U):
        """U weights per payload word (0.0 for p < 0 and for rows outside the slot's local rows)."""
        out = np.zeros((p.size, U), np.float32)
        for i, v in enumerate(p):
            if v >= 0 and v // self.F < self.lin[v % self.F].shape[0]:
                out[i] = self.lin[v % self.F].numpy()[v // self.F, 0::4]
        return out

    def linear_gather_units(self, recv, cap, out):
        U = self.lin[0].shape[1] // 4
        o = out.numpy()
        if cap is None:
            o[:recv.numel() * U] = self._unit_weights_of(recv.numpy(), U).reshape(-1)
            return
        r = recv.numpy().reshape(self.P, cap + 1)
        o[:self.P * cap * U] = 0.0                     # every word is written
        for s in range(self.P):
            nv = int(r[s, 0] & 0xffffffff)
            o[s * cap * U:(s * cap + nv) * U] = self._unit_weights_of(r[s, 1:1 + nv], U).reshape(-1)

    def linear_finish_units(self, wback, inv2d, U, bias, out):
        iv, wb = inv2d.numpy(), wback.numpy().reshape(-1, U)
        acc = np.zeros((iv.shape[0], U), np.float32)
        for f in range(iv.shape[1]):                   # float32, slot order, per unit: dir_linear_onehot_rows_f32's sum
            acc = acc + np.where((iv[:, f] >= 0)[:, None], wb[np.maximum(iv[:, f], 0)], np.float32(0)).astype(np.float32)
        if bias is not None:
            acc = acc + bias.numpy().reshape(1, U).astype(np.float32)
        else:
            acc = acc + np.float32(0)
        out.copy_(torch.from_numpy(acc.astype(np.float32)))

    def linear_grad_units(self, g, inv2d, U, send):
        iv, gg, sd = inv2d.numpy(), g.detach().numpy().reshape(-1, U), send.numpy().reshape(-1, U)
        sd[:] = 0.0
        for b in range(iv.shape[0]):
            for f in range(iv.shape[1]):
                if iv[b, f] >= 0:
                    sd[iv[b, f]] = gg[b]

    def apply_ftrl_units(self, payload, grad, lr, l1, l2, sorted_by=None):
        self.units_calls += 1
        U = self.lin[0].shape[1] // 4
        p, g = payload.numpy(), grad.numpy().astype(np.float64).reshape(-1, U)
        assert g.shape[0] == p.size
        for f in range(self.F):
            sel = (p >= 0) & (p % self.F == f)
            rows = p[sel] // self.F
            r = self.lin[f].numpy()
            gs = np.zeros((r.shape[0], U))
            np.add.at(gs, rows, g[sel])                # ALL duplicates of a row are summed before n, z and w move
            t = np.zeros(r.shape[0], bool)
            t[rows] = True
            for u in range(U):
                c = 4 * u
                r[t, c], r[t, c + 1], r[t, c + 2] = self._ftrl(*(r[t, c + k].astype(np.float64) for k in range(3)), gs[t, u], lr, l1, l2)
