"""NumPy stand-ins of the backend methods that row groups add to dir_amd.shard.HipBackend (finish_groups, grad_groups), on top of
tests/shard_standin.NumpyBackend -- whose routing, slabs, owner gather and Adagrad are width-generic and are reused as they are with
K = G * K, and whose first-order steps take rows of any number of units.  Shared by tests/test_shard_groups_gloo.py (the CPU worlds) and
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
    """NumpyBackend over tables of G*K-float rows (local[f] is [local rows, G*K])."""

    def __init__(self, local, vocab, parts, first, P, K, G=1):
        super().__init__(local, vocab, parts, first, P, K * G)
        self.G, self.Kg = G, K

    # ---- row groups ----
    def finish_groups(self, back, inv2d, K, outs):
        for o, v in zip(outs, finish_groups_np(back.numpy(), inv2d.numpy(), len(outs), K)):
            o.copy_(torch.from_numpy(v))

    def grad_groups(self, grads, inv2d, K, send):
        send.copy_(torch.from_numpy(grad_groups_np([g.detach().numpy() for g in grads], inv2d.numpy(), K, send.shape[0])))

    def accums(self, opt):
        return [torch.from_numpy(a) for a in opt["acc"]]
