#!/usr/bin/env python
"""mf_probe.py [--out FILE] [--limit SECONDS] -- time the three paths of csrc/mf.hip against what a user would write without them:

  score            ops.mf_score                       vs  three index_selects (P[u], Q[i], the biases), the [B, C, K] product and its sum
  score+backward   ops.mf_score + mf_score_backward   vs  the same expression over F.embedding(..., sparse=True) tables with autograd
                   (both sides end with per-occurrence row gradients: the kernel's slabs, torch's uncoalesced sparse .grads)
  sampler          ops.neg_sample                     vs  a host NumPy rejection loop (draw, test membership by searchsorted on the sorted
                   (user, item) keys, redraw the rejected: models/BPR/bpr_sampler.py:102-111 vectorised), including its copy to the device

B = 65 536, C in {1, 2, 100} (the sampler: n_neg = C), on three table sets: the reference's own sizes (U = 69 878, I = 10 677, K = 16: both
tables cache-resident) and U = I = 10 000 000, K = 64 with uniform and with Zipf(1.05) ids.

One process with its own time limit (SIGALRM).  Every shape is warmed up for at least 200 ms on both sides; then the two sides alternate,
every call between two device events (the host loop: a host clock around it and the synchronised copy), and the minimum of N is reported.
Both sides' results are compared before anything is timed.  Bytes moved: what the kernel has to read and write once."""
import argparse
import os
import signal
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def host_one(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def warm(fn, seconds=0.2):
    t = time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        if time.perf_counter() - t >= seconds:
            return


def alternate(kernel, plain, n, plain_timer=one):
    warm(kernel)
    warm(plain)
    tk, tp = [], []
    for _ in range(n):
        tk.append(one(kernel))
        tp.append(plain_timer(plain))
    return min(tk), min(tp)


def torch_score(P, Q, bu, bi, b0, ids):
    u, it = ids[:, 0], ids[:, 1:]
    pu = P.index_select(0, u)
    qi = Q.index_select(0, it.reshape(-1)).view(it.shape[0], it.shape[1], -1)
    b = bu.index_select(0, u).unsqueeze(1) + bi.index_select(0, it.reshape(-1)).view(it.shape)
    return (pu.unsqueeze(1) * qi).sum(-1) + (b + b0)


def torch_score_backward(P, Q, bu, bi, b0, ids, dl):
    F = torch.nn.functional
    u, it = ids[:, 0], ids[:, 1:]
    for t in (P, Q, bu, bi):
        t.grad = None
    s = (F.embedding(u, P, sparse=True).unsqueeze(1) * F.embedding(it, Q, sparse=True)).sum(-1) + \
        ((F.embedding(u, bu, sparse=True) + F.embedding(it, bi, sparse=True).squeeze(-1)) + b0)
    s.backward(dl)
    return s


def host_rejection(users, keys, num_items, n_neg, rng, dev):
    """The reference's loop, vectorised: redraw until no (user, item) is a known pair."""
    u = np.repeat(users, n_neg)
    j = rng.integers(0, num_items, u.size)
    bad = np.arange(u.size)
    while bad.size:
        k = u[bad] * num_items + j[bad]
        at = np.searchsorted(keys, k)
        hit = (at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == k)
        bad = bad[hit]
        j[bad] = rng.integers(0, num_items, bad.size)
    return torch.from_numpy(j.reshape(-1, n_neg)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mf_probe.txt"))
    ap.add_argument("--limit", type=int, default=540, help="seconds before the process ends itself")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    signal.alarm(args.limit)
    if not torch.cuda.is_available():
        raise SystemExit("mf_probe: no GPU -- nothing measured")
    import dir_amd
    from dir_amd import ops
    dir_amd.load_library()
    dev = torch.device("cuda:0")
    B, N = args.batch, args.rounds
    rng = np.random.default_rng(11)
    lines = ["mf_probe: %s, B = %d, min of %d alternating calls after >= 200 ms of warm-up per side" % (torch.cuda.get_device_name(0), B, N)]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for name, U, I, K, zipf in (("reference sizes", 69878, 10677, 16, False), ("10M x 10M uniform", 10_000_000, 10_000_000, 64, False),
                                ("10M x 10M Zipf(1.05)", 10_000_000, 10_000_000, 64, True)):
        gen = torch.Generator(device=dev).manual_seed(3)
        P = torch.randn((U, K), generator=gen, device=dev) * 0.1
        Q = torch.randn((I, K), generator=gen, device=dev) * 0.1
        bu, bi = torch.randn(U, generator=gen, device=dev) * 0.1, torch.randn(I, generator=gen, device=dev) * 0.1
        b0 = torch.full((1,), 0.25, device=dev)
        gP, gQ, gbu, gbi = [t.clone().requires_grad_() for t in (P, Q, bu.unsqueeze(1), bi.unsqueeze(1))]
        draw = (lambda n, V: (rng.zipf(1.05, n) - 1) % V) if zipf else (lambda n, V: rng.integers(0, V, n))
        say("%s: U = %d, I = %d, K = %d (tables %.0f MB)" % (name, U, I, K, (U + I) * K * 4 / 1e6))
        # every user's interacted items: 16 draws per user of the batch's user pool (the sampler reads only those users' lists)
        pool = np.unique(draw(B, U))
        pu, pi = np.repeat(pool, 16), draw(pool.size * 16, I)
        ui = ops.UserItems.from_pairs(torch.from_numpy(pu).to(dev), torch.from_numpy(pi).to(dev), U, I)
        keys = np.unique(pu.astype(np.int64) * I + pi)
        state = ops.DropoutState(seed=5, device=dev)
        for C in (1, 2, 100):
            users = pool[rng.integers(0, pool.size, B)]
            ids = torch.from_numpy(np.concatenate([users[:, None], draw(B * C, I).reshape(B, C)], 1).astype(np.int64)).to(dev)
            dl = torch.randn((B, C), generator=gen, device=dev)
            got, ref = ops.mf_score(P, Q, ids, bu, bi, b0), torch_score(P, Q, bu, bi, b0, ids)
            err = float(((got - ref).abs() / (1 + ref.abs())).max())
            assert err <= 1e-5, "score: kernel and torch disagree (%.3e)" % err
            fwd = B * (1 + C) * (8 + 4 * K + 4) + 4 * B * C
            bwd = fwd + 4 * B * C + B * (1 + C) * (4 * K + 4)
            tk, tp = alternate(lambda: ops.mf_score(P, Q, ids, bu, bi, b0), lambda: torch_score(P, Q, bu, bi, b0, ids), N)
            say("  C = %3d score:          %6.1f MB moved | kernel %8.1f us = %5.0f GB/s | torch %8.1f us | torch / kernel %.2f"
                % (C, fwd / 1e6, tk, fwd / tk / 1e3, tp, tp / tk))

            def kernel_both():
                ops.mf_score(P, Q, ids, bu, bi, b0)
                return ops.mf_score_backward(P, Q, ids, dl, bu, bi)

            tk, tp = alternate(kernel_both, lambda: torch_score_backward(gP, gQ, gbu, gbi, b0, ids, dl), N)
            say("  C = %3d score+backward: %6.1f MB moved | kernel %8.1f us = %5.0f GB/s | torch %8.1f us | torch / kernel %.2f"
                % (C, bwd / 1e6, tk, bwd / tk / 1e3, tp, tp / tk))
            tu = torch.from_numpy(users.astype(np.int64)).to(dev)
            neg = ops.neg_sample(tu, ui, C, state).cpu().numpy()
            assert not np.isin(users[:, None] * I + neg, keys).any() and neg.min() >= 0 and neg.max() < I, "sampler: a positive was drawn"
            tk, tp = alternate(lambda: ops.neg_sample(tu, ui, C, state), lambda: host_rejection(users, keys, I, C, rng, dev), max(3, N // 2),
                               plain_timer=host_one)
            say("  n_neg = %3d sampler:    %6.1f MB moved | kernel %8.1f us                | host loop %10.1f us | host / kernel %.1f"
                % (C, B * (8 + 16 + 8 * C) / 1e6, tk, tp, tp / tk))
        del P, Q, bu, bi, gP, gQ, gbu, gbi, ui
        torch.cuda.empty_cache()

    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
