#!/usr/bin/env python
"""rank_metrics_probe.py [--out FILE] [--limit SECONDS] -- time ops.group_rank_stats (csrc/rank_metrics.hip, the one kernel behind
metrics.GroupedMetrics.result()) against a straightforward torch formulation of the same statistics, on two shapes:

  (a) 65 536 blocks of 100 scores with the positive at index 0: the protocol of metrics/NCF_evaluation/ndcg_hr_mrr.py at the project's batch.
      torch: the [G, 100] compare of every row against its column 0.
  (b) 65 536 ragged groups, Zipf-like sizes with a mean near 50 and a few groups above the workgroup route's tile; labels at rate 0.3.
      torch: the groups padded to [G, n_max] and every pair compared by broadcast, as many groups at a time as 2^28 pair cells allow.

One process with its own time limit (SIGALRM).  Every shape is warmed up before its timed window; the windows are device events around
whole loops and the two sides alternate, three rounds each; the best round is reported beside the spread.  Both sides' integer statistics are
compared before anything is timed.  Bytes moved: what the kernel has to read and write once (12 B per entry, 8 B per offset, 56 B per group).
"""
import argparse
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def torch_blocks(s2):
    """Shape (a): [G, n] scores, the positive in column 0 -> gt, eq, rank (the other statistics are constants or products of these)."""
    pos, neg = s2[:, :1], s2[:, 1:]
    a, e = (neg > pos).sum(1), (neg == pos).sum(1)
    return neg.shape[1] - a - e, e, 1 + a


def torch_padded(s, y, w, offsets, cells=1 << 28):
    """Shape (b): pad to [G, n_max], compare all pairs by broadcast -> n_pos, n_neg, gt, eq, mis_w, tot_w."""
    G = offsets.numel() - 1
    sizes = offsets[1:] - offsets[:-1]
    n_max = int(sizes.max())
    gid = torch.repeat_interleave(torch.arange(G, device=s.device), sizes)
    col = torch.arange(s.numel(), device=s.device) - offsets[gid]
    S = torch.zeros(G, n_max, device=s.device)
    P = torch.zeros(G, n_max, dtype=torch.bool, device=s.device)
    N = torch.zeros(G, n_max, dtype=torch.bool, device=s.device)
    Wt = torch.zeros(G, n_max, dtype=torch.float64, device=s.device)
    S[gid, col], P[gid, col], N[gid, col], Wt[gid, col] = s, y > 0.5, ~(y > 0.5), w.double()
    out = [[] for _ in range(6)]
    step = max(1, cells // (n_max * n_max))
    for c in range(0, G, step):
        sc, p, n, wt = S[c:c + step], P[c:c + step], N[c:c + step], Wt[c:c + step]
        a = ((sc.unsqueeze(1) > sc.unsqueeze(2)) & n.unsqueeze(1)).sum(2)          # [g, i]: negatives j above entry i
        e = ((sc.unsqueeze(1) == sc.unsqueeze(2)) & n.unsqueeze(1)).sum(2)
        n_pos, n_neg = p.sum(1), n.sum(1)
        for o, v in zip(out, (n_pos, n_neg, ((n_neg.unsqueeze(1) - a - e) * p).sum(1), (e * p).sum(1), (wt * (a + e) * p).sum(1),
                              (wt * n_neg.unsqueeze(1) * p).sum(1))):
            o.append(v)
    return [torch.cat(o) for o in out]


def zipf_sizes(rng, G, tile):
    """Zipf-like sizes: a power law (P(size > x) = (25 / x)^2, smallest group 25, mean near 50) with the tail cut at 2 tile + 100; about one
    group in 400 lies above a tile of 512."""
    return np.minimum(np.floor(25.0 / np.sqrt(1.0 - rng.random(G))).astype(np.int64), 2 * tile + 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "rank_metrics_probe.txt"))
    ap.add_argument("--limit", type=int, default=420, help="seconds before the process ends itself")
    ap.add_argument("--groups", type=int, default=65536)
    args = ap.parse_args()
    signal.alarm(args.limit)
    if not torch.cuda.is_available():
        raise SystemExit("rank_metrics_probe: no GPU -- nothing measured")
    import dir_amd
    from dir_amd import ops
    dir_amd.load_library()
    W, T = ops.group_rank_limits()
    G = args.groups
    rng = np.random.default_rng(7)
    dev = torch.device("cuda:0")
    lines = ["rank_metrics_probe: %s, G = %d, route limits wave_max = %d tile = %d" % (torch.cuda.get_device_name(0), G, W, T)]

    def report(name, n_entries, kernel, plain, kernel_iters, plain_iters):
        for _ in range(3):                                       # warm up both sides at this shape
            kernel()
        plain()
        torch.cuda.synchronize()
        tk, tp = [], []
        for _ in range(3):                                       # alternate the two sides
            tk.append(timed(kernel, kernel_iters))
            tp.append(timed(plain, plain_iters))
        moved = 12 * n_entries + 8 * (G + 1) + 56 * G
        lines.append("%s: %d entries, %.1f MB moved | kernel %.1f us (rounds %s) = %.0f GB/s | torch %.1f us (rounds %s) | torch / kernel %.2f"
                     % (name, n_entries, moved / 1e6, min(tk), " ".join("%.1f" % t for t in tk), moved / min(tk) / 1e3, min(tp),
                        " ".join("%.1f" % t for t in tp), min(tp) / min(tk)))
        print(lines[-1], flush=True)

    # (a) blocks of 100
    n = 100
    s2 = torch.from_numpy(rng.random((G, n)).astype(np.float32)).to(dev)
    y = torch.zeros(G, n, device=dev)
    y[:, 0] = 1.0
    s, y, w = s2.reshape(-1), y.reshape(-1), torch.ones(G * n, device=dev)
    off = torch.arange(G + 1, device=dev, dtype=torch.int64) * n
    st = ops.group_rank_stats(s, y, w, off)
    gt, eq, rank = torch_blocks(s2)
    assert torch.equal(st["gt"], gt) and torch.equal(st["eq"], eq) and torch.equal(st["rank"], rank), "shape (a): kernel and torch disagree"
    report("(a) %d blocks of %d" % (G, n), G * n, lambda: ops.group_rank_stats(s, y, w, off), lambda: torch_blocks(s2), 200, 200)

    # (b) ragged
    sizes = zipf_sizes(rng, G, T)
    N = int(sizes.sum())
    s = torch.from_numpy((rng.integers(0, 1 << 16, N) / np.float32(1 << 16)).astype(np.float32)).to(dev)
    y = torch.from_numpy((rng.random(N) < 0.3).astype(np.float32)).to(dev)
    w = torch.from_numpy(rng.integers(0, 8, N).astype(np.float32)).to(dev)            # integer-valued: both sides' float64 sums are exact
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
    st = ops.group_rank_stats(s, y, w, off)
    ref = torch_padded(s, y, w, off)
    for k, r in zip(("n_pos", "n_neg", "gt", "eq", "mis_w", "tot_w"), ref):
        assert torch.equal(st[k], r), "shape (b): kernel and torch disagree on %s" % k
    lines.append("(b) sizes: mean %.1f, median %d, max %d, %d groups above wave_max, %d above tile"
                 % (sizes.mean(), int(np.median(sizes)), sizes.max(), int((sizes > W).sum()), int((sizes > T).sum())))
    print(lines[-1], flush=True)
    report("(b) %d ragged groups" % G, N, lambda: ops.group_rank_stats(s, y, w, off), lambda: torch_padded(s, y, w, off), 50, 1)

    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
