"""tools/shard_din_probe.py (GPU box): times of the rank-local kernels of ShardedDINTrainer's lookup and backward on ONE GPU, in the manner
of tools/shard_bags_train_probe.py, on BASELINE config 4's shapes: B = 65 536 samples, T = 50 history ids + the candidate (51 entries per
sample, flattened to a one-slot lookup) over a 10 M x 64 goods table, uniform and Zipf(1.05) ids (tools/dedup_probe.py's generator).

  world 1   one rank: the slabs hold the whole batch
  world 2   rank 0's kernels of a two-rank step, emulated in one process: rank 0's half of the table as the local shard, the received
            slabs = rank 0's own slab for owner 0, twice; no exchange runs (nothing here measures a link).
Per world and id distribution, de-duplicated (dir_shard_bucket_cap_dedup) and plain (dir_shard_bucket_cap):
  bucket_us, owner_gather_us (dir_gather_slabs_f32),
  scatter_us: the requester's gradient slab -- dedup: dir_rows_scatter_sum_f32 as a whole, sort_us of it = the in-tree radix sort alone on
      the same (position, entry) pairs, sum_us = scatter_us - sort_us (key pass + zero fill + tile sums + fix pass); plain: the torch.zeros +
      torch.where + index_copy_ that lookup_train(dedup=False)'s backward runs,
  owner_update_us (dir_sparse_adagrad_sorted_payload_f32 over the received payload),
  travel: the share of the live entries that still travels (sent payload words / live entries),
  row_bytes_per_peer_P8_arith: ARITHMETIC, not a measurement -- B * 51 / 8 entries per peer x travel x K x 4 bytes, each way.
Prints one JSON line per measurement (median of --iters timed runs after 3 warm-up runs, HIP events); profiles/shard_din_probe.jsonl keeps
the lines of one run."""
import argparse
import ctypes
import json
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import _lib, ops  # noqa: E402
from dir_amd.shard import div_range  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--world", type=int, default=0, help="1 or 2 (default: both)")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--batch", type=int, default=65536)
args = ap.parse_args()

dir_amd.load_library()
lib = _lib.load()
dev = torch.device("cuda", 0)
B, T, K, V = args.batch, 50, 64, 10_000_000
n = B * (T + 1)
gen = torch.Generator(device=dev).manual_seed(1)
full = torch.randn((V, K), generator=gen, device=dev) * 0.1
G = torch.randn((n, K), generator=gen, device=dev)
vdev = torch.tensor([V], dtype=torch.int64, device=dev)


def med_us(fn, iters=args.iters):
    ts = []
    for i in range(iters + 3):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def draw(dist):
    if dist == "uniform":
        return torch.randint(0, V, (n, 1), generator=gen, device=dev)
    u = torch.rand((n, 1), generator=gen, device=dev, dtype=torch.float64)
    a = 1.05
    return ((V ** (1 - a) - 1) * u + 1).pow(1 / (1 - a)).floor().long().clamp_(1, V) - 1


def sort_us(idx, R):
    """The in-tree radix sort alone on rows_scatter_sum's pairs: keys = positions (R for the dropped), values = entry numbers."""
    bits = max(1, int(R).bit_length())
    k = torch.where((idx >= 0) & (idx < R), idx, torch.full_like(idx, R)).to(torch.int32)
    v = torch.arange(idx.numel(), device=dev, dtype=torch.int32)
    need = int(lib.dir_debug_radix_sort_workspace_bytes(idx.numel(), bits))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ko, vo, ki, vi = torch.empty_like(k), torch.empty_like(v), k.clone(), v.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        assert lib.dir_debug_radix_sort_pairs_u32(p(ki), p(vi), idx.numel(), bits, p(ko), p(vo), p(ws), need, st) == 0
    return med_us(run)


for P in ((1, 2) if args.world == 0 else (args.world,)):
    lo, hi = div_range(V, P, 0)
    local = full[lo:hi].contiguous()
    ts = ops.TableSet([local])
    sopt = ops.SparseAdagrad(ts, 0.05, 0.1)
    for dist in ("uniform", "zipf1.05"):
        ids = draw(dist)
        flat = ids.reshape(-1).contiguous()
        live = n
        for dedup in (True, False):
            cap = n                                      # roomy first, then this batch's demand + 5 %
            for rep in range(2):
                payload = torch.empty(P * (cap + 1), dtype=torch.int64, device=dev)
                inv = torch.empty(n, dtype=torch.int64, device=dev)
                counts = torch.empty(P, dtype=torch.int64, device=dev)
                over = torch.zeros(1, dtype=torch.int32, device=dev)
                ws = torch.zeros(128, dtype=torch.int32, device=dev)
                if dedup:
                    bucket = lambda: ops.shard_bucket_cap_dedup(ids, vdev, P, cap, payload, inv, counts, over, ws)      # noqa: E731
                else:
                    bucket = lambda: ops.shard_bucket_cap(flat, vdev, P, cap, payload, inv, counts, over, ws)           # noqa: E731
                bucket()
                torch.cuda.synchronize()
                sent, demand = int(counts.sum()), int(counts.max())
                if rep == 0:
                    cap = int(demand * 1.05) // 16 * 16 + 64
            assert not int(over), "the second pass's slabs must hold the batch"
            t_bucket = med_us(bucket)
            slabs = payload.view(P, cap + 1)
            recv = slabs.clone()
            recv[:] = slabs[0]                           # every sender's slab for rank 0 looks like rank 0's own
            recv = recv.reshape(-1)
            rows = torch.empty((P * cap, K), dtype=torch.float32, device=dev)
            t_gather = med_us(lambda: ops.gather_slabs(ts, recv, P, cap, rows))
            R = P * cap
            if dedup:
                out = torch.empty((R, K), dtype=torch.float32, device=dev)
                t_scatter = med_us(lambda: ops.rows_scatter_sum(inv, G, R, out=out))
                t_sort = sort_us(inv, R)
                extra = dict(sort_us=round(t_sort, 1), sum_us=round(t_scatter - t_sort, 1))
            else:
                def index_copy():
                    gsend = torch.zeros((R + 1, K), dtype=torch.float32, device=dev)
                    gsend.index_copy_(0, torch.where(inv < 0, torch.full_like(inv, R), inv), G)
                t_scatter = med_us(index_copy)
                extra = {}
            hdr = recv.view(P, cap + 1)[:, 0] & 0xffffffff
            pos = torch.arange(cap, device=dev)
            pay = torch.where(pos.unsqueeze(0) < hdr.unsqueeze(1), recv.view(P, cap + 1)[:, 1:], torch.full_like(recv.view(P, cap + 1)[:, 1:], -1)).reshape(-1)
            grecv = torch.randn((P * cap, K), generator=gen, device=dev)
            t_update = med_us(lambda: sopt.step_payload(pay, grecv))
            travel = sent / live
            emit(what="sharded_din_rank_local", world=P, ids=dist, dedup=dedup, B=B, T=T, K=K, entries=n, sent_words=sent, travel=round(travel, 4),
                 cap=cap, bucket_us=round(t_bucket, 1), owner_gather_us=round(t_gather, 1), scatter_us=round(t_scatter, 1),
                 owner_update_us=round(t_update, 1), row_bytes_per_peer_P8_arith=int(n / 8 * travel * K * 4), **extra)
            del payload, inv, recv, rows, grecv, pay
            torch.cuda.empty_cache()
    del sopt, ts, local
    torch.cuda.empty_cache()
