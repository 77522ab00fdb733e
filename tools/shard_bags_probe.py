"""tools/shard_bags_probe.py (GPU box): times of the three rank-local kernels of ShardedTables.lookup_bags (csrc/shard_bags.hip) on ONE GPU.

Workload: B = 65 536 samples, one history slot of exactly L = 50 ids over a 10 M-row table plus 26 one-hot slots (100 000 rows
each), K = 64, mean combiner, FM fused into the combine.

  world 1   the three kernels as lookup_bags runs them with one rank (one slab; every bag has one owner), beside the single-GPU
            ops.embedding_bag (bag_csr_k) on the same bags
  world 2   rank 0's kernels of a two-rank lookup, emulated in one process: bucket into 2 slabs, rank 0's half of every table as the
            local shard, the received buffer = rank 0's own slab twice (the peer's slab has the same statistics), then pool and combine.
            No exchange runs: these are the rank-local kernel times only, and nothing here measures a link.
Prints one JSON line per measurement (median of 20 timed runs after 5 warm-up runs, HIP events)."""
import json
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import ops  # noqa: E402
from dir_amd.shard import div_range  # noqa: E402

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, L, K, NF, VH, VO = 65536, 50, 64, 26, 10_000_000, 100_000
F = NF + 1
vocab = [VH] + [VO] * NF
gen = torch.Generator(device=dev).manual_seed(1)
full = [torch.randn((v, K), generator=gen, device=dev) * 0.1 for v in vocab]
vals = torch.cat([torch.randint(0, VH, (B, L), generator=gen, device=dev)] +
                 [torch.randint(0, VO, (B, 1), generator=gen, device=dev) for _ in range(NF)], dim=1).reshape(-1).contiguous()
lens = torch.ones((B, F), dtype=torch.int64, device=dev)
lens[:, 0] = L
offs = torch.zeros(B * F + 1, dtype=torch.int64, device=dev)
offs[1:] = torch.cumsum(lens.reshape(-1), 0)
nnz = vals.numel()


def med_us(fn, n=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def emit(**kw):
    print(json.dumps(kw), flush=True)


full_ts = ops.TableSet(full)
emit(what="single_gpu_embedding_bag", B=B, F=F, K=K, nnz=nnz, us=round(med_us(lambda: ops.embedding_bag(full_ts, vals, offs, combiner="mean")), 1))

for P in (1, 2):
    local = [t[slice(*div_range(v, P, 0))].contiguous() for t, v in zip(full, vocab)]
    ts = ops.TableSet(local)
    vdev = torch.tensor(vocab, dtype=torch.int64, device=dev)
    nb = B * F
    ws = torch.zeros(256, dtype=torch.int32, device=dev)
    stat = torch.zeros(3, dtype=torch.int64, device=dev)
    # capacities: the exact demand of this batch (first call with roomy slabs), + 5 %
    cap_e, cap_b = nnz, nb
    for rep in range(2):
        slabs = torch.empty(P * (cap_e + 1) * 2, dtype=torch.int64, device=dev)
        pos = torch.empty(nb * P, dtype=torch.int32, device=dev)
        mask = torch.empty(nb, dtype=torch.int64, device=dev)
        denom = torch.empty(nb, dtype=torch.float32, device=dev)
        ops.shard_bags_bucket(vals, offs, None, B, F, 1, vdev, P, None, ops.MEAN, 0, cap_e, cap_b, slabs, pos, mask, denom, ws, stat=stat)
        torch.cuda.synchronize()
        over, de, db = (int(x) for x in stat.tolist())
        if rep == 0:
            cap_e, cap_b = int(de * 1.05) // 16 * 16 + 64, int(db * 1.05) // 16 * 16 + 64
    assert not over
    rows = torch.empty((P * cap_b, K), dtype=torch.float32, device=dev)
    recv = slabs.view(P, cap_e + 1, 2).clone()
    recv[:] = slabs.view(P, cap_e + 1, 2)[0]                       # every sender's slab for rank 0 looks like rank 0's own
    recv = recv.reshape(-1)
    out = torch.empty((B, F * K), dtype=torch.float32, device=dev)
    fm = torch.empty((B, 1), dtype=torch.float32, device=dev)
    t_b = med_us(lambda: ops.shard_bags_bucket(vals, offs, None, B, F, 1, vdev, P, None, ops.MEAN, 0, cap_e, cap_b, slabs, pos, mask, denom,
                                               ws))
    t_p = med_us(lambda: ops.shard_bags_pool(ts, recv, P, cap_e, cap_b, None, 0.0, rows))
    t_c = med_us(lambda: ops.shard_bags_combine(rows, P, pos, mask, denom, B, F, None, ops.MEAN, out, fm))
    if P == 1:      # one consistent bucket -> pool -> combine (the slab layout of every bucket call is its own)
        ops.shard_bags_bucket(vals, offs, None, B, F, 1, vdev, P, None, ops.MEAN, 0, cap_e, cap_b, slabs, pos, mask, denom, ws)
        ops.shard_bags_pool(ts, slabs, P, cap_e, cap_b, None, 0.0, rows)
        ops.shard_bags_combine(rows, P, pos, mask, denom, B, F, None, ops.MEAN, out, fm)
        ref = ops.embedding_bag(full_ts, vals, offs, combiner="mean")
        same = bool(torch.equal(out, ref)) and bool(torch.equal(fm, ops.fm_logit(out, F, K)))
    else:
        same = None
    emit(what="lookup_bags_rank_local", world=P, B=B, F=F, K=K, nnz=nnz, entries_per_owner=de, partial_rows_per_owner=db,
         partial_row_bytes_per_peer=db * K * 4, raw_row_bytes_per_peer=de * K * 4, cap_e=cap_e, cap_b=cap_b,
         bucket_us=round(t_b, 1), pool_us=round(t_p, 1), combine_fm_us=round(t_c, 1), total_us=round(t_b + t_p + t_c, 1),
         bitwise_vs_embedding_bag=same)
