"""tools/shard_bags_train_probe.py (GPU box): the training leg of tools/shard_bags_probe.py -- times of the rank-local kernels of the
backward of ShardedTables.lookup_bags_train (csrc/shard_bags.hip: bags_grad_k; csrc/backward.hip: dir_sparse_adagrad_sorted_bags_f32) on
ONE GPU, on that probe's workload: B = 65 536 samples, one history slot of exactly L = 50 ids over a 10 M-row table plus 26 one-hot slots
(100 000 rows each), K = 64, mean combiner.

  world 1   the requester's gradient scatter and the owner's update as lookup_bags_train's backward runs them with one rank, beside the
            single-GPU multi-hot step on the same bags: autograd.embedding_bag's backward (sparse table gradients) + torch.optim.Adagrad
  world 2   rank 0's kernels of a two-rank step, emulated in one process as shard_bags_probe.py does: rank 0's half of every table as the
            local shard, the received slabs = rank 0's own slab twice; no exchange runs (nothing here measures a link).
  owner_update_us = key pass + radix sort + adagrad_tile_k + adagrad_fix_k in one call; `--world N --iters I --no-single` runs one world
  only, for a rocprofv3 --kernel-trace --stats pass that splits it per kernel.
Prints one JSON line per measurement (median of --iters timed runs after 3 warm-up runs, HIP events)."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import autograd as ag  # noqa: E402
from dir_amd import ops  # noqa: E402
from dir_amd.shard import div_range  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--world", type=int, default=0, help="1 or 2 (default: both)")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--no-single", action="store_true", help="skip the single-GPU step")
args = ap.parse_args()

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
G = torch.randn((B, F * K), generator=gen, device=dev)


def med_us(fn, n=args.iters, pre=None):
    ts = []
    for i in range(n + 3):
        if pre is not None:
            pre()
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


if not args.no_single:
    params = [torch.nn.Parameter(t.clone()) for t in full]
    pts = ops.TableSet([p.data for p in params])
    opt = torch.optim.Adagrad(params, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    state = {}

    def fwd():
        opt.zero_grad(set_to_none=True)
        state["out"] = ag.embedding_bag(pts, vals, params, offs, None, combiner="mean")

    def bwd_step():
        state["out"].backward(G)
        opt.step()
    t_single = med_us(bwd_step, pre=fwd)
    emit(what="single_gpu_multihot_step", B=B, F=F, K=K, nnz=nnz, backward_plus_sparse_adagrad_us=round(t_single, 1))
    del params, pts, opt, state
    torch.cuda.empty_cache()

for P in ((1, 2) if args.world == 0 else (args.world,)):
    local = [t[slice(*div_range(v, P, 0))].contiguous() for t, v in zip(full, vocab)]
    ts = ops.TableSet(local)
    sopt = ops.SparseAdagrad(ts, 0.05, 0.1)
    vdev = torch.tensor(vocab, dtype=torch.int64, device=dev)
    nb = B * F
    ws = torch.zeros(256, dtype=torch.int32, device=dev)
    stat = torch.zeros(3, dtype=torch.int64, device=dev)
    cap_e, cap_b = nnz, nb                       # the exact demand of this batch (first call with roomy slabs), + 5 %
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
    recv = slabs.view(P, cap_e + 1, 2).clone()
    recv[:] = slabs.view(P, cap_e + 1, 2)[0]                       # every sender's slab for rank 0 looks like rank 0's own
    recv = recv.reshape(-1)
    send = torch.zeros((P * cap_b, K), dtype=torch.float32, device=dev)
    t_s = med_us(lambda: ops.shard_bags_grad(G, P, pos, mask, denom, B, F, None, ops.MEAN, cap_b, send))
    grecv = send.clone()
    grecv.view(P, cap_b, K)[:] = send.view(P, cap_b, K)[0]          # the gradients rank 0 would receive: its own, twice
    n0 = int(recv.view(P, cap_e + 1, 2)[0, 0, 0]) & 0xffffffff        # rank 0's own slab: its entry count
    rows_touched = int(torch.unique(recv.view(P, cap_e + 1, 2)[0, 1:1 + n0, 0]).numel())
    t_u = med_us(lambda: sopt.step_bags(recv, P, cap_e, cap_b, grecv))
    emit(what="lookup_bags_train_rank_local", world=P, B=B, F=F, K=K, nnz=nnz, entries_per_owner=de, partial_rows_per_owner=db,
         received_entries=P * n0, distinct_rows_touched=rows_touched, sort_entries=P * cap_e, gradient_row_bytes_per_peer=db * K * 4,
         scatter_us=round(t_s, 1), owner_update_us=round(t_u, 1), total_us=round(t_s + t_u, 1))
    del sopt, ts, local
    torch.cuda.empty_cache()
