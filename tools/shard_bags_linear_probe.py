"""tools/shard_bags_linear_probe.py (GPU box): what DeepFM's first-order term costs over row-sharded multi-hot bags (csrc/shard_linear.hip:
bags_linear_pool_k, bags_linear_denom_k, bags_linear_combine_k, bags_linear_grad_k; csrc/backward.hip: dir_sparse_ftrl_rows_sorted_bags_f32)
on ONE GPU, on the workload of tools/shard_bags_probe.py: B = 65 536 samples, one history slot of exactly L = 50 ids over a 10 M-row table
plus 26 one-hot slots (100 000 rows each), K = 64, mean combiner for the embeddings.

  world 1   ShardedTables as one rank runs it:
            lookup_bags(want_fm=True) without and with want_lin             -> the term's added forward time
            lookup_bags_train forward + backward without and with the term  -> the term's added training time
            (the calls without the term run the code of before the term existed: they are the baseline)
  kernels   world 1, and rank 0 of an emulated world 2 (rank 0's half of every table and weight vector as the local shard, the received
            slabs = rank 0's own slab twice, as tools/shard_bags_train_probe.py does; no exchange runs: nothing here measures a link):
            owner pool, requester combine (sum: one kernel; mean: + the denominator kernel), requester gradient scatter, the owner's
            FTRL on the Adagrad step's sort and on its own sort; beside the pool its bare access pattern -- dir_shard_linear_gather_f32
            over a flat payload of the same (row, slot) words: one 8-byte word + one 4-byte row read + one 4-byte write per entry
  single    ops.linear_logit on the same bags over the unsharded weights (the single-GPU yardstick)
One JSON line per measurement, printed and written to --out: median of --iters timed runs (HIP events) after >= 200 ms of warm-up runs
(profiles/NOTES.md R6.3: the clocks after idle)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import ops  # noqa: E402
from dir_amd.shard import ShardedTables, div_range  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--out", default="profiles/shard_bags_linear_probe.jsonl")
ap.add_argument("--only", default="", help="comma-separated subset of: lookup, train, kernels, single (for a rocprofv3 --kernel-trace --stats pass)")
args = ap.parse_args()
only = set(filter(None, args.only.split(",")))

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, L, K, NF, VH, VO = args.batch, 50, 64, 26, 10_000_000, 100_000
F = NF + 1
vocab = [VH] + [VO] * NF
gen = torch.Generator(device=dev).manual_seed(1)
full = [torch.randn((v, K), generator=gen, device=dev) * 0.1 for v in vocab]
full_w = [torch.randn((v,), generator=gen, device=dev) * 0.1 for v in vocab]
vals = torch.cat([torch.randint(0, VH, (B, L), generator=gen, device=dev)] +
                 [torch.randint(0, VO, (B, 1), generator=gen, device=dev) for _ in range(NF)], dim=1).reshape(-1).contiguous()
lens = torch.ones((B, F), dtype=torch.int64, device=dev)
lens[:, 0] = L
offs = torch.zeros(B * F + 1, dtype=torch.int64, device=dev)
offs[1:] = torch.cumsum(lens.reshape(-1), 0)
nnz = vals.numel()
G = torch.randn((B, F * K), generator=gen, device=dev)
g = torch.randn((B, 1), generator=gen, device=dev)
bias = torch.zeros(1, device=dev)
FTRL = dict(lr=0.2, l1=0.001, l2=0.001)
LINES = []


def med_us(fn, n=args.iters):
    t0 = time.perf_counter()
    runs = 0
    while runs < 3 or time.perf_counter() - t0 < 0.2:         # >= 200 ms of warm-up: the clocks come up
        fn()
        torch.cuda.synchronize()
        runs += 1
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 1)


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def want(name):
    return not only or name in only


shape = dict(B=B, F=F, K=K, nnz=nnz, history_len=L)

if want("lookup") or want("train"):
    st = ShardedTables.from_full(full).attach_linear_from_full(full_w)
    st.enable_training(0.05, 0.1).enable_linear_training(**FTRL)
    if want("lookup"):
        for lc in ("sum", "mean"):
            t0 = med_us(lambda: st.lookup_bags(vals, offs, None, combiner="mean", want_fm=True))
            t1 = med_us(lambda: st.lookup_bags(vals, offs, None, combiner="mean", want_fm=True, want_lin=True, lin_combiner=lc, lin_bias=bias))
            emit(what="lookup_bags_fm", world=1, **shape, lin_combiner=lc, without_lin_us=t0, with_lin_us=t1, added_us=round(t1 - t0, 1))
    if want("train"):
        def train(lc):
            if lc:
                emb, lin = st.lookup_bags_train(vals, offs, None, combiner="mean", with_linear=True, lin_combiner=lc)
                torch.autograd.backward([emb, lin], [G, g])
            else:
                st.lookup_bags_train(vals, offs, None, combiner="mean").backward(G)
        for lc in ("sum", "mean"):
            t0 = med_us(lambda: train(None))
            t1 = med_us(lambda: train(lc))
            emit(what="lookup_bags_train_forward_backward", world=1, **shape, lin_combiner=lc, without_linear_us=t0, with_linear_us=t1,
                 added_us=round(t1 - t0, 1))
    del st
    torch.cuda.empty_cache()

if want("single"):
    t = med_us(lambda: ops.linear_logit(full_w, vals, offs, None, combiner="sum", bias=bias))
    t_m = med_us(lambda: ops.linear_logit(full_w, vals, offs, None, combiner="mean", bias=bias))
    emit(what="single_gpu_linear_logit", **shape, sum_us=t, mean_us=t_m)

if want("kernels"):
    for P in (1, 2):
        local = [t[slice(*div_range(v, P, 0))].contiguous() for t, v in zip(full, vocab)]
        local_w = [w[slice(*div_range(v, P, 0))] for w, v in zip(full_w, vocab)]
        ts = ops.TableSet(local)
        lin_ts = ops.TableSet.ftrl_rows(local_w, 0.1)
        sopt = ops.SparseAdagrad(ts, 0.05, 0.1)
        fopt = ops.SparseFtrl(lin_ts, FTRL["lr"], l1=FTRL["l1"], l2=FTRL["l2"])
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
        n0 = int(recv.view(P, cap_e + 1, 2)[0, 0, 0]) & 0xffffffff        # rank 0's own slab: its entry count
        lrows = torch.zeros(P * cap_b, dtype=torch.float32, device=dev)
        lden = torch.ones(nb, dtype=torch.float32, device=dev)
        lin = torch.empty((B, 1), dtype=torch.float32, device=dev)
        t_pool = med_us(lambda: ops.shard_bags_linear_pool(lin_ts, recv, P, cap_e, cap_b, lrows))
        flat = recv.view(P, cap_e + 1, 2)[:, 1:1 + n0, 0].reshape(-1).contiguous()      # the same (row, slot) words as a flat payload
        bare = torch.empty(flat.numel(), dtype=torch.float32, device=dev)
        t_bare = med_us(lambda: ops.shard_linear_gather(lin_ts, flat, P, None, bare))
        t_sum = med_us(lambda: ops.shard_bags_linear_combine(lrows, P, cap_b, pos, mask, vals, offs, None, F, 1, vdev, 0, B, F, "sum", None,
                                                             bias, lin))
        t_mean = med_us(lambda: ops.shard_bags_linear_combine(lrows, P, cap_b, pos, mask, vals, offs, None, F, 1, vdev, 0, B, F, "mean", lden,
                                                              bias, lin))
        gsend = torch.zeros(P * cap_b, dtype=torch.float32, device=dev)
        t_scat = med_us(lambda: ops.shard_bags_linear_grad(g, P, cap_b, pos, mask, lden, B, F, "mean", gsend))
        grecv = gsend.clone()
        grecv.view(P, cap_b)[:] = gsend.view(P, cap_b)[0]               # the gradients rank 0 would receive: its own, twice
        grows = torch.randn((P * cap_b, K), generator=gen, device=dev)

        def both():
            sopt.step_bags(recv, P, cap_e, cap_b, grows)
            fopt.step_bags(recv, P, cap_e, cap_b, grecv, sorted_by=sopt)
        t_a = med_us(lambda: sopt.step_bags(recv, P, cap_e, cap_b, grows))
        t_own = med_us(lambda: fopt.step_bags(recv, P, cap_e, cap_b, grecv))
        t_both = med_us(both)
        emit(what="bags_linear_kernels_rank_local", world=P, **shape, entries_per_owner=de, partial_rows_per_owner=db, received_entries=P * n0,
             sort_entries=P * cap_e, float_bytes_per_peer=db * 4, owner_pool_us=t_pool, bare_gather_same_entries_us=t_bare,
             combine_sum_us=t_sum, combine_mean_with_denominators_us=t_mean, grad_scatter_us=t_scat, owner_adagrad_us=t_a,
             owner_ftrl_own_sort_us=t_own, owner_adagrad_then_ftrl_on_its_sort_us=t_both, owner_ftrl_on_adagrad_sort_us=round(t_both - t_a, 1))
        del sopt, fopt, ts, lin_ts, local, local_w
        torch.cuda.empty_cache()

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")
