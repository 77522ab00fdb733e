"""tools/shard_adam_probe.py (GPU box): what one training lookup costs under the owner-side sparse Adam of the row-sharded tables
(ShardedTables.enable_training_adam; csrc/backward.hip: dir_sparse_adam_payload_norm_f32 / dir_sparse_adam_payload_apply_f32) at world
size 1 on ONE GPU, on the headline shape: B = 65 536 samples x F = 26 slots x 1 M-row tables, K = 16, uniform ids.

  sharded_adam      lookup_train forward + backward under Adam, clip_norm = 100 (norm pass + apply + decay pass) and clip_norm = 0
  (i)  single_adam  ops.SparseAdam.step on the unsharded tables, same ids and gradient          -- the one-GPU yardstick
  (ii) sharded_adagrad  the same lookup_train forward + backward under Adagrad (code this change leaves alone), and ops.SparseAdagrad.step
                    on unsharded tables: their difference is what the sharded route (bucket, owner gather, finish, gradient scatter) costs
  and the two halves of the owner's step on their own: the norm pass, the apply with a sort of its own (the norm pass's sort forgotten),
  norm + apply on the norm pass's sort without and with the sum of the shares in between, and the decay pass alone.
The decay pass streams every row of var, m and v in and out (26 x 1 M x 16 x 4 B x 6 = 10 GB) and bounds both Adam figures from below.
No exchange runs at world 1 (nothing here measures a link).  The comparands alternate inside one timed loop (other work shares the
host); prints one JSON line per measurement: median of --iters timed runs after 3 warm-up runs of every comparand, HIP events."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import ops  # noqa: E402
from dir_amd.shard import ShardedTables  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--rows", type=int, default=1_000_000)
args = ap.parse_args()

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, F, K, V = args.batch, 26, 16, args.rows
gen = torch.Generator(device=dev).manual_seed(1)
full = [torch.randn((V, K), generator=gen, device=dev) * 0.1 for _ in range(F)]
ids = torch.randint(0, V, (B, F), generator=gen, device=dev)
G = torch.randn((B, F * K), generator=gen, device=dev) * 0.01
B1, B2, EPS, LR_T = 0.9, 0.999, 1e-4, 0.003


def alternate_us(fns, n=args.iters):
    """{name: median microseconds}: every round runs each comparand once, in turn; 3 warm-up rounds."""
    ts = {k: [] for k in fns}
    for i in range(n + 3):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ts[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: round(sorted(v)[len(v) // 2], 1) for k, v in ts.items()}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def sharded_adam(clip):
    st = ShardedTables.from_full([t.clone() for t in full]).enable_training_adam(B1, B2, EPS, clip)
    st.optimizer.lr_t = LR_T
    return st


shape = dict(world=1, B=B, F=F, K=K, rows_per_table=V, device=torch.cuda.get_device_name(0))
st_clip, st_noclip = sharded_adam(100.0), sharded_adam(0.0)
st_ada = ShardedTables.from_full([t.clone() for t in full]).enable_training(0.05, 0.1)
single_adam = ops.SparseAdam(ops.TableSet([t.clone() for t in full]), B1, B2, EPS, 100.0)
single_adam.lr_t = LR_T
single_ada = ops.SparseAdagrad(ops.TableSet([t.clone() for t in full]), 0.05, 0.1)

t = alternate_us({
    "sharded_adam_clip100_us": lambda: st_clip.lookup_train(ids).backward(G),
    "sharded_adam_noclip_us": lambda: st_noclip.lookup_train(ids).backward(G),
    "single_gpu_adam_step_us": lambda: single_adam.step(ids, G),
    "sharded_adagrad_us": lambda: st_ada.lookup_train(ids).backward(G),
    "single_gpu_adagrad_step_us": lambda: single_ada.step(ids, G),
    "sharded_lookup_forward_only_us": lambda: st_ada.lookup(ids),
})
emit(what="sharded_lookup_train_forward_backward", **shape, **t,
     adam_excess_over_single_us=round(t["sharded_adam_clip100_us"] - t["single_gpu_adam_step_us"], 1),
     adagrad_excess_over_single_us=round(t["sharded_adagrad_us"] - t["single_gpu_adagrad_step_us"], 1),
     decay_pass_bytes=F * V * K * 4 * 6)

# the two halves of the owner's step on the payload and gradient rows of one lookup (every entry live at world 1)
be, opt = st_clip.backend, st_clip.optimizer
pay = (torch.randint(0, V, (B * F,), generator=gen, device=dev) * F + torch.arange(B * F, device=dev) % F).contiguous()
rows = torch.randn((B * F, K), generator=gen, device=dev) * 0.01
norms = st_clip._sum_norm_shares(be.adam_norm(opt, pay, rows))


def halves():
    be.adam_apply(opt, pay, rows, st_clip._sum_norm_shares(be.adam_norm(opt, pay, rows)))


def apply_own_sort():
    opt.forget_sort()                                      # forget the norm pass's sort of this payload: key pass + sort run again
    be.adam_apply(opt, pay, rows, norms)


def apply_on_norm_sort():
    be.adam_norm(opt, pay, rows)                           # (timed with it: the difference to the norm pass alone is the apply)
    be.adam_apply(opt, pay, rows, norms)


t = alternate_us({
    "owner_norm_pass_us": lambda: be.adam_norm(opt, pay, rows),
    "owner_apply_own_sort_us": apply_own_sort,
    "owner_norm_then_apply_on_its_sort_us": apply_on_norm_sort,
    "owner_norm_sum_apply_us": halves,
    "owner_decay_only_us": lambda: be.adam_apply(opt, pay[:0], rows[:0], norms),
})
emit(what="owner_adam_halves", **shape, entries=B * F, **t)
