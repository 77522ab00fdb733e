"""tools/shard_bags_adam_probe.py (GPU box): what one multi-hot training lookup costs under the owner-side sparse Adam of the row-sharded
tables (ShardedTables.lookup_bags_train under enable_training_adam; csrc/backward.hip: dir_sparse_adam_bags_norm_f32 /
dir_sparse_adam_bags_apply_f32) at world size 1 on ONE GPU: B = 65 536 samples x F = 26 slots x 1 M-row tables, K = 16, bags of 1..5
entries (mean 3), ids uniform and Zipf(1.05).

  bags_adam        lookup_bags_train forward + backward under Adam, clip_norm = 100 (norm pass + apply + decay pass) and clip_norm = 0
  (1) bags_adagrad the same call under Adagrad (code this change leaves alone: the parent's number)
  (2) onehot_adam  the one-hot lookup_train forward + backward under Adam on the same box (DESIGN.md 5.3's table)
  and the owner's halves on the records and gradient rows of one lookup: the norm half, the apply half with a sort of its own, norm +
  apply on the norm half's sort, the decay pass alone, and the Adagrad bag step's owner pass over the same records.
The decay pass streams every row of var, m and v in and out (26 x 1 M x 16 x 4 B x 6 = 10 GB) and bounds every Adam figure from below.
No exchange runs at world 1 (nothing here measures a link).  The comparands alternate inside one timed loop (other work shares the
host); prints one JSON line per measurement: median of --iters timed runs after 3 warm-up runs of every comparand, HIP events."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd.shard import ShardedTables  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=15)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dist", default="uniform,zipf")
args = ap.parse_args()

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, F, K, V = args.batch, 26, 16, args.rows
gen = torch.Generator(device=dev).manual_seed(1)
full = [torch.randn((V, K), generator=gen, device=dev) * 0.1 for _ in range(F)]
G = torch.randn((B, F * K), generator=gen, device=dev) * 0.01
B1, B2, EPS, LR_T = 0.9, 0.999, 1e-4, 0.003


def draw_ids(n, dist):
    if dist == "uniform":
        return torch.randint(0, V, (n,), generator=gen, device=dev)
    # Zipf(1.05) over the V rows: inverse CDF of p(r) ~ r^-1.05 on the device
    cdf = torch.cumsum(torch.arange(1, V + 1, device=dev, dtype=torch.float64) ** -1.05, 0)
    u = torch.rand(n, generator=gen, device=dev, dtype=torch.float64) * cdf[-1]
    return torch.searchsorted(cdf, u).clamp_(max=V - 1)


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
st_clip, st_noclip, st_one = sharded_adam(100.0), sharded_adam(0.0), sharded_adam(100.0)
st_ada = ShardedTables.from_full([t.clone() for t in full]).enable_training(0.05, 0.1)

for dist in args.dist.split(","):
    lens = torch.randint(1, 6, (B * F,), generator=gen, device=dev)                    # bag (b, f) = b * F + f, 1..5 entries
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    nnz = int(offsets[-1])
    values = draw_ids(nnz, dist)
    ids = draw_ids(B * F, dist).view(B, F)
    kw = dict(combiner="mean")
    t = alternate_us({
        "bags_adam_clip100_us": lambda: st_clip.lookup_bags_train(values, offsets, **kw).backward(G),
        "bags_adam_noclip_us": lambda: st_noclip.lookup_bags_train(values, offsets, **kw).backward(G),
        "bags_adagrad_us": lambda: st_ada.lookup_bags_train(values, offsets, **kw).backward(G),
        "onehot_adam_clip100_us": lambda: st_one.lookup_train(ids).backward(G),
        "bags_forward_only_us": lambda: st_ada.lookup_bags(values, offsets, **kw),
    })
    emit(what="lookup_bags_train_forward_backward", ids=dist, entries=nnz, **shape, **t,
         adam_excess_over_adagrad_us=round(t["bags_adam_clip100_us"] - t["bags_adagrad_us"], 1), decay_pass_bytes=F * V * K * 4 * 6)

    # the owner's halves on the records and gradient rows of one lookup (every record live at world 1)
    be, opt = st_clip.backend, st_clip.optimizer
    emb = st_clip.lookup_bags_train(values, offsets, **kw)
    plan = emb.grad_fn.saved[0]
    emb.backward(G)                                                                    # leaves the gradient rows in plan.back
    rec = (plan.recv, plan.cap_e, plan.cap_b, plan.back, None)
    norms = st_clip._sum_norm_shares(be.bags_adam_norm(opt, *rec))
    emb_a = st_ada.lookup_bags_train(values, offsets, **kw)
    plan_a = emb_a.grad_fn.saved[0]
    emb_a.backward(G)
    pay0 = torch.zeros(0, dtype=torch.int64, device=dev)
    rows0 = torch.zeros((0, K), dtype=torch.float32, device=dev)

    def apply_own_sort():
        opt.forget_sort()                                      # forget the norm half's sort of these slabs: key pass + sort run again
        be.bags_adam_apply(opt, *rec, norms)

    def apply_on_norm_sort():
        be.bags_adam_norm(opt, *rec)                           # (timed with it: the difference to the norm half alone is the apply)
        be.bags_adam_apply(opt, *rec, norms)

    t = alternate_us({
        "owner_norm_half_us": lambda: be.bags_adam_norm(opt, *rec),
        "owner_apply_own_sort_us": apply_own_sort,
        "owner_norm_then_apply_on_its_sort_us": apply_on_norm_sort,
        "owner_decay_only_us": lambda: be.adam_apply(opt, pay0, rows0, norms),
        "owner_adagrad_bags_us": lambda: st_ada.backend.bags_adagrad(st_ada.optimizer, plan_a.recv, plan_a.cap_e, plan_a.cap_b, plan_a.back, None),
    })
    emit(what="owner_bag_adam_halves", ids=dist, entries=nnz, entry_slots=plan.cap_e, **shape, **t,
         apply_on_norm_sort_us=round(t["owner_norm_then_apply_on_its_sort_us"] - t["owner_norm_half_us"], 1),
         excess_over_decay_us=round(t["owner_norm_then_apply_on_its_sort_us"] - t["owner_decay_only_us"], 1))
