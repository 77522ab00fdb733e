"""tools/shard_groups_probe.py (GPU box): what storing ESMM's two sub-models' rows side by side buys on the row-sharded tables
(ShardedTables(groups=2) + attach_linear([rows, 2]); csrc/ids.hip: finish_groups_k / grad_groups_k, csrc/shard_linear.hip: the linear_*
kernels at U = 2, csrc/backward.hip: dir_sparse_ftrl_rows_units_sorted_payload_f32) at world size 1 on ONE GPU, on the headline shape:
B = 65 536 samples x F = 26 slots x 1 M-row tables, K = 16, G = 2, U = 2, uniform ids.

  (a) grouped lookup(want_lin=True)                        against  two ShardedTables with attach_linear, back to back (the only way without
  (b) grouped lookup_train forward + backward              against  row groups: the baseline)
  (c) the new kernels on their own: grouped finish, grouped gradient scatter, the three linear kernels at U = 2, the owner's FTRL over
      U units on its own sort and on the Adagrad step's sort
  (d) the owner gather (dir_gather_slabs_f32) at 128-byte rows (G*K = 32 floats) beside the same gather at 64-byte rows
No exchange runs at world 1 (nothing here measures a link; no N > 1 figure exists on a one-GPU box).  Every measurement: median of --iters
timed runs, HIP events, after at least 0.25 s of the same work as warm-up (the clocks after idle: profiles/NOTES.md R6.3); (a) and (b)
alternate the two versions twice and list both rounds.  One JSON line
per measurement, appended to --out."""
import argparse
import json
import sys
import time

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd.shard import ShardedTables  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--out", default="profiles/shard_groups_probe.jsonl")
ap.add_argument("--only", default="", help="comma-separated subset of: lookup, train, kernels, gather")
args = ap.parse_args()
only = set(filter(None, args.only.split(",")))

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, F, K, V, G, U = args.batch, 26, 16, args.rows, 2, 2
gen = torch.Generator(device=dev).manual_seed(1)
full_g = [[torch.randn((V, K), generator=gen, device=dev) * 0.1 for _ in range(F)] for _ in range(G)]
full_w = [torch.randn((V, U), generator=gen, device=dev) * 0.1 for _ in range(F)]
ids = torch.randint(0, V, (B, F), generator=gen, device=dev)
Gs = [torch.randn((B, F * K), generator=gen, device=dev) for _ in range(G)]
g = torch.randn((B, U), generator=gen, device=dev)
bias = torch.zeros(U, device=dev)
FTRL = dict(lr=0.2, l1=0.001, l2=0.001)
out_f = open(args.out, "a")


def med_us(fn, n=args.iters):
    t0 = time.perf_counter()
    k = 0
    while k < 3 or time.perf_counter() - t0 < 0.25:       # warm-up: the clocks come up under load
        fn()
        torch.cuda.synchronize()
        k += 1
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


def ab(fa, fb, rounds=2):
    """The two versions alternated (A, B, A, B): a difference has to show in every round to count.  -> ([A medians], [B medians])"""
    a, b = [], []
    for _ in range(rounds):
        a.append(round(med_us(fa), 1))
        b.append(round(med_us(fb), 1))
    return a, b


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out_f.write(line + "\n")
    out_f.flush()


def want(name):
    return not only or name in only


shape = dict(world=1, B=B, F=F, K=K, G=G, U=U, rows_per_table=V, iters=args.iters)
grouped = ShardedTables.from_full_groups(full_g).attach_linear_from_full(full_w)
grouped.enable_training(0.05, 0.1).enable_linear_training(**FTRL)
# the baseline: one ShardedTables per sub-model, each with its own first-order weights
pair = [ShardedTables.from_full(full_g[k]).attach_linear_from_full([w[:, k].contiguous() for w in full_w]) for k in range(G)]
for st in pair:
    st.enable_training(0.05, 0.1).enable_linear_training(**FTRL)

if want("lookup"):
    t_g, t_p = ab(lambda: grouped.lookup(ids, want_lin=True, lin_bias=bias),
                  lambda: [st.lookup(ids, want_lin=True, lin_bias=bias[k:k + 1]) for k, st in enumerate(pair)])
    emit(what="lookup_want_lin", **shape, grouped_us=t_g, two_tables_us=t_p, ratio=round(sum(t_g) / sum(t_p), 3))

if want("train"):
    def train_grouped():
        embs, lin = grouped.lookup_train(ids, with_linear=True)
        torch.autograd.backward(list(embs) + [lin], Gs + [g])

    def train_pair():
        for k, st in enumerate(pair):
            emb, lin = st.lookup_train(ids, with_linear=True)
            torch.autograd.backward([emb, lin], [Gs[k], g[:, k:k + 1]])
    t_g, t_p = ab(train_grouped, train_pair)
    emit(what="lookup_train_forward_backward", **shape, grouped_us=t_g, two_tables_us=t_p, ratio=round(sum(t_g) / sum(t_p), 3))

if want("kernels") or want("gather"):
    be = grouped.backend
    plan = grouped._plan(B, "train")
    grouped.lookup_train(ids, with_linear=True)            # fills the plan's slabs and inverse positions (no backward: nothing moves)
    torch.cuda.synchronize()
    cap = plan.cap
    inv2d = be.inv2d(plan.inv[0], B, F, False)

if want("kernels"):
    lrows, lback = plan.lin_buffers(U)
    outs = [torch.empty((B, F * K), device=dev) for _ in range(G)]
    lin = torch.empty((B, U), device=dev)
    send = torch.empty((cap, G * K), device=dev)
    lsend = torch.empty(cap * U, device=dev)
    t_fin = med_us(lambda: be.finish_groups(plan.back[0], inv2d, K, outs))
    t_grad = med_us(lambda: be.grad_groups(Gs, inv2d, K, send))
    t_lg = med_us(lambda: be.linear_gather(plan.recv[0], cap, lrows[0]))
    t_lf = med_us(lambda: be.linear_finish(lback[0], inv2d, bias, lin))
    t_ls = med_us(lambda: be.linear_grad(g, inv2d, lsend))
    # the finish pass the parent commit would run twice: one gather per sub-model's [n, K] buffer
    b_st = pair[0]
    b_plan = b_st._plan(B, "train")
    b_st.lookup_train(ids)
    torch.cuda.synchronize()
    b_inv = b_st.backend.inv2d(b_plan.inv[0], B, F, False)
    t_fin1 = med_us(lambda: b_st.backend.finish_chunk(b_plan.back[0], b_inv, False, outs[0], None))
    hdr = int(plan.recv[0][0]) & 0xffffffff
    pay = plan.recv[0][1:].clone()
    pay[hdr:] = -1
    grad_rows = torch.randn((cap, G * K), generator=gen, device=dev)

    def both():
        be.apply_adagrad(grouped.optimizer, pay, grad_rows)
        be.apply_ftrl(pay, lsend, FTRL["lr"], FTRL["l1"], FTRL["l2"], sorted_by=grouped.optimizer)
    t_a = med_us(lambda: be.apply_adagrad(grouped.optimizer, pay, grad_rows))
    t_own = med_us(lambda: be.apply_ftrl(pay, lsend, FTRL["lr"], FTRL["l1"], FTRL["l2"]))
    t_both = med_us(both)
    emit(what="groups_kernels", **shape, slab_slots=cap, finish_groups_us=round(t_fin, 1), finish_one_table_us=round(t_fin1, 1),
         grad_groups_us=round(t_grad, 1), linear_gather_units_us=round(t_lg, 1), linear_finish_units_us=round(t_lf, 1),
         linear_grad_units_us=round(t_ls, 1), owner_adagrad_width_GK_us=round(t_a, 1), owner_ftrl_units_own_sort_us=round(t_own, 1),
         owner_adagrad_then_ftrl_units_on_its_sort_us=round(t_both, 1), owner_ftrl_units_on_adagrad_sort_us=round(t_both - t_a, 1))

if want("gather"):
    b_st = pair[0]
    b_plan = b_st._plan(B, "train")
    b_st.lookup_train(ids)
    torch.cuda.synchronize()
    t128 = med_us(lambda: be.gather_slabs(plan.recv[0], cap, plan.rows[0]))
    t64 = med_us(lambda: b_st.backend.gather_slabs(b_plan.recv[0], b_plan.cap, b_plan.rows[0]))
    n = B * F
    emit(what="owner_gather_row_width", **shape, rows_gathered=n, gather_128B_rows_us=round(t128, 1), gather_64B_rows_us=round(t64, 1),
         two_64B_gathers_us=round(2 * t64, 1), gather_128B_GBps=round(2 * n * 128 / t128 / 1e3, 1), gather_64B_GBps=round(2 * n * 64 / t64 / 1e3, 1))
