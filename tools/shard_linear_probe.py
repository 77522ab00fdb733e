"""tools/shard_linear_probe.py (GPU box): what DeepFM's first-order term costs on the row-sharded tables (ShardedTables.attach_linear;
csrc/shard_linear.hip, csrc/backward.hip: dir_sparse_ftrl_rows_sorted_payload_f32) at world size 1 on ONE GPU, on the headline shape:
B = 65 536 samples x F = 26 slots x 1 M-row tables, K = 16, uniform ids.

  (a) lookup(want_fm=True) without and with want_lin                      -> the term's added forward time
  (b) lookup_train forward + backward without and with with_linear         -> the term's added training time (its FTRL step reuses the
                                                                              Adagrad step's sort of the payload)
  (c) ops.linear_logit on TableSet.ftrl_rows (the single-GPU forward)     -- the yardsticks that exist without the shards
  (d) ops.SparseFtrl.step on the same ids (the single-GPU update)
  and the three new kernels on their own (owner gather, requester finish, requester gradient scatter) plus the owner's FTRL call with its
  own sort and on the Adagrad step's sort.
No exchange runs at world 1 (nothing here measures a link).  Prints one JSON line per measurement: median of --iters timed runs after 3
warm-up runs, HIP events."""
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
ap.add_argument("--only", default="", help="comma-separated subset of: lookup, train, single, kernels (for a rocprofv3 --kernel-trace --stats pass)")
args = ap.parse_args()
only = set(filter(None, args.only.split(",")))

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, F, K, V = args.batch, 26, 16, args.rows
vocab = [V] * F
gen = torch.Generator(device=dev).manual_seed(1)
full = [torch.randn((V, K), generator=gen, device=dev) * 0.1 for _ in range(F)]
full_w = [torch.randn((V,), generator=gen, device=dev) * 0.1 for _ in range(F)]
ids = torch.randint(0, V, (B, F), generator=gen, device=dev)
G = torch.randn((B, F * K), generator=gen, device=dev)
g = torch.randn((B, 1), generator=gen, device=dev)
bias = torch.zeros(1, device=dev)
FTRL = dict(lr=0.2, l1=0.001, l2=0.001)


def med_us(fn, n=args.iters):
    ts = []
    for i in range(n + 3):
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


def want(name):
    return not only or name in only


shape = dict(world=1, B=B, F=F, K=K, rows_per_table=V)
st = ShardedTables.from_full(full).attach_linear_from_full(full_w)
st.enable_training(0.05, 0.1).enable_linear_training(**FTRL)

if want("lookup"):
    t0 = med_us(lambda: st.lookup(ids, want_fm=True))
    t1 = med_us(lambda: st.lookup(ids, want_fm=True, want_lin=True, lin_bias=bias))
    emit(what="sharded_lookup_fm", **shape, without_lin_us=round(t0, 1), with_lin_us=round(t1, 1), added_us=round(t1 - t0, 1))

if want("train"):
    def train(with_linear):
        if with_linear:
            emb, lin = st.lookup_train(ids, with_linear=True)
            torch.autograd.backward([emb, lin], [G, g])
        else:
            st.lookup_train(ids).backward(G)
    t0 = med_us(lambda: train(False))
    t1 = med_us(lambda: train(True))
    emit(what="sharded_lookup_train_forward_backward", **shape, without_linear_us=round(t0, 1), with_linear_us=round(t1, 1),
         added_us=round(t1 - t0, 1))

if want("single"):
    rows = ops.TableSet.ftrl_rows(full_w)
    t_c = med_us(lambda: ops.linear_logit(rows, ids, bias=bias))
    single = ops.SparseFtrl(rows, FTRL["lr"], l1=FTRL["l1"], l2=FTRL["l2"])
    t_d = med_us(lambda: single.step(ids, g))
    emit(what="single_gpu_linear", **shape, linear_logit_us=round(t_c, 1), sparse_ftrl_step_us=round(t_d, 1))
    del rows, single

if want("kernels"):
    be = st.backend
    plan = st._plan(B, "train")
    st.lookup_train(ids, with_linear=True)                 # fills the plan's slabs and inverse positions (no backward: nothing moves)
    torch.cuda.synchronize()
    cap = plan.cap
    lrows, lback = plan.lin_buffers()
    inv2d = be.inv2d(plan.inv[0], B, F, False)
    lin = torch.empty((B, 1), device=dev)
    t_g = med_us(lambda: be.linear_gather(plan.recv[0], cap, lrows[0]))
    t_f = med_us(lambda: be.linear_finish(lback[0], inv2d, bias, lin))
    send = torch.empty(cap, device=dev)
    t_s = med_us(lambda: be.linear_grad(g, inv2d, send))
    hdr = int(plan.recv[0][0]) & 0xffffffff
    pay = plan.recv[0][1:].clone()
    pay[hdr:] = -1
    grad_rows = torch.randn((cap, K), generator=gen, device=dev)

    def both(reuse):
        be.apply_adagrad(st.optimizer, pay, grad_rows)
        be.apply_ftrl(pay, send, FTRL["lr"], FTRL["l1"], FTRL["l2"], sorted_by=st.optimizer if reuse else None)
    t_a = med_us(lambda: be.apply_adagrad(st.optimizer, pay, grad_rows))
    t_own = med_us(lambda: be.apply_ftrl(pay, send, FTRL["lr"], FTRL["l1"], FTRL["l2"]))
    t_both = med_us(lambda: both(True))
    emit(what="shard_linear_kernels", **shape, slab_slots=cap, owner_gather_us=round(t_g, 1), requester_finish_us=round(t_f, 1),
         requester_grad_scatter_us=round(t_s, 1), owner_ftrl_own_sort_us=round(t_own, 1), owner_adagrad_us=round(t_a, 1),
         owner_adagrad_then_ftrl_on_its_sort_us=round(t_both, 1), owner_ftrl_on_adagrad_sort_us=round(t_both - t_a, 1))
