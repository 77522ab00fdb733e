"""tools/shared_embedding_probe.py (GPU box): what a table shared between two slots costs the sorted sparse Adagrad step
(feature_column.shared_embedding_columns; csrc/backward.hip: dir_sparse_adagrad_sorted_shared_f32 / _rows_shared_f32) on the headline
shape: B = 65 536 samples x F = 26 slots x 1 M-row tables, K = 16, uniform ids.

  unshared   26 tables, the slot-major sort (ids [B, F] with B >= 4096)
  shared     25 tables, slots 0 and 1 on one of them: keys over the distinct tables, the global sort
  identity   the unshared set through the shared export with an identity map: the global sort alone, nothing shared
for the plain layout (step) and the packed training rows with the FM backward folded in (step_fm).
Prints one JSON line per measurement: median of --iters timed runs after 3 warm-up runs, HIP events."""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import ops, _lib  # noqa: E402
from dir_amd._abi import _ptr, _stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--rows", type=int, default=1_000_000)
args = ap.parse_args()

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, F, K, V = args.batch, 26, 16, args.rows
gen = torch.Generator(device=dev).manual_seed(1)
ids = torch.randint(0, V, (B, F), generator=gen, device=dev)
G = torch.randn((B, F * K), generator=gen, device=dev) * 0.1
fm_g = torch.randn((B, 1), generator=gen, device=dev) * 0.1


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


def tables(shared):
    tabs = [torch.randn((V, K), generator=gen, device=dev) * 0.1 for _ in range(F - 1 if shared else F)]
    return [tabs[0]] + tabs if shared else tabs


def identity_step(opt):
    ts, lib = opt.ts, _lib.load()
    ident = torch.arange(F, dtype=torch.int32, device=dev)
    ws, need, _ = opt._sort_area("probe", lib.dir_sparse_adagrad_sorted_workspace_bytes, B, F, K)

    def fn():
        _lib.check(lib.dir_sparse_adagrad_sorted_shared_f32(_ptr(ts.ptrs), _ptr(opt.acc_ptrs), F, K, _ptr(ids), ids.stride(0), ids.stride(1),
                                                            _ptr(G), G.stride(0), opt.lr, B, _ptr(opt.row_base), opt.total_rows, _ptr(ident), F,
                                                            ws, need, _stream()))
    return fn


out = dict(what="sparse_adagrad_step_shared_tables", B=B, F=F, K=K, rows_per_table=V, sharing_slots=2)
for name, shared in (("unshared", False), ("shared", True)):
    opt = ops.SparseAdagrad(ops.TableSet(tables(shared)), lr=0.05)
    out["plain_%s_us" % name] = round(med_us(lambda: opt.step(ids, G)), 1)
    if not shared:
        out["plain_identity_map_us"] = round(med_us(identity_step(opt)), 1)
    del opt
    ts = ops.TableSet.train_rows(tables(shared), 0.1)
    opt = ops.SparseAdagrad(ts, lr=0.05)
    fsum = torch.empty((B, K), device=dev)
    ops.gather_fm(ts, ids, fsum=fsum)
    out["packed_fm_%s_us" % name] = round(med_us(lambda: opt.step_fm(ids, G, fm_g, fsum)), 1)
    del opt, ts
print(json.dumps(out), flush=True)
