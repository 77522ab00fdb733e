"""shared_adam_probe.py -- what sharing one embedding table between two columns costs the DCN training step (BASELINE config 3: 26 id
columns of 10^6 ids x 16, 13 numeric columns, cross x 3, 1024-1024, BN; Adam, epsilon 1e-4, clip_by_norm 100, cosine decay) at
B = 65 536: `shared` puts C00 and C01 on one table through feature_column.shared_embedding_columns (25 tables), `unshared` is config 3.

    python tools/shared_adam_probe.py --variant shared                       # one process, one figure: this tree's eager step time (ms)
    python tools/shared_adam_probe.py --compare /path/to/parent_tree --runs 6 # parent shared, head shared, head unshared, alternating
    python tools/shared_adam_probe.py --bench /path/to/parent_tree --runs 3   # bench.py --workload dcn_train, parent and head alternating

The baseline of a comparison is another checkout (the parent commit, built), never this code under another switch: --compare starts
`python tools/shared_adam_probe.py` of THIS file with --root <tree> for each side in turn, the order reversed every other run, so all
sides see the same clocks and the same neighbours, and prints the min-max of the runs' medians.  Before dir_sparse_adam_shared_f32 a
group with a shared table lost the HIP Adam (dense gradient + torch Adam over every table of the group): that is what `parent shared`
times.  Each run: warm-up steps, then `blocks` timed blocks of `steps` steps between two device events; the figure is the median block's
time per step (a fresh process timed right after start-up reads 10-15 % slow on the matrix-bound kernels: profiles/NOTES.md R6.3).
--bench runs `python bench.py --gpus 1 --workload dcn_train` in each tree's own directory and compares the slowest runs.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SPREAD = 0.06          # README: another box reads +- 3-6 %


def build_step(variant, B, torch, device):
    from dir_amd import feature_column as fc
    from dir_amd.dcn import DeepCrossNetwork
    F, K, V = 26, 16, 1000000
    gen = torch.Generator(device=device).manual_seed(1)
    idsl = [torch.randint(0, V, (B, F), generator=gen, device=device) for _ in range(4)]
    labels = (torch.rand((B, 1), generator=gen, device=device) < 0.25).float()
    cats = [fc.categorical_column_with_identity("C%02d" % i, V) for i in range(F)]
    if variant == "shared":
        cols = fc.shared_embedding_columns(cats[:2], K) + [fc.embedding_column(c, K) for c in cats[2:]]
    else:
        cols = [fc.embedding_column(c, K) for c in cats]
    cols += [fc.numeric_column("I%02d" % i) for i in range(13)]
    model = DeepCrossNetwork(columns=cols, cross_layer_num=3, dnn_hidden_units=[1024, 1024], batch_norm=True, optimizer="Adam",
                             optimizer_spec={"epsilon": 1e-4},
                             learning_rate_spec={"learning_rate": 0.001, "decay_method": "cosine_decay", "decay_steps": 3000,
                                                 "alpha": 0.5}).to(device)
    train_op = model.train_step()
    dense = torch.rand((B, 13), generator=gen, device=device)
    feats = []
    for ids in idsl:
        f = {"C%02d" % i: ids[:, i].contiguous() for i in range(F)}
        f.update({"I%02d" % i: dense[:, i].contiguous() for i in range(13)})
        feats.append(f)
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def step(i):
        train_op(bce(model(feats[i % len(feats)]), labels))

    model.train()
    hip_tables = sum(len(getattr(o, "owned", ())) for o in train_op.sparse_adam)
    return step, hip_tables, len(model.input_layer.embedding_weights)


def measure(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import dir_amd
    assert os.path.abspath(os.path.dirname(dir_amd.__file__)).startswith(os.path.abspath(args.root)), dir_amd.__file__
    device = torch.device("cuda")
    step, hip_tables, tables = build_step(args.variant, args.batch, torch, device)
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    times = []
    for b in range(args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            step(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / args.steps)
    times.sort()
    print(json.dumps({"variant": args.variant, "batch": args.batch, "ms_per_step": round(times[len(times) // 2], 4),
                      "blocks_ms": [round(t, 4) for t in times], "tables": tables, "tables_on_the_hip_adam": hip_tables,
                      "root": os.path.abspath(args.root)}))


def _child(cmd, cwd, timeout, what):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    if r.returncode != 0:                      # a failed child ends the comparison: nothing more is started on the GPU
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit("shared_adam_probe: %s failed with exit code %d" % (what, r.returncode))
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


def compare(args):
    parent, head = os.path.abspath(args.compare), os.path.abspath(args.root)
    sides = (("parent shared", parent, "shared"), ("head shared", head, "shared"), ("head unshared", head, "unshared"))
    results = {}
    for run in range(args.runs):
        for side, root, variant in (sides if run % 2 == 0 else sides[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--variant", variant, "--batch", str(args.batch), "--steps",
                   str(args.steps), "--warmup", str(args.warmup), "--blocks", str(args.blocks)]
            line = _child(cmd, None, args.child_timeout, side)
            results.setdefault(side, []).append(line["ms_per_step"])
            print(json.dumps(dict(line, side=side, run=run)), flush=True)
    print("side            ms per step (min-max of %d runs)" % args.runs)
    for side, v in results.items():
        print("%-15s %8.3f - %-8.3f" % (side, min(v), max(v)))
    floor, shared = results["head unshared"], results["head shared"]
    print(json.dumps({"head_shared_over_head_unshared": [round(min(shared) / min(floor), 4), round(max(shared) / max(floor), 4)],
                      "within_the_box_to_box_spread": max(shared) <= max(floor) * (1 + SPREAD),
                      "parent_shared_over_head_shared": round(min(results["parent shared"]) / min(shared), 3)}))


def bench(args):
    sides = (("parent", os.path.abspath(args.bench)), ("head", os.path.abspath(args.root)))
    results = {}
    for run in range(args.runs):
        for side, root in (sides if run % 2 == 0 else sides[::-1]):
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--workload", "dcn_train", "--steps", str(args.steps), "--warmup", str(args.warmup)]
            line = _child(cmd, root, args.child_timeout, "bench.py in the %s tree" % side)
            results.setdefault(side, []).append(line["ms_per_step"])
            print(json.dumps({"side": side, "run": run, "ms_per_step": line["ms_per_step"]}), flush=True)
    for side, v in results.items():
        print("%-7s bench.py dcn_train ms per step: %8.3f - %-8.3f" % (side, min(v), max(v)))
    print(json.dumps({"head_slowest_over_parent_slowest": round(max(results["head"]) / max(results["parent"]), 4),
                      "no_regression": max(results["head"]) <= max(results["parent"]) * (1 + SPREAD)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the tree whose dir_amd is measured (default: this file's)")
    ap.add_argument("--variant", choices=("shared", "unshared"), default="shared")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--compare", default=None, metavar="PARENT_TREE", help="a built checkout of the parent commit")
    ap.add_argument("--bench", default=None, metavar="PARENT_TREE", help="bench.py's DCN training line in both trees")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    args = ap.parse_args()
    if args.compare:
        compare(args)
    elif args.bench:
        bench(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
