"""tools/shard_xdeepfm_probe.py (GPU box): what the first-order term costs on the de-duplicated training exchange, in the manner of
tools/shard_din_probe.py, on BASELINE config 5's batch: B = 65 536 samples x 26 slots, K = 16, world 1 (one rank: the slabs hold the whole
batch; nothing here measures a link), uniform and Zipf(1.05) ids (tools/dedup_probe.py's generator) over --vocab rows per slot.

  (a) fused_us     dir_rows_scatter_sum_side_f32: the gradient slab and the first-order slab from ONE key pass, sort and run discovery,
                   d lin [B, 1] read in place (side_div = 26);
  (b) parent_us    the same two slabs the way the code before this entry could form them: the [n, 1] expansion of d lin
                   (repeat_interleave, timed: expand_us), dir_rows_scatter_sum_f32 at K (rows_us) and again at K = 1 on the expansion
                   (side_us) -- two key passes, two sorts.  (a) and (b) run ALTERNATELY, one after the other per iteration;
  (c) step_us      the whole ShardedXDeepFMTrainer.step (CIN 3 x 128, tower 400-400, linear=) with dedup on and off, beside
                   ShardedDeepFMTrainer.step with the same settings.
Prints one JSON line per measurement -- median, min and max of --iters timed runs after 3 warm-up runs, HIP events -- and appends them to
profiles/shard_xdeepfm_probe.jsonl."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--vocab", type=int, default=1_000_000, help="rows per slot")
ap.add_argument("--skip-steps", action="store_true", help="(a) and (b) only")
ap.add_argument("--out", default="profiles/shard_xdeepfm_probe.jsonl")
args = ap.parse_args()

dir_amd.load_library()
dev = torch.device("cuda", 0)
B, F, K, V = args.batch, 26, 16, args.vocab
n = B * F
gen = torch.Generator(device=dev).manual_seed(1)
LINES = []


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(ts):
    ts = sorted(ts)
    return dict(med=round(ts[len(ts) // 2], 1), min=round(ts[0], 1), max=round(ts[-1], 1))


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def draw(dist):
    if dist == "uniform":
        return torch.randint(0, V, (B, F), generator=gen, device=dev)
    u = torch.rand((B, F), generator=gen, device=dev, dtype=torch.float64)
    a = 1.05
    return ((V ** (1 - a) - 1) * u + 1).pow(1 / (1 - a)).floor().long().clamp_(1, V) - 1


vdev = torch.tensor([V] * F, dtype=torch.int64, device=dev)
G = torch.randn((n, K), generator=gen, device=dev)
g_lin = torch.randn((B, 1), generator=gen, device=dev)
batches = {dist: draw(dist) for dist in ("uniform", "zipf1.05")}

for dist, ids in batches.items():
    cap = n
    for rep in range(2):                                 # roomy first, then this batch's demand + 5 %
        payload = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        inv = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.empty(1, dtype=torch.int64, device=dev)
        over = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.zeros(128, dtype=torch.int32, device=dev)
        ops.shard_bucket_cap_dedup(ids, vdev, 1, cap, payload, inv, counts, over, ws)
        torch.cuda.synchronize()
        sent = int(counts.sum())
        if rep == 0:
            cap = int(sent * 1.05) // 16 * 16 + 64
    assert not int(over), "the second pass's slab must hold the batch"
    R = cap
    idx = inv.view(F, B).t().reshape(-1).contiguous()    # entry b * F + f: what the backward hands the scatter-sum
    out, out_side = torch.empty((R, K), device=dev), torch.empty((R, 1), device=dev)
    out2, side2 = torch.empty((R, K), device=dev), torch.empty((R, 1), device=dev)
    box = {}

    def fused():
        ops.rows_scatter_sum_side(idx, G, g_lin, F, R, out=out, out_side=out_side)

    def expand():
        box["e"] = g_lin.repeat_interleave(F, 0)

    def rows():
        ops.rows_scatter_sum(idx, G, R, out=out2)

    def side():
        ops.rows_scatter_sum(idx, box["e"], R, out=side2)

    ta, tb, te, tr, ts_ = [], [], [], [], []
    for i in range(args.iters + 3):
        a = timed(fused)
        e, r, s = timed(expand), timed(rows), timed(side)
        if i >= 3:
            ta.append(a), tb.append(e + r + s), te.append(e), tr.append(r), ts_.append(s)
    assert torch.equal(out, out2) and torch.equal(out_side, side2), "the fused call and the two plain calls differ in bits"
    emit(what="first_order_slab", ids=dist, B=B, F=F, K=K, entries=n, positions=sent, travel=round(sent / n, 4), fused_us=stats(ta),
         parent_us=stats(tb), expand_us=stats(te), rows_us=stats(tr), side_us=stats(ts_))
    del payload, inv, idx, out, out_side, out2, side2, box
    torch.cuda.empty_cache()

if not args.skip_steps:
    from dir_amd import feature_column as fc
    from dir_amd.deepfm import DeepFM
    from dir_amd.shard import ShardedDeepFMTrainer, ShardedTables, ShardedXDeepFMTrainer
    from dir_amd.xdeepfm import XDeepFM
    ftrl = dict(lr=0.05, l1=0.0, l2=0.0)
    labels = torch.randint(0, 2, (B, 1), generator=gen, device=dev).float()
    sparse = ("embedding_weights", "linear_weights")
    for kind in ("xdeepfm", "deepfm"):
        for dedup in (True, False):
            cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
            cols = [fc.embedding_column(c, K) for c in cats]
            torch.manual_seed(7)
            if kind == "xdeepfm":
                model = XDeepFM(linear_feature_columns=cats, dnn_feature_columns=cols, cin_layer_sizes=(128, 128, 128), dnn_hidden_units=(400, 400)).to(dev)
            else:
                model = DeepFM(linear_feature_columns=cats, dnn_feature_columns=cols, dnn_hidden_units=[400, 400], fm_embedding_size=K).to(dev)
            dense = [p for name, p in model.named_parameters() if not name.startswith(sparse) and name != "linear_bias"]
            opt = torch.optim.Adagrad(dense, lr=0.01)
            tables = ShardedTables.from_full([p.data for p in model.embedding_weights])
            tables.attach_linear_from_full([p.data for p in model.linear_weights])
            cls = ShardedXDeepFMTrainer if kind == "xdeepfm" else ShardedDeepFMTrainer
            tr_ = cls(model, tables, 0.05, opt, linear=ftrl, dedup=dedup)
            for dist, ids in batches.items():
                ts = [timed(lambda: tr_.step(ids, labels)) for _ in range(args.iters + 3)][3:]
                emit(what="trainer_step", trainer=cls.__name__, ids=dist, dedup=dedup, B=B, F=F, K=K, step_us=stats(ts))
            del model, tables, tr_, opt, dense
            torch.cuda.empty_cache()

os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "a") as fh:
    fh.write("\n".join(LINES) + "\n")
