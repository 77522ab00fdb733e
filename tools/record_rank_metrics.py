#!/usr/bin/env python
"""record_rank_metrics.py REFERENCE_CHECKOUT [OUT.npz] -- record what the reference's own metric functions return on seeded inputs.

Lifts `_mrr`, `_hit`, `_ndcg` (metrics/NCF_evaluation/ndcg_hr_mrr.py) and `weighted_loss` (metrics/weighted_loss/weighted_loss.py) out of
their modules with `ast` at run time -- the modules themselves import TensorFlow, pandas and a trained model, the four functions are pure
NumPy -- executes them, and writes inputs and results to tests/golden/ref_rank_metrics.npz.  Nothing of the reference's text is in this
file or in the fixture: only the numbers its functions consume and return.

HR / NDCG / MRR@10: blocks of 100 scores with the positive at index 0, pairwise distinct inside each block (the reference sorts with an
unstable quicksort, so a tie would be implementation-defined); the top-10 list is np.argsort(-pred, kind="quicksort")[:10] as at
ndcg_hr_mrr.py:71-75.  Blocks 0, 1, 2 hold the positive at rank 1, 10 and 11.

weighted_loss: users with ties in the scores; user 0 has no positive, user 1 no negative, user 2 pairs whose weights are all zero (NaN: a
float division), the rest are ordinary.  The weights are multiples of 1/8 below 64, so the reference's repeated float64 additions are exact
and do not depend on the order its argsort walks the pairs in.  The samples of all users are interleaved.  wl_mean is sum / len over all
users (weighted_loss.py:81; NaN because of user 2), wl_mean_ordinary the same over the users other than user 2.
"""
import ast
import contextlib
import io
import os
import sys

import numpy as np


def lift(path, names):
    tree = ast.parse(open(path).read(), filename=path)
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    if missing:
        raise SystemExit("%s: no function %s" % (path, ", ".join(missing)))
    return [ns[n] for n in names]


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    ref = argv[1]
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_rank_metrics.npz")
    _mrr, _hit, _ndcg = lift(os.path.join(ref, "metrics", "NCF_evaluation", "ndcg_hr_mrr.py"), ["_mrr", "_hit", "_ndcg"])
    (weighted_loss,) = lift(os.path.join(ref, "metrics", "weighted_loss", "weighted_loss.py"), ["weighted_loss"])
    rng = np.random.default_rng(20181127)

    # ---- blocks of 100, the positive at index 0
    B, n = 48, 100
    blocks = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.float32) / np.float32(128.0) - np.float32(0.25)
    for b, want in enumerate([1, 10, 11]):                       # put the positive at a chosen rank: swap it with the want-th largest
        at = int(np.argsort(-blocks[b], kind="stable")[want - 1])
        blocks[b, 0], blocks[b, at] = blocks[b, at], blocks[b, 0]
    hit, ndcg, mrr = [], [], []
    for b in range(B):
        top = np.argsort(-blocks[b], kind="quicksort")[:10]
        ndcg.append(_ndcg(0, top))
        hit.append(_hit(0, top))
        mrr.append(_mrr(0, top))

    # ---- weighted_loss per user
    U = 24
    uid, label, weight, pred = [], [], [], []
    for u in range(U):
        m = int(rng.integers(3, 40))
        y = (rng.random(m) < 0.35).astype(np.float32)
        if u == 0:
            y[:] = 0.0
        elif u == 1:
            y[:] = 1.0
        elif y.min() == y.max():                                 # an ordinary user holds both classes
            y[0], y[1] = 1.0, 0.0
        w = (rng.integers(0, 512, m) / 8.0).astype(np.float32)
        if u == 2:
            w[:] = 0.0
        p = (rng.integers(0, 12, m) / np.float32(16.0)).astype(np.float32)      # 12 values: ties inside every user
        uid += [1000 + 7 * u] * m
        label.append(y); weight.append(w); pred.append(p)      # noqa: E702
    uid = np.array(uid, np.int64)
    label, weight, pred = np.concatenate(label), np.concatenate(weight), np.concatenate(pred)
    order = rng.permutation(uid.size)                            # interleave the users' samples
    uid, label, weight, pred = uid[order], label[order], weight[order], pred[order]
    users = np.unique(uid)
    losses = []
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(invalid="ignore"):
        for u in users:
            k = uid == u
            losses.append(weighted_loss(label[k].astype(np.float64), weight[k].astype(np.float64), pred[k].astype(np.float64)))
    losses = np.array(losses, np.float64)
    ordinary = users != 1000 + 7 * 2
    np.savez_compressed(out, blk_scores=blocks, blk_hit=np.array(hit, np.float64), blk_ndcg=np.array(ndcg, np.float64),
                        blk_mrr=np.array(mrr, np.float64), hr=np.array(hit).mean(), ndcg=np.array(ndcg).mean(), mrr=np.array(mrr).mean(),
                        wl_uid=uid, wl_label=label, wl_weight=weight, wl_pred=pred, wl_users=users, wl_loss=losses,
                        wl_mean=np.sum(losses) / len(losses), wl_mean_ordinary=np.sum(losses[ordinary]) / int(ordinary.sum()))
    print("%s: %d blocks (hr %.4f ndcg %.4f mrr %.4f), %d users (mean over the ordinary ones %.6f), %d bytes"
          % (out, B, np.mean(hit), np.mean(ndcg), np.mean(mrr), len(users), np.sum(losses[ordinary]) / int(ordinary.sum()), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv)
