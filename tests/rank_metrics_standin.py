"""The definitions behind ops.group_rank_stats and metrics.GroupedMetrics as literal loops in float64 NumPy: what the HIP kernel and the
class are tested against.  Nothing here is vectorised on purpose -- every line is the sentence of include/dir_hip.h it stands for."""
import numpy as np

INT_STATS = ("n_pos", "n_neg", "gt", "eq", "rank")
STATS = ("n_pos", "n_neg", "gt", "eq", "mis_w", "tot_w", "rank")


def group_stats(scores, labels, weights, offsets):
    """scores / labels / weights (None: ones) flat, offsets [G + 1] -> dict of the seven per-group arrays."""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels, dtype=np.float32)
    w = np.ones(s.shape, np.float32) if weights is None else np.asarray(weights, dtype=np.float32)
    off = [int(o) for o in np.asarray(offsets)]
    G = len(off) - 1
    out = {k: np.zeros(G, np.int64) for k in INT_STATS}
    out.update(mis_w=np.zeros(G, np.float64), tot_w=np.zeros(G, np.float64))
    sl, yl = s.tolist(), y.tolist()                       # fp32 values as Python floats: the compares are those of the fp32 values
    for g in range(G):
        ent = range(off[g], off[g + 1])
        P = [i for i in ent if yl[i] > 0.5]
        N = [j for j in ent if not yl[j] > 0.5]
        n_neg = len(N)
        gt = eq = 0
        mis = tot = np.float64(0.0)
        for i in P:
            a = e = 0
            for j in N:
                if sl[j] > sl[i]:
                    a += 1
                elif sl[j] == sl[i]:
                    e += 1
            gt += n_neg - a - e
            eq += e
            mis = mis + np.float64(w[i]) * np.float64(a + e)
            tot = tot + np.float64(w[i]) * np.float64(n_neg)
        rank = 0
        if len(P) == 1:
            i = P[0]
            rank = 1
            for j in ent:
                if j != i and (sl[j] > sl[i] or (j < i and sl[j] == sl[i])):
                    rank += 1
        out["n_pos"][g], out["n_neg"][g], out["gt"][g], out["eq"][g], out["rank"][g] = len(P), n_neg, gt, eq, rank
        out["mis_w"][g], out["tot_w"][g] = mis, tot
    return out


def stable_rank(scores, i):
    """1 + the position of entry i in np.argsort(-scores, kind="stable")."""
    order = np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")
    return 1 + int(np.where(order == i)[0][0])


def aggregate(st, k=10):
    """The dict GroupedMetrics.result() returns, from the per-group statistics."""
    G = len(st["n_pos"])
    num = den = 0.0
    gauc_groups = ranking_groups = 0
    losses, hr, ndcg, mrr = [], [], [], []
    for g in range(G):
        n_pos, n_neg = int(st["n_pos"][g]), int(st["n_neg"][g])
        if n_pos > 0 and n_neg > 0:
            auc = (float(st["gt"][g]) + float(st["eq"][g]) / 2.0) / float(n_pos * n_neg)
            num += (n_pos + n_neg) * auc
            den += n_pos + n_neg
            gauc_groups += 1
            with np.errstate(invalid="ignore"):
                losses.append(np.float64(st["mis_w"][g]) / np.float64(st["tot_w"][g]))
        else:
            losses.append(np.float64(0.0))
        if n_pos == 1:
            r = int(st["rank"][g])
            ranking_groups += 1
            hit = r <= k
            hr.append(1.0 if hit else 0.0)
            ndcg.append(1.0 / np.log2(r + 1.0) if hit else 0.0)
            mrr.append(1.0 / r if hit else 0.0)
    mean = lambda v: float(np.sum(np.array(v, np.float64)) / len(v)) if v else 0.0  # noqa: E731
    return {"gauc": num / den if den > 0 else 0.0, "gauc_groups": gauc_groups, "weighted_loss": mean(losses),
            "hr@%d" % k: mean(hr), "ndcg@%d" % k: mean(ndcg), "mrr@%d" % k: mean(mrr), "ranking_groups": ranking_groups, "groups": G}


def ragged(seed, sizes, score_values=None, pos_rate=0.3, int_weights=True):
    """Seeded flat inputs for groups of the given sizes -> scores, labels, weights (float32), offsets (int64).  score_values: draw the scores
    from that many distinct values (ties everywhere); None: pairwise distinct inside the whole input."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    n = int(sizes.sum())
    if score_values:
        scores = (rng.integers(0, score_values, n) / np.float32(8.0)).astype(np.float32)
    else:
        assert n < (1 << 20)                                # i / n are then distinct fp32 values
        scores = (rng.permutation(n) / np.float32(max(n, 1))).astype(np.float32)
    labels = (rng.random(n) < pos_rate).astype(np.float32)
    weights = rng.integers(0, 8, n).astype(np.float32) if int_weights else rng.random(n).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return scores, labels, weights, offsets
