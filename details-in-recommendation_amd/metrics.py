"""metrics.py -- the evaluation metrics of the reference's model_fns, as streaming accumulators on the device.

Mirrors `_get_metric_op` (models/DeepCrossNetwork/DeepCrossNetwork.py:293-319; the canned head of DeepFM and
ESMM.py:178-215 report the same family): average_loss = tf.metrics.mean(unweighted_loss, weights), accuracy / precision /
recall of class_ids against the labels (weighted), accuracy_baseline = max(label mean, 1 - label mean), and auc =
[TF-upstream] tf.metrics.auc with its defaults -- 200 thresholds (0, 1 and 198 interior points, each side moved out by
1e-7), ROC curve, trapezoidal summation.  Host-side bookkeeping of a few counters; nothing here is on the hot path.

GroupedMetrics is the grouped family of the reference's metrics/ directory (HR / NDCG / MRR@K of metrics/NCF_evaluation/ndcg_hr_mrr.py, the
per-user loss of metrics/weighted_loss/weighted_loss.py) and the DIN paper's GAUC: buffered samples, one HIP launch (csrc/rank_metrics.hip) at
result().
"""
import torch

_RANK_INT = ("n_pos", "n_neg", "gt", "eq", "rank")


def _group_rank_stats_torch(scores, labels, weights, offsets):
    """ops.group_rank_stats restated with torch broadcasts (include/dir_hip.h holds the definitions): what GroupedMetrics(device="cpu")
    runs, so that the host logic can be tested without a GPU.  Pads the groups to [G, n_max] and compares all pairs, some groups at a time:
    O(G n_max^2) work -- not a path for production sizes."""
    G = offsets.numel() - 1
    dev = scores.device
    out = {k: torch.zeros(G, dtype=torch.int64, device=dev) for k in _RANK_INT}
    out.update({k: torch.zeros(G, dtype=torch.float64, device=dev) for k in ("mis_w", "tot_w")})
    if G == 0 or scores.numel() == 0:
        return out
    sizes = (offsets[1:] - offsets[:-1]).clamp_min(0)
    n_max = int(sizes.max())
    gid = torch.repeat_interleave(torch.arange(G, device=dev), sizes)
    src = torch.arange(gid.numel(), device=dev) + offsets[0]
    col = src - offsets[gid]
    S = torch.zeros(G, n_max, dtype=torch.float32, device=dev)
    V = torch.zeros(G, n_max, dtype=torch.bool, device=dev)
    P = torch.zeros(G, n_max, dtype=torch.bool, device=dev)
    W = torch.zeros(G, n_max, dtype=torch.float64, device=dev)
    S[gid, col] = scores[src]
    V[gid, col] = True
    P[gid, col] = labels[src] > 0.5
    W[gid, col] = 1.0 if weights is None else weights[src].to(torch.float64)
    N = V & ~P
    before = torch.arange(n_max, device=dev).unsqueeze(0) < torch.arange(n_max, device=dev).unsqueeze(1)      # [i, j]: j < i
    step = max(1, (1 << 22) // (n_max * n_max))
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for c in range(0, G, step):
        s, v, p, n, w = S[c:c + step], V[c:c + step], P[c:c + step], N[c:c + step], W[c:c + step]
        above = s.unsqueeze(1) > s.unsqueeze(2)                  # [g, i, j]: s_j > s_i
        equal = s.unsqueeze(1) == s.unsqueeze(2)
        a = (above & n.unsqueeze(1)).sum(2)
        e = (equal & n.unsqueeze(1)).sum(2)
        n_pos, n_neg = p.sum(1), n.sum(1)
        other = v.unsqueeze(1) & ~torch.eye(n_max, dtype=torch.bool, device=dev)
        place = 1 + ((above & other) | (equal & other & before)).sum(2)
        sl = slice(c, c + step)
        out["n_pos"][sl], out["n_neg"][sl] = n_pos, n_neg
        out["gt"][sl] = ((n_neg.unsqueeze(1) - a - e) * p).sum(1)
        out["eq"][sl] = (e * p).sum(1)
        out["mis_w"][sl] = torch.where(p, w * (a + e).to(torch.float64), zero).sum(1)
        out["tot_w"][sl] = torch.where(p, w * n_neg.unsqueeze(1).to(torch.float64), zero).sum(1)
        out["rank"][sl] = torch.where(n_pos == 1, (place * p).sum(1), torch.zeros_like(n_pos))
    return out


class GroupedMetrics:
    """Grouped ranking metrics over everything that was fed, from ONE launch of the per-group pair statistics (ops.group_rank_stats):

      gauc, gauc_groups      the DIN paper's user-weighted AUC (arXiv:1706.06978 section 6.2): sum n_g auc_g / sum n_g over the groups that
                             hold both classes, auc_g = (gt + eq / 2) / (n_pos n_neg), n_g the group's size (its impressions)
      weighted_loss          metrics/weighted_loss/weighted_loss.py:27-50,80-81: the mean over ALL groups of mis_w / tot_w -- the weight of
                             the (pos, neg) pairs with pred_pos <= pred_neg over the weight of all pairs; 0 for a group without a pair, NaN
                             where pairs exist and their weights sum to zero (the float division there)
      hr@k, ndcg@k, mrr@k,   metrics/NCF_evaluation/ndcg_hr_mrr.py:14-44,58-84 over the groups with exactly one positive: rank <= k,
      ranking_groups         1 / log2(rank + 1) and 1 / rank where hit, else 0 (MRR is cut at k as there); ties rank in entry order
                             (a stable sort; the reference's quicksort leaves them undefined)
      groups                 the number of groups

    update() takes samples in any order (a group may span calls) and only keeps the tensors it is given -- no kernel, no synchronisation; do
    not overwrite them before result().  update_blocks() takes the layout of ndcg_hr_mrr.py: complete consecutive groups of `block` scores
    with the positive at a fixed index; its groups are distinct from every group id of update().  result() orders the samples by group with a
    stable sort (so a group's entries keep the order they were fed in), builds the offsets and runs the kernel once.  device="cpu" computes
    the same statistics with torch broadcasts (for tests of this host logic; quadratic in the largest group)."""

    def __init__(self, k=10, device="cuda"):
        self.k = int(k)
        if self.k < 1:
            raise ValueError("GroupedMetrics: k must be at least 1, got %r" % k)
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        self._fed = []        # (group_ids, labels, scores, weights or None), flat
        self._blocks = []     # (scores [g, block], positive_index)
        return self

    def _flat(self, t, name):
        if not isinstance(t, torch.Tensor) or t.device.type != self.device.type:
            raise RuntimeError("GroupedMetrics(device=%r): %s must be a tensor on that device" % (str(self.device), name))
        return t.detach().reshape(-1)

    def update(self, group_ids, labels, scores, weights=None):
        g, y, s = self._flat(group_ids, "group_ids"), self._flat(labels, "labels"), self._flat(scores, "scores")
        w = None if weights is None else self._flat(weights, "weights")
        if g.dtype not in (torch.int64, torch.int32):
            raise TypeError("GroupedMetrics.update: group_ids must be int64 or int32, got %s" % g.dtype)
        if not (g.numel() == y.numel() == s.numel() and (w is None or w.numel() == s.numel())):
            raise ValueError("GroupedMetrics.update: group_ids, labels, scores and weights must hold the same number of samples")
        self._fed.append((g, y, s, w))
        return self

    def update_blocks(self, scores, block=100, positive_index=0):
        s = self._flat(scores, "scores")
        block, positive_index = int(block), int(positive_index)
        if block < 1 or s.numel() % block or not (0 <= positive_index < block):
            raise ValueError("GroupedMetrics.update_blocks: %d scores are not complete blocks of %d with the positive at %d"
                             % (s.numel(), block, positive_index))
        self._blocks.append((s.reshape(-1, block), positive_index))
        return self

    @torch.no_grad()
    def _gather(self):
        """-> scores, labels, weights (float32 [n]), offsets (int64 [G + 1]): the fed samples by group (stable), then the blocks."""
        dev, f32 = self.device, torch.float32
        ss, ys, ws, sizes = [], [], [], []
        if self._fed:
            g = torch.cat([f[0].to(torch.int64) for f in self._fed])
            y = torch.cat([f[1].to(f32) for f in self._fed])
            s = torch.cat([f[2].to(f32) for f in self._fed])
            w = torch.cat([torch.ones(f[2].numel(), dtype=f32, device=f[2].device) if f[3] is None else f[3].to(f32) for f in self._fed])
            g, order = torch.sort(g, stable=True)
            _, counts = torch.unique_consecutive(g, return_counts=True)
            ss.append(s[order]); ys.append(y[order]); ws.append(w[order]); sizes.append(counts)      # noqa: E702
        for s2, pi in self._blocks:
            y2 = torch.zeros(s2.shape, dtype=f32, device=s2.device)
            y2[:, pi] = 1.0
            ss.append(s2.to(f32).reshape(-1)); ys.append(y2.reshape(-1)); ws.append(torch.ones(s2.numel(), dtype=f32, device=s2.device))      # noqa: E702
            sizes.append(torch.full((s2.shape[0],), s2.shape[1], dtype=torch.int64, device=s2.device))
        if not ss:
            e = torch.zeros(0, dtype=f32, device=dev)
            return e, e, e, torch.zeros(1, dtype=torch.int64, device=dev)
        offsets = torch.zeros(sum(c.numel() for c in sizes) + 1, dtype=torch.int64, device=ss[0].device)
        torch.cumsum(torch.cat(sizes), 0, out=offsets[1:])
        return torch.cat(ss).contiguous(), torch.cat(ys).contiguous(), torch.cat(ws).contiguous(), offsets

    @torch.no_grad()
    def group_stats(self):
        """The seven per-group tensors of everything fed so far (ops.group_rank_stats's dict), groups in the order of _gather()."""
        s, y, w, offsets = self._gather()
        if self.device.type == "cpu":
            return _group_rank_stats_torch(s, y, w, offsets)
        from . import ops
        return ops.group_rank_stats(s, y, w, offsets)

    @torch.no_grad()
    def result(self):
        st = self.group_stats()
        f64 = torch.float64
        n_pos, n_neg = st["n_pos"], st["n_neg"]
        G = n_pos.numel()
        pairs = (n_pos * n_neg).to(f64)
        both = pairs > 0
        size = (n_pos + n_neg).to(f64)
        auc = (st["gt"].to(f64) + st["eq"].to(f64) / 2.0) / pairs.clamp_min(1.0)
        zero = torch.zeros((), dtype=f64, device=n_pos.device)
        loss = torch.where(both, st["mis_w"] / st["tot_w"], zero)            # 0 / 0 -> NaN where the pairs' weights are all zero
        one = n_pos == 1
        rank = st["rank"].clamp_min(1).to(f64)
        hit = one & (st["rank"] <= self.k)
        sums = torch.stack([both.sum().to(f64), torch.where(both, size, zero).sum(), torch.where(both, size * auc, zero).sum(), loss.sum(),
                            one.sum().to(f64), hit.sum().to(f64), torch.where(hit, 1.0 / torch.log2(rank + 1.0), zero).sum(),
                            torch.where(hit, 1.0 / rank, zero).sum()]).tolist()
        div = lambda a, b: a / b if b > 0 else 0.0  # noqa: E731  (an empty accumulator reports zeros)
        k = self.k
        return {"gauc": div(sums[2], sums[1]), "gauc_groups": int(sums[0]), "weighted_loss": div(sums[3], float(G)),
                "hr@%d" % k: div(sums[5], sums[4]), "ndcg@%d" % k: div(sums[6], sums[4]), "mrr@%d" % k: div(sums[7], sums[4]),
                "ranking_groups": int(sums[4]), "groups": G}


class BinaryMetrics:
    def __init__(self, num_thresholds=200, device="cuda"):
        eps = 1e-7
        t = [(i + 1) * 1.0 / (num_thresholds - 1) for i in range(num_thresholds - 2)]
        self.thresholds = torch.tensor([0.0 - eps] + t + [1.0 + eps], dtype=torch.float64, device=device)
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)  # noqa: E731
        self.tp, self.fp, self.tn, self.fn = z(num_thresholds), z(num_thresholds), z(num_thresholds), z(num_thresholds)
        self.sums = z(8)   # w, w*loss, w*label, w*correct, w*tp@.5, w*fp@.5, w*fn@.5, w*logistic

    @torch.no_grad()
    def update(self, labels, logistic, unweighted_loss=None, weights=None):
        """labels, logistic (and loss, weights): [B] or [B,1] on the metrics' device."""
        y = labels.reshape(-1).to(torch.float64)
        p = logistic.reshape(-1).to(torch.float64)
        w = torch.ones_like(y) if weights is None else weights.reshape(-1).to(torch.float64)
        loss = torch.zeros_like(y) if unweighted_loss is None else unweighted_loss.reshape(-1).to(torch.float64)
        pred = (p > 0.5).to(torch.float64)                  # class_ids = argmax([1-p, p])
        pos = y > 0.5
        above = p.unsqueeze(0) > self.thresholds.unsqueeze(1)              # [T, B]
        wp, wn = (w * pos).unsqueeze(0), (w * (~pos)).unsqueeze(0)
        self.tp += (above * wp).sum(1)
        self.fn += ((~above) * wp).sum(1)
        self.fp += (above * wn).sum(1)
        self.tn += ((~above) * wn).sum(1)
        self.sums += torch.stack([w.sum(), (w * loss).sum(), (w * y).sum(), (w * (pred == y)).sum(), (w * pred * y).sum(),
                                  (w * pred * (1 - y)).sum(), (w * (1 - pred) * y).sum(), (w * p).sum()])
        return self

    def result(self):
        s = self.sums.tolist()
        wsum = s[0]
        div = lambda a, b: a / b if b > 0 else 0.0  # noqa: E731
        eps = 1e-6                                           # tf.metrics.auc's epsilon in the rates
        tpr = (self.tp + eps) / (self.tp + self.fn + eps)
        fpr = self.fp / (self.fp + self.tn + eps)
        auc = float(((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0).sum())
        label_mean = div(s[2], wsum)
        return {"average_loss": div(s[1], wsum), "accuracy": div(s[3], wsum), "precision": div(s[4], s[4] + s[5]),
                "recall": div(s[4], s[4] + s[6]), "accuracy_baseline": max(label_mean, 1.0 - label_mean), "auc": auc,
                "label/mean": label_mean, "prediction/mean": div(s[7], wsum)}
