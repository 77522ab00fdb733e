"""model_ref64.py -- the five models restated in plain float64 torch, written from their definitions: what the whole-model tests
(tests/test_gpu_model_grads.py) hold the HIP training and inference paths to, and what tests/test_model_ref64.py pins first against the
reference-text fixtures, oracle/np_ref.py and the C oracle.

A plain module (not a conftest).  It imports nothing of the product's ops / autograd / dense modules and calls no model.forward:
indexing, einsum, relu, sigmoid and exp are all it needs, so torch.autograd differentiates every line of it.

  DeepFM    models/DeepFM/deepFM.py:143-223 (inputs -> fm_logit_fn :321-335 + dnn_logit_fn :284-319 + linear :255-275, add_n :223)
  DCN       models/DeepCrossNetwork/DeepCrossNetwork.py:118-141 (_cross_op :345-346, _deep_architecture :370-410, concat + dense(1) :134-139)
  ESMM      models/ESMM/ESMM.py:62-92 (two towers :130-147, ctcvr :69-74) and _get_loss :150-175
  xDeepFM   arXiv:1803.05170 eq. 6 as include/dir_hip.h states it (x_out[b,h,d] = sum_ij W[h,i,j] xk[b,i,d] x0[b,j,d], pooled over d)
  DIN       arXiv:1706.06978 (unit on [h, a, h - a, h * a], 80-40-1; PReLU; Dice eq. 3) as include/dir_hip.h A13 states it

Conventions: every parameter is given in the MODULE's layout (nn.Linear weights [out, in]) as a float64 tensor -- `leaves` makes
detached double leaves with requires_grad -- ids are int64 with id < 0 pruned (a zero row, no gradient); dropout is 0 everywhere (its
mask is not reproducible).  Batch-norm / Dice in TRAIN mode normalise with the batch mean and POPULATION variance and return the batch
statistics, so that the caller can form the moving statistics (`moving_update`)."""
import contextlib
import math

import torch

_KINKS = None


@contextlib.contextmanager
def kinks():
    """Collects the pre-activation of every relu / prelu evaluated inside the block (detached, leading dimension = batch): the points where
    those functions have no derivative.  A caller that compares gradients with an fp32 implementation uses it to keep its inputs a margin
    away from them -- at |pre-activation| below fp32's rounding of it the two sides may stand on different sides of the kink, and each
    is then a correct one-sided derivative of a different branch."""
    global _KINKS
    _KINKS = []
    try:
        yield _KINKS
    finally:
        _KINKS = None


def relu(x):
    if _KINKS is not None:
        _KINKS.append(x.detach())
    return torch.relu(x)


def leaves(tensors, dtype=torch.float64):
    """Detached float64 copies that require grad, in the structure given (tensor | list / tuple | dict | None).  dtype=torch.float32
    makes the same graph a plain fp32 one: what measures fp32's own distance from float64 when a bar is in question."""
    if tensors is None:
        return None
    if isinstance(tensors, torch.Tensor):
        return tensors.detach().to(dtype).clone().requires_grad_(True)
    if isinstance(tensors, dict):
        return {k: leaves(v, dtype) for k, v in tensors.items()}
    return [leaves(t, dtype) for t in tensors]


def flatten(struct, prefix=""):
    """[(path, tensor)] of a nested dict / list / tuple of tensors, in a fixed order (dict keys sorted): pairs a module's parameters with
    the leaves made from them."""
    if struct is None:
        return []
    if isinstance(struct, torch.Tensor):
        return [(prefix, struct)]
    items = sorted(struct.items()) if isinstance(struct, dict) else enumerate(struct)
    out = []
    for k, v in items:
        out += flatten(v, "%s.%s" % (prefix, k) if prefix else str(k))
    return out


# ---- input columns ------------------------------------------------------------------------------------------------------------------
def onehot(table, ids):
    """One id per sample: table[ids], a zero row for id < 0 (deepFM.py:383-393).  table [V, K] or [V]."""
    ok = ids >= 0
    rows = table[ids.clamp_min(0)]
    return rows * (ok.to(rows.dtype) if rows.dim() == 1 else ok.to(rows.dtype).unsqueeze(-1))


def bag(table, values, offsets, weights=None, combiner="mean"):
    """[TF-upstream] safe_embedding_lookup_sparse over one CSR column: sample b owns values[offsets[b]:offsets[b + 1]]; id < 0 is pruned;
    sum | mean (/ sum w) | sqrtn (/ sqrt(sum w^2)); an empty bag is a zero row."""
    B = offsets.numel() - 1
    counts = offsets[1:] - offsets[:-1]
    rows = torch.repeat_interleave(torch.arange(B, device=values.device), counts)
    w = torch.ones(values.shape, dtype=table.dtype, device=values.device) if weights is None else weights.to(table.dtype)
    w = w * (values >= 0).to(table.dtype)
    picked = table[values.clamp_min(0)] * w.unsqueeze(-1)
    acc = torch.zeros((B, table.shape[1]), dtype=table.dtype, device=values.device).index_add(0, rows, picked)
    if combiner == "sum":
        return acc
    zero = torch.zeros(B, dtype=table.dtype, device=values.device)
    den = zero.index_add(0, rows, w) if combiner == "mean" else zero.index_add(0, rows, w * w).sqrt()
    return acc / torch.where(den > 0, den, torch.ones_like(den)).unsqueeze(-1)


def indicator(ids, depth, dtype=torch.float64):
    """[TF-upstream] indicator_column of one id per sample: a one-hot row, all zero for id < 0."""
    out = torch.zeros((ids.numel(), depth), dtype=dtype, device=ids.device)
    ok = ids.reshape(-1) >= 0
    out[torch.arange(ids.numel(), device=ids.device)[ok], ids.reshape(-1)[ok]] = 1.0
    return out


def input_layer(named_blocks):
    """[TF-upstream] input_layer: the columns' blocks concatenated SORTED BY COLUMN NAME.  named_blocks: {column name: [B, width]}."""
    return torch.cat([named_blocks[k] for k in sorted(named_blocks)], dim=1)


# ---- layers -------------------------------------------------------------------------------------------------------------------------
def dense(x, W, b=None):
    y = x @ W.t()
    return y if b is None else y + b


def batch_norm(x, beta, gamma=None, eps=1e-3, moving=None):
    """tf.layers.batch_normalization / contrib batch_norm.  moving = (mean, variance): the inference form; None: the TRAIN form on the
    batch's mean and population variance.  -> (y, (mean, variance) used)."""
    if moving is None:
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)
    else:
        mean, var = moving
    inv = 1.0 / torch.sqrt(var + eps)
    if gamma is not None:
        inv = inv * gamma
    return (x - mean) * inv + beta, (mean, var)


def moving_update(moving, batch, momentum):
    """moving <- moving * momentum + batch * (1 - momentum)."""
    return moving.double() * momentum + batch.detach() * (1.0 - momentum)


def sigmoid_cross_entropy(logits, labels):
    """tf.nn.sigmoid_cross_entropy_with_logits: max(z, 0) - z y + log(1 + exp(-|z|))."""
    labels = labels.to(logits.dtype).reshape(logits.shape)
    return logits.clamp_min(0) - logits * labels + torch.log1p(torch.exp(-logits.abs()))


def weighted_loss(logits, labels, weights=None, reduction="mean"):
    """[TF-upstream] compute_weighted_loss of the sigmoid cross entropy: "sum" = sum(w l), "mean" = sum(w l) / sum(w)."""
    un = sigmoid_cross_entropy(logits, labels)
    w = torch.ones_like(un) if weights is None else weights.to(un.dtype).reshape(-1, 1).expand_as(un)
    total = (un * w).sum()
    return total if reduction == "sum" else total / w.sum()


def linear_logit(weights, ids, bias):
    """linear_model(units = 1, 'sum') over one-hot columns: sum_f w_f[ids[:, f]] + bias -> [B, 1] (deepFM.py:255-275)."""
    out = bias.reshape(1, 1)
    for f, w in enumerate(weights):
        out = out + onehot(w.reshape(-1), ids[:, f]).unsqueeze(1)
    return out


# ---- DeepFM -------------------------------------------------------------------------------------------------------------------------
def fm_logit(emb, F, K):
    """fm_logit_fn (deepFM.py:329-334): 0.5 * sum_k ((sum_f e)^2 - sum_f e^2) -> [B, 1]."""
    e = emb.reshape(-1, F, K)
    return 0.5 * (e.sum(dim=1) ** 2 - (e ** 2).sum(dim=1)).sum(dim=1, keepdim=True)


def deepfm(emb, F, K, hidden, head, linear, bns=None, train=False, eps=1e-3):
    """emb [B, F K]: the dnn columns' concatenation; hidden [(W, b)]; head (W [1, h], b [1]); linear [B, 1]: the first-order term with
    its bias; bns: per hidden layer {gamma, beta, moving_mean, moving_variance} (dense -> relu -> batch norm, deepFM.py:295-308).
    -> (logits [B, 1], [(batch mean, batch variance)] per batch norm when train)."""
    net, stats = emb, []
    for i, (W, b) in enumerate(hidden):
        net = relu(dense(net, W, b))
        if bns is not None:
            bn = bns[i]
            net, st = batch_norm(net, bn["beta"], bn.get("gamma"), eps, None if train else (bn["moving_mean"], bn["moving_variance"]))
            stats.append(st)
    return fm_logit(emb, F, K) + dense(net, *head) + linear, stats          # deepFM.py:337-338, :223


# ---- DCN ----------------------------------------------------------------------------------------------------------------------------
def cross_network(x0, w, b):
    """_cross_architecture (DeepCrossNetwork.py:361-365): x_{l+1} = x0 * (x_l . w_l) + b_l + x_l."""
    xl = x0
    for l in range(w.shape[0]):
        xl = x0 * (xl @ w[l]).unsqueeze(1) + b[l] + xl
    return xl


def dcn(x0, cross_w, cross_b, hidden, bns, head, train=False, eps=1e-3):
    """hidden [(W, b)]; bns: one {beta, moving_mean, moving_variance} per hidden layer but the last (contrib batch_norm: no gamma,
    :401-403, :413-419); head (W [1, d + h], b [1]) over concat([cross, deep]) (:134-139).  -> (logits, batch statistics when train)."""
    cross = cross_network(x0, cross_w, cross_b)
    net, stats = x0, []
    for i, (W, b) in enumerate(hidden):
        net = relu(dense(net, W, b))
        if bns is not None and i < len(hidden) - 1:
            bn = bns[i]
            net, st = batch_norm(net, bn["beta"], None, eps, None if train else (bn["moving_mean"], bn["moving_variance"]))
            stats.append(st)
    return dense(torch.cat([cross, net], dim=1), *head), stats


# ---- xDeepFM ------------------------------------------------------------------------------------------------------------------------
def cin(x0, Ws):
    """x0 [B, m, D]; Ws[k] [H_k, H_{k-1} m] (H_0 = m) -> the layers' sum-pooled maps, concatenated [B, sum H_k] (arXiv:1803.05170 eq. 6-7)."""
    m = x0.shape[1]
    xk, pooled = x0, []
    for W in Ws:
        H = W.shape[0]
        xk = torch.einsum("hij,bid,bjd->bhd", W.reshape(H, xk.shape[1], m), xk, x0)
        pooled.append(xk.sum(dim=2))
    return torch.cat(pooled, dim=1)


def xdeepfm(emb, m, D, cin_W, cin_out, hidden, dnn_out, linear=None):
    """emb [B, m D]; cin_out / dnn_out (W [1, n], b [1]); linear [B, 1] or None -> logits [B, 1] = CIN + DNN + linear."""
    logits = dense(cin(emb.reshape(-1, m, D), cin_W), *cin_out)
    net = emb
    for W, b in hidden:
        net = relu(dense(net, W, b))
    logits = logits + dense(net, *dnn_out)
    return logits if linear is None else logits + linear


# ---- ESMM ---------------------------------------------------------------------------------------------------------------------------
def tower(x, hidden, head):
    """_base_model after its input layer (ESMM.py:139-146): (dense + relu)* -> dense(1)."""
    for W, b in hidden:
        x = relu(dense(x, W, b))
    return dense(x, *head)


def esmm(x_ctr, x_cvr, ctr, cvr, eps=1e-7):
    """x_ctr / x_cvr: each tower's own input layer output; ctr / cvr = (hidden, head).  -> {ctr_logits, cvr_logits, ctcvr_logits} with
    ctcvr = logit(clip(sigmoid(ctr) sigmoid(cvr), 1e-7, 1 - 1e-7)) (ESMM.py:69-74)."""
    ctr_logits, cvr_logits = tower(x_ctr, *ctr), tower(x_cvr, *cvr)
    p = (torch.sigmoid(ctr_logits) * torch.sigmoid(cvr_logits)).clamp(eps, 1 - eps)
    return {"ctr_logits": ctr_logits, "cvr_logits": cvr_logits, "ctcvr_logits": torch.log(p / (1 - p))}


def esmm_loss(out, click, convert, ctr_weights=None, ctcvr_weights=None):
    """_get_loss (ESMM.py:150-175): the CTR and CTCVR cross entropies, each MEAN-reduced under its own weight column, added."""
    return (weighted_loss(out["ctr_logits"], click, ctr_weights, "mean")
            + weighted_loss(out["ctcvr_logits"], convert, ctcvr_weights, "mean"))


# ---- DIN ----------------------------------------------------------------------------------------------------------------------------
def dice(s, alpha, valid=None, eps=1e-8, moving=None):
    """Dice (arXiv:1706.06978 eq. 3): f(s) = p s + (1 - p) alpha s, p = sigmoid((s - E[s]) / sqrt(Var[s] + eps)) over the last
    dimension's units.  moving = (mean, variance): inference; None: the statistics of the rows `valid` marks (all rows when None), population
    variance.  -> (f(s), (mean, variance) used)."""
    if moving is None:
        flat = s.reshape(-1, s.shape[-1])
        if valid is None:
            mean = flat.mean(dim=0)
            var = ((flat - mean) ** 2).mean(dim=0)
        else:
            v = valid.reshape(-1, 1).to(s.dtype)
            n = v.sum()
            mean = (flat * v).sum(dim=0) / n
            var = (((flat - mean) ** 2) * v).sum(dim=0) / n
    else:
        mean, var = moving
    p = torch.sigmoid((s - mean) / torch.sqrt(var + eps))
    return p * s + (1 - p) * alpha * s, (mean, var)


def prelu(s, alpha):
    if _KINKS is not None:
        _KINKS.append(s.detach())
    return torch.where(s > 0, s, alpha * s)


def _din_act(s, kind, act, valid, train, stats):
    """act: None (sigmoid / relu take none) or {alpha[, moving_mean, moving_variance]}."""
    if kind == "sigmoid":
        return torch.sigmoid(s)
    if kind == "relu":
        return relu(s)
    if kind == "prelu":
        return prelu(s, act["alpha"])
    y, st = dice(s, act["alpha"], valid, moving=None if train else (act["moving_mean"], act["moving_variance"]))
    stats.append(st)
    return y


def din_attention_pool(table, hist, hist_len, cand, unit, activation="sigmoid", acts=None, normalize=False, train=False):
    """The local activation unit and the weighted sum pooling.  hist [B, T] (id < 0: padding), hist_len [B] or None, cand [B];
    unit = (W1 [4K, H1], b1, W2 [H1, H2], b2, W3 [H2], b3 [1]); acts = (act1, act2) for prelu / dice.  A position counts when it is inside
    the length and its id is >= 0; the score of (h, a) is the 80-40-1 MLP on [h, a, h - a, h * a]; normalize: softmax of score / sqrt(K)
    over the counted positions, otherwise the raw scores weigh the rows.  Training-mode Dice takes its statistics over the counted rows of
    the whole batch.  -> (pooled [B, K], scores [B, T], [(mean, variance)] per Dice layer)."""
    W1, b1, W2, b2, W3, b3 = unit
    B, T = hist.shape
    K = table.shape[1]
    valid = hist >= 0
    if hist_len is not None:
        valid = valid & (torch.arange(T, device=hist.device).unsqueeze(0) < hist_len.reshape(-1, 1))
    h = table[hist.clamp_min(0)]                                                  # [B, T, K]
    a = onehot(table, cand).unsqueeze(1).expand(B, T, K)
    u = torch.cat([h, a, h - a, h * a], dim=-1)
    stats = []
    acts = acts or (None, None)
    z1 = _din_act(u @ W1 + b1, activation, acts[0], valid, train, stats)
    z2 = _din_act(z1 @ W2 + b2, activation, acts[1], valid, train, stats)
    s = z2 @ W3.reshape(-1) + b3.reshape(())
    vf = valid.to(s.dtype)
    if normalize:
        s = s / math.sqrt(K)
        smax = torch.where(valid, s, torch.full_like(s, torch.finfo(s.dtype).min / 4)).max(dim=1, keepdim=True).values.detach()
        e = torch.exp(torch.where(valid, s - smax, torch.zeros_like(s))) * vf
        den = e.sum(dim=1, keepdim=True)
        w = e / torch.where(den > 0, den, torch.ones_like(den))
    else:
        w = s * vf
    return (w.unsqueeze(-1) * h * vf.unsqueeze(-1)).sum(dim=1), w, stats


def din(table, hist, hist_len, cand, unit, hidden, head, columns=None, attention_activation="sigmoid", attention_acts=None,
        normalize=False, dnn_activation="dice", dnn_acts=None, train=False):
    """The model (paper figure 2): concat([profile / context block `columns` [B, W] or None, interest vector, candidate embedding]) ->
    hidden [(W, b)] with relu | sigmoid | prelu | dice (dnn_acts: one {alpha, ...} per layer) -> head.  -> (logits [B, 1], the unit's Dice
    statistics, the tail's Dice statistics)."""
    pooled, _, ustats = din_attention_pool(table, hist, hist_len, cand, unit, attention_activation, attention_acts, normalize, train)
    net = torch.cat(([columns] if columns is not None else []) + [pooled, onehot(table, cand)], dim=1)
    tstats = []
    for i, (W, b) in enumerate(hidden):
        net = _din_act(dense(net, W, b), dnn_activation, dnn_acts[i] if dnn_acts else None, None, train, tstats)
    return dense(net, *head), ustats, tstats
