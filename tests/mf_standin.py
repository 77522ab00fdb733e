"""The matrix-factorisation family of csrc/mf.hip and dir_amd.mf restated literally in NumPy: the score (MF_model.py:164-194), its gradients
in float64, the losses (MF_model.py:124-145 restated by hand -- the recorder does not execute those lines -- and :196-215) and the negative
sampler with the counter layout of include/dir_hip.h (dir_neg_sample_i64), built on tests/dropout_ref.philox4x32_10.  The reference of
tests/test_mf_host.py and tests/test_gpu_mf.py."""
import numpy as np

from tests.dropout_ref import philox4x32_10


def score(P, Q, ids, bu=None, bi=None, b0=None, dtype=np.float64):
    """ids [B, 1 + C] -> logits [B, C] = sum_k P[u, k] Q[i_c, k] + ((bu[u] + bi[i_c]) + b0)"""
    P, Q = np.asarray(P, dtype), np.asarray(Q, dtype)
    u, it = ids[:, 0], ids[:, 1:]
    out = (P[u][:, None, :] * Q[it]).sum(-1)
    if bu is not None:
        b = np.asarray(bu, dtype).reshape(-1)[u][:, None] + np.asarray(bi, dtype).reshape(-1)[it]
        if b0 is not None:
            b = b + dtype(np.asarray(b0).reshape(()))
        out = out + b
    elif b0 is not None:
        out = out + dtype(np.asarray(b0).reshape(()))
    return out


def score_grads(P, Q, ids, dl, bu=None, bi=None, l2=0.0):
    """float64 -> (grad [B, (1 + C) K], gbias [B, 1 + C]): per (sample, slot) gradients, the l2 terms per occurrence."""
    P, Q, dl = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(dl, np.float64)
    B, C, K = ids.shape[0], ids.shape[1] - 1, P.shape[1]
    u, it = ids[:, 0], ids[:, 1:]
    grad = np.zeros((B, 1 + C, K))
    grad[:, 0] = (dl[:, :, None] * Q[it]).sum(1) + l2 * P[u]
    grad[:, 1:] = dl[:, :, None] * P[u][:, None, :] + l2 * Q[it]
    gbias = np.zeros((B, 1 + C))
    gbias[:, 0] = dl.sum(1)
    gbias[:, 1:] = dl
    if bu is not None and l2:
        gbias[:, 0] += l2 * np.asarray(bu, np.float64).reshape(-1)[u]
        gbias[:, 1:] += l2 * np.asarray(bi, np.float64).reshape(-1)[it]
    return grad.reshape(B, (1 + C) * K), gbias


def scatter_rows(ids_col, rows, vocab):
    """sum of rows[i] into row ids_col[i] of a [vocab, ...] array (float64)"""
    out = np.zeros((vocab,) + rows.shape[1:])
    np.add.at(out, ids_col, rows)
    return out


def label_weights(labels, is_implicit=False, weights=None, weights_coef=0, label_threshold=4.0, dtype=np.float64):
    """MF_model.py:124-145 -> (labels [B, 1], weights [B] or a scalar)"""
    y = np.asarray(labels, dtype).reshape(-1)
    if label_threshold is not None:
        y = (y >= label_threshold).astype(dtype)
    term = 0.0
    if is_implicit:
        y = np.clip(y, 0, 1)
        term = np.log1p(y) if weights == "log_weight" else (y if weights == "normal_weight" else 0.0)
    return y[:, None], dtype(1.0) + dtype(weights_coef) * term


def data_loss(loss, preds, labels, weights):
    """tf.losses.log_loss (epsilon 1e-7) / mean_squared_error, reduction SUM_BY_NONZERO_WEIGHTS; weights [B] meet labels [B, 1] as [B, 1]"""
    preds, labels = np.asarray(preds), np.asarray(labels)
    dt = preds.dtype.type
    if loss == "cross entropy":
        eps = dt(1e-7)
        per = -labels * np.log(preds + eps) - (dt(1) - labels) * np.log(dt(1) - preds + eps)
    else:
        per = np.square(preds - labels)
    w = np.asarray(weights, preds.dtype)
    if w.ndim == per.ndim - 1 and w.ndim:
        w = w[..., None]
    w = np.broadcast_to(w, per.shape)
    nz = np.count_nonzero(w)
    return (per * w).sum() / dt(nz) if nz else dt(0)


def preds_of(loss, logits):
    return 1.0 / (1.0 + np.exp(-logits)) if loss == "cross entropy" else logits


def reg(P, Q, ids, reg_pen, bu=None, bi=None, dtype=np.float64):
    """reg_pen * (l2_loss of the looked-up rows and biases), tf.nn.l2_loss(t) = sum(t ** 2) / 2"""
    u, it = ids[:, 0], ids[:, 1:]
    l2 = lambda t: np.square(np.asarray(t, dtype)).sum() / dtype(2)      # noqa: E731
    r = l2(np.asarray(P)[u]) + l2(np.asarray(Q)[it])
    if bu is not None:
        r = r + (l2(np.asarray(bu).reshape(-1)[u]) + l2(np.asarray(bi).reshape(-1)[it]))
    return r * dtype(reg_pen)


def cost(loss, P, Q, ids, labels, weights, reg_pen, bu=None, bi=None, b0=None, dtype=np.float64):
    """-> (logits [B, 1], preds [B, 1], cost) of BaseMFModel for labels [B, 1] and weights as label_weights gives them"""
    logits = score(P, Q, ids, bu, bi, b0, dtype)
    preds = preds_of(loss, logits)
    return logits, preds, data_loss(loss, preds, np.asarray(labels, dtype), weights) + reg(P, Q, ids, reg_pen, bu, bi, dtype)


def neg_sample(users, offsets, items, num_items, n_neg, seed, draw=0, stream_id=0, first=0):
    """out [B, n_neg] int64 (and the status word): dir_neg_sample_i64's draws.  Draw e = first + b n_neg + c: one Philox block with counter
    (e & 0xffffffff, e >> 32, stream_id, draw) and key (seed & 0xffffffff, seed >> 32); w = r[0] | r[1] << 32; k = (w (num_items - n_u)) >> 64;
    the item is k + (the number of the user's items j with items[j] - j <= k)."""
    users, offsets, items = np.asarray(users, np.int64), np.asarray(offsets, np.int64), np.asarray(items, np.int64)
    B = users.shape[0]
    n = B * n_neg
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    e = [int(first) + i for i in range(n)]
    r = philox4x32_10([np.array([x & 0xFFFFFFFF for x in e], np.uint64), np.array([(x >> 32) & 0xFFFFFFFF for x in e], np.uint64),
                       np.full(n, stream_id, np.uint64), np.full(n, draw & 0xFFFFFFFF, np.uint64)], [seed & 0xFFFFFFFF, seed >> 32])
    out = np.empty(n, np.int64)
    status = 0
    for i in range(n):
        u = users[i // n_neg]
        mine = items[offsets[u]:offsets[u + 1]]
        m = int(num_items) - mine.shape[0]
        if m <= 0:
            out[i], status = -1, 1
            continue
        w = int(r[0][i]) | (int(r[1][i]) << 32)
        k = (w * m) >> 64                                        # mulhi64, as Python integers
        p = int(np.searchsorted(mine - np.arange(mine.shape[0], dtype=np.int64), k, side="right"))
        out[i] = k + p
    return out.reshape(B, n_neg), status
