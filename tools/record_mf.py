#!/usr/bin/env python
"""record_mf.py REFERENCE_CHECKOUT [OUT.npz] -- record what the reference's matrix-factorisation model text computes on seeded inputs.

Loads models/LFM/Mixture_1/MF_model.py under the NumPy stand-in for TensorFlow (oracle/tf_stub.py: the reference's OWN text is executed,
every tf primitive it calls is the stub's) and calls BaseMFModel._logit_fn and BaseMFModel._get_loss for loss in {mse, cross entropy},
intercepts in {True, False}, two weight vectors, in fp32 and fp64.  Inputs, tables, logits, preds and costs go to tests/golden/ref_mf.npz:
numbers only, "stubbed tf" like the ref_text_* fixtures (it pins op order, axes and constants to the reference's text, not TensorFlow's
numerics).  Nothing of the reference's text is in this file or in the fixture.

The four primitives the text needs that the stub lacks are registered here, with tf_stub._put ([TF-upstream] behaviour restated):
  tf.nn.l2_loss(t) = sum(t ** 2) / 2;  tf.identity;  tf.losses.log_loss (epsilon 1e-7) and tf.losses.mean_squared_error, both with the default
  reduction SUM_BY_NONZERO_WEIGHTS = sum(losses * weights) / count_nonzero(weights), weights of rank one less than the losses taking a
  trailing axis (compute_weighted_loss's squeeze_or_expand_dimensions: the text passes weights [B] beside labels [B, 1]).
The stub keys an embedding column's variable by its _var_scope_name under ONE `input_layer` scope, so the K-wide and the 1-wide column of
one key would meet on one variable: the four columns get distinct scope names here.  _model_fn's label lines (MF_model.py:124-145) are NOT
executed (the stub's cast does not cover them): labels and weights are handed to _get_loss as those lines would leave them, and
tests/mf_standin.label_weights restates them by hand.

Sizes: B = 64, U = 50, I = 40, K = 16.
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

B, U, I, K = 64, 50, 40, 16
REG_PEN = 0.05


def register(tf_stub):
    t = tf_stub._t

    def weighted(per, weights):
        per = np.asarray(per)
        w = np.asarray(weights, dtype=per.dtype)
        if w.ndim and w.ndim == per.ndim - 1:
            w = w[..., None]
        w = np.broadcast_to(w, per.shape)
        nz = np.count_nonzero(w)
        return t((per * w).sum() / per.dtype.type(nz) if nz else per.dtype.type(0))

    def log_loss(labels=None, predictions=None, weights=1.0, epsilon=1e-7, **kw):
        p, y = np.asarray(predictions), np.asarray(labels)
        eps = p.dtype.type(epsilon)
        return weighted(-y * np.log(p + eps) - (1 - y) * np.log(1 - p + eps), weights)

    def mean_squared_error(labels=None, predictions=None, weights=1.0, **kw):
        return weighted(np.square(np.asarray(predictions) - np.asarray(labels)), weights)

    tf_stub._put("tensorflow.nn.l2_loss", lambda x, name=None: t(np.square(np.asarray(x)).sum() / np.asarray(x).dtype.type(2)))
    tf_stub._put("tensorflow.identity", lambda x, name=None: t(np.asarray(x)))
    tf_stub._put("tensorflow.losses.log_loss", log_loss)
    tf_stub._put("tensorflow.losses.mean_squared_error", mean_squared_error)


def main(argv):
    if len(argv) < 2:
        raise SystemExit(__doc__)
    ref = argv[1]
    out = argv[2] if len(argv) > 2 else os.path.join(ROOT, "tests", "golden", "ref_mf.npz")
    from oracle import tf_stub
    mod = tf_stub.load_reference(os.path.join(ref, "models", "LFM", "Mixture_1", "MF_model.py"), "ref_mf_model")
    register(tf_stub)

    rng = np.random.default_rng(20181112)
    users, items = rng.integers(0, U, B).astype(np.int64), rng.integers(0, I, B).astype(np.int64)
    users[:2], items[:2] = [0, U - 1], [I - 1, 0]
    P = (rng.standard_normal((U, K)) * 0.25)
    Q = (rng.standard_normal((I, K)) * 0.25)
    bu, bi, b0 = rng.standard_normal((U, 1)) * 0.1, rng.standard_normal((I, 1)) * 0.1, np.float64(0.125)
    labels = (rng.random(B) < 0.4).astype(np.float64)            # what MF_model.py:126-128 leaves: 0 / 1
    w_log = 1.0 + 0.75 * np.log1p(labels)                        # :134-135, :143 with weights_coef = 0.75
    w_zero = (rng.integers(0, 5, B) / 4.0)                       # multiples of 1/4 with zeros: the non-zero count matters
    f32 = lambda a: np.asarray(a, np.float32)                     # noqa: E731
    rec = {"users": users, "items": items, "labels": f32(labels), "P": f32(P), "Q": f32(Q), "bu": f32(bu), "bi": f32(bi), "b0": f32(b0),
           "w_log": f32(w_log), "w_zero": f32(w_zero), "reg_pen": np.float64(REG_PEN)}

    cols = {n: tf_stub.EmbeddingColumn(key, buckets, dim) for n, key, buckets, dim in
            (("user_embedding", "user", U, K), ("item_embedding", "item", I, K), ("user_bias", "user", U, 1), ("item_bias", "item", I, 1))}
    for n, c in cols.items():
        c._var_scope_name = n
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        for loss, ltag in (("mse", "mse"), ("cross entropy", "xent")):
            for intercepts in (True, False):
                tf_stub.reset(dt)
                pre = "inputs/input_layer/%s/embedding_weights"
                tf_stub.VARS.update({pre % "user_embedding": rec["P"], pre % "item_embedding": rec["Q"], pre % "user_bias": rec["bu"],
                                     pre % "item_bias": rec["bi"], "inputs/global_bias": rec["b0"]})
                model = mod.BaseMFModel(embedding_cols=[[cols["user_embedding"]], [cols["item_embedding"]]],
                                        bias_cols=[[cols["user_bias"]], [cols["item_bias"]]], reg_pen=REG_PEN, learning_rate=0.01, loss=loss,
                                        intercepts=intercepts)
                logits, preds = model._logit_fn({"user": users, "item": items})
                key = "%s_%s_int%d" % (tag, ltag, int(intercepts))
                rec[key + "_logits"], rec[key + "_preds"] = np.asarray(logits), np.asarray(preds)
                assert np.asarray(logits).dtype == dt and np.asarray(logits).shape == (B, 1)
                for wname in ("w_log", "w_zero"):
                    c = model._get_loss(np.asarray(rec["labels"], dt).reshape(B, 1).view(tf_stub.T), preds, np.asarray(rec[wname], dt).view(tf_stub.T))
                    rec["%s_%s_cost" % (key, wname)] = np.asarray(c)
    np.savez_compressed(out, **rec)
    print("%s: %d arrays, %d bytes; e.g. f64_xent_int1 cost (w_log) %.12f" % (out, len(rec), os.path.getsize(out), float(rec["f64_xent_int1_w_log_cost"])))


if __name__ == "__main__":
    main(sys.argv)
