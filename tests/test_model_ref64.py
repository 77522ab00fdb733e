"""tests/model_ref64.py pinned before anything is measured against it (CPU, float64).

* DeepFM (onehot, onehot_bn in its inference form), DCN and ESMM reproduce the `*_f64` logits -- and ESMM's loss -- that the reference's own
  text computed on the fixtures' inputs and variables (tests/golden/ref_text_v1.npz, ref_text_v2_esmm.npz; tests/test_ref_text.py) at 1e-6,
  the bar that file uses for float64.
* xDeepFM's CIN and the DIN unit / model have no reference text: they are held to oracle/np_ref.py and to the C oracle's
  din_attention_pool(acc64=True) on one small case each, at 1e-6.
* torch.autograd.gradcheck of one scalar loss per restatement at a tiny shape (B <= 5)."""
import os

import numpy as np
import pytest
import torch

from tests import model_ref64 as M

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "ref_text_v1.npz"))
G2 = np.load(os.path.join(HERE, "golden", "ref_text_v2_esmm.npz"))


def T(a):
    a = np.asarray(a)
    return torch.from_numpy(a.astype(np.float64)) if a.dtype.kind == "f" else torch.from_numpy(a.astype(np.int64))


def _close(got, ref, tol=1e-6):
    got, ref = np.asarray(got.detach() if isinstance(got, torch.Tensor) else got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref) / (1 + np.abs(ref))
    assert err.max() <= tol, err.max()


@pytest.mark.parametrize("variant", ["onehot", "onehot_bn"])
def test_deepfm_restatement_reproduces_the_reference_text(variant):
    V = {k[len("deepfm_var:"):]: G[k] for k in G.files if k.startswith("deepfm_var:")}
    ids = T(G["deepfm_ids"])
    tabs = [T(V["dnn_fm_inputs/myself_input_layer/C%d_embedding/embedding_weights" % f]) for f in range(6)]
    emb = torch.cat([M.onehot(tabs[f], ids[:, f]) for f in range(6)], dim=1)
    _close(emb, G["deepfm_%s_inputs_f64" % variant])
    hidden = [(T(V["dnn_fm/hiddenlayer_%d/kernel" % i]).t(), T(V["dnn_fm/hiddenlayer_%d/bias" % i])) for i in range(2)]
    bns = None
    if variant == "onehot_bn":
        bns = [{n: T(V["dnn_fm/hiddenlayer_%d/batchnorm_%d/%s" % (i, i, n)]) for n in ("gamma", "beta", "moving_mean", "moving_variance")}
               for i in range(2)]
    lin_ids = torch.cat([ids, T(G["deepfm_ids_extra"])], dim=1)
    lws = [T(V["linear/linear_model/%s/weights" % n]) for n in ["C%d" % f for f in range(6)] + ["L0", "L1"]]
    linear = M.linear_logit(lws, lin_ids, T(V["linear/linear_model/bias_weights"]))
    _close(linear, G["deepfm_%s_linear_f64" % variant])
    _close(M.fm_logit(emb, 6, 8), G["deepfm_%s_fm_f64" % variant])
    logits, _ = M.deepfm(emb, 6, 8, hidden, (T(V["dnn_fm/logits/kernel"]).t(), T(V["dnn_fm/logits/bias"])), linear, bns=bns, train=False)
    _close(logits, G["deepfm_%s_logits_f64" % variant])


def test_dcn_restatement_reproduces_the_reference_text():
    D = {k[len("dcn_var:"):]: G[k] for k in G.files if k.startswith("dcn_var:")}
    pre = "dcn_model/input_from_feature_columns/"
    f = lambda k: T(G["dcn_feat:" + k])      # noqa: E731
    blocks = {"age": f("age"), "hours": f("hours"), "gain": f("gain"),
              "workclass_indicator": M.indicator(f("workclass"), 9), "marital_indicator": M.indicator(f("marital"), 7),
              "occupation_embedding": M.onehot(T(D[pre + "input_layer/occupation_embedding/embedding_weights"]), f("occupation").reshape(-1)),
              "native_embedding": M.bag(T(D[pre + "input_layer/native_embedding/embedding_weights"]), f("native_values"), f("native_offsets"),
                                        None, "sqrtn")}
    x0 = M.input_layer(blocks)
    _close(x0, G["dcn_x0_f64"])
    hidden = [(T(D[pre + "hidden_layer_%d/kernel" % i]).t(), T(D[pre + "hidden_layer_%d/bias" % i])) for i in range(3)]
    bns = [{n: T(D[pre + "hidden_layer_%d/bn_%d/%s" % (i, i, n)]) for n in ("beta", "moving_mean", "moving_variance")} for i in range(2)]
    head = (T(D["dcn_model/logits/dense/kernel"]).t(), T(D["dcn_model/logits/dense/bias"]))
    logits, _ = M.dcn(x0, T(D[pre + "cross_w"]), T(D[pre + "cross_b"]), hidden, bns, head, train=False)
    _close(logits, G["dcn_logits_f64"])
    _close(M.weighted_loss(logits, T(G["dcn_labels"]), None, "mean"), G["dcn_loss_f64"])


def test_esmm_restatement_reproduces_the_reference_text():
    V = {k[len("esmm_var:"):]: G2[k] for k in G2.files if k.startswith("esmm_var:")}
    f = lambda k: T(G2["esmm_feat:" + k])      # noqa: E731
    nh = len(G2["esmm_hidden"])

    def inputs(pre):
        return M.input_layer({
            "age": f("age"), "price": f("price"),
            "item_embedding": M.onehot(T(V[pre + "input_layer/item_embedding/embedding_weights"]), f("item").reshape(-1)),
            "user_embedding": M.onehot(T(V[pre + "input_layer/user_embedding/embedding_weights"]), f("user").reshape(-1)),
            "tags_embedding": M.bag(T(V[pre + "input_layer/tags_embedding/embedding_weights"]), f("tags_values"), f("tags_offsets"),
                                    f("tags_weights"), "sqrtn")})

    def tower(pre):
        return ([(T(V[pre + "hiddenlayer_%d/kernel" % i]).t(), T(V[pre + "hiddenlayer_%d/bias" % i])) for i in range(nh)],
                (T(V[pre + "dense/kernel"]).t(), T(V[pre + "dense/bias"])))
    x_cvr = inputs("esmm/cvr_model/")
    _close(x_cvr, G2["esmm_cvr_inputs_f64"])
    out = M.esmm(inputs("esmm/ctr_model/"), x_cvr, tower("esmm/ctr_model/"), tower("esmm/cvr_model/"))
    for k in ("ctr_logits", "cvr_logits", "ctcvr_logits"):
        _close(out[k], G2["esmm_%s_f64" % k])
    loss = M.esmm_loss(out, T(G2["esmm_click_label"]), T(G2["esmm_convert_label"]), ctr_weights=f("w_click"))
    _close(loss, G2["esmm_loss_f64"])


# ---- no reference text: oracle/np_ref.py and the C oracle -----------------------------------------------------------------------------
def _xdeepfm_case(rng, B, m, D, Hs, hid):
    emb = rng.standard_normal((B, m * D)) * 0.3
    Ws, hp = [], m
    for h in Hs:
        Ws.append(rng.standard_normal((h, hp * m)) / np.sqrt(hp * m))
        hp = h
    cin_out = (rng.standard_normal((1, sum(Hs))) / np.sqrt(sum(Hs)), rng.standard_normal(1) * 0.1)
    hidden, d = [], m * D
    for n in hid:
        hidden.append((rng.standard_normal((n, d)) / np.sqrt(d), rng.standard_normal(n) * 0.1))
        d = n
    dnn_out = (rng.standard_normal((1, d)) / np.sqrt(d), rng.standard_normal(1) * 0.1)
    linear = rng.standard_normal((B, 1)) * 0.1
    return emb, Ws, cin_out, hidden, dnn_out, linear


def test_xdeepfm_restatement_matches_np_ref():
    from oracle import np_ref as R
    rng = np.random.default_rng(5)
    B, m, D, Hs = 7, 5, 6, (9, 4, 3)
    emb, Ws, cin_out, hidden, dnn_out, linear = _xdeepfm_case(rng, B, m, D, Hs, (10, 6))
    x0 = emb.reshape(B, m, D)
    xk, pooled = x0, []
    for W in Ws:
        xk, p = R.cin_layer(x0, xk, W)
        pooled.append(p)
    pooled = np.concatenate(pooled, axis=1)
    _close(M.cin(T(x0), [T(W) for W in Ws]), pooled)
    dnn = R.dnn_logit(emb, [(W.T, b) for W, b in hidden], (dnn_out[0].T, dnn_out[1]))
    ref = pooled @ cin_out[0].T + cin_out[1] + dnn + linear
    tt = lambda pairs: [(T(a), T(b)) for a, b in pairs]      # noqa: E731
    got = M.xdeepfm(T(emb), m, D, [T(W) for W in Ws], tt([cin_out])[0], tt(hidden), tt([dnn_out])[0], T(linear))
    _close(got, ref)


def _din_case(rng, B, T_, K, V, H1, H2, kind):
    table = rng.standard_normal((V, K)) * 0.3
    hist = rng.integers(0, V, size=(B, T_))
    hist[rng.random((B, T_)) < 0.15] = -1
    hl = rng.integers(0, T_ + 1, size=B).astype(np.int32)
    hl[0] = 0                                           # an empty history
    cand = rng.integers(0, V, size=B)
    cand[1] = -1                                        # a pruned candidate
    unit = [rng.standard_normal((4 * K, H1)) / np.sqrt(4 * K), rng.standard_normal(H1) * 0.1, rng.standard_normal((H1, H2)) / np.sqrt(H1),
            rng.standard_normal(H2) * 0.1, rng.standard_normal(H2) / np.sqrt(H2), rng.standard_normal(1) * 0.1]
    acts = None
    if kind != "sigmoid":
        acts = [{"alpha": 0.25 + rng.standard_normal(h) * 0.1, "moving_mean": rng.standard_normal(h) * 0.2, "moving_variance": rng.random(h) + 0.5}
                for h in (H1, H2)]
    return table, hist, hl, cand, unit, acts


def _act_params(acts, kind, eps=1e-8):
    """The flat [alpha, scale, shift] x 2 form the oracles take (Dice's inference form: p = sigmoid(scale s + shift))."""
    if acts is None:
        return None
    out = []
    for a in acts:
        n = a["alpha"].size
        scale = 1.0 / np.sqrt(a["moving_variance"] + eps) if kind == "dice" else np.zeros(n)
        shift = -a["moving_mean"] * scale if kind == "dice" else np.zeros(n)
        out += [a["alpha"], scale, shift]
    return np.concatenate(out)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("kind", ["sigmoid", "prelu", "dice"])
def test_din_restatement_matches_np_ref_and_the_c_oracle(oracle, kind, normalize):
    from oracle import np_ref as R
    rng = np.random.default_rng(11)
    B, T_, K, V, H1, H2 = 9, 6, 8, 30, 12, 8
    table, hist, hl, cand, unit, acts = _din_case(rng, B, T_, K, V, H1, H2, kind)
    ap = _act_params(acts, kind)
    tacts = [{k: T(v) for k, v in a.items()} for a in acts] if acts else None
    got, scores, _ = M.din_attention_pool(T(table), T(hist), T(hl), T(cand), [T(u) for u in unit], kind, tacts, normalize, train=False)
    ref, ref_scores = R.din_attention_pool(table, hist, hl, cand, *unit, normalize=normalize, activation=kind, act_params=ap)
    _close(got, ref)
    _close(scores, ref_scores)
    f32 = lambda a: np.asarray(a, np.float32)      # noqa: E731
    table32, unit32 = f32(table), [f32(u) for u in unit]
    cref = oracle.din_attention_pool(table32, hist, hl, cand, *unit32, normalize=normalize, acc64=True, activation=kind,
                                     act_params=f32(ap) if ap is not None else None)[0]
    t32acts = [{k: T(f32(v)) for k, v in a.items()} for a in acts] if acts else None
    got32, _, _ = M.din_attention_pool(T(table32), T(hist), T(hl), T(cand), [T(u) for u in unit32], kind, t32acts, normalize, train=False)
    _close(got32, cref)
    # the whole model against np_ref.din_model_logits, the tail with the same activation kind (sigmoid unit: a relu tail)
    tail_kind = "relu" if kind == "sigmoid" else kind
    cols = rng.standard_normal((B, 3)) * 0.5
    hidden, d = [], 3 + 2 * K
    for n in (10, 6):
        hidden.append((rng.standard_normal((n, d)) / np.sqrt(d), rng.standard_normal(n) * 0.1))
        d = n
    head = (rng.standard_normal((1, d)) / np.sqrt(d), rng.standard_normal(1) * 0.1)
    dacts, mlp = None, []
    if tail_kind != "relu":
        dacts = [{"alpha": 0.25 + rng.standard_normal(n) * 0.1, "moving_mean": rng.standard_normal(n) * 0.2, "moving_variance": rng.random(n) + 0.5}
                 for n in (10, 6)]
    for i, (W, b) in enumerate(hidden):
        params = None
        if dacts is not None:
            params = _act_params([dacts[i]], tail_kind).reshape(3, -1)
        mlp.append((W, b, tail_kind, params))
    ref = R.din_model_logits(cols, table, hist, hl, cand, unit, mlp, head, normalize=normalize, activation=kind, act_params=ap)
    tdacts = [{k: T(v) for k, v in a.items()} for a in dacts] if dacts else None
    got, _, _ = M.din(T(table), T(hist), T(hl), T(cand), [T(u) for u in unit], [(T(W), T(b)) for W, b in hidden], (T(head[0]), T(head[1])),
                      columns=T(cols), attention_activation=kind, attention_acts=tacts, normalize=normalize, dnn_activation=tail_kind,
                      dnn_acts=tdacts, train=False)
    _close(got, ref)


# ---- gradcheck: one scalar loss per restatement, B <= 5 ------------------------------------------------------------------------------
def _gradcheck(fn, tensors):
    leaves = [t.detach().double().clone().requires_grad_(True) for t in tensors]
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6, rtol=1e-4)


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _mlp_params(g, dims):
    out = []
    for a, b in zip(dims[:-1], dims[1:]):
        out += [_rand(g, b, a, scale=a ** -0.5), _rand(g, b, scale=0.1)]
    return out


def _pairs(flat):
    return [(flat[i], flat[i + 1]) for i in range(0, len(flat), 2)]


def test_gradcheck_deepfm_with_training_batch_norm():
    g = torch.Generator().manual_seed(1)
    B, F, K, Vn = 5, 3, 4, 6
    ids = torch.randint(0, Vn, (B, F), generator=g)
    ids[1, 0] = -1
    ids[2] = ids[0]                                     # duplicate ids
    labels = torch.randint(0, 2, (B, 1), generator=g)
    tabs = [_rand(g, Vn, K, scale=0.3) for _ in range(F)]
    lws = [_rand(g, Vn, scale=0.1) for _ in range(F)]
    mlp = _mlp_params(g, [F * K, 5, 4, 1])
    bn = [1 + _rand(g, 5, scale=0.1), _rand(g, 5, scale=0.1), 1 + _rand(g, 4, scale=0.1), _rand(g, 4, scale=0.1)]

    def loss(*p):
        tabs, lws, lb, mlp, bn = p[:F], p[F:2 * F], p[2 * F], p[2 * F + 1:2 * F + 7], p[2 * F + 7:]
        emb = torch.cat([M.onehot(tabs[f], ids[:, f]) for f in range(F)], dim=1)
        layers = _pairs(mlp)
        bns = [{"gamma": bn[0], "beta": bn[1]}, {"gamma": bn[2], "beta": bn[3]}]
        logits, _ = M.deepfm(emb, F, K, layers[:2], layers[2], M.linear_logit(lws, ids, lb), bns=bns, train=True)
        return M.weighted_loss(logits, labels, None, "sum")
    _gradcheck(loss, tabs + lws + [_rand(g, 1, scale=0.1)] + mlp + bn)


def test_gradcheck_dcn_with_training_batch_norm():
    g = torch.Generator().manual_seed(2)
    B, d = 5, 7
    x0 = _rand(g, B, d, scale=0.5)
    labels = torch.randint(0, 2, (B, 1), generator=g)
    mlp = _mlp_params(g, [d, 6, 4])

    def loss(x0, cw, cb, beta, hw, hb, *mlp):
        logits, _ = M.dcn(x0, cw, cb, _pairs(mlp), [{"beta": beta}], (hw, hb), train=True)
        return M.weighted_loss(logits, labels, None, "mean")
    _gradcheck(loss, [x0, _rand(g, 2, d, scale=0.3), _rand(g, 2, d, scale=0.1), _rand(g, 6, scale=0.1), _rand(g, 1, d + 4, scale=0.3),
                      _rand(g, 1, scale=0.1)] + mlp)


def test_gradcheck_xdeepfm():
    g = torch.Generator().manual_seed(3)
    B, m, D, Hs = 4, 3, 4, (5, 3)
    labels = torch.randint(0, 2, (B, 1), generator=g)
    Ws = [_rand(g, 5, m * m, scale=0.3), _rand(g, 3, 5 * m, scale=0.3)]
    mlp = _mlp_params(g, [m * D, 5, 1])

    def loss(emb, W0, W1, cw, cb, lin, *mlp):
        layers = _pairs(mlp)
        return M.weighted_loss(M.xdeepfm(emb, m, D, [W0, W1], (cw, cb), layers[:1], layers[1], lin), labels, None, "sum")
    _gradcheck(loss, [_rand(g, B, m * D, scale=0.4)] + Ws + [_rand(g, 1, sum(Hs), scale=0.4), _rand(g, 1, scale=0.1), _rand(g, B, 1, scale=0.1)] + mlp)


def test_gradcheck_esmm_loss():
    g = torch.Generator().manual_seed(4)
    B, d = 5, 6
    click, conv = torch.randint(0, 2, (B,), generator=g), torch.randint(0, 2, (B,), generator=g)
    w = torch.rand(B, 1, generator=g, dtype=torch.float64) + 0.5
    ctr, cvr = _mlp_params(g, [d, 5, 4, 1]), _mlp_params(g, [d, 5, 4, 1])

    def loss(xa, xb, *p):
        a, b = _pairs(p[:6]), _pairs(p[6:])
        out = M.esmm(xa, xb, (a[:2], a[2]), (b[:2], b[2]))
        return M.esmm_loss(out, click, conv, ctr_weights=w)
    _gradcheck(loss, [_rand(g, B, d, scale=0.5), _rand(g, B, d, scale=0.5)] + ctr + cvr)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("kind", ["sigmoid", "prelu", "dice"])
def test_gradcheck_din(kind, normalize):
    g = torch.Generator().manual_seed(6)
    B, T_, K, Vn, H1, H2 = 4, 3, 4, 7, 6, 4
    hist = torch.randint(0, Vn, (B, T_), generator=g)
    hist[0, 1] = -1
    hl = torch.tensor([3, 0, 2, 3])                     # one empty history
    cand = torch.tensor([2, 5, -1, 2])                  # a pruned candidate, a duplicate
    labels = torch.randint(0, 2, (B, 1), generator=g)
    unit = [_rand(g, 4 * K, H1, scale=(4 * K) ** -0.5), _rand(g, H1, scale=0.1), _rand(g, H1, H2, scale=H1 ** -0.5), _rand(g, H2, scale=0.1),
            _rand(g, H2, scale=H2 ** -0.5), _rand(g, 1, scale=0.1)]
    tail_kind = "relu" if kind == "sigmoid" else kind
    alphas = [0.25 + _rand(g, n, scale=0.1) for n in (H1, H2, 5)]
    mlp = _mlp_params(g, [2 * K, 5, 1])

    def loss(table, *p):
        unit, alphas, mlp = p[:6], p[6:9], p[9:]
        layers = _pairs(mlp)
        acts = [{"alpha": alphas[0]}, {"alpha": alphas[1]}] if kind != "sigmoid" else None
        dacts = [{"alpha": alphas[2]}] if tail_kind != "relu" else None
        logits, _, _ = M.din(table, hist, hl, cand, unit, layers[:1], layers[1], attention_activation=kind, attention_acts=acts,
                             normalize=normalize, dnn_activation=tail_kind, dnn_acts=dacts, train=True)
        return M.weighted_loss(logits, labels, None, "mean")
    _gradcheck(loss, [_rand(g, Vn, K, scale=0.3)] + unit + alphas + mlp)
