"""Dropout on the HIP training path (csrc/dropout.hip): the masks bit for bit against the NumPy restatement of the generator
(tests/dropout_ref.py), the values against (x / keep_prob) * mask in fp32, the backward on the forward's mask, the masks' statistics, the
models against float64 autograd on the same masks (tests/dropout_ref64.py), magnitudes that a stale row maximum would overflow, the routing
(no library dropout, the fused nodes kept) and a captured training step."""
import numpy as np
import pytest
import torch

from tests import dropout_ref as R
from tests import dropout_ref64 as D
from tests import model_ref64 as M

pytestmark = pytest.mark.gpu

RATES = (0.1, 0.5, 0.9)


def _close(got, ref, tol=1e-5):
    """tests/test_gpu_backward.py:_close."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref) / (1 + np.abs(ref))
    print("max scaled err %.3e" % err.max())
    assert err.max() <= tol, "max scaled err %.3e" % err.max()


def _same_bits(got, ref):
    """fp32 tensors equal bit for bit, NaNs matching NaNs."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn)
    assert torch.equal(got[~gn].view(torch.int32), ref[~rn].view(torch.int32))


def _ref_values(x, mask, rate):
    """(x / keep_prob) * mask in torch fp32 on the host (IEEE division)."""
    keep = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(rate, dtype=torch.float32)
    return (x.detach().cpu() / keep) * torch.as_tensor(mask).reshape(x.shape).to(torch.float32)


# ---- 1. the mask, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 4099, 2 ** 20 + 3])
def test_mask_matches_the_reference_generator(built_lib, n):
    from dir_amd import ops
    seed = 0x1234567887654321
    st = ops.DropoutState(seed=seed)
    for rate in RATES:
        for sid, draw in ((0, 0), (7, 5), (0, 0xfffffffe)):
            st.set_state((seed, draw))
            got = ops.dropout_mask(n, rate, st, sid).cpu().numpy()
            assert np.array_equal(got, R.mask(n, rate, seed, draw=draw, stream_id=sid)), (n, rate, sid, draw)
    assert st.get_state() == (seed, 0xfffffffe)


def test_mask_counter_high_word_and_unaligned_first(built_lib):
    from dir_amd import ops
    seed = 77
    st = ops.DropoutState(seed=seed).set_state((seed, 3))
    first = 2 ** 34 - 32                     # q crosses 2^32 inside the 64 elements: the counter's second word
    got = ops.dropout_mask(64, 0.5, st, 7, first=first).cpu().numpy()
    assert np.array_equal(got, R.mask(64, 0.5, seed, draw=3, stream_id=7, first=first))
    for first in (1, 2, 3, 2 ** 34 - 31):      # quads that straddle two blocks
        got = ops.dropout_mask(70, 0.5, st, 1, first=first).cpu().numpy()
        assert np.array_equal(got, R.mask(70, 0.5, seed, draw=3, stream_id=1, first=first)), first
    # `used` (seed, draw) overrides both of the state's words
    used = torch.tensor([1234, 9], dtype=torch.int64, device="cuda")
    assert np.array_equal(ops.dropout_mask(64, 0.5, st, 0, used=used).cpu().numpy(), R.mask(64, 0.5, 1234, draw=9))


# ---- 2. the values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (0.0,) + RATES)
def test_values_match_division_then_mask(built_lib, rate):
    from dir_amd import ops
    seed = 2024
    st = ops.DropoutState(seed=seed).set_state((seed, 2))
    g = torch.Generator().manual_seed(3)
    for n in (1, 3, 4, 5, 65, 4099, 300001):
        x = torch.randn(n, generator=g)
        if n >= 65:
            x[:8] = torch.tensor([float("inf"), float("-inf"), float("nan"), -0.0, 0.0, float("nan"), float("inf"), -0.0])
            x[n - 3:] = torch.tensor([float("nan"), -0.0, float("inf")])           # (the tail elements too)
        ref = _ref_values(x, R.mask(n, rate, seed, draw=2, stream_id=4), rate) if rate else x
        xd = x.cuda()
        out, used = ops.dropout(xd, rate, st, 4, want_used=True)
        _same_bits(out, ref)
        assert used.tolist() == [seed, 2]
        assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32))          # the input is left alone
        alias = xd.clone()
        assert ops.dropout(alias, rate, st, 4, out=alias) is alias
        _same_bits(alias, ref)
        # a view 4 bytes into an allocation: the scalar path, the same values
        buf = torch.empty(n + 1, device="cuda")
        buf[1:].copy_(xd)
        _same_bits(ops.dropout(buf[1:], rate, st, 4), ref)
    # 2-D: the element index is the flat index
    x2 = torch.randn((37, 12), generator=g)
    ref2 = _ref_values(x2, R.mask(37 * 12, rate, seed, draw=2, stream_id=0), rate) if rate else x2
    _same_bits(ops.dropout(x2.cuda(), rate, st, 0), ref2)


def test_rate_outside_the_unit_interval_raises(built_lib):
    from dir_amd import ops
    st = ops.DropoutState(seed=1)
    x = torch.ones(8, device="cuda")
    for rate in (1.0, -0.1):
        with pytest.raises(ValueError):
            ops.dropout(x, rate, st)
        with pytest.raises(ValueError):
            ops.dropout_mask(8, rate, st)


def test_bn_affine_dropout_matches_affine_then_dropout(built_lib):
    from dir_amd import ops
    seed = 5
    st = ops.DropoutState(seed=seed).set_state((seed, 1))
    g = torch.Generator().manual_seed(8)
    B, N = 37, 24
    y, scale, shift = torch.randn((B, N), generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    out, used = ops.bn_affine_dropout(y.cuda(), scale.cuda(), shift.cuda(), 0.5, st, 3, want_used=True)
    aff = torch.from_numpy(np.float32(y.double().numpy() * scale.double().numpy() + shift.double().numpy()))   # (fma: one rounding)
    _same_bits(out, _ref_values(aff, R.mask(B * N, 0.5, seed, draw=1, stream_id=3), 0.5))
    assert used.tolist() == [seed, 1]


# ---- 3. the backward uses the forward's mask ---------------------------------------------------------------------------------------------
def test_backward_regenerates_the_forwards_mask(built_lib):
    from dir_amd import autograd as ag, ops
    seed = 99
    st = ops.DropoutState(seed=seed)
    gen = torch.Generator().manual_seed(1)
    shape = (1001, 37)
    n = shape[0] * shape[1]
    xa = torch.randn(shape, generator=gen).cuda().requires_grad_(True)
    xb = torch.randn(shape, generator=gen).cuda().requires_grad_(True)
    a = ag.dropout(xa, 0.5, st, 0)                                  # forward A (draw 0)
    a2 = ag.dropout(xa, 0.5, st, 1)                                 # a second site of the same shape in the same forward
    mask_a, mask_a2 = ops.dropout_mask(n, 0.5, st, 0).cpu().numpy(), ops.dropout_mask(n, 0.5, st, 1).cpu().numpy()
    st.advance()
    b = ag.dropout(xb, 0.5, st, 0)                                  # forward B (draw 1) on the same state
    mask_b = ops.dropout_mask(n, 0.5, st, 0).cpu().numpy()
    st.advance()
    assert np.array_equal(mask_a, R.mask(n, 0.5, seed, draw=0)) and np.array_equal(mask_b, R.mask(n, 0.5, seed, draw=1))
    assert not np.array_equal(mask_a, mask_b)                       # two consecutive steps
    assert not np.array_equal(mask_a, mask_a2)                      # two sites of one forward
    _same_bits(a, _ref_values(xa, mask_a, 0.5))
    _same_bits(b, _ref_values(xb, mask_b, 0.5))
    g = torch.randn(shape, generator=gen).cuda()
    st.set_state((777, 40))                                         # a new seed as well: the backward reads nothing of the state
    a.backward(g)                                                   # backward A, two draws and one reseeding later
    _same_bits(xa.grad, _ref_values(g, mask_a, 0.5))
    xa.grad = None
    a2.backward(g)
    _same_bits(xa.grad, _ref_values(g, mask_a2, 0.5))
    assert st.get_state() == (777, 40)


def test_set_state_reproduces_a_sequence(built_lib):
    from dir_amd import ops
    st = ops.DropoutState(seed=31337)
    st.advance().advance()
    saved = st.get_state()
    assert saved == (31337, 2)
    x = torch.randn(5000, generator=torch.Generator().manual_seed(2)).cuda()

    def run():
        outs = []
        for _ in range(3):
            outs.append(ops.dropout(x, 0.5, st, 0))
            st.advance()
        return outs
    first = run()
    assert st.get_state() == (31337, 5)
    assert not torch.equal(first[0], first[1])
    st.set_state(saved)
    assert all(torch.equal(p, q) for p, q in zip(first, run()))
    st.manual_seed(31337)
    assert st.get_state() == (31337, 0)
    # the default seed is torch's
    torch.manual_seed(424242)
    assert ops.DropoutState().get_state() == (424242, 0)


# ---- 4. statistics of the mask --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_mask_statistics(built_lib, rate):
    from dir_amd import ops
    B, N, seed = 4096, 256, 20240607
    n = B * N
    st = ops.DropoutState(seed=seed)
    keep = 1.0 - rate
    m0 = ops.dropout_mask(n, rate, st, 0).cpu().numpy().astype(np.int64).reshape(B, N)
    m_s1 = ops.dropout_mask(n, rate, st, 1).cpu().numpy().astype(np.int64).reshape(B, N)
    m_d1 = ops.dropout_mask(n, rate, st.advance(), 0).cpu().numpy().astype(np.int64).reshape(B, N)
    z = lambda count, trials, p: (count - trials * p) / np.sqrt(trials * p * (1 - p))      # noqa: E731
    zt = z(m0.sum(), n, keep)
    zr, zc = z(m0.sum(axis=1), N, keep), z(m0.sum(axis=0), B, keep)
    agree = keep * keep + rate * rate
    za1, za2 = z((m0 == m_s1).sum(), n, agree), z((m0 == m_d1).sum(), n, agree)
    print("rate %.1f: total z %.2f, rows max |z| %.2f, columns max |z| %.2f, agreement z %.2f (stream 1) %.2f (draw 1)"
          % (rate, zt, np.abs(zr).max(), np.abs(zc).max(), za1, za2))
    assert abs(zt) <= 4.0
    assert np.abs(zr).max() <= 5.0 and np.abs(zc).max() <= 5.0
    assert abs(za1) <= 4.0 and abs(za2) <= 4.0


# ---- the models ---------------------------------------------------------------------------------------------------------------------------
F_, K_, VOCABS = 4, 4, (50, 61, 40, 77)


def _fill(model, seed, table_scale=0.3, cross_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "embedding_weights" in name:
                v = torch.randn(tuple(p.shape), generator=g) * table_scale
            elif name == "cross_w":
                v = torch.randn(tuple(p.shape), generator=g) * p.shape[1] ** -0.5 * cross_scale
            elif p.dim() == 2:
                v = torch.randn(tuple(p.shape), generator=g) * p.shape[1] ** -0.5
            else:
                v = torch.randn(tuple(p.shape), generator=g) * 0.1
            p.copy_(v.to(p.device))


def _lin(l):
    return (l.weight, l.bias)


def _build(kind, rate, B=256, hidden=(32, 16), batch_norm=False, table_scale=0.3, cross_scale=1.0):
    from dir_amd import feature_column as fc
    torch.manual_seed(1234)                                   # (the models' dropout states take torch's seed)
    cats = [fc.categorical_column_with_identity("C%d" % f, VOCABS[f]) for f in range(F_)]
    embs = [fc.embedding_column(c, K_) for c in cats]
    g = torch.Generator().manual_seed(17)
    ids = torch.stack([torch.randint(0, v, (B,), generator=g) for v in VOCABS], dim=1).cuda()
    feats = {"C%d" % f: ids[:, f].contiguous() for f in range(F_)}
    labels = torch.randint(0, 2, (B, 1), generator=g).float().cuda()
    if kind == "deepfm":
        from dir_amd.deepfm import DeepFM
        model = DeepFM(linear_feature_columns=cats, dnn_feature_columns=embs, dnn_hidden_units=list(hidden), fm_embedding_size=K_,
                       dnn_dropout=rate, batch_norm=batch_norm)
    elif kind == "esmm":
        from dir_amd.esmm import ESMM
        model = ESMM(columns=embs, dnn_hidden_units=list(hidden), dnn_dropout=rate)
        labels = {"click_label": labels, "convert_label": torch.randint(0, 2, (B, 1), generator=g).float().cuda()}
    else:
        from dir_amd.dcn import DeepCrossNetwork
        model = DeepCrossNetwork(columns=embs, cross_layer_num=2, dnn_hidden_units=list(hidden), batch_norm=batch_norm, dnn_dropout=rate)
    model = model.cuda().train()
    _fill(model, 5, table_scale, cross_scale)
    return model, feats, labels, ids


def _params(kind, model):
    if kind == "deepfm":
        P = {"tabs": list(model.embedding_weights), "lws": list(model.linear_weights), "lb": model.linear_bias,
             "hidden": [_lin(l) for l in model.hidden], "head": _lin(model.logits_layer)}
        if len(model.bns):
            P["bns"] = [{"gamma": b.gamma, "beta": b.beta} for b in model.bns]
        return P
    if kind == "esmm":
        return {t: {"tabs": list(m.input_layer.embedding_weights), "hidden": [_lin(l) for l in m.hidden], "head": _lin(m.logits)}
                for t, m in (("ctr", model.ctr_model), ("cvr", model.cvr_model))}
    P = {"tabs": list(model.embedding_weights), "cross_w": model.cross_w, "cross_b": model.cross_b,
         "hidden": [_lin(l) for l in model.hidden], "head": _lin(model.logits_layer)}
    if len(model.bns):
        P["beta"] = [b.beta for b in model.bns]
    return P


def _masks(model, rate, B, widths, base=0):
    from dir_amd import ops
    return [ops.dropout_mask(B * w, rate, model.dropout_rng, base + i).reshape(B, w).double() for i, w in enumerate(widths)]


def _reference(kind, model, ids, labels, rate, hidden):
    """float64 autograd on the masks of the model's current draw -> (leaves, logits, loss)."""
    B = ids.shape[0]
    keep = D.keep_prob(rate)
    P = M.leaves(_params(kind, model))
    emb = lambda tabs: torch.cat([M.onehot(t, ids[:, f]) for f, t in enumerate(tabs)], dim=1)      # noqa: E731
    if kind == "deepfm":
        logits, _ = D.deepfm(emb(P["tabs"]), F_, K_, P["hidden"], P["head"], M.linear_logit(P["lws"], ids, P["lb"]),
                             _masks(model, rate, B, hidden), keep, bns=P.get("bns"), eps=1e-3)
        return P, logits, M.weighted_loss(logits, labels, None, "sum")
    if kind == "esmm":
        L = len(hidden)
        logits = D.esmm(emb(P["ctr"]["tabs"]), emb(P["cvr"]["tabs"]), (P["ctr"]["hidden"], P["ctr"]["head"]),
                        (P["cvr"]["hidden"], P["cvr"]["head"]), _masks(model, rate, B, hidden), _masks(model, rate, B, hidden, base=L), keep)
        return P, logits, M.esmm_loss(logits, labels["click_label"], labels["convert_label"])
    logits, _ = D.dcn(emb(P["tabs"]), P["cross_w"], P["cross_b"], P["hidden"], P.get("beta"), P["head"], _masks(model, rate, B, hidden), keep)
    return P, logits, M.weighted_loss(logits, labels, None, "mean")


def _loss(kind, model, feats, labels, logits):
    return model.get_loss(feats, labels, logits)[0] if kind == "esmm" else model.create_loss(feats, logits, labels)[0]


def _check_against_float64(kind, rate, hidden, batch_norm=False, table_scale=0.3, cross_scale=1.0):
    model, feats, labels, ids = _build(kind, rate, hidden=hidden, batch_norm=batch_norm, table_scale=table_scale, cross_scale=cross_scale)
    logits = model(feats)
    loss = _loss(kind, model, feats, labels, logits)
    loss.backward()
    torch.cuda.synchronize()
    draw = model.dropout_rng.get_state()[1]
    assert draw == 1                                           # one draw per training forward
    P, ref_logits, ref_loss = _reference(kind, model, ids, labels, rate, hidden)
    pairs = list(zip(M.flatten(_params(kind, model)), M.flatten(P)))
    ref_grads = torch.autograd.grad(ref_loss, [r for _, (_, r) in pairs])
    if kind == "esmm":
        for k in ("ctr_logits", "cvr_logits", "ctcvr_logits"):
            _close(logits[k], ref_logits[k])
    else:
        _close(logits, ref_logits)
    _close(loss, ref_loss)
    for ((path, p), _), rg in zip(pairs, ref_grads):
        assert p.grad is not None, path
        print(path, end=": ")
        _close(p.grad.to_dense() if p.grad.is_sparse else p.grad, rg)
    return model


# ---- 5. the models against float64 autograd on the same masks -------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (0.2, 0.5))
@pytest.mark.parametrize("kind,hidden,bn", [("deepfm", (32, 16), False), ("deepfm", (32, 16), True), ("esmm", (32, 16), False),
                                            ("dcn", (32, 16, 8), True), ("dcn", (32, 16), True), ("dcn", (32, 16), False)])
def test_models_match_float64_on_the_same_masks(built_lib, kind, hidden, bn, rate):
    _check_against_float64(kind, rate, hidden, batch_norm=bn)


# ---- 6. magnitudes ---------------------------------------------------------------------------------------------------------------------------
def test_stack_with_large_activations_rate_09(built_lib):
    """A two-layer stack at the batch the row-scaled fp16 x 2 kernels take, first-layer activations ~1e6, rate 0.9: the second layer and the
    weight gradients must scale by the maxima of the DROPPED activation (ten times the layer's own; a stale maximum overflows fp16).
    The bar is the scaled error |got - ref| / (1 + |ref|) <= 1e-5, which at these magnitudes is an elementwise relative error: the case is
    laid out so that no compared sum cancels -- the second layer's bias keeps its outputs near 5e7 (its ReLU open), the loss weights are
    positive (dW2, db2 are sums of non-negative terms) and small enough that the sums which do cancel (dW1, db1, dx) are O(1) or less."""
    from dir_amd import dense, ops
    B, d, rate = 12288, 64, 0.9
    assert ops.dense_auto_arith(B, d, 128) == "bf16x3" and ops.dense_auto_arith(B, 128, 128) == "bf16x3"      # the row-scaled kernel's routing
    keep = D.keep_prob(rate)
    g = torch.Generator().manual_seed(4)
    lins = [torch.nn.Linear(d, 128), torch.nn.Linear(128, 128)]
    with torch.no_grad():
        lins[0].weight.copy_(torch.randn((128, d), generator=g) * 1e3 * d ** -0.5)
        lins[0].bias.copy_(torch.randn(128, generator=g) * 1e5)
        lins[1].weight.copy_(torch.randn((128, 128), generator=g) * 128 ** -0.5)
        lins[1].bias.copy_(5e7 + torch.randn(128, generator=g) * 1e6)
    lins = [l.cuda() for l in lins]
    st = ops.DropoutState(seed=12)
    masks = [ops.dropout_mask(B * 128, rate, st, s).reshape(B, 128).double() for s in (0, 1)]
    x = torch.randn((B, d), generator=g) * 1e3
    W = [l.weight.detach().double() for l in lins]
    bs = [l.bias.detach().double() for l in lins]
    for _ in range(20):       # rows with a pre-activation within fp32's rounding of a kink draw again (tests/test_gpu_model_grads.py: build)
        xd = x.cuda().double()
        p1 = xd @ W[0].t() + bs[0]
        p2 = D.drop(torch.relu(p1), masks[0], keep) @ W[1].t() + bs[1]
        assert float(p2.min()) > 1e7
        near = (p1.abs().min(dim=1).values < 10.0).cpu()               # (|p1| ~ 1e6: ten times fp32's rounding of it)
        if not near.any():
            break
        x[near] = torch.randn((int(near.sum()), d), generator=g) * 1e3
    assert not near.any()
    r = ((torch.rand((B, 128), generator=g) + 0.5) * 1e-6).cuda()
    xg = x.cuda().requires_grad_(True)
    out = dense.mlp_stack(lins, xg, embedding_input=False, drop=dense.Drop(rate, st, [0, 1]))
    (out * r).sum().backward()
    torch.cuda.synchronize()
    P = M.leaves({"x": xg, "hidden": [_lin(l) for l in lins]})
    h = P["x"]
    for (Wl, bl), m in zip(P["hidden"], masks):
        h = D.drop(torch.relu(M.dense(h, Wl, bl)), m, keep)
    assert float(h.detach().abs().max()) > 1e6
    ref = torch.autograd.grad((h * r.double()).sum(), [P["x"]] + [t for pr in P["hidden"] for t in pr])
    _close(out, h)
    for got, rg in zip([xg.grad] + [t.grad for l in lins for t in (l.weight, l.bias)], ref):
        _close(got, rg)


def test_dcn_batch_norm_rate_09_inputs_times_1000(built_lib):
    """The DCN cases with their inputs (the embedding rows) a thousand times larger: the layers behind a batch norm read a normalised
    activation times up to 1 / keep_prob = 10.  The cross branch is cubic in the input's scale (two layers of x0 (x . w)): with O(1) cross
    weights the logits would be sums of ~1e8 terms that cancel to 1e5, where the scaled error is fp32's own cancellation and says nothing
    about the dropout.  The cross weights are therefore a thousand times smaller (x . w stays O(1)): the logits keep the inputs' magnitude
    and the bar holds what it holds in the other cases."""
    _check_against_float64("dcn", 0.9, (32, 16, 8), batch_norm=True, table_scale=300.0, cross_scale=1e-3)
    _check_against_float64("dcn", 0.9, (32, 16), batch_norm=True, table_scale=300.0, cross_scale=1e-3)


# ---- 7. routing ------------------------------------------------------------------------------------------------------------------------------
def _node_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo += [n for n, _ in fn.next_functions]
    return names


def test_training_with_dropout_stays_on_the_hip_nodes(built_lib, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.dropout on the HIP training path")
    monkeypatch.setattr(torch.nn.functional, "dropout", refuse)
    # DeepFM (binary head): the tower and the logit layer as one node
    model, feats, labels, _ = _build("deepfm", 0.5)
    logits = model(feats)
    assert "_MlpHeadFnBackward" in _node_names(logits)
    _loss("deepfm", model, feats, labels, logits).backward()
    # DeepFM with a batch norm: layer + dropout + batch norm as one node per layer
    model, feats, labels, _ = _build("deepfm", 0.5, batch_norm=True)
    logits = model(feats)
    assert "_DenseBnFnBackward" in _node_names(logits)
    _loss("deepfm", model, feats, labels, logits).backward()
    # ESMM: both towers
    model, feats, labels, _ = _build("esmm", 0.5)
    out = model(feats)
    assert type(out["ctr_logits"].grad_fn).__name__ == "_MlpHeadFnBackward" and type(out["cvr_logits"].grad_fn).__name__ == "_MlpHeadFnBackward"
    _loss("esmm", model, feats, labels, out).backward()
    # a multi-class DeepFM keeps the stack node
    from dir_amd import feature_column as fc
    from dir_amd.deepfm import DeepFM
    cats = [fc.categorical_column_with_identity("C%d" % f, VOCABS[f]) for f in range(F_)]
    m3 = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K_) for c in cats], dnn_hidden_units=[32, 16],
                fm_embedding_size=K_, dnn_dropout=0.5, n_classes=3).cuda().train()
    l3 = m3(feats)
    assert "_MlpStackFnBackward" in _node_names(l3)
    l3.sum().backward()
    # DCN: the split logit form, the last layer's dropout inside the head node
    model, feats, labels, _ = _build("dcn", 0.5, hidden=(32, 16), batch_norm=True)
    got = []
    inner = model._train_logits
    monkeypatch.setattr(model, "_train_logits", lambda x0, cross: got.append(inner(x0, cross)) or got[-1])
    logits = model(feats)
    assert len(got) == 1 and isinstance(got[0], torch.Tensor) and logits is got[0]
    names = _node_names(logits)
    assert "_MlpHeadFnBackward" in names and "_DenseBnFnBackward" in names
    _loss("dcn", model, feats, labels, logits).backward()
    assert all(p.grad is not None for p in model.parameters())


def test_eval_and_no_grad_are_the_identity_and_leave_the_state(built_lib):
    from dir_amd.deepfm import _dropout_train, dropout_rng_of
    m = torch.nn.Module()
    x = torch.randn(64, 8, device="cuda")
    before = dropout_rng_of(m).get_state()
    with torch.no_grad():
        assert _dropout_train(m, x, 0.5) is x
    m.eval()
    assert _dropout_train(m, x, 0.5) is x
    assert _dropout_train(torch.nn.Module(), x, None) is x
    assert dropout_rng_of(m).get_state() == before
    m.train()
    d = _dropout_train(m, x, 0.5)
    assert set((d / x).round().unique().tolist()) == {0.0, 2.0}
    for kind, bn in (("deepfm", False), ("esmm", False), ("dcn", True)):
        model, feats, _, _ = _build(kind, 0.5, hidden=(32, 16), batch_norm=bn)
        state = model.dropout_rng.get_state()
        with torch.no_grad():
            a = model(feats)
        model.eval()
        b = model(feats)
        with torch.no_grad():
            c = model(feats)
        assert model.dropout_rng.get_state() == state
        first = lambda o: o["ctr_logits"] if isinstance(o, dict) else o      # noqa: E731
        _close(first(b), first(c))                               # no site drops anything: eval() with and without autograd agree
        if not bn:
            _close(first(a), first(c))                           # (train() under no_grad takes the inference forms: the moving statistics)
        model.train()
        model(feats)
        assert model.dropout_rng.get_state() == (state[0], state[1] + 1)


# ---- 8. a captured training step ---------------------------------------------------------------------------------------------------------------
def test_captured_step_with_dropout_equals_eager_steps(built_lib):
    """The pattern of tests/test_gpu_graph_replay.py (a captured graph against its eager twin, bit for bit) on a training step held in
    ops.CapturedStep, with dnn_dropout = 0.5: the state's words live on the device and advance inside the
    graph, so two replays from one set_state equal two eager steps from the same state and parameters bit for bit -- on different masks."""
    from dir_amd import autograd as ag, feature_column as fc, ops
    from dir_amd.deepfm import DeepFM
    B, F, K, V = 4096, 8, 16, 2000

    def build():
        torch.manual_seed(11)
        cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
        m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[64, 32],
                   fm_embedding_size=K, dnn_dropout=0.5).cuda()
        m.fused_sparse_adagrad(lr=0.05, packed=True)
        m.fused_sparse_ftrl(lr=0.2)
        skip = {id(p) for p in m.linear_weights} | {id(p) for p in m.embedding_weights} | {id(m.linear_bias)}
        od = ag.Adagrad([p for p in m.parameters() if id(p) not in skip], lr=0.05, initial_accumulator_value=0.1)
        ol = ag.Ftrl([m.linear_bias], lr=0.2)
        return m, od, ol

    def step(m, od, ol, feats, y):
        od.zero_grad(set_to_none=False)
        ol.zero_grad(set_to_none=False)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(m(feats), y)
        loss.backward()
        od.step()
        ol.step()
        return loss

    gen = torch.Generator(device="cuda").manual_seed(5)
    batches = [torch.randint(0, V, (B, F), generator=gen, device="cuda") for _ in range(3)]
    labels = [(torch.rand((B, 1), generator=gen, device="cuda") < 0.25).float() for _ in range(3)]
    feats = lambda i: {"C%d" % f: batches[i][:, f] for f in range(F)}      # noqa: E731
    ma, oda, ola = build()          # eager twin
    mb, odb, olb = build()          # captured
    ids_s, y_s = batches[0].clone(), labels[0].clone()
    feats_s = {"C%d" % f: ids_s[:, f] for f in range(F)}
    cap = ops.CapturedStep(lambda: step(mb, odb, olb, feats_s, y_s), written=ops.written_of(mb), warmup=3)
    for _ in range(3):              # the constructor's warm-up steps are real steps: the twin takes the same three
        step(ma, oda, ola, feats(0), labels[0])
    torch.cuda.synchronize()
    assert ma.dropout_rng.get_state() == mb.dropout_rng.get_state() == (11, 3)
    assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters()))
    ma.dropout_rng.set_state((11, 100))
    mb.dropout_rng.set_state((11, 100))
    n0 = B * 64
    masks = []
    for i in (1, 2):
        ids_s.copy_(batches[i]); y_s.copy_(labels[i])
        cap.replay()
        masks.append(ops.dropout_mask(n0, 0.5, mb.dropout_rng, 0).cpu())
        step(ma, oda, ola, feats(i), labels[i])
    torch.cuda.synchronize()
    assert mb.dropout_rng.get_state() == ma.dropout_rng.get_state() == (11, 102)
    assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters())), "replays differ from eager steps"
    assert not torch.equal(masks[0], masks[1])
    assert np.array_equal(masks[0].numpy(), R.mask(n0, 0.5, 11, draw=101)) and np.array_equal(masks[1].numpy(), R.mask(n0, 0.5, 11, draw=102))
