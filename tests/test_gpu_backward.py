"""GPU tests of the backward path: HIP backward kernels and the autograd wrappers against
float64 torch autograd of the same reference expressions (deepFM.py:329-334, DeepCrossNetwork.py:345-346,363-365),
tolerance 1e-5 * (1 + |ref|); plus a few optimiser steps of a small DeepFM / DCN with the reference's optimisers."""
import numpy as np
import pytest
import torch

from oracle.np_ref import sparse_adam_step

pytestmark = pytest.mark.gpu


def _close(got, ref, tol=1e-5):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return
    err = np.abs(got - ref) / (1 + np.abs(ref))
    assert err.max() <= tol, "max scaled err %.3e" % err.max()


def _ref_fm(emb, F, K):
    e = emb.view(-1, F, K)
    return 0.5 * (e.sum(1) ** 2 - (e ** 2).sum(1)).sum(1, keepdim=True)


def _ref_cross(x0, w, b):
    xl = x0
    for l in range(w.shape[0]):
        xl = x0 * (xl @ w[l])[:, None] + b[l] + xl
    return xl


@pytest.mark.parametrize("B,F,K", [(1, 1, 4), (64, 26, 16), (1000, 26, 8), (333, 5, 64), (77, 3, 6), (50, 4, 1)])
def test_fm_backward(built_lib, B, F, K):
    from dir_amd import ops
    g = torch.Generator().manual_seed(B + K)
    emb = (torch.randn(B, F * K, generator=g) * 0.3)
    gout = torch.randn(B, 1, generator=g)
    gdnn = torch.randn(B, F * K, generator=g)
    e64 = emb.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(_ref_fm(e64, F, K), e64, gout.double())
    got = ops.fm_logit_backward(emb.cuda(), gout.cuda(), F, K)
    _close(got, ref)
    got2 = ops.fm_logit_backward(emb.cuda(), gout.cuda(), F, K, add_in=gdnn.cuda())
    _close(got2, ref + gdnn.double())


@pytest.mark.parametrize("B,d,L", [(1, 4, 1), (64, 416, 3), (257, 429, 3), (100, 51, 2), (33, 1024, 4), (500, 64, 6), (9, 10, 0), (40, 2048, 2)])
def test_cross_backward(built_lib, B, d, L):
    from dir_amd import ops
    g = torch.Generator().manual_seed(d + L)
    x0 = torch.randn(B, d, generator=g) * 0.3
    w = (torch.randn(max(L, 1), d, generator=g) * 0.1).clamp(-0.2, 0.2)[:L]
    b = (torch.randn(max(L, 1), d, generator=g) * 0.1).clamp(-0.2, 0.2)[:L]
    gout = torch.randn(B, d, generator=g)
    x64, w64, b64 = x0.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    out = _ref_cross(x64, w64, b64)
    if L > 0:
        rx, rw, rb = torch.autograd.grad(out, (x64, w64, b64), gout.double())
    else:
        (rx,) = torch.autograd.grad(out, (x64,), gout.double())
        rw = rb = torch.zeros(0, d, dtype=torch.float64)
    gx, gw, gb = ops.cross_network_backward(x0.cuda(), w.cuda().reshape(L, d), b.cuda().reshape(L, d), gout.cuda())
    _close(gx, rx)
    # batch-summed weight gradients: scale the bar by sqrt(B) terms of magnitude |g||x|
    _close(gw, rw, tol=1e-5 * max(1.0, B ** 0.5))
    _close(gb, rb, tol=1e-5 * max(1.0, B ** 0.5))
    # reproducible: fixed-order partial sums
    gx2, gw2, gb2 = ops.cross_network_backward(x0.cuda(), w.cuda().reshape(L, d), b.cuda().reshape(L, d), gout.cuda())
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2) and torch.equal(gx, gx2)


def test_deepfm_autograd_matches_float64(built_lib):
    """Whole-model gradients: DeepFM with HIP forward + HIP/sparse backward vs the same graph in float64 torch."""
    from dir_amd.deepfm import DeepFM
    from dir_amd import feature_column as fc
    torch.manual_seed(3)
    B, F, K, V = 200, 6, 8, 40
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
    model = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                   dnn_hidden_units=[16, 8], fm_embedding_size=K).cuda()
    with torch.no_grad():
        for w in model.linear_weights:
            w.normal_(0, 0.1)
    ids = torch.randint(0, V, (B, F))
    ids[::7, 2] = -1                                   # pruned ids get no gradient
    labels = torch.randint(0, 2, (B, 1)).float()
    feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
    logits = model(feats)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels.cuda(), reduction="sum")   # head: SUM reduction (deepFM.py:72)
    loss.backward()
    # float64 reference graph
    tabs = [p.detach().cpu().double().requires_grad_(True) for p in model.embedding_weights]
    lws = [p.detach().cpu().double().requires_grad_(True) for p in model.linear_weights]
    lb = model.linear_bias.detach().cpu().double().requires_grad_(True)
    hid = [(l.weight.detach().cpu().double().requires_grad_(True), l.bias.detach().cpu().double().requires_grad_(True)) for l in model.hidden]
    lw, lbias = model.logits_layer.weight.detach().cpu().double().requires_grad_(True), model.logits_layer.bias.detach().cpu().double().requires_grad_(True)
    ok = (ids >= 0)
    cl = ids.clamp(min=0)
    emb = torch.cat([tabs[f][cl[:, f]] * ok[:, f:f + 1].double() for f in range(F)], 1)
    net = emb
    for W, bb in hid:
        net = torch.relu(net @ W.T + bb)
    ref_logits = _ref_fm(emb, F, K) + net @ lw.T + lbias + sum(lws[f][cl[:, f]] * ok[:, f].double() for f in range(F))[:, None] + lb
    ref_loss = torch.nn.functional.binary_cross_entropy_with_logits(ref_logits, labels.double(), reduction="sum")
    ref_loss.backward()
    _close(logits, ref_logits)
    for p, r in zip(model.embedding_weights, tabs):
        assert p.grad.is_sparse
        _close(p.grad.to_dense(), r.grad, tol=2e-5)
    for p, r in zip(model.linear_weights, lws):
        _close(p.grad.to_dense(), r.grad, tol=2e-5)
    _close(model.linear_bias.grad, lb.grad, tol=2e-5)
    for l, (W, bb) in zip(model.hidden, hid):
        _close(l.weight.grad, W.grad, tol=5e-5)
        _close(l.bias.grad, bb.grad, tol=5e-5)


def test_training_steps_reduce_loss(built_lib):
    """A few steps with the reference's optimisers (Adagrad on the dnn/fm/embedding side, FTRL on the linear side:
    deepFM.py:58,61) on a learnable synthetic target: the loss must go down; DCN likewise with Adam."""
    from dir_amd.deepfm import DeepFM
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd import feature_column as fc
    from dir_amd.autograd import Ftrl
    torch.manual_seed(0)
    B, F, K, V = 512, 5, 8, 30
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
    ids = torch.randint(0, V, (B, F))
    labels = (ids[:, 0] < V // 2).float().reshape(B, 1).cuda()      # learnable from one field
    feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
    model = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                   dnn_hidden_units=[32, 16], fm_embedding_size=K).cuda()
    lin = list(model.linear_weights) + [model.linear_bias]
    lin_ids = {id(p) for p in lin}
    opt_dnn = torch.optim.Adagrad([p for p in model.parameters() if id(p) not in lin_ids], lr=0.1, initial_accumulator_value=0.1)
    opt_lin = Ftrl(lin, lr=0.2)
    losses = []
    for _ in range(60):
        opt_dnn.zero_grad(); opt_lin.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model(feats), labels)
        loss.backward()
        opt_dnn.step(); opt_lin.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.75 * losses[0], losses[::10]
    dcn = DeepCrossNetwork(columns=[fc.embedding_column(c, K) for c in cats] + [fc.numeric_column("x")], cross_layer_num=2,
                           dnn_hidden_units=[32, 16], batch_norm=False).cuda()
    feats["x"] = torch.rand(B).cuda()
    opt = torch.optim.Adam([p for p in dcn.parameters() if p.dim() > 0 and not any(p is q for q in dcn.embedding_weights)], lr=0.01)
    opt_e = torch.optim.SparseAdam(list(dcn.embedding_weights), lr=0.01)
    l0 = None
    for _ in range(30):
        opt.zero_grad(); opt_e.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(dcn(feats), labels)
        loss.backward()
        opt.step(); opt_e.step()
        l0 = l0 or float(loss.detach())
    assert float(loss.detach()) < 0.8 * l0


@pytest.mark.parametrize("method", ["sorted", "chains"])
@pytest.mark.parametrize("B,F,K,V", [(1, 1, 4, 5), (300, 5, 16, 20), (4096, 26, 16, 1000), (777, 3, 6, 50), (500, 4, 64, 7),
                                     (3000, 2, 16, 3), (1025, 1, 8, 1), (700, 3, 16, 100000)])
def test_fused_sparse_adagrad(built_lib, B, F, K, V, method):
    """dir_sparse_adagrad_sorted_f32 / dir_sparse_adagrad_f32 vs a float64 dedup-sum Adagrad ([TF-upstream]: duplicates
    summed, then accum += g^2, var -= lr*g/sqrt(accum)); two consecutive steps (the chain heads must be left clean).
    V = 3 and V = 1: runs of equal rows spanning many 256-entry tiles (the carry / fix-up path of the sorted kernel)."""
    from dir_amd import ops
    rng = np.random.default_rng(B + K)
    tabs = [rng.standard_normal((V, K)).astype(np.float32) for _ in range(F)]
    dev = [torch.from_numpy(t.copy()).cuda() for t in tabs]
    opt = ops.SparseAdagrad(dev, lr=0.05, initial_accumulator_value=0.1, method=method)
    ref_w = [t.astype(np.float64) for t in tabs]
    ref_a = [np.full((V, K), 0.1) for _ in range(F)]
    for step in range(2):
        ids = rng.integers(-1, V, size=(B, F)).astype(np.int64)          # many duplicates, some pruned
        grad = (rng.standard_normal((B, F * K)) * 0.5).astype(np.float32)
        opt.step(torch.from_numpy(ids).cuda(), torch.from_numpy(grad).cuda())
        for f in range(F):
            gsum = np.zeros((V, K))
            ok = ids[:, f] >= 0
            np.add.at(gsum, ids[ok, f], grad[ok, f * K:(f + 1) * K].astype(np.float64))
            touched = np.zeros(V, bool); touched[ids[ok, f]] = True
            ref_a[f][touched] += gsum[touched] ** 2
            ref_w[f][touched] -= 0.05 * gsum[touched] / np.sqrt(ref_a[f][touched])
        if method == "chains":
            assert int((opt.head != -1).sum()) == 0
    for f in range(F):
        _close(dev[f], ref_w[f], tol=2e-5)
        _close(opt.accums[f], ref_a[f], tol=2e-5)


@pytest.mark.parametrize("method", ["sorted", "chains"])
def test_sparse_updates_never_write_outside_a_table(built_lib, method):
    """an id >= vocab_f must not alias a row of the NEXT table (key = row_base[f] + id) nor write past the
    end: the update kernels derive vocab_f from row_base / total_rows and skip such ids like pruned ones.  The tables live
    back to back in one arena with guard rows, so any stray write is caught."""
    from dir_amd import ops
    rng = np.random.default_rng(21)
    B, F, K = 2048, 3, 16
    vocab = [5, 9, 7]
    arena = torch.zeros(sum(vocab) + 8, K, device="cuda")                      # 8 guard rows behind the last table
    tabs, o = [], 0
    for v in vocab:
        tabs.append(arena[o:o + v])
        o += v
    init = torch.randn(sum(vocab), K, device="cuda")
    arena[:sum(vocab)] = init
    opt = ops.SparseAdagrad(tabs, lr=0.05, method=method)
    acc0 = [a.clone() for a in opt.accums]
    ids = np.stack([rng.integers(-1, v + 6, size=B) for v in vocab], 1).astype(np.int64)     # up to 5 rows past each table
    grad = rng.standard_normal((B, F * K)).astype(np.float32)
    opt.step(torch.from_numpy(ids).cuda(), torch.from_numpy(grad).cuda())
    assert float(arena[sum(vocab):].abs().max()) == 0.0                        # nothing written behind the last table
    o = 0
    for f, v in enumerate(vocab):
        ok = (ids[:, f] >= 0) & (ids[:, f] < v)
        gsum = np.zeros((v, K))
        np.add.at(gsum, ids[ok, f], grad[ok, f * K:(f + 1) * K].astype(np.float64))
        touched = np.zeros(v, bool); touched[ids[ok, f]] = True
        a = np.full((v, K), 0.1); a[touched] += gsum[touched] ** 2
        w = init[o:o + v].cpu().double().numpy(); w[touched] -= 0.05 * gsum[touched] / np.sqrt(a[touched])
        _close(tabs[f], w, tol=2e-5)
        _close(opt.accums[f], a, tol=2e-5)
        assert torch.equal(opt.accums[f][~torch.from_numpy(touched).cuda()], acc0[f][~torch.from_numpy(touched).cuda()])
        o += v
    # FTRL through the same sorted machinery
    lw = [torch.zeros(v, device="cuda") for v in vocab]
    ftrl = ops.SparseFtrl(lw, lr=0.2)
    ftrl.step(torch.from_numpy(ids).cuda(), torch.from_numpy(grad[:, :1].copy()).cuda())
    for f, v in enumerate(vocab):
        untouched = np.ones(v, bool); untouched[ids[(ids[:, f] >= 0) & (ids[:, f] < v), f]] = False
        assert float(lw[f][torch.from_numpy(untouched).cuda()].abs().sum()) == 0.0


def test_sorted_updates_over_the_slot_major_sort(built_lib):
    """B >= 4096: the sorted updates run the slot-major sort (csrc/radix_sort.hip: local rows, 10 bits per launch; a slot's digit count
    follows its vocabulary).  Tables of 3, 1030, 70 000 and 2^20 + 5 rows in one update (1, 2, 2 and 3 digits), pruned ids (-1) and ids past
    the vocabulary (skipped like pruned ones: nothing outside a table is written), heavy duplicates in the small tables: Adagrad against
    the float64 dedup-sum rule over two steps, bitwise equal to a second run, and FTRL through the same sort."""
    from dir_amd import ops
    rng = np.random.default_rng(77)
    B, K = 9000, 16
    vocab = [3, 1030, 70000, (1 << 20) + 5]
    F = len(vocab)
    assert built_lib.dir_debug_slot_sort_workspace_bytes(B, F, sum(vocab)) > 0
    tabs = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in vocab]
    runs = []
    for rep in range(2):
        rng2 = np.random.default_rng(5)
        dev = [torch.from_numpy(t.copy()).cuda() for t in tabs]
        opt = ops.SparseAdagrad(dev, lr=0.05, initial_accumulator_value=0.1, method="sorted")
        ref_w = [t.astype(np.float64) for t in tabs]
        ref_a = [np.full((v, K), 0.1) for v in vocab]
        for step in range(2):
            ids = np.stack([rng2.integers(-1, v + 3, size=B) for v in vocab], 1).astype(np.int64)
            grad = (rng2.standard_normal((B, F * K)) * 0.5).astype(np.float32)
            opt.step(torch.from_numpy(ids).cuda(), torch.from_numpy(grad).cuda())
            if rep:
                continue
            for f, v in enumerate(vocab):
                ok = (ids[:, f] >= 0) & (ids[:, f] < v)
                rows, inv = np.unique(ids[ok, f], return_inverse=True)
                gsum = np.zeros((len(rows), K))
                np.add.at(gsum, inv, grad[ok, f * K:(f + 1) * K].astype(np.float64))
                ref_a[f][rows] += gsum ** 2
                ref_w[f][rows] -= 0.05 * gsum / np.sqrt(ref_a[f][rows])
        if not rep:
            for f in range(F):
                _close(dev[f], ref_w[f], tol=2e-5)
                _close(opt.accums[f], ref_a[f], tol=2e-5)
        runs.append([d.clone() for d in dev] + [a.clone() for a in opt.accums])
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    lw = [torch.zeros(v, device="cuda") for v in vocab]
    ftrl = ops.SparseFtrl(lw, lr=0.2)
    ids = np.stack([rng.integers(-1, v + 3, size=B) for v in vocab], 1).astype(np.int64)
    ftrl.step(torch.from_numpy(ids).cuda(), torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).cuda())
    for f, v in enumerate(vocab):
        untouched = np.ones(v, bool)
        untouched[ids[(ids[:, f] >= 0) & (ids[:, f] < v), f]] = False
        assert float(lw[f][torch.from_numpy(untouched).cuda()].abs().sum()) == 0.0
        assert float(lw[f][torch.from_numpy(~untouched).cuda()].abs().sum()) > 0.0 or v == 0


def test_sorted_adagrad_bitwise_reproducible_on_skewed_ids(built_lib):
    from dir_amd import ops
    g = torch.Generator().manual_seed(9)
    B, F, K, V = 8192, 4, 16, 5000
    ids = (torch.rand(B, F, generator=g) ** 6 * V).long().clamp(max=V - 1).cuda()      # heavy head: hot rows repeat thousands of times
    grad = torch.randn(B, F * K, generator=g).cuda()
    outs = []
    for _ in range(2):
        tabs = [torch.zeros(V, K, device="cuda") for _ in range(F)]
        opt = ops.SparseAdagrad(tabs, lr=0.1)
        opt.step(ids, grad)
        outs.append(torch.stack(tabs).clone())
    assert torch.equal(outs[0], outs[1])


def test_deepfm_fused_adagrad_matches_torch_adagrad(built_lib):
    """The fused path (row gradients consumed inside backward) must equal torch.optim.Adagrad on the sparse grads."""
    from dir_amd.deepfm import DeepFM
    from dir_amd import feature_column as fc
    B, F, K, V = 256, 4, 8, 12        # tiny vocabulary: many duplicate ids per batch
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]

    def make():
        torch.manual_seed(5)
        return DeepFM(linear_feature_columns=[], dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                      dnn_hidden_units=[16], fm_embedding_size=K).cuda()
    a, b = make(), make()
    fused = a.fused_sparse_adagrad(lr=0.1)
    opt_b = torch.optim.Adagrad(list(b.embedding_weights), lr=0.1, initial_accumulator_value=0.1, eps=0.0)
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        ids = torch.randint(0, V, (B, F), generator=g)
        labels = torch.randint(0, 2, (B, 1), generator=g).float().cuda()
        feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
        for m in (a, b):
            m.zero_grad(set_to_none=True)
            torch.nn.functional.binary_cross_entropy_with_logits(m(feats), labels, reduction="sum").backward()
        assert a.embedding_weights[0].grad is None          # consumed by the fused kernel
        opt_b.step()
    for pa, pb in zip(a.embedding_weights, b.embedding_weights):
        _close(pa, pb, tol=2e-5)
    assert fused.accums[0].min().item() >= 0.1


# ---- CIN backward (no reference code; derivatives of the definition in include/dir_hip.h A14) -----------------------
@pytest.mark.parametrize("B,m,D,Hp,H", [(64, 26, 16, 26, 128), (33, 26, 16, 128, 128), (7, 5, 4, 6, 7), (9, 8, 8, 5, 32),
                                         (5, 3, 4, 2, 3), (3, 8, 16, 9, 200), (21, 39, 16, 39, 96), (1, 4, 4, 3, 5),
                                         (18, 13, 32, 50, 130), (250, 10, 4, 45, 64),
                                         # 128 < H, Hp <= 256: two slices of H per field, two column blocks adding their dx0 shares
                                         (19, 26, 16, 200, 200), (11, 8, 8, 130, 256), (9, 26, 4, 256, 129), (7, 5, 16, 129, 40),
                                         (6, 4, 16, 20, 257),
                                         # tile counts that follow the widths (cin_bwd.hip): 3-tile column blocks (Hp 65..96, 193..224), slices
                                         # of 96 rows (H 65..96) and 128 + 32/64/96/128, h blocks of 1 / 2 / 3 tiles in dW
                                         (10, 26, 16, 70, 96), (10, 26, 16, 96, 70), (8, 8, 8, 200, 150), (8, 8, 8, 224, 190), (8, 8, 8, 100, 224),
                                         (7, 26, 16, 160, 160), (7, 16, 4, 192, 225), (9, 12, 16, 40, 64), (9, 12, 16, 33, 33),
                                         # one and two fields (a staged chunk of the bf16x3 data-gradient form holds two), row counts off the 256 grid
                                         (40, 1, 16, 70, 33), (17, 2, 8, 64, 64), (300, 7, 16, 128, 65), (33, 3, 32, 65, 128)])
def test_cin_dw_and_data_grads_vs_oracle(built_lib, B, m, D, Hp, H):
    from dir_amd import ops
    from oracle import oracle as O
    rng = np.random.default_rng(B * 7 + Hp)
    x0 = (rng.standard_normal((B, m, D)) * 0.5).astype(np.float32)
    xk = (rng.standard_normal((B, Hp, D)) * 0.5).astype(np.float32)
    W = (rng.standard_normal((H, Hp * m)) / np.sqrt(Hp * m)).astype(np.float32)
    G = (rng.standard_normal((B, H, D)) * 0.5).astype(np.float32)
    ref_dW, ref_dxk, ref_dx0 = O.cin_backward(x0, xk, W, G)
    dev = lambda a: torch.from_numpy(a).cuda()
    dx0, dxk, dW = ops.cin_layer_backward(dev(x0), dev(xk), dev(W), dev(G), arith="f32")      # dir_cin_dx_f32 / forward form, dir_cin_dw_f32
    _close(dxk, ref_dxk)
    _close(dx0, ref_dx0)
    if ops.cin_bf16x3_covers(m, D):     # both data gradients in one pass of the split-arithmetic kernel (dir_cin_layer_dot_add_*_f32), bitwise reproducible
        for split in ("bf16x3", "f16x2"):
            sxk, sx0 = ops.cin_dx_bf16x3(dev(x0), dev(xk), dev(W), dev(G), split=split)
            _close(sxk, ref_dxk)
            _close(sx0, ref_dx0)
            cxk, cx0 = ops.cin_dx_bf16x3(dev(x0), dev(xk), dev(W), dev(G), split=split)
            assert torch.equal(cxk, sxk) and torch.equal(cx0, sx0)
        # fp16 x 2 scales every row of G by a power of two inside the kernel: a gradient 2^-30 times smaller, or whose samples differ by
        # powers of two over 40 binades, gives the same bits times those powers (nothing underflows into fp16's subnormals)
        pw = torch.from_numpy(np.ldexp(1.0, rng.integers(-30, 10, size=(B, 1, 1))).astype(np.float32)).cuda()
        pxk, px0 = ops.cin_dx_bf16x3(dev(x0), dev(xk), dev(W), dev(G) * pw, split="f16x2")
        assert torch.equal(pxk, sxk * pw) and torch.equal(px0, sx0 * pw)
        gb = []                                                                  # the tensor maximum of G rides along (cin_dw's scale)
        ops.cin_dx_bf16x3(dev(x0), dev(xk), dev(W), dev(G), split="f16x2", g_bits_out=gb)
        assert int(gb[0]) == int(np.abs(G).max().view(np.int32))
        bxk, bx0 = ops.cin_dx_bf16x3(dev(x0), dev(xk), dev(W), dev(G))          # split=None: ops.CIN_BWD_SPLIT
        if ops.CIN_BWD_SPLIT == "f16x2":
            assert torch.equal(bxk, sxk) and torch.equal(bx0, sx0)
        ax0, axk, _ = ops.cin_layer_backward(dev(x0), dev(xk), dev(W), dev(G), need_w=False)  # "auto": one of the two, bitwise
        want = (bx0, bxk) if ops.cin_auto_arith(m, D, H, Hp) == "bf16x3" else (dx0, dxk)
        assert torch.equal(ax0, want[0]) and torch.equal(axk, want[1])
    # the other formulation of the data gradients (forward kernel on permuted weights; the only one for H or Hp > 128)
    fx0, fxk, _ = ops.cin_layer_backward(dev(x0), dev(xk), dev(W), dev(G), need_w=False, force_forward_form=True)
    _close(fxk, ref_dxk)
    _close(fx0, ref_dx0)
    # dW sums B*D fp32 terms: scale the tolerance by the magnitude that was summed
    mag = np.sqrt(B * D) * 0.125 + 1.0
    err = np.abs(dW.cpu().double().numpy() - ref_dW) / (mag + np.abs(ref_dW))
    assert err.max() <= 1e-5, "dW max scaled err %.3e" % err.max()
    if D >= 8:                          # the bf16x3 weight-gradient kernel (dir_cin_dw_bf16x3_f32): same bar, bitwise reproducible, accumulate form
        bW = ops.cin_dw(dev(x0), dev(xk), dev(G), arith="bf16x3")
        err = np.abs(bW.cpu().double().numpy() - ref_dW) / (mag + np.abs(ref_dW))
        assert err.max() <= 1e-5, "bf16x3 dW max scaled err %.3e" % err.max()
        assert torch.equal(ops.cin_dw(dev(x0), dev(xk), dev(G), arith="bf16x3"), bW)
        acc2 = ops.cin_dw(dev(x0), dev(xk), dev(G), dW=bW.clone(), accumulate=True, arith="bf16x3")
        assert torch.allclose(acc2, 2 * bW, rtol=1e-6, atol=1e-6)
        # fp16 x 2 (dir_cin_dw_f16x2_f32): G scaled by one power of two for the tensor; same bar; a 2^-30 times smaller G gives the same bits
        hW = ops.cin_dw(dev(x0), dev(xk), dev(G), arith="f16x2")
        err = np.abs(hW.cpu().double().numpy() - ref_dW) / (mag + np.abs(ref_dW))
        assert err.max() <= 1e-5, "f16x2 dW max scaled err %.3e" % err.max()
        assert torch.equal(ops.cin_dw(dev(x0), dev(xk), dev(G), arith="f16x2"), hW)
        assert torch.equal(ops.cin_dw(dev(x0), dev(xk), dev(G) * 2.0 ** -30, arith="f16x2"), hW * 2.0 ** -30)
        bound = torch.tensor([np.float32(np.abs(G).max() * 1.5).view(np.int32)], dtype=torch.int32, device="cuda")      # an upper bound's bits
        gW = ops.cin_dw(dev(x0), dev(xk), dev(G), arith="f16x2", g_absmax_bits=bound)
        err = np.abs(gW.cpu().double().numpy() - ref_dW) / (mag + np.abs(ref_dW))
        assert err.max() <= 1e-5, "f16x2 dW (given bound) max scaled err %.3e" % err.max()
        if ops.CIN_BWD_SPLIT == "f16x2" and ops.cin_dw_auto_arith(m, D, Hp, H) == "bf16x3":
            bW = hW                                                  # what "auto" runs now
    # accumulate form and bitwise reproducibility
    again = ops.cin_dw(dev(x0), dev(xk), dev(G), arith="f32")
    assert torch.equal(again, dW)
    acc = dW.clone()
    ops.cin_dw(dev(x0), dev(xk), dev(G), dW=acc, accumulate=True, arith="f32")
    auto = ops.cin_dw(dev(x0), dev(xk), dev(G))                      # "auto" is one of the two kernels, bitwise
    assert torch.equal(auto, bW if (D >= 8 and ops.cin_dw_auto_arith(m, D, Hp, H) == "bf16x3") else dW)
    _close(acc, 2 * ref_dW, tol=1e-5 * mag)


def test_cin_dw_large_rows(built_lib):
    """Many row groups per split (the pipelined main loop), a row count with R % 8 == 4, all-ones check of the sums."""
    from dir_amd import ops
    B, m, D, Hp, H = 4097, 6, 4, 5, 40
    x0 = torch.full((B, m, D), 0.5, device="cuda")
    xk = torch.full((B, Hp, D), 2.0, device="cuda")
    G = torch.ones((B, H, D), device="cuda")
    dW = ops.cin_dw(x0, xk, G)
    assert torch.equal(dW, torch.full_like(dW, float(B * D)))      # 1 * 2 * 0.5 summed over B*D rows, exact in fp32


def test_cin_autograd_matches_float64(built_lib):
    from dir_amd import autograd as ag
    g = torch.Generator().manual_seed(5)
    B, m, D, Hs = 37, 7, 8, (12, 9)
    x0 = (torch.randn(B, m, D, generator=g) * 0.5)
    Ws = [torch.randn(Hs[0], m * m, generator=g) / m, torch.randn(Hs[1], Hs[0] * m, generator=g) / (Hs[0] * m) ** 0.5]
    head = torch.randn(sum(Hs), generator=g)

    def model64():
        x = x0.double().requires_grad_(True)
        ws = [w.double().requires_grad_(True) for w in Ws]
        xk, outs = x, []
        for w in ws:
            H = w.shape[0]
            xk = torch.einsum("hij,bid,bjd->bhd", w.view(H, xk.shape[1], m), xk, x)
            outs.append(xk.sum(2))
        loss = (torch.cat(outs, 1) @ head.double()).square().sum()
        loss.backward()
        return loss, x.grad, [w.grad for w in ws]

    l64, gx64, gw64 = model64()
    x = x0.cuda().requires_grad_(True)
    ws = [w.cuda().requires_grad_(True) for w in Ws]
    xk, outs = x, []
    for w in ws:
        xk, p = ag.cin_layer(x, xk, w)
        outs.append(p)
    loss = (torch.cat(outs, 1) @ head.cuda()).square().sum()
    loss.backward()
    _close(loss, l64, tol=1e-5)
    scale = float(gx64.abs().max())
    _close(x.grad / scale, gx64 / scale, tol=2e-5)
    for w, g64 in zip(ws, gw64):
        s = float(g64.abs().max())
        _close(w.grad / s, g64 / s, tol=2e-5)


def test_xdeepfm_training_step(built_lib):
    """A few SGD steps of a small xDeepFM through the HIP backward path reduce a logistic loss."""
    from dir_amd import feature_column as fc
    from dir_amd.xdeepfm import XDeepFM
    torch.manual_seed(0)
    F, V, D, B = 6, 50, 8, 256
    cats = [fc.categorical_column_with_identity("c%d" % i, V) for i in range(F)]
    model = XDeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, D) for c in cats],
                    cin_layer_sizes=(16, 16), dnn_hidden_units=(32,)).cuda()
    g = torch.Generator().manual_seed(1)
    feats = {"c%d" % i: torch.randint(0, V, (B,), generator=g).cuda() for i in range(F)}
    y = ((feats["c0"] + feats["c1"]) % 2).float().reshape(B, 1)
    dense = [p for n, p in model.named_parameters() if not (n.startswith("embedding_weights") or n.startswith("linear_weights"))]
    sparse = [p for n, p in model.named_parameters() if n.startswith("embedding_weights") or n.startswith("linear_weights")]
    opt = torch.optim.Adagrad(dense, lr=0.05)
    opt_s = torch.optim.SGD(sparse, lr=0.5)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        opt_s.zero_grad(set_to_none=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model(feats), y)
        loss.backward()
        assert all(w.grad is not None for w in model.cin_W)
        opt.step()
        opt_s.step()
        losses.append(loss.item())
    assert losses[-1] < 0.8 * losses[0], losses[::6]


def test_xdeepfm_training_with_fused_sparse_optimisers(built_lib):
    """XDeepFM.fused_sparse_adagrad / fused_sparse_ftrl (the DeepFM recipe on the CIN model): the tables and the linear columns are
    updated inside backward() from ONE id matrix and one sort; the embedding tables end up bit-identical to the same model trained
    with separately sorted updates, and the loss goes down."""
    from dir_amd import feature_column as fc
    from dir_amd.xdeepfm import XDeepFM
    F, V, D, B = 6, 50, 8, 512
    def build(link):
        torch.manual_seed(4)
        cats = [fc.categorical_column_with_identity("c%d" % i, V) for i in range(F)]
        m = XDeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, D) for c in cats],
                    cin_layer_sizes=(16, 16), dnn_hidden_units=(32,)).cuda()
        a, f = m.fused_sparse_adagrad(lr=0.1), m.fused_sparse_ftrl(lr=0.2)
        if not link:
            a._share = f._share = None
        sparse = {id(p) for p in m.embedding_weights} | {id(p) for p in m.linear_weights}
        return m, a, torch.optim.Adagrad([p for p in m.parameters() if id(p) not in sparse], lr=0.05)
    (ma, aa, oa), (mb, ab, ob) = build(True), build(False)
    assert aa._share is not None
    g = torch.Generator().manual_seed(1)
    feats = {"c%d" % i: torch.randint(0, V, (B,), generator=g).cuda() for i in range(F)}
    y = ((feats["c0"] + feats["c1"]) % 2).float().reshape(B, 1)
    losses = []
    for _ in range(30):
        for m, o in ((ma, oa), (mb, ob)):
            o.zero_grad(set_to_none=True)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(m(feats), y)
            loss.backward()
            o.step()
        losses.append(loss.item())
    assert aa._share.hits == 30
    assert all(p.grad is None for p in ma.embedding_weights)                # updated in place by the fused optimiser
    for pa, pb in zip(list(ma.embedding_weights) + list(ma.linear_weights), list(mb.embedding_weights) + list(mb.linear_weights)):
        assert torch.equal(pa.data, pb.data)
    assert losses[-1] < 0.8 * losses[0], losses[::6]


# ---- DIN backward (no reference code; derivatives of the unit defined in include/dir_hip.h A13) ---------------------
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B,T,K,H1,H2,V", [(33, 50, 64, 80, 40, 500), (17, 7, 16, 12, 8, 40), (9, 20, 32, 36, 20, 64),
                                           # the fused backward's shape class: > one sample per workgroup, full-length T = 64 with
                                           # narrower layers, a single position, H2 at its 48 limit
                                           (600, 50, 64, 80, 40, 3000), (70, 64, 64, 72, 36, 200), (5, 1, 64, 8, 4, 30),
                                           (21, 30, 64, 80, 48, 100)])
def test_din_autograd_matches_float64(built_lib, normalize, B, T, K, H1, H2, V):
    from dir_amd import autograd as ag
    g = torch.Generator().manual_seed(B + T)
    table = torch.randn(V, K, generator=g) * 0.3
    hist = torch.randint(0, V, (B, T), generator=g)
    hist[1, min(2, T - 1)] = -1                                # a pruned id inside the valid range
    hl = torch.randint(0, T + 1, (B,), generator=g).int()
    hl[0] = 0                                                 # an empty history
    cand = torch.randint(0, V, (B,), generator=g)
    Ws = [torch.randn(4 * K, H1, generator=g) * 0.2, torch.randn(H1, generator=g) * 0.1, torch.randn(H1, H2, generator=g) * 0.3,
          torch.randn(H2, generator=g) * 0.1, torch.randn(H2, generator=g) * 0.4, torch.randn(1, generator=g) * 0.1]
    gout = torch.randn(B, K, generator=g)

    # float64 dense restatement of the definition
    t64 = table.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in Ws]
    h = t64[hist.clamp(min=0)]                                 # [B,T,K]
    a = t64[cand].unsqueeze(1).expand(B, T, K)
    u = torch.cat([h, a, h - a, h * a], dim=2)
    s = torch.sigmoid(torch.sigmoid(u @ w64[0] + w64[1]) @ w64[2] + w64[3]) @ w64[4] + w64[5]
    valid = (torch.arange(T).unsqueeze(0) < hl.unsqueeze(1)) & (hist >= 0)
    if normalize:
        x = (s / K ** 0.5).masked_fill(~valid, float("-inf"))
        w = torch.softmax(x, dim=1)
        w = torch.where(valid, w, torch.zeros_like(w))
    else:
        w = torch.where(valid, s, torch.zeros_like(s))
    out64 = (w.unsqueeze(2) * h).sum(1)
    out64.backward(gout.double())

    tab = table.cuda().requires_grad_(True)
    ws = [w.cuda().requires_grad_(True) for w in Ws]
    out = ag.din_attention_pool(tab, hist.cuda(), hl.cuda(), cand.cuda(), *ws, normalize=normalize)
    _close(out, out64, tol=2e-5)
    out.backward(gout.cuda())
    assert tab.grad.is_sparse
    _close(tab.grad.to_dense(), t64.grad, tol=2e-5)
    for w, r in zip(ws, w64):
        _close(w.grad, r.grad, tol=5e-5)


def test_din_module_training_step(built_lib):
    from dir_amd.din import DINAttentionPool
    torch.manual_seed(3)
    V, K, B, T = 200, 16, 128, 12
    pool = DINAttentionPool(V, embedding_dim=K, hidden_units=(16, 8), normalize=True).cuda()
    head = torch.nn.Linear(K, 1).cuda()
    g = torch.Generator().manual_seed(4)
    hist = torch.randint(0, V, (B, T), generator=g).cuda()
    hl = torch.randint(1, T + 1, (B,), generator=g).int().cuda()
    cand = torch.randint(0, V, (B,), generator=g).cuda()
    y = (cand % 2).float().reshape(B, 1)
    dense = [p for n, p in pool.named_parameters() if n != "table"] + list(head.parameters())
    opt = torch.optim.Adagrad(dense, lr=0.1)
    opt_t = torch.optim.SGD([pool.table], lr=1.0)
    losses = []
    for _ in range(40):
        opt.zero_grad(set_to_none=True)
        opt_t.zero_grad(set_to_none=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(head(pool(hist, hl, cand)), y)
        loss.backward()
        assert pool.table.grad.is_sparse
        opt.step()
        opt_t.step()
        losses.append(loss.item())
    assert losses[-1] < 0.85 * losses[0], losses[::8]


def test_dcn_reference_train_step(built_lib):
    """DeepCrossNetwork.train_step(): the reference train_op (Adam eps 1e-4, cosine decay, per-tensor clip_by_norm 100,
    DeepCrossNetwork.py:264-290 with the spec of DeepCrossNetwork/train.py:111-125) over the HIP forward/backward."""
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd import feature_column as fc
    torch.manual_seed(1)
    B, F, K, V = 512, 5, 8, 30
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
    ids = torch.randint(0, V, (B, F))
    labels = (ids[:, 0] < V // 2).float().reshape(B, 1).cuda()
    feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
    feats["x"] = torch.rand(B).cuda()
    dcn = DeepCrossNetwork(columns=[fc.embedding_column(c, K) for c in cats] + [fc.numeric_column("x")], cross_layer_num=2,
                           dnn_hidden_units=[32, 16], batch_norm=False, l2_reg=1e-4, optimizer="Adam",
                           optimizer_spec={"epsilon": 1e-4, "learning_rate": 123.0},     # the spec's own lr is dropped (:275-279)
                           learning_rate_spec={"learning_rate": 0.02, "decay_method": "cosine_decay", "decay_steps": 40,
                                               "alpha": 0.5}).cuda()
    step = dcn.train_step()
    assert step.optimizer.defaults["eps"] == 1e-4
    losses, lrs = [], []
    for _ in range(50):
        loss, lr = step(torch.nn.functional.binary_cross_entropy_with_logits(dcn(feats), labels))
        losses.append(loss.item())
        lrs.append(lr)
    assert lrs[0] == pytest.approx(0.02) and lrs[40] == pytest.approx(0.01) and lrs[-1] == pytest.approx(0.01)
    assert step.global_step == 50
    assert losses[-1] < 0.8 * losses[0], losses[::10]


@pytest.mark.parametrize("B,F,K,V,shared", [(300, 5, 1, 20, True), (4096, 26, 1, 1000, True), (777, 3, 4, 50, False), (2000, 2, 1, 3, True),
                                            (513, 4, 8, 7, False)])
def test_fused_sparse_ftrl(built_lib, B, F, K, V, shared):
    """dir_sparse_ftrl_sorted_f32 vs a float64 FTRL-Proximal ([TF-upstream] tf.train.FtrlOptimizer: duplicates summed first),
    l1 and l2 active, two steps; `shared`: one [B, K] gradient row for every slot (the linear term)."""
    from dir_amd import ops
    rng = np.random.default_rng(B + K + F)
    shape = (V,) if K == 1 else (V, K)
    tabs = [(rng.standard_normal(shape) * 0.1).astype(np.float32) for _ in range(F)]
    dev = [torch.from_numpy(t.copy()).cuda() for t in tabs]
    lr, l1, l2 = 0.2, 0.01, 0.05
    opt = ops.SparseFtrl(dev, lr=lr, initial_accumulator_value=0.1, l1=l1, l2=l2)
    w = [t.astype(np.float64).reshape(V, K) for t in tabs]
    n = [np.full((V, K), 0.1) for _ in range(F)]
    z = [np.zeros((V, K)) for _ in range(F)]
    for step in range(2):
        ids = rng.integers(-1, V, size=(B, F)).astype(np.int64)
        grad = (rng.standard_normal((B, K if shared else F * K)) * 0.5).astype(np.float32)
        opt.step(torch.from_numpy(ids).cuda(), torch.from_numpy(grad).cuda())
        for f in range(F):
            gsum = np.zeros((V, K))
            ok = ids[:, f] >= 0
            gf = grad if shared else grad[:, f * K:(f + 1) * K]
            np.add.at(gsum, ids[ok, f], gf[ok].astype(np.float64))
            t = np.zeros(V, bool); t[ids[ok, f]] = True
            n_new = n[f][t] + gsum[t] ** 2
            sigma = (np.sqrt(n_new) - np.sqrt(n[f][t])) / lr
            z_new = z[f][t] + gsum[t] - sigma * w[f][t]
            quad = np.sqrt(n_new) / lr + 2 * l2
            w[f][t] = np.where(np.abs(z_new) > l1, (np.sign(z_new) * l1 - z_new) / quad, 0.0)
            n[f][t], z[f][t] = n_new, z_new
    for f in range(F):
        _close(dev[f].reshape(V, K), w[f], tol=2e-5)
        _close(opt.accums[f].reshape(V, K), n[f], tol=2e-5)
        _close(opt.linears[f].reshape(V, K), z[f], tol=5e-5)


@pytest.mark.parametrize("B,F,V,per_slot", [(300, 5, 20, False), (4096, 26, 1000, False), (2000, 2, 3, False), (65536, 3, 50000, False),
                                            (777, 4, 33, True)])
def test_fused_sparse_ftrl_packed_rows_bit_exact(built_lib, B, F, V, per_slot):
    """The packed linear training rows (TableSet.ftrl_rows: [w | n | z | -], dir_sparse_ftrl_rows_sorted_f32 and the forward
    dir_linear_onehot_rows_f32) against the three-array form on the same ids and gradients (pruned ids, duplicates, l1 / l2 active):
    w, n, z and the forward's logits bit for bit over three steps."""
    from dir_amd import ops
    g = torch.Generator().manual_seed(B + F)
    w0 = [(torch.randn(V, generator=g) * 0.1).cuda() for _ in range(F)]
    plain = [w.clone() for w in w0]
    opt_a = ops.SparseFtrl(plain, lr=0.2, initial_accumulator_value=0.1, l1=0.01, l2=0.05)
    rows = ops.TableSet.ftrl_rows([w.clone() for w in w0], 0.1)
    assert rows.ld == 4 and all(r.data_ptr() % 16 == 0 for r in rows.rows)
    opt_b = ops.SparseFtrl(rows, lr=0.2, initial_accumulator_value=0.1, l1=0.01, l2=0.05)
    assert opt_b.packed and not opt_a.packed
    bias = torch.tensor([0.25], device="cuda")
    for step in range(3):
        ids = torch.randint(-1, V, (B, F), generator=g).cuda()
        if step == 1:
            ids = ids.t().contiguous().t()            # field-major strides
        grad = (torch.randn(B, F if per_slot else 1, generator=g) * 0.5).cuda()
        la = ops.linear_logit(plain, ids, bias=bias)
        lb = ops.linear_logit(rows, ids, bias=bias)
        assert torch.equal(la, lb)
        acc = torch.randn(B, 1, generator=g).cuda()
        a2, b2 = acc.clone(), acc.clone()
        ops.linear_logit(plain, ids, out=a2, accumulate=True)
        ops.linear_logit(rows, ids, out=b2, accumulate=True)
        assert torch.equal(a2, b2)
        opt_a.step(ids, grad)
        opt_b.step(ids, grad)
        for f in range(F):
            assert torch.equal(rows.tables[f].reshape(-1), plain[f]), (step, f)
            assert torch.equal(rows.accums[f].reshape(-1), opt_a.accums[f].reshape(-1)), (step, f)
            assert torch.equal(rows.linears[f].reshape(-1), opt_a.linears[f].reshape(-1)), (step, f)
            assert float(rows.rows[f][:, 3].abs().max()) == 0.0          # the row's fourth float is never written
    with pytest.raises(ValueError, match="one-hot"):
        ops.linear_logit(rows, torch.zeros(4, dtype=torch.int64, device="cuda"), offsets=torch.arange(0, F + 1, device="cuda"))


def test_deepfm_packed_ftrl_rows_train_like_the_plain_columns(built_lib):
    """DeepFM.fused_sparse_ftrl(packed=True) beside fused_sparse_adagrad(packed=True) (one shared sort per step): logits, linear weights
    and embedding tables bit-identical to the unpacked fused optimisers after three steps; the parameters stay [vocab, 1] views of the
    rows and inference afterwards (the packed SERVING rows are rebuilt from them) agrees too."""
    from dir_amd.deepfm import DeepFM
    from dir_amd import feature_column as fc
    B, F, K, V = 512, 5, 16, 40
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]

    def make(packed):
        torch.manual_seed(3)
        m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                   dnn_hidden_units=[32, 16], fm_embedding_size=K).cuda()
        with torch.no_grad():
            for p in m.linear_weights:
                p.normal_(0, 0.05)
        m.fused_sparse_adagrad(lr=0.05, packed=packed)
        f = m.fused_sparse_ftrl(lr=0.2, l1=0.001, packed=packed)
        assert f.packed == packed
        return m
    a, b = make(False), make(True)
    assert all(p.data.stride(0) == 4 and p.data.shape == q.data.shape for p, q in zip(b.linear_weights, a.linear_weights))
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        ids = torch.randint(0, V, (B, F), generator=g)
        labels = torch.randint(0, 2, (B, 1), generator=g).float().cuda()
        feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
        outs = []
        for m in (a, b):
            m.train()
            m.zero_grad(set_to_none=True)
            out = m(feats)
            torch.nn.functional.binary_cross_entropy_with_logits(out, labels, reduction="sum").backward()
            outs.append(out.detach())
        assert torch.equal(outs[0], outs[1])
        assert b.linear_weights[0].grad is None and b.linear_bias.grad is not None
        with torch.no_grad():                       # (the dense parameters: plain SGD, the same on both)
            for m in (a, b):
                for p in m.parameters():
                    if p.grad is not None:
                        p -= 0.01 * p.grad
    for pa, pb in zip(a.linear_weights, b.linear_weights):
        assert torch.equal(pa.data, pb.data)
    for pa, pb in zip(a.embedding_weights, b.embedding_weights):
        assert torch.equal(pa.data, pb.data)
    a.eval(); b.eval()
    with torch.no_grad():
        assert torch.equal(a(feats), b(feats))
    sa, sd = a.state_dict(), b.state_dict()
    assert all(sd[k].shape == sa[k].shape for k in sd if "linear_weights" in k)


@pytest.mark.parametrize("B,F,K,V", [(1000, 26, 16, 500), (65, 3, 8, 20), (4097, 5, 4, 9), (16, 2, 32, 7), (300, 39, 16, 100)])
def test_gather_fm_rows_leaves_row_maxima(built_lib, B, F, K, V):
    """dir_gather_fm_rows_bits_f32: emb, fm and the field sums bit-identical to dir_gather_fm_rows_f32, and the row / tensor maxima it leaves
    on emb equal to dir_row_absmax_bits_f32's pass over emb (pruned ids, ragged tails; packed training rows and plain tables + fsum)."""
    from dir_amd import ops
    g = torch.Generator().manual_seed(B + K)
    tabs = [(torch.randn(V, K, generator=g) * (0.01 + f)).cuda() for f in range(F)]
    ids = torch.randint(-1, V + 1, (B, F), generator=g).cuda()
    for ts in (ops.TableSet.train_rows([t.clone() for t in tabs]), ops.TableSet(tabs)):
        f0 = torch.empty(B, K, device="cuda"); f1 = torch.empty(B, K, device="cuda")
        e0, m0 = ops.gather_fm(ts, ids, fsum=f0)
        e1, m1 = ops.gather_fm(ts, ids, fsum=f1, want_bits=True)
        assert torch.equal(e0, e1) and torch.equal(m0, m1) and torch.equal(f0, f1)
        assert not hasattr(e0, "_dir_bits")
        rb, ab, ver = e1._dir_bits
        want_rb, want_ab = ops.row_absmax_bits(e1.clone())
        assert ver == e1._version and torch.equal(rb, want_rb) and torch.equal(ab, want_ab)
        assert float(ab.view(torch.float32)) == float(e1.abs().max())
        e2, _ = ops.gather_fm(ts, ids, fsum=f1, want_bits=True)       # the ticket word is back at zero: a second call gives the same
        assert torch.equal(e2._dir_bits[1], want_ab) and torch.equal(e2._dir_bits[0], want_rb)


@pytest.mark.parametrize("B,F,K,V", [(1000, 26, 16, 500), (65, 3, 8, 20), (4097, 5, 4, 9), (300, 39, 16, 100)])
def test_onehot_embedding_bag_leaves_row_maxima(built_lib, B, F, K, V):
    """ops.embedding_bag(want_bits=True) on one-hot ids (what an input layer of embedding columns runs under training): the same output,
    bit for bit, as the bag entry (pruned ids, field-major ids), with dir_row_absmax_bits_f32's row / tensor maxima left on it; multi-hot
    or clipped lookups ignore the request."""
    from dir_amd import ops
    g = torch.Generator().manual_seed(B + 3 * K)
    tabs = [(torch.randn(V, K, generator=g) * (0.02 + 0.5 * f)).cuda() for f in range(F)]
    ts = ops.TableSet(tabs)
    for ids in (torch.randint(-1, V + 1, (B, F), generator=g).cuda(), torch.randint(0, V, (F, B), generator=g).cuda().t()):
        e0 = ops.embedding_bag(ts, ids)
        e1 = ops.embedding_bag(ts, ids, want_bits=True)
        assert torch.equal(e0, e1) and not hasattr(e0, "_dir_bits")
        rb, ab, ver = e1._dir_bits
        want_rb, want_ab = ops.row_absmax_bits(e1.clone())
        assert ver == e1._version and torch.equal(rb, want_rb) and torch.equal(ab, want_ab)
    clipped = ops.embedding_bag(ts, ids, max_norm=0.5, want_bits=True)
    assert not hasattr(clipped, "_dir_bits") and torch.equal(clipped, ops.embedding_bag(ts, ids, max_norm=0.5))


def test_deepfm_train_step_takes_the_first_layers_row_maxima_from_the_gather(built_lib, monkeypatch):
    """A DeepFM training step on packed training rows: with the gather's row maxima (default) the first dense layer runs no max pass of its
    own over the embedding output, and logits, losses and updated tables are bit-identical to the step without them."""
    from dir_amd.deepfm import DeepFM
    from dir_amd import feature_column as fc, ops
    B, F, K, V = 16384, 26, 16, 300          # (>= ops.DENSE_BF3_MIN_ROWS: the layers run the row-scaled kernel)
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (B, F), generator=g)
    labels = torch.randint(0, 2, (B, 1), generator=g).float().cuda()
    feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
    res = []
    for bits in (True, False):
        monkeypatch.setattr(ops, "GATHER_BITS", bits)
        torch.manual_seed(4)
        m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                   dnn_hidden_units=[400, 400, 400], fm_embedding_size=K).cuda()
        m.fused_sparse_adagrad(lr=0.05, packed=True)
        m.fused_sparse_ftrl(lr=0.2, packed=True)
        calls = []
        real = ops.row_absmax_bits
        monkeypatch.setattr(ops, "row_absmax_bits", lambda x, want_all=True: (calls.append(tuple(x.shape)), real(x, want_all))[1])
        m.train()
        out = m(feats)
        torch.nn.functional.binary_cross_entropy_with_logits(out, labels, reduction="sum").backward()
        monkeypatch.setattr(ops, "row_absmax_bits", real)
        first = [c for c in calls if c == (B, F * K)]
        assert (len(first) == 0) if bits else (len(first) >= 1), calls
        res.append((out.detach().clone(), [p.data.clone() for p in m.embedding_weights], [p.grad.clone() for p in m.hidden.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
        assert torch.equal(a, b)


def test_deepfm_fused_ftrl_matches_torch_ftrl(built_lib):
    from dir_amd.deepfm import DeepFM
    from dir_amd import feature_column as fc
    from dir_amd.autograd import Ftrl
    B, F, K, V = 256, 4, 8, 12
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]

    def make():
        torch.manual_seed(7)
        m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                   dnn_hidden_units=[16], fm_embedding_size=K).cuda()
        with torch.no_grad():
            for p in m.linear_weights:
                p.normal_(0, 0.05)
        return m
    a, b = make(), make()
    a.fused_sparse_ftrl(lr=0.2)
    opt_b = Ftrl(list(b.linear_weights), lr=0.2)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        ids = torch.randint(0, V, (B, F), generator=g)
        labels = torch.randint(0, 2, (B, 1), generator=g).float().cuda()
        feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
        for m in (a, b):
            m.zero_grad(set_to_none=True)
            torch.nn.functional.binary_cross_entropy_with_logits(m(feats), labels, reduction="sum").backward()
        assert a.linear_weights[0].grad is None and a.linear_bias.grad is not None
        opt_b.step()
    for pa, pb in zip(a.linear_weights, b.linear_weights):
        _close(pa, pb, tol=2e-5)


@pytest.mark.parametrize("combiner", ["mean", "sum", "sqrtn"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("field_major", [False, True])
def test_multihot_bag_backward(built_lib, combiner, weighted, field_major):
    """Sparse table gradients of weighted variable-length bags ([TF-upstream] embedding_lookup_sparse: id < 0 pruned, empty bag
    -> zeros, mean = sum / sum(w), sqrtn = sum / sqrt(sum(w^2))) against float64 autograd of the same expression."""
    from dir_amd import autograd as ag, ops
    g = torch.Generator().manual_seed(11)
    B, F, K, V = 37, 3, 8, 20
    lens = torch.randint(0, 5, (B * F,), generator=g)
    lens[3] = 0
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    nnz = int(offs[-1])
    ids = torch.randint(-1, V, (nnz,), generator=g)
    wts = (torch.rand(nnz, generator=g) + 0.25) if weighted else None
    tabs = [torch.randn(V, K, generator=g) * 0.3 for _ in range(F)]
    gout = torch.randn(B, F * K, generator=g)

    t64 = [t.double().requires_grad_(True) for t in tabs]
    out64 = torch.zeros(B, F * K, dtype=torch.float64)
    rows = []
    for bag in range(B * F):
        b, f = (bag % B, bag // B) if field_major else (bag // F, bag % F)
        s, e = int(offs[bag]), int(offs[bag + 1])
        acc = torch.zeros(K, dtype=torch.float64)
        sw = 0.0
        sw2 = 0.0
        for i in range(s, e):
            if ids[i] < 0:
                continue
            w = float(wts[i]) if weighted else 1.0
            acc = acc + w * t64[f][ids[i]]
            sw += w
            sw2 += w * w
        if combiner == "mean" and sw > 0:
            acc = acc / sw
        if combiner == "sqrtn" and sw2 > 0:
            acc = acc / sw2 ** 0.5
        rows.append((b, f, acc))
    out64 = torch.stack([torch.cat([r[2] for r in sorted(rows, key=lambda x: (x[0], x[1])) if r[0] == b]) for b in range(B)])
    out64.backward(gout.double())

    dev = [t.cuda().requires_grad_(True) for t in tabs]
    ts = ops.TableSet([t.data for t in dev])
    out = ag.embedding_bag(ts, ids.cuda(), dev, offs.cuda(), wts.cuda() if weighted else None, combiner=combiner, field_major=field_major)
    _close(out, out64, tol=2e-6)
    out.backward(gout.cuda())
    for t, r in zip(dev, t64):
        assert t.grad.is_sparse
        _close(t.grad.to_dense(), r.grad if r.grad is not None else torch.zeros_like(r), tol=1e-5)


def test_esmm_and_dcn_training_with_reference_losses(built_lib):
    """ESMM.get_loss (ESMM.py:150-175, with a click weight column) and DeepCrossNetwork.create_loss (:209-225) drive a few
    optimiser steps through the HIP forward/backward; dropout and train-mode batch norm are active (TRAIN mode)."""
    from dir_amd.esmm import ESMM
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd import feature_column as fc
    torch.manual_seed(3)
    B, V = 512, 40
    cols = [fc.numeric_column("x"), fc.embedding_column(fc.categorical_column_with_identity("a", V), dimension=8),
            fc.embedding_column(fc.categorical_column_with_identity("b", V), dimension=8)]
    g = torch.Generator().manual_seed(5)
    a, b = torch.randint(0, V, (B,), generator=g), torch.randint(0, V, (B,), generator=g)
    feats = {"x": torch.rand(B, generator=g).cuda(), "a": a.cuda(), "b": b.cuda(), "w": (torch.rand(B, generator=g) + 0.5).cuda()}
    click = (a < V // 2).float().cuda()
    convert = ((a < V // 2) & (b < V // 2)).float().cuda()
    esmm = ESMM(columns=cols, dnn_hidden_units=[32, 16], dnn_dropout=0.1, ctr_weight_column="w").cuda()
    dense = [p for n, p in esmm.named_parameters() if "embedding_weights" not in n]
    sparse = [p for n, p in esmm.named_parameters() if "embedding_weights" in n]
    opt, opt_s = torch.optim.Adam(dense, lr=0.01), torch.optim.SparseAdam(sparse, lr=0.01)
    losses = []
    for _ in range(40):
        opt.zero_grad(); opt_s.zero_grad()
        loss, unw = esmm.get_loss(feats, {"click_label": click, "convert_label": convert}, esmm(feats))
        assert unw.shape == (B, 1)
        loss.backward()
        opt.step(); opt_s.step()
        losses.append(loss.item())
    assert losses[-1] < 0.8 * losses[0], losses[::8]
    dcn = DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[32, 16, 8], dnn_dropout=0.2, batch_norm=True,
                           weight_column="w", optimizer="Adam", optimizer_spec={"epsilon": 1e-4},
                           learning_rate_spec={"learning_rate": 0.01}).cuda()
    step = dcn.train_step()
    first = last = None
    for _ in range(40):
        loss, _ = dcn.create_loss(feats, dcn(feats), click)
        loss, _lr = step(loss)
        first = first if first is not None else float(loss)
        last = float(loss)
    assert last < 0.85 * first
    assert float(dcn.bns[0].moving_mean.abs().sum()) > 0          # the moving statistics moved (TRAIN-mode batch norm)
    dcn.eval()
    with torch.no_grad():
        p = dcn.predict(feats)
    assert set(p) >= {"logits", "logistic", "probabilities", "class_ids"}
    # the reference's evaluation metrics (DeepCrossNetwork.py:293-319) on the fitted batch: the label is a function of field a
    from dir_amd.metrics import BinaryMetrics
    _, unw = dcn.create_loss(feats, p["logits"], click)
    m = BinaryMetrics().update(click, p["logistic"], unw, feats["w"]).result()
    assert m["auc"] > 0.9 and m["accuracy"] > m["accuracy_baseline"] and 0.0 < m["average_loss"] < 0.7, m


def test_train_step_clips_table_gradients_by_their_dense_norm(built_lib):
    """train_spec.TrainStep on an embedding table's sparse gradient (duplicate ids): tf.clip_by_norm over the dense-equivalent gradient
    (DeepCrossNetwork.py:281-286), whose norm is taken from the looked-up rows only -- sum_i <vals_i, S_row(i)> -- not from a pass over
    the table."""
    from dir_amd.train_spec import TrainStep, CLIP_NORM
    V, K, B = 500, 8, 3000
    torch.manual_seed(2)
    emb = torch.nn.Embedding(V, K, sparse=True).cuda()
    ids = torch.randint(0, 40, (B,), device="cuda")                      # heavy duplication
    coef = torch.randn(B, K, device="cuda") * 7.0
    w0 = emb.weight.detach().clone()
    step = TrainStep(emb, optimizer="SGD", learning_rate_spec={"learning_rate": 1.0})
    step((emb(ids) * coef).sum())
    dense = torch.zeros(V, K, device="cuda", dtype=torch.float64).index_add_(0, ids, coef.double())
    norm = float(dense.norm())
    assert norm > CLIP_NORM                                               # the clip is active
    want = w0.double() - dense * (CLIP_NORM / norm)
    assert float((emb.weight.detach().double() - want).abs().max()) <= 1e-5 * (1 + float(want.abs().max()))
    # a small gradient passes unclipped, and the persistent buffer went back to zero
    w1 = emb.weight.detach().clone()
    step((emb(ids[:10]) * 0.01).sum())
    d2 = torch.zeros(V, K, device="cuda").index_add_(0, ids[:10], torch.full((10, K), 0.01, device="cuda"))
    assert torch.allclose(emb.weight.detach(), w1 - d2, atol=1e-6)


def test_esmm_towers_share_ids_and_one_sort(built_lib):
    """ESMM's two towers read the same columns into their own tables: one id matrix per forward (collect_ids memo) and one sort per step
    for their two fused sparse Adagrad updates (ESMM.fused_sparse_adagrad) -- tables and accumulators bit-identical to towers that
    collect and sort for themselves."""
    from dir_amd.esmm import ESMM
    from dir_amd import feature_column as fc
    F, V, K, B = 6, 200, 16, 1024
    def build(shared):
        torch.manual_seed(31)
        cols = [fc.embedding_column(fc.categorical_column_with_identity("C%d" % i, V), K) for i in range(F)]
        m = ESMM(columns=cols, dnn_hidden_units=[32, 16]).cuda()
        if shared:
            opts = m.fused_sparse_adagrad(0.05)
        else:
            opts = m.ctr_model.input_layer.fused_sparse_adagrad(0.05) + m.cvr_model.input_layer.fused_sparse_adagrad(0.05)
        dense = [p for n, p in m.named_parameters() if "embedding_weights" not in n]
        return m, opts, torch.optim.SGD(dense, lr=0.05)
    (a, oa, da), (b, ob, db) = build(True), build(False)
    assert oa[0]._share is not None and oa[0]._share is oa[1]._share and ob[0]._share is None
    g = torch.Generator(device="cuda").manual_seed(8)
    for _ in range(3):
        ids = torch.randint(0, V, (B, F), generator=g, device="cuda")
        feats = {"C%d" % f: ids[:, f].contiguous() for f in range(F)}
        labels = {"click_label": (torch.rand((B, 1), generator=g, device="cuda") < 0.3).float(),
                  "convert_label": (torch.rand((B, 1), generator=g, device="cuda") < 0.1).float()}
        for m, d in ((a, da), (b, db)):
            d.zero_grad(set_to_none=True)
            loss, _ = m.get_loss(feats, labels, m(feats))
            loss.backward()
            d.step()
    assert oa[0]._share.hits == 3
    for (na, pa), (nb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert na == nb and torch.equal(pa.data, pb.data), na
    for xa, xb in zip(oa[0].accums + oa[1].accums, ob[0].accums + ob[1].accums):
        assert torch.equal(xa, xb)


@pytest.mark.parametrize("normalize", [False, True])
def test_din_fused_backward_matches_composite(built_lib, normalize, monkeypatch):
    """The fused HIP backward against the GPU composite it replaces (same inputs, hist_len = None, pruned ids and a pruned
    candidate), and bitwise run-to-run reproducibility of its weight gradients."""
    from dir_amd import autograd as ag
    B, T, K, H1, H2, V = 300, 40, 64, 80, 40, 1000
    g = torch.Generator().manual_seed(5)
    table = (torch.randn(V, K, generator=g) * 0.3).cuda()
    hist = torch.randint(-1, V, (B, T), generator=g).cuda()
    cand = torch.randint(0, V, (B,), generator=g).cuda()
    Ws = [torch.randn(4 * K, H1, generator=g) * 0.2, torch.randn(H1, generator=g) * 0.1, torch.randn(H1, H2, generator=g) * 0.3,
          torch.randn(H2, generator=g) * 0.1, torch.randn(H2, generator=g) * 0.4, torch.randn(1, generator=g) * 0.1]
    gout = torch.randn(B, K, generator=g).cuda()

    def run():
        tab = table.clone().requires_grad_(True)
        ws = [w.cuda().requires_grad_(True) for w in Ws]
        ag.din_attention_pool(tab, hist, None, cand, *ws, normalize=normalize).backward(gout)
        return [tab.grad.to_dense()] + [w.grad for w in ws]

    fused = run()
    again = run()
    for a, b in zip(fused[1:], again[1:]):
        assert torch.equal(a, b)
    monkeypatch.setattr(ag, "_DIN_COMPOSITE_BACKWARD", True)
    comp = run()
    for a, b in zip(fused, comp):
        _close(a, b, tol=2e-5)


def test_din_fused_backward_empty_and_limits(built_lib):
    from dir_amd import ops
    from dir_amd._lib import DirError
    K, H1, H2, T, V = 64, 80, 40, 10, 50
    g = torch.Generator().manual_seed(1)
    table = torch.randn(V, K, generator=g).cuda()
    Ws = [torch.randn(4 * K, H1, generator=g).cuda(), torch.zeros(H1).cuda(), torch.randn(H1, H2, generator=g).cuda(), torch.zeros(H2).cuda(),
          torch.randn(H2, generator=g).cuda(), torch.zeros(1).cuda()]
    hist = torch.randint(0, V, (4, T), generator=g).cuda()
    r = ops.din_attention_pool_backward(table, hist, torch.zeros(4, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int64).cuda(),
                                        *Ws, torch.randn(4, K, generator=g).cuda())
    assert r["gh"].shape == (0, K) and r["ids_h"].numel() == 0
    for k in ("ga", "gW1", "gb1", "gW2", "gb2", "gW3", "gb3"):
        assert float(r[k].abs().max()) == 0.0, k
    assert not ops.din_backward_supported(32, 10, 36, 20) and not ops.din_backward_supported(64, 65, 80, 40)
    t32 = torch.randn(V, 32).cuda()
    with pytest.raises(DirError):
        ops.din_attention_pool_backward(t32, hist, None, torch.zeros(4, dtype=torch.int64).cuda(), torch.randn(128, 36).cuda(),
                                        torch.zeros(36).cuda(), torch.randn(36, 20).cuda(), torch.zeros(20).cuda(),
                                        torch.randn(20).cuda(), torch.zeros(1).cuda(), torch.randn(4, 32).cuda())


def test_din_saved_activations_edges(built_lib):
    """The training pair at its edges: every history empty (no tile, no record), full-length histories of T = 64 (four tiles), a batch of
    one, an empty batch through autograd, and the C entry's argument checks (unsupported shape class, workspace too small)."""
    import ctypes
    from dir_amd import _lib, ops
    from dir_amd import autograd as ag
    from dir_amd._lib import DirError
    K, H1, H2, V = 64, 80, 40, 300
    g = torch.Generator().manual_seed(11)
    table = (torch.randn(V, K, generator=g) * 0.3).cuda()
    Ws = [(torch.randn(4 * K, H1, generator=g) * 0.1).cuda(), torch.zeros(H1).cuda(), (torch.randn(H1, H2, generator=g) * 0.2).cuda(),
          torch.zeros(H2).cuda(), (torch.randn(H2, generator=g) * 0.5).cuda(), torch.zeros(1).cuda()]
    for B, T, lens in ((5, 10, "zero"), (3, 64, "full"), (1, 50, "full"), (6, 33, "mixed")):
        hist = torch.randint(0, V, (B, T), generator=g).cuda()
        hl = {"zero": torch.zeros(B, dtype=torch.int32), "full": torch.full((B,), T, dtype=torch.int32),
              "mixed": torch.randint(0, T + 1, (B,), generator=g).to(torch.int32)}[lens].cuda()
        cand = torch.randint(0, V, (B,), generator=g).cuda()
        gout = torch.randn(B, K, generator=g).cuda()
        for normalize in (True, False):
            out, sc, saved = ops.din_attention_pool_save(table, hist, hl, cand, *Ws, normalize=normalize)
            packed, ops.DIN_PACKED = ops.DIN_PACKED, False          # the inference form of the SAME kernel (din_wave_k): bit for bit
            try:
                out0, sc0 = ops.din_attention_pool(table, hist, hl, cand, *Ws, normalize=normalize, want_scores=True)
            finally:
                ops.DIN_PACKED = packed
            assert torch.equal(out, out0) and torch.equal(sc, sc0)
            outp, scp = ops.din_attention_pool(table, hist, hl, cand, *Ws, normalize=normalize, want_scores=True)     # round 6: the packed kernel (another summation order)
            assert float((outp - out).abs().max()) <= 2e-6 * (1 + float(out.abs().max())) and float((scp - sc).abs().max()) <= 2e-6 * (1 + float(sc.abs().max()))
            assert saved[0].n_tiles == int(((hl.clamp(0, T).long() + 15) // 16).sum())
            ref = ops.din_attention_pool_backward(table, hist, hl, cand, *Ws, gout, normalize=normalize, scores=sc0)
            got = ops.din_attention_pool_backward(table, hist, hl, cand, *Ws, gout, normalize=normalize, scores=sc, saved=saved)
            for k in ("gh", "ga", "gW1", "gb1", "gW2", "gb2", "gW3", "gb3"):
                a, b = ref[k].double(), got[k].double()
                err = ((a - b).abs() / (1e-3 + 0.05 * a.abs().max() + a.abs())).max().item() if a.numel() else 0.0
                assert err < (5e-3 if (k == "gb3" and normalize) else 2e-4), (B, T, lens, normalize, k, err)
    # an empty batch through autograd: zero gradients of the right shapes
    params = [w.clone().requires_grad_(True) for w in Ws]
    tab = table.clone().requires_grad_(True)
    e = ag.din_attention_pool(tab, torch.zeros((0, 7), dtype=torch.int64).cuda(), torch.zeros(0, dtype=torch.int32).cuda(),
                              torch.zeros(0, dtype=torch.int64).cuda(), *params, normalize=True)
    assert tuple(e.shape) == (0, K)
    e.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in params)
    # argument checks of the C entry
    with pytest.raises(DirError):                       # K = 32 is not this kernel's shape class
        ops.din_attention_pool_save(torch.randn(V, 32).cuda(), hist, hl, cand, torch.randn(128, 36).cuda(), torch.zeros(36).cuda(),
                                    torch.randn(36, 20).cuda(), torch.zeros(20).cuda(), torch.randn(20).cuda(), torch.zeros(1).cuda())
    lib = _lib.load()
    plan = ops.DinTrainPlan(hist, hl)
    small = torch.empty(256, dtype=torch.uint8, device="cuda")
    out = torch.empty((hist.shape[0], K), device="cuda")
    sc = torch.empty(hist.shape, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.dir_din_attention_pool_save_f32(p(table), K, p(hist), p(hl), p(cand), hist.shape[1], p(Ws[0]), p(Ws[1]), H1, p(Ws[2]), p(Ws[3]), H2,
                                             p(Ws[4]), p(Ws[5]), 1, hist.shape[0], p(out), p(sc), p(plan.tile_off), plan.n_tiles, p(small), 256, None)
    assert rc == _lib.DIR_E_BADARG and b"workspace" in lib.dir_last_error()


def test_input_layer_fused_sparse_adagrad_matches_torch(built_lib):
    """InputLayer.fused_sparse_adagrad (the ESMM / DCN towers' tables updated inside backward) against torch's sparse Adagrad."""
    from dir_amd import feature_column as fc
    from dir_amd.esmm import ESMM
    V, K, F, B = 60, 8, 5, 90
    cols = [fc.embedding_column(fc.categorical_column_with_identity("C%d" % i, V), K) for i in range(F)]
    torch.manual_seed(3)
    a = ESMM(columns=cols, dnn_hidden_units=[16, 8]).cuda()
    b = ESMM(columns=cols, dnn_hidden_units=[16, 8]).cuda()
    b.load_state_dict(a.state_dict())
    tabs_b = [p for n, p in b.named_parameters() if "embedding_weights" in n]
    opt_b = torch.optim.Adagrad(tabs_b, lr=0.1, initial_accumulator_value=0.1, eps=0.0)
    keep = a.ctr_model.input_layer.fused_sparse_adagrad(0.1) + a.cvr_model.input_layer.fused_sparse_adagrad(0.1)
    assert keep
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        ids = torch.randint(0, V, (B, F), generator=g)
        feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
        labels = {"click_label": torch.randint(0, 2, (B, 1), generator=g).float().cuda(),
                  "convert_label": torch.randint(0, 2, (B, 1), generator=g).float().cuda()}
        la, _ = a.get_loss(feats, labels, a(feats))
        la.backward()
        opt_b.zero_grad(set_to_none=True)
        lb, _ = b.get_loss(feats, labels, b(feats))
        lb.backward()
        opt_b.step()
        for p in a.parameters():            # the dense parameters are not stepped in this test
            p.grad = None
        for p in b.parameters():
            p.grad = None
    ta = [p for n, p in a.named_parameters() if "embedding_weights" in n]
    for pa, pb in zip(ta, tabs_b):
        _close(pa, pb, tol=2e-6)


@pytest.mark.parametrize("dims,M", [([416, 400, 400, 400], 300), ([64, 80, 16], 300), ([32, 1024], 300),
                                    # at >= ops.DENSE_BF3_MIN_ROWS rows the layers (forward, gated data gradients) run on the bf16x3 kernel
                                    ([416, 400, 400, 400], 12288), ([432, 1024, 1024], 12300)])
def test_mlp_stack_matches_float64(built_lib, dims, M):
    """dense._MlpStackFn (dir_dense_f32 / dir_dense_bf16x3_f32 forward, gated data gradients through the ReLUs) against float64
    autograd."""
    from dir_amd import dense as D
    from dir_amd import ops
    g = torch.Generator().manual_seed(sum(dims))
    assert (ops.dense_auto_arith(M, dims[0], dims[1]) == "bf16x3") == (M >= ops.DENSE_BF3_MIN_ROWS)
    torch.manual_seed(sum(dims) + M)             # nn.Linear's default initialisation draws from the global generator
    lins = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]).cuda()
    # A ReLU is discontinuous in its gradient: a pre-activation within rounding of zero may land on either side in fp32 (either
    # arithmetic) and flips a whole row of dL/dx by one unit's contribution.  With 12 288 rows x 1 200 units some always do, so rows
    # with a pre-activation closer to zero than 2e-5 (float64) are left out of the inputs.
    xraw = torch.randn(M + M // 4 + 8, dims[0], generator=g)
    with torch.no_grad():
        h, keep = xraw.double(), torch.ones(xraw.shape[0], dtype=torch.bool)
        for l in lins:
            z = h @ l.weight.detach().double().cpu().t() + l.bias.detach().double().cpu()
            keep &= z.abs().min(dim=1).values > 2e-5
            h = torch.relu(z)
    assert int(keep.sum()) >= M
    x = xraw[keep][:M].contiguous().cuda().requires_grad_(True)
    gout = torch.randn(M, dims[-1], generator=g).cuda()
    assert D.mlp_stack_supported(lins, x, torch.relu)
    y = D.mlp_stack(lins, x)
    y.backward(gout)
    if M >= ops.DENSE_BF3_MIN_ROWS:              # run-to-run bitwise reproducibility of the bf16x3 dense kernel
        for _ in range(3):
            assert torch.equal(D.mlp_stack(lins, x.detach().requires_grad_(True)).detach(), y.detach())
    x64 = x.detach().double().cpu().requires_grad_(True)
    p64 = [(l.weight.detach().double().cpu().requires_grad_(True), l.bias.detach().double().cpu().requires_grad_(True)) for l in lins]
    h = x64
    for w, b in p64:
        h = torch.relu(h @ w.t() + b)
    h.backward(gout.double().cpu())
    _close(y, h, tol=1e-5)
    _close(x.grad, x64.grad, tol=2e-5)
    for l, (w, b) in zip(lins, p64):
        scale = 1 + float(w.grad.abs().max())
        assert float((l.weight.grad.double().cpu() - w.grad).abs().max()) <= 2e-5 * scale
        assert float((l.bias.grad.double().cpu() - b.grad).abs().max()) <= 2e-5 * (1 + float(b.grad.abs().max()))
    assert not D.mlp_stack_supported(lins, x, torch.tanh)
    with torch.no_grad():
        assert not D.mlp_stack_supported(lins, x, torch.relu)


@pytest.mark.parametrize("M,N,K,gpad,xpad", [(300, 40, 52, 0, 0), (1, 16, 16, 0, 0), (33, 20, 4, 4, 8), (1000, 400, 416, 0, 16), (257, 260, 212, 4, 0),
                                              (4100, 516, 132, 0, 0), (8192, 400, 400, 0, 0), (9000, 1024, 432, 0, 0), (5000, 300, 1028, 8, 8)])
def test_dense_dw_bf16x3_matches_float64(built_lib, M, N, K, gpad, xpad):
    """dir_dense_dw_bf16x3_f32 (dW = g^T x with both operands transposed and split on the fly) against float64: every tail (rows off the
    32 grid, widths off the 16 / 256 / block grids), strided operands, bitwise reproducible, same bar as the library formulation."""
    from dir_amd import ops
    gen = torch.Generator().manual_seed(M + N + K)
    gbuf = (torch.randn(M, N + gpad, generator=gen) * 0.5).cuda()
    xbuf = torch.randn(M, K + xpad, generator=gen).cuda()
    g, x = gbuf[:, :N], xbuf[:, :K]
    ref = g.double().t() @ x.double()
    got = ops.dense_dw(g, x, arith="bf16x3")
    assert got.shape == (N, K)
    scale = 1 + M ** 0.5 * 0.5
    err = float((got.double() - ref).abs().max()) / scale
    lib = float((ops.dense_dw(g, x, arith="f32").double() - ref).abs().max()) / scale
    assert err <= 1e-5, (err, lib)
    assert torch.equal(ops.dense_dw(g, x, arith="bf16x3"), got)
    gw2, gb = ops.dense_dw(g, x, arith="bf16x3", want_bias=True)           # the bias gradient from the same pass over g
    assert torch.equal(gw2, got)
    assert float((gb.double() - g.double().sum(0)).abs().max()) <= 1e-5 * scale
    assert torch.equal(ops.dense_dw(g, x, arith="bf16x3", want_bias=True)[1], gb)
    auto = ops.dense_dw(g, x)
    assert torch.equal(auto, got) == (ops.dense_dw_auto_arith(M, N, K) == "bf16x3") or M < 16


@pytest.mark.parametrize("M,N,K,gpad,xpad", [(65536, 80, 64, 0, 0), (5000, 128, 128, 0, 4), (2049, 4, 128, 4, 0), (3000, 84, 36, 0, 0), (7, 16, 8, 0, 0),
                                              (40000, 48, 32, 8, 8), (33, 128, 4, 0, 0), (65536, 80, 200, 0, 0), (4000, 64, 256, 0, 0), (3000, 128, 128, 0, 0)])
def test_dense_dw_small_matches_float64(built_lib, M, N, K, gpad, xpad):
    """dir_dense_dw_small_f32 (the tall-and-skinny TN product on fp32 FMAs; the DIN unit's per-sample term is 80 x 64) against float64,
    with the column sums of g; strided operands, every register-tile shape, bitwise reproducible."""
    from dir_amd import ops
    gen = torch.Generator().manual_seed(M + N + K)
    g = (torch.randn(M, N + gpad, generator=gen) * 0.5).cuda()[:, :N]
    x = torch.randn(M, K + xpad, generator=gen).cuda()[:, :K]
    ref = g.double().t() @ x.double()
    got, gb = ops.dense_dw(g, x, arith="small", want_bias=True)
    scale = 1 + M ** 0.5 * 0.5
    assert float((got.double() - ref).abs().max()) <= 1e-5 * scale
    assert float((gb.double() - g.double().sum(0)).abs().max()) <= 1e-5 * scale
    again, gb2 = ops.dense_dw(g, x, arith="small", want_bias=True)
    assert torch.equal(again, got) and torch.equal(gb2, gb)
    assert torch.equal(ops.dense_dw(g, x, arith="small"), got)
    if 2048 <= M < ops.DENSE_DW_MIN_ROWS and N * K >= 512:                  # (tall gradients take the MFMA kernel: faster at every such shape)
        assert ops.dense_dw_auto_arith(M, N, K) == "small" and torch.equal(ops.dense_dw(g, x), got)
    elif M >= ops.DENSE_DW_MIN_ROWS and N >= 32:
        assert ops.dense_dw_auto_arith(M, N, K) == "bf16x3" and torch.equal(ops.dense_dw(g, x), ops.dense_dw(g, x, arith="bf16x3"))
    with pytest.raises(ValueError):
        ops.dense_dw(torch.zeros(64, 132, device="cuda"), torch.zeros(64, 8, device="cuda"), arith="small")
    with pytest.raises(ValueError):
        ops.dense_dw(torch.zeros(64, 128, device="cuda"), torch.zeros(64, 256, device="cuda"), arith="small")       # 512 tiles of 8 x 8


@pytest.mark.parametrize("M,N,K,arith", [(65536, 400, 416, "bf16x3"), (65521, 1024, 432, "bf16x3"), (65536, 80, 64, "small"), (65536, 64, 256, "small")])
def test_dense_dw_full_size_selection_is_exact(built_lib, M, N, K, arith):
    """A size-independent property at the BASELINE batch: with g[r_n, n] = 1 for one row r_n per output row n (zero elsewhere) the
    gradient row n is x[r_n, :] EXACTLY -- the three bf16 pieces of a value sum to it, products with 1 and sums with 0 are exact --
    and the bias gradient is all ones; with g = 2^-3 on two selected rows per n, the sum of two scaled rows (exact on the FMA kernel)."""
    from dir_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(N + K)
    x = torch.randn((M, K), generator=gen, device="cuda") * 3.0
    rows = torch.randperm(M, generator=gen, device="cuda")[:2 * N]
    r1, r2 = rows[:N], rows[N:]
    g = torch.zeros((M, N), device="cuda")
    g[r1, torch.arange(N, device="cuda")] = 1.0
    dW, db = ops.dense_dw(g, x, arith=arith, want_bias=True)
    assert torch.equal(dW, x[r1]) and torch.equal(db, torch.ones(N, device="cuda"))
    g[r2, torch.arange(N, device="cuda")] = 0.125
    g[r1, torch.arange(N, device="cuda")] = 0.125
    dW2 = ops.dense_dw(g, x, arith=arith)
    want = x[r1] * 0.125 + x[r2] * 0.125
    if arith == "small":          # fp32 FMAs: two exact products, one rounding -- the fp32 sum, in whichever order the spans add them
        assert torch.equal(dW2, want)
    else:                         # bf16x3: the six piece products of the two terms interleave in the fp32 accumulator (fp32-equivalent, not fp32-identical)
        assert float((dW2 - want).abs().max()) <= 2e-6 * float(want.abs().max())


def test_dense_dw_bf16x3_edges(built_lib):
    from dir_amd import ops
    z, zb = ops.dense_dw(torch.empty(0, 24, device="cuda"), torch.empty(0, 36, device="cuda"), arith="bf16x3", want_bias=True)    # empty batch: zero gradients
    assert z.shape == (24, 36) and float(z.abs().max()) == 0.0 and zb.shape == (24,) and float(zb.abs().max()) == 0.0
    big = torch.full((64, 16), 3.0e18, device="cuda")                                                               # fp32 exponent range
    small = torch.full((64, 16), 1.0e-18, device="cuda")
    got = ops.dense_dw(big, small, arith="bf16x3")
    assert float((got - 192.0).abs().max()) <= 1e-3
    with pytest.raises(ValueError):
        ops.dense_dw(torch.zeros(8, 4, device="cuda"), torch.zeros(9, 4, device="cuda"))
    odd_g, odd_x = torch.randn(64, 18, device="cuda"), torch.randn(64, 20, device="cuda")       # N % 4 != 0: the library takes it
    with pytest.raises(ValueError):
        ops.dense_dw(odd_g, odd_x, arith="bf16x3")
    assert torch.allclose(ops.dense_dw(odd_g, odd_x), odd_g.t() @ odd_x, atol=1e-4)
    with pytest.raises(ValueError):
        ops.dense_dw(torch.randn(64, 24, device="cuda")[:, 1:21], odd_x, arith="bf16x3")        # a view that is not 16-byte aligned
    assert ops.dense_dw_auto_arith(65536, 400, 416) == "bf16x3" and ops.dense_dw_auto_arith(65536, 200, 360) == "bf16x3"
    assert ops.dense_dw_auto_arith(65536, 360, 416) == "bf16x3" and ops.dense_dw_auto_arith(65536, 320, 320) == "bf16x3"
    assert ops.dense_dw_auto_arith(65536, 128, 1024) == "f32" and ops.dense_dw_auto_arith(65536, 1024, 128) == "bf16x3"
    assert ops.dense_dw_auto_arith(65536, 80, 200) == "bf16x3" and ops.dense_dw_auto_arith(65536, 16, 416) == "f32"
    assert ops.dense_dw_auto_arith(4096, 400, 416) == "f32" and ops.dense_dw_auto_arith(4096, 80, 64) == "small"


@pytest.mark.parametrize("B,N,pad", [(300, 400, 0), (1, 16, 0), (65, 64, 4), (1000, 1024, 0), (777, 520, 8), (4096, 4096, 0), (33, 132, 0)])
def test_units1_relu_backward_kernel(built_lib, B, N, pad):
    """dir_units1_relu_backward_f32 (the logit layer's backward through the ReLU below it, one pass) against float64, strided
    activations, bitwise reproducible; refusals."""
    from dir_amd import ops
    g = torch.Generator().manual_seed(B + N)
    ybuf = torch.relu(torch.randn(B, N + pad, generator=g)).cuda()
    y = ybuf[:, :N]
    dl = torch.randn(B, 1, generator=g).cuda()
    w = (torch.randn(1, N, generator=g) / N ** 0.5).cuda()
    gx, gw, gb = ops.units1_relu_backward(dl, w, y)
    y64, dl64, w64 = y.double().cpu(), dl.double().cpu(), w.double().cpu()
    rx = torch.where(y64 > 0, dl64 * w64, torch.zeros((), dtype=torch.float64))
    assert torch.equal(gx.cpu(), torch.where(y.cpu() > 0, dl.cpu() * w.cpu(), torch.zeros(())))      # one fp32 product per element: exact
    _close(gw, (dl64 * y64).sum(0), tol=1e-5 * (1 + B ** 0.5 * 0.05))
    _close(gb, rx.sum(0), tol=1e-5 * (1 + B ** 0.5 * 0.05))
    gx2, gw2, gb2 = ops.units1_relu_backward(dl.reshape(B), w.reshape(N), y)
    assert torch.equal(gx2, gx) and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    with pytest.raises(ValueError):
        ops.units1_relu_backward(dl, w[:, :N - 1], y)
    if N >= 8:
        with pytest.raises(ValueError):
            ops.units1_relu_backward(dl, w[:, :N - 2], y[:, :N - 2])          # N % 4 != 0


@pytest.mark.parametrize("dims,M", [([416, 400, 400, 400], 300), ([64, 80, 16], 300), ([416, 400, 400], 12288)])
def test_mlp_head_matches_float64(built_lib, dims, M):
    """dense._MlpHeadFn (the tower and its units = 1 logit layer as one node: dir_units1_relu_backward_f32 + the stack's gated data
    gradients) against float64 autograd, and against the two-node formulation (mlp_stack + units1)."""
    from dir_amd import dense as D
    g = torch.Generator().manual_seed(sum(dims) + 1)
    torch.manual_seed(sum(dims) + M + 1)
    lins = torch.nn.ModuleList([torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]).cuda()
    head = torch.nn.Linear(dims[-1], 1).cuda()
    xraw = torch.randn(M + M // 4 + 8, dims[0], generator=g)
    with torch.no_grad():                        # rows with a pre-activation within 2e-5 of zero are left out (see test_mlp_stack_matches_float64)
        h, keep = xraw.double(), torch.ones(xraw.shape[0], dtype=torch.bool)
        for l in lins:
            z = h @ l.weight.detach().double().cpu().t() + l.bias.detach().double().cpu()
            keep &= z.abs().min(dim=1).values > 2e-5
            h = torch.relu(z)
    x = xraw[keep][:M].contiguous().cuda().requires_grad_(True)
    gout = torch.randn(M, 1, generator=g).cuda()
    assert D.mlp_head_supported(lins, head, x, torch.relu)
    y = D.mlp_head(lins, head, x)
    y.backward(gout)
    got = [x.grad.clone(), head.weight.grad.clone(), head.bias.grad.clone()] + [p.grad.clone() for l in lins for p in (l.weight, l.bias)]
    x64 = x.detach().double().cpu().requires_grad_(True)
    p64 = [(l.weight.detach().double().cpu().requires_grad_(True), l.bias.detach().double().cpu().requires_grad_(True)) for l in lins]
    hw, hb = head.weight.detach().double().cpu().requires_grad_(True), head.bias.detach().double().cpu().requires_grad_(True)
    h = x64
    for w, b in p64:
        h = torch.relu(h @ w.t() + b)
    out = h @ hw.t() + hb
    out.backward(gout.double().cpu())
    _close(y, out, tol=1e-5)
    ref = [x64.grad, hw.grad, hb.grad] + [t.grad for wb in p64 for t in wb]
    for a, r in zip(got, ref):
        assert float((a.double().cpu() - r).abs().max()) <= 2e-5 * (1 + float(r.abs().max()))
    # the two-node formulation computes the same thing with torch ops for the head
    for p in [x, head.weight, head.bias] + [q for l in lins for q in (l.weight, l.bias)]:
        p.grad = None
    y2 = D.units1(head, D.mlp_stack(lins, x))
    y2.backward(gout)
    _close(y2, y, tol=1e-6)
    two = [x.grad, head.weight.grad, head.bias.grad] + [p.grad for l in lins for p in (l.weight, l.bias)]
    for a, r in zip(got, two):
        assert float((a - r).abs().max()) <= 2e-5 * (1 + float(r.abs().max()))


def test_dense_act_pads_odd_input_width(built_lib):
    """dense.dense_act with in_features % 4 != 0 (DCN's 429-wide first layer): zero-padded onto the HIP kernel, forward and
    gradients equal to nn.Linear + ReLU in float64."""
    from dir_amd import dense as D
    g = torch.Generator().manual_seed(9)
    M, Kd, N = 200, 429, 64
    lin = torch.nn.Linear(Kd, N).cuda()
    x = torch.randn(M, Kd, generator=g).cuda().requires_grad_(True)
    gout = torch.randn(M, N, generator=g).cuda()
    y = D.dense_act(lin, x, torch.relu)
    y.backward(gout)
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64 = lin.weight.detach().double().cpu().requires_grad_(True)
    b64 = lin.bias.detach().double().cpu().requires_grad_(True)
    ref = torch.relu(x64 @ w64.t() + b64)
    ref.backward(gout.double().cpu())
    _close(y, ref, tol=1e-5)
    _close(x.grad, x64.grad, tol=2e-5)
    assert lin.weight.grad.shape == (N, Kd)
    assert float((lin.weight.grad.double().cpu() - w64.grad).abs().max()) <= 2e-5 * (1 + float(w64.grad.abs().max()))
    assert float((lin.bias.grad.double().cpu() - b64.grad).abs().max()) <= 2e-5 * (1 + float(b64.grad.abs().max()))
    with torch.no_grad():
        y2 = D.dense_act(lin, x.detach(), torch.relu)
    assert torch.equal(y2, y.detach())


# ---- packed training rows + FM backward folded into the update (include/dir_hip.h: dir_gather_fm_rows_f32,
# dir_sparse_adagrad_sorted_rows_f32) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["uniform", "hot"])
@pytest.mark.parametrize("K", [16, 8, 32])
def test_packed_train_rows_bit_identical_to_split_layout(built_lib, dist, K):
    """Three training steps of the sparse side (gather + FM, FM backward + DNN-branch gradient, sorted sparse Adagrad) on the
    packed [embedding | accumulator] rows and with the FM backward folded into the update: forward values, tables and
    accumulators bit-identical to the split layout with the separate FM-backward pass, including duplicate, pruned and
    out-of-range ids."""
    from dir_amd import ops
    g = torch.Generator(device="cuda").manual_seed(K)
    B, F, V = 3000, 5, 700
    tabs = [torch.randn((V + 13 * f, K), generator=g, device="cuda") * 0.25 for f in range(F)]
    split = ops.TableSet([t.clone() for t in tabs])
    packed = ops.TableSet.train_rows(tabs, 0.1)
    fold = ops.TableSet([t.clone() for t in tabs])                   # split layout, FM backward folded in
    o_split, o_packed, o_fold = (ops.SparseAdagrad(ts, lr=0.05) for ts in (split, packed, fold))
    for step in range(3):
        if dist == "hot":
            ids = (torch.rand((B, F), generator=g, device="cuda") ** 6 * V).long()
        else:
            ids = torch.randint(0, V, (B, F), generator=g, device="cuda")
        ids[::97, 1] = -1                                            # pruned
        ids[5::89, 2] = V + 13 * 2 + 4                               # out of range: zero row, never written
        gfm = torch.randn((B, 1), generator=g, device="cuda") * 0.1
        gdnn = torch.randn((B, F * K), generator=g, device="cuda") * 0.1
        emb_s, fm_s = ops.gather_fm(split, ids)
        fsum = torch.empty((B, K), device="cuda")
        emb_p, fm_p = ops.gather_fm(packed, ids, fsum=fsum)
        assert torch.equal(emb_s, emb_p) and torch.equal(fm_s, fm_p)
        fsum_f = torch.empty((B, K), device="cuda")
        emb_f, fm_f = ops.gather_fm(fold, ids, fsum=fsum_f)          # the rows kernel on plain [V, K] tables (ld = K)
        assert torch.equal(emb_s, emb_f) and torch.equal(fm_s, fm_f) and torch.equal(fsum, fsum_f)
        assert torch.equal(fsum, emb_s.view(B, F, K).transpose(0, 1).contiguous().cumsum(0)[-1]) or \
            torch.allclose(fsum, emb_s.view(B, F, K).sum(1), atol=1e-5)
        demb = ops.fm_logit_backward(emb_s, gfm, F, K, add_in=gdnn)
        o_split.step(ids, demb)
        o_packed.step_fm(ids, gdnn, gfm, fsum) if step % 2 == 0 else o_packed.step(ids, demb)
        o_fold.step_fm(ids, gdnn, gfm, fsum_f)
        for f in range(F):
            assert torch.equal(split.tables[f], packed.tables[f]), (step, f)
            assert torch.equal(o_split.accums[f], o_packed.accums[f]), (step, f)
            assert torch.equal(split.tables[f], fold.tables[f]) and torch.equal(o_split.accums[f], o_fold.accums[f]), (step, f)
    with pytest.raises(ValueError):
        ops.embedding_bag(packed, ids)                               # the packed layout is read by gather_fm / SparseAdagrad only


def test_deepfm_packed_training_matches_split(built_lib):
    """DeepFM.fused_sparse_adagrad(packed=True): the same model trained three steps on packed rows and on the reference layout
    ends with identical logits and embedding tables (the dense side is the same code; the sparse side is bit-identical)."""
    from dir_amd import feature_column as fc
    from dir_amd.deepfm import DeepFM
    torch.manual_seed(3)
    F, V, K, B = 6, 500, 16, 2048
    def build():
        torch.manual_seed(11)
        cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
        return DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                      dnn_hidden_units=[32, 16], fm_embedding_size=K).cuda()
    a, b = build(), build()
    a.fused_sparse_adagrad(lr=0.05)
    b.fused_sparse_adagrad(lr=0.05, packed=True)
    a.fused_sparse_ftrl(lr=0.1)               # the linear columns through the (ordered, reproducible) fused update as well:
    b.fused_sparse_ftrl(lr=0.1)               # torch's sparse gradients sum duplicates in no fixed order
    assert b.embedding_weights[0].stride() == (2 * K, 1)
    def dense_params(m):
        skip = {id(p) for p in m.embedding_weights} | {id(p) for p in m.linear_weights}
        return [p for p in m.parameters() if id(p) not in skip]
    oa, ob = torch.optim.SGD(dense_params(a), lr=0.05), torch.optim.SGD(dense_params(b), lr=0.05)
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(3):
        ids = torch.randint(0, V, (B, F), generator=g, device="cuda")
        feats = {"C%d" % f: ids[:, f] for f in range(F)}
        y = (torch.rand((B, 1), generator=g, device="cuda") < 0.3).float()
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad(set_to_none=True)
            torch.nn.functional.binary_cross_entropy_with_logits(m(feats), y).backward()
            o.step()
    for pa, pb in zip(a.embedding_weights, b.embedding_weights):
        assert torch.equal(pa.data, pb.data)
    with torch.no_grad():
        assert torch.equal(a(feats), b(feats))
    sd = b.state_dict()
    assert sd["embedding_weights.0"].shape == (V, K)


@pytest.mark.parametrize("packed", [False, True])
def test_deepfm_sparse_optimisers_share_one_sort(built_lib, packed):
    """Adagrad on the embedding tables and FTRL on the linear columns of the same categorical columns see the same id matrix: the second
    update of a step takes the first one's sorted (row, entry) pairs (dir_sparse_*_sorted_*_from_f32).  Same tables, accumulators and
    linear weights, bit for bit, as two updates that sort themselves; a changed id tensor or a reallocated workspace is not shared."""
    from dir_amd import feature_column as fc
    from dir_amd.deepfm import DeepFM
    F, V, K, B = 5, 300, 16, 1500
    def build():
        torch.manual_seed(21)
        cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
        m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats],
                   dnn_hidden_units=[32, 16], fm_embedding_size=K).cuda()
        return m, m.fused_sparse_adagrad(lr=0.05, packed=packed), m.fused_sparse_ftrl(lr=0.1, l1=0.001)
    (a, a_ada, a_ftrl), (b, b_ada, b_ftrl) = build(), build()
    assert a_ada._share is not None and a_ada._share is a_ftrl._share
    b_ada._share = b_ftrl._share = None                              # b: every update sorts for itself
    def dense_params(m):
        skip = {id(p) for p in m.embedding_weights} | {id(p) for p in m.linear_weights}
        return [p for p in m.parameters() if id(p) not in skip]
    oa, ob = torch.optim.SGD(dense_params(a), lr=0.05), torch.optim.SGD(dense_params(b), lr=0.05)
    g = torch.Generator(device="cuda").manual_seed(6)
    for step in range(4):
        ids = torch.randint(-1 if step == 2 else 0, V, (B + 7 * step, F), generator=g, device="cuda")      # a growing batch: workspaces get reallocated
        feats = {"C%d" % f: ids[:, f] for f in range(F)}
        y = (torch.rand((ids.shape[0], 1), generator=g, device="cuda") < 0.3).float()
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad(set_to_none=True)
            torch.nn.functional.binary_cross_entropy_with_logits(m(feats), y).backward()
            o.step()
    assert a_ada._share.hits == 4                                    # one sort saved per step
    for pa, pb in zip(list(a.embedding_weights) + list(a.linear_weights), list(b.embedding_weights) + list(b.linear_weights)):
        assert torch.equal(pa.data, pb.data)
    for xa, xb in zip(a_ada.accums + a_ftrl.accums + a_ftrl.linears, b_ada.accums + b_ftrl.accums + b_ftrl.linears):
        assert torch.equal(xa, xb)
    # a token is bound to the id tensor: another tensor (same values) is not shared
    sh = a_ada._share
    ids2 = ids.clone()
    gr = torch.zeros((ids.shape[0], 1), device="cuda")
    a_ftrl.step(ids, gr)
    assert sh.token is not None
    a_ada.step(ids2, torch.zeros((ids.shape[0], F * K), device="cuda"))
    assert sh.hits == 4


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,T,H1,H2", [(300, 50, 80, 40), (67, 64, 80, 48), (41, 17, 36, 20), (9, 5, 64, 32), (130, 33, 72, 44)])
def test_din_rows_backward_matches_single_kernel(built_lib, normalize, B, T, H1, H2):
    """dir_din_attention_pool_backward_rows_f32 (wave-per-sample row pass + streaming weight-gradient pass, fed with the forward's
    attention weights) against the round-1 single-kernel backward on the same inputs: every output within fp32 summation-order
    noise; pruned ids, empty and full-length histories, pruned candidates included."""
    import os
    from dir_amd import ops
    K, V = 64, 5000
    g = torch.Generator().manual_seed(B + T)
    table = (torch.randn(V, K, generator=g) * 0.3).cuda()
    Ws = [(torch.randn(4 * K, H1, generator=g) * 0.1).cuda(), (torch.randn(H1, generator=g) * 0.1).cuda(),
          (torch.randn(H1, H2, generator=g) * 0.2).cuda(), (torch.randn(H2, generator=g) * 0.1).cuda(),
          (torch.randn(H2, generator=g) * 0.5).cuda(), torch.randn(1, generator=g).cuda()]
    hist = torch.randint(0, V, (B, T), generator=g)
    hist[torch.rand((B, T), generator=g) < 0.1] = -1
    hl = torch.randint(0, T + 1, (B,), generator=g).to(torch.int32)
    hl[0], hl[1 % B] = T, 0
    cand = torch.randint(0, V, (B,), generator=g)
    cand[3 % B] = -1
    hist, hl, cand = hist.cuda(), hl.cuda(), cand.cuda()
    gout = torch.randn(B, K, generator=g).cuda()
    out, scores = ops.din_attention_pool(table, hist, hl, cand, *Ws, normalize=normalize, want_scores=True)
    ref = ops.din_attention_pool_backward(table, hist, hl, cand, *Ws, gout, normalize=normalize)
    got = ops.din_attention_pool_backward(table, hist, hl, cand, *Ws, gout, normalize=normalize, scores=scores)
    assert torch.equal(ref["ids_h"], got["ids_h"])
    for k in ("gh", "ga", "gW1", "gb1", "gW2", "gb2", "gW3", "gb3"):
        a, b = ref[k].double(), got[k].double()
        err = ((a - b).abs() / (1e-3 + 0.05 * a.abs().max() + a.abs())).max().item() if a.numel() else 0.0
        # (with the softmax, d b3 = sum of d score is a sum that cancels to ~0: only its absolute size is meaningful)
        assert err < (5e-3 if (k == "gb3" and normalize) else 2e-4), (k, err)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,T,H1,H2", [(300, 50, 80, 40), (67, 64, 80, 48), (41, 17, 36, 20), (9, 5, 64, 32)])
def test_din_saved_activations_backward_matches_recompute(built_lib, normalize, B, T, H1, H2, monkeypatch):
    """The training pair dir_din_attention_pool_save_f32 + dir_din_attention_pool_backward_saved_f32 (the forward leaves z1 / z2 of every
    history row in a workspace, the row pass reads them) against the recomputing row pass on the same inputs: same forward outputs bit
    for bit, every gradient within the 2e-4 bar of the row-pass test above (sums that cancel under the softmax set it; the saved activations come from the forward's bf16x3 arithmetic, the recomputed ones from
    fp32 MFMA: both within 1e-6 of the exact sigmoid).  Pruned ids, empty and full-length histories, a pruned candidate included."""
    from dir_amd import ops
    K, V = 64, 5000
    g = torch.Generator().manual_seed(B * 3 + T)
    table = (torch.randn(V, K, generator=g) * 0.3).cuda()
    Ws = [(torch.randn(4 * K, H1, generator=g) * 0.1).cuda(), (torch.randn(H1, generator=g) * 0.1).cuda(),
          (torch.randn(H1, H2, generator=g) * 0.2).cuda(), (torch.randn(H2, generator=g) * 0.1).cuda(),
          (torch.randn(H2, generator=g) * 0.5).cuda(), torch.randn(1, generator=g).cuda()]
    hist = torch.randint(0, V, (B, T), generator=g)
    hist[torch.rand((B, T), generator=g) < 0.1] = -1
    hl = torch.randint(0, T + 1, (B,), generator=g).to(torch.int32)
    hl[0], hl[1 % B] = T, 0
    cand = torch.randint(0, V, (B,), generator=g)
    cand[3 % B] = -1
    hist, hl, cand = hist.cuda(), hl.cuda(), cand.cuda()
    gout = torch.randn(B, K, generator=g).cuda()
    for arith in ("f16x2", "bf16x3", "f32"):
        monkeypatch.setenv("DIR_DIN_ARITH", arith)
        out0, sc0 = ops.din_attention_pool(table, hist, hl, cand, *Ws, normalize=normalize, want_scores=True)
        out1, sc1, saved = ops.din_attention_pool_save(table, hist, hl, cand, *Ws, normalize=normalize)
        assert torch.equal(out0, out1) and torch.equal(sc0, sc1)
        ref = ops.din_attention_pool_backward(table, hist, hl, cand, *Ws, gout, normalize=normalize, scores=sc0)
        got = ops.din_attention_pool_backward(table, hist, hl, cand, *Ws, gout, normalize=normalize, scores=sc1, saved=saved)
        assert torch.equal(ref["ids_h"], got["ids_h"])
        for k in ("gh", "ga", "gW1", "gb1", "gW2", "gb2", "gW3", "gb3"):
            a, b = ref[k].double(), got[k].double()
            err = ((a - b).abs() / (1e-3 + 0.05 * a.abs().max() + a.abs())).max().item() if a.numel() else 0.0
            assert err < (5e-3 if (k == "gb3" and normalize) else 2e-4), (arith, k, err)
        # bitwise reproducible
        out2, sc2, saved2 = ops.din_attention_pool_save(table, hist, hl, cand, *Ws, normalize=normalize)
        got2 = ops.din_attention_pool_backward(table, hist, hl, cand, *Ws, gout, normalize=normalize, scores=sc2, saved=saved2)
        for k in ("gh", "ga", "gW1", "gb1", "gW2", "gb2", "gW3", "gb3"):
            assert torch.equal(got[k], got2[k]), k


# ---- tf.train.AdamOptimizer on the embedding tables (dir_sparse_adam_f32) ----------------------------------------------------------
@pytest.mark.parametrize("K,gscale,clip", [(16, 0.01, 100.0), (16, 40.0, 100.0), (8, 0.01, 0.0), (64, 5.0, 100.0)])
def test_sparse_adam_matches_tf_semantics_over_steps(built_lib, K, gscale, clip):
    """5 steps of dir_sparse_adam_f32 (duplicate and pruned ids, clipping idle / active) against the float64 restatement at 1e-5; every
    row moves every step; a second optimiser fed the same data ends bitwise equal."""
    from dir_amd import ops
    rng = np.random.default_rng(K + int(gscale * 10))
    F, B, vocab = 3, 700, [50, 400, 7]
    w0 = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in vocab]
    b1, b2, eps, lr = 0.9, 0.999, 1e-4, 0.01
    ref_w = [w.astype(np.float64) for w in w0]
    ref_m = [np.zeros_like(w) for w in ref_w]
    ref_v = [np.zeros_like(w) for w in ref_w]
    runs = []
    for rep in range(2):
        tabs = [torch.from_numpy(w.copy()).cuda() for w in w0]
        opt = ops.SparseAdam(ops.TableSet(tabs), b1, b2, eps, clip)
        rng_s = np.random.default_rng(99)
        for t in range(1, 6):
            ids = np.stack([rng_s.integers(-1, v + 1, size=B) for v in vocab], 1).astype(np.int64)
            grad = (rng_s.standard_normal((B, F * K)) * gscale).astype(np.float32)
            opt.lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            opt.step(torch.from_numpy(ids).cuda(), torch.from_numpy(grad).cuda())
            if rep == 0:
                sparse_adam_step(ref_w, ref_m, ref_v, ids, grad, lr, b1, b2, eps, clip, t)
        runs.append(([t.cpu().numpy() for t in tabs], [m.cpu().numpy() for m in opt.ms], [v.cpu().numpy() for v in opt.vs]))
    for f in range(F):
        for what, got, ref in (("var", runs[0][0][f], ref_w[f]), ("m", runs[0][1][f], ref_m[f]), ("v", runs[0][2][f], ref_v[f])):
            # 1e-5 of the array's scale (m and v are orders of magnitude smaller than var: an absolute bar alone would not test them)
            err = np.abs(got - ref) / (np.abs(ref).max() + 1e-30)
            assert float(err.max()) <= 1e-5, "table %d %s: max error %.3e of the array's scale" % (f, what, float(err.max()))
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a[f], b[f])
    assert not np.array_equal(runs[0][0][0], w0[0])
    untouched = np.ones(vocab[1], bool)                  # rows never looked up still move (momentum of a zero gradient is zero here:
    assert (runs[0][1][1][untouched] == runs[0][1][1][untouched]).all()   # their m, v stay 0 and var is unchanged) -- checked via ref above


def test_dcn_train_step_hip_adam_equals_the_dense_torch_formulation(built_lib):
    """train_spec.TrainStep on a DeepCrossNetwork with Adam (eps 1e-4, clip_by_norm 100, cosine decay: DeepCrossNetwork/train.py:119-124):
    3 steps with the HIP sparse Adam on the tables against the same steps with DIR_TRAIN_HIP_ADAM=0 (dense gradient + torch Adam):
    tables and dense weights within 1e-5; then a fresh TrainStep resumed at global_step 7 takes its step with t = 8."""
    import os
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd import feature_column as fc

    def build():
        torch.manual_seed(5)
        cols = [fc.embedding_column(fc.categorical_column_with_identity("C%02d" % i, 300), 16) for i in range(6)]
        cols += [fc.numeric_column("I%02d" % i) for i in range(3)]
        return DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[64, 32], batch_norm=False, optimizer="Adam",
                                optimizer_spec={"epsilon": 1e-4},
                                learning_rate_spec={"learning_rate": 0.01, "decay_method": "cosine_decay", "decay_steps": 100, "alpha": 0.5}).cuda()

    gen = torch.Generator(device="cuda").manual_seed(1)
    B = 2048
    batches = []
    for _ in range(4):
        ids = torch.randint(0, 300, (B, 6), generator=gen, device="cuda")
        f = {"C%02d" % i: ids[:, i].contiguous() for i in range(6)}
        f.update({"I%02d" % i: torch.rand((B,), generator=gen, device="cuda") for i in range(3)})
        batches.append((f, (torch.rand((B, 1), generator=gen, device="cuda") < 0.3).float()))

    def run(hip, start_step=0, steps=3):
        os.environ["DIR_TRAIN_HIP_ADAM"] = "1" if hip else "0"
        try:
            model = build()
            op = model.train_step()
            assert bool(op.sparse_adam) == hip
            op.global_step = start_step
            for f, y in batches[:steps]:
                op(torch.nn.functional.binary_cross_entropy_with_logits(model(f), y))
            return [p.detach().clone() for p in model.parameters()], op
        finally:
            del os.environ["DIR_TRAIN_HIP_ADAM"]

    a, _ = run(True)
    b, _ = run(False)
    for x, y in zip(a, b):
        assert float((x - y).abs().max()) <= 1e-5
    # resumed: the first step of a fresh optimizer at global_step 7 uses t = 8 on both paths (torch's per-parameter counters)
    a7, op7 = run(True, start_step=7, steps=1)
    b7, _ = run(False, start_step=7, steps=1)
    for x, y in zip(a7, b7):
        assert float((x - y).abs().max()) <= 1e-5
    assert op7.global_step == 8
    a0, _ = run(True, start_step=0, steps=1)
    assert any(float((x - y).abs().max()) > 1e-6 for x, y in zip(a7, a0))      # t = 8 and t = 1 give different steps


def _bn_ref64(y64, gamma64, beta64, eps):
    mean = y64.mean(dim=0)
    var = y64.var(dim=0, unbiased=False)
    inv = torch.rsqrt(var + eps)
    scale = inv * gamma64 if gamma64 is not None else inv
    return y64 * scale + ((beta64 if beta64 is not None else 0.0) - mean * scale), mean, var


@pytest.mark.parametrize("B,N,pad,scale", [(1, 4, 0, True), (300, 16, 4, True), (1000, 400, 0, False), (4097, 1024, 8, True), (257, 2048, 0, False),
                                           (65, 36, 0, True)])
def test_bn_train_kernels_match_float64(built_lib, B, N, pad, scale):
    """dir_bn_train_stats_f32 / dir_bn_train_backward_f32 (training-mode batch norm, deepFM.py:303-308 / DeepCrossNetwork.py:400-403) against
    float64 autograd of the same expression: statistics, moving statistics, the normalised activation, dL/dy with and without the ReLU gate,
    dgamma, dbeta; strided operands; reruns bitwise equal."""
    from dir_amd import ops
    g = torch.Generator().manual_seed(B * 7 + N)
    eps, mom = 1e-3, 0.999
    ybuf = (torch.relu(torch.randn(B, N + pad, generator=g)) * 1.7 + 0.1 * torch.randn(B, N + pad, generator=g).abs()).cuda()
    y = ybuf[:, :N]
    gbuf = torch.randn(B, N + pad, generator=g).cuda()
    gout = gbuf[:, :N]
    gamma = (1.0 + 0.3 * torch.randn(N, generator=g)).cuda() if scale else None
    beta = (0.2 * torch.randn(N, generator=g)).cuda()
    mm0, mv0 = torch.randn(N, generator=g).cuda(), (torch.rand(N, generator=g) + 0.5).cuda()
    mm, mv = mm0.clone(), mv0.clone()
    mean, inv, sc, sh = ops.bn_train_stats(y, gamma, beta, mm, mv, eps, mom)
    y64 = y.double().cpu().requires_grad_(True)
    g64 = None if gamma is None else gamma.double().cpu().requires_grad_(True)
    b64 = beta.double().cpu().requires_grad_(True)
    out64, mean64, var64 = _bn_ref64(y64, g64, b64, eps)
    _close(mean, mean64)
    _close(inv, torch.rsqrt(var64 + eps), tol=2e-5)
    _close(y * sc + sh, out64, tol=2e-5)
    _close(mm, mm0.double().cpu() * mom + mean64 * (1 - mom))
    _close(mv, mv0.double().cpu() * mom + var64 * (1 - mom))
    out64.backward(gout.double().cpu())
    gy, gb, gg = ops.bn_train_backward(gout, y, mean, inv, gamma, relu_gate=False)
    bar = 2e-5 * (1 + B ** 0.5 * 0.05)
    _close(gy, y64.grad, tol=bar)
    _close(gb, b64.grad, tol=bar)
    if gamma is not None:
        _close(gg, g64.grad, tol=bar)
    gy2, gb2, gg2 = ops.bn_train_backward(gout, y, mean, inv, gamma, relu_gate=True)
    assert torch.equal(gy2, torch.where(y > 0, gy, torch.zeros((), device="cuda"))) and torch.equal(gb2, gb) and torch.equal(gg2, gg)
    mm2, mv2 = mm0.clone(), mv0.clone()
    again = ops.bn_train_stats(y, gamma, beta, mm2, mv2, eps, mom)
    assert all(torch.equal(a, b) for a, b in zip(again, (mean, inv, sc, sh))) and torch.equal(mm2, mm) and torch.equal(mv2, mv)
    assert torch.equal(ops.bn_train_backward(gout, y, mean, inv, gamma, relu_gate=False)[0], gy)
    if N >= 8:
        with pytest.raises(ValueError):
            ops.bn_train_stats(y[:, :N - 2], None, None, None, None, eps, mom)          # N % 4 != 0
    with pytest.raises(ValueError):
        ops.bn_train_stats(y[:0], gamma, beta, None, None, eps, mom)


@pytest.mark.parametrize("din,dout,M,scale", [(416, 400, 8192, True), (432, 1024, 6200, False)])
def test_dense_bn_train_node_matches_the_torch_formulation(built_lib, din, dout, M, scale):
    """dense._DenseBnFn (hidden layer + training batch norm as one node) against float64 autograd of relu(x W^T + b) -> batch norm and against
    the module formulation it replaces (DIR_BN_TRAIN_FUSED=0: _DenseFn + _BatchNormInfer): output, every gradient, the moving statistics."""
    from dir_amd import dense as D
    from dir_amd.deepfm import _BatchNormInfer
    g = torch.Generator().manual_seed(din + dout)
    torch.manual_seed(din)
    lin = torch.nn.Linear(din, dout).cuda()
    bn = _BatchNormInfer(dout, eps=1e-3, scale=scale).cuda().train()
    with torch.no_grad():
        bn.beta.copy_(0.1 * torch.randn(dout, generator=g))
        if scale:
            bn.gamma.copy_(1.0 + 0.2 * torch.randn(dout, generator=g))
    xraw = torch.randn(M + M // 4, din, generator=g)
    with torch.no_grad():                        # rows with a pre-activation within 2e-5 of zero are left out (the ReLU gate is discontinuous there)
        z = xraw.double() @ lin.weight.detach().double().cpu().t() + lin.bias.detach().double().cpu()
        keep = z.abs().min(dim=1).values > 2e-5
    x = xraw[keep][:M].contiguous().cuda().requires_grad_(True)
    assert x.shape[0] == M
    gout = torch.randn(M, dout, generator=g).cuda()
    params = [lin.weight, lin.bias, bn.beta] + ([bn.gamma] if scale else [])

    def run(fused):
        for p in [x] + params:
            p.grad = None
        bn.moving_mean.zero_()
        bn.moving_variance.fill_(1.0)
        D.BN_TRAIN_FUSED = fused
        try:
            out = D.dense_act(lin, x, torch.relu, bn=bn)
        finally:
            D.BN_TRAIN_FUSED = True
        out.backward(gout)
        return [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params] + [bn.moving_mean.clone(), bn.moving_variance.clone()]

    got = run(True)
    two = run(False)
    x64 = x.detach().double().cpu().requires_grad_(True)
    p64 = [p.detach().double().cpu().requires_grad_(True) for p in params]
    y64 = torch.relu(x64 @ p64[0].t() + p64[1])
    out64, mean64, var64 = _bn_ref64(y64, p64[3] if scale else None, p64[2], 1e-3)
    out64.backward(gout.double().cpu())
    ref = [out64.detach(), x64.grad] + [p.grad for p in p64] + [mean64.detach() * 0.001, 0.999 + var64.detach() * 0.001]
    for a, r in zip(got, ref):
        assert float((a.double().cpu() - r).abs().max()) <= 3e-5 * (1 + float(r.abs().max()))
    for a, r in zip(got, two):
        assert float((a - r).abs().max()) <= 3e-5 * (1 + float(r.abs().max()))


def test_dcn_training_forward_without_the_concat_equals_the_plain_form(built_lib):
    """DeepCrossNetwork in TRAIN mode: logits and every parameter gradient of the split form (cross . w_c + deep . w_d, last hidden layer +
    logit share as one node, hidden layer + batch norm as one node) against the plain form (concat + nn.Linear, module batch norm)."""
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd import feature_column as fc
    from dir_amd import dense as D
    torch.manual_seed(5)
    B, F, K, V = 6400, 6, 8, 50
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
    cols = [fc.embedding_column(c, K) for c in cats] + [fc.numeric_column("x")]            # d = 49: the odd-width first layer
    dcn = DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[64, 32, 48], batch_norm=True).cuda().train()
    ids = torch.randint(0, V, (B, F))
    feats = {"C%d" % i: ids[:, i].cuda() for i in range(F)}
    feats["x"] = torch.rand(B).cuda()
    labels = (torch.rand(B, 1) < 0.3).float().cuda()
    params = [p for p in dcn.parameters()]

    def run(split):
        for p in params:
            p.grad = None
        for bn in dcn.bns:
            bn.moving_mean.zero_()
            bn.moving_variance.fill_(1.0)
        old = (D.BN_TRAIN_FUSED, dcn._train_logits)
        if not split:
            D.BN_TRAIN_FUSED = False
            dcn._train_logits = lambda x0, cross: None
        try:
            out = dcn(feats)
            torch.nn.functional.binary_cross_entropy_with_logits(out, labels).backward()
        finally:
            D.BN_TRAIN_FUSED = old[0]
            if not split:
                del dcn._train_logits
        grads = [(p.grad.to_dense() if p.grad.is_sparse else p.grad).clone() for p in params]
        return out.detach().clone(), grads, [bn.moving_mean.clone() for bn in dcn.bns]

    out_a, grads_a, mm_a = run(True)
    out_b, grads_b, mm_b = run(False)
    assert float((out_a - out_b).abs().max()) <= 2e-5 * (1 + float(out_b.abs().max()))
    for a, b in zip(grads_a, grads_b):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 3e-5 * (1 + float(b.abs().max()))
    for a, b in zip(mm_a, mm_b):
        assert float((a - b).abs().max()) <= 1e-6


@pytest.mark.parametrize("B,N,pad", [(1, 1, 0), (300, 429, 3), (4099, 51, 0), (65, 1453, 0), (1000, 16, 4)])
def test_units1_backward_kernel_any_width(built_lib, B, N, pad):
    """dir_units1_backward_f32 (the units = 1 layer on an activation of any width: DCN's 429-wide cross output) against float64; strided x;
    reruns bitwise equal; the gx-less form; an empty batch."""
    from dir_amd import ops
    g = torch.Generator().manual_seed(B + N)
    xbuf = torch.randn(B, N + pad, generator=g).cuda()
    x = xbuf[:, :N]
    dl = torch.randn(B, 1, generator=g).cuda()
    w = (torch.randn(1, N, generator=g) / N ** 0.5).cuda()
    gx, gw = ops.units1_backward(dl, w, x)
    assert torch.equal(gx, dl * w)                                         # one fp32 product per element: exact
    _close(gw, (dl.double().cpu() * x.double().cpu()).sum(0), tol=1e-5 * (1 + B ** 0.5 * 0.05))
    gx2, gw2 = ops.units1_backward(dl.reshape(B), w.reshape(N), x, want_gx=False)
    assert gx2 is None and torch.equal(gw2, gw)
    e = ops.units1_backward(dl[:0], w, x[:0])
    assert e[0].shape == (0, N) and float(e[1].abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.units1_backward(dl, w[:, :N - 1] if N > 1 else torch.zeros(1, 2).cuda(), x)


@pytest.mark.parametrize("shape,l1,l2", [((1,), 0.0, 0.0), ((1000, 3), 0.01, 0.05), ((257,), 0.5, 0.0)])
def test_dense_ftrl_step_matches_the_torch_formulation(built_lib, shape, l1, l2):
    """autograd.Ftrl on a dense CUDA variable (dir_ftrl_dense_f32: one pass) against the same optimiser's torch-op path on the CPU
    ([TF-upstream] tf.train.FtrlOptimizer's rule, deepFM.py:58), five steps, including weights that l1 holds at zero."""
    from dir_amd.autograd import Ftrl
    g = torch.Generator().manual_seed(len(shape) + int(l1 * 100))
    w0 = torch.randn(shape, generator=g) * 0.1
    a = torch.nn.Parameter(w0.clone().cuda())
    b = torch.nn.Parameter(w0.clone())
    oa, ob = Ftrl([a], lr=0.2, l1=l1, l2=l2), Ftrl([b], lr=0.2, l1=l1, l2=l2)
    for _ in range(5):
        grad = torch.randn(shape, generator=g) * 0.3
        a.grad, b.grad = grad.cuda(), grad.clone()
        oa.step()
        ob.step()
        _close(a, b, tol=2e-6)
    _close(oa.state[a]["accum"], ob.state[b]["accum"], tol=2e-6)
    _close(oa.state[a]["linear"], ob.state[b]["linear"], tol=2e-6)
    if l1 >= 0.5:
        assert float((b == 0).float().mean()) > 0.2 and torch.equal(a.detach().cpu() == 0, b.detach() == 0)


def test_dense_adagrad_step_matches_torch_adagrad(built_lib):
    """autograd.Adagrad (dir_adagrad_dense_f32 per dense CUDA variable) against torch.optim.Adagrad on the CPU over five steps: weights
    and accumulators; a sparse gradient and a weight_decay group fall back to the library's step."""
    from dir_amd.autograd import Adagrad
    g = torch.Generator().manual_seed(11)
    shapes = [(400, 416), (400,), (1, 400), (1,)]
    w0 = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    pa = [torch.nn.Parameter(w.clone().cuda()) for w in w0]
    pb = [torch.nn.Parameter(w.clone()) for w in w0]
    oa = Adagrad(pa, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    ob = torch.optim.Adagrad(pb, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    for it in range(5):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g) * 0.2
            a.grad, b.grad = gr.cuda(), gr.clone()
        if it == 3:
            pa[1].grad = pb[1].grad = None                       # a variable without a gradient is skipped
        oa.step()
        ob.step()
        for a, b in zip(pa, pb):
            _close(a, b, tol=2e-6)
    for a, b in zip(pa, pb):
        _close(oa.state[a]["sum"], ob.state[b]["sum"], tol=2e-6)
        assert float(oa.state[a]["step"]) == float(ob.state[b]["step"])
    # fallbacks: weight decay, a sparse gradient
    e1, e2 = torch.nn.Parameter(torch.zeros(10, 4).cuda()), torch.nn.Parameter(torch.zeros(10, 4))
    d1, d2 = torch.nn.Parameter(torch.ones(5).cuda()), torch.nn.Parameter(torch.ones(5))
    o1 = Adagrad([{"params": [e1]}, {"params": [d1], "weight_decay": 0.1}], lr=0.1)
    o2 = torch.optim.Adagrad([{"params": [e2]}, {"params": [d2], "weight_decay": 0.1}], lr=0.1)
    idx, val = torch.tensor([[1, 7]]), torch.ones(2, 4)
    e1.grad, e2.grad = torch.sparse_coo_tensor(idx.cuda(), val.cuda(), (10, 4)), torch.sparse_coo_tensor(idx, val, (10, 4))
    d1.grad, d2.grad = torch.full((5,), 0.5).cuda(), torch.full((5,), 0.5)
    o1.step()
    o2.step()
    _close(e1, e2, tol=2e-6)
    _close(d1, d2, tol=2e-6)


@pytest.mark.parametrize("B,m,D,H", [(64, 26, 16, 128), (300, 26, 16, 128), (33, 40, 8, 70), (17, 1, 16, 16), (129, 7, 32, 200), (4097, 5, 8, 130),
                                     (50, 28, 16, 64)])
def test_cin_dw_first_layer_symmetric_kernel(built_lib, B, m, D, H):
    """dir_cin_dw_sym_bf16x3_f32 (first layer: xk is x0, the unordered field pairs are the GEMM's columns) against the double-accumulating
    oracle at the bar of the other weight-gradient kernels, against the fp32-MFMA kernel, symmetric bit for bit, reruns bitwise equal,
    accumulate form; one / two / three pair blocks (m = 26 / 28 / 40), several h blocks, rows off the 32-row step."""
    from dir_amd import ops
    from oracle import oracle as O
    rng = np.random.default_rng(B * 3 + m)
    x0n = (rng.standard_normal((B, m, D)) * 0.5).astype(np.float32)
    Gn = (rng.standard_normal((B, H, D)) * 0.5).astype(np.float32)
    Wn = np.zeros((H, m * m), np.float32)
    ref_dW, _, _ = O.cin_backward(x0n, x0n, Wn, Gn)
    x0, G = torch.from_numpy(x0n).cuda(), torch.from_numpy(Gn).cuda()
    dW = ops.cin_dw(x0, x0, G, arith="bf16x3_sym")
    mag = np.sqrt(B * D) * 0.125 + 1.0
    err = np.abs(dW.cpu().double().numpy() - ref_dW) / (mag + np.abs(ref_dW))
    assert err.max() <= 1e-5, "sym dW max scaled err %.3e" % err.max()
    d3 = dW.view(H, m, m)
    assert torch.equal(d3, d3.transpose(1, 2))                                   # both halves come from one sum
    f32 = ops.cin_dw(x0, x0, G, arith="f32")
    assert float((dW - f32).abs().max()) <= 2e-5 * mag * (1 + float(f32.abs().max()))
    assert torch.equal(ops.cin_dw(x0, x0, G), dW)                                # "auto" on a first layer is this kernel
    assert torch.equal(ops.cin_dw(x0, x0, G, arith="bf16x3_sym"), dW)
    acc = ops.cin_dw(x0, x0, G, dW=dW.clone(), accumulate=True, arith="bf16x3_sym")
    assert torch.allclose(acc, 2 * dW, rtol=1e-6, atol=1e-6)
    # fp16 x 2 (dir_cin_dw_sym_f16x2_f32): "auto" with the tensor's maximum given (the forward-form contraction's kernel leaves it) -- same bar,
    # symmetric, reproducible, and a 2^-30 times smaller G gives the same bits times 2^-30
    if ops.CIN_BWD_SPLIT == "f16x2":
        bits = torch.tensor([np.float32(np.abs(Gn).max()).view(np.int32)], dtype=torch.int32, device="cuda")
        hW = ops.cin_dw(x0, x0, G, g_absmax_bits=bits)
        err = np.abs(hW.cpu().double().numpy() - ref_dW) / (mag + np.abs(ref_dW))
        assert err.max() <= 1e-5, "f16x2 sym dW max scaled err %.3e" % err.max()
        h3 = hW.view(H, m, m)
        assert torch.equal(h3, h3.transpose(1, 2)) and torch.equal(ops.cin_dw(x0, x0, G, g_absmax_bits=bits), hW) and not torch.equal(hW, dW)
        small = torch.tensor([np.float32(np.abs(Gn).max() * 2.0 ** -30).view(np.int32)], dtype=torch.int32, device="cuda")
        assert torch.equal(ops.cin_dw(x0, x0, G * 2.0 ** -30, g_absmax_bits=small), hW * 2.0 ** -30)
        if m >= 8 and ops.cin_bf16x3_covers(m, D):               # the contraction's by-product IS that maximum
            gb = []
            Ws_ = torch.zeros((m, H * m), device="cuda")
            ops.cin_layer(x0, G, Ws_, grad_operand=True, g_bits_out=gb)
            if gb:
                assert int(gb[0]) == int(bits)
    with pytest.raises(ValueError):
        ops.cin_dw(x0, x0.clone(), G, arith="bf16x3_sym")                        # xk must BE x0
    e = ops.cin_dw(x0[:0], x0[:0], G[:0], arith="bf16x3_sym") if False else None  # (an empty batch has no storage to alias: covered by the C entry below)
    z = torch.full((H, m * m), 7.0, device="cuda")
    lib = __import__("dir_amd._lib", fromlist=["load"]).load()
    assert lib.dir_cin_dw_sym_bf16x3_f32(None, None, m, H, D, 0, 0, z.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert float(z.abs().max()) == 0.0


@pytest.mark.parametrize("B,m,D,Hs", [(37, 7, 8, (12, 9)), (300, 26, 16, (128, 128, 128)), (65, 5, 4, (20, 33)), (129, 12, 16, (40, 64, 16)), (50, 3, 32, (8,))])
def test_cin_stack_node_matches_float64_and_the_per_layer_nodes(built_lib, B, m, D, Hs):
    """autograd.CinStack (the whole CIN stack as one node: pooled gradients added in the data-gradient kernels' epilogues, dx0 accumulated by
    dir_sum_partials_f32) against float64 autograd of the definition and against the per-layer nodes (autograd.CinLayer)."""
    from dir_amd import autograd as ag
    g = torch.Generator().manual_seed(B + m)
    x0 = torch.randn(B, m, D, generator=g) * 0.5
    Ws, hp = [], m
    for h in Hs:
        Ws.append(torch.randn(h, hp * m, generator=g) / (hp * m) ** 0.5)
        hp = h
    head = torch.randn(sum(Hs), generator=g)

    x64 = x0.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in Ws]
    xk, outs = x64, []
    for w in w64:
        xk = torch.einsum("hij,bid,bjd->bhd", w.view(w.shape[0], xk.shape[1], m), xk, x64)
        outs.append(xk.sum(2))
    l64 = (torch.cat(outs, 1) @ head.double()).square().sum()
    l64.backward()

    def run(stack):
        x = x0.cuda().requires_grad_(True)
        ws = [w.cuda().requires_grad_(True) for w in Ws]
        if stack:
            pooled = ag.cin_stack(x, ws)
        else:
            xk, outs = x, []
            for w in ws:
                xk, p = ag.cin_layer(x, xk, w)
                outs.append(p)
            pooled = torch.cat(outs, 1)
        loss = (pooled @ head.cuda()).square().sum()
        loss.backward()
        return loss.detach(), pooled.detach(), x.grad, [w.grad for w in ws]

    ls, ps, gxs, gws = run(True)
    ll, pl, gxl, gwl = run(False)
    _close(ls, l64, tol=1e-5)
    _close(ps, pl, tol=1e-5)                                            # (the stack's last layer runs in its pooled form: another summation order)
    sx = float(x64.grad.abs().max())
    _close(gxs / sx, x64.grad / sx, tol=2e-5)
    _close(gxs / sx, gxl / sx, tol=2e-5)
    for a, b, r in zip(gws, gwl, w64):
        sw = float(r.grad.abs().max())
        _close(a / sw, r.grad / sw, tol=2e-5)
        _close(a / sw, b / sw, tol=2e-5)
    ls2, _, gxs2, gws2 = run(True)                                      # bitwise reproducible
    assert torch.equal(gxs2, gxs) and all(torch.equal(a, b) for a, b in zip(gws2, gws))


def _deepfm_for_eval_train_eval(batch_norm):
    from dir_amd.deepfm import DeepFM
    from dir_amd import feature_column as fc
    torch.manual_seed(11)
    F, K, V = 26, 16, 400
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
    return DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[400, 400],
                  fm_embedding_size=K, batch_norm=batch_norm).cuda(), F, V


@pytest.mark.parametrize("batch_norm,packed_rows", [(False, False), (True, False), (False, True)])
def test_eval_train_eval_sees_the_trained_weights(built_lib, batch_norm, packed_rows):
    """the inference caches (DeepFM's packed serving rows, tower / dense bf16x3 images, padded weight copies, folded batch
    norm) key on tensor._version; the HIP optimisers and the training batch norm write through raw pointers.  eval -> train -> eval in one
    process (the reference's train_and_evaluate): the second eval must equal the layer-by-layer grad-mode forward of the TRAINED model,
    not the first eval's cached images."""
    from dir_amd import autograd as ag, ops
    model, F, V = _deepfm_for_eval_train_eval(batch_norm)
    model.fused_sparse_adagrad(lr=0.05, packed=packed_rows)
    model.fused_sparse_ftrl(lr=0.2)
    skip = {id(p) for p in model.linear_weights} | {id(p) for p in model.embedding_weights} | {id(model.linear_bias)}
    opt_d = ag.Adagrad([p for p in model.parameters() if id(p) not in skip], lr=0.05, initial_accumulator_value=0.1)
    opt_l = ag.Ftrl([model.linear_bias], lr=0.2)
    gen = torch.Generator(device="cuda").manual_seed(3)
    B = 8192                                    # a batch the fused tower / packed rows cover
    ids = torch.randint(0, V, (B, F), generator=gen, device="cuda")
    feats = {"C%d" % i: ids[:, i].contiguous() for i in range(F)}
    y = (torch.rand((B, 1), generator=gen, device="cuda") < 0.3).float()

    def eval_fused():
        model.eval()
        with torch.no_grad():
            return model(feats).clone()

    def eval_plain():                           # the differentiable layer-by-layer forward: reads the parameters themselves
        model.eval()
        return model(feats).detach().clone()

    e0 = eval_fused()
    assert float((e0 - eval_plain()).abs().max()) <= 2e-5 * (1 + float(e0.abs().max()))
    vers0 = [p._version for p in model.parameters()]
    model.train()
    for _ in range(3):
        opt_d.zero_grad(set_to_none=True)
        opt_l.zero_grad(set_to_none=True)
        torch.nn.functional.binary_cross_entropy_with_logits(model(feats), y).backward()
        opt_d.step()
        opt_l.step()
    assert all(p._version > v for p, v in zip(model.parameters(), vers0)), "a HIP update left a parameter's version counter where it was"
    e1, p1 = eval_fused(), eval_plain()
    assert float((p1 - e0).abs().max()) > 1e-3, "training did not move the logits: the test would pass vacuously"
    err = float(((e1 - p1).abs() / (1 + p1.abs())).max())
    assert err <= 2e-5, "inference after training ran on stale cached weights: %.3e" % err
    if batch_norm:                              # the moving statistics are written by dir_bn_train_stats_f32 through detached pointers
        assert all(b.moving_mean._version > 0 and b.moving_variance._version > 0 for b in model.bns)
    ops.invalidate_caches()
    assert torch.equal(eval_fused(), e1)        # a forced rebuild of the images gives the same bits: they were current


def test_train_step_adam_with_multihot_columns_still_trains_their_tables(built_lib):
    """TrainStep under Adam hands the embedding tables to the HIP sparse Adam, whose sink only fires for one-hot
    batches.  A multi-hot (ragged) column's table gets its gradient as sparse .grad instead: it must take the same tf.train.AdamOptimizer
    step (same m / v, all rows), its .grad must not accumulate, and the result must equal the DIR_TRAIN_HIP_ADAM=0 path."""
    import os
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd import feature_column as fc

    def build():
        torch.manual_seed(9)
        cols = [fc.embedding_column(fc.categorical_column_with_identity("C%02d" % i, 200), 16, combiner="mean") for i in range(4)]
        cols += [fc.numeric_column("I00")]
        return DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[32], batch_norm=False, optimizer="Adam",
                                optimizer_spec={"epsilon": 1e-4}, learning_rate_spec={"learning_rate": 0.01}).cuda()

    gen = torch.Generator(device="cuda").manual_seed(4)
    B = 512
    lens = torch.randint(0, 4, (B,), generator=gen, device="cuda")
    offs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), lens.cumsum(0)])
    vals = torch.randint(0, 200, (int(offs[-1]),), generator=gen, device="cuda")
    onehot = {"C%02d" % i: torch.randint(0, 200, (B,), generator=gen, device="cuda") for i in range(4)}
    ragged = dict(onehot)
    for i in range(4):
        ragged["C%02d" % i] = fc.Ragged(vals, offs)      # every embedding column multi-hot: the group's lookups take the CSR path
    num = {"I00": torch.rand((B,), generator=gen, device="cuda")}
    y = (torch.rand((B, 1), generator=gen, device="cuda") < 0.3).float()
    batches = [dict(onehot, **num), dict(ragged, **num), dict(onehot, **num)]

    def run(hip):
        os.environ["DIR_TRAIN_HIP_ADAM"] = "1" if hip else "0"
        try:
            model = build()
            op = model.train_step()
            assert bool(op.sparse_adam) == hip
            for f in batches:
                op(torch.nn.functional.binary_cross_entropy_with_logits(model(f), y))
            tabs = list(model.input_layer.embedding_weights)
            assert all(t.grad is None or not hip for t in tabs), "an owned table kept a .grad"
            return [p.detach().clone() for p in model.parameters()]
        finally:
            del os.environ["DIR_TRAIN_HIP_ADAM"]

    a, b = run(True), run(False)
    for x, z in zip(a, b):
        assert float((x - z).abs().max()) <= 1e-5


def test_deepfm_training_step_replays_from_a_hip_graph(built_lib):
    """one whole DeepFM training step (forward, loss, backward with the fused sorted Adagrad / FTRL inside, the HIP dense
    Adagrad / FTRL steps) captured in a torch.cuda.CUDAGraph and replayed: parameters bitwise equal to an eager twin after every step,
    also after the twin ran 70 eager steps in between (what made the round-3 attempt fault: rocPRIM's memset nodes, NOTES R4.3)."""
    from dir_amd import autograd as ag, feature_column as fc
    from dir_amd.deepfm import DeepFM
    B, F, K, V = 8192, 26, 16, 30000

    def build():
        torch.manual_seed(7)
        cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
        m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[400, 400],
                   fm_embedding_size=K).cuda()
        m.fused_sparse_adagrad(lr=0.01, packed=True)
        m.fused_sparse_ftrl(lr=0.2)
        skip = {id(p) for p in m.linear_weights} | {id(p) for p in m.embedding_weights} | {id(m.linear_bias)}
        od = ag.Adagrad([p for p in m.parameters() if id(p) not in skip], lr=0.01, initial_accumulator_value=0.1)
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

    gen = torch.Generator(device="cuda").manual_seed(3)
    batches = [torch.randint(0, V, (B, F), generator=gen, device="cuda") for _ in range(6)]
    labels = [(torch.rand((B, 1), generator=gen, device="cuda") < 0.25).float() for _ in range(6)]
    ma, oda, ola = build()
    mb, odb, olb = build()
    ids_s, y_s = batches[0].clone(), labels[0].clone()
    feats_s = {"C%d" % f: ids_s[:, f] for f in range(F)}
    feats = lambda i: {"C%d" % f: batches[i][:, f] for f in range(F)}      # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(3):
            ids_s.copy_(batches[i]); y_s.copy_(labels[i])
            step(mb, odb, olb, feats_s, y_s)
    torch.cuda.current_stream().wait_stream(s)
    for i in range(3):
        step(ma, oda, ola, feats(i), labels[i])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss_s = step(mb, odb, olb, feats_s, y_s)
    for i in (3, 4, 5):
        ids_s.copy_(batches[i]); y_s.copy_(labels[i])
        g.replay()
        la = step(ma, oda, ola, feats(i), labels[i])
        torch.cuda.synchronize()
        assert float(la) == float(loss_s)
        assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters())), "replayed step %d differs from eager" % i
    # the twin trains on alone for 70 eager steps (its own sorts, fills, allocations); the graph must still replay afterwards
    mc, odc, olc = build()
    for i in range(70):
        step(mc, odc, olc, feats(i % 6), labels[i % 6])
    ids_s.copy_(batches[0]); y_s.copy_(labels[0])
    g.replay()
    step(ma, oda, ola, feats(0), labels[0])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters()))


def test_captured_step_keeps_caches_honest(built_lib):
    """(a) graph replays update weights, tables and batch-norm statistics through raw pointers -- ops.CapturedStep bumps
    the version counters after every replay, so an eager EVAL after the replays sees the trained weights (serving rows, weight images and
    folded batch norms are rebuilt); (b) a capture taken right after an eager eval forward (every per-version cache holds a VALID entry at
    capture time) still packs its weight images inside the graph: the replays equal eager steps bit for bit instead of training against
    the images of the capture-time weights."""
    from dir_amd import autograd as ag, feature_column as fc, ops
    from dir_amd.deepfm import DeepFM
    B, F, K, V = 8192, 26, 16, 20000

    def build():
        torch.manual_seed(11)
        cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
        m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[400, 400],
                   fm_embedding_size=K, batch_norm=True).cuda()
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

    def evaluate(m, feats):
        m.eval()
        with torch.no_grad():
            out = m(feats).clone()
        m.train()
        return out

    gen = torch.Generator(device="cuda").manual_seed(5)
    batches = [torch.randint(0, V, (B, F), generator=gen, device="cuda") for _ in range(5)]
    labels = [(torch.rand((B, 1), generator=gen, device="cuda") < 0.25).float() for _ in range(5)]
    feats = lambda i: {"C%d" % f: batches[i][:, f] for f in range(F)}      # noqa: E731
    ma, oda, ola = build()          # eager twin
    mb, odb, olb = build()          # captured
    ids_s, y_s = batches[0].clone(), labels[0].clone()
    feats_s = {"C%d" % f: ids_s[:, f] for f in range(F)}
    # the constructor's warm-up steps are real steps: give the twin the same three
    cap = ops.CapturedStep(lambda: step(mb, odb, olb, feats_s, y_s), written=ops.written_of(mb), warmup=3)
    for _ in range(3):
        step(ma, oda, ola, feats(0), labels[0])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters()))
    e0 = evaluate(mb, feats(4))                                  # builds serving rows / images / folded batch norms of the CURRENT weights
    assert torch.equal(e0, evaluate(ma, feats(4)))
    for i in (1, 2, 3):
        ids_s.copy_(batches[i]); y_s.copy_(labels[i])
        cap.replay()
        step(ma, oda, ola, feats(i), labels[i])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters())), "replays differ from eager steps"
    assert all(torch.equal(x, y) for x, y in zip(ma.buffers(), mb.buffers())), "batch-norm statistics differ"
    e1b, e1a = evaluate(mb, feats(4)), evaluate(ma, feats(4))    # (a): the eval after the replays sees the trained weights
    assert torch.equal(e1b, e1a) and not torch.equal(e1b, e0)
    # (b): capture AFTER an eager eval forward, with no update in between -- every cache entry is valid when the capture starts
    mc, odc, olc = build()
    for _ in range(2):
        step(mc, odc, olc, feats(0), labels[0])
    evaluate(mc, feats(4))
    mc.train()
    # one hidden-layer image by hand as well: a hit at capture time
    ops.dense_bf3_image(mc.hidden[0].weight.detach(), "f16x2")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        step(mc, odc, olc, feats_s, y_s)
    md, odd, old_ = build()
    for _ in range(2):
        step(md, odd, old_, feats(0), labels[0])
    for i in (1, 2, 3, 4):
        ids_s.copy_(batches[i]); y_s.copy_(labels[i])
        g.replay()
        step(md, odd, old_, feats(i), labels[i])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(mc.parameters(), md.parameters())), "a graph captured behind valid caches trained against stale images"


@pytest.mark.parametrize("B", [300, 6144])
def test_dcn_training_step_advances_the_moving_statistics_once(built_lib, monkeypatch, B):
    """With the PRODUCT's dense.MIN_ROWS (6144; the suite's environment sets 1) a batch below it has no fused last layer, and forward() used
    to run the hidden layers under it a second time through deep_architecture: two launches of dir_bn_train_stats_f32 per batch norm and
    step, the moving statistics advanced twice.  One launch per batch norm, and moving = moving * momentum + batch * (1 - momentum) once,
    on both sides of the threshold."""
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd import feature_column as fc
    from dir_amd import dense as D, _lib
    monkeypatch.setattr(D, "MIN_ROWS", 6144)
    lib = _lib.load()
    calls = []
    real = lib.dir_bn_train_stats_f32
    monkeypatch.setattr(lib, "dir_bn_train_stats_f32", lambda *a: (calls.append(1), real(*a))[1])
    g = torch.Generator().manual_seed(B)
    F, K, V = 4, 8, 50
    cols = [fc.embedding_column(fc.categorical_column_with_identity("C%d" % i, V), K) for i in range(F)] + [fc.numeric_column("x")]
    dcn = DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[32, 32, 16], batch_norm=True).cuda().train()
    feats = {"C%d" % i: torch.randint(0, V, (B,), generator=g).cuda() for i in range(F)}
    feats["x"] = torch.rand(B, generator=g).cuda()
    with torch.no_grad():
        for bn in dcn.bns:
            bn.moving_mean.copy_(torch.randn(bn.moving_mean.shape, generator=g) * 0.2)
    before = [bn.moving_mean.double().clone() for bn in dcn.bns]
    dcn(feats).sum().backward()
    assert len(calls) == len(dcn.bns) == 2
    # the first batch norm's batch mean in float64, from the module's own input layer and first layer weights
    with torch.no_grad():
        x0 = dcn.input_layer(feats).double()
        y = torch.relu(x0 @ dcn.hidden[0].weight.double().t() + dcn.hidden[0].bias.double())
    m = dcn.bns[0].momentum
    want = before[0] * m + y.mean(dim=0) * (1 - m)
    assert float((dcn.bns[0].moving_mean.double() - want).abs().max()) <= 1e-5 * (1 + float(want.abs().max()))
    twice = want * m + y.mean(dim=0) * (1 - m)
    assert float((twice - want).abs().max()) > 1e-4                                # (the bar tells one update from two)
