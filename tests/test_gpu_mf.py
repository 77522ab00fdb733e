"""The matrix-factorisation family on the GPU (csrc/mf.hip, dir_amd.mf): the fused score and its backward against the float64 stand-in
(tests/mf_standin.py) at the project's bar, the negative sampler bit for bit against the stand-in's Philox draws, the models against their
CPU formulation, one fused sparse Adagrad step against float64, the link to metrics.GroupedMetrics and a captured training step."""
import copy

import numpy as np
import pytest
import torch

from tests import mf_standin as S
from tests import rank_metrics_standin as RS

pytestmark = pytest.mark.gpu

U, I = 37, 29                   # small vocabularies: every batch holds duplicate users and items
KS = (4, 12, 16, 20, 64, 100, 256)
CS = (1, 2, 3, 5, 100, 101)
BAR = 1e-5


def _dev():
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _err(got, ref):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref) / (1 + np.abs(ref))).max()) if got.size else 0.0


def _close(got, ref, what=""):
    e = _err(got, ref)
    print("%s max scaled err %.3e" % (what, e))
    assert e <= BAR, "%s: max scaled err %.3e" % (what, e)


def _tables(K, seed=0):
    rng = np.random.default_rng(1000 + K + seed)
    f = lambda *s: (rng.standard_normal(s) * 0.5).astype(np.float32)      # noqa: E731
    return f(U, K), f(I, K), f(U), f(I), np.array([0.375], np.float32)


def _ids(rng, B, C):
    ids = np.concatenate([rng.integers(0, U, (B, 1)), rng.integers(0, I, (B, C))], 1).astype(np.int64)
    ids[0, 0], ids[-1, 0], ids[0, 1], ids[-1, -1] = 0, U - 1, 0, I - 1      # both ends of both vocabularies
    return ids


# ---- score ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_score_vs_standin(K):
    from dir_amd import ops
    P, Q, bu, bi, b0 = _tables(K)
    tP, tQ, tbu, tbi, tb0 = T(P), T(Q), T(bu), T(bi), T(b0)
    rng = np.random.default_rng(K)
    for B in (1, 63, 64, 65, 257):
        for C in CS:
            ids = _ids(rng, B, C)
            tid = T(ids)
            dot = S.score(P, Q, ids)
            bias = bu.astype(np.float64)[ids[:, 0]][:, None] + bi.astype(np.float64)[ids[:, 1:]]
            what = "K=%d B=%d C=%d" % (K, B, C)
            full = ops.mf_score(tP, tQ, tid, tbu, tbi, tb0)
            assert full.shape == (B, C) and full.dtype == torch.float32
            _close(full, dot + (bias + np.float64(b0[0])), what + " bu bi b0")
            _close(ops.mf_score(tP, tQ, tid, tbu, tbi), dot + bias, what + " bu bi")
            _close(ops.mf_score(tP, tQ, tid), dot, what + " plain")
            _close(ops.mf_score(tP, tQ, tid, b0=tb0), dot + np.float64(b0[0]), what + " b0")
            again = ops.mf_score(tP, tQ, tid, tbu, tbi, tb0)
            assert torch.equal(full.view(torch.int32), again.view(torch.int32)), what + ": a second call differs in bits"
            out = torch.full((B, C), float("nan"), device=_dev())
            assert ops.mf_score(tP, tQ, tid, tbu, tbi, tb0, out=out) is out and torch.equal(out.view(torch.int32), full.view(torch.int32))


@pytest.mark.parametrize("K,B,C", [(16, 65, 3), (20, 64, 101), (256, 63, 5), (4, 257, 1)])
def test_score_strided_ids(K, B, C):
    from dir_amd import ops
    P, Q, bu, bi, b0 = _tables(K, seed=1)
    rng = np.random.default_rng(7 * K + C)
    ids = _ids(rng, B, C)
    want = S.score(P, Q, ids, bu, bi, b0)
    wide = np.full((B, C + 6), -12345, np.int64)                 # a column slice of a wider matrix: row stride C + 6
    wide[:, 2:3 + C] = ids
    sl = T(wide)[:, 2:3 + C]
    assert not sl.is_contiguous() and sl.stride() == (C + 6, 1)
    tr = T(ids.T.copy()).t()                                      # field-major storage handed over transposed: strides (1, B)
    assert tr.shape == (B, 1 + C) and (B == 1 or tr.stride() == (1, B))
    args = (T(P), T(Q))
    kw = dict(bu=T(bu), bi=T(bi), b0=T(b0))
    base = ops.mf_score(*args, T(ids), **kw)
    _close(base, want, "contiguous")
    for name, view in (("slice", sl), ("transposed", tr)):
        got = ops.mf_score(*args, view, **kw)
        assert torch.equal(got.view(torch.int32), base.view(torch.int32)), name
        g1, b1 = ops.mf_score_backward(*args, view, base, kw["bu"], kw["bi"], l2=0.1)
        g0, b0_ = ops.mf_score_backward(*args, T(ids), base, kw["bu"], kw["bi"], l2=0.1)
        assert torch.equal(g1.view(torch.int32), g0.view(torch.int32)) and torch.equal(b1.view(torch.int32), b0_.view(torch.int32)), name


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_backward_vs_standin(K):
    from dir_amd import ops
    P, Q, bu, bi, _ = _tables(K, seed=2)
    tP, tQ, tbu, tbi = T(P), T(Q), T(bu), T(bi)
    rng = np.random.default_rng(50 + K)
    for B in (1, 65, 257):
        for C in CS:
            ids = _ids(rng, B, C)
            dl = rng.standard_normal((B, C)).astype(np.float32)
            for l2 in (0.0, 0.1):
                what = "K=%d B=%d C=%d l2=%g" % (K, B, C, l2)
                wg, wb = S.score_grads(P, Q, ids, dl, bu, bi, l2=np.float64(np.float32(l2)))
                grad, gbias = ops.mf_score_backward(tP, tQ, T(ids), T(dl), tbu, tbi, l2=l2)
                assert grad.shape == (B, (1 + C) * K) and gbias.shape == (B, 1 + C)
                _close(grad, wg, what + " grad")
                _close(gbias, wb, what + " gbias")
            wg, wb = S.score_grads(P, Q, ids, dl, None, None, l2=np.float64(np.float32(0.1)))      # no intercepts: gbias = the plain sums
            grad, gbias = ops.mf_score_backward(tP, tQ, T(ids), T(dl), l2=0.1)
            _close(grad, wg, "no bias grad")
            _close(gbias, wb, "no bias gbias")


def test_backward_one_item_at_many_slots():
    from dir_amd import ops
    K, B, C = 16, 130, 7
    P, Q, bu, bi, _ = _tables(K, seed=3)
    rng = np.random.default_rng(99)
    ids = _ids(rng, B, C)
    ids[::2, 1:] = 11                                            # every slot of every other sample
    ids[1::2, 3] = 11                                            # and one slot of the rest
    dl = rng.standard_normal((B, C)).astype(np.float32)
    wg, wb = S.score_grads(P, Q, ids, dl, bu, bi, l2=np.float64(np.float32(0.1)))
    grad, gbias = ops.mf_score_backward(T(P), T(Q), T(ids), T(dl), T(bu), T(bi), l2=0.1)
    _close(grad, wg, "grad")
    _close(gbias, wb, "gbias")


@pytest.mark.parametrize("K,C,l2", [(16, 3, 0.0), (20, 5, 0.1), (64, 1, 0.1)])
def test_mf_score_autograd_sparse_grads(K, C, l2):
    from dir_amd import autograd as ag
    B = 65
    P, Q, bu, bi, b0 = _tables(K, seed=4)
    rng = np.random.default_rng(5)
    ids = _ids(rng, B, C)
    if C > 1:
        ids[:, 2] = ids[:, 1]                                    # an item at two slots of one sample
    dl = rng.standard_normal((B, C)).astype(np.float32)
    tp = [T(a).requires_grad_() for a in (P, Q, bu.reshape(-1, 1), bi.reshape(-1, 1), b0.reshape(()))]
    out = ag.mf_score(tp[0], tp[1], T(ids), tp[2], tp[3], tp[4], l2=l2)
    _close(out, S.score(P, Q, ids, bu, bi, b0), "forward")
    out.backward(T(dl))
    wg, wb = S.score_grads(P, Q, ids, dl, bu, bi, l2=np.float64(np.float32(l2)))
    for t in tp[:4]:                                             # coalesced: every row once, in ascending order (autograd's accumulation copies
        idx = t.grad._indices()[0].cpu().numpy()                 # a sparse gradient without its is_coalesced flag, so the indices are checked)
        assert t.grad.is_sparse and (np.diff(idx) > 0).all()
    _close(tp[0].grad.to_dense(), S.scatter_rows(ids[:, 0], wg[:, :K], U), "dP")
    _close(tp[1].grad.to_dense(), S.scatter_rows(ids[:, 1:].reshape(-1), wg[:, K:].reshape(B * C, K), I), "dQ")
    _close(tp[2].grad.to_dense(), S.scatter_rows(ids[:, 0], wb[:, :1], U), "dbu")
    _close(tp[3].grad.to_dense(), S.scatter_rows(ids[:, 1:].reshape(-1), wb[:, 1:].reshape(B * C, 1), I), "dbi")
    assert tp[4].grad.shape == tp[4].shape and _err(tp[4].grad.reshape(()), dl.astype(np.float64).sum()) <= BAR
    # without intercepts
    tq = [T(a).requires_grad_() for a in (P, Q)]
    ag.mf_score(tq[0], tq[1], T(ids), l2=l2).backward(T(dl))
    wg, _ = S.score_grads(P, Q, ids, dl, None, None, l2=np.float64(np.float32(l2)))
    _close(tq[0].grad.to_dense(), S.scatter_rows(ids[:, 0], wg[:, :K], U), "dP (no intercepts)")


# ---- sampler ----------------------------------------------------------------------------------------------------------------------------
N_ITEMS = 50


def _sampler_users():
    """user 0: nothing; 1 / 2 / 3: all but item 0 / 25 / 49; 4: one contiguous run; 5: items 0 and N - 1; 6: scattered"""
    every = np.arange(N_ITEMS)
    lists = [np.zeros(0, np.int64), every[every != 0], every[every != 25], every[every != N_ITEMS - 1], np.arange(10, 31),
             np.array([0, N_ITEMS - 1]), np.array([1, 2, 7, 8, 9, 30, 31, 48])]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return lists, offsets, np.concatenate(lists).astype(np.int64)


def _check_draws(out, users, lists, num_items):
    out = out.cpu().numpy()
    assert ((out >= 0) & (out < num_items)).all()
    for b, u in enumerate(users):
        assert not np.isin(out[b], lists[u]).any(), (b, u, out[b])


@pytest.mark.parametrize("n_neg", [1, 4, 7])
def test_sampler_bit_for_bit(n_neg):
    from dir_amd import ops
    lists, offsets, items = _sampler_users()
    ui = ops.UserItems(T(offsets), T(items), N_ITEMS)
    st = ops.DropoutState(seed=0x1234567890ABCDEF, device=_dev())
    rng = np.random.default_rng(n_neg)
    for B in (1, 64, 65, 1000):
        users = rng.integers(0, len(lists), B).astype(np.int64)
        users[:min(B, len(lists))] = np.arange(len(lists))[:min(B, len(lists))]
        got, status = ops.neg_sample(T(users), ui, n_neg, st, return_status=True)
        want, _ = S.neg_sample(users, offsets, items, N_ITEMS, n_neg, *st.get_state())
        assert got.shape == (B, n_neg) and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), want), "B=%d" % B
        assert int(status) == 0
        _check_draws(got, users, lists, N_ITEMS)
        for u, left in ((1, 0), (2, 25), (3, N_ITEMS - 1)):      # one item left: at the front, in the middle, at the end
            assert (got.cpu().numpy()[users == u] == left).all()


def test_sampler_counter_stream_and_state():
    from dir_amd import ops
    lists, offsets, items = _sampler_users()
    ui = ops.UserItems(T(offsets), T(items), N_ITEMS)
    st = ops.DropoutState(seed=77, device=_dev())
    users = np.array([0, 6, 5, 4, 0, 6, 0, 0], np.int64)
    first = (1 << 32) - 3                                        # the 8 x 4 draws cross the counter's high word
    got = ops.neg_sample(T(users), ui, 4, st, first=first)
    want, _ = S.neg_sample(users, offsets, items, N_ITEMS, 4, 77, 0, first=first)
    assert np.array_equal(got.cpu().numpy(), want)
    other = ops.neg_sample(T(users), ui, 4, st, stream_id=1, first=first)
    want1, _ = S.neg_sample(users, offsets, items, N_ITEMS, 4, 77, 0, stream_id=1, first=first)
    assert np.array_equal(other.cpu().numpy(), want1) and not np.array_equal(want, want1)
    out = torch.empty((8, 4), dtype=torch.int64, device=_dev())
    assert ops.neg_sample(T(users), ui, 4, st, first=first, out=out) is out and torch.equal(out, got)      # the same state: the same draws
    st.advance()
    nxt = ops.neg_sample(T(users), ui, 4, st, first=first)
    assert st.get_state() == (77, 1) and not torch.equal(nxt, got)
    assert np.array_equal(nxt.cpu().numpy(), S.neg_sample(users, offsets, items, N_ITEMS, 4, 77, 1, first=first)[0])
    st.set_state((77, 0))
    assert torch.equal(ops.neg_sample(T(users), ui, 4, st, first=first), got)
    _check_draws(nxt, users, lists, N_ITEMS)


def test_sampler_size_edges():
    from dir_amd import ops
    st = ops.DropoutState(seed=5, device=_dev())
    one = ops.UserItems(T(np.array([0, 0], np.int64)), T(np.zeros(0, np.int64)), 1)          # one item, no interaction: always item 0
    assert (ops.neg_sample(T(np.zeros(9, np.int64)), one, 3, st) == 0).all()
    big, pos = 1 << 40, np.array([0, 3, 1 << 20, (1 << 39) + 1, (1 << 40) - 1], np.int64)
    offsets = np.array([0, 5, 5], np.int64)
    ui = ops.UserItems(T(offsets), T(pos), big)
    users = np.array([0, 1] * 40, np.int64)
    got = ops.neg_sample(T(users), ui, 4, st)
    want, _ = S.neg_sample(users, offsets, pos, big, 4, 5, 0)
    assert np.array_equal(got.cpu().numpy(), want) and want.max() > (1 << 32)
    _check_draws(got, users, [pos, np.zeros(0, np.int64)], big)


def test_sampler_saturated_user_sets_status():
    from dir_amd import ops
    offsets, items = np.array([0, 2, 5, 5], np.int64), np.array([1, 3, 0, 1, 2], np.int64)
    with pytest.raises(ValueError, match="no negative is left"):
        ops.UserItems(T(offsets), T(items), 3)
    ui = ops.UserItems(T(offsets), T(items), 3, _check=False)   # user 1 holds all three items
    st = ops.DropoutState(seed=9, device=_dev())
    users = np.array([0, 1, 2, 1, 0], np.int64)
    got, status = ops.neg_sample(T(users), ui, 2, st, return_status=True)
    want, wstatus = S.neg_sample(users, offsets, items, 3, 2, 9, 0)
    assert wstatus == 1 and int(status) != 0
    assert np.array_equal(got.cpu().numpy(), want)
    assert (got.cpu().numpy()[users == 1] == -1).all() and (got.cpu().numpy()[users != 1] >= 0).all()


# ---- models -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["mse", "cross entropy"])
@pytest.mark.parametrize("intercepts", [True, False])
def test_biased_mf_device_matches_cpu(loss, intercepts):
    from dir_amd import feature_column as fc
    from dir_amd.mf import BiasedMF
    K, B = 16, 257
    cu, ci = fc.categorical_column_with_identity("user", U), fc.categorical_column_with_identity("item", I)
    cpu = BiasedMF(embedding_cols=[fc.embedding_column(cu, K), fc.embedding_column(ci, K)],
                   bias_cols=[fc.embedding_column(cu, 1), fc.embedding_column(ci, 1)], reg_pen=0.05, learning_rate=0.01, loss=loss,
                   intercepts=intercepts, is_implicit=True, weights="log_weight", weights_coef=0.75)
    if intercepts:
        with torch.no_grad():
            cpu.global_bias.fill_(0.25)
    gpu = copy.deepcopy(cpu).to(_dev())
    rng = np.random.default_rng(3)
    ids = _ids(rng, B, 1)
    ratings = rng.integers(1, 6, B).astype(np.float32)
    fcpu = {"user": torch.from_numpy(ids[:, 0]), "item": torch.from_numpy(ids[:, 1])}
    fgpu = {k: v.to(_dev()) for k, v in fcpu.items()}
    lc, lg = cpu(fcpu), gpu(fgpu)
    assert lg.is_cuda and lg.shape == (B, 1)
    _close(lg, lc.detach().numpy(), "logits")
    cost_c, cost_g = cpu.create_loss(fcpu, lc, torch.from_numpy(ratings)), gpu.create_loss(fgpu, lg, torch.from_numpy(ratings).to(_dev()))
    _close(cost_g, cost_c.detach().numpy(), "cost")
    pc, pg = cpu.predict(fcpu), gpu.predict(fgpu)
    assert set(pc) == set(pg)
    for k in pc:
        if k == "class_ids":
            sure = (lc.detach().abs() > 1e-4).reshape(-1)         # (a logit within rounding of 0 may fall on either side)
            assert torch.equal(pg[k].cpu()[sure], pc[k][sure])
        else:
            _close(pg[k], pc[k].numpy(), k)
    # the gradients: the HIP backward (with its l2 terms) against the CPU formulation's graph
    cost_c.backward()
    cost_g.backward()
    names = ["user_emb", "item_emb"] + (["user_bias", "item_bias", "global_bias"] if intercepts else [])
    for n in names:
        g = getattr(gpu, n).grad
        _close(g.to_dense() if g.is_sparse else g, getattr(cpu, n).grad.numpy(), "d " + n)


def test_bpr_fused_adagrad_step():
    from dir_amd.mf import BPR
    K, B, n_neg, lr, reg = 16, 64, 2, 0.05, 0.01
    torch.manual_seed(3)
    m = BPR(U, I, K, reg_pen=reg, n_neg=n_neg).to(_dev())
    rows_opt, bias_opt = m.fused_sparse_adagrad(lr)
    assert bias_opt is not None                                  # the sorted Adagrad step takes K = 1
    rng = np.random.default_rng(8)
    ids = np.concatenate([rng.integers(0, 20, (B, 1)), rng.integers(0, 15, (B, 1 + n_neg))], 1).astype(np.int64)      # rows 20.. / 15.. stay untouched
    ids[0, 1], ids[1, 2], ids[2, 3], ids[3, 1], ids[3, 2] = 5, 5, 5, 6, 6      # item 5: positive in one sample, negative in two others
    before = {n: getattr(m, n).detach().cpu().double().numpy().copy() for n in ("user_emb", "item_emb", "user_bias", "item_bias")}
    diff = m(T(ids[:, 0]), T(ids[:, 1]), T(ids[:, 2:]))
    loss = m.create_loss(diff)
    loss.backward()
    torch.cuda.synchronize()
    assert all(getattr(m, n).grad is None for n in before)      # the sinks took the gradients
    P, Q, bu, bi = before["user_emb"], before["item_emb"], before["user_bias"], before["item_bias"]
    s = S.score(P, Q, ids, bu, bi)
    d = s[:, :1] - s[:, 1:]
    _close(diff, d, "diff")
    _close(loss, np.log1p(np.exp(-d)).mean() + S.reg(P, Q, ids, reg, bu, bi), "loss")
    dd = -(1.0 / (1.0 + np.exp(d))) / d.size                     # d mean(-log sigmoid(d)) / d d
    dl = np.concatenate([dd.sum(1, keepdims=True), -dd], 1)
    wg, wb = S.score_grads(P, Q, ids, dl, bu, bi, l2=np.float64(np.float32(reg)))
    C = 1 + n_neg
    sums = {"user_emb": S.scatter_rows(ids[:, 0], wg[:, :K], U),
            "item_emb": S.scatter_rows(ids[:, 1:].reshape(-1), wg[:, K:].reshape(B * C, K), I),          # a row's slots summed first: ONE step
            "user_bias": S.scatter_rows(ids[:, 0], wb[:, :1], U),
            "item_bias": S.scatter_rows(ids[:, 1:].reshape(-1), wb[:, 1:].reshape(B * C, 1), I)}
    touched = {"user_emb": np.unique(ids[:, 0]), "item_emb": np.unique(ids[:, 1:])}
    touched["user_bias"], touched["item_bias"] = touched["user_emb"], touched["item_emb"]
    for n, g in sums.items():
        after = getattr(m, n).detach().cpu().double().numpy()
        rest = np.setdiff1d(np.arange(after.shape[0]), touched[n])
        assert rest.size and np.array_equal(after[rest], before[n][rest]), n + ": an untouched row moved"
        want = before[n].copy()
        t = touched[n]
        want[t] = before[n][t] - lr * g[t] / np.sqrt(0.1 + g[t] * g[t])
        _close(after, want, n)
        assert np.abs(after[t] - before[n][t]).max() > 1e-4, n + ": nothing moved"


def test_score_blocks_feed_grouped_metrics():
    from dir_amd.metrics import GroupedMetrics
    from dir_amd.mf import BPR
    blocks, C, NU, NI, K = 48, 100, 60, 500, 20
    torch.manual_seed(4)
    m = BPR(NU, NI, K).to(_dev())
    rng = np.random.default_rng(12)
    users = rng.integers(0, NU, blocks).astype(np.int64)
    items = np.stack([rng.permutation(NI)[:C] for _ in range(blocks)]).astype(np.int64)
    scores = m.score_blocks(T(users), T(items))
    assert scores.shape == (blocks, C) and not scores.requires_grad
    P, Q, bu, bi = [getattr(m, n).detach().cpu().numpy() for n in ("user_emb", "item_emb", "user_bias", "item_bias")]
    want = S.score(P, Q, np.concatenate([users[:, None], items], 1), bu, bi)
    _close(scores, want, "scores")
    got = GroupedMetrics(k=10, device=_dev()).update_blocks(scores.reshape(-1), block=C, positive_index=0).result()
    labels = np.zeros((blocks, C), np.float32)
    labels[:, 0] = 1.0
    st = RS.group_stats(want.astype(np.float32).reshape(-1), labels.reshape(-1), None, np.arange(blocks + 1) * C)
    ref = RS.aggregate(st, k=10)
    for k in ("hr@10", "ndcg@10", "mrr@10"):
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])
    assert got["ranking_groups"] == blocks


def test_bpr_captured_step_draws_fresh_negatives():
    from dir_amd import ops
    from dir_amd.mf import BPR
    K, B, n_neg, lr = 16, 128, 2, 0.05
    rng = np.random.default_rng(21)
    pu, pi = rng.integers(0, U, 300), rng.integers(0, I, 300)
    ui = ops.UserItems.from_pairs(T(pu), T(pi), U, I)
    offsets, items = ui.offsets.cpu().numpy(), ui.items.cpu().numpy()
    users, pos = T(pu[:B].astype(np.int64)), T(pi[:B].astype(np.int64))

    def build():
        torch.manual_seed(6)
        m = BPR(U, I, K, reg_pen=0.01, n_neg=n_neg, user_items=ui, seed=31).to(_dev())
        return m, m.fused_sparse_adagrad(lr)

    def step(m):
        loss = m.create_loss(m(users, pos))
        loss.backward()
        return loss

    ma, _ = build()                 # eager twin
    mb, _ = build()                 # captured
    cap = ops.CapturedStep(lambda: step(mb), written=ops.written_of(mb), warmup=2)
    for _ in range(2):              # the constructor's warm-up steps are real steps: the twin takes the same two
        step(ma)
    torch.cuda.synchronize()
    assert ma.sampler_rng.get_state() == mb.sampler_rng.get_state() == (31, 2)
    assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters()))
    ma.sampler_rng.set_state((31, 100))
    mb.sampler_rng.set_state((31, 100))
    drawn = []
    for _ in range(3):
        cap.replay()
        drawn.append(mb._last_ids[:, 2:].clone())
        step(ma)
    torch.cuda.synchronize()
    assert ma.sampler_rng.get_state() == mb.sampler_rng.get_state() == (31, 103)
    assert all(torch.equal(x, y) for x, y in zip(ma.parameters(), mb.parameters())), "replays differ from eager steps"
    for i, neg in enumerate(drawn):
        want, _ = S.neg_sample(pu[:B], offsets, items, I, n_neg, 31, 100 + i)
        assert np.array_equal(neg.cpu().numpy(), want), "replay %d" % i
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
