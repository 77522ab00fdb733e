"""shard.ShardedDINTrainer on the GPU: the DIN model over a row-sharded goods table, world 1 and two ranks on cuda:0 over gloo (the
harness of tests/test_gpu_shard_multiproc.py: exchanges staged through host memory).

predict: bit for bit the single-GPU din.DIN holding the full table on the same local batch -- sigmoid, PReLU and Dice (eval mode) units,
with de-duplicated and plain inference lookups.
step: both sides run the same forward and backward kernels (the sharded side through the received rows and the entries' positions), so the
comparison isolates the new path.  Dense gradients against the single-GPU model's at the bound tests/test_gpu_din_model.py holds DIN
training to (5e-5 scaled; the test prints whether they are in fact bitwise).  Table and accumulator: the single-GPU model's sparse table
gradient coalesced in float64 and pushed through the float64 Adagrad rule; bar 1e-5 scaled (tests/hot_rows_inputs.scaled).
World 2: ranks hold 64 / 32 of the 96 samples; compared against ONE single-process step over the concatenated batch (gradients ADD over
the ranks).  No Dice there: its batch statistics are per rank.

Shapes: K = 64, attention 80-40, T in {7, 50}, B = 96, vocabulary 300 (most rows repeat), lengths 0 and T included, padding ids inside the
valid length, a candidate of -1."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.hot_rows_inputs import scaled
from tests.test_gpu_shard_multiproc import _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, B = 300, 64, 96
LR, LR_DENSE, ACC0 = 0.05, 1e-3, 0.1
DENSE_TOL, SPARSE_TOL = 5e-5, 1e-5


def _model(att, dnn, seed=5):
    from dir_amd.din import DIN
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    m = DIN(item_vocab_size=V, embedding_dim=K, attention_hidden_units=(80, 40), attention_activation=att, dnn_hidden_units=(200, 80),
            dnn_activation_fn=dnn).cuda()
    with torch.no_grad():
        for mod in m.modules():
            if hasattr(mod, "alpha"):
                mod.alpha.copy_(torch.from_numpy(rng.uniform(-0.2, 0.6, mod.alpha.numel()).astype(np.float32)))
            if mod.__class__.__name__ == "Dice":
                mod.moving_mean.copy_(torch.from_numpy((rng.standard_normal(mod.moving_mean.numel()) * 0.3).astype(np.float32)))
                mod.moving_variance.copy_(torch.from_numpy(rng.uniform(0.2, 2.0, mod.moving_variance.numel()).astype(np.float32)))
        a = m.attention
        a.b1.normal_(0, 0.05); a.b2.normal_(0, 0.05); a.b3.fill_(0.02)
        for lin in list(m.hidden) + [m.logits_layer]:
            lin.bias.normal_(0, 0.05)
    return m


def _batch(T, seed, n=B):
    rng = np.random.default_rng(seed)
    hist = rng.integers(-1, V, size=(n, T)).astype(np.int64)          # -1: padding inside the valid length
    hl = rng.integers(0, T + 1, size=n).astype(np.int32)
    hl[0], hl[1], hl[n - 1] = 0, T, T
    cand = rng.integers(0, V, size=n).astype(np.int64)
    cand[2] = -1
    y = rng.integers(0, 2, size=(n, 1)).astype(np.float32)
    return hist, hl, cand, y


def _feats(hist, hl, cand, s=0, e=None):
    return {"hist": torch.from_numpy(hist[s:e]).cuda(), "hist_len": torch.from_numpy(hl[s:e]).cuda(), "cand": torch.from_numpy(cand[s:e]).cuda()}


def _dense(m):
    return [(n, p) for n, p in m.named_parameters() if n != "attention.table"]


def _reference_step(ref, feats, y, w0, acc0):
    """One single-GPU step of `ref` (a din.DIN in train mode) on the batch: -> its dense gradients {name: grad} and the float64 Adagrad
    result (w, acc) of its sparse table gradient, coalesced in float64, from the fp32 state (w0, acc0)."""
    for p in ref.parameters():
        p.grad = None
    loss = torch.nn.functional.binary_cross_entropy_with_logits(ref(feats), y, reduction="sum")
    loss.backward()
    g = ref.attention.table.grad
    G = torch.zeros((V, K), dtype=torch.float64, device="cuda")
    G.index_add_(0, g._indices()[0], g._values().double())
    touched = torch.zeros(V, dtype=torch.bool, device="cuda")
    touched[g._indices()[0]] = True
    acc = acc0.double().clone()
    w = w0.double().clone()
    acc[touched] += G[touched] ** 2
    w[touched] -= LR * G[touched] / acc[touched].sqrt()
    return {n: p.grad.detach().clone() for n, p in _dense(ref) if p.grad is not None}, w, acc, float(loss.detach())


def _check_dense(model, grads, what):
    worst, bitwise = 0.0, True
    for n, p in _dense(model):
        if n not in grads:
            assert p.grad is None, n
            continue
        err = scaled(p.grad.detach().cpu().numpy(), grads[n].cpu().numpy())
        worst = max(worst, err)
        bitwise = bitwise and torch.equal(p.grad.detach(), grads[n])
        assert err <= DENSE_TOL, "%s: dL/d%s %.3e" % (what, n, err)
    print("%s: dense gradients worst %.3e, bitwise %s" % (what, worst, bitwise))
    return worst, bitwise


def _check_shard(st, w, acc, what, lo=0, hi=V):
    ew = scaled(st.local_tables[0].cpu().numpy(), w[lo:hi].cpu().numpy())
    ea = scaled(st.optimizer.accums[0].cpu().numpy(), acc[lo:hi].cpu().numpy())
    print("%s: table %.3e accumulator %.3e of the float64 Adagrad step" % (what, ew, ea))
    assert ew <= SPARSE_TOL and ea <= SPARSE_TOL, "%s: table %.3e accumulator %.3e" % (what, ew, ea)
    return max(ew, ea)


@pytest.mark.parametrize("dedup", [True, False])
@pytest.mark.parametrize("T", [7, 50])
@pytest.mark.parametrize("att,dnn", [("sigmoid", "relu"), ("prelu", "prelu"), ("dice", "dice")])
def test_predict_world1_is_the_single_gpu_model_bit_for_bit(built_lib, att, dnn, T, dedup):
    from dir_amd.shard import ShardedDINTrainer
    m = _model(att, dnn).eval()
    hist, hl, cand, _ = _batch(T, 40 + T)
    feats = _feats(hist, hl, cand)
    with torch.no_grad():
        want = m(feats)
    st = ShardedDINTrainer.tables_from_model(m, dedup=dedup)
    tr = ShardedDINTrainer(m, st, LR, torch.optim.SGD([p for _, p in _dense(m)], lr=LR_DENSE))
    got = tr.predict(feats)
    again = tr.predict(feats)
    torch.cuda.synchronize()
    assert got.shape == (B, 1) and torch.equal(got, again)
    assert torch.equal(got, want), "predict differs from the single-GPU model: %.3e" % float((got - want).abs().max())


@pytest.mark.parametrize("T", [7, 50])
@pytest.mark.parametrize("att,dnn", [("sigmoid", "relu"), ("prelu", "prelu"), ("dice", "dice")])
def test_step_world1_against_the_single_gpu_step(built_lib, att, dnn, T):
    """Two steps with an inference predict in between; the reference restarts every step from the sharded side's fp32 state."""
    from dir_amd.shard import ShardedDINTrainer
    m = _model(att, dnn).train()
    ref = copy.deepcopy(m).train()
    st = ShardedDINTrainer.tables_from_model(m)
    tr = ShardedDINTrainer(m, st, LR, torch.optim.SGD([p for _, p in _dense(m)], lr=LR_DENSE), initial_accumulator_value=ACC0)
    ref_opt = torch.optim.SGD([p for _, p in _dense(ref)], lr=LR_DENSE)
    for step in range(2):
        hist, hl, cand, y = _batch(T, 60 + 10 * step + T)
        feats, yy = _feats(hist, hl, cand), torch.from_numpy(y).cuda()
        w0, acc0 = st.local_tables[0].clone(), st.optimizer.accums[0].clone()
        with torch.no_grad():
            ref.attention.table.copy_(w0)
        grads, w, acc, ref_loss = _reference_step(ref, feats, yy, w0, acc0)
        loss = tr.step(feats, yy)
        torch.cuda.synchronize()
        what = "%s/%s T=%d step %d" % (att, dnn, T, step)
        assert abs(float(loss) - ref_loss) <= 1e-4 * (1 + abs(ref_loss)), (float(loss), ref_loss)
        _check_dense(m, grads, what)
        _check_shard(st, w, acc, what)
        ref.attention.table.grad = None
        ref_opt.step()
        for (n, p), (_, q) in zip(_dense(m), _dense(ref)):
            assert scaled(p.detach().cpu().numpy(), q.detach().cpu().numpy()) <= DENSE_TOL, n
        if step == 0:
            with torch.no_grad():
                ref.attention.table.copy_(st.local_tables[0])
                want = ref.eval()(feats)
                ref.train()
            got = tr.predict(feats)                       # an inference lookup between two training steps
            assert m.training, "predict must leave the model in its mode"
            if att != "dice" and dnn != "dice":           # (the two models' Dice moving averages agree to rounding only)
                assert scaled(got.cpu().numpy(), want.cpu().numpy()) <= DENSE_TOL
    assert st._updates == 2


def test_step_world1_without_dedup_and_refusals(built_lib):
    from dir_amd import feature_column as fc
    from dir_amd.din import DIN
    from dir_amd.shard import ShardedDINTrainer
    m = _model("sigmoid", "relu").train()
    ref = copy.deepcopy(m).train()
    st = ShardedDINTrainer.tables_from_model(m, dedup=False)
    tr = ShardedDINTrainer(m, st, LR, torch.optim.SGD([p for _, p in _dense(m)], lr=LR_DENSE), dedup=False)
    hist, hl, cand, y = _batch(50, 91)
    feats, yy = _feats(hist, hl, cand), torch.from_numpy(y).cuda()
    w0, acc0 = st.local_tables[0].clone(), st.optimizer.accums[0].clone()
    grads, w, acc, _ = _reference_step(ref, feats, yy, w0, acc0)
    tr.step(feats, yy)
    _check_dense(m, grads, "dedup=False")
    _check_shard(st, w, acc, "dedup=False")
    cols = [fc.embedding_column(fc.categorical_column_with_identity("city", 20), 8)]
    bad = DIN(feature_columns=cols, item_vocab_size=V, embedding_dim=K).cuda()
    with pytest.raises(NotImplementedError, match="sparse gradient"):
        ShardedDINTrainer(bad, ShardedDINTrainer.tables_from_model(bad), LR, torch.optim.SGD([bad.logits_layer.weight], lr=LR_DENSE))


# ---- two ranks on cuda:0 ------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, att, dnn, T, q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        os.environ["DIR_SHARD_HOST_STAGED"] = "1"          # two ranks on ONE GPU: exchanges staged through host memory over gloo
        os.environ.setdefault("DIR_DENSE_MIN_ROWS", "1")
        import datetime
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        try:
            torch.cuda.set_device(0)
            import dir_amd  # noqa: F401
            from dir_amd.shard import ShardedDINTrainer, div_range
            m = _model(att, dnn).train()                   # the same replicated model on every rank
            ref = copy.deepcopy(m).train()
            st = ShardedDINTrainer.tables_from_model(m)
            assert st.P == world and type(st.backend).__name__ == "HipBackend"
            tr = ShardedDINTrainer(m, st, LR, torch.optim.SGD([p for _, p in _dense(m)], lr=LR_DENSE), initial_accumulator_value=ACC0)
            lo, hi = div_range(V, world, rank)
            s, e = (0, 64) if rank == 0 else (64, B)
            out = {}
            hist, hl, cand, y = _batch(T, 77 + T)
            with torch.no_grad():
                want = ref.eval()(_feats(hist, hl, cand, s, e))
                ref.train()
            got = tr.predict(_feats(hist, hl, cand, s, e))
            out["predict_bitwise"] = bool(torch.equal(got, want))
            w0 = ref.attention.table.detach().clone()
            grads, w, acc, _ = _reference_step(ref, _feats(hist, hl, cand), torch.from_numpy(y).cuda(), w0, torch.full_like(w0, ACC0))
            tr.step(_feats(hist, hl, cand, s, e), torch.from_numpy(y[s:e]).cuda())
            torch.cuda.synchronize()
            out["dense"], out["dense_bitwise"] = _check_dense(m, grads, "rank %d" % rank)
            out["shard"] = _check_shard(st, w, acc, "rank %d" % rank, lo, hi)
            q.put((rank, True, out))
        finally:
            dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, False, traceback.format_exc()))


def _run_world2(att, dnn, T):
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, att, dnn, T, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(2):
            res.append(q.get(timeout=150))
    except queue.Empty:
        res = None
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()                      # the exact processes this test started
    return res


@pytest.mark.parametrize("att,dnn,T", [("sigmoid", "relu", 50), ("prelu", "prelu", 7)])
def test_two_ranks_equal_one_step_over_the_concatenated_batch(built_lib, att, dnn, T):
    res = _run_world2(att, dnn, T)
    if res is None or any(isinstance(w, str) and ("onnect" in w or "imeout" in w or "store" in w.lower()) for _, _, w in res):
        res = _run_world2(att, dnn, T)    # one retry for a failed rendezvous (transport hiccup, not the code under test)
    assert res is not None, "workers did not report within the time limit"
    for rank, ok, out in res:
        assert ok, "rank %d raised:\n%s" % (rank, out)
        assert out["predict_bitwise"], "rank %d: predict differs from the single-GPU model on the local batch" % rank
        print("rank %d: %s" % (rank, out))


def test_lookup_train_dedup_on_the_hip_backend(built_lib):
    """ShardedTables.lookup_train(dedup=True) at world 1 with the product backend, three slots of skewed ids: the forward is bit for bit the
    plain lookup's on the same tables (and so dedup=False's), and every Adagrad step is within 1e-5 scaled of the float64 synchronous
    step -- dedup=True, a dedup=False step in between, dedup=True again."""
    from dir_amd.shard import ShardedTables
    from oracle import np_ref as R
    vocab, Kk, Bb = [50, 400, 3], 16, 300
    rng = np.random.default_rng(3)
    full = [rng.standard_normal((v, Kk)).astype(np.float32) for v in vocab]
    st = ShardedTables.from_full([torch.from_numpy(t.copy()).cuda() for t in full]).enable_training(LR, ACC0)
    ref_w, ref_a = [t.astype(np.float64) for t in full], [np.full(t.shape, ACC0) for t in full]
    for step, dedup in enumerate((True, False, True)):
        ids = np.stack([np.minimum(rng.zipf(1.3, size=Bb) - 2, v + 1) for v in vocab], axis=1).astype(np.int64)      # -1 and >= vocab included
        G = rng.standard_normal((Bb, len(vocab) * Kk)).astype(np.float32)
        d_ids, d_G = torch.from_numpy(ids).cuda(), torch.from_numpy(G).cuda()
        with torch.no_grad():
            plain = st.lookup(d_ids).clone()
        emb = st.lookup_train(d_ids, dedup=dedup)
        assert torch.equal(emb.detach(), plain), "step %d: lookup_train(dedup=%s)'s forward differs from the lookup's" % (step, dedup)
        (emb * d_G).sum().backward()
        R.sparse_adagrad_step(ref_w, ref_a, np.where((ids >= 0) & (ids < np.array(vocab)[None, :]), ids, -1), G.astype(np.float64), LR)
        for f in range(len(vocab)):
            ew = scaled(st.local_tables[f].cpu().numpy(), ref_w[f])
            ea = scaled(st.optimizer.accums[f].cpu().numpy(), ref_a[f])
            assert ew <= SPARSE_TOL and ea <= SPARSE_TOL, "step %d slot %d: table %.3e accumulator %.3e" % (step, f, ew, ea)
