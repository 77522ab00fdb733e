"""ShardedXDeepFMTrainer (and ShardedDeepFMTrainer(dedup=True, linear=)) on the GPU with the PRODUCT HIP backend: one training step over
row-sharded embedding tables and first-order weights on the de-duplicated exchange (dir_rows_scatter_sum_side_f32 on the requester),
against the single-GPU model that holds the full tables, on the concatenated batch.  World 1 in this process; two ranks (64 and 32 of
96 samples) as two processes on the one GPU, exchanges staged through host memory over gloo (tests/test_gpu_shard_multiproc.py's harness).

Model: F = 6, vocab [50, 400, 7, 1, 33, 120], D = 8, cin_layer_sizes (16, 16), dnn_hidden_units (32,), linear columns on the same
categoricals; ids Zipf-skewed and in range (positions are shared).
Bars: dense gradients (every cin_W, cin_out, the tower, linear_bias) 5e-5 scaled -- the bound tests/test_gpu_shard_din.py and
tests/test_gpu_backward.py hold dense gradients to; the embedding shards and accumulators against the single-GPU model's sparse embedding
gradient coalesced in float64 and pushed through the float64 Adagrad rule, and the first-order shards' w, n, z against its linear gradient
through the float64 FTRL rule: tests/hot_rows_inputs.BAR (1e-5, scaled); dedup=True against dedup=False: BAR."""
import os

import numpy as np
import pytest
import torch

from tests.hot_rows_inputs import BAR, scaled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, D = [50, 400, 7, 1, 33, 120], 8
F = len(VOCAB)
B_ALL, SPLIT = 96, (64, 32)
LR, ACC0, DENSE_BAR = 0.05, 0.1, 5e-5
FTRL = dict(lr=0.15, l1=0.01, l2=0.02)
SPARSE = ("embedding_weights", "linear_weights")


def _build(kind, linear_columns=True):
    """linear_columns=False: the same model (same seed, same dense initialisation) without its first-order term."""
    from dir_amd import feature_column as fc
    cats = [fc.categorical_column_with_identity("c%d" % i, v) for i, v in enumerate(VOCAB)]
    lin_cats = cats if linear_columns else None
    torch.manual_seed(7)                                   # the same replicated model on every rank
    if kind == "xdeepfm":
        from dir_amd.xdeepfm import XDeepFM
        m = XDeepFM(linear_feature_columns=lin_cats, dnn_feature_columns=[fc.embedding_column(c, D) for c in cats], cin_layer_sizes=(16, 16),
                    dnn_hidden_units=(32,))
    else:
        from dir_amd.deepfm import DeepFM
        m = DeepFM(linear_feature_columns=lin_cats or [], dnn_feature_columns=[fc.embedding_column(c, D) for c in cats], dnn_hidden_units=[16, 16],
                   fm_embedding_size=D)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for w in m.linear_weights:
            w.copy_(0.3 * torch.randn(w.shape, generator=g))
        m.linear_bias.fill_(0.05)
    return m.cuda()


def _batch():
    rng = np.random.default_rng(21)
    ids = np.stack([np.minimum(rng.zipf(1.3, size=B_ALL) - 1, v - 1) for v in VOCAB], axis=1).astype(np.int64)
    y = rng.integers(0, 2, size=(B_ALL, 1)).astype(np.float32)
    return torch.from_numpy(ids), torch.from_numpy(y)


def _dense_names(m, linear):
    return [n for n, _ in m.named_parameters() if not n.startswith(SPARSE) and (linear or n != "linear_bias")]


def _ftrl64(w, n, z, g, lr, l1, l2):
    n_new = n + g * g
    z_new = z + g - (np.sqrt(n_new) - np.sqrt(n)) / lr * w
    return np.where(np.abs(z_new) > l1, (np.sign(z_new) * l1 - z_new) / (np.sqrt(n_new) / lr + 2 * l2), 0.0), n_new, z_new


def _reference(kind, linear):
    """One step of the single-GPU model on the whole batch -> its dense gradients and the float64 state of every table after the float64
    Adagrad / FTRL rules on its coalesced sparse gradients."""
    ids, y = _batch()
    ref = _build(kind, linear_columns=bool(linear)).train()      # (without linear=: the CIN + DNN model, no first-order term)
    logits = ref({"c%d" % f: ids[:, f].cuda() for f in range(F)})
    torch.nn.functional.binary_cross_entropy_with_logits(logits, y.cuda(), reduction="sum").backward()
    named = dict(ref.named_parameters())
    dense = {n: named[n].grad.detach().clone() for n in _dense_names(ref, linear)}
    T, A, Wn = [], [], []
    touched = [np.zeros(v, bool) for v in VOCAB]
    for f in range(F):
        touched[f][ids[:, f].numpy()] = True
        p = ref.embedding_weights[f]
        g = p.grad
        g = g.double().coalesce().to_dense().cpu().numpy() if g.is_sparse else g.double().cpu().numpy()      # (sparse: summed in float64)
        acc = np.full(g.shape, ACC0) + g * g
        T.append(p.detach().double().cpu().numpy() - LR * g / np.sqrt(acc))
        A.append(acc)
        if linear:
            w = ref.linear_weights[f]
            gw = w.grad
            gw = (gw.double().coalesce().to_dense() if gw.is_sparse else gw.double()).cpu().numpy().reshape(-1)
            w0 = w.detach().double().cpu().numpy().reshape(-1)
            new = _ftrl64(w0, np.full(w0.shape, ACC0), np.zeros(w0.shape), gw, FTRL["lr"], FTRL["l1"], FTRL["l2"])
            t = touched[f]
            Wn.append(tuple(np.where(t, a, b) for a, b in zip(new, (w0, np.full(w0.shape, ACC0), np.zeros(w0.shape)))))
    return dict(dense=dense, T=T, A=A, W=Wn)


_REF = {}


def reference(kind, linear):
    key = (kind, bool(linear))
    if key not in _REF:
        _REF[key] = _reference(kind, linear)
    return _REF[key]


def _trainer(kind, model, linear, dedup, **kw):
    from dir_amd.shard import ShardedDeepFMTrainer, ShardedTables, ShardedXDeepFMTrainer
    named = dict(model.named_parameters())
    opt = torch.optim.SGD([named[n] for n in _dense_names(model, False)], lr=0.01)      # (linear_bias takes the FTRL step)
    if kind == "xdeepfm":
        tables = ShardedXDeepFMTrainer.tables_from_model(model, linear=bool(linear), **kw)
        return ShardedXDeepFMTrainer(model, tables, LR, opt, initial_accumulator_value=ACC0, linear=FTRL if linear else None, dedup=dedup), tables
    tables = ShardedTables.from_full([p.detach().clone() for p in model.embedding_weights], **kw)
    if linear:
        tables.attach_linear_from_full([p.detach().clone() for p in model.linear_weights], ACC0)
    return ShardedDeepFMTrainer(model, tables, LR, opt, initial_accumulator_value=ACC0, linear=FTRL if linear else None, dedup=dedup), tables


def run_case(rank, world, kind="xdeepfm", linear=True, dedup=True, **kw):
    """One trainer step on this rank's part of the batch -> (errors against the single-GPU reference, the shards' state as CPU tensors,
    whether the dense gradients are bitwise the reference's, the trainer)."""
    ids, y = _batch()
    lo = 0 if world == 1 else sum(SPLIT[:rank])
    hi = B_ALL if world == 1 else lo + SPLIT[rank]
    ref = reference(kind, linear)
    model = _build(kind)
    tr, tables = _trainer(kind, model, linear, dedup, **kw)
    tr.step(ids[lo:hi].cuda(), y[lo:hi].cuda())
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    errs = {"dense": 0.0}
    bitwise = True
    for n, want in ref["dense"].items():
        got = named[n].grad
        assert got is not None, "%s has no gradient" % n
        errs["dense"] = max(errs["dense"], scaled(got.double().cpu().numpy(), want.double().cpu().numpy()))
        bitwise = bitwise and torch.equal(got, want)
    if not linear:
        assert named["linear_bias"].grad is None and float(named["linear_bias"].detach()) == pytest.approx(0.05)
    state = {}
    sl = tables.slices
    w, n_, z = tables.linear_state() if linear else (None, None, None)
    for f, (s, e) in enumerate(sl):
        state["T%d" % f], state["A%d" % f] = tables.local_tables[f].cpu(), tables.optimizer.accums[f].cpu()
        errs["emb"] = max(errs.get("emb", 0.0), scaled(state["T%d" % f].numpy(), ref["T"][f][s:e]))
        errs["acc"] = max(errs.get("acc", 0.0), scaled(state["A%d" % f].numpy(), ref["A"][f][s:e]))
        if linear:
            for name, got, want in zip("wnz", (w[f], n_[f], z[f]), ref["W"][f]):
                state[name + str(f)] = got.cpu().clone()
                errs[name] = max(errs.get(name, 0.0), scaled(state[name + str(f)].numpy(), want[s:e]))
    return errs, state, bitwise, tr, (ids[lo:hi].cuda(), model, tables)


def _check(errs, what):
    print("%s: %s" % (what, "  ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    assert errs["dense"] <= DENSE_BAR, "%s: dense gradients %.3e off the single-GPU model's" % (what, errs["dense"])
    for k, v in errs.items():
        if k != "dense":
            assert v <= BAR, "%s: %s %.3e off the float64 rule on the single-GPU model's gradient" % (what, k, v)


def _between(a, b):
    assert a.keys() == b.keys()
    return max(scaled(a[k].numpy(), b[k].double().numpy()) for k in a)


# ---- world 1 ---------------------------------------------------------------------------------------------------------------------
def test_step_matches_the_single_gpu_model_world_1(built_lib):
    from dir_amd.shard import xdeepfm_predict
    errs, on, bitwise, tr, (ids, model, tables) = run_case(0, 1, dedup=True)
    print("world 1: the dense gradients are %sbitwise the single-GPU model's" % ("" if bitwise else "NOT "))
    _check(errs, "xDeepFM world 1 dedup=True")
    assert tr.dedup is True and tables.stats["fallbacks"] == 0
    assert torch.equal(tr.predict(ids), xdeepfm_predict(model, tables, ids))
    errs, off, _, _, _ = run_case(0, 1, dedup=False)
    _check(errs, "xDeepFM world 1 dedup=False")
    worst = _between(on, off)
    print("dedup=True against dedup=False: %.2e" % worst)
    assert worst <= BAR


def test_dedup_off_is_todays_lookup_train_bit_for_bit(built_lib):
    """The dedup=False trainer's shards against lookup_train(ids, with_linear=True) -- the call as it stands today, without the new
    argument -- on twin tables, driven with the SAME upstream gradients (recorded off the trainer's own lookup by hooks: the model's
    backward is not what is compared)."""
    from dir_amd.shard import ShardedTables
    _, y = _batch()
    # every row of a slot at most once, pruned ids (-1) where a slot has fewer rows than the batch has samples: where DUPLICATES of a row
    # sit in the one-position-per-entry slabs depends on the order of the bucket pass's reservation atomics, so two runs of the very same
    # dedup=False step agree to fp32 rounding only (tests/test_gpu_shard_linear.py says so of lookup_train); with one gradient per row
    # there is no order, and any difference would be this pull request's doing
    rng = np.random.default_rng(33)
    ids = torch.full((B_ALL, F), -1, dtype=torch.int64)
    for f, v in enumerate(VOCAB):
        at = rng.permutation(B_ALL)[:min(v, B_ALL)]
        ids[at, f] = torch.from_numpy(rng.permutation(v)[:at.size])
    model = _build("xdeepfm")
    tr, tables = _trainer("xdeepfm", model, True, False)
    twin = ShardedTables.from_full([p.detach().clone() for p in model.embedding_weights])
    twin.attach_linear_from_full([p.detach().clone() for p in model.linear_weights], ACC0)
    twin.enable_training(LR, ACC0).enable_linear_training(FTRL["lr"], FTRL["l1"], FTRL["l2"])
    seen, real = {}, tables.lookup_train

    def recording(ids_, **kw):
        assert kw == dict(with_linear=True, dedup=False)
        emb, lin = real(ids_, **kw)
        emb.register_hook(lambda g: seen.__setitem__("g_emb", g.clone()))
        lin.register_hook(lambda g: seen.__setitem__("g_lin", g.clone()))
        return emb, lin
    tables.lookup_train = recording
    tr.step(ids.cuda(), y.cuda())
    emb2, lin2 = twin.lookup_train(ids.cuda(), with_linear=True)
    torch.autograd.backward([emb2, lin2], [seen["g_emb"], seen["g_lin"]])
    torch.cuda.synchronize()
    for a, b in zip(tables.linear_state(), twin.linear_state()):
        for f in range(F):
            assert torch.equal(a[f], b[f]), "first-order state, slot %d" % f
    for f in range(F):
        assert torch.equal(tables.local_tables[f], twin.local_tables[f]) and torch.equal(tables.optimizer.accums[f], twin.optimizer.accums[f]), f
    assert tables._updates == twin._updates == 1


def test_linear_none_trains_the_cin_dnn_model(built_lib):
    errs, _, _, tr, _ = run_case(0, 1, linear=False, dedup=True)
    _check(errs, "xDeepFM world 1 linear=None")
    assert tr.linear is None


def test_deepfm_trainer_dedup_with_linear(built_lib):
    errs, on, _, tr, _ = run_case(0, 1, kind="deepfm", dedup=True)
    _check(errs, "DeepFM world 1 dedup=True linear=")
    assert tr.dedup is True
    errs, off, _, tr, _ = run_case(0, 1, kind="deepfm", dedup=False)
    _check(errs, "DeepFM world 1 default")
    assert tr.dedup is False and _between(on, off) <= BAR


def test_constructor_refusals(built_lib):
    from dir_amd.shard import ShardedXDeepFMTrainer
    model = _build("xdeepfm")
    tables = ShardedXDeepFMTrainer.tables_from_model(model)
    with pytest.raises(ValueError, match="linear_bias"):
        ShardedXDeepFMTrainer(model, tables, LR, torch.optim.SGD(list(model.parameters()), lr=0.01), linear=FTRL)
    bare = ShardedXDeepFMTrainer.tables_from_model(model, linear=False)
    dense = [p for n, p in model.named_parameters() if not n.startswith(SPARSE) and n != "linear_bias"]
    with pytest.raises(ValueError, match="first-order"):
        ShardedXDeepFMTrainer(model, bare, LR, torch.optim.SGD(dense, lr=0.01), linear=FTRL)
    from dir_amd import feature_column as fc
    from dir_amd.xdeepfm import XDeepFM
    cats = [fc.categorical_column_with_identity("c%d" % i, v) for i, v in enumerate(VOCAB)]
    other = XDeepFM(linear_feature_columns=cats[:3], dnn_feature_columns=[fc.embedding_column(c, D) for c in cats], cin_layer_sizes=(16,),
                    dnn_hidden_units=(32,)).cuda()
    with pytest.raises(ValueError, match="categoricals"):
        ShardedXDeepFMTrainer.tables_from_model(other)
    assert ShardedXDeepFMTrainer.tables_from_model(other, linear=False).lin_rows is None


# ---- two ranks on one GPU --------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        os.environ["DIR_SHARD_HOST_STAGED"] = "1"          # two ranks on ONE GPU: exchanges staged through host memory over gloo
        import datetime
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="file://" + port, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        try:
            torch.cuda.set_device(0)
            import dir_amd  # noqa: F401
            from dir_amd.shard import xdeepfm_predict
            out = {}
            errs, on, _, tr, (ids, model, tables) = run_case(rank, world, dedup=True)
            out["dedup"] = errs
            assert tables.P == world and type(tables.backend).__name__ == "HipBackend" and tables.stats["fallbacks"] == 0
            out["predict"] = bool(torch.equal(tr.predict(ids), xdeepfm_predict(model, tables, ids)))
            errs, off, _, _, _ = run_case(rank, world, dedup=False)
            out["plain"] = errs
            out["between"] = _between(on, off)
            errs, _, _, _, (_, _, tables) = run_case(rank, world, dedup=True, slack=0.02, mode="fixed", chunks=1)
            out["overflow"], out["fallbacks"] = errs, tables.stats["fallbacks"]
            out["deepfm"] = run_case(rank, world, kind="deepfm", dedup=True)[0]
            q.put((rank, True, out))
        finally:
            dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, False, traceback.format_exc()))


def test_two_ranks_equal_one_step_over_the_concatenated_batch(built_lib):
    import queue
    import torch.multiprocessing as mp
    from tests.test_gpu_shard_multiproc import _free_port
    ctx = mp.get_context("spawn")

    def run():
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
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
                p.kill()
        return res

    res = run()
    if res is None or any(isinstance(w, str) and ("onnect" in w or "imeout" in w or "store" in w.lower()) for _, _, w in res):
        res = run()
    assert res is not None, "workers did not report within the time limit"
    for rank, ok, out in res:
        assert ok, "rank %d raised:\n%s" % (rank, out)
        _check(out["dedup"], "rank %d xDeepFM dedup=True" % rank)
        _check(out["plain"], "rank %d xDeepFM dedup=False" % rank)
        _check(out["overflow"], "rank %d xDeepFM after a forced overflow" % rank)
        _check(out["deepfm"], "rank %d DeepFM dedup=True linear=" % rank)
        assert out["fallbacks"] >= 1, "slack=0.02 did not overflow"
        assert out["between"] <= BAR, "rank %d: dedup=True and dedup=False differ by %.3e" % (rank, out["between"])
        assert out["predict"], "rank %d: predict differs from xdeepfm_predict" % rank
