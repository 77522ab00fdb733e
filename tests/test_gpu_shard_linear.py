"""DeepFM's first-order (linear) term over row-sharded weights on the GPU (ShardedTables.attach_linear / lookup(want_lin=) /
lookup_train(with_linear=) / ShardedDeepFMTrainer(linear=) with the PRODUCT HIP backend: dir_shard_linear_gather_f32,
dir_shard_linear_finish_f32, dir_shard_linear_grad_f32, dir_sparse_ftrl_rows_sorted_payload_f32).

  (a) world size 1, forward: bitwise equal to ops.linear_logit over the unsharded packed rows (F in {1, 3, 26}, B in {0, 1, 37, 4096},
      pruned ids, with and without bias, de-duplicated, exact path);
  (b) world size 1, training against float64 (oracle.np_ref.sparse_ftrl_step): uniform ids, l1 = l2 = 0 and both non-zero; skewed ids (one
      row hit > 600 times in a batch of 1500, a Zipf(1.3) slot; one row hit 3000 times in a batch of 4096);
  (c) world size 1 against the single-GPU path (ops.SparseFtrl on TableSet.ftrl_rows);
  (d) one node: the linear term does not perturb the Adagrad side, bit for bit;
  (e) a captured lookup(want_fm, want_lin) replays the eager result bitwise after a training step;
  (f) two ranks on cuda:0 over host-staged gloo: the forward is still bitwise ops.linear_logit's; ShardedDeepFMTrainer(linear=) two steps +
      predict against the float64 model; (g) the same over RCCL with one rank per GPU (skipped with a reason on a one-GPU box).
Error measure (tests/test_gpu_shard_bags_train.py::_close): max |got - ref| / (1 + |ref|) against float64, bar 1e-5 unless stated."""
import os

import numpy as np
import pytest
import torch

from tests.test_shard_linear_gloo import Reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, ACC0 = 0.3, 0.1


def _store():
    import tempfile
    return os.path.join(tempfile.mkdtemp(prefix="dir_pg_"), "store")


def _close(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else got
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max()) if got.size else 0.0


def _draw(vocab, K, seed, dev):
    rng = np.random.default_rng(seed)
    full = [torch.from_numpy(rng.standard_normal((v, K)).astype(np.float32)).to(dev) for v in vocab]
    full_w = [torch.from_numpy((0.3 * rng.standard_normal(v)).astype(np.float32)).to(dev) for v in vocab]
    return full, full_w


def _ids(rng, vocab, B, dev, lo=-2, over=2):
    a = np.stack([rng.integers(lo, v + over, size=B) for v in vocab], axis=1).astype(np.int64).reshape(B, len(vocab))
    return torch.from_numpy(a).to(dev)


@pytest.mark.parametrize("F", [1, 3, 26])
def test_world1_forward_bitwise_equals_linear_logit(built_lib, F):
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = [500, 1000, 7][:F] if F <= 3 else [200 + 37 * i for i in range(F)]
    K = 16
    full, full_w = _draw(vocab, K, 3 + F, dev)
    rows = ops.TableSet.ftrl_rows(full_w)
    bias = torch.tensor([0.37], dtype=torch.float32, device=dev)
    rng = np.random.default_rng(17)
    for kw in ({}, {"dedup": True}, {"mode": "exact"}):
        st = ShardedTables.from_full(full, **kw).attach_linear_from_full(full_w)
        for B in (1, 37, 4096, 0):
            ids = _ids(rng, vocab, B, dev)
            for b in (bias, None):
                emb, fm, lin = st.lookup(ids, want_fm=True, want_lin=True, lin_bias=b)
                torch.cuda.synchronize()
                assert tuple(lin.shape) == (B, 1) and tuple(emb.shape) == (B, F * K) and tuple(fm.shape) == (B, 1)
                if B == 0:                                                  # an empty [0, 1] result, no launch error (the single-GPU
                    continue                                                # kernel takes no empty batch: nothing to compare with)
                assert torch.equal(lin, ops.linear_logit(rows, ids, bias=b)), (kw, B, b is not None)
                assert torch.equal(emb, st.lookup(ids))                     # callers that do not ask see today's results
            emb2, lin2 = st.lookup(ids, want_lin=True)
            assert tuple(lin2.shape) == (B, 1) and torch.equal(emb2, emb)
            assert B == 0 or torch.equal(lin2, ops.linear_logit(rows, ids))


def _train(st, ids, G, g):
    emb, lin = st.lookup_train(ids, with_linear=True)
    ((emb * G).sum() + (lin * g).sum()).backward()
    return emb, lin


def _state_err(st, ref):
    w, n, z = st.linear_state()
    F = len(w)
    return tuple(max(_close(got[f], want[f][:, 0]) for f in range(F)) for got, want in ((w, ref.w), (n, ref.n), (z, ref.z)))


@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (0.05, 0.1)])
def test_world1_training_matches_float64(built_lib, l1, l2):
    """Uniform ids over vocab = [500, 1000, 7], five steps: w, n, z within 1e-5 of oracle.np_ref.sparse_ftrl_step in float64; the embedding
    tables and accumulators of the same node within 1e-5 of float64 Adagrad."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, B = [500, 1000, 7], 16, 1500
    F = len(vocab)
    full, full_w = _draw(vocab, K, 5, dev)
    ftrl = dict(lr=0.2, l1=l1, l2=l2)
    st = ShardedTables.from_full([t.clone() for t in full]).attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(**ftrl)
    ref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
    rng = np.random.default_rng(23)
    for step in range(5):
        ids = _ids(rng, vocab, B, dev)
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).to(dev)
        _train(st, ids, G, g)
        ref.step(ids.cpu().numpy(), G.cpu().numpy(), g.cpu().numpy(), ftrl)
        ew, en, ez = _state_err(st, ref)
        print("step %d l1=%g l2=%g: w %.2e n %.2e z %.2e" % (step, l1, l2, ew, en, ez))
        assert ew <= 1e-5 and en <= 1e-5 and ez <= 1e-5, (step, ew, en, ez)
    et = max(_close(st.local_tables[f], ref.T[f]) for f in range(F))
    ea = max(_close(st.optimizer.accums[f], ref.acc[f]) for f in range(F))
    print("tables %.2e accumulators %.2e" % (et, ea))
    assert et <= 1e-5 and ea <= 1e-5
    if l1 > 0:
        assert any(bool((w == 0).any()) for w in st.linear_weights()), "l1 clips some touched weights to exactly 0.0"


def _skewed(rng, vocab, B, hot_row, dev):
    a = np.stack([rng.integers(0, v, size=B) for v in vocab], axis=1).astype(np.int64)
    a[:, 0] = np.minimum(rng.zipf(1.3, size=B) - 1, vocab[0] - 1)         # a Zipf(1.3) slot
    hot = rng.permutation(B)[:700]
    a[hot, 1] = hot_row                                                    # one row in most of the batch
    return torch.from_numpy(a).to(dev)


def _train_against_float64(make_ids, B, seed, min_hits, hot_row, gscale=1.0):
    """Three steps on ids from make_ids: the worst error of w, n, z, the embedding tables and the Adagrad accumulators against float64."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K = [500, 1000, 7], 16
    F = len(vocab)
    full, full_w = _draw(vocab, K, seed, dev)
    ftrl = dict(lr=0.2, l1=0.01, l2=0.02)
    st = ShardedTables.from_full([t.clone() for t in full]).attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(**ftrl)
    ref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
    rng = np.random.default_rng(seed + 22)
    for step in range(3):
        ids = make_ids(rng, vocab, B, dev)
        hits = int((ids[:, 1] == hot_row).sum())
        assert hits >= min_hits, hits
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
        g = torch.from_numpy((rng.standard_normal((B, 1)) * gscale).astype(np.float32)).to(dev)
        _train(st, ids, G, g)
        ref.step(ids.cpu().numpy(), G.cpu().numpy(), g.cpu().numpy(), ftrl)
        ew, en, ez = _state_err(st, ref)
        et = max(_close(st.local_tables[f], ref.T[f]) for f in range(F))
        ea = max(_close(st.optimizer.accums[f], ref.acc[f]) for f in range(F))
        print("step %d (%d hits): w %.2e n %.2e z %.2e tables %.2e accumulators %.2e" % (step, hits, ew, en, ez, et, ea))
        assert max(ew, en, ez, et, ea) <= 1e-5, (step, ew, en, ez, et, ea)


def test_world1_training_skewed_ids_match_float64(built_lib):
    """One row hit more than 600 times in a batch of 1500 and a Zipf(1.3) slot: its run crosses sort tiles (the carry / fix path).  w, n, z,
    the tables and the accumulators within 1e-5: the sorted update compensates its run sums (csrc/backward.hip: run_sum)."""
    _train_against_float64(lambda rng, vocab, B, dev: _skewed(rng, vocab, B, 321, dev), 1500, 7, 601, 321)


def _hot(rng, vocab, B, dev):
    a = np.stack([rng.integers(0, v, size=B) for v in vocab], axis=1).astype(np.int64)
    a[rng.permutation(B)[:3000], 1] = 321
    return torch.from_numpy(a).to(dev)


def test_world1_training_hot_row_matches_float64(built_lib):
    """One row hit 3000 times in a batch of 4096: a run over twelve sort tiles whose entries arrive in the order the slab's atomics left --
    not the same from run to run -- so the bar must hold for any order: every state within 1e-5 over three steps.  (d lin is drawn at
    0.3: the row's summed gradient, sigma ~ 16, stays below 64, where fp32's own rounding of the sum is under 4e-6.)"""
    _train_against_float64(_hot, 4096, 31, 3000, 321, gscale=0.3)


def test_world1_matches_single_gpu_sparse_ftrl(built_lib):
    """The same ids and d logit through ops.SparseFtrl on TableSet.ftrl_rows: w, n, z within 1e-5 of each other (not bitwise: after
    bucketing, duplicates may be summed in a different order)."""
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, B = [500, 1000, 7], 16, 1500
    F = len(vocab)
    full, full_w = _draw(vocab, K, 9, dev)
    ftrl = dict(lr=0.2, l1=0.02, l2=0.05)
    st = ShardedTables.from_full([t.clone() for t in full]).attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(**ftrl)
    rows = ops.TableSet.ftrl_rows(full_w, ACC0)
    single = ops.SparseFtrl(rows, ftrl["lr"], l1=ftrl["l1"], l2=ftrl["l2"])
    rng = np.random.default_rng(31)
    for step in range(3):
        ids = _ids(rng, vocab, B, dev)
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).to(dev)
        _train(st, ids, G, g)
        clean = torch.where((ids >= 0) & (ids < torch.tensor(vocab, device=dev)), ids, torch.full_like(ids, -1))
        single.step(clean, g)
        torch.cuda.synchronize()
        for c, name in enumerate("wnz"):
            err = max(_close(st.lin_rows[f][:, c], rows.rows[f][:, c].double().cpu().numpy()) for f in range(F))
            print("step %d %s: %.2e" % (step, name, err))
            assert err <= 1e-5, (step, name, err)


def test_one_node_leaves_the_adagrad_side_bitwise(built_lib):
    """lookup_train(ids, with_linear=True): emb equals lookup(ids) bit for bit, and after (emb * G).sum() + (lin * g).sum() went back the
    embedding tables and accumulators equal, bitwise, those of a twin trained with lookup_train(ids) and G alone.
    The ids of a slot are distinct here (plus pruned ones): where DUPLICATES of a row sit in the slabs depends on the order of the bucket
    pass's reservation atomics, so two runs of the very same step add a row's gradients in different orders and agree to fp32 rounding
    only (ShardedTables.lookup_bags_train's docstring says so of lookup_train); with one gradient per row there is no order, and any
    difference would be the linear term's doing."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, B = [5000, 3000, 1700], 16, 1500
    F = len(vocab)
    full, full_w = _draw(vocab, K, 13, dev)
    st = ShardedTables.from_full([t.clone() for t in full]).attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(0.2, 0.01, 0.02)
    twin = ShardedTables.from_full([t.clone() for t in full]).enable_training(LR, ACC0)
    rng = np.random.default_rng(37)
    for step in range(2):
        a = np.stack([rng.permutation(v)[:B] for v in vocab], axis=1).astype(np.int64)
        a[rng.permutation(B)[:40], rng.integers(0, F, size=40)] = -1
        ids = torch.from_numpy(a).to(dev)
        G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).to(dev)
        plain = st.lookup(ids).clone()
        before = st._updates
        w0 = [w.clone() for w in st.linear_weights()]
        emb, lin = st.lookup_train(ids, with_linear=True)
        assert torch.equal(emb, plain)
        ((emb * G).sum() + (lin * g).sum()).backward()
        assert st._updates == before + 1
        e2 = twin.lookup_train(ids)
        (e2 * G).sum().backward()
        torch.cuda.synchronize()
        for f in range(F):
            assert torch.equal(st.local_tables[f], twin.local_tables[f]), (step, f)
            assert torch.equal(st.optimizer.accums[f], twin.optimizer.accums[f]), (step, f)
            assert not torch.equal(st.linear_weights()[f], w0[f])          # ... while the first-order rows did take their step


def test_owner_ftrl_on_its_own_sort_equals_on_the_adagrad_sort(built_lib):
    """The owner's FTRL takes the Adagrad step's sorted pairs when that step has just run over the same payload (sorted_by), and sorts for
    itself otherwise: Adagrad then FTRL on its sort, and FTRL on its own sort then Adagrad, leave the same rows bit for bit (one payload,
    one stable sort, the same run sums)."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, n = [500, 1000, 7], 16, 6000
    F = len(vocab)
    full, full_w = _draw(vocab, K, 53, dev)
    rng = np.random.default_rng(59)
    slot = rng.integers(0, F, size=n)
    row = np.array([rng.integers(0, vocab[f]) for f in slot])
    pay = row * F + slot
    pay[rng.permutation(n)[:100]] = -1
    pay = torch.from_numpy(pay.astype(np.int64)).to(dev)
    grows = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    sts = []
    for reuse in (True, False):
        st = ShardedTables.from_full([t.clone() for t in full]).attach_linear_from_full(full_w, ACC0)
        st.enable_training(LR, ACC0).enable_linear_training(0.2, 0.01, 0.02)
        be = st.backend
        if reuse:
            be.apply_adagrad(st.optimizer, pay, grows)
            be.apply_ftrl(pay, g, 0.2, 0.01, 0.02, sorted_by=st.optimizer)
        else:
            be.apply_ftrl(pay, g, 0.2, 0.01, 0.02)
            be.apply_adagrad(st.optimizer, pay, grows)
        sts.append(st)
    torch.cuda.synchronize()
    for f in range(F):
        assert torch.equal(sts[0].lin_rows[f], sts[1].lin_rows[f]), f
        assert torch.equal(sts[0].local_tables[f], sts[1].local_tables[f]), f
        assert not torch.equal(sts[0].lin_rows[f][:, 0], full_w[f])


def test_world1_graph_replay_equals_eager_after_training(built_lib):
    """lookup(ids, want_fm=True, want_lin=True) with check="never" captured once; after one training step (the rows moved) one replay
    equals the eager result bit for bit."""
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, B = [300, 800, 20], 16, 512
    F = len(vocab)
    full, full_w = _draw(vocab, K, 19, dev)
    st = ShardedTables.from_full([t.clone() for t in full], check="never").attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(0.2, 0.01, 0.0)
    rng = np.random.default_rng(41)
    ids = _ids(rng, vocab, B, dev)
    bias = torch.tensor([-0.21], dtype=torch.float32, device=dev)
    e0, f0, l0 = (t.clone() for t in st.lookup(ids, want_fm=True, want_lin=True, lin_bias=bias))
    step = ops.CapturedStep(lambda: st.lookup(ids, want_fm=True, want_lin=True, lin_bias=bias))
    G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)).to(dev)
    _train(st, ids, G, g)
    e1, f1, l1 = (t.clone() for t in st.lookup(ids, want_fm=True, want_lin=True, lin_bias=bias))
    step.replay()
    torch.cuda.synchronize()
    assert torch.equal(step.out[0], e1) and torch.equal(step.out[1], f1) and torch.equal(step.out[2], l1)
    assert not torch.equal(l1, l0) and not torch.equal(e1, e0)                 # the step did move what the graph reads


def test_world1_predict_adds_the_linear_term_on_both_routes(built_lib):
    """ShardedDeepFMTrainer(linear=).predict = the FM + DNN predict of a twin without the term + ops.linear_logit, on the one-launch tower
    route (K = 16, 2048 rows) and on the fallback route (K = 8)."""
    from dir_amd import feature_column as fc, ops
    from dir_amd.deepfm import DeepFM
    from dir_amd.shard import ShardedDeepFMTrainer, ShardedTables
    dev = torch.device("cuda", 0)
    for K, B in ((16, 2048), (8, 64)):
        V, F = 300, 4
        cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
        torch.manual_seed(7)
        model = DeepFM(linear_feature_columns=[], dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[16, 16],
                       fm_embedding_size=K).cuda()
        with torch.no_grad():
            model.linear_bias.fill_(0.125)
        full = [p.detach().clone() for p in model.embedding_weights]
        _, full_w = _draw([V] * F, K, 43, dev)
        dense = [p for n, p in model.named_parameters() if not n.startswith(("embedding_weights", "linear_weights")) and n != "linear_bias"]
        mk = lambda: torch.optim.Adagrad(dense, lr=0.05, initial_accumulator_value=0.1, eps=0.0)      # noqa: E731
        with_lin = ShardedDeepFMTrainer(model, ShardedTables.from_full(full).attach_linear_from_full(full_w), 0.05, mk(), linear=dict(lr=0.2))
        without = ShardedDeepFMTrainer(model, ShardedTables.from_full(full), 0.05, mk())
        ids = _ids(np.random.default_rng(47), [V] * F, B, dev, lo=0, over=0)
        want = without.predict(ids) + ops.linear_logit(ops.TableSet.ftrl_rows(full_w), ids, bias=model.linear_bias.data)
        got = with_lin.predict(ids)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (K, B, float((got - want).abs().max()))


# ---- two ranks ------------------------------------------------------------------------------------------------------------------------
def _scenarios(rank, world, device):
    import torch.distributed as dist
    from dir_amd import feature_column as fc, ops
    from dir_amd.deepfm import DeepFM
    from dir_amd.shard import ShardedDeepFMTrainer, ShardedTables, local_slice
    out = []
    V, K, F, B, steps = 50, 8, 4, 64, 2
    vocab = [V] * F
    ftrl = dict(lr=0.15, l1=0.01, l2=0.02)
    cats = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(F)]
    torch.manual_seed(7)                                   # the same dense initialisation on every rank
    model = DeepFM(linear_feature_columns=[], dnn_feature_columns=[fc.embedding_column(c, K) for c in cats], dnn_hidden_units=[16, 16],
                   fm_embedding_size=K).to(device)
    full = [p.detach().clone() for p in model.embedding_weights]
    full_w = [torch.from_numpy((0.3 * np.random.default_rng(3 + f).standard_normal(V)).astype(np.float32)).to(device) for f in range(F)]
    st = ShardedTables.from_full(full).attach_linear_from_full(full_w, 0.1)

    # the forward at two ranks is still ops.linear_logit's over the unsharded rows, bit for bit (per sample, slot order, whoever the owners)
    rows = ops.TableSet.ftrl_rows(full_w)
    bias = torch.tensor([0.37], dtype=torch.float32, device=device)
    ids0 = _ids(np.random.default_rng(100 + rank), vocab, 37 + 5 * rank, device)
    emb, fm, lin = st.lookup(ids0, want_fm=True, want_lin=True, lin_bias=bias)
    torch.cuda.synchronize()
    out.append(("forward_bitwise", torch.equal(lin, ops.linear_logit(rows, ids0, bias=bias)) and torch.equal(emb, st.lookup(ids0)), ""))

    names = [n for n, _ in model.named_parameters() if not n.startswith(("embedding_weights", "linear_weights")) and n != "linear_bias"]
    dense = [p for n, p in model.named_parameters() if n in names]
    opt = torch.optim.Adagrad(dense, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    tr = ShardedDeepFMTrainer(model, st, lr_sparse=0.05, dense_optimizer=opt, linear=ftrl)
    ref = Reference([t.cpu().numpy() for t in full], [w.cpu().numpy() for w in full_w])
    d64 = [p.detach().double().cpu().clone().requires_grad_(True) for p in dense]
    dacc = [torch.full_like(p, 0.1) for p in d64]
    b64, bn, bz = torch.zeros(1, dtype=torch.float64, requires_grad=True), np.full(1, 0.1), np.zeros(1)
    pd = dict(zip(names, d64))

    def model64(T, W, ids):
        emb = torch.cat([T[f][ids[:, f]] for f in range(F)], dim=1)
        e3 = emb.view(-1, F, K)
        fm = 0.5 * ((e3.sum(1) ** 2) - (e3 ** 2).sum(1)).sum(1, keepdim=True)
        net = emb
        for i in range(2):
            net = torch.relu(net @ pd["hidden.%d.weight" % i].t() + pd["hidden.%d.bias" % i])
        lin = sum(W[f][ids[:, f]] for f in range(F)) + b64
        return fm + net @ pd["logits_layer.weight"].t() + pd["logits_layer.bias"] + lin

    from oracle import np_ref as R
    losses = []
    for s in range(steps):
        gb = torch.Generator().manual_seed(1000 + s)
        ids_all = torch.randint(0, V, (world * B, F), generator=gb)
        ids_all[::B, 0] = 3
        ids_all[1::B, 0] = 3                               # one row in every rank's batch, twice
        lab_all = torch.randint(0, 2, (world * B, 1), generator=gb).double()
        ids, lab = ids_all[rank * B:(rank + 1) * B].to(device), lab_all[rank * B:(rank + 1) * B].float().to(device)
        loss = tr.step(ids, lab)
        T = [torch.from_numpy(t).requires_grad_(True) for t in ref.T]
        W = [torch.from_numpy(w) for w in ref.w]
        logit = model64(T, W, ids_all)
        logit.retain_grad()
        per = torch.nn.functional.binary_cross_entropy_with_logits(logit, lab_all, reduction="none")
        grads = torch.autograd.grad(per.sum(), T + d64 + [b64, logit])
        losses.append(_close(loss.reshape(1), per[rank * B:(rank + 1) * B].sum().detach().numpy().reshape(1)))
        for f in range(F):
            g = grads[f].numpy()
            ref.acc[f] += g * g
            ref.T[f] -= 0.05 * g / np.sqrt(ref.acc[f])
        R.sparse_ftrl_step(ref.w, ref.n, ref.z, ids_all.numpy(), grads[-1].numpy(), ftrl["lr"], ftrl["l1"], ftrl["l2"])
        with torch.no_grad():
            for p, a, g in zip(d64, dacc, grads[F:F + len(d64)]):
                a += g ** 2
                p -= 0.05 * g / a.sqrt()
            g = grads[F + len(d64)].numpy()
            n_new = bn + g * g
            z_new = bz + g - (np.sqrt(n_new) - np.sqrt(bn)) / ftrl["lr"] * b64.numpy()
            b64.copy_(torch.from_numpy(np.where(np.abs(z_new) > ftrl["l1"], (np.sign(z_new) * ftrl["l1"] - z_new)
                                                / (np.sqrt(n_new) / ftrl["lr"] + 2 * ftrl["l2"]), 0.0)))
            bn, bz = n_new, z_new
    sl = [slice(*local_slice(v, world, 0, world, rank)) for v in vocab]
    w, n, z = st.linear_state()
    errs = dict(loss=max(losses),
                tables=max(_close(st.local_tables[f], ref.T[f][sl[f]]) for f in range(F)),
                accums=max(_close(st.optimizer.accums[f], ref.acc[f][sl[f]]) for f in range(F)),
                w=max(_close(w[f], ref.w[f][sl[f], 0]) for f in range(F)),
                n=max(_close(n[f], ref.n[f][sl[f], 0]) for f in range(F)),
                z=max(_close(z[f], ref.z[f][sl[f], 0]) for f in range(F)),
                dense=max(_close(p, r.detach().numpy()) for p, r in zip(dense, d64)),
                bias=_close(torch.cat([model.linear_bias.data, tr.bias_accum, tr.bias_linear]), np.concatenate([b64.detach().numpy(), bn, bz])))
    got = tr.predict(ids)
    with torch.no_grad():
        want = model64([torch.from_numpy(t) for t in ref.T], [torch.from_numpy(w_) for w_ in ref.w], ids_all[rank * B:(rank + 1) * B]).numpy()
    errs["predict"] = _close(got, want)
    out.append(("trainer", got.shape == (B, 1) and all(v <= 1e-5 for v in errs.values()), " ".join("%s %.2e" % kv for kv in errs.items())))
    mine = torch.cat([model.linear_bias.data, tr.bias_accum, tr.bias_linear])
    every = [torch.empty_like(mine) if dist.get_backend() == "nccl" else torch.empty(3) for _ in range(world)]
    dist.all_gather(every, mine if dist.get_backend() == "nccl" else mine.cpu())
    out.append(("bias_identical", all(torch.equal(e, every[0]) for e in every), ""))
    return out


def _worker(rank, world, store, transport, q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        import datetime
        import torch.distributed as dist
        if transport == "nccl":
            dev = torch.device("cuda", rank)
            torch.cuda.set_device(dev)
            dist.init_process_group("nccl", init_method="file://" + store, rank=rank, world_size=world, device_id=dev,
                                    timeout=datetime.timedelta(seconds=300))
        else:
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            os.environ["DIR_SHARD_HOST_STAGED"] = "1"                     # several ranks on ONE GPU: exchanges staged through host memory
            dev = torch.device("cuda", 0)
            torch.cuda.set_device(dev)
            dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
        try:
            import dir_amd
            dir_amd.load_library()
            res = _scenarios(rank, world, dev)
            torch.cuda.synchronize()
            q.put((rank, res))
        finally:
            dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


def _run(world, transport, timeout=300):
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = _store()
    procs = [ctx.Process(target=_worker, args=(r, world, store, transport, q)) for r in range(world)]      # fresh child processes
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=timeout))
    except queue.Empty:
        res = None
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()                      # the exact processes this test started
    return res


def _check(res, world):
    assert res is not None, "the ranks did not report within the time limit"
    assert sorted(r for r, _ in res) == list(range(world))
    for rank, got in res:
        assert not isinstance(got, str), "rank %d raised:\n%s" % (rank, got)
        print("rank %d: %s" % (rank, got))
        bad = [(n, d) for n, ok, d in got if not ok]
        assert not bad, "rank %d: %s" % (rank, bad)
        assert len(got) == 3


def test_linear_two_ranks_on_one_gpu(built_lib):
    """(f) two ranks on cuda:0 (gloo, host-staged exchanges)."""
    _check(_run(2, "gloo_same_device"), 2)


def test_linear_over_rccl_one_rank_per_gpu(built_lib):
    """(g) backend nccl (= RCCL), world = min(8, visible devices), one rank per GPU.  Skipped on a one-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL at world > 1 needs >= 2 visible GPUs (this box shows %d); the same scenarios run on one GPU over gloo" % n)
    world = min(8, n)
    _check(_run(world, "nccl"), world)
