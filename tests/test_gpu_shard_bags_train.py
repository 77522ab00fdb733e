"""Training through the row-sharded multi-hot bags on the GPU (ShardedTables.lookup_bags_train / ShardedDeepFMTrainer.step_bags with
the PRODUCT HIP backend: dir_shard_bags_grad_f32 + dir_sparse_adagrad_sorted_bags_f32).

  (a) world size 1 against float64 autograd + [TF-upstream] Adagrad: K in {6, 8, 12, 16, 64, 256} (6 and 12 leave idle lanes in a
      row's lane group), every combiner with and without weights and max_norm, PRUNE_NONPOSITIVE_WEIGHTS, both layouts; skewed ids (a
      Zipf slot, one row hit > 600 times -- its run crosses sort tiles and goes through the carry / fix path) and a bag of > 256 entries;
      one row named by more than 3000 entries of a batch of 4096 bags;
  (b) world size 1 against the single-GPU path: autograd.embedding_bag + torch.optim.Adagrad(eps=0) on its sparse gradients;
  (c) two ranks on cuda:0 over host-staged gloo: a direct lookup_bags_train step with a row hot on every rank, then three
      ShardedDeepFMTrainer.step_bags steps against a float64 single-process run of the same global batches (tables, accumulators,
      dense parameters) and predict_bags on the trained model;
  (d) the same over RCCL with one rank per GPU (skipped with a reason on a one-GPU box)."""
import os

import numpy as np
import pytest
import torch

from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr
from tests.test_shard_bags_train_gloo import adagrad64, bags_forward64, ref_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, ACC0 = 0.3, 0.1


def _store():
    import tempfile
    return os.path.join(tempfile.mkdtemp(prefix="dir_pg_"), "store")


def _dev(v, o, w, device):
    return (torch.from_numpy(v).to(device), torch.from_numpy(o).to(device), None if w is None else torch.from_numpy(w).to(device))


def _close(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else got
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max()) if got.size else 0.0


def _skewed_bags(rng, B, vocab, hot_row, zipf_slot, long_bag):
    """Slot zipf_slot: Zipf-distributed ids; slot 1: bags of 0..8 entries, one row in most of them (> 600 hits over the batch); one bag of
    long_bag entries in slot 2."""
    bags = draw_bags(rng, B, vocab, [20, 8, 12], "pos")
    for b in range(B):
        ids, w = bags[b][zipf_slot]
        z = np.minimum(rng.zipf(1.3, size=len(ids)) - 1, vocab[zipf_slot] - 1)
        bags[b][zipf_slot] = (z.astype(np.int64), w)
        ids, w = bags[b][1]
        if len(ids):
            ids[0] = hot_row
        if len(ids) > 3:
            ids[3] = hot_row
    L = long_bag
    bags[0][2] = (rng.integers(0, vocab[2], size=L).astype(np.int64), rng.uniform(0.1, 2.0, size=L).astype(np.float32))
    return bags


def _train_once(st, bags, F, case, G, device):
    from dir_amd import ops
    wmode, comb, mn, fmaj, prune = case
    v, o, w = _dev(*to_csr(bags, F, fmaj), device)
    kw = dict(combiner=comb, max_norm=mn, field_major=fmaj, flags=ops.PRUNE_NONPOSITIVE_WEIGHTS if prune else 0)
    want, _ = st.lookup_bags(v, o, w, **kw)
    emb = st.lookup_bags_train(v, o, w, **kw)
    same = bool(torch.equal(emb.detach(), want))
    emb.backward(G.to(device))
    return same


def test_world1_matches_float64(built_lib):
    """(a) world size 1 against float64: every K class, every case, then skewed ids through the carry / fix path."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = [500, 1000, 7]
    F = len(vocab)
    rng = np.random.default_rng(11)
    bad = []
    for K in (6, 8, 12, 16, 64, 256):
        full = [(rng.standard_normal((v, K)) * 0.5 / np.sqrt(K / 8.0)).astype(np.float32) for v in vocab]
        st = ShardedTables.from_full([torch.from_numpy(t).to(dev) for t in full]).enable_training(LR, ACC0)
        ref = [t.astype(np.float64) for t in full]
        acc = [np.full(t.shape, ACC0) for t in full]
        for c, case in enumerate(CASES):
            B = (37, 300, 0, 64, 129)[c]
            bags = draw_bags(rng, B, vocab, [60, 1, 3], case[0])
            G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32))
            same = _train_once(st, bags, F, case, G, dev)
            ref_step(ref, acc, bags, G.numpy(), case[1], case[2], case[4], LR)
            et = max(_close(st.local_tables[f], ref[f]) for f in range(F))
            ea = max(_close(st.optimizer.accums[f], acc[f]) for f in range(F))
            if not (same and et <= 1e-5 and ea <= 1e-5):
                bad.append((K, c, same, et, ea))
        assert st._updates == len(CASES)
    # skewed ids: a Zipf slot, one row hit > 600 times, a bag of 300 entries; max_norm on the hot slot, with and without weights' prune
    for K in (16, 64):
        vocab = [5000, 2000, 800]
        full = [(rng.standard_normal((v, K)) * 0.3).astype(np.float32) for v in vocab]
        st = ShardedTables.from_full([torch.from_numpy(t).to(dev) for t in full]).enable_training(LR, ACC0)
        ref = [t.astype(np.float64) for t in full]
        acc = [np.full(t.shape, ACC0) for t in full]
        for step, case in enumerate([("pos", ["mean", "sum", "sqrtn"], [None, 1.2, None], False, False),
                                     ("pos", ["sqrtn", "mean", "sum"], None, True, False)]):
            B = 1500
            bags = _skewed_bags(rng, B, vocab, 17, 0, 300)
            hits = sum(int((bg[1][0] == 17).sum()) for bg in bags)
            assert hits > 600, hits
            G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32))
            same = _train_once(st, bags, F, case, G, dev)
            ref_step(ref, acc, bags, G.numpy(), case[1], case[2], case[4], LR)
            et = max(_close(st.local_tables[f], ref[f]) for f in range(F))
            ea = max(_close(st.optimizer.accums[f], acc[f]) for f in range(F))
            if not (same and et <= 1e-5 and ea <= 1e-5):
                bad.append(("skew", K, step, same, et, ea))
    assert not bad, bad


def _hot_bags(rng, B, vocab, hot_row, hits):
    """Short bags (slot 1: exactly one entry); `hits` of slot 1's bags name hot_row."""
    bags = draw_bags(rng, B, vocab, [3, 1, 2], "pos")
    for b in rng.permutation(B)[:hits]:
        bags[b][1][0][0] = hot_row
    return bags


def test_world1_hot_row_matches_float64(built_lib):
    """3200 of 4096 bags name one row: its run spans more than twelve sort tiles, in the order the slab's atomics left the entries -- not
    the same from run to run -- so the bar must hold for any order.  Three steps (weights, max_norm on the hot slot, both layouts), K = 16
    and 64: tables and accumulators within 1e-5 of float64."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, B = [5000, 2000, 800], 4096
    F = len(vocab)
    rng = np.random.default_rng(41)
    bad = []
    for K in (16, 64):
        full = [(rng.standard_normal((v, K)) * 0.3).astype(np.float32) for v in vocab]
        st = ShardedTables.from_full([torch.from_numpy(t).to(dev) for t in full]).enable_training(LR, ACC0)
        ref = [t.astype(np.float64) for t in full]
        acc = [np.full(t.shape, ACC0) for t in full]
        for step, case in enumerate([("pos", ["mean", "sum", "sqrtn"], [None, 1.2, None], False, False),
                                     ("pos", ["sqrtn", "mean", "sum"], None, True, False),
                                     ("pos", "sum", None, False, False)]):
            bags = _hot_bags(rng, B, vocab, 17, 3200)
            hits = sum(int((bg[1][0] == 17).sum()) for bg in bags)
            assert hits >= 3000, hits
            G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32))
            same = _train_once(st, bags, F, case, G, dev)
            ref_step(ref, acc, bags, G.numpy(), case[1], case[2], case[4], LR)
            et = max(_close(st.local_tables[f], ref[f]) for f in range(F))
            ea = max(_close(st.optimizer.accums[f], acc[f]) for f in range(F))
            print("hot row K=%d step %d (%d entries): tables %.2e accumulators %.2e" % (K, step, hits, et, ea))
            if not (same and et <= 1e-5 and ea <= 1e-5):
                bad.append((K, step, same, et, ea))
    assert not bad, bad


def test_world1_matches_single_gpu_embedding_bag_training(built_lib):
    """(b) the same bags trained by the single-GPU path (autograd.embedding_bag's sparse gradients + torch.optim.Adagrad, eps = 0)."""
    from dir_amd import autograd as ag
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = [400, 900, 7]
    F = len(vocab)
    rng = np.random.default_rng(12)
    bad = []
    for K in (8, 64):
        full = [(rng.standard_normal((v, K)) * 0.5).astype(np.float32) for v in vocab]
        st = ShardedTables.from_full([torch.from_numpy(t).to(dev) for t in full]).enable_training(LR, ACC0)
        params = [torch.nn.Parameter(torch.from_numpy(t).to(dev)) for t in full]
        ts = ops.TableSet([p.data for p in params])
        opt = torch.optim.Adagrad(params, lr=LR, initial_accumulator_value=ACC0, eps=0.0)
        for c, case in enumerate([cs for cs in CASES if not cs[4]] * 2):          # (the single-GPU backward takes no prune flag)
            wmode, comb, mn, fmaj, _ = case
            B = 90 + 13 * c
            bags = draw_bags(rng, B, vocab, [40, 1, 5], wmode)
            G = torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev)
            _train_once(st, bags, F, case, G, dev)
            v, o, w = _dev(*to_csr(bags, F, fmaj), dev)
            opt.zero_grad(set_to_none=True)
            out = ag.embedding_bag(ts, v, params, o, w, combiner=comb, field_major=fmaj, max_norm=mn)
            out.backward(G)
            opt.step()
            ops.invalidate_caches()
            for f in range(F):
                e = _close(st.local_tables[f], params[f].detach().double().cpu().numpy())
                ea = _close(st.optimizer.accums[f], opt.state[params[f]]["sum"].double().cpu().numpy())
                if not (e <= 1e-5 and ea <= 1e-5):
                    bad.append((K, c, f, e, ea))
    assert not bad, bad


# ---- several ranks -------------------------------------------------------------------------------------------------------------------
def _scenarios(rank, world, device):
    import torch.distributed as dist
    from dir_amd.shard import ShardedTables, ShardedDeepFMTrainer
    from dir_amd import feature_column as fc
    from dir_amd.deepfm import DeepFM
    out = []
    vocab, K = [700, 2000, 3], 16                                    # (3 rows: a table barely larger than the world)
    F = len(vocab)
    # 1. one lookup_bags_train step, a row hot on every rank, prune + per-slot max_norm, uneven batches (one of them empty)
    rng = np.random.default_rng(77)
    full = [(rng.standard_normal((v, K)) * 0.3).astype(np.float32) for v in vocab]
    st = ShardedTables.from_full([torch.from_numpy(t).to(device) for t in full]).enable_training(LR, ACC0)
    ref = [t.astype(np.float64) for t in full]
    acc = [np.full(t.shape, ACC0) for t in full]
    ok = True
    for step, case in enumerate([CASES[2], CASES[1]]):
        g = np.random.default_rng(900 + step)
        Bs = [41 + 17 * r if (r + step) % 2 == 0 else (0 if r == world - 1 else 9) for r in range(world)]
        bags_all = [draw_bags(g, Bs[r], vocab, [40, 1, 3], case[0]) for r in range(world)]
        for bl in bags_all:
            for row in bl:
                if len(row[0][0]) > 1:
                    row[0][0][:2] = 5                                # row 5 of slot 0: repeated in bags, across bags and ranks
        G_all = [g.standard_normal((Bs[r], F * K)).astype(np.float32) for r in range(world)]
        same = _train_once(st, bags_all[rank], F, case, torch.from_numpy(G_all[rank]), device)
        ref_step(ref, acc, [b for bl in bags_all for b in bl], np.concatenate(G_all, axis=0), case[1], case[2], case[4], LR)
        from dir_amd.shard import local_slice
        sl = [slice(*local_slice(v, world, 0, world, rank)) for v in vocab]
        et = max(_close(st.local_tables[f], ref[f][sl[f]]) for f in range(F))
        ea = max(_close(st.optimizer.accums[f], acc[f][sl[f]]) for f in range(F))
        ok = ok and same and et <= 1e-5 and ea <= 1e-5
        out.append(("lookup_bags_train_step%d" % step, same and et <= 1e-5 and ea <= 1e-5, "tables %.2e accums %.2e" % (et, ea)))

    # 2. ShardedDeepFMTrainer.step_bags x 3 against a float64 single-process run, then predict_bags
    B, steps = 48, 3
    combs, mns = ["mean", "sqrtn", "sum"], [None, 0.8, None]
    cats = [fc.categorical_column_with_identity("C%d" % i, v) for i, v in enumerate(vocab)]
    torch.manual_seed(7)                                             # the same model on every rank
    cols = [fc.embedding_column(c, K, combiner=cb, max_norm=mn) for c, cb, mn in zip(cats, combs, mns)]
    model = DeepFM(linear_feature_columns=[], dnn_feature_columns=cols, dnn_hidden_units=[16, 16], fm_embedding_size=K).to(device)
    full = [p.detach().clone() for p in model.embedding_weights]
    stt = ShardedTables.from_full(full)
    dense = [p for n, p in model.named_parameters() if not n.startswith(("embedding_weights", "linear_weights"))]
    names = [n for n, _ in model.named_parameters() if not n.startswith(("embedding_weights", "linear_weights"))]
    opt = torch.optim.Adagrad(dense, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    tr = ShardedDeepFMTrainer(model, stt, lr_sparse=0.05, dense_optimizer=opt)
    t64 = [t.double().cpu().numpy().copy() for t in full]
    acc64 = [np.full(t.shape, 0.1) for t in t64]
    d64 = [p.detach().double().cpu().clone().requires_grad_(True) for p in dense]
    dacc = [torch.full_like(p, 0.1) for p in d64]
    pd = dict(zip(names, d64))

    def model64(T, bags):
        emb = bags_forward64(T, bags, combs, mns, False)
        e3 = emb.view(-1, F, K)
        fm = 0.5 * ((e3.sum(1) ** 2) - (e3 ** 2).sum(1)).sum(1, keepdim=True)
        net = emb
        for i in range(2):
            net = torch.relu(net @ pd["hidden.%d.weight" % i].t() + pd["hidden.%d.bias" % i])
        return fm + net @ pd["logits_layer.weight"].t() + pd["logits_layer.bias"]
    for s in range(steps):
        g = np.random.default_rng(1000 + s)
        bags_all = [draw_bags(g, B, vocab, [12, 1, 3], "pos") for _ in range(world)]
        lab_all = g.integers(0, 2, size=(world * B, 1)).astype(np.float64)
        v, o, w = _dev(*to_csr(bags_all[rank], F, s % 2 == 1), device)
        tr.step_bags(v, o, torch.from_numpy(lab_all[rank * B:(rank + 1) * B]).float().to(device), weights=w, field_major=s % 2 == 1)
        T = [torch.from_numpy(t).requires_grad_(True) for t in t64]
        logit = model64(T, [b for bl in bags_all for b in bl])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, torch.from_numpy(lab_all), reduction="sum")
        grads = torch.autograd.grad(loss, T + d64, allow_unused=True)
        adagrad64(t64, acc64, [None if gr is None else gr.numpy() for gr in grads[:F]], 0.05)
        with torch.no_grad():
            for p, a, gr in zip(d64, dacc, grads[F:]):
                if gr is not None:
                    a += gr ** 2
                    p -= 0.05 * gr / a.sqrt()
    from dir_amd.shard import local_slice
    sl = [slice(*local_slice(v, world, 0, world, rank)) for v in vocab]
    et = max(_close(stt.local_tables[f], t64[f][sl[f]]) for f in range(F))
    ea = max(_close(stt.optimizer.accums[f], acc64[f][sl[f]]) for f in range(F))
    ed = max(_close(p, r.detach().numpy()) for p, r in zip(dense, d64))
    out.append(("step_bags", et <= 2e-5 and ea <= 2e-5 and ed <= 2e-5, "tables %.2e accums %.2e dense %.2e" % (et, ea, ed)))
    v, o, w = _dev(*to_csr(bags_all[rank], F, False), device)
    got = tr.predict_bags(v, o, w)
    with torch.no_grad():
        want = model64([torch.from_numpy(t) for t in t64], bags_all[rank]).numpy()
    ep = _close(got, want)
    out.append(("predict_bags", got.shape == (B, 1) and ep <= 1e-4, "err=%.2e" % ep))
    ones = torch.ones(1, device=device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(ones)
    out.append(("ranks_seen", int(ones.item()) == world, "seen=%d" % int(ones.item())))
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


def _run(world, transport, timeout=420):
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = _store()
    procs = [ctx.Process(target=_worker, args=(r, world, store, transport, q)) for r in range(world)]
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
        bad = [(n, d) for n, ok, d in got if not ok]
        assert not bad, "rank %d: %s" % (rank, bad)
        assert len(got) == 5


def test_bags_train_two_ranks_on_one_gpu(built_lib):
    """(c) two ranks on cuda:0 (gloo, host-staged exchanges)."""
    _check(_run(2, "gloo_same_device"), 2)


def test_bags_train_over_rccl_one_rank_per_gpu(built_lib):
    """(d) backend nccl (= RCCL), world = min(8, visible devices), one rank per GPU.  Skipped on a one-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL at world > 1 needs >= 2 visible GPUs (this box shows %d); the same scenarios run on one GPU over gloo" % n)
    world = min(8, n)
    _check(_run(world, "nccl"), world)
