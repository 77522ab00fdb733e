"""Row-sharded multi-hot bags on the GPU (ShardedTables.lookup_bags with the PRODUCT HIP backend: csrc/shard_bags.hip).

  * world size 1: bit for bit ops.embedding_bag on the same tables over bag lengths 0..60, pruned / out-of-vocabulary ids, per-slot
    combiners and max_norm, weights / no weights / PRUNE_NONPOSITIVE_WEIGHTS, both layouts, K in {8, 16, 64, 128}; the fused FM logit
    bit for bit ops.fm_logit of the result; a HIP-graph replay bit for bit the eager call.
  * two ranks on cuda:0 over gloo (exchanges staged through host memory, the harness of tests/test_gpu_shard_nccl.py): against
    ops.embedding_bag on the full tables (fp32 summation tolerance; bit for bit where every bag's live entries sit on one owner),
    repeatability, the overflow -> grown-capacity repeat, ShardedDeepFMTrainer.predict_bags against the single-process model.
  * the same scenarios over RCCL with one rank per GPU (skipped with a reason on a one-GPU box)."""
import os

import numpy as np
import pytest
import torch

from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _store():
    import tempfile
    return os.path.join(tempfile.mkdtemp(prefix="dir_pg_"), "store")


def _full(vocab, K, device, seed=99):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((v, K), generator=g) * 0.4).to(device) for v in vocab]


def _dev(v, o, w, device):
    return (torch.from_numpy(v).to(device), torch.from_numpy(o).to(device), None if w is None else torch.from_numpy(w).to(device))


def _both(st, ts, bags, F, case, device):
    """-> (sharded emb, sharded fm, ops.embedding_bag on the full tables)."""
    from dir_amd import ops
    wmode, comb, mn, fmaj, prune = case
    v, o, w = _dev(*to_csr(bags, F, fmaj), device)
    flags = ops.PRUNE_NONPOSITIVE_WEIGHTS if prune else 0
    emb, fm = st.lookup_bags(v, o, w, combiner=comb, max_norm=mn, field_major=fmaj, flags=flags, want_fm=True)
    ref = ops.embedding_bag(ts, v, o, w, combiner=comb, field_major=fmaj, flags=flags, max_norm=mn)
    return emb, fm, ref


def test_world1_bitwise_equals_embedding_bag(built_lib):
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = [500, 1000, 7]
    F = len(vocab)
    rng = np.random.default_rng(3)
    bad = []
    for K in (8, 16, 64, 128):
        full = _full(vocab, K, dev)
        st = ShardedTables.from_full(full)
        ts = ops.TableSet(full)
        for c, case in enumerate(CASES):
            for B in (37, 300, 0):
                bags = draw_bags(rng, B, vocab, [1, 60, 4], case[0])
                emb, fm, ref = _both(st, ts, bags, F, case, dev)
                ok = emb.shape == (B, F * K) and bool(torch.equal(emb, ref))
                ok = ok and (B == 0 or bool(torch.equal(fm, ops.fm_logit(emb, F, K))))
                if not ok:
                    bad.append((K, c, B))
    assert not bad, "lookup_bags differs from ops.embedding_bag (K, case, B): %s" % bad


def test_world1_graph_replay_equals_eager(built_lib):
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K = [300, 800, 20], 16
    F = len(vocab)
    full = _full(vocab, K, dev, seed=5)
    st = ShardedTables.from_full(full)
    rng = np.random.default_rng(11)
    bags = draw_bags(rng, 256, vocab, [1, 40, 3], "pos")
    v, o, w = _dev(*to_csr(bags, F, True), dev)
    kw = dict(combiner=["sum", "mean", "sqrtn"], max_norm=[None, 0.8, None], field_major=True, want_fm=True)
    e0, f0 = (t.clone() for t in st.lookup_bags(v, o, w, **kw))
    step = ops.CapturedStep(lambda: st.lookup_bags(v, o, w, **kw))
    step.replay()
    torch.cuda.synchronize()
    assert torch.equal(step.out[0], e0) and torch.equal(step.out[1], f0)
    # new ids and weights in the captured buffers (same nnz): the replay computes the new bags
    v2 = torch.from_numpy(rng.integers(-1, 300, size=v.numel())).to(dev)
    v.copy_(v2)
    w.copy_(torch.from_numpy(rng.uniform(0.1, 2.0, size=w.numel()).astype(np.float32)).to(dev))
    e1, f1 = (t.clone() for t in st.lookup_bags(v, o, w, **kw))
    step.replay()
    torch.cuda.synchronize()
    assert torch.equal(step.out[0], e1) and torch.equal(step.out[1], f1) and not torch.equal(e1, e0)


def test_world1_graph_replay_survives_plan_eviction(built_lib):
    """The plan a captured lookup writes through raw pointers stays alive when eager lookups at other nnz evict it from the plan cache:
    after five other batch shapes and fresh allocations of the sizes the freed blocks would have, the replay still equals the eager
    result, and nothing it writes lands in the new allocations."""
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K = [300, 800, 20], 16
    F = len(vocab)
    full = _full(vocab, K, dev, seed=6)
    st = ShardedTables.from_full(full)
    rng = np.random.default_rng(12)
    bags = draw_bags(rng, 128, vocab, [1, 40, 3], "pos")
    v, o, w = _dev(*to_csr(bags, F, False), dev)
    kw = dict(combiner="mean", max_norm=0.9, want_fm=True)
    e0, f0 = (t.clone() for t in st.lookup_bags(v, o, w, **kw))
    step = ops.CapturedStep(lambda: st.lookup_bags(v, o, w, **kw))
    key = next(iter(st._bag_plans))
    for L in (2, 100, 200, 400, 800):                                 # five other entry capacities: the cache (4 plans) drops the captured one
        b2 = draw_bags(rng, 128, vocab, [1, L, 3], "pos")
        e2, _, ref2 = _both(st, ops.TableSet(full), b2, F, ("pos", "mean", 0.9, False, False), dev)
        assert torch.equal(e2, ref2)
    assert key not in st._bag_plans
    torch.cuda.synchronize()
    fill = [torch.full((n,), 7, dtype=torch.int32, device=dev) for n in (256, 4096, 65536, 1 << 20) for _ in range(24)]
    for _ in range(2):
        step.replay()
    torch.cuda.synchronize()
    assert torch.equal(step.out[0], e0) and torch.equal(step.out[1], f0)
    assert all(bool((t == 7).all()) for t in fill)


# ---- several ranks ----------------------------------------------------------------------------------------------------------------
def _one_owner_bags(rng, B, vocab, world, max_len, rank_of):
    """Bags whose ids all lie in ONE owner's 'div' range (pruned ids mixed in): one partial row per bag, so the sharded result is the
    single-GPU one bit for bit."""
    from dir_amd.shard import div_range
    bags = []
    for b in range(B):
        row = []
        for f, v in enumerate(vocab):
            s, e = div_range(v, world, rank_of(b, f))
            L = int(rng.integers(0, max_len + 1))
            ids = rng.integers(s, max(e, s + 1), size=L).astype(np.int64) if e > s else np.full(L, -1, np.int64)
            ids[rng.random(L) < 0.1] = -1
            row.append((ids, rng.uniform(0.1, 2.0, size=L).astype(np.float32)))
        bags.append(row)
    return bags


def _scenarios(rank, world, device):
    import torch.distributed as dist
    from dir_amd import ops
    from dir_amd.shard import ShardedTables, ShardedDeepFMTrainer
    out = []
    rng = np.random.default_rng(500 + rank)                          # every rank draws its own bags
    vocab = [700, 2000, 3]                                           # (3 rows: a table barely larger than the world)
    F = len(vocab)

    def close(emb, ref):
        return bool(((emb - ref).abs() <= 2e-5 * (1 + ref.abs())).all())

    for K in (16, 64):
        full = _full(vocab, K, device, seed=K)
        ts = ops.TableSet(full)
        st = ShardedTables.from_full(full)
        assert st.P == world and type(st.backend).__name__ == "HipBackend"
        # 1. the matrix against the full tables; uneven local batches, one of them empty
        ok, det = True, []
        for c, case in enumerate(CASES):
            B = [41 + 17 * rank, 0 if rank == world - 1 else 9][c % 2]
            bags = draw_bags(rng, B, vocab, [60, 1, 3], case[0])
            emb, fm, ref = _both(st, ts, bags, F, case, device)
            good = emb.shape == (B, F * K) and close(emb, ref) and (B == 0 or close(fm, ops.fm_logit(ref, F, K)))
            ok = ok and good
            det.append("c%d:%s" % (c, good))
        out.append(("matrix_K%d" % K, ok, " ".join(det)))
        # 2. every bag's live entries on one owner: bit for bit
        bags = _one_owner_bags(rng, 64 + rank, vocab, world, 30, lambda b, f: (b + f) % world)
        case = ("pos", ["mean", "sqrtn", "sum"], [None, 0.9, None], False, False)
        emb, fm, ref = _both(st, ts, bags, F, case, device)
        out.append(("one_owner_bitwise_K%d" % K, bool(torch.equal(emb, ref)) and bool(torch.equal(fm, ops.fm_logit(ref, F, K))), ""))
        # 3. two identical lookups: identical bits
        bags = draw_bags(rng, 80, vocab, [50, 1, 3], "pos")
        e1, f1, _ = _both(st, ts, bags, F, CASES[1], device)
        e1, f1 = e1.clone(), f1.clone()
        e2, f2, _ = _both(st, ts, bags, F, CASES[1], device)
        out.append(("repeatable_K%d" % K, bool(torch.equal(e1, e2)) and bool(torch.equal(f1, f2)), ""))
        del st

    # 4. slabs too small: the verdict is read off the received headers, the lookup repeated with grown capacities
    K = 16
    full = _full(vocab, K, device, seed=3)
    ts = ops.TableSet(full)
    sto = ShardedTables.from_full(full, slack=0.02)
    ok = True
    for rep in range(3):
        bags = draw_bags(rng, 120, vocab, [40, 1, 3], None)
        emb, fm, ref = _both(sto, ts, bags, F, CASES[0], device)
        ok = ok and close(emb, ref)
    fb = sto.stats.get("bag_fallbacks", 0)
    out.append(("overflow_grows", ok and 1 <= fb < 3, "fallbacks=%d caps=%s" % (fb, sto.stats.get("bag_cap"))))

    # 5. ShardedDeepFMTrainer.predict_bags against the single-process FM + DNN over ops.embedding_bag on the full tables
    from dir_amd.deepfm import DeepFM
    from dir_amd import feature_column as fc
    torch.manual_seed(4242)                                          # the same model on every rank
    cats = [fc.categorical_column_with_identity("C%d" % i, v) for i, v in enumerate(vocab)]
    cols = [fc.embedding_column(c, K, combiner=cb) for c, cb in zip(cats, ["mean", "sqrtn", "sum"])]
    m = DeepFM(linear_feature_columns=cats, dnn_feature_columns=cols, dnn_hidden_units=[64, 32], fm_embedding_size=K).to(device)
    stp = ShardedTables.from_full(full)
    tr = ShardedDeepFMTrainer(m, stp, 0.05, torch.optim.Adagrad([p for n, p in m.named_parameters() if "embedding" not in n], lr=0.01))
    bags = draw_bags(rng, 200 + 7 * rank, vocab, [30, 1, 3], "pos")
    v, o, w = _dev(*to_csr(bags, F, True), device)
    got = tr.predict_bags(v, o, w, field_major=True)
    with torch.no_grad():
        m.eval()
        emb = ops.embedding_bag(ts, v, o, w, combiner=[c.combiner for c in cols], field_major=True)
        want = m.dnn_logit_fn(emb, adds=(ops.fm_logit(emb, F, K),), range_ok=ops.f16_range_ok(ts.absmax()))
    err = float(((got - want).abs() / (1 + want.abs())).max())
    out.append(("predict_bags", got.shape == want.shape and err <= 1e-4, "err=%.2e" % err))

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
        assert len(got) == 9


def test_bags_over_rccl_one_rank_per_gpu(built_lib):
    """backend nccl (= RCCL), world = min(8, visible devices), one rank per GPU.  Skipped on a one-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL at world > 1 needs >= 2 visible GPUs (this box shows %d); the same scenarios run on one GPU over gloo" % n)
    world = min(8, n)
    _check(_run(world, "nccl"), world)


def test_bags_two_ranks_on_one_gpu(built_lib):
    """The scenarios with two ranks on cuda:0 (gloo, host-staged exchanges)."""
    _check(_run(2, "gloo_same_device"), 2)
