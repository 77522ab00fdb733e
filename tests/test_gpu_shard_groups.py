"""Row groups and units > 1 on the row-sharded tables, on the GPU with the PRODUCT HIP backend (ShardedTables(groups=G),
attach_linear([rows, U]), ShardedESMMTrainer: dir_shard_finish_groups_f32, dir_shard_grad_groups_f32, dir_shard_linear_gather_units_f32,
dir_shard_linear_finish_units_f32, dir_shard_linear_grad_units_f32, dir_sparse_ftrl_rows_units_sorted_payload_f32).

  (a) world size 1, forward: group g's output is ShardedTables.from_full(tables_g).lookup(ids) bit for bit (a pure copy) for (G, K) in
      {(2, 16), (2, 8), (3, 4)}, F in {1, 3, 26}, B in {0, 1, 37, 4096}, pruned ids, de-duplicated, exact path; lin[:, u] is ops.linear_logit
      over unit u's unsharded packed rows bit for bit (U in {2, 3}, with and without bias); G = 1 / U = 1 give today's results;
  (b) world size 1, training, five steps against float64 (per group Adagrad, per unit FTRL), uniform and skewed ids, one row hit 3000
      times in a batch of 4096; the FTRL on the
      Adagrad step's sort against the FTRL on its own sort, bit for bit;
  (c) the gradient kernel: the buffer the owner receives equals the NumPy stand-in's, zero wherever no entry points -- over poisoned memory;
  (d) a captured grouped lookup(want_lin=True) replays the eager result bitwise after a training step;
  (e) two ranks on cuda:0 over host-staged gloo: forward still bitwise per group; ShardedESMMTrainer two steps + predict against the float64
      model of the global batch; the same over RCCL with one rank per GPU (skipped with a reason on a one-GPU box);
  (f) what grouped tables do not cover raises NotImplementedError before any launch.
Error measure (tests/test_gpu_shard_linear.py): max |got - ref| / (1 + |ref|) against float64, bar 1e-5."""
import os

import numpy as np
import pytest
import torch

from tests.shard_standin_groups import grad_groups_np
from tests.test_shard_groups_gloo import ACC0, LR, Reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5


def _close(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else got
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max()) if got.size else 0.0


def _draw(vocab, K, G, U, seed, dev):
    rng = np.random.default_rng(seed)
    full_g = [[torch.from_numpy(rng.standard_normal((v, K)).astype(np.float32)).to(dev) for v in vocab] for _ in range(G)]
    full_w = [torch.from_numpy((0.3 * rng.standard_normal((v, U))).astype(np.float32)).to(dev) for v in vocab]
    return full_g, full_w


def _ids(rng, vocab, B, dev, lo=-2, over=2):
    a = np.stack([rng.integers(lo, v + over, size=B) for v in vocab], axis=1).astype(np.int64).reshape(B, len(vocab))
    return torch.from_numpy(a).to(dev)


def _vocab(F):
    return [500, 1000, 7][:F] if F <= 3 else [200 + 37 * i for i in range(F)]


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 26])
@pytest.mark.parametrize("G,K,U", [(2, 16, 2), (2, 8, 3), (3, 4, 2)])
def test_world1_forward_bitwise_per_group_and_unit(built_lib, G, K, U, F):
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = _vocab(F)
    full_g, full_w = _draw(vocab, K, G, U, 3 + F + G, dev)
    rows_u = [ops.TableSet.ftrl_rows([w[:, u].contiguous() for w in full_w]) for u in range(U)]
    plain = [ShardedTables.from_full(full_g[g]) for g in range(G)]
    bias = torch.tensor([0.37, -1.25, 0.5][:U], dtype=torch.float32, device=dev)
    rng = np.random.default_rng(17)
    for kw in ({}, {"dedup": True}, {"mode": "exact"}):
        st = ShardedTables.from_full_groups(full_g, **kw).attach_linear_from_full(full_w)
        assert st.G == G and st.K == K and st.U == U and tuple(st.local_tables[0].shape) == (vocab[0], G * K)
        for B in (1, 37, 4096, 0):
            ids = _ids(rng, vocab, B, dev)
            for b in (bias, None):
                embs, lin = st.lookup(ids, want_lin=True, lin_bias=b)
                torch.cuda.synchronize()
                assert isinstance(embs, tuple) and len(embs) == G and tuple(lin.shape) == (B, U)
                for g in range(G):
                    assert tuple(embs[g].shape) == (B, F * K)
                    assert torch.equal(embs[g], plain[g].lookup(ids)), (kw, B, g)
                if B == 0:                                                  # (the single-GPU linear kernel takes no empty batch)
                    continue
                for u in range(U):
                    want = ops.linear_logit(rows_u[u], ids, bias=None if b is None else b[u:u + 1].contiguous())
                    assert torch.equal(lin[:, u:u + 1], want), (kw, B, u, b is not None)
            alone = st.lookup(ids)
            assert isinstance(alone, tuple) and all(torch.equal(a, e) for a, e in zip(alone, embs))


def test_world1_one_group_one_unit_is_todays_lookup(built_lib):
    """groups = 1 and [rows, 1] weights: one tensor [B, F*K] and lin [B, 1], bitwise what from_full / attach_linear_from_full give."""
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K = _vocab(3), 16
    full_g, full_w = _draw(vocab, K, 1, 1, 5, dev)
    ids = _ids(np.random.default_rng(2), vocab, 37, dev)
    a = ShardedTables.from_full_groups(full_g).attach_linear_from_full(full_w)
    b = ShardedTables.from_full(full_g[0]).attach_linear_from_full([w[:, 0] for w in full_w])
    assert a.G == 1 and a.U == 1
    ea, la = a.lookup(ids, want_lin=True)
    eb, lb = b.lookup(ids, want_lin=True)
    torch.cuda.synchronize()
    assert isinstance(ea, torch.Tensor) and torch.equal(ea, eb) and tuple(la.shape) == (37, 1) and torch.equal(la, lb)
    assert torch.equal(la, ops.linear_logit(ops.TableSet.ftrl_rows([w[:, 0].contiguous() for w in full_w]), ids))
    assert all(tuple(w.shape) == (v,) for w, v in zip(a.linear_weights(), vocab))


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
def _train(st, ids, Gs, g):
    embs, lin = st.lookup_train(ids, with_linear=True)
    (sum((e * G).sum() for e, G in zip(embs, Gs)) + (lin * g).sum()).backward()


def _state_errs(st, ref):
    errs = {}
    F = st.F
    for g in range(st.G):
        errs["emb%d" % g] = max(_close(st.group_tables(g)[f], ref.T[g][f]) for f in range(F))
        errs["acc%d" % g] = max(_close(st.group_accums(g)[f], ref.acc[g][f]) for f in range(F))
    w, n, z = st.linear_state()
    for u in range(st.U):
        for name, got, want in (("w", w, ref.w), ("n", n, ref.n), ("z", z, ref.z)):
            errs["%s%d" % (name, u)] = max(_close(got[f][:, u], want[u][f][:, 0]) for f in range(F))
    return errs


def _run_training(l1, l2, make_ids, G=2, K=16, U=2, steps=5, seed=5, B=1500, gscale=1.0):
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = [500, 1000, 7]
    F = len(vocab)
    full_g, full_w = _draw(vocab, K, G, U, seed, dev)
    ftrl = dict(lr=0.2, l1=l1, l2=l2)
    st = ShardedTables.from_full_groups([[t.clone() for t in tg] for tg in full_g]).attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(**ftrl)
    ref = Reference([[t.cpu().numpy() for t in tg] for tg in full_g], [w.cpu().numpy() for w in full_w])
    rng = np.random.default_rng(23)
    for step in range(steps):
        ids = make_ids(rng, vocab, B, dev)
        Gs = [torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev) for _ in range(G)]
        g = torch.from_numpy((rng.standard_normal((B, U)) * gscale).astype(np.float32)).to(dev)
        _train(st, ids, Gs, g)
        ref.step(ids.cpu().numpy(), [x.cpu().numpy() for x in Gs], g.cpu().numpy(), ftrl)
        errs = _state_errs(st, ref)
        print("step %d l1=%g l2=%g: %s" % (step, l1, l2, " ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
        assert all(v <= BAR for v in errs.values()), (step, errs)
    return st


@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (0.05, 0.1)])
def test_world1_training_matches_float64(built_lib, l1, l2):
    """Uniform ids (pruned ones included) over vocab = [500, 1000, 7], B = 1500, five steps: every group's tables and accumulators and
    every unit's w, n, z within 1e-5 of float64; with l1 > 0 some touched weight is exactly 0.0.
    The 7-row table is the hard part: a row takes ~140 hits per step, and z_prev + g can cancel to O(0.1) against summed gradients of
    O(10), where the measure's 1 + |ref| no longer covers the summands.  A plain fp32 run sum (off by 1e-6 to 2.2e-5 for those 144 values,
    depending on the order the slab's atomics left) read 1.5e-5 to 2.1e-5 there in about half the runs; the sorted updates compensate
    their run sums (csrc/backward.hip: run_sum) and read 1.1e-6 to 2.4e-6."""
    st = _run_training(l1, l2, _ids)
    if l1 > 0:
        assert any(bool((w == 0).any()) for w in st.linear_weights()), "l1 clips some touched weights to exactly 0.0"


def _skewed(rng, vocab, B, dev):
    a = np.stack([rng.integers(0, v, size=B) for v in vocab], axis=1).astype(np.int64)
    a[rng.permutation(B)[:700], 1] = 321                                  # one row in most of the batch: its run crosses sort tiles
    return torch.from_numpy(a).to(dev)


def test_world1_training_skewed_ids_match_float64(built_lib):
    """One row hit 700 times in a batch of 1500 (the carry / fix path of the sorted update at width G*K and at K = U)."""
    _run_training(0.05, 0.1, _skewed, steps=3, seed=7)


def _hot(rng, vocab, B, dev):
    a = np.stack([rng.integers(0, v, size=B) for v in vocab], axis=1).astype(np.int64)
    a[rng.permutation(B)[:3000], 1] = 321
    return torch.from_numpy(a).to(dev)


def test_world1_training_hot_row_matches_float64(built_lib):
    """One row hit 3000 times in a batch of 4096 (a run over twelve sort tiles, at width G*K and at K = U), three steps, every state within
    1e-5 -- in whatever order the slab's atomics left the run's entries.  (d lin is drawn at 0.3: the row's summed gradient, sigma ~ 16,
    stays below 64, where fp32's own rounding of the sum is under 4e-6.)"""
    _run_training(0.05, 0.1, _hot, steps=3, seed=11, B=4096, gscale=0.3)


@pytest.mark.parametrize("U", [2, 3, 4, 8])
def test_owner_ftrl_units_on_its_own_sort_equals_on_the_adagrad_sort(built_lib, U):
    """The units FTRL on the Adagrad step's sort (sorted_by) against the units FTRL that sorts for itself: BITWISE equal.  Reading
    sparse_sorted_update (csrc/backward.hip): with sorted_from the tile pass reads the pair arrays k1 / v1 of the other workspace; without
    it the same key pass (adagrad_keys_payload_k: the keys depend on payload, row_base and total_rows only) and the same stable radix sort
    (its digit passes depend on n and the key bits, i.e. total_rows, only) produce those arrays for itself -- neither depends on the row
    width K -- so the runs, their order and every sum are the same.  U = 4 and 8 take the 16-byte gradient loads (four units per lane)."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, G, n = [500, 1000, 7], 16, 2, 6000
    F = len(vocab)
    full_g, full_w = _draw(vocab, K, G, U, 53, dev)
    rng = np.random.default_rng(59)
    slot = rng.integers(0, F, size=n)
    row = np.array([rng.integers(0, vocab[f]) for f in slot])
    row[:800] = 11                                                         # runs that cross sort tiles
    slot[:800] = 1
    pay = row * F + slot
    pay[rng.permutation(n)[:100]] = -1
    payload = torch.from_numpy(pay.astype(np.int64)).to(dev)
    grows = torch.from_numpy(rng.standard_normal((n, G * K)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((n, U)).astype(np.float32)).to(dev)
    sts = []
    for reuse in (True, False):
        st = ShardedTables.from_full_groups([[t.clone() for t in tg] for tg in full_g]).attach_linear_from_full(full_w, ACC0)
        st.enable_training(LR, ACC0).enable_linear_training(0.2, 0.01, 0.02)
        be = st.backend
        if reuse:
            be.apply_adagrad(st.optimizer, payload, grows)
            be.apply_ftrl(payload, g, 0.2, 0.01, 0.02, sorted_by=st.optimizer)
        else:
            be.apply_ftrl(payload, g, 0.2, 0.01, 0.02)
            be.apply_adagrad(st.optimizer, payload, grows)
        sts.append(st)
    torch.cuda.synchronize()
    # ... and both against float64 (one step from the initial state)
    ref = Reference([[t.cpu().numpy() for t in tg] for tg in full_g], [w.cpu().numpy() for w in full_w])
    ok = pay >= 0
    for u in range(U):
        for f in range(F):
            sel = ok & (pay % F == f)
            gs = np.zeros(vocab[f])
            np.add.at(gs, pay[sel] // F, g.cpu().numpy().astype(np.float64)[sel, u])
            t = np.zeros(vocab[f], bool)
            t[pay[sel] // F] = True
            w0, n0, z0 = ref.w[u][f][:, 0], ref.n[u][f][:, 0], ref.z[u][f][:, 0]
            n1 = n0 + gs * gs
            z1 = z0 + gs - (np.sqrt(n1) - np.sqrt(n0)) / 0.2 * w0
            w1 = np.where(np.abs(z1) > 0.01, (np.sign(z1) * 0.01 - z1) / (np.sqrt(n1) / 0.2 + 2 * 0.02), 0.0)
            got = sts[0].lin_rows[f]
            assert _close(got[:, 4 * u], np.where(t, w1, w0)) <= BAR and _close(got[:, 4 * u + 1], np.where(t, n1, n0)) <= BAR
            assert _close(got[:, 4 * u + 2], np.where(t, z1, z0)) <= BAR
    for f in range(F):
        assert torch.equal(sts[0].lin_rows[f], sts[1].lin_rows[f]), f
        assert torch.equal(sts[0].local_tables[f], sts[1].local_tables[f]), f
        assert not torch.equal(sts[0].lin_rows[f][:, 0], full_w[f][:, 0])


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,K,F,B", [(2, 16, 3, 37), (3, 4, 26, 300), (2, 8, 1, 1)])
def test_gradient_kernel_fills_the_owner_buffer_like_the_stand_in(built_lib, G, K, F, B):
    """lookup_train + backward with known gradients at world 1: the [P*cap, G*K] buffer handed to the owner's update equals the NumPy
    transpose of the grouped finish, and every position no entry names (pruned entries, the slab's padding) is 0.0 -- although the buffer's
    block held NaN bytes before (blocks of its size are filled with 0xFF and handed back to the caching allocator first)."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = _vocab(F)
    full_g, _ = _draw(vocab, K, G, 1, 9, dev)
    st = ShardedTables.from_full_groups(full_g).enable_training(LR, ACC0)
    rng = np.random.default_rng(13)
    ids = _ids(rng, vocab, B, dev)
    if B > 1:
        ids[0, 0], ids[B - 1, F - 1] = -1, vocab[F - 1]                    # pruned entries for sure: below 0 and past the vocabulary
    Gs = [torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev) for _ in range(G)]
    seen = []
    st.backend.apply_adagrad = lambda opt, pay, grows: seen.append((pay.clone(), grows.clone()))        # (the update itself is (b)'s subject)
    embs = st.lookup_train(ids)
    plan = next(p for k, p in st._plans.items() if k[1] == "train")
    nbytes = st.P * plan.cap * G * K * 4
    poison = [torch.full((nbytes,), 255, dtype=torch.uint8, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    del poison
    sum((e * g_).sum() for e, g_ in zip(embs, Gs)).backward()
    torch.cuda.synchronize()
    assert len(seen) == 1
    pay, grows = seen[0]
    inv = plan.inv[0].view(B, F).cpu().numpy()
    want = grad_groups_np([g_.cpu().numpy() for g_ in Gs], inv, K, st.P * plan.cap)
    got = grows.cpu().numpy()
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.array_equal(got, want)
    named = np.zeros(want.shape[0], bool)
    named[inv[inv >= 0]] = True
    assert (B == 1 or (inv < 0).any()) and (~named).any() and np.all(got[~named] == 0.0)
    assert np.array_equal(pay.cpu().numpy() >= 0, named)                   # the payload the owner walks names exactly those positions


# ---- (d) -----------------------------------------------------------------------------------------------------------------------------
def test_world1_graph_replay_equals_eager_after_training(built_lib):
    """A grouped lookup(ids, want_lin=True) with check="never" captured once; after one training step (rows of every group and unit moved)
    one replay equals the eager result bit for bit."""
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab, K, G, U, B = [300, 800, 20], 16, 2, 2, 512
    F = len(vocab)
    full_g, full_w = _draw(vocab, K, G, U, 19, dev)
    st = ShardedTables.from_full_groups([[t.clone() for t in tg] for tg in full_g], check="never").attach_linear_from_full(full_w, ACC0)
    st.enable_training(LR, ACC0).enable_linear_training(0.2, 0.01, 0.0)
    rng = np.random.default_rng(41)
    ids = _ids(rng, vocab, B, dev)
    bias = torch.tensor([-0.21, 0.4], dtype=torch.float32, device=dev)
    e0, l0 = st.lookup(ids, want_lin=True, lin_bias=bias)
    e0, l0 = [t.clone() for t in e0], l0.clone()
    step = ops.CapturedStep(lambda: st.lookup(ids, want_lin=True, lin_bias=bias))
    Gs = [torch.from_numpy(rng.standard_normal((B, F * K)).astype(np.float32)).to(dev) for _ in range(G)]
    g = torch.from_numpy(rng.standard_normal((B, U)).astype(np.float32)).to(dev)
    _train(st, ids, Gs, g)
    e1, l1 = st.lookup(ids, want_lin=True, lin_bias=bias)
    e1, l1 = [t.clone() for t in e1], l1.clone()
    step.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(step.out[0], e1)) and torch.equal(step.out[1], l1)
    assert not torch.equal(l1, l0) and not any(torch.equal(a, b) for a, b in zip(e1, e0))       # the step did move what the graph reads


# ---- (f) -----------------------------------------------------------------------------------------------------------------------------
def test_grouped_tables_refuse_what_they_do_not_cover(built_lib):
    """want_fm, lookup_consume, lookup_rows and the bag forms raise NotImplementedError on grouped tables before any launch; so do the bag
    forms of the first-order term on units > 1 rows; K % 4 != 0 and more than 8 units raise ValueError."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    vocab = _vocab(3)
    full_g, full_w = _draw(vocab, 8, 2, 2, 1, dev)
    st = ShardedTables.from_full_groups(full_g).attach_linear_from_full(full_w).enable_training(LR)
    ids = _ids(np.random.default_rng(1), vocab, 5, dev)
    empty, offs = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(5 * 3 + 1, dtype=torch.int64, device=dev)
    before = dict(st.stats)
    for call in (lambda: st.lookup(ids, want_fm=True), lambda: st.lookup_async(ids, want_fm=True), lambda: st.lookup_consume(ids, lambda *a: None),
                 lambda: st.lookup_rows(ids), lambda: st.lookup_bags(empty, offs), lambda: st.lookup_bags_train(empty, offs)):
        with pytest.raises(NotImplementedError, match="grouped"):
            call()
    assert st.stats == before and not st._plans and not st._bag_plans, "nothing was enqueued"
    one = ShardedTables.from_full(full_g[0]).attach_linear_from_full(full_w).enable_training(LR).enable_linear_training(0.1)
    with pytest.raises(NotImplementedError, match="units"):
        one.lookup_bags(empty, offs, want_lin=True)
    with pytest.raises(NotImplementedError, match="units"):
        one.lookup_bags_train(empty, offs, with_linear=True)
    with pytest.raises(ValueError, match="multiple of 4"):
        ShardedTables.from_full_groups([[torch.zeros(9, 6, device=dev)], [torch.zeros(9, 6, device=dev)]])
    with pytest.raises(ValueError, match="units"):
        one.attach_linear_from_full([torch.zeros(v, 9, device=dev) for v in vocab])


# ---- (e) two ranks -------------------------------------------------------------------------------------------------------------------
def _scenarios(rank, world, device):
    from dir_amd.shard import ShardedTables
    from tests.test_shard_groups_gloo import _trainer
    out = []
    vocab, K, G, U = [50, 50, 3, 50], 8, 2, 2
    full_g, full_w = _draw(vocab, K, G, U, 3, device)
    st = ShardedTables.from_full_groups(full_g).attach_linear_from_full(full_w)
    ids = _ids(np.random.default_rng(100 + rank), vocab, 37 + 5 * rank, device)           # uneven local batches, pruned ids
    embs, lin = st.lookup(ids, want_lin=True)
    torch.cuda.synchronize()
    idc = ids.cpu().numpy()
    ok = True
    for g in range(G):
        for f, v in enumerate(vocab):
            live = torch.from_numpy((idc[:, f] >= 0) & (idc[:, f] < v)).to(device)
            want = torch.where(live[:, None], full_g[g][f][ids[:, f].clamp(0, v - 1)], torch.zeros((), device=device))
            ok = ok and torch.equal(embs[g][:, f * K:(f + 1) * K], want)
    out.append(("forward_bitwise_per_group", ok and tuple(lin.shape) == (ids.shape[0], U), ""))
    sizes = [24 + 9 * r for r in range(world)]                                               # the ranks hold different batch sizes
    for linear in (True, False):
        out.append(("trainer_linear" if linear else "trainer", True,
                    _trainer(rank, world, linear, dev=device, VOCAB=[50, 50, 3, 50], K=8, hidden=(16, 16), sizes=sizes)))
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
    import tempfile
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = os.path.join(tempfile.mkdtemp(prefix="dir_pg_"), "store")
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


def test_groups_two_ranks_on_one_gpu(built_lib):
    """(e) two ranks on cuda:0 (gloo, host-staged exchanges), under its own time limit."""
    _check(_run(2, "gloo_same_device"), 2)


def test_groups_over_rccl_one_rank_per_gpu(built_lib):
    """(e) backend nccl (= RCCL), world = min(8, visible devices), one rank per GPU.  Skipped on a one-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL at world > 1 needs >= 2 visible GPUs (this box shows %d); the same scenarios run on one GPU over gloo" % n)
    world = min(8, n)
    _check(_run(world, "nccl"), world)
