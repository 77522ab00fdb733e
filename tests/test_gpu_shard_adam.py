"""The owner-side sparse Adam over row-sharded tables on the GPU (ShardedTables.enable_training_adam, ShardedDCNTrainer with the PRODUCT HIP
backend: dir_sparse_adam_payload_norm_f32, dir_sparse_adam_payload_apply_f32).

  (a) world size 1, five steps, (K, gscale, clip) as the one-GPU Adam test: the fixed and the exact path, one and two micro-batches,
      against float64; against ops.SparseAdam.step on unsharded copies at the same bar (not bitwise: its run sums see another entry
      order); two identical sharded runs end bitwise equal;
  (b) world size 1, one row takes 600 of 1500 entries, gradient scale 40, the clip active;
  (c) world size 1, an EMPTY batch after two ordinary steps: every row still moves as the reference says, no launch error;
  (d) two ranks on cuda:0 over host-staged gloo, local batches of 400 and 300 entries, gradient scale 1.23, clip 100: the 400-row
      table's global gradient norm is above the clip while each owner's share of it is below (asserted from the float64 reference) --
      an owner-local norm cannot pass; then the silent-owner step: only rank 0 receives live entries;
  (e) ShardedDCNTrainer at world size 1 and at two ranks on cuda:0 against model.train_step() on one GPU over the concatenated batch,
      with the default column names and with names that interleave embedding and numeric columns in sorted order;
  (f) (d) and (e) over RCCL with one rank per GPU (skipped with a reason on a one-GPU box);
  (g) a sharded Adam step refuses graph capture, in lookup_train before anything is enqueued and in the owner's step.  The refusal is
      host logic on torch.cuda.is_current_stream_capturing(); the test answers that question itself instead of opening a capture it
      would then abandon with an exception.
Reference: oracle.np_ref.sparse_adam_step in float64 on the unsharded tables with the global batch.  Error measure: the one-GPU Adam
test's, max |got - ref| / max |ref| per array, bar 1e-5, for var, m and v separately; the trainer: 1e-5 absolute
(test_dcn_train_step_hip_adam_equals_the_dense_torch_formulation's bar)."""
import os

import numpy as np
import pytest
import torch

from tests.test_shard_adam_gloo import B1, B2, EPS, Reference, lr_t_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = [50, 400, 7]
BAR = 1e-5


def _store():
    import tempfile
    return os.path.join(tempfile.mkdtemp(prefix="dir_pg_"), "store")


def _errs(tables, m, v, ref, slices=None):
    """max |got - ref| / max |ref| per array kind, this rank's rows against the scale of the whole reference array."""
    out = {"var": 0.0, "m": 0.0, "v": 0.0}
    for f in range(len(tables)):
        s, e = slices[f] if slices is not None else (0, ref.T[f].shape[0])
        if e == s:
            continue
        for name, got, want in (("var", tables[f], ref.T[f]), ("m", m[f], ref.m[f]), ("v", v[f], ref.v[f])):
            g = got.detach().double().cpu().numpy()
            out[name] = max(out[name], float(np.abs(g - want[s:e]).max() / max(np.abs(want).max(), 1e-300)))
    return out


def _train(st, ids, G, t):
    st.optimizer.lr_t = lr_t_of(t)
    emb = st.lookup_train(ids)
    (emb * G).sum().backward()


def _single_rank_group():
    import torch.distributed as dist
    if dist.is_initialized():
        return False
    dist.init_process_group("nccl", init_method="file://" + _store(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
    return True


@pytest.mark.parametrize("K,gscale,clip", [(16, 0.01, 100.0), (16, 40.0, 100.0), (8, 0.01, 0.0), (64, 5.0, 100.0)])
def test_world1_five_steps_match_float64_and_the_one_gpu_adam(built_lib, K, gscale, clip):
    """(a)"""
    import torch.distributed as dist
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(K + int(gscale * 10))
    F, B = len(VOCAB), 700
    w0 = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in VOCAB]
    data = []
    ref = Reference(w0, clip)
    for t in range(5):
        ids = np.stack([rng.integers(-1, v + 1, size=B) for v in VOCAB], 1).astype(np.int64)
        grad = (rng.standard_normal((B, F * K)) * gscale).astype(np.float32)
        data.append((torch.from_numpy(ids).to(dev), torch.from_numpy(grad).to(dev)))
        ref.step(ids, grad)
    if clip > 0:
        assert (max(max(n) for n in ref.norms) > clip) == (gscale >= 5.0), "the clip is %s here" % ("active" if gscale >= 5.0 else "idle")

    def run(**kw):
        st = ShardedTables.from_full([torch.from_numpy(w.copy()).to(dev) for w in w0], **kw).enable_training_adam(B1, B2, EPS, clip)
        for t, (ids, grad) in enumerate(data, 1):
            _train(st, ids, grad, t)
        torch.cuda.synchronize()
        m, v = st.adam_state()
        return st.local_tables, m, v

    created = _single_rank_group()
    try:
        runs = {"fixed": run(), "exact": run(mode="exact"), "chunks1": run(chunks=1, force_collective=True),
                "chunks2": run(chunks=2, force_collective=True)}
        again = run()
    finally:
        if created:
            dist.destroy_process_group()
    for name, (tabs, m, v) in runs.items():
        e = _errs(tabs, m, v, ref)
        print("K=%d gscale=%g clip=%g %s: var %.2e m %.2e v %.2e" % (K, gscale, clip, name, e["var"], e["m"], e["v"]))
        assert all(x <= BAR for x in e.values()), (name, e)
    # the one-GPU update on unsharded copies: the same bar (its sort sees the entries in batch order, the owner in slab order)
    tabs = [torch.from_numpy(w.copy()).to(dev) for w in w0]
    opt = ops.SparseAdam(ops.TableSet(tabs), B1, B2, EPS, clip)
    for t, (ids, grad) in enumerate(data, 1):
        opt.lr_t = lr_t_of(t)
        opt.step(ids, grad)
    torch.cuda.synchronize()
    for f in range(F):
        for name, got, want in (("var", runs["fixed"][0][f], tabs[f]), ("m", runs["fixed"][1][f], opt.ms[f]), ("v", runs["fixed"][2][f], opt.vs[f])):
            err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
            assert err <= BAR, "table %d %s against ops.SparseAdam.step: %.3e" % (f, name, err)
    # two identical sharded runs: bitwise (every run sum is formed in double: the slab order of a row's duplicates does not show, short
    # of a double sum within 2^-53 of an fp32 rounding boundary -- 2^-29 per sum, about 1e-4 over the 1e5 sums of this test)
    for a, b in zip(runs["fixed"], again):
        for f in range(F):
            assert torch.equal(a[f], b[f]), "table %d differs between two identical runs" % f
    assert not torch.equal(runs["fixed"][0][1].cpu(), torch.from_numpy(w0[1]))


def test_world1_hot_row_with_the_clip_active(built_lib):
    """(b) one row of the 400-row table takes 600 of 1500 entries, gradient scale 40."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(71)
    K, F, B, clip = 16, len(VOCAB), 1500, 100.0
    w0 = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in VOCAB]
    st = ShardedTables.from_full([torch.from_numpy(w.copy()).to(dev) for w in w0]).enable_training_adam(B1, B2, EPS, clip)
    ref = Reference(w0, clip)
    for t in range(1, 4):
        ids = np.stack([rng.integers(0, v, size=B) for v in VOCAB], 1).astype(np.int64)
        ids[rng.permutation(B)[:600], 1] = 123
        grad = (rng.standard_normal((B, F * K)) * 40.0).astype(np.float32)
        _train(st, torch.from_numpy(ids).to(dev), torch.from_numpy(grad).to(dev), t)
        ref.step(ids, grad)
        assert int((ids[:, 1] == 123).sum()) >= 600 and min(ref.norms[-1]) > clip
        m, v = st.adam_state()
        e = _errs(st.local_tables, m, v, ref)
        print("hot row, step %d: var %.2e m %.2e v %.2e" % (t, e["var"], e["m"], e["v"]))
        assert all(x <= BAR for x in e.values()), (t, e)


def test_world1_empty_batch_still_moves_every_row(built_lib):
    """(c) B = 0 after two ordinary steps: m *= beta1, v *= beta2, var -= lr_t m / (sqrt(v) + eps) on every row; no launch error."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(73)
    K, F, clip = 16, len(VOCAB), 100.0
    w0 = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in VOCAB]
    for kw in ({}, {"mode": "exact"}):
        st = ShardedTables.from_full([torch.from_numpy(w.copy()).to(dev) for w in w0], **kw).enable_training_adam(B1, B2, EPS, clip)
        ref = Reference(w0, clip)
        for t, B in enumerate((700, 700, 0), 1):
            ids = np.stack([rng.integers(-1, v + 1, size=B) for v in VOCAB], 1).astype(np.int64).reshape(B, F)
            grad = (rng.standard_normal((B, F * K)) * 5.0).astype(np.float32)
            before = [t_.clone() for t_ in st.local_tables]
            _train(st, torch.from_numpy(ids).to(dev), torch.from_numpy(grad).to(dev), t)
            torch.cuda.synchronize()                        # a launch error would surface here
            ref.step(ids, grad)
            m, v = st.adam_state()
            e = _errs(st.local_tables, m, v, ref)
            assert all(x <= BAR for x in e.values()), (kw, t, e)
        assert all(not torch.equal(a, b) for a, b in zip(before, st.local_tables)), "the empty step moved no row"


def test_graph_capture_of_a_sharded_adam_step_is_refused(built_lib, monkeypatch):
    """(g) NotImplementedError naming the reason, from the forward and from the owner's step; Adagrad on the same tables is not refused."""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    K = 16
    w0 = [torch.zeros((v, K), device=dev) for v in VOCAB]
    st = ShardedTables.from_full([w.clone() for w in w0]).enable_training_adam(B1, B2, EPS, 100.0)
    ids = torch.zeros((4, len(VOCAB)), dtype=torch.int64, device=dev)
    emb = st.lookup_train(ids)                              # an eager forward whose backward would run under the capture
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="captured in a graph"):
        st.lookup_train(ids)
    with pytest.raises(NotImplementedError, match="captured in a graph"):
        st._owner_step(torch.full((8,), -1, dtype=torch.int64, device=dev), torch.zeros((8, K), device=dev))
    ada = ShardedTables.from_full([w.clone() for w in w0]).enable_training(0.05)
    ada._refuse_adam_capture(ids)                           # (no refusal of its own: the Adagrad step's rules are unchanged)
    monkeypatch.undo()
    st.optimizer.lr_t = lr_t_of(1)
    emb.sum().backward()                                    # the tables still train once the capture is over
    torch.cuda.synchronize()
    assert st._updates == 1


# ---- ShardedDCNTrainer -------------------------------------------------------------------------------------------------------------------
def _dcn(interleave):
    from dir_amd import feature_column as fc
    from dir_amd.dcn import DeepCrossNetwork
    torch.manual_seed(5)                                    # the same initialisation wherever it is built
    nums = ["C00_x", "C02_x", "C04_x"] if interleave else ["I00", "I01", "I02"]       # "C00_embedding" < "C00_x" < "C01_embedding" < ...
    cols = [fc.embedding_column(fc.categorical_column_with_identity("C%02d" % i, 300), 16) for i in range(6)]
    cols += [fc.numeric_column(n) for n in nums]
    model = DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[64, 32], batch_norm=False, optimizer="Adam",
                             optimizer_spec={"epsilon": 1e-4}, l2_reg=1e-4,
                             learning_rate_spec={"learning_rate": 0.01, "decay_method": "cosine_decay", "decay_steps": 100, "alpha": 0.5}).cuda()
    return model, nums


def _dcn_batches(nums, n, steps):
    gen = torch.Generator().manual_seed(1)
    out = []
    for _ in range(steps):
        ids = torch.randint(0, 300, (n, 6), generator=gen)
        ids[::5, 0] = 7                                     # a row every rank looks up, many times
        f = {"C%02d" % i: ids[:, i].contiguous().cuda() for i in range(6)}
        f.update({k: torch.rand((n,), generator=gen).cuda() for k in nums})
        out.append((f, (torch.rand((n, 1), generator=gen) < 0.3).float().cuda()))
    return out


def _dcn_trainer_errors(interleave, rank, world, group=None):
    """Three steps of ShardedDCNTrainer (this rank's share of the global batch of 512) against model.train_step() on the whole batch; ->
    the worst absolute differences."""
    from dir_amd.shard import ShardedDCNTrainer
    model, nums = _dcn(interleave)
    ref_model, _ = _dcn(interleave)
    names = [c.name for c in model.input_layer.columns]
    kinds = [n.endswith("_embedding") for n in names]
    assert (kinds != sorted(kinds, reverse=True)) == interleave, names          # interleaved <=> not "all embeddings, then all numerics"
    tables = ShardedDCNTrainer.tables_from_model(model, group=group)
    tr = ShardedDCNTrainer(model, tables, group=group)
    ref_op = ref_model.train_step()
    n = 512
    cut = [0, n] if world == 1 else [0, 300, n]             # uneven local batches: the loss is the GLOBAL mean
    lo, hi = cut[rank], cut[rank + 1]
    batches = _dcn_batches(nums, n, 4)
    for f, y in batches[:3]:
        tr.step({k: v[lo:hi] for k, v in f.items()}, y[lo:hi])
        ref_op(torch.nn.functional.binary_cross_entropy_with_logits(ref_model(f), y))
    torch.cuda.synchronize()
    errs = {"global_step": float(abs(tr.global_step - 3) + abs(ref_op.global_step - 3))}
    errs["dense"] = max(float((p.detach() - q.detach()).abs().max()) for (a, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters())
                        if "embedding_weights" not in a)
    errs["tables"] = max(float((tables.local_tables[i] - ref_model.input_layer.embedding_weights[i].detach()[s:e]).abs().max())
                         for i, (s, e) in enumerate(tables.slices) if e > s)
    f, _ = batches[3]
    got = tr.predict({k: v[lo:hi] for k, v in f.items()})
    want = ref_model.predict(f)
    errs["predict"] = max(float((got[k].float() - want[k][lo:hi].float()).abs().max()) for k in ("logits", "logistic", "probabilities"))
    moved = float((ref_model.input_layer.embedding_weights[0].detach() - _dcn(interleave)[0].input_layer.embedding_weights[0].detach()).abs().max())
    assert moved > 1e-3, "the reference's tables must have moved"
    return errs


@pytest.mark.parametrize("interleave", [False, True])
def test_dcn_trainer_world1_equals_train_step(built_lib, interleave):
    """(e) at world size 1: every dense parameter and every table row within 1e-5 absolute, predict within 1e-5, global_step == 3."""
    errs = _dcn_trainer_errors(interleave, 0, 1)
    print(errs)
    assert all(v <= 1e-5 for v in errs.values()), errs


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------------
def _scenarios(rank, world, device):
    import torch.distributed as dist
    from dir_amd.shard import ShardedTables, partition_layout
    from oracle import np_ref as R
    out = []
    K, F, clip, gscale = 16, len(VOCAB), 100.0, 1.23
    sizes = [400, 300] + [300] * (world - 2)
    rng = np.random.default_rng(81)
    w0 = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in VOCAB]
    st = ShardedTables.from_full([torch.from_numpy(w.copy()).to(device) for w in w0]).enable_training_adam(B1, B2, EPS, clip)
    _, _, slices = partition_layout(VOCAB, K, world, rank, None)
    ref = Reference(w0, clip)
    worst, proof = {"var": 0.0, "m": 0.0, "v": 0.0}, []
    for t in range(1, 5):
        ids_all = [np.stack([rng.integers(0, v, size=b) for v in VOCAB], 1).astype(np.int64) for b in sizes]
        G_all = [(rng.standard_normal((b, F * K)) * gscale).astype(np.float32) for b in sizes]
        if t == 4:                                          # the silent-owner step: only rank 0 receives live entries
            for a in ids_all:
                for f in range(F):
                    owner, _ = R.shard_div_owner(a[:, f], VOCAB[f], world)
                    a[:, f] = np.where(owner == 0, a[:, f], -1)
        ids, G = np.concatenate(ids_all), np.concatenate(G_all)
        if t <= 3:
            # what makes the comparison a proof: table 1's GLOBAL gradient norm is above the clip, every owner's share of it below
            g = np.zeros((VOCAB[1], K))
            np.add.at(g, ids[:, 1], G[:, K:2 * K].astype(np.float64))
            owner, _ = R.shard_div_owner(np.arange(VOCAB[1]), VOCAB[1], world)
            shares = [float(np.sqrt((g[owner == o] ** 2).sum())) for o in range(world)]
            total = float(np.sqrt((g * g).sum()))
            proof.append(total > clip and all(s < clip for s in shares))
            assert proof[-1], "step %d: global norm %.1f, owners' shares %s, clip %g: adjust gscale" % (t, total, shares, clip)
        _train(st, torch.from_numpy(ids_all[rank]).to(device), torch.from_numpy(G_all[rank]).to(device), t)
        torch.cuda.synchronize()
        ref.step(ids, G)
        m, v = st.adam_state()
        e = _errs(st.local_tables, m, v, ref, slices)
        if t == 3:
            out.append(("adam_three_steps", all(x <= BAR for x in worst.values()) and all(x <= BAR for x in e.values()) and all(proof),
                        "var %.2e m %.2e v %.2e" % (e["var"], e["m"], e["v"])))
        if t == 4:
            out.append(("silent_owner", all(x <= BAR for x in e.values()), "var %.2e m %.2e v %.2e" % (e["var"], e["m"], e["v"])))
        worst = {k: max(worst[k], e[k]) for k in worst}
    errs = _dcn_trainer_errors(False, rank, world)
    out.append(("dcn_trainer", all(v <= 1e-5 for v in errs.values()), " ".join("%s %.2e" % kv for kv in errs.items())))
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
        assert [n for n, _, _ in got] == ["adam_three_steps", "silent_owner", "dcn_trainer"]


def test_adam_two_ranks_on_one_gpu(built_lib):
    """(d) + (e) two ranks on cuda:0 (gloo, host-staged exchanges)."""
    _check(_run(2, "gloo_same_device"), 2)


def test_adam_over_rccl_one_rank_per_gpu(built_lib):
    """(f) backend nccl (= RCCL), two ranks, one per GPU.  Skipped on a one-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL at world > 1 needs >= 2 visible GPUs (this box shows %d); the same scenarios run on one GPU over gloo" % n)
    _check(_run(2, "nccl"), 2)
