"""The owner-side sparse Adam over multi-hot bags on the GPU (ShardedTables.lookup_bags_train under enable_training_adam, ShardedDCNTrainer
on ragged features, with the PRODUCT HIP backend: dir_sparse_adam_bags_norm_f32, dir_sparse_adam_bags_apply_f32).

  (a) world size 1, five steps against float64: K in {8, 16, 64}, F = 3, vocab [50, 400, 7], B = 96, bags of 0 to 6 entries, one step per
      tests.test_shard_bags_gloo.CASES combination; the max_norms clip some touched rows and leave others (asserted on the reference);
      clip idle, active and 0;
  (b) where no max_norm is set, against ops.SparseAdam.step on unsharded copies fed the dense-equivalent sparse gradient (one one-hot
      entry per live bag entry, w_e * c_bag * g[b, f]) -- the same bar, not bitwise;
  (c) one hot row with >= 700 entries in a step (>= three 256-entry tiles: the carry rows and adagrad_fix_k), max_norm on that row, the
      row carrying > 99 % of its table's ||g||^2, the table norm above 65 536 (the high norm word) and below; the norm share against the
      float64 ||g||^2 * 2^32;
  (d) an empty local batch, and slabs with no live record: every row still decays and steps;
  (e) two identical runs of three steps end bitwise equal in var, m and v (every run sum is formed in double, whatever order the slab's
      atomics left the records in -- short of a double sum within 2^-53 of an fp32 rounding boundary, as for the payload form);
  (f) a one-hot lookup_train step after a bag step equals, bitwise, the same step on a fresh optimiser that took the same history
      (duplicate-free ids): the shared marks, first_call state and sort area do not show;
  (g) graph capture of a bag Adam step is refused before anything is enqueued (the test answers the capture question itself, as
      tests/test_gpu_shard_adam.py does);
  (h) ShardedDCNTrainer at world size 1 on ragged + weighted + max_norm columns interleaved with numeric columns against
      model.train_step() on the unsharded model, three steps, and predict;
  (i) two ranks on cuda:0 over host-staged gloo, and over RCCL with one rank per GPU (skipped below two GPUs): the gloo file's scenarios
      (uneven and empty batches, a hot row in bags / across bags / across ranks, alternating one-hot and bag steps, clip 0, a silent
      owner) and the trainer, on the HIP backend.
Reference: tests.shard_standin_bags_adam.BagsAdamReference (float64 autograd of the bag forward over the full tables on the global batch,
then a float64 dense Adam with the per-table clip_by_norm).  Error measure and bar: tests/test_gpu_shard_adam.py's (_errs, BAR); the
trainer: test_dcn_trainer_world1_equals_train_step's."""
import os

import numpy as np
import pytest
import torch

from tests.shard_standin import per_slot
from tests.shard_standin_bags_adam import BagsAdamReference
from tests.test_gpu_shard_adam import BAR, VOCAB, _errs, _store
from tests.test_shard_adam_gloo import B1, B2, EPS, LR, lr_t_of
from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = len(VOCAB)
SHARE_BAR = 1e-6                # the norm share against float64 ||g||^2 * 2^32: test_gpu_sort_plans.test_adam_clip_norm_across_its_range's bound
TRAINER_BAR = 1e-5              # test_gpu_shard_adam.test_dcn_trainer_world1_equals_train_step's


def _tables(K, seed, scale=None):
    """Row norms around 0.85 whatever K: above some of the CASES' max_norms (0.6 ... 1.1) and below others."""
    rng = np.random.default_rng(seed)
    s = 0.3 * np.sqrt(8.0 / K) if scale is None else scale
    return [(rng.standard_normal((v, K)) * s).astype(np.float32) for v in VOCAB]


def _sharded(w0, clip, dev):
    from dir_amd.shard import ShardedTables
    return ShardedTables.from_full([torch.from_numpy(w.copy()).to(dev) for w in w0]).enable_training_adam(B1, B2, EPS, clip)


def _bag_step(st, bags, case, G, t, dev):
    from dir_amd import ops
    _, comb, mn, fmaj, prune = case
    v, o, w = to_csr(bags, F, fmaj)
    st.optimizer.lr_t = lr_t_of(t)
    emb = st.lookup_bags_train(torch.from_numpy(v).to(dev), torch.from_numpy(o).to(dev), None if w is None else torch.from_numpy(w).to(dev),
                               combiner=comb, max_norm=mn, field_major=fmaj, flags=ops.PRUNE_NONPOSITIVE_WEIGHTS if prune else 0)
    emb.backward(torch.from_numpy(G).to(dev))


def _state(st):
    m, v = st.adam_state()
    return st.local_tables, m, v


@pytest.mark.parametrize("gscale,clip", [(0.01, 100.0), (40.0, 100.0), (1.0, 0.0)], ids=["idle", "active", "noclip"])
@pytest.mark.parametrize("K", [8, 16, 64])
def test_world1_five_steps_match_float64(built_lib, K, gscale, clip):
    """(a)"""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(100 * K + int(gscale * 10))
    w0 = _tables(K, K)
    st = _sharded(w0, clip, dev)
    ref = BagsAdamReference(w0, LR, B1, B2, EPS, clip)
    B = 96
    for t, case in enumerate(CASES, 1):
        bags = draw_bags(rng, B, VOCAB, [6, 6, 6], case[0])
        G = (rng.standard_normal((B, F * K)) * gscale).astype(np.float32)
        _bag_step(st, bags, case, G, t, dev)
        ref.step(bags, G, case[1], case[2], case[4])
        e = _errs(*_state(st), ref)
        print("K=%d gscale=%g clip=%g step %d: var %.2e m %.2e v %.2e" % (K, gscale, clip, t, e["var"], e["m"], e["v"]))
        assert all(x <= BAR for x in e.values()), (t, e)
    assert st._updates == len(CASES)
    clipped, left = sum(c for c, _ in ref.row_clipped), sum(u for _, u in ref.row_clipped)
    assert clipped > 0 and left > 0, "max_norm must clip some touched rows and leave others: %d clipped, %d not" % (clipped, left)
    if clip > 0:
        assert (max(max(n) for n in ref.norms) > clip) == (gscale >= 5.0), "the clip is %s here" % ("active" if gscale >= 5.0 else "idle")


def _dense_equivalent(bags, G, combiner, K):
    """The bag step as one-hot entries: ids [n, F] (-1 = padding), grad [n, F*K] fp32, one row per live entry = w_e * c_bag * g[b, f]."""
    comb = per_slot(combiner, F)
    per = []
    for f in range(F):
        ids, gs = [], []
        for b, row in enumerate(bags):
            i_, w_ = row[f]
            live = [(int(i), 1.0 if w_ is None else float(w_[j])) for j, i in enumerate(i_) if 0 <= i < VOCAB[f]]
            if not live:
                continue
            ws = np.array([w for _, w in live])
            if comb[f] == "mean":
                den = ws.sum() if w_ is not None else float(len(live))
            elif comb[f] == "sqrtn":
                den = np.sqrt((ws * ws).sum() if w_ is not None else float(len(live)))
            else:
                den = 1.0
            for i, w in live:
                ids.append(i)
                gs.append(w / den * G[b, f * K:(f + 1) * K].astype(np.float64))
        per.append((ids, gs))
    n = max(1, max(len(p[0]) for p in per))
    ids = np.full((n, F), -1, np.int64)
    grad = np.zeros((n, F * K), np.float32)
    for f, (i_, g_) in enumerate(per):
        if i_:
            ids[:len(i_), f] = i_
            grad[:len(i_), f * K:(f + 1) * K] = np.asarray(g_)
    return ids, grad


@pytest.mark.parametrize("K", [8, 64])
def test_world1_matches_the_one_gpu_adam_where_no_max_norm_is_set(built_lib, K):
    """(b) CASES without a max_norm and without pruning: mean without weights, per-slot combiners with weights, field-major."""
    from dir_amd import ops
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(300 + K)
    clip, gscale, B = 100.0, 40.0, 96
    cases = [c for c in CASES if c[2] is None and not c[4]]
    assert len(cases) == 2
    w0 = _tables(K, 3 * K)
    st = _sharded(w0, clip, dev)
    tabs = [torch.from_numpy(w.copy()).to(dev) for w in w0]
    opt = ops.SparseAdam(ops.TableSet(tabs), B1, B2, EPS, clip)
    for t in range(1, 6):
        case = cases[t % 2]
        bags = draw_bags(rng, B, VOCAB, [6, 6, 6], case[0])
        G = (rng.standard_normal((B, F * K)) * gscale).astype(np.float32)
        _bag_step(st, bags, case, G, t, dev)
        ids, grad = _dense_equivalent(bags, G, case[1], K)
        opt.lr_t = lr_t_of(t)
        opt.step(torch.from_numpy(ids).to(dev), torch.from_numpy(grad).to(dev))
    torch.cuda.synchronize()
    got = _state(st)
    for f in range(F):
        for name, a, b in (("var", got[0][f], tabs[f]), ("m", got[1][f], opt.ms[f]), ("v", got[2][f], opt.vs[f])):
            err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            print("K=%d table %d %s against ops.SparseAdam.step: %.2e" % (K, f, name, err))
            assert err <= BAR, "table %d %s against ops.SparseAdam.step: %.3e" % (f, name, err)
    assert not torch.equal(got[0][1].cpu(), torch.from_numpy(w0[1]))


@pytest.mark.parametrize("gscale,high", [(60.0, True), (1.0, False)], ids=["above_65536", "below_65536"])
def test_world1_hot_row_through_the_carry_rows(built_lib, gscale, high):
    """(c) 400 bags of slot 1 hold row 123 twice each: its run spans at least three tiles of the sort.  Coherent gradients (one common
    direction plus noise) so that the 800 entries add up instead of cancelling; max_norm 0.5 on the slot, below the row's norm."""
    dev = torch.device("cuda", 0)
    K, B, clip, hot = 16, 420, 100.0, 123
    rng = np.random.default_rng(71)
    w0 = _tables(K, 7, scale=0.2)
    st = _sharded(w0, clip, dev)
    ref = BagsAdamReference(w0, LR, B1, B2, EPS, clip)
    case = ("pos", ["mean", "sum", "sqrtn"], [None, 0.5, None], False, False)
    shares = []
    norm_of = st.backend.bags_adam_norm
    st.backend.bags_adam_norm = lambda *a: shares.append(norm_of(*a)) or shares[-1]
    assert float(np.sqrt((w0[1][hot].astype(np.float64) ** 2).sum())) > 0.5, "the hot row must be clipped by its max_norm"
    for t in range(1, 4):
        bags = draw_bags(rng, B, VOCAB, [3, 1, 2], "pos")
        for b in range(400):
            bags[b][1] = (np.array([hot, hot], np.int64), rng.uniform(0.5, 1.5, size=2).astype(np.float32))
        base = rng.standard_normal(K)
        G = (rng.standard_normal((B, F * K)) * gscale).astype(np.float32)
        G[:, K:2 * K] = (gscale * (base[None, :] + 0.1 * rng.standard_normal((B, K)))).astype(np.float32)
        hits = sum(int((bg[1][0] == hot).sum()) for bg in bags)
        assert hits >= 700, hits
        gs = ref.grads(bags, G, case[1], case[2], case[4])
        n2 = [float((g * g).sum()) for g in gs]
        assert float((gs[1][hot] ** 2).sum()) > 0.99 * n2[1], "the hot row carries %.4f of its table's ||g||^2" % (float((gs[1][hot] ** 2).sum()) / n2[1])
        assert (np.sqrt(n2[1]) > 65536.0) == high and np.sqrt(n2[1]) > clip, "table 1's gradient norm is %g" % np.sqrt(n2[1])
        _bag_step(st, bags, case, G, t, dev)
        ref.step(bags, G, case[1], case[2], case[4])
        if t == 1:                                  # (the tables are still the reference's bit for bit: the share is the kernel's alone)
            words = shares[-1].cpu().numpy().astype(np.uint64)
            got = [int(lo) + (int(hi) << 32) for lo, hi in zip(words[0], words[1])]
            errs = [abs(g / (n * 4294967296.0) - 1.0) for g, n in zip(got, n2)]
            print("hot row gscale=%g: norm shares off float64 by %s" % (gscale, ["%.2e" % x for x in errs]))
            assert max(errs) <= SHARE_BAR, "the norm share is %.3e off float64 ||g||^2 * 2^32" % max(errs)
        e = _errs(*_state(st), ref)
        print("hot row gscale=%g step %d (%d entries): var %.2e m %.2e v %.2e" % (gscale, t, hits, e["var"], e["m"], e["v"]))
        assert all(x <= BAR for x in e.values()), (t, e)
    assert len(shares) == 3


def test_world1_empty_batch_and_dead_slabs_still_move_every_row(built_lib):
    """(d) after two ordinary steps: B = 0, then a batch whose every id is pruned -- no live record; m *= beta1, v *= beta2 and var steps
    on every row; no launch error."""
    dev = torch.device("cuda", 0)
    K, clip = 16, 100.0
    rng = np.random.default_rng(73)
    w0 = _tables(K, 9)
    st = _sharded(w0, clip, dev)
    ref = BagsAdamReference(w0, LR, B1, B2, EPS, clip)
    case = CASES[1]
    for t, B in enumerate((96, 96, 0, 40), 1):
        bags = draw_bags(rng, B, VOCAB, [6, 6, 6], case[0])
        if t == 4:
            for row in bags:
                for f in range(F):
                    row[f][0][:] = -1
        G = (rng.standard_normal((B, F * K)) * 5.0).astype(np.float32)
        before = [x.clone() for x in st.local_tables]
        _bag_step(st, bags, case, G, t, dev)
        torch.cuda.synchronize()                        # a launch error would surface here
        ref.step(bags, G, case[1], case[2], case[4])
        e = _errs(*_state(st), ref)
        assert all(x <= BAR for x in e.values()), (t, e)
        if t >= 3:
            assert max(ref.norms[-1]) == 0.0
            assert all(not torch.equal(a, b) for a, b in zip(before, st.local_tables)), "step %d moved no row" % t


def test_two_identical_runs_end_bitwise_equal(built_lib):
    """(e)"""
    dev = torch.device("cuda", 0)
    K, clip, B = 16, 100.0, 96
    w0 = _tables(K, 11)

    def run():
        rng = np.random.default_rng(75)
        st = _sharded(w0, clip, dev)
        for t, c in enumerate((1, 2, 4), 1):
            bags = draw_bags(rng, B, VOCAB, [6, 6, 6], CASES[c][0])
            for row in bags:                        # a hot row inside bags and across them
                if len(row[1][0]) >= 2:
                    row[1][0][:2] = 3
            _bag_step(st, bags, CASES[c], (rng.standard_normal((B, F * K)) * 40.0).astype(np.float32), t, dev)
        torch.cuda.synchronize()
        return _state(st)
    a, b = run(), run()
    for name, x, y in zip(("var", "m", "v"), a, b):
        for f in range(F):
            assert torch.equal(x[f], y[f]), "%s of table %d differs between two identical runs" % (name, f)
    assert not torch.equal(a[0][1].cpu(), torch.from_numpy(w0[1]))


def test_one_hot_step_after_a_bag_step_is_unchanged(built_lib):
    """(f)"""
    from dir_amd.shard import ShardedTables
    dev = torch.device("cuda", 0)
    K, clip, B = 16, 100.0, 96
    rng = np.random.default_rng(77)
    w0 = _tables(K, 13)
    st = _sharded(w0, clip, dev)
    bags = draw_bags(rng, B, VOCAB, [6, 6, 6], CASES[2][0])
    _bag_step(st, bags, CASES[2], (rng.standard_normal((B, F * K)) * 40.0).astype(np.float32), 1, dev)
    torch.cuda.synchronize()
    # a fresh optimiser with the same history: the tables, m and v as the bag step left them
    fresh = ShardedTables.from_full([x.clone() for x in st.local_tables]).enable_training_adam(B1, B2, EPS, clip)
    m, v = st.adam_state()
    fm, fv = fresh.adam_state()
    for f in range(F):
        fm[f].copy_(m[f])
        fv[f].copy_(v[f])
    n = 7                                           # duplicate-free ids in every slot (the smallest table has 7 rows)
    ids = torch.from_numpy(np.stack([rng.permutation(vv)[:n] for vv in VOCAB], 1).astype(np.int64)).to(dev)
    G = torch.from_numpy((rng.standard_normal((n, F * K)) * 40.0).astype(np.float32)).to(dev)
    for s in (st, fresh):
        s.optimizer.lr_t = lr_t_of(2)
        s.lookup_train(ids).backward(G)
    torch.cuda.synchronize()
    for name, x, y in zip(("var", "m", "v"), _state(st), _state(fresh)):
        for f in range(F):
            assert torch.equal(x[f], y[f]), "%s of table %d: the one-hot step after a bag step differs" % (name, f)
    # ... and a bag step after the one-hot step still follows (the marks were left clean)
    bags = draw_bags(rng, B, VOCAB, [6, 6, 6], CASES[0][0])
    G2 = (rng.standard_normal((B, F * K)) * 40.0).astype(np.float32)
    for s in (st, fresh):
        _bag_step(s, bags, CASES[0], G2, 3, dev)
    torch.cuda.synchronize()
    for name, x, y in zip(("var", "m", "v"), _state(st), _state(fresh)):
        for f in range(F):
            assert torch.equal(x[f], y[f]), "%s of table %d: the bag step after a one-hot step differs" % (name, f)


def test_graph_capture_of_a_bag_adam_step_is_refused(built_lib, monkeypatch):
    """(g) NotImplementedError naming the reason, from the forward and from the backward, with nothing enqueued and no update counted."""
    dev = torch.device("cuda", 0)
    K = 16
    st = _sharded([np.zeros((v, K), np.float32) for v in VOCAB], 100.0, dev)
    rng = np.random.default_rng(79)
    bags = draw_bags(rng, 8, VOCAB, [3, 3, 3], None)
    v, o, _ = to_csr(bags, F, False)
    v, o = torch.from_numpy(v).to(dev), torch.from_numpy(o).to(dev)
    emb = st.lookup_bags_train(v, o)                        # an eager forward whose backward would run under the capture
    lookups = st.stats["bag_train_lookups"]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="captured in a graph"):
        st.lookup_bags_train(v, o)
    with pytest.raises(NotImplementedError, match="captured in a graph"):
        emb.backward(torch.ones_like(emb))
    assert st.stats["bag_train_lookups"] == lookups and st._updates == 0
    monkeypatch.undo()
    st.optimizer.lr_t = lr_t_of(1)
    st.lookup_bags_train(v, o).sum().backward()             # the tables still train once the capture is over
    torch.cuda.synchronize()
    assert st._updates == 1


# ---- ShardedDCNTrainer on ragged features ----------------------------------------------------------------------------------------------
V_DCN = 300


def _dcn():
    from dir_amd import feature_column as fc
    from dir_amd.dcn import DeepCrossNetwork
    torch.manual_seed(5)                                    # the same initialisation wherever it is built
    ident = [fc.categorical_column_with_identity("C%02d" % i, V_DCN) for i in range(4)]
    # "C00_embedding" < "C00_x" < "C01_weighted_by_C01_w_embedding" < "C02_embedding" < "C02_x" < "C03_embedding"
    cols = [fc.embedding_column(ident[0], 16, combiner="sqrtn", max_norm=0.9),
            fc.embedding_column(fc.weighted_categorical_column(ident[1], "C01_w"), 16, combiner="mean"),
            fc.embedding_column(ident[2], 16, combiner="sum", max_norm=0.8),
            fc.embedding_column(ident[3], 16, combiner="mean")]
    nums = ["C00_x", "C02_x"]
    cols += [fc.numeric_column(n) for n in nums]
    model = DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[64, 32], batch_norm=False, optimizer="Adam",
                             optimizer_spec={"epsilon": 1e-4}, l2_reg=1e-4,
                             learning_rate_spec={"learning_rate": 0.01, "decay_method": "cosine_decay", "decay_steps": 100, "alpha": 0.5}).cuda()
    return model, nums


def _dcn_batch(n, seed):
    """n samples: C00 bags of 0..5 ids (a hot id; -1 mixed in), C01 weighted bags of 1..3, C02 bags of 0..2, C03 one id per sample."""
    g = torch.Generator().manual_seed(seed)
    lens = {"C00": torch.randint(0, 6, (n,), generator=g), "C01": torch.randint(1, 4, (n,), generator=g), "C02": torch.randint(0, 3, (n,), generator=g)}
    f = {}
    for k, l in lens.items():
        vals = torch.randint(0, V_DCN, (int(l.sum()),), generator=g)
        f[k] = (vals, l)
    f["C00"][0][::4] = 7                                    # a row every rank looks up, many times, inside bags and across them
    f["C00"][0][1::9] = -1
    f["C01_w"] = (torch.rand(int(lens["C01"].sum()), generator=g) * 1.9 + 0.1, lens["C01"])
    f["C03"] = torch.randint(0, V_DCN, (n,), generator=g)
    f.update({k: torch.rand((n,), generator=g) for k in ("C00_x", "C02_x")})
    return f, (torch.rand((n, 1), generator=g) < 0.3).float()


def _take(f, lo, hi):
    from dir_amd.feature_column import Ragged
    out = {}
    for k, v in f.items():
        if isinstance(v, tuple):
            vals, lens = v
            offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
            out[k] = Ragged(vals[int(offs[lo]):int(offs[hi])].clone().cuda(), (offs[lo:hi + 1] - offs[lo]).clone().cuda())
        else:
            out[k] = v[lo:hi].cuda()
    return out


def _dcn_trainer_errors(rank, world, group=None):
    """Three steps of ShardedDCNTrainer (this rank's share of the global batch of 256) against model.train_step() on the whole batch; ->
    the worst absolute differences."""
    from dir_amd.shard import ShardedDCNTrainer
    model, nums = _dcn()
    ref_model, _ = _dcn()
    names = [c.name for c in model.input_layer.columns]
    kinds = [n.endswith("_embedding") for n in names]
    assert names == sorted(names) and kinds != sorted(kinds, reverse=True), names          # embedding and numeric columns interleave
    tables = ShardedDCNTrainer.tables_from_model(model, group=group)
    tr = ShardedDCNTrainer(model, tables, group=group)
    ref_op = ref_model.train_step()
    n = 256
    cut = [0, n] if world == 1 else [0, 150, n]             # uneven local batches: the loss is the GLOBAL mean
    lo, hi = cut[rank], cut[rank + 1]
    start = [p.detach().clone() for p in ref_model.input_layer.embedding_weights]
    for s in range(3):
        f, y = _dcn_batch(n, 1 + s)
        tr.step(_take(f, lo, hi), y[lo:hi].cuda())
        ref_op(torch.nn.functional.binary_cross_entropy_with_logits(ref_model(_take(f, 0, n)), y.cuda()))
    torch.cuda.synchronize()
    errs = {"global_step": float(abs(tr.global_step - 3) + abs(ref_op.global_step - 3))}
    errs["dense"] = max(float((p.detach() - q.detach()).abs().max()) for (a, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters())
                        if "embedding_weights" not in a)
    ref_tabs = [p.detach() for p in ref_model.input_layer.embedding_weights]           # (both in the input layer's name-sorted order)
    assert [c.name for c in tr.emb_cols] == [c.name for c in ref_model.input_layer.emb_cols]
    errs["tables"] = max(float((tables.local_tables[i] - ref_tabs[i][s:e]).abs().max()) for i, (s, e) in enumerate(tables.slices) if e > s)
    f, _ = _dcn_batch(n, 9)
    got = tr.predict(_take(f, lo, hi))
    want = ref_model.predict(_take(f, 0, n))
    errs["predict"] = max(float((got[k].float() - want[k][lo:hi].float()).abs().max()) for k in ("logits", "logistic", "probabilities"))
    moved = min(float((p.detach() - q).abs().max()) for p, q in zip(ref_model.input_layer.embedding_weights, start))
    assert moved > 1e-3, "the reference's tables must have moved"
    return errs


def test_dcn_trainer_world1_on_ragged_features_equals_train_step(built_lib):
    """(h) every dense parameter and every table row within 1e-5 absolute, predict within 1e-5, global_step == 3."""
    errs = _dcn_trainer_errors(0, 1)
    print(errs)
    assert all(v <= TRAINER_BAR for v in errs.values()), errs


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------------
def _steps(rank, world, device, seed, kinds, sizes, gscale, clip, hot=None, silent_step=None, K=16):
    """tests/test_shard_bags_adam_gloo._steps on the HIP backend: -> the worst errors over the steps."""
    from dir_amd.shard import partition_layout
    from oracle import np_ref as R
    w0 = _tables(K, seed)
    st = _sharded(w0, clip, device)
    _, _, slices = partition_layout(VOCAB, K, world, rank, None)
    ref = BagsAdamReference(w0, LR, B1, B2, EPS, clip)
    worst = {"var": 0.0, "m": 0.0, "v": 0.0}
    for t, kind in enumerate(kinds, 1):
        rng = np.random.default_rng(seed + 1000 * t)
        G_all = [(gscale * rng.standard_normal((sizes[r], F * K))).astype(np.float32) for r in range(world)]
        if kind == "onehot":
            ids_all = [np.stack([rng.integers(-2, v + 2, size=sizes[r]) for v in VOCAB], 1).astype(np.int64).reshape(sizes[r], F) for r in range(world)]
            st.optimizer.lr_t = lr_t_of(t)
            st.lookup_train(torch.from_numpy(ids_all[rank]).to(device)).backward(torch.from_numpy(G_all[rank]).to(device))
            ref.step_onehot(np.concatenate(ids_all), np.concatenate(G_all))
        else:
            case = CASES[kind]
            bags_all = [draw_bags(rng, sizes[r], VOCAB, [6, 6, 6], case[0]) for r in range(world)]
            for bl in bags_all:
                for row in bl:
                    if hot is not None and len(row[hot[0]][0]) >= 2:
                        row[hot[0]][0][:2] = hot[1]          # one row inside bags, across bags and across ranks
                    if t == silent_step:                     # every id whose owner is not rank 0 becomes -1
                        for f in range(F):
                            ids = row[f][0]
                            ok = (ids >= 0) & (ids < VOCAB[f])
                            owner, _ = R.shard_div_owner(np.where(ok, ids, 0), VOCAB[f], world)
                            ids[:] = np.where(ok & (np.asarray(owner) == 0), ids, -1)
            _bag_step(st, bags_all[rank], case, G_all[rank], t, device)
            ref.step([b for bl in bags_all for b in bl], np.concatenate(G_all), case[1], case[2], case[4])
        torch.cuda.synchronize()
        e = _errs(*_state(st), ref, slices)
        worst = {k: max(worst[k], e[k]) for k in worst}
    assert st._updates == len(kinds)
    return worst, ref


def _scenarios(rank, world, device):
    out = []

    def add(name, worst, extra=True):
        out.append((name, bool(extra) and all(x <= BAR for x in worst.values()), "var %.2e m %.2e v %.2e" % (worst["var"], worst["m"], worst["v"])))
    sizes = [40 + 13 * r for r in range(world)]
    empty = [0 if r == 1 else 40 + 13 * r for r in range(world)]
    w, ref = _steps(rank, world, device, 201, [2, 1, 4], empty, 40.0, 100.0, hot=(1, 3))
    add("cases_clip_active_hot_row_empty_batch", w, max(max(n) for n in ref.norms) > 100.0)
    w, ref = _steps(rank, world, device, 203, [0, 3, 2], sizes, 0.01, 100.0)
    add("cases_clip_idle", w, max(max(n) for n in ref.norms) < 100.0)
    w, _ = _steps(rank, world, device, 205, [1, "onehot", 2, "onehot"], sizes, 40.0, 100.0, hot=(1, 3), K=8)
    add("one_hot_and_bag_steps_alternate", w)
    w, _ = _steps(rank, world, device, 207, [2, 3, 0], empty, 1.0, 0.0, hot=(1, 3), K=64)
    add("no_clip", w)
    w, _ = _steps(rank, world, device, 209, [0, 2, 4], sizes, 40.0, 100.0, silent_step=2)
    add("silent_owner", w)
    errs = _dcn_trainer_errors(rank, world)
    out.append(("dcn_trainer", all(v <= TRAINER_BAR for v in errs.values()), " ".join("%s %.2e" % kv for kv in errs.items())))
    return out


NAMES = ["cases_clip_active_hot_row_empty_batch", "cases_clip_idle", "one_hot_and_bag_steps_alternate", "no_clip", "silent_owner", "dcn_trainer"]


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
        assert [n for n, _, _ in got] == NAMES


def test_bag_adam_two_ranks_on_one_gpu(built_lib):
    """(i) two ranks on cuda:0 (gloo, host-staged exchanges)."""
    _check(_run(2, "gloo_same_device"), 2)


def test_bag_adam_over_rccl_one_rank_per_gpu(built_lib):
    """(i) backend nccl (= RCCL), two ranks, one per GPU.  Skipped on a one-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("RCCL at world > 1 needs >= 2 visible GPUs (this box shows %d); the same scenarios run on one GPU over gloo" % n)
    _check(_run(2, "nccl"), 2)
