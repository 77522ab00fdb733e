"""Multi-process CPU test of the owner-side sparse Adam over multi-hot bags (dir_amd.shard.ShardedTables.lookup_bags_train under
enable_training_adam, ShardedDCNTrainer on ragged features) over the gloo backend, world sizes 1, 2, 3 and 8.

What runs here is what runs under RCCL on a GPU box: the training plans of the bag lookup, the gradient scatter and the reversed
partial-row exchange, then the owner's step in its two halves around the exact integer sum of the norm shares -- on every rank, also
one whose slabs hold no live record.  The HIP steps cannot run without a GPU: tests/shard_standin_bags_adam.NumpyBagsAdamBackend takes
their place.  Setting: tests/test_shard_adam_gloo.py's (vocab [50, 400, 7] -- a table with fewer rows than ranks at world 8 --, K = 8,
3 steps) with the bags and cases of tests/test_shard_bags_gloo.py.
Reference: float64 torch autograd of test_shard_bags_train_gloo.bags_forward64 over the FULL tables on the GLOBAL batch, then a float64
dense Adam with the per-table clip_by_norm in which every row moves (shard_standin_bags_adam.BagsAdamReference), the same on every rank.
Error measure and bar: test_shard_adam_gloo's -- max |got - ref| / max |ref| per array for var, m and v separately, 1e-6."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.shard_standin import run_ranks
from tests.shard_standin_adam import NumpyAdamBackend
from tests.shard_standin_bags_adam import BagsAdamReference, NumpyBagsAdamBackend
from tests.test_shard_adam_gloo import B1, B2, EPS, K, LR, STEPS, VOCAB, _batch, _compare, _draw, _TinyDCN, lr_t_of
from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr

MAX_LEN = [3, 12, 4]
F = len(VOCAB)


def _tables(rank, world, seed, clip, backend=NumpyBagsAdamBackend, **kw):
    from dir_amd.shard import ShardedTables, partition_layout
    full = [0.5 * t for t in _draw(seed)]                          # row norms around 1.4: some above the cases' max_norm, some below
    parts, first, slices = partition_layout(VOCAB, K, world, rank, None)
    local = [torch.from_numpy(full[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    be = backend(local, VOCAB, parts, first, world, K)
    st = ShardedTables(local, VOCAB, backend=be, **kw)
    st.enable_training_adam(B1, B2, EPS, clip)
    return st, be, full, slices


def _sizes(world, empty=True):
    return [0 if (empty and r == 1) else 5 + 3 * r for r in range(world)]


def _silence(bags_all, world):
    """Every id whose owner is not rank 0 becomes -1: every other rank receives no live record."""
    from oracle import np_ref as R
    for bl in bags_all:
        for row in bl:
            for f in range(F):
                ids, _ = row[f]
                ok = (ids >= 0) & (ids < VOCAB[f])
                owner, _ = R.shard_div_owner(np.where(ok, ids, 0), VOCAB[f], world)
                ids[:] = np.where(ok & (np.asarray(owner) == 0), ids, -1)


def _steps(rank, world, seed, kinds, sizes, gscale, clip, kw=None, hot=None, silent_step=None, want_active=None):
    """One training step per entry of `kinds` (an index into CASES, or "onehot") against the reference, compared after every step."""
    st, be, full, slices = _tables(rank, world, seed, clip, **(kw or {}))
    ref = BagsAdamReference(full, LR, B1, B2, EPS, clip)
    for step, kind in enumerate(kinds):
        rng = np.random.default_rng(seed + 1000 * step)            # every rank draws the GLOBAL batch, then takes its own part
        G_all = [(gscale * rng.standard_normal((sizes[r], F * K))).astype(np.float32) for r in range(world)]
        st.optimizer.lr_t = lr_t_of(step + 1)
        before = st.optimizer.empty_applies
        if kind == "onehot":
            ids_all = [_batch(sizes[r], seed, r, step) for r in range(world)]
            emb = st.lookup_train(torch.from_numpy(ids_all[rank]))
            emb.backward(torch.from_numpy(G_all[rank]))
            ref.step_onehot(np.concatenate(ids_all), np.concatenate(G_all))
        else:
            wmode, comb, mn, fmaj, prune = CASES[kind]
            bags_all = [draw_bags(rng, sizes[r], VOCAB, MAX_LEN, wmode) for r in range(world)]
            if hot is not None:                                     # one row repeated inside bags, across bags and across ranks
                f_h, id_h = hot
                for bl in bags_all:
                    for row in bl:
                        if len(row[f_h][0]) >= 2:
                            row[f_h][0][:2] = id_h
            if step == silent_step:
                _silence(bags_all, world)
            v, o, w = to_csr(bags_all[rank], F, fmaj)
            emb = st.lookup_bags_train(torch.from_numpy(v), torch.from_numpy(o), None if w is None else torch.from_numpy(w), combiner=comb,
                                       max_norm=mn, field_major=fmaj, flags=1 if prune else 0)
            assert emb.shape == (sizes[rank], F * K) and emb.requires_grad
            emb.backward(torch.from_numpy(G_all[rank]))
            if step == silent_step and rank != 0:
                assert st.optimizer.empty_applies == before + 1, "rank %d must have received no live record in the silent step" % rank
            ref.step([b for bl in bags_all for b in bl], np.concatenate(G_all), comb, mn, prune)
        _compare(st, be, ref, slices, "kinds %s, step %d (%s), scale %g, clip %g" % (kinds, step, kind, gscale, clip))
    assert st.optimizer.apply_calls == len(kinds) and st._updates == len(kinds)
    assert st.optimizer.norm_calls == (len(kinds) if clip > 0 else 0), "clip_norm == 0: no norm pass (and no collective)"
    if want_active is not None:
        top = max(max(n) for n in ref.norms)
        assert (top > clip) == want_active, "the reference's largest table-gradient norm is %g, clip %g" % (top, clip)
    return st, ref


def sc_cases(rank, world):
    """Every CASES combination (sum / mean / sqrtn, weights, pruning, max_norm, field-major), clip idle and active; uneven batches with
    an empty one; 7 rows < 8 ranks."""
    sizes = _sizes(world)
    for c in range(len(CASES)):
        _steps(rank, world, 11 + c, [c] * STEPS, sizes, 0.01, 100.0, want_active=False)       # clip idle
        _steps(rank, world, 31 + c, [c] * STEPS, sizes, 40.0, 100.0, want_active=True)        # clip active
    return "ok"


def sc_mixed(rank, world):
    """A hot row repeated inside bags, across bags and across ranks; one-hot and bag steps alternating on one ShardedTables; clip 0
    (no norm call, no collective); a silent owner."""
    sizes = _sizes(world, empty=False)
    _steps(rank, world, 51, [0, 2, 1], sizes, 40.0, 100.0, hot=(1, 3), want_active=True)
    _steps(rank, world, 53, [1, "onehot", 2], sizes, 40.0, 100.0, hot=(1, 3))
    _steps(rank, world, 55, ["onehot", 4, "onehot"], _sizes(world), 0.01, 100.0)
    _steps(rank, world, 57, [2, 3, 0], _sizes(world), 1.0, 0.0, hot=(1, 3))
    _steps(rank, world, 59, [0, 2, 4], sizes, 40.0, 100.0, silent_step=1)
    return "ok"


def sc_refusals(rank, world):
    """with_linear under Adam stays refused; a backend without the bag form raises with the documented words; the Adagrad route stands."""
    st, be, full, slices = _tables(rank, world, 61, 100.0)
    st.attach_linear([torch.zeros(t.shape[0]) for t in st.local_tables])
    st.enable_linear_training(0.1)
    v, o = torch.zeros(0, dtype=torch.int64), torch.zeros(4 * F + 1, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="with_linear"):
        st.lookup_bags_train(v, o, with_linear=True)
    st2, _, _, _ = _tables(rank, world, 61, 100.0, backend=NumpyAdamBackend)
    with pytest.raises(NotImplementedError, match="^lookup_bags_train under enable_training_adam"):
        st2.lookup_bags_train(v, o)
    return "ok"


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------
class _TinyBagDCN(_TinyDCN):
    """test_shard_adam_gloo._TinyDCN whose own (unsharded) lookup takes ragged and weighted features: every embedding column's bag with
    its combiner and max_norm, in torch ops ([TF-upstream] safe_embedding_lookup_sparse as the input layer applies it)."""

    def x0_of(self, features):
        from dir_amd._input import categorical_of
        from dir_amd.feature_column import EmbeddingColumn
        il, pieces, e = self.input_layer, [], 0
        for c in il.columns:                                   # name-sorted
            if not isinstance(c, EmbeddingColumn):
                pieces.append(features[c.key].float().reshape(-1, 1))
                continue
            table = il.embedding_weights[e]
            e += 1
            got = categorical_of(c).ids(features, torch.device("cpu"))
            if not isinstance(got, tuple):
                got = (got, torch.arange(got.numel() + 1), None)
            vals, offs, w = got
            B = offs.numel() - 1
            bag = torch.repeat_interleave(torch.arange(B), offs[1:] - offs[:-1])
            ok = vals >= 0
            r = table[vals[ok]]
            if c.max_norm:
                r = r * (c.max_norm / torch.clamp_min(r.norm(dim=1, keepdim=True), c.max_norm))
            ww = torch.ones(int(ok.sum())) if w is None else w[ok].float()
            out = torch.zeros((B, table.shape[1])).index_add(0, bag[ok], ww[:, None] * r)
            cnt = torch.zeros(B).index_add(0, bag[ok], torch.ones_like(ww))
            if c.combiner == "mean":
                den = torch.zeros(B).index_add(0, bag[ok], ww) if w is not None else cnt
            elif c.combiner == "sqrtn":
                den = (torch.zeros(B).index_add(0, bag[ok], ww * ww) if w is not None else cnt).sqrt()
            else:
                den = torch.ones(B)
            pieces.append(out / torch.where(cnt > 0, den, torch.ones_like(den))[:, None])
        return torch.cat(pieces, dim=1)


def tiny_bag_columns(V, Kc):
    """A ragged column with max_norm, a weighted one, a one-hot one with max_norm, interleaved with numeric columns in sorted order."""
    from dir_amd import feature_column as fc
    ident = [fc.categorical_column_with_identity("C%d" % i, V) for i in range(3)]
    cols = [fc.embedding_column(ident[0], Kc, combiner="sqrtn", max_norm=0.9),
            fc.embedding_column(fc.weighted_categorical_column(ident[1], "C1_w"), Kc, combiner="mean"),
            fc.embedding_column(ident[2], Kc, combiner="sum", max_norm=1.2)]
    cols += [fc.numeric_column("C%d_x" % i) for i in range(2)]
    return cols


def tiny_bag_features(V, n, seed):
    """n samples: C0 bags of 0..4 ids (a hot id, some -1), C1 weighted bags of 1..3, C2 one id per sample; two numerics; labels."""
    g = torch.Generator().manual_seed(seed)
    l0 = torch.randint(0, 5, (n,), generator=g)
    l1 = torch.randint(1, 4, (n,), generator=g)
    v0 = torch.randint(-1, V, (int(l0.sum()),), generator=g)
    v0[::3] = 3                                                 # one row in every rank's batch, inside bags and across them
    v1 = torch.randint(0, V, (int(l1.sum()),), generator=g)
    w1 = torch.rand(int(l1.sum()), generator=g) * 1.9 + 0.1
    feats = {"C0": (v0, l0), "C1": (v1, l1), "C1_w": (w1, l1), "C2": torch.randint(0, V, (n,), generator=g)}
    feats.update({"C%d_x" % i: torch.randn(n, generator=g) for i in range(2)})
    return feats, torch.randint(0, 2, (n, 1), generator=g).float()


def take_samples(feats, lo, hi):
    """The samples [lo, hi) of tiny_bag_features' dict, as the features dict a model takes (Ragged for the multi-hot ones)."""
    from dir_amd.feature_column import Ragged
    out = {}
    for k, v in feats.items():
        if isinstance(v, tuple):
            vals, lens = v
            offs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
            out[k] = Ragged(vals[int(offs[lo]):int(offs[hi])].clone(), (offs[lo:hi + 1] - offs[lo]).clone())
        else:
            out[k] = v[lo:hi]
    return out


def _tiny_bag(V, Kc):
    hp = dict(optimizer_spec={"epsilon": 1e-4}, l2_reg=1e-2,
              learning_rate_spec={"learning_rate": 0.01, "decay_method": "cosine_decay", "decay_steps": 100, "alpha": 0.5})
    return _TinyBagDCN(tiny_bag_columns(V, Kc), [12, 6], hp)


def sc_trainer(rank, world):
    """ShardedDCNTrainer on ragged + weighted + max_norm columns against train_spec.TrainStep on the concatenated batch, as
    test_shard_adam_gloo.sc_trainer does for one-hot ids (same bars); a backend without the bag Adam raises at the first ragged batch."""
    from dir_amd.shard import ShardedDCNTrainer, ShardedTables, partition_layout
    from dir_amd.train_spec import TrainStep
    V, Kc, steps = 23, 4, 3
    sizes = [5 + 6 * r for r in range(world)]
    model, ref_model = _tiny_bag(V, Kc), _tiny_bag(V, Kc)
    names = [c.name for c in model.input_layer.columns]
    assert names == sorted(names) and [n.endswith("_embedding") for n in names] == [True, False, True, False, True]
    vocab = [V] * 3
    parts, first, slices = partition_layout(vocab, Kc, world, rank, None)

    def sharded(m, backend):
        local = [p.data[s:e].clone() for p, (s, e) in zip(m.input_layer.embedding_weights, slices)]
        return ShardedTables(local, vocab, backend=backend(local, vocab, parts, first, world, Kc))
    st = sharded(model, NumpyBagsAdamBackend)
    tr = ShardedDCNTrainer(model, st)
    hp = ref_model.hparams
    ref_step = TrainStep(ref_model, optimizer="Adam", optimizer_spec=hp["optimizer_spec"], learning_rate_spec=hp["learning_rate_spec"],
                         l2_reg=hp["l2_reg"], l2_params=[lin.weight for lin in ref_model.hidden], params=list(ref_model.parameters()))
    off, n = sum(sizes[:rank]), sum(sizes)
    plain = _tiny_bag(V, Kc)
    tr_plain = ShardedDCNTrainer(plain, sharded(plain, NumpyAdamBackend))          # constructs; refuses at the first ragged batch
    f_all, y_all = tiny_bag_features(V, n, 100)
    with pytest.raises(NotImplementedError, match="^lookup_bags_train under enable_training_adam"):
        tr_plain.step(take_samples(f_all, off, off + sizes[rank]), y_all[off:off + sizes[rank]])
    for step in range(steps):
        f_all, y_all = tiny_bag_features(V, n, 100 + step)
        loss = tr.step(take_samples(f_all, off, off + sizes[rank]), y_all[off:off + sizes[rank]])
        logits = ref_model(take_samples(f_all, 0, n))
        ref_loss, _ = ref_step(torch.nn.functional.binary_cross_entropy_with_logits(logits, y_all, reduction="mean"))
        total = loss.detach().clone().reshape(1)
        dist.all_reduce(total)
        assert abs(float(total) - float(ref_loss)) <= 1e-5, "the ranks' loss shares add up to the global loss (l2 once): %g vs %g" % (float(total), float(ref_loss))
    assert tr.global_step == steps == ref_step.global_step
    errs = {}
    for (nm, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters()):
        if "embedding_weights" not in nm:
            errs[nm] = float((p.detach() - q.detach()).abs().max())
    for f, (s, e) in enumerate(slices):
        errs["table%d" % f] = float((st.local_tables[f] - ref_model.input_layer.embedding_weights[f].detach()[s:e]).abs().max()) if e > s else 0.0
    f_all, _ = tiny_bag_features(V, n, 199)
    got, want = tr.predict(take_samples(f_all, off, off + sizes[rank])), ref_model.predict(take_samples(f_all, 0, n))
    errs["predict"] = float((got["logits"] - want["logits"][off:off + sizes[rank]]).abs().max())
    assert all(v <= 1e-5 for v in errs.values()), errs
    return "ok"


_FUNCS = dict(cases=sc_cases, mixed=sc_mixed, refusals=sc_refusals, trainer=sc_trainer)


def _scenarios(rank, world, names):
    return [(n, _FUNCS[n](rank, world)) for n in names]


def _run(world, names):
    res = run_ranks(world, _scenarios, names, timeout=600)
    for rank, got in sorted(res.items()):
        assert [n for n, _ in got] == list(names), "rank %d ran %s" % (rank, got)
    return res


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_owner_side_bag_adam_matches_float64_on_every_case(world):
    _run(world, ("cases",))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_hot_rows_alternating_steps_no_clip_and_a_silent_owner(world):
    _run(world, ("mixed", "refusals"))


def test_dcn_trainer_world2_on_ragged_features_equals_trainstep_on_the_global_batch():
    _run(2, ("trainer",))
