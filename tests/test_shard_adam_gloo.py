"""Multi-process CPU test of the owner-side sparse Adam over row-sharded tables (dir_amd.shard.ShardedTables.enable_training_adam,
ShardedDCNTrainer) over the gloo backend, world sizes 2, 3 and 8.

What runs here is what runs under RCCL on a GPU box: the gradient exchange, the norm pass, the exact integer sum of the [F] norm shares
over the ranks, the apply pass with the GLOBAL norms -- on the fixed-capacity path, the exact path and the overflow fallback, with one
or two micro-batches, uneven and empty local batches, pruned and out-of-range ids, a table with fewer rows than ranks -- and the
trainer.  The HIP steps cannot run without a GPU: tests/shard_standin_adam.NumpyAdamBackend takes their place.
Reference: oracle.np_ref.sparse_adam_step in float64 on the UNSHARDED tables with the GLOBAL batch, the same on every rank.
Error measure: the one-GPU Adam test's, max |got - ref| / max |ref| per array, for var, m and v separately; bar 1e-6 -- the stand-in's
m and v are float64, its var is stored in fp32 after every step (3 steps x 2^-24 = 1.8e-7 of the scale)."""
import math

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.shard_standin import run_ranks
from tests.shard_standin_adam import NumpyAdamBackend

VOCAB, K, STEPS = [50, 400, 7], 8, 3
LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-4
TOL = 1e-6


def lr_t_of(t):
    return LR * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)


class Reference:
    """float64 Adam over the FULL tables."""

    def __init__(self, full, clip):
        self.T = [t.astype(np.float64) for t in full]
        self.m = [np.zeros(t.shape) for t in full]
        self.v = [np.zeros(t.shape) for t in full]
        self.clip, self.t = clip, 0
        self.norms = []                       # per step: ||g|| of every table's gradient (unclipped)

    def step(self, ids, G):
        from oracle import np_ref as R
        self.t += 1
        Kk = self.T[0].shape[1]
        nf = []
        for f, T in enumerate(self.T):
            g = np.zeros_like(T)
            ok = (ids[:, f] >= 0) & (ids[:, f] < T.shape[0])
            np.add.at(g, ids[ok, f], np.asarray(G, np.float64)[ok, f * Kk:(f + 1) * Kk])
            nf.append(float(np.sqrt((g * g).sum())))
        self.norms.append(nf)
        R.sparse_adam_step(self.T, self.m, self.v, ids, np.asarray(G, np.float64), LR, B1, B2, EPS, self.clip, self.t)


def _draw(seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((v, K)).astype(np.float32) for v in VOCAB]


def _batch(B, seed, rank, step):
    """ids below 0 and past the vocabulary included."""
    rng = np.random.default_rng(seed + 1000 * step + 17 * rank + 5)
    return np.stack([rng.integers(-2, v + 2, size=B) for v in VOCAB], axis=1).astype(np.int64).reshape(B, len(VOCAB))


def _tables(rank, world, seed, clip, **kw):
    from dir_amd.shard import ShardedTables, partition_layout
    full = _draw(seed)
    parts, first, slices = partition_layout(VOCAB, K, world, rank, None)
    local = [torch.from_numpy(full[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    be = NumpyAdamBackend(local, VOCAB, parts, first, world, K)
    st = ShardedTables(local, VOCAB, backend=be, **kw)
    st.enable_training_adam(B1, B2, EPS, clip)
    return st, be, full, slices


def _compare(st, be, ref, slices, what):
    m, v = st.adam_state()
    worst = {"var": 0.0, "m": 0.0, "v": 0.0}
    for f, (s, e) in enumerate(slices):
        if e == s:
            continue
        # the measure is per ARRAY: this rank's rows against the scale of the whole table
        for name, got, want in (("var", be.local[f].numpy(), ref.T[f]), ("m", m[f], ref.m[f]), ("v", v[f], ref.v[f])):
            err = float(np.abs(np.asarray(got, np.float64) - want[s:e]).max() / max(np.abs(want).max(), 1e-300))
            worst[name] = max(worst[name], err)
    assert all(x <= TOL for x in worst.values()), "%s: %s" % (what, worst)
    return worst


def _steps(rank, world, seed, sizes, gscale, clip, kw, silent_step=None, want_active=None):
    """STEPS training steps against the reference, compared after every step.  silent_step: in that step every id whose owner is not
    rank 0 becomes -1, so that every other rank receives nothing live."""
    from oracle import np_ref as R
    st, be, full, slices = _tables(rank, world, seed, clip, **kw)
    ref = Reference(full, clip)
    F = len(VOCAB)
    for step in range(STEPS):
        ids_all = [_batch(sizes[r], seed, r, step) for r in range(world)]
        if step == silent_step:
            for a in ids_all:
                for f in range(F):
                    ok = (a[:, f] >= 0) & (a[:, f] < VOCAB[f])
                    owner, _ = R.shard_div_owner(np.where(ok, a[:, f], 0), VOCAB[f], world)
                    a[:, f] = np.where(ok & (owner == 0), a[:, f], -1)
        G_all = [(gscale * np.random.default_rng(seed + 31 * step + r).standard_normal((sizes[r], F * K))).astype(np.float32) for r in range(world)]
        st.optimizer.lr_t = lr_t_of(step + 1)
        before = st.optimizer.empty_applies
        emb = st.lookup_train(torch.from_numpy(ids_all[rank]))
        (emb * torch.from_numpy(G_all[rank])).sum().backward()
        if step == silent_step and rank != 0:
            assert st.optimizer.empty_applies == before + 1, "rank %d must have received nothing live in the silent step" % rank
        ref.step(np.concatenate(ids_all), np.concatenate(G_all))
        _compare(st, be, ref, slices, "%s, step %d" % (kw, step))
    assert st.optimizer.apply_calls == STEPS and st._updates == STEPS
    assert st.optimizer.norm_calls == (STEPS if clip > 0 else 0), "clip_norm == 0: no norm pass (and no collective)"
    if want_active is not None:
        top = max(max(n) for n in ref.norms)
        assert (top > clip) == want_active, "the reference's largest table-gradient norm is %g, clip %g" % (top, clip)
    return st, ref


def _sizes(world, empty=True):
    return [0 if (empty and r == 1) else 5 + 3 * r for r in range(world)]


def sc_paths(rank, world):
    """The fixed path, mode="exact", chunks 1 and 2, clip idle / active / off; uneven batches with an empty one; 7 rows < 8 ranks."""
    sizes = _sizes(world)
    for kw in ({}, {"mode": "exact"}, {"chunks": 1}, {"chunks": 2, "force_collective": True}):
        _steps(rank, world, 11, sizes, 1.0, 100.0, kw, want_active=False)          # clip idle
        _steps(rank, world, 13, sizes, 40.0, 100.0, kw, want_active=True)          # clip active
    _steps(rank, world, 17, sizes, 1.0, 0.0, {})                                   # no clip: no norm pass
    return "ok"


def sc_overflow(rank, world):
    """A slab so small that the first training lookup overflows: the step is repeated on the exact path inside the step."""
    st, _ = _steps(rank, world, 19, [40 + r for r in range(world)], 40.0, 100.0,
                   {"slack": 0.1, "mode": "fixed", "chunks": 1, "force_collective": True}, want_active=True)
    assert st.stats["fallbacks"] >= 1, st.stats
    return "fallbacks %d" % st.stats["fallbacks"]


def sc_silent(rank, world):
    """One silent owner: in step 1 only rank 0 receives live entries; every other rank's var / m / v still follow the reference (they
    decay and step with zero gradient) and still take part in the norm sum."""
    for kw in ({}, {"mode": "exact"}):
        _steps(rank, world, 23, _sizes(world, empty=False), 40.0, 100.0, kw, silent_step=1)
    return "ok"


def sc_unsupported(rank, world):
    """with_linear, bags and groups=2 each raise under Adam; nothing is half-supported."""
    from dir_amd.shard import ShardedTables, partition_layout
    st, be, full, slices = _tables(rank, world, 29, 100.0)
    st.attach_linear([torch.zeros(t.shape[0]) for t in st.local_tables])
    st.enable_linear_training(0.1)
    ids = torch.from_numpy(_batch(4, 29, rank, 0))
    with pytest.raises(NotImplementedError, match="with_linear"):
        st.lookup_train(ids, with_linear=True)
    with pytest.raises(NotImplementedError, match="lookup_bags_train"):
        st.lookup_bags_train(torch.zeros(0, dtype=torch.int64), torch.zeros(4 * len(VOCAB) + 1, dtype=torch.int64))
    parts, first, sl = partition_layout(VOCAB, K, world, rank, None)
    local2 = [torch.zeros((e - s, 2 * K)) for s, e in sl]
    st2 = ShardedTables(local2, VOCAB, backend=NumpyAdamBackend(local2, VOCAB, parts, first, world, 2 * K), groups=2)
    with pytest.raises(NotImplementedError, match="groups"):
        st2.enable_training_adam()
    with pytest.raises(ValueError):
        st.enable_training_adam(beta1=1.0)
    return "ok"


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------
class _TinyDCN(torch.nn.Module):
    """What ShardedDCNTrainer uses of a dcn.DeepCrossNetwork (input_layer, hparams, hidden, forward(x0), predict(x0)), in torch ops --
    the HIP model cannot run without a GPU.  forward(features dict) looks the embedding columns up in the model's OWN tables: the
    unsharded reference."""

    def __init__(self, columns, hidden, hparams):
        super().__init__()
        from dir_amd.input_layer import InputLayer
        self.input_layer = InputLayer(columns)
        d = self.input_layer.column_num
        self.hparams = dict(weight_column=None, dnn_dropout=None, optimizer=None, **hparams)
        g = torch.Generator().manual_seed(5)
        self.cross_w = torch.nn.Parameter(0.1 * torch.randn(2, d, generator=g))
        self.cross_b = torch.nn.Parameter(0.1 * torch.randn(2, d, generator=g))
        self.hidden = torch.nn.ModuleList()
        h = d
        for n in hidden:
            self.hidden.append(torch.nn.Linear(h, n))
            h = n
        self.logits_layer = torch.nn.Linear(d + h, 1)
        with torch.no_grad():
            for p in list(self.hidden.parameters()) + list(self.logits_layer.parameters()):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            for p in self.input_layer.embedding_weights:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))

    def x0_of(self, features):
        from dir_amd.feature_column import EmbeddingColumn
        il, pieces, e = self.input_layer, [], 0
        for c in il.columns:                                   # name-sorted
            if isinstance(c, EmbeddingColumn):
                pieces.append(il.embedding_weights[e][features[c.categorical_column.key]])
                e += 1
            else:
                pieces.append(features[c.key].float().reshape(-1, 1))
        return torch.cat(pieces, dim=1)

    def forward(self, x):
        x0 = x if isinstance(x, torch.Tensor) else self.x0_of(x)
        xl = x0
        for l in range(2):
            xl = x0 * (xl @ self.cross_w[l]).unsqueeze(1) + self.cross_b[l] + xl
        net = x0
        for lin in self.hidden:
            net = torch.relu(lin(net))
        return self.logits_layer(torch.cat([xl, net], dim=1))

    @torch.no_grad()
    def predict(self, x):
        logits = self.forward(x)
        return {"logits": logits, "logistic": torch.sigmoid(logits)}


def _tiny(V, Kc):
    from dir_amd import feature_column as fc
    # "C0_embedding" < "C0_x" < "C1_embedding" < "C1_x" < "C2_embedding": embedding and numeric columns interleave in sorted order
    cols = [fc.embedding_column(fc.categorical_column_with_identity("C%d" % i, V), Kc) for i in range(3)]
    cols += [fc.numeric_column("C%d_x" % i) for i in range(2)]
    hp = dict(optimizer_spec={"epsilon": 1e-4}, l2_reg=1e-2,
              learning_rate_spec={"learning_rate": 0.01, "decay_method": "cosine_decay", "decay_steps": 100, "alpha": 0.5})
    return _TinyDCN(cols, [12, 6], hp)


def sc_trainer(rank, world):
    """ShardedDCNTrainer against train_spec.TrainStep on the concatenated batch, CPU tensors, uneven local batches: the global-mean
    loss scaling, the l2 term counted once, the per-tensor clip on the summed gradients, global_step, predict."""
    from dir_amd.shard import ShardedDCNTrainer, ShardedTables, partition_layout
    from dir_amd.train_spec import TrainStep
    V, Kc, steps = 23, 4, 3
    sizes = [5 + 6 * r for r in range(world)]
    model, ref_model = _tiny(V, Kc), _tiny(V, Kc)
    names = [c.name for c in model.input_layer.columns]
    assert names == sorted(names) and [n.endswith("_embedding") for n in names] == [True, False, True, False, True]
    vocab = [V] * 3
    parts, first, slices = partition_layout(vocab, Kc, world, rank, None)
    local = [p.data[s:e].clone() for p, (s, e) in zip(model.input_layer.embedding_weights, slices)]
    st = ShardedTables(local, vocab, backend=NumpyAdamBackend(local, vocab, parts, first, world, Kc))
    tr = ShardedDCNTrainer(model, st)
    hp = ref_model.hparams
    # (params= keeps TrainStep from attaching the HIP Adam to the reference's tables: on CPU tensors torch's dense Adam steps every row)
    ref_step = TrainStep(ref_model, optimizer="Adam", optimizer_spec=hp["optimizer_spec"], learning_rate_spec=hp["learning_rate_spec"],
                         l2_reg=hp["l2_reg"], l2_params=[lin.weight for lin in ref_model.hidden], params=list(ref_model.parameters()))
    bad = _tiny(V, Kc)
    bad.hparams["weight_column"] = "w"
    with pytest.raises(NotImplementedError, match="weight_column"):
        ShardedDCNTrainer(bad, st)
    bad.hparams.update(weight_column=None, dnn_dropout=0.5)
    with pytest.raises(NotImplementedError, match="dropout"):
        ShardedDCNTrainer(bad, st)

    def feats(step):
        g = torch.Generator().manual_seed(100 + step)
        n = sum(sizes)
        f = {"C%d" % i: torch.randint(0, V, (n,), generator=g) for i in range(3)}
        f.update({"C%d_x" % i: torch.randn(n, generator=g) for i in range(2)})
        f["C0"][::3] = 3                                      # one row in every rank's batch, several times
        return f, torch.randint(0, 2, (n, 1), generator=g).float()

    off = sum(sizes[:rank])
    for step in range(steps):
        f_all, y_all = feats(step)
        mine = {k: v[off:off + sizes[rank]] for k, v in f_all.items()}
        loss = tr.step(mine, y_all[off:off + sizes[rank]])
        logits = ref_model(f_all)
        ref_loss, _ = ref_step(torch.nn.functional.binary_cross_entropy_with_logits(logits, y_all, reduction="mean"))
        total = loss.detach().clone().reshape(1)
        dist.all_reduce(total)
        assert abs(float(total) - float(ref_loss)) <= 1e-5, "the ranks' loss shares add up to the global loss (l2 once): %g vs %g" % (float(total), float(ref_loss))
    assert tr.global_step == steps == ref_step.global_step
    errs = {}
    for (n, p), (_, q) in zip(model.named_parameters(), ref_model.named_parameters()):
        if "embedding_weights" not in n:
            errs[n] = float((p.detach() - q.detach()).abs().max())
    for f, (s, e) in enumerate(slices):
        errs["table%d" % f] = float((st.local_tables[f] - ref_model.input_layer.embedding_weights[f].detach()[s:e]).abs().max()) if e > s else 0.0
    f_all, _ = feats(99)
    mine = {k: v[off:off + sizes[rank]] for k, v in f_all.items()}
    got, want = tr.predict(mine), ref_model.predict(f_all)
    errs["predict"] = float((got["logits"] - want["logits"][off:off + sizes[rank]]).abs().max())
    assert all(v <= 1e-5 for v in errs.values()), errs
    return "ok"


_FUNCS = dict(paths=sc_paths, overflow=sc_overflow, silent=sc_silent, unsupported=sc_unsupported, trainer=sc_trainer)


def _scenarios(rank, world, names):
    return [(n, _FUNCS[n](rank, world)) for n in names]


def _run(world, names):
    res = run_ranks(world, _scenarios, names, timeout=600)
    for rank, got in sorted(res.items()):
        assert [n for n, _ in got] == list(names), "rank %d ran %s" % (rank, got)
    return res


@pytest.mark.parametrize("world", [2, 3, 8])
def test_owner_side_adam_matches_float64_on_every_path(world):
    _run(world, ("paths", "overflow"))


@pytest.mark.parametrize("world", [2, 3, 8])
def test_a_silent_owner_still_decays_and_joins_the_norm_sum(world):
    _run(world, ("silent", "unsupported"))


def test_dcn_trainer_world2_equals_trainstep_on_the_global_batch():
    _run(2, ("trainer",))
