"""Multi-process CPU test of de-duplicated training lookups over row-sharded tables (dir_amd.shard.ShardedTables.lookup_train(dedup=True),
lookup_rows_train / backward_rows) over the gloo backend, world sizes 2 and 3.

What runs here is what runs under RCCL on a GPU box: the de-duplicating bucket pass on the training plans' own capacity, the exchanges,
the requester-side scatter-sum of the entry gradients into the slab positions they share, the reversed exchange and the owner's step
(Adagrad, or Adam with its norm exchange) -- on the fixed-capacity path and after a forced overflow.  The HIP steps cannot run without a
GPU: tests/shard_standin_din.NumpyDinBackend takes their place (rows_scatter_sum in the kernels' order and arithmetic).
Reference: oracle.np_ref.sparse_adagrad_step / sparse_adam_step in float64 on the UNSHARDED tables with the GLOBAL batch.
Error measure and bar: tests/hot_rows_inputs.scaled, |got - ref| / (1 + |ref|) <= 1e-5 -- the project's bar for sorted run sums."""
import math

import numpy as np
import pytest
import torch

from tests.hot_rows_inputs import BAR, scaled
from tests.shard_standin import run_ranks
from tests.shard_standin_din import NumpyDinBackend

VOCAB, K = [50, 400, 1], 8           # the last table has fewer rows than ranks
F = len(VOCAB)
LR = 0.05
ADAM = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-4, clip=3.0)


def _draw(seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((v, K)).astype(np.float32) for v in VOCAB]


def _uniform(B, seed, rank):
    """ids below 0 and past the vocabulary included; a third of the samples repeat one row per slot."""
    rng = np.random.default_rng(seed + 17 * rank + 5)
    ids = np.stack([rng.integers(-2, v + 2, size=B) for v in VOCAB], axis=1).astype(np.int64).reshape(B, F)
    ids[::3] = np.minimum(3, np.array(VOCAB) - 1)
    return ids


def _zipf(B, seed, rank):
    rng = np.random.default_rng(seed + 17 * rank + 7)
    return np.stack([np.minimum(rng.zipf(1.05, size=B) - 1, v - 1) for v in VOCAB], axis=1).astype(np.int64).reshape(B, F)


def _hot(B, seed, rank):
    """Rank 0: 4096 samples, 3000 of them on row 7 of slot 0; the others a handful of uniform samples."""
    if rank:
        return _uniform(6 + rank, seed, rank)
    rng = np.random.default_rng(seed + 3)
    ids = np.stack([rng.integers(-1, v, size=4096) for v in VOCAB], axis=1).astype(np.int64)
    ids[ids[:, 0] == 7, 0] = 8
    ids[np.sort(rng.permutation(4096)[:3000]), 0] = 7
    return ids


def _grads(ids_all, seed, scale=1.0):
    return [(scale * np.random.default_rng(seed + 31 + r).standard_normal((a.shape[0], F * K))).astype(np.float32) for r, a in enumerate(ids_all)]


def _tables(rank, world, seed, adam=False, **kw):
    from dir_amd.shard import ShardedTables, partition_layout
    full = _draw(seed)
    parts, first, slices = partition_layout(VOCAB, K, world, rank, None)
    local = [torch.from_numpy(full[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    be = NumpyDinBackend(local, VOCAB, parts, first, world, K)
    st = ShardedTables(local, VOCAB, backend=be, **kw)
    if adam:
        st.enable_training_adam(ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["clip"])
    else:
        st.enable_training(LR, 0.1)
    return st, be, full, slices


class Reference:
    """The float64 synchronous step over the FULL tables and the GLOBAL batch."""

    def __init__(self, full, adam=False):
        self.T = [t.astype(np.float64) for t in full]
        self.adam, self.t = adam, 0
        if adam:
            self.m, self.v = [np.zeros(t.shape) for t in full], [np.zeros(t.shape) for t in full]
        else:
            self.a = [np.full(t.shape, 0.1) for t in full]

    def step(self, ids_all, G_all):
        from oracle import np_ref as R
        ids, G = np.concatenate(ids_all), np.concatenate(G_all).astype(np.float64)
        ids = np.where((ids >= 0) & (ids < np.array(VOCAB)[None, :]), ids, -1)
        self.t += 1
        if self.adam:
            R.sparse_adam_step(self.T, self.m, self.v, ids, G, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["clip"], self.t)
        else:
            R.sparse_adagrad_step(self.T, self.a, ids, G, LR)

    def compare(self, st, be, slices, what):
        worst = 0.0
        for f, (s, e) in enumerate(slices):
            if e == s:
                continue
            pairs = [(be.local[f].numpy(), self.T[f])]
            if self.adam:
                m, v = st.adam_state()
                pairs += [(m[f], self.m[f]), (v[f], self.v[f])]
            else:
                pairs += [(st.optimizer["acc"][f], self.a[f])]
            worst = max([worst] + [scaled(got, want[s:e]) for got, want in pairs])
        assert worst <= BAR, "%s: %.3e off the float64 synchronous step" % (what, worst)
        return worst


def _lr_t(t):
    return ADAM["lr"] * math.sqrt(1.0 - ADAM["b2"] ** t) / (1.0 - ADAM["b1"] ** t)


def _train(st, ids, G, dedup):
    if st._adam:
        st.optimizer.lr_t = _lr_t(st._updates + 1)
    emb = st.lookup_train(torch.from_numpy(ids), dedup=dedup)
    (emb * torch.from_numpy(G)).sum().backward()
    return emb.detach()


def _sizes(world):
    return [0 if r == 1 else 9 + 4 * r for r in range(world)]          # uneven, rank 1 empty


def sc_steps(rank, world, adam):
    """dedup=True, dedup=False, dedup=True: every step against the reference; the forward bit for bit dedup=False's; capacities apart."""
    for kw in ({}, {"chunks": 1}, {"chunks": 2, "force_collective": True}):
        st, be, full, slices = _tables(rank, world, 11, adam=adam, **kw)
        ref = Reference(full, adam)
        for step, dedup in enumerate((True, False, True)):
            ids_all = [_uniform(n, 100 + step, r) for r, n in enumerate(_sizes(world))]
            G_all = _grads(ids_all, 200 + step, 4.0 if adam else 1.0)
            with torch.no_grad():
                plain = st.lookup(torch.from_numpy(ids_all[rank]))
            calls = be.scatter_calls
            emb = _train(st, ids_all[rank], G_all[rank], dedup)
            assert torch.equal(emb, plain), "lookup_train(dedup=%s)'s forward differs from the lookup's" % dedup
            assert (be.scatter_calls > calls) == dedup, "the scatter-sum runs under dedup=True only"
            ref.step(ids_all, G_all)
            ref.compare(st, be, slices, "%s step %d dedup=%s" % (kw, step, dedup))
        assert st.stats["fallbacks"] == 0 and st._updates == 3
        # the one-position-per-entry capacity is what the first lookup agreed on; the de-duplicated one may only have shrunk
        assert st._cap_train == st._cap0 and st._cap_train_dedup <= st._cap0, (st._cap_train, st._cap_train_dedup, st._cap0)
    return "ok"


def sc_forward_bitwise(rank, world):
    """The two training forwards side by side on twin tables (same shards): bitwise equal outputs."""
    a, _, _, _ = _tables(rank, world, 13)
    b, _, _, _ = _tables(rank, world, 13)
    ids = torch.from_numpy(_zipf(40 + 5 * rank, 300, rank))
    ea, eb = a.lookup_train(ids, dedup=True), b.lookup_train(ids)
    assert torch.equal(ea.detach(), eb.detach())
    return "ok"


def sc_zipf(rank, world):
    """Zipf(1.05) ids: fewer payload words leave this rank than it has live entries (read off the slab headers), and the step holds."""
    st, be, full, slices = _tables(rank, world, 17, chunks=1)
    ref = Reference(full)
    ids_all = [_zipf(120 + 10 * r, 400, r) for r in range(world)]
    G_all = _grads(ids_all, 500)
    _train(st, ids_all[rank], G_all[rank], True)
    plan = [p for (B, slot, cap), p in st._plans.items() if slot == "train_dedup"][0]
    sent = int((plan.send_all.view(-1, plan.cap + 1)[:, 0] & 0xffffffff).sum())
    live = int(((ids_all[rank] >= 0) & (ids_all[rank] < np.array(VOCAB)[None, :])).sum())
    assert 0 < sent < live, "de-duplicated demand %d, live entries %d" % (sent, live)
    assert be.longest_run > 1
    ref.step(ids_all, G_all)
    ref.compare(st, be, slices, "zipf")
    return "sent %d of %d" % (sent, live)


def sc_hot(rank, world, adam):
    """One row hit 3000 times in 4096 samples of rank 0: one run of 3000 entries through the tiles' compensated sums."""
    st, be, full, slices = _tables(rank, world, 19, adam=adam, chunks=1)
    ref = Reference(full, adam)
    ids_all = [_hot(0, 600, r) for r in range(world)]
    G_all = _grads(ids_all, 700, 0.5)
    _train(st, ids_all[rank], G_all[rank], True)
    if rank == 0:
        assert be.longest_run >= 3000, be.longest_run
    ref.step(ids_all, G_all)
    return "%.2e" % ref.compare(st, be, slices, "hot row")


def sc_overflow(rank, world, adam):
    """Slabs too small for the first de-duplicated training lookup: it ends on the exact path (one row per entry: the scatter-sum sees
    runs of one) with the same result."""
    st, be, full, slices = _tables(rank, world, 23, adam=adam, slack=0.05, mode="fixed", chunks=1, force_collective=True)
    ref = Reference(full, adam)
    rng = np.random.default_rng(900)
    ids_all = [np.stack([rng.permutation(400)[:40 + r] % v for v in VOCAB], axis=1).astype(np.int64) for r in range(world)]   # (mostly distinct rows)
    G_all = _grads(ids_all, 800)
    with torch.no_grad():
        plain = st.lookup(torch.from_numpy(ids_all[rank]))
    fb = st.stats["fallbacks"]
    emb = _train(st, ids_all[rank], G_all[rank], True)
    assert st.stats["fallbacks"] > fb, st.stats
    assert torch.equal(emb, plain)
    assert be.scatter_calls == 1 and be.longest_run == 1, (be.scatter_calls, be.longest_run)
    ref.step(ids_all, G_all)
    ref.compare(st, be, slices, "overflow")
    return "ok"


def sc_rows(rank, world, adam):
    """lookup_rows_train: rows[inv] is the full table's row bit for bit; backward_rows with the per-entry gradients in a shuffled order
    takes the same step; an inference lookup in between leaves the training buffers alone; backward_rows runs once."""
    for kw, dedup in (({}, True), ({"chunks": 1}, True), ({}, False), ({"mode": "exact"}, True)):
        st, be, full, slices = _tables(rank, world, 29, adam=adam, **kw)
        ref = Reference(full, adam)
        ids_all = [_uniform(n, 1000, r) for r, n in enumerate(_sizes(world))]
        G_all = _grads(ids_all, 1100, 4.0 if adam else 1.0)
        ids, G = ids_all[rank], G_all[rank]
        if adam:
            st.optimizer.lr_t = _lr_t(1)
        h = st.lookup_rows_train(torch.from_numpy(ids), dedup=dedup)
        inv = h.inv.numpy()
        assert inv.shape == ids.shape
        ok = (ids >= 0) & (ids < np.array(VOCAB)[None, :])
        assert ((inv >= 0) == ok).all()
        rows = h.rows.numpy().copy()
        for f in range(F):
            assert np.array_equal(rows[inv[ok[:, f], f]], full[f][ids[ok[:, f], f]]), "slot %d" % f
        with torch.no_grad():
            st.lookup(torch.from_numpy(_uniform(ids.shape[0] + 2, 1200, rank)))          # (every rank: SPMD)
        used = np.unique(inv[ok])                                                     # (the slabs' unused tails are uninitialised memory)
        assert np.array_equal(h.rows.numpy()[used], rows[used]), "an inference lookup wrote the training lookup's rows"
        perm = np.random.default_rng(5 + rank).permutation(ids.size)
        idx = torch.from_numpy(inv.reshape(-1)[perm].copy())
        g = torch.from_numpy(G.reshape(-1, K)[perm].copy())
        h.backward_rows(idx, g)
        with pytest.raises(RuntimeError, match="has run already"):
            h.backward_rows(idx, g)
        ref.step(ids_all, G_all)
        ref.compare(st, be, slices, "lookup_rows_train %s dedup=%s" % (kw, dedup))
        assert st._updates == 1
    return "ok"


def sc_refusals(rank, world):
    from dir_amd.shard import ShardedTables, partition_layout
    from tests.shard_standin_adam import NumpyAdamBackend
    st, _, _, _ = _tables(rank, world, 31)
    st.attach_linear([torch.zeros(t.shape[0]) for t in st.local_tables])
    st.enable_linear_training(0.1)
    ids = torch.from_numpy(_uniform(4, 31, rank))
    with pytest.raises(NotImplementedError, match="with_linear"):
        st.lookup_train(ids, with_linear=True, dedup=True)
    parts, first, sl = partition_layout(VOCAB, K, world, rank, None)
    local2 = [torch.zeros((e - s, 2 * K)) for s, e in sl]
    st2 = ShardedTables(local2, VOCAB, backend=NumpyDinBackend(local2, VOCAB, parts, first, world, 2 * K), groups=2).enable_training(LR)
    with pytest.raises(NotImplementedError, match="groups"):
        st2.lookup_train(ids, dedup=True)
    local3 = [torch.zeros((e - s, K)) for s, e in sl]
    st3 = ShardedTables(local3, VOCAB, backend=NumpyAdamBackend(local3, VOCAB, parts, first, world, K)).enable_training(LR)
    with pytest.raises(NotImplementedError, match="rows_scatter_sum"):
        st3.lookup_train(ids, dedup=True)
    with pytest.raises(NotImplementedError, match="rows_scatter_sum"):
        st3.lookup_rows_train(ids)
    return "ok"


_FUNCS = dict(steps=sc_steps, hot=sc_hot, overflow=sc_overflow, rows=sc_rows)


def _scenarios(rank, world, names, adam):
    out = []
    for n in names:
        if n in _FUNCS:
            out.append((n, _FUNCS[n](rank, world, adam)))
        else:
            out.append((n, dict(forward=sc_forward_bitwise, zipf=sc_zipf, refusals=sc_refusals)[n](rank, world)))
    return out


def _run(world, names, adam=False):
    res = run_ranks(world, _scenarios, names, adam, timeout=600)
    for rank, got in sorted(res.items()):
        assert [n for n, _ in got] == list(names), "rank %d ran %s" % (rank, got)
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_dedup_training_adagrad_matches_float64(world):
    _run(world, ("forward", "steps", "zipf", "hot", "overflow"))


@pytest.mark.parametrize("world", [2, 3])
def test_dedup_training_adam_with_clip_matches_float64(world):
    _run(world, ("steps", "hot", "overflow"), adam=True)


@pytest.mark.parametrize("world", [2, 3])
def test_lookup_rows_train_and_backward_rows(world):
    _run(world, ("rows", "refusals"))
    _run(world, ("rows",), adam=True)


def test_scatter_sum_stand_in_against_float64():
    """The stand-in itself: runs of one bit for bit, long runs across tile borders within the bar, dropped entries, untouched rows zero."""
    from tests.shard_standin_din import scatter_sum
    rng = np.random.default_rng(1)
    idx = np.concatenate([np.full(700, 5), rng.integers(-2, 12, size=300), np.full(513, 9)]).astype(np.int64)
    rng.shuffle(idx)
    vals = rng.standard_normal((idx.size, 4)).astype(np.float32)
    out, longest = scatter_sum(idx, vals, 10)
    want = np.zeros((10, 4))
    ok = (idx >= 0) & (idx < 10)
    np.add.at(want, idx[ok], vals[ok].astype(np.float64))
    assert scaled(out, want) <= BAR and longest >= 700
    one, _ = scatter_sum(np.array([3, -1, 0, 99]), vals[:4], 6)
    assert np.array_equal(one[3], vals[0]) and np.array_equal(one[0], vals[2]) and not one[[1, 2, 4, 5]].any()
