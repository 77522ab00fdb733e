"""Multi-process CPU test of the row-sharded multi-hot bags (dir_amd.shard.ShardedTables.lookup_bags) over the gloo backend, world sizes
2, 3 and 8.

The exchange logic under test is what runs under RCCL on a GPU box: capacity agreement, slabs of CSR entries bucketed by owner, the
equal-split all_to_all of the slabs, the owner pooling its entries into one partial row per (bag, owner), the all_to_all of the partial
rows, the requester's combine, the overflow verdict read off the received headers and the repeat with grown capacities.  The three HIP
steps cannot run without a GPU, so NumPy stand-ins take their place through the `backend` injection point -- writing the same slab
format (include/dir_hip.h: dir_shard_bags_bucket) into the same buffers.  Reference: a float64 restatement of the bag semantics
(ops.embedding_bag / [TF-upstream] embedding_lookup_sparse with max_norm) over the FULL tables, the same on every rank."""
import numpy as np
import torch

from tests.shard_standin import NumpyBackend, per_slot, run_checked


# ---- bags, layouts and the float64 reference (also used by tests/test_gpu_shard_bags.py) --------------------------------------------
def draw_bags(rng, B, vocab, max_len, weights=None):
    """Per logical bag (b, f): (ids, weights) with pruned (-1) and out-of-vocabulary ids mixed in.  max_len[f]: bag lengths 0..max_len[f]
    (1: exactly one entry).  weights: None, "pos" (0.1..2) or "signed" (-1..2, for PRUNE_NONPOSITIVE_WEIGHTS)."""
    bags = []
    for b in range(B):
        row = []
        for f, v in enumerate(vocab):
            L = 1 if max_len[f] == 1 else int(rng.integers(0, max_len[f] + 1))
            ids = rng.integers(0, v, size=L).astype(np.int64)
            if L:
                odd = rng.random(L)
                ids[odd < 0.06] = -1                       # pruned
                ids[(odd >= 0.06) & (odd < 0.1)] = v + 2   # out of vocabulary: nobody owns it
            if weights is None:
                w = None
            elif weights == "pos":
                w = rng.uniform(0.1, 2.0, size=L).astype(np.float32)
            else:
                w = rng.uniform(-1.0, 2.0, size=L).astype(np.float32)
            row.append((ids, w))
        bags.append(row)
    return bags


def to_csr(bags, F, field_major):
    """-> (values [nnz] int64, offsets [B*F+1] int64, weights [nnz] fp32 or None) in sample-major or field-major bag order."""
    B = len(bags)
    order = [(b, f) for f in range(F) for b in range(B)] if field_major else [(b, f) for b in range(B) for f in range(F)]
    vals, wts, offs = [], [], [0]
    has_w = B > 0 and any(bags[b][f][1] is not None for b in range(B) for f in range(F))
    for b, f in order:
        ids, w = bags[b][f]
        vals.append(ids)
        if has_w:
            wts.append(w if w is not None else np.ones(len(ids), np.float32))
        offs.append(offs[-1] + len(ids))
    v = np.concatenate(vals).astype(np.int64) if vals else np.zeros(0, np.int64)
    w = (np.concatenate(wts).astype(np.float32) if wts else np.zeros(0, np.float32)) if has_w else None
    return v, np.asarray(offs, np.int64), w


def bags_ref(full, bags, combiner, max_norm, prune):
    """float64 restatement: -> (emb [B, F*K], scale [B, F*K]) where scale bounds the fp32 rounding (the same combine over |w * row|)."""
    F, K = len(full), full[0].shape[1]
    comb, mn = per_slot(combiner, F), per_slot(max_norm, F)
    B = len(bags)
    out = np.zeros((B, F * K))
    scale = np.zeros((B, F * K))
    for b in range(B):
        for f in range(F):
            ids, w = bags[b][f]
            acc, aab, ws, w2, n = np.zeros(K), np.zeros(K), 0.0, 0.0, 0
            for j, i in enumerate(ids):
                wj = 1.0 if w is None else float(w[j])
                if i < 0 or i >= full[f].shape[0] or (prune and w is not None and not wj > 0):
                    continue
                r = full[f][i].astype(np.float64)
                if mn[f]:
                    nrm = np.sqrt((r * r).sum())
                    r = r * mn[f] / max(nrm, mn[f])
                acc += wj * r
                aab += abs(wj * r)
                ws += wj
                w2 += wj * wj
                n += 1
            if n:
                if comb[f] == "mean":
                    d = ws if w is not None else n
                elif comb[f] == "sqrtn":
                    d = np.sqrt(w2) if w is not None else np.sqrt(n)
                else:
                    d = 1.0
                acc, aab = acc / d, aab / abs(d)
            out[b, f * K:(f + 1) * K] = acc
            scale[b, f * K:(f + 1) * K] = aab
    return out, scale


def fm_ref(emb, F, K):
    e = emb.reshape(-1, F, K).astype(np.float64)
    return 0.5 * ((e.sum(1) ** 2) - (e ** 2).sum(1)).sum(1)


# ---- the ranks --------------------------------------------------------------------------------------------------------------------
CASES = [   # (weights, combiner, max_norm, field_major, prune)
    (None, "mean", None, False, False),
    ("pos", "sqrtn", 0.9, True, False),
    ("signed", ["sum", "mean", "sqrtn"], [None, 1.1, 0.6], False, True),
    ("pos", ["mean", "sum", "mean"], None, True, False),
    (None, ["sqrtn", "sqrtn", "sum"], [0.7, None, None], True, False),
]


def _scenarios(rank, world, spec):
    from dir_amd.shard import ShardedTables, partition_layout
    vocab, K = spec["vocab"], spec["K"]
    F = len(vocab)
    parts, first, slices = partition_layout(vocab, K, world, rank, spec.get("partitions"))
    rng = np.random.default_rng(7)                                  # the same full tables on every rank
    full = [(rng.standard_normal((v, K)) * 0.5).astype(np.float32) for v in vocab]
    local = [torch.from_numpy(full[f][s:e].copy()) for f, (s, e) in enumerate(slices)]
    be = NumpyBackend(local, vocab, parts, first, world, K)
    kw = {k: spec[k] for k in ("partitions", "slack", "check") if k in spec}
    st = ShardedTables(local, vocab, backend=be, **kw)
    rng_b = np.random.default_rng(1000 + rank)                      # every rank draws its own bags
    res = []
    if spec.get("lazy_overflow"):
        return _lazy_overflow(st, full, rng_b, spec), 0, st.stats.get("bag_cap")
    for c, (wmode, comb, mn, fmaj, prune) in enumerate(spec.get("cases", CASES)):
        B = spec["batch"][rank % len(spec["batch"])] if c % 2 == 0 else spec["batch"][(rank + 1) % len(spec["batch"])]
        bags = draw_bags(rng_b, B, vocab, spec["max_len"], wmode)
        v, o, w = to_csr(bags, F, fmaj)
        emb, fm = st.lookup_bags(torch.from_numpy(v), torch.from_numpy(o), None if w is None else torch.from_numpy(w), combiner=comb,
                                 max_norm=mn, field_major=fmaj, flags=1 if prune else 0, want_fm=True)
        ref, scale = bags_ref(full, bags, comb, mn, prune)
        err = float((np.abs(emb.numpy() - ref) / (1e-6 + 1e-5 * (scale + 1))).max()) if B else 0.0
        ferr = float(np.abs(fm.numpy()[:, 0] - fm_ref(ref, F, K)).max() / (1 + np.abs(fm_ref(ref, F, K)).max())) if B else 0.0
        res.append(("case%d" % c, emb.shape == (B, F * K) and fm.shape == (B, 1) and err <= 1.0 and ferr <= 1e-4,
                    "B=%d err=%.3g fm=%.3g" % (B, err, ferr)))
    res.append(("stats", True, "caps=%s fallbacks=%d" % (st.stats.get("bag_cap"), st.stats.get("bag_fallbacks", 0))))
    return res, st.stats.get("bag_fallbacks", 0), st.stats.get("bag_cap")


def _lazy_overflow(st, full, rng_b, spec):
    """check="lazy": no lookup waits for its own verdict.  The first lookup's slabs are too small; its verdict is read when the second
    lookup_bags has been enqueued, which raises on every rank with the capacities grown; the lookups after that fit and are right."""
    vocab, F, K = spec["vocab"], len(spec["vocab"]), spec["K"]
    res = []

    def one():
        bags = draw_bags(rng_b, spec["batch"][0], vocab, spec["max_len"], None)
        v, o, _ = to_csr(bags, F, False)
        emb, _ = st.lookup_bags(torch.from_numpy(v), torch.from_numpy(o))
        ref, scale = bags_ref(full, bags, "mean", None, False)
        return float((np.abs(emb.numpy() - ref) / (1e-6 + 1e-5 * (scale + 1))).max())
    one()                                                            # overflows: incomplete, not yet known
    caps0 = st.stats["bag_cap"]
    raised = []
    for _ in range(3):                # a lookup enqueued before the verdict that grew the capacities ran on the old ones: it raises too
        try:
            one()
            raised.append(False)
        except RuntimeError:
            raised.append(True)
    fb = st.stats.get("bag_fallbacks", 0)
    res.append(("raised_at_next", raised[0] and not raised[-1] and fb == sum(raised), "raised %s caps %s -> %s" % (raised, caps0, st._bag_cap)))
    err = max(one() for _ in range(3))
    st.check_overflow()
    res.append(("then_fits", err <= 1.0 and st.stats.get("bag_fallbacks", 0) == fb and st._bag_cap[0] > caps0[0], "err=%.3g" % err))
    return res


def _run(world, spec):
    return run_checked(world, _scenarios, spec)


def test_bags_world2_matrix():
    """Bag lengths 0..60 beside one-hot and short slots; pruned and out-of-vocabulary ids; per-slot combiners and max_norm; weights and
    no weights and PRUNE_NONPOSITIVE_WEIGHTS; both layouts; one rank with an EMPTY local batch in some lookups."""
    _run(2, dict(vocab=[500, 1000, 7], K=8, max_len=[1, 60, 4], batch=[23, 0]))


def test_bags_world3_partitions_and_tiny_tables():
    """partitions= lists (a table cut fewer ways than there are ranks, dealt round-robin) and a table with fewer rows than ranks."""
    _run(3, dict(vocab=[300, 2, 41], K=4, max_len=[12, 3, 1], batch=[9, 17, 4], partitions=[2, 1, 3]))


def test_bags_world8():
    """World size 8 (the last review's missing coverage): uneven and empty local batches, tables with fewer rows than ranks."""
    _run(8, dict(vocab=[5, 900, 60], K=4, max_len=[2, 30, 1], batch=[6, 0, 11, 3, 1, 9, 0, 5],
                 cases=CASES[:3]))


def test_bags_overflow_grows_capacities():
    """Tiny first capacities (slack): the verdict read off the received headers says overflow on every rank, the lookup is repeated with
    the capacities grown to the demands the headers carry, and the result is still right; later lookups fit."""
    res = _run(2, dict(vocab=[400, 50], K=4, max_len=[40, 3], batch=[60, 45], slack=0.02, cases=CASES[:4]))
    for rank, (_, fallbacks, caps) in res.items():
        assert 1 <= fallbacks < 4, (rank, fallbacks)
        assert caps[0] > 16 and caps[1] > 16, caps
    assert len({tuple(c) for _, _, c in res.values()}) == 1                # the same capacities on every rank


def test_bags_lazy_verdict_raises_at_the_next_lookup():
    """check="lazy": the verdict of a lookup is read once the next lookup_bags has been enqueued (no host wait on the lookup's own work);
    an overflow raises there on every rank, the capacities have grown, and the following lookups are right."""
    _run(2, dict(vocab=[400, 50], K=4, max_len=[40, 3], batch=[60], slack=0.02, check="lazy", lazy_overflow=True))


def test_bags_world1_capacity_buckets():
    """One rank: the entry capacity is rounded up to an eighth of its power of two, so batches of similar nnz share one plan."""
    from dir_amd.shard import ShardedTables
    local = [torch.zeros((10, 4)), torch.zeros((7, 4))]
    st = ShardedTables(local, [10, 7], backend=NumpyBackend(local, [10, 7], [1, 1], [0, 0], 1, 4))
    assert st._bag_caps(50, 1000) == st._bag_caps(50, 1010) == (1024, 112)
    for n in (0, 1, 17, 1000, 5000, 123457, 4980736):
        ce, _ = st._bag_caps(50, n)
        assert max(n, 16) <= ce <= max(16, n * 1.125 + 16), (n, ce)
