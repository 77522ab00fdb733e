"""Multi-process CPU test of the row-sharded multi-hot bags (dir_amd.shard.ShardedTables.lookup_bags) over the gloo backend, world sizes
2, 3 and 8.

The exchange logic under test is what runs under RCCL on a GPU box: capacity agreement, slabs of CSR entries bucketed by owner, the
equal-split all_to_all of the slabs, the owner pooling its entries into one partial row per (bag, owner), the all_to_all of the partial
rows, the requester's combine, the overflow verdict read off the received headers and the repeat with grown capacities.  The three HIP
steps cannot run without a GPU, so NumPy stand-ins take their place through the `backend` injection point -- writing the same slab
format (include/dir_hip.h: dir_shard_bags_bucket) into the same buffers.  Reference: a float64 restatement of the bag semantics
(ops.embedding_bag / [TF-upstream] embedding_lookup_sparse with max_norm) over the FULL tables, the same on every rank."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CODES = {"sum": 0, "mean": 1, "sqrtn": 2}


def _store():
    import tempfile
    return os.path.join(tempfile.mkdtemp(prefix="dir_pg_"), "store")


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


def per_slot(x, F):
    return list(x) if isinstance(x, (list, tuple)) else [x] * F


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


# ---- NumPy stand-ins for the three HIP steps ---------------------------------------------------------------------------------------
def numpy_bags_backend(local, vocab, parts, first, P, K):
    """The three lookup_bags steps of shard.HipBackend in NumPy, on the slab format of include/dir_hip.h (fp32 arithmetic in the
    kernels' order: entries in entry order inside a partial, partials in ascending owner order)."""
    from oracle import np_ref as R
    F = len(vocab)

    def codes(combiner):
        return [_CODES[c] for c in per_slot(combiner, F)]

    class Backend:
        def new_bags_workspace(self, device):
            return torch.zeros(256, dtype=torch.int32)

        def bags_bucket(self, values, offsets, weights, B, sb, sf, combiner, flags, cap_e, cap_b, slabs, pos, mask, denom, workspace):
            vals, offs = values.numpy(), offsets.numpy()
            wts = None if weights is None else weights.numpy()
            prune = wts is not None and bool(flags & 1)
            cb_ = codes(combiner)
            sl = slabs.numpy().reshape(P, cap_e + 1, 2)
            ps, mk, dn = pos.numpy(), mask.numpy(), denom.numpy()
            ne, nb = np.zeros(P, np.int64), np.zeros(P, np.int64)
            for b in range(B):
                for f in range(F):
                    g = b * F + f
                    s0, s1 = offs[b * sb + f * sf], offs[b * sb + f * sf + 1]
                    runs = {}
                    wsum, w2sum, n = np.float32(0), np.float32(0), 0
                    for e in range(s0, s1):
                        i = vals[e]
                        w = np.float32(1) if wts is None else np.float32(wts[e])
                        if i < 0 or i >= vocab[f] or (prune and not w > 0):
                            continue
                        o, l = R.shard_div_owner([i], vocab[f], parts[f])
                        o = (int(o[0]) + first[f]) % P
                        runs.setdefault(o, []).append((int(l[0]) * F + f, w))
                        wsum = np.float32(wsum + w)
                        w2sum = np.float32(w2sum + np.float32(w * w))
                        n += 1
                    if cb_[f] == 1:
                        dn[g] = wsum if wts is not None else np.float32(n)
                    elif cb_[f] == 2:
                        dn[g] = np.sqrt(w2sum) if wts is not None else np.sqrt(np.float32(n))
                    else:
                        dn[g] = 1.0
                    m = 0
                    for o in sorted(runs):
                        m |= 1 << o
                        q = nb[o]
                        nb[o] += 1
                        ps[g * P + o] = o * cap_b + q if q < cap_b else -1
                        for packed, w in runs[o]:
                            if ne[o] < cap_e:
                                ret = q if q < cap_b else -1
                                sl[o, 1 + ne[o], 0] = packed
                                sl[o, 1 + ne[o], 1] = int(np.float32(w).view(np.uint32)) | (int(np.uint32(ret & 0xffffffff)) << 32)
                            ne[o] += 1
                    mk[g] = np.int64(np.uint64(m).astype(np.int64)) if m < (1 << 63) else np.int64(m - (1 << 64))
            de, db = int(ne.max()), int(nb.max())
            for o in range(P):
                sl[o, 0, 0] = min(ne[o], cap_e) | (min(nb[o], cap_b) << 32)
                sl[o, 0, 1] = de | (db << 32)

        def bags_pool(self, recv, cap_e, cap_b, max_norm, rows, stat=None):
            sl = recv.numpy().reshape(P, cap_e + 1, 2)
            mn = per_slot(max_norm, F)
            out = rows.numpy()
            for s in range(P):
                ne = int(sl[s, 0, 0] & 0xffffffff)
                prev, acc = None, None
                for j in range(ne + 1):
                    ret = int(np.int64(sl[s, 1 + j, 1]) >> 32) if j < ne else None
                    if ret != prev and prev is not None and prev >= 0:
                        out[s * cap_b + prev] = acc
                    if j == ne:
                        break
                    if ret != prev:
                        acc = np.zeros(K, np.float32)
                    prev = ret
                    packed = int(sl[s, 1 + j, 0])
                    w = np.array([sl[s, 1 + j, 1] & 0xffffffff], np.uint64).astype(np.uint32).view(np.float32)[0]
                    f, l = packed % F, packed // F
                    r = local[f][l].numpy().astype(np.float32)
                    if mn[f]:
                        l2 = np.float32(0)
                        for x in r:
                            l2 = np.float32(l2 + np.float32(x * x))
                        nrm = np.sqrt(l2) if l2 > 0 else l2
                        r = (r * np.float32(mn[f])) / np.float32(max(nrm, np.float32(mn[f])))
                    acc = (acc + r * w).astype(np.float32)
            if stat is not None:
                de = max(int(sl[s, 0, 1] & 0xffffffff) for s in range(P))
                db = max(int(sl[s, 0, 1] >> 32) for s in range(P))
                stat.copy_(torch.tensor([int(de > cap_e or db > cap_b), de, db]))

        def bags_combine(self, back, cap_b, pos, mask, denom, B, combiner, out, fm=None):
            cb_ = codes(combiner)
            bk, ps, mk, dn = back.numpy(), pos.numpy(), mask.numpy(), denom.numpy()
            o_ = out.numpy()
            for b in range(B):
                for f in range(F):
                    g = b * F + f
                    m = int(mk[g]) & ((1 << 64) - 1)
                    acc = np.zeros(K, np.float32)
                    for o in range(P):
                        if (m >> o) & 1 and ps[g * P + o] >= 0:
                            acc = (acc + bk[ps[g * P + o]]).astype(np.float32)
                    if m and cb_[f] != 0:
                        acc = (acc / dn[g]).astype(np.float32)
                    o_[b, f * K:(f + 1) * K] = acc
            if fm is not None:
                fm.copy_(torch.from_numpy(fm_ref(o_, F, K).astype(np.float32)[:, None]))

    return Backend()


# ---- the ranks --------------------------------------------------------------------------------------------------------------------
CASES = [   # (weights, combiner, max_norm, field_major, prune)
    (None, "mean", None, False, False),
    ("pos", "sqrtn", 0.9, True, False),
    ("signed", ["sum", "mean", "sqrtn"], [None, 1.1, 0.6], False, True),
    ("pos", ["mean", "sum", "mean"], None, True, False),
    (None, ["sqrtn", "sqrtn", "sum"], [0.7, None, None], True, False),
]


def _worker(rank, world, store, spec, q):
    try:
        import sys
        sys.path.insert(0, ROOT)
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        import datetime
        dist.init_process_group("gloo", init_method="file://" + store, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
        try:
            q.put((rank, _scenarios(rank, world, spec)))
        finally:
            dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))


def _scenarios(rank, world, spec):
    from dir_amd.shard import ShardedTables, local_slice, place_slices
    vocab, K = spec["vocab"], spec["K"]
    F = len(vocab)
    parts = spec.get("partitions") or [world] * F
    first = place_slices(parts, world) if spec.get("partitions") else [0] * F
    rng = np.random.default_rng(7)                                  # the same full tables on every rank
    full = [(rng.standard_normal((v, K)) * 0.5).astype(np.float32) for v in vocab]
    local = [torch.from_numpy(full[f][slice(*local_slice(v, parts[f], first[f], world, rank))].copy()) for f, v in enumerate(vocab)]
    be = numpy_bags_backend(local, vocab, parts, first, world, K)
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
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = _store()
    procs = [ctx.Process(target=_worker, args=(r, world, store, spec, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    out = {}
    for rank, got in res:
        assert not isinstance(got, str), "rank %d raised:\n%s" % (rank, got)
        bad = [(n, d) for n, ok, d in got[0] if not ok]
        assert not bad, "rank %d: %s" % (rank, bad)
        out[rank] = got
    return out


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
    import sys
    sys.path.insert(0, ROOT)
    from dir_amd.shard import ShardedTables
    local = [torch.zeros((10, 4)), torch.zeros((7, 4))]
    st = ShardedTables(local, [10, 7], backend=numpy_bags_backend(local, [10, 7], [1, 1], [0, 0], 1, 4))
    assert st._bag_caps(50, 1000) == st._bag_caps(50, 1010) == (1024, 112)
    for n in (0, 1, 17, 1000, 5000, 123457, 4980736):
        ce, _ = st._bag_caps(50, n)
        assert max(n, 16) <= ce <= max(16, n * 1.125 + 16), (n, ce)
