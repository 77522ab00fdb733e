"""Multi-process CPU test of training through the row-sharded multi-hot bags (dir_amd.shard.ShardedTables.lookup_bags_train) over the
gloo backend, world sizes 1, 2, 3 and 8.

What runs here is what runs under RCCL on a GPU box: the training plans, the forward's own overflow verdict and its repeat, the gradient
scatter onto the partial rows, the partial-row exchange in reverse, the owner's update over the bag records it kept, the bookkeeping
shared with the one-hot lookup_train.  The HIP steps cannot run without a GPU, so NumPy stand-ins take their place through the `backend`
injection point, writing and reading the same buffers (include/dir_hip.h: dir_shard_bags_grad_f32, dir_sparse_adagrad_sorted_bags_f32).
Reference: float64 torch autograd of the bag forward over the FULL tables on the GLOBAL batch, then [TF-upstream] Adagrad on every table
(duplicates summed before the accumulator moves) -- the same on every rank."""
import numpy as np
import torch

from tests.shard_standin import NumpyBackend, per_slot, run_checked
from tests.test_shard_bags_gloo import CASES, draw_bags, to_csr

LR, ACC0 = 0.3, 0.1


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------
def bags_forward64(T, bags, combiner, max_norm, prune):
    """The bag forward in float64 torch (differentiable in the tables T): -> emb [B, F*K]."""
    F, K = len(T), T[0].shape[1]
    comb, mn = per_slot(combiner, F), per_slot(max_norm, F)
    B = len(bags)
    outs = []
    for f in range(F):
        bag_i, ids, ws = [], [], []
        for b in range(B):
            i_, w_ = bags[b][f]
            for j, i in enumerate(i_):
                wj = 1.0 if w_ is None else float(w_[j])
                if i < 0 or i >= T[f].shape[0] or (prune and w_ is not None and not wj > 0):
                    continue
                bag_i.append(b)
                ids.append(int(i))
                ws.append(wj)
        bag_i = torch.tensor(bag_i, dtype=torch.int64)
        wt = torch.tensor(ws, dtype=torch.float64)
        has_w = any(bags[b][f][1] is not None for b in range(B))
        r = T[f][torch.tensor(ids, dtype=torch.int64)] if ids else torch.zeros((0, K), dtype=torch.float64)
        if mn[f]:
            n = r.norm(dim=1, keepdim=True)
            r = r * mn[f] / torch.clamp_min(n, mn[f])
        out = torch.zeros((B, K), dtype=torch.float64).index_add(0, bag_i, wt[:, None] * r)
        cnt = torch.zeros(B, dtype=torch.float64).index_add(0, bag_i, torch.ones_like(wt))
        if comb[f] == "mean":
            den = torch.zeros(B, dtype=torch.float64).index_add(0, bag_i, wt) if has_w else cnt
        elif comb[f] == "sqrtn":
            den = (torch.zeros(B, dtype=torch.float64).index_add(0, bag_i, wt * wt) if has_w else cnt).sqrt()
        else:
            den = torch.ones(B, dtype=torch.float64)
        den = torch.where(cnt > 0, den, torch.ones_like(den))
        outs.append(out / den[:, None])
    return torch.cat(outs, dim=1) if B else torch.zeros((0, F * K), dtype=torch.float64)


def adagrad64(full, acc, grads, lr):
    """[TF-upstream] Adagrad on every table, in place (untouched rows have a zero gradient and do not move)."""
    for f, g in enumerate(grads):
        g = np.zeros_like(full[f]) if g is None else g
        acc[f] += g * g
        full[f] -= lr * g / np.sqrt(acc[f])


def ref_step(full, acc, bags, G, combiner, max_norm, prune, lr):
    """One step of the reference on the FULL tables (float64 numpy arrays, in place): autograd of sum(bag forward * G) over the global
    batch, then Adagrad."""
    T = [torch.from_numpy(t).requires_grad_(True) for t in full]
    emb = bags_forward64(T, bags, combiner, max_norm, prune)
    if len(bags):
        (emb * torch.from_numpy(np.asarray(G, np.float64))).sum().backward()
    adagrad64(full, acc, [None if t.grad is None else t.grad.numpy() for t in T], lr)


# ---- the ranks --------------------------------------------------------------------------------------------------------------------
def _close(got, ref):
    return float((np.abs(got.astype(np.float64) - ref) / (1.0 + np.abs(ref))).max()) if got.size else 0.0


def _scenario(rank, world, spec):
    from dir_amd.shard import ShardedTables, partition_layout
    vocab, K = spec["vocab"], spec["K"]
    F = len(vocab)
    parts, first, slices = partition_layout(vocab, K, world, rank, spec.get("partitions"))
    rng = np.random.default_rng(7)                                  # the same full tables on every rank
    full = [(rng.standard_normal((v, K)) * 0.5).astype(np.float32) for v in vocab]
    mine = [slice(s, e) for s, e in slices]
    local = [torch.from_numpy(full[f][mine[f]].copy()) for f in range(F)]
    be = NumpyBackend(local, vocab, parts, first, world, K)
    kw = {k: spec[k] for k in ("partitions", "slack", "check") if k in spec}
    st = ShardedTables(local, vocab, backend=be, **kw).enable_training(LR, ACC0)
    ref = [t.astype(np.float64) for t in full]
    acc = [np.full(t.shape, ACC0) for t in full]
    batch = spec["batch"]
    res = []
    for step, kind in enumerate(spec["steps"]):
        rng_s = np.random.default_rng(1000 + step)                  # every rank draws the GLOBAL batch, then takes its own part
        Bs = [batch[(r + step) % len(batch)] for r in range(world)]
        if kind == "onehot":
            ids_all = [np.stack([rng_s.integers(-1, v, size=Bs[r]) for v in vocab], axis=1).astype(np.int64).reshape(Bs[r], F)
                       for r in range(world)]
            bags_all = [[[(np.array([i]), None) for i in row] for row in ids] for ids in ids_all]
            comb, mn, fmaj, prune, wmode = "sum", None, False, False, None
        else:
            wmode, comb, mn, fmaj, prune = spec.get("cases", CASES)[kind]
            bags_all = [draw_bags(rng_s, Bs[r], vocab, spec["max_len"], wmode) for r in range(world)]
            hot = spec.get("hot")
            if hot is not None:                                     # one row repeated inside bags, across bags and across ranks
                f_h, id_h = hot
                for bl in bags_all:
                    for row in bl:
                        ids, w = row[f_h]
                        if len(ids) >= 2:
                            ids[:2] = id_h
        G_all = [rng_s.standard_normal((Bs[r], F * K)).astype(np.float32) for r in range(world)]
        B = Bs[rank]
        G = torch.from_numpy(G_all[rank])
        if kind == "onehot":
            emb = st.lookup_train(torch.from_numpy(ids_all[rank]))
            emb.backward(G)
        else:
            v, o, w = to_csr(bags_all[rank], F, fmaj)
            args = (torch.from_numpy(v), torch.from_numpy(o), None if w is None else torch.from_numpy(w))
            kw_b = dict(combiner=comb, max_norm=mn, field_major=fmaj, flags=1 if prune else 0)
            lazy = spec.get("lazy_pending") and step == 0
            inf, _ = st.lookup_bags(*args, **kw_b)                 # (lazy: overflows; its verdict is read at the NEXT lookup_bags)
            emb = st.lookup_bags_train(*args, **kw_b)
            same = emb.shape == (B, F * K) and emb.requires_grad and (lazy or bool(torch.equal(emb.detach(), inf)))
            res.append(("forward%d" % step, same, "B=%d" % B))
            if not lazy:
                # an inference lookup of OTHER bags between the forward and its backward: the update below is unchanged
                other = draw_bags(np.random.default_rng(5000 + 10 * step + rank), B, vocab, spec["max_len"], wmode)
                v2, o2, w2 = to_csr(other, F, fmaj)
                st.lookup_bags(torch.from_numpy(v2), torch.from_numpy(o2), None if w2 is None else torch.from_numpy(w2), **kw_b)
            emb.backward(G)
            if lazy:
                try:                                                # the inference verdict is still pending (not read by training)
                    st.lookup_bags(*args, **kw_b)
                    raised = False
                except RuntimeError:
                    raised = True
                res.append(("lazy_verdict_kept", raised, "fallbacks=%s" % st.stats.get("bag_fallbacks")))
        ref_step(ref, acc, [b for bl in bags_all for b in bl], np.concatenate(G_all, axis=0), comb, mn, prune, LR)
        et = max(_close(local[f].numpy(), ref[f][mine[f]]) for f in range(F))
        ea = max(_close(st.optimizer["acc"][f], acc[f][mine[f]]) for f in range(F))
        res.append(("step%d" % step, et <= 1e-5 and ea <= 1e-5, "%s B=%d tables %.3g accums %.3g" % (kind, B, et, ea)))
    res.append(("updates", st._updates == len(spec["steps"]), "updates=%d" % st._updates))
    return res, st.stats.get("bag_fallbacks", 0), st._bag_cap


def _run(world, spec):
    return run_checked(world, _scenario, spec)


def test_bags_train_world1():
    """One rank (no exchange, nothing can overflow): every combiner, weights, PRUNE_NONPOSITIVE_WEIGHTS, max_norm, both layouts."""
    _run(1, dict(vocab=[50, 300, 7], K=8, max_len=[1, 30, 4], batch=[17], steps=[0, 1, 2, 3, 4]))


def test_bags_train_world2_duplicates_and_empty_batch():
    """A hot row repeated inside bags, across bags and across ranks beside a 7-row table; one rank with an EMPTY local batch."""
    _run(2, dict(vocab=[500, 1000, 7], K=8, max_len=[1, 40, 6], batch=[23, 0], hot=(1, 3), steps=[0, 2, 1]))


def test_bags_train_world3_partitions_and_tiny_tables():
    """partitions= lists (a table cut fewer ways than there are ranks, dealt round-robin) and a table with fewer rows than ranks."""
    _run(3, dict(vocab=[300, 2, 41], K=4, max_len=[12, 3, 1], batch=[9, 17, 4], partitions=[2, 1, 3], steps=[2, 4, 1]))


def test_bags_train_world3_reference_partitions():
    """partitions="reference": the reference partitioner's slice counts (one slice per small table), dealt round-robin."""
    _run(3, dict(vocab=[60, 200, 5], K=4, max_len=[6, 20, 2], batch=[8, 5, 11], partitions="reference", steps=[0, 3, 2]))


def test_bags_train_world8():
    """World size 8: uneven and empty local batches, tables with fewer rows than ranks."""
    _run(8, dict(vocab=[5, 900, 60], K=4, max_len=[2, 30, 1], batch=[6, 0, 11, 3, 1, 9, 0, 5], steps=[0, 2, 1]))


def test_bags_train_overflow_repeats_with_grown_capacities():
    """Tiny first capacities: the training forward reads its own verdict (the same on every rank), repeats with the capacities grown to
    the demands the headers carry, and the step is still right."""
    res = _run(2, dict(vocab=[400, 50, 9], K=4, max_len=[40, 3, 5], batch=[60, 45], slack=0.02, steps=[0, 2, 3]))
    for rank, (_, fallbacks, caps) in res.items():
        assert fallbacks >= 1, (rank, fallbacks)
    assert len({tuple(c) for _, _, c in res.values()}) == 1                # the same capacities on every rank


def test_bags_train_keeps_lazy_verdicts_pending():
    """check="lazy": an overflowing inference lookup_bags leaves its verdict pending; the training step in between reads only its own
    (and repeats), so the NEXT lookup_bags still raises for the inference lookup on every rank."""
    _run(2, dict(vocab=[400, 50, 9], K=4, max_len=[40, 3, 5], batch=[60], slack=0.02, check="lazy", lazy_pending=True, steps=[0]))


def test_bags_and_onehot_steps_share_accumulators():
    """A one-hot lookup_train step between bag steps: one optimiser, one set of accumulators (sum-combined single-entry bags in the
    reference)."""
    _run(2, dict(vocab=[120, 300, 9], K=4, max_len=[5, 20, 3], batch=[13, 7], steps=[0, "onehot", 2, "onehot"]))
