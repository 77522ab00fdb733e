"""shard.HipBackend at 1, 2, 3, 8, 33 and 64 owners, in ONE process on one GPU (tests/shard_loopback.py), against the NumPy stand-ins of
the gloo tests step by step and against the full-table references end to end.

The kernels behind every dir_shard_* entry take 1 <= P <= 64 owners; the multi-process GPU tests reach P = 1 and P = 2.  Here every
rank's backend runs the product's call sequence over guarded buffers, the exchanges are slab transposes, and after each step the
kernel's output is compared with what the stand-in makes of the SAME input (where a slab's slot order depends on atomic order the
kernel's slabs feed the next step of both sides).  What is covered: per-owner LDS counters and `owner < P` lanes, the 64-bit owner mask
(owners 32..62 and 63, the sign bit of the int64 the mask travels in), 'div' routing with V % P != 0, empty shards and first != 0
wrap-around, the 64-bit routing branch (V >= 2^31 - 1), the launch switches (n > 256 * 1024, B * F > 2^20, ids >= 2^32 - 1), and the far
end of every [P * cap] buffer (guard words behind each: an index error is a failed assertion, not a fault).

Figures measured on an MI355X (worst |got - ref| / scale of the bag lookup against its derived bound) are in
test_bags_lookup_against_standin_and_float64's docstring."""
import numpy as np
import pytest
import torch

from tests.shard_loopback import JUNK32, Guards, Loopback, hip_factory, standin_factory
from tests.shard_standin import NumpyBackend
from tests.shard_standin_bags_linear import lin_entries, lin_forward64, lin_ftrl64
from tests.test_gpu_shard_bags import _one_owner_bags
from tests.test_shard_bags_gloo import CASES, bags_ref, draw_bags, to_csr
from tests.test_shard_bags_train_gloo import _close, ref_step
from tests.test_shard_linear_gloo import Reference
from tests.test_shard_loopback import ACC0, BAG_PARTS, FTRL, LR, ONEHOT_PARTS, ONEHOT_VOCAB, OWNERS, _layouts, draw_ids, draw_tables, onehot_rows

pytestmark = pytest.mark.gpu

PK = [(P, 16) for P in OWNERS] + [(8, 6), (8, 64)]       # K = 6: idle lanes and the scalar row path; K = 64: four chunks per row
VOCAB = list(ONEHOT_VOCAB[:3]) + [4096]                  # [300, 2, 641, 4096]: the 2-row table leaves most ranks an empty shard at P >= 3
PARTS = ONEHOT_PARTS                                     # {3: [2, 2, 3, 1], 8: [3, 1, 8, 2]}: slice owners wrap around past P - 1
BAG_VOCAB, BAG_MAXLEN = [300, 2, 4096], [24, 3, 1]
CAP = 176                                                # >= 40 samples x 4 slots: ample whatever the owners
CAP_E, CAP_B = 1152, 128                                 # >= 40 x 28 entries, >= 40 x 3 bags
DEV = "cuda:0"


def sizes(P):
    """Per-rank batches of 0..40 samples (0..12 from 33 ranks on: the stand-ins are Python loops); the last rank has none (P >= 2)."""
    Bs = [(7 + 13 * r) % 41 if P <= 8 else (7 + 5 * r) % 13 for r in range(P)]
    if P >= 2:
        Bs[-1] = 0
    return Bs


def _np(t):
    return t.detach().cpu().numpy()


def _cpu(t):
    return t.detach().cpu().clone()


def _pair(full, lin, P, partitions):
    """(HipBackend ranks on the GPU, stand-in ranks on the CPU) over the same full tables."""
    tf, tl = [torch.from_numpy(t) for t in full], [torch.from_numpy(w) for w in lin]
    hip = Loopback(tf, P, hip_factory, device=DEV, partitions=partitions, lin_full=tl, acc0=ACC0)
    std = Loopback(tf, P, standin_factory, partitions=partitions, lin_full=tl, acc0=ACC0)
    return hip, std


def _router(vocab, P, partitions=None):
    """A stand-in without tables: its route() is the 'div' rule with the layout's parts / first."""
    from dir_amd.shard import partition_layout
    parts, first, _ = partition_layout(vocab, 1, P, 0, partitions)
    return NumpyBackend(None, list(vocab), parts, first, P, 1)


def _ulps(a, b):
    """Distance in units of the last place between two fp32 arrays of one sign pattern (0 where bitwise equal)."""
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ---- b / c: what a bucketing pass must leave, whatever the atomic order -------------------------------------------------------------
def check_bucket_plain(router, flat, F, P, cap, send, inv, counts, flags, cstat):
    """The invariants of dir_shard_bucket_cap over flat ids [n] (slot = i % F): -> (counts, kept per owner)."""
    own, loc = router.route(flat)
    live = own >= 0
    want = np.bincount(own[live], minlength=P).astype(np.int64)
    over, demand = int((want > cap).any()), int(want.max()) if want.size else 0
    assert np.array_equal(counts, want), (counts, want)
    assert int(flags) == over and list(cstat) == [over, demand]
    slabs = send.reshape(P, cap + 1)
    assert np.array_equal(slabs[:, 0], np.minimum(want, cap) | (np.int64(demand) << 32))
    assert (inv[~live] == -1).all()
    kept = live & (inv >= 0)
    assert (inv[live & ~kept] == -1).all()
    o_of, p_of = inv[kept] // cap, inv[kept] % cap
    assert np.array_equal(o_of, own[kept])
    assert (p_of < np.minimum(want, cap)[o_of]).all()
    assert np.unique(inv[kept]).size == int(kept.sum())
    assert np.array_equal(np.bincount(o_of, minlength=P), np.minimum(want, cap))       # exactly min(count, cap) slots filled per owner
    idx = np.nonzero(kept)[0]
    assert np.array_equal(slabs[o_of, 1 + p_of], loc[kept] * F + idx % F)
    return want


def check_bucket_dedup(router, ids2d, P, cap, send, inv2d, counts, flags, cstat, tile):
    """The invariants of dir_shard_bucket_cap_dedup over ids [B, F]; inv2d [B, F] as HipBackend.inv2d gives it.  tile: samples of one
    slot per workgroup (duplicates inside it share one position)."""
    B, F = ids2d.shape
    own, loc = (a.reshape(B, F) for a in router.route(ids2d.reshape(-1)))
    live = own >= 0
    f_of = np.broadcast_to(np.arange(F), (B, F))
    assert (inv2d[~live] == -1).all()
    plain = np.bincount(own[live], minlength=P)
    key = f_of[live].astype(np.int64) * (1 << 42) + ids2d[live]                    # (slot, id): ids of this test stay below 2^42
    uniq = np.bincount(own[live][np.unique(key, return_index=True)[1]], minlength=P)
    assert (uniq <= counts).all() and (counts <= plain).all(), (uniq, counts, plain)
    over, demand = int((counts > cap).any()), int(counts.max())
    assert int(flags) == over and list(cstat) == [over, demand]
    slabs = send.reshape(P, cap + 1)
    assert np.array_equal(slabs[:, 0], np.minimum(counts, cap) | (np.int64(demand) << 32))
    assert not over, "the capacities of the de-duplication cases are ample"
    pos = inv2d[live]
    assert (pos >= 0).all() and np.array_equal(pos // cap, own[live]) and (pos % cap < counts[pos // cap]).all()
    assert np.array_equal(slabs[pos // cap, 1 + pos % cap], loc[live] * F + f_of[live])       # every live element finds its payload word
    assert np.array_equal(np.bincount(np.unique(pos) // cap, minlength=P), counts)            # every reserved slot is somebody's
    narrow = live & (ids2d < 0xffffffff)
    b_of = np.broadcast_to(np.arange(B)[:, None], (B, F))
    gkey = (f_of[narrow].astype(np.int64) * (B // tile + 1) + b_of[narrow] // tile) * (1 << 34) + ids2d[narrow]
    _, ginv = np.unique(gkey, return_inverse=True)
    lo, hi = np.full(ginv.max() + 1 if ginv.size else 0, np.iinfo(np.int64).max), np.full(ginv.max() + 1 if ginv.size else 0, -1)
    np.minimum.at(lo, ginv, inv2d[narrow])
    np.maximum.at(hi, ginv, inv2d[narrow])
    assert np.array_equal(lo, hi), "equal (slot, id) pairs inside one tile must share one position"
    wide = inv2d[live & ~narrow]
    assert np.unique(wide).size == wide.size                                                  # ids >= 2^32 - 1: sent once each


def _bucket_buffers(G, P, cap, n):
    return (G.alloc("send", 0, P * (cap + 1), torch.int64, cap + 1), G.alloc("inv", 0, max(1, n), torch.int64, 64)[:n],
            G.alloc("counts", 0, P, torch.int64, 64, fill=0), G.alloc("flags", 0, 1, torch.int32, 64, fill=0),
            G.alloc("cstat", 0, 2, torch.int64, 64, fill=0), torch.zeros(128, dtype=torch.int32, device=DEV))


# ---- a. routing -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [3, 8, 64])
def test_routing_at_the_32_bit_boundary(built_lib, P):
    """ops.shard_route, bucket_cap and bags_bucket against oracle.np_ref.shard_div_owner for vocabularies on both sides of
    FieldDiv::small (V < 2^31 - 1) and far past it: owners and local rows exact at every shard edge."""
    from dir_amd import ops
    from oracle import np_ref as R
    vocab = [2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5, 2 ** 40 + 3]
    F = len(vocab)
    cols = []
    for V in vocab:
        q, r = divmod(V, P)
        thr = r * (q + 1)
        edges = [x for o in range(P) for x in ((o * (q + 1), o * (q + 1) + q) if o < r else (thr + (o - r) * q, thr + (o - r) * q + q - 1))]
        cols.append(np.array([0, thr - 1, thr, thr + 1] + edges + [V - 1, V, -1], np.int64))
    ids = np.stack(cols, axis=1)
    n = ids.shape[0]
    ok = (ids >= 0) & (ids < np.array(vocab)[None, :])
    want_o, want_l = np.zeros_like(ids), np.zeros_like(ids)
    for f, V in enumerate(vocab):
        o, l = R.shard_div_owner(np.where(ok[:, f], ids[:, f], 0), V, P)
        want_o[:, f], want_l[:, f] = o, l
    assert {int(x) for x in want_o[ok]} == set(range(P))                      # every owner is somebody's
    vocab_dev = torch.tensor(vocab, dtype=torch.int64, device=DEV)
    tid = torch.from_numpy(ids).to(DEV)
    # 1. the routing entry
    o, l = ops.shard_route(tid.reshape(-1), vocab_dev, P)
    o, l = _np(o).reshape(n, F), _np(l).reshape(n, F)
    assert np.array_equal(o[ok], want_o[ok]) and np.array_equal(l[ok], want_l[ok])
    assert (l[ids < 0] == -1).all()
    # 2. the one-hot bucketing: owner = the slab, local row = the payload word
    G = Guards(DEV)
    cap = n * F
    send, inv, counts, flags, cstat, ws = _bucket_buffers(G, P, cap, n * F)
    ops.shard_bucket_cap(tid.reshape(-1), vocab_dev, P, cap, send, inv, counts, flags, ws, stat=cstat)
    G.check("shard_bucket_cap")
    iv, sl = _np(inv).reshape(n, F), _np(send).reshape(P, cap + 1)
    assert (iv[~ok] == -1).all() and (iv[ok] >= 0).all()
    assert np.array_equal(iv[ok] // cap, want_o[ok])
    word = sl[iv[ok] // cap, 1 + iv[ok] % cap]
    assert np.array_equal(word // F, want_l[ok]) and np.array_equal(word % F, np.broadcast_to(np.arange(F), (n, F))[ok])
    check_bucket_plain(_router(vocab, P), ids.reshape(-1), F, P, cap, _np(send), _np(inv), _np(counts), _np(flags)[0], _np(cstat))
    # 3. the bag bucketing: one entry per bag -> the mask bit is the owner, the record's payload the local row
    cap_e = cap_b = n * F
    slabs = G.alloc("bag slabs", 0, P * (cap_e + 1) * 2, torch.int64, (cap_e + 1) * 2)
    pos = G.alloc("pos", 0, n * F * P, torch.int32, P)
    mask = G.alloc("mask", 0, n * F, torch.int64, 64)
    denom = G.alloc("denom", 0, n * F, torch.float32, 64)
    offs = torch.arange(n * F + 1, dtype=torch.int64, device=DEV)
    ops.shard_bags_bucket(tid.reshape(-1), offs, None, n, F, 1, vocab_dev, P, None, 0, 0, cap_e, cap_b, slabs, pos, mask, denom,
                          torch.zeros(256, dtype=torch.int32, device=DEV))
    G.check("shard_bags_bucket")
    mk = _np(mask).reshape(n, F).astype(np.uint64)
    assert (mk[~ok] == 0).all()
    assert np.array_equal(mk[ok], np.uint64(1) << want_o[ok].astype(np.uint64))
    ps = _np(pos).reshape(n, F, P)
    rec = _np(slabs).reshape(P, cap_e + 1, 2)
    hdr_e = rec[:, 0, 0] & 0xffffffff
    assert np.array_equal(hdr_e, np.bincount(want_o[ok], minlength=P))
    found = {}
    for o_ in range(P):                                                       # (return position -> payload) of every owner's records
        for j in range(int(hdr_e[o_])):
            found[(o_, int(rec[o_, 1 + j, 1] >> 32))] = int(rec[o_, 1 + j, 0])
    for b, f in zip(*np.nonzero(ok)):
        p = int(ps[b, f, want_o[b, f]])
        assert p >= 0 and p // cap_b == want_o[b, f]
        assert found[(int(want_o[b, f]), p % cap_b)] == int(want_l[b, f]) * F + f


# ---- b. bucket_cap, plain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", OWNERS)
def test_bucket_cap_plain(built_lib, P):
    """Ample capacity, a capacity some owners overflow, and all ids on one owner; default and custom layouts."""
    vocab = VOCAB
    F = len(vocab)
    rng = np.random.default_rng(10 + P)
    for partitions in _layouts(P, PARTS):
        router = _router(vocab, P, partitions)
        be = hip_factory([torch.zeros((1, 16), device=DEV)] * F, vocab, router.parts, router.first, P, 16, DEV, partitions is not None)
        std = standin_factory(None, vocab, router.parts, router.first, P, 16, "cpu", False)
        B = 40
        spread = draw_ids(rng, vocab, B, hot=False)
        one = spread.copy()
        one[:, 0], one[:, 1], one[:, 2], one[:, 3] = rng.integers(0, 2, B), -(rng.integers(0, 2, B)), rng.integers(0, 2, B), rng.integers(0, 3, B)     # rows 0..2: slice 0
        own_s, _ = router.route(spread.reshape(-1))
        median = int(np.sort(np.bincount(own_s[own_s >= 0], minlength=P))[(P - 1) // 2])       # the upper half of the owners want more
        for name, ids, cap in (("ample", spread, 176), ("some overflow", spread, max(1, median)), ("one owner", one, 48)):
            G = Guards(DEV)
            send, inv, counts, flags, cstat, ws = _bucket_buffers(G, P, cap, B * F)
            be.bucket_cap(torch.from_numpy(ids).to(DEV), cap, send, inv, counts, flags, ws, stat=cstat)
            G.check("bucket_cap (%s)" % name)
            want = check_bucket_plain(router, ids.reshape(-1), F, P, cap, _np(send), _np(inv), _np(counts), _np(flags)[0], _np(cstat))
            if name == "some overflow" and P >= 3:
                assert (want > cap).any() and not (want > cap).all(), (name, want, cap)
            if name == "one owner":
                assert int(flags) == 1 and (partitions is not None or (want > 0).sum() == 1)
            # the stand-in on the same ids: counts, verdict, statistic, headers; the same words in every slab when nothing overflowed
            s_send, s_inv = torch.zeros(P * (cap + 1), dtype=torch.int64), torch.zeros(B * F, dtype=torch.int64)
            s_counts, s_flags, s_stat = torch.zeros(P, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
            std.bucket_cap(torch.from_numpy(ids), cap, s_send, s_inv, s_counts, s_flags, None, stat=s_stat)
            assert torch.equal(_cpu(counts), s_counts) and int(flags) == int(s_flags) and torch.equal(_cpu(cstat), s_stat)
            hs, ss = _np(send).reshape(P, cap + 1), s_send.numpy().reshape(P, cap + 1)
            assert np.array_equal(hs[:, 0], ss[:, 0])
            if not int(flags):
                for o in range(P):
                    c = int(hs[o, 0] & 0xffffffff)
                    assert np.array_equal(np.sort(hs[o, 1:1 + c]), np.sort(ss[o, 1:1 + c]))
            assert bool((ws == 0).all())                                      # the slab and arrival counters come back to zero


@pytest.mark.parametrize("P", [8, 64])
def test_bucket_cap_crosses_the_launch_switch(built_lib, P):
    """n = 10 100 x 26 ids, just above 256 * 1024: workgroups of 1024 threads, more than one of them; twice on one workspace (the
    arrival counter and the slab counters must come back to zero), the second time with slabs that some owners overflow."""
    from dir_amd import ops
    B, F = 10100, 26
    vocab = [3 + 5 * f for f in range(F)]                                    # tiny tables: V % P != 0, fewer rows than owners at P = 64
    rng = np.random.default_rng(20 + P)
    ids = np.stack([rng.integers(-1, v + 1, size=B) for v in vocab], axis=1).astype(np.int64)
    assert ids.size > 256 * 1024
    router = _router(vocab, P)
    own, _ = router.route(ids.reshape(-1))
    want = np.bincount(own[own >= 0], minlength=P)
    vocab_dev = torch.tensor(vocab, dtype=torch.int64, device=DEV)
    tid = torch.from_numpy(ids).to(DEV).reshape(-1)
    ws = torch.zeros(128, dtype=torch.int32, device=DEV)
    for cap in (int(want.max()) + 3, int(np.sort(want)[P // 2]) + 1):        # ample; then the median demand: the upper half overflows
        G = Guards(DEV)
        send, inv, counts, flags, cstat, _ = _bucket_buffers(G, P, cap, ids.size)
        ops.shard_bucket_cap(tid, vocab_dev, P, cap, send, inv, counts, flags, ws, stat=cstat)
        G.check("shard_bucket_cap (cap %d)" % cap)
        check_bucket_plain(router, ids.reshape(-1), F, P, cap, _np(send), _np(inv), _np(counts), _np(flags)[0], _np(cstat))
        assert bool((ws == 0).all())
    assert int(flags) == 1


# ---- c. bucket_cap(dedup=True) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", OWNERS)
def test_bucket_cap_dedup_heavy_duplicates(built_lib, P):
    vocab = VOCAB
    F = len(vocab)
    rng = np.random.default_rng(30 + P)
    for partitions in _layouts(P, PARTS):
        router = _router(vocab, P, partitions)
        be = hip_factory([torch.zeros((1, 16), device=DEV)] * F, vocab, router.parts, router.first, P, 16, DEV, partitions is not None)
        B = 2500                                                              # two 2048-sample tiles per slot
        ids = np.stack([rng.integers(-1, min(v, 12) + 1, size=B) for v in vocab], axis=1).astype(np.int64)
        cap = B * F
        G = Guards(DEV)
        send, inv, counts, flags, cstat, ws = _bucket_buffers(G, P, cap, B * F)
        be.bucket_cap(torch.from_numpy(ids).to(DEV), cap, send, inv, counts, flags, ws, stat=cstat, dedup=True)
        G.check("bucket_cap(dedup)")
        check_bucket_dedup(router, ids, P, cap, _np(send), _np(be.inv2d(inv, B, F, True)), _np(counts), _np(flags)[0], _np(cstat), 2048)
        assert int(_np(counts).sum()) <= 2 * F * 13 and bool((ws == 0).all())


def test_bucket_cap_dedup_large_batch_and_wide_ids(built_lib):
    """B * F just above 2^20 (the 4096-sample tiles), and a 2^33-row vocabulary with duplicated ids >= 2^32 (too wide for the 32-bit hash
    table: sent once each, still routed right).  P = 8; routing only, no gather behind it."""
    from dir_amd import ops
    P = 8
    B, F = 40330, 26
    vocab = [3 + 5 * f for f in range(F)]
    rng = np.random.default_rng(41)
    ids = np.stack([rng.integers(-1, v + 1, size=B) for v in vocab], axis=1).astype(np.int64)
    assert ids.size > 1 << 20
    for vocab_, ids_, tile in ((vocab, ids, 4096), ([1 << 33, 50], None, 2048)):
        if ids_ is None:
            wide = (1 << 32) + rng.integers(-2, 40, size=600) * ((1 << 33) // 40 - 7)         # a few values, many times each, spread over the owners
            ids_ = np.stack([np.clip(wide, -1, (1 << 33) + 1), rng.integers(-1, 52, size=600)], axis=1).astype(np.int64)
            ids_[::7, 0] = rng.integers(0, 1 << 32, size=ids_[::7, 0].size) // 1000 * 1000     # narrow ids in the same tile
            assert (ids_[:, 0] >= (1 << 32)).sum() > 100
        Bc, Fc = ids_.shape
        router = _router(vocab_, P)
        cap = 8192 if Bc > 10000 else Bc * Fc
        G = Guards(DEV)
        send, inv, counts, flags, cstat, ws = _bucket_buffers(G, P, cap, Bc * Fc)
        ops.shard_bucket_cap_dedup(torch.from_numpy(ids_).to(DEV), torch.tensor(vocab_, dtype=torch.int64, device=DEV), P, cap, send, inv,
                                   counts, flags, ws, stat=cstat)
        G.check("shard_bucket_cap_dedup")
        check_bucket_dedup(router, ids_, P, cap, _np(send), _np(inv.view(Fc, Bc).t()), _np(counts), _np(flags)[0], _np(cstat), tile)
        assert bool((ws == 0).all())


# ---- d / e. the one-hot lookup, step by step and end to end ---------------------------------------------------------------------------
@pytest.mark.parametrize("P,K", PK)
def test_onehot_lookup_against_standin_and_full_tables(built_lib, P, K):
    """gather_slabs (also with sanitize), gather_packed, linear_gather and slab_stat on the slabs the kernels bucketed: bit for bit the
    stand-in's on the same slabs.  End to end: emb = full-table indexing, FM = oracle.fm_second_order, the linear term = ops.linear_logit
    over the unsharded packed rows, all bit for bit, on the fixed path (plain and de-duplicated) and on the exact path."""
    from dir_amd import ops
    from oracle import oracle as O
    vocab = VOCAB
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rows_full = ops.TableSet.ftrl_rows([torch.from_numpy(w).to(DEV) for w in lin])
    bias = torch.tensor([0.25], device=DEV)
    rng = np.random.default_rng(50 + P)
    for partitions in _layouts(P, PARTS):
        hip, std = _pair(full, lin, P, partitions)
        ids = [draw_ids(rng, vocab, B) for B in sizes(P)]
        tid = [torch.from_numpy(i) for i in ids]
        want_lin = [_np(ops.linear_logit(rows_full, t.to(DEV), bias=bias)) if t.shape[0] else np.zeros((0, 1), np.float32) for t in tid]
        for dedup in (False, True):
            R = hip.onehot_lookup(tid, CAP, dedup=dedup, want_fm=True, want_lin=True, bias=bias)
            demand = max(int(s.counts.max()) for s in R)
            for r, s in enumerate(R):
                recv = _cpu(s.recv)
                hdr = recv.view(P, CAP + 1)[:, 0].numpy() & 0xffffffff
                valid = (np.arange(CAP)[None, :] < hdr[:, None]).reshape(-1)
                # d. the owner steps on the received slabs
                rows = torch.full((P * CAP, K), 7.0)
                std.be[r].gather_slabs(recv, CAP, rows)
                assert np.array_equal(_np(s.rows)[valid], rows.numpy()[valid]), (P, partitions, dedup, r)
                assert (_np(s.rows).view(np.int32)[~valid] == JUNK32).all()                  # rows behind a header are not written
                lw = torch.full((P * CAP,), 7.0)
                std.be[r].linear_gather(recv, CAP, lw)
                assert np.array_equal(_np(s.lrows), lw.numpy())
                stat = torch.zeros(2, dtype=torch.int64)
                std.be[r].slab_stat(recv, P, CAP, stat)
                assert torch.equal(_cpu(s.stat), stat) and stat.tolist() == [0, demand]
                G = Guards(DEV)
                recv2, rows2 = G.alloc("recv", r, P * (CAP + 1), torch.int64, CAP + 1), G.alloc("rows", r, (P * CAP, K), torch.float32, CAP * K)
                recv2.copy_(s.recv)
                ops.gather_slabs(hip.be[r].ts, recv2, P, CAP, rows2, sanitize=True)
                G.check("gather_slabs(sanitize)")
                assert np.array_equal(_np(rows2)[valid], rows.numpy()[valid])
                body = _np(recv2).reshape(P, CAP + 1)
                assert np.array_equal(body[:, 0], recv.view(P, CAP + 1)[:, 0].numpy())
                assert (body[:, 1:].reshape(-1)[~valid] == -1).all() and np.array_equal(body[:, 1:].reshape(-1)[valid], recv.view(P, CAP + 1)[:, 1:].reshape(-1).numpy()[valid])
                # e. end to end
                ref = onehot_rows(full, ids[r])
                assert np.array_equal(_np(s.out), ref), (P, partitions, dedup, r)
                assert np.array_equal(_np(s.fm)[:, 0], O.fm_second_order(ref, F, K))
                assert np.array_equal(_np(s.lin), want_lin[r])
        R = hip.exact_lookup(tid, want_fm=True, want_lin=True, bias=bias)
        for r, s in enumerate(R):
            assert np.array_equal(_np(s.rows), std.be[r].gather_packed(_cpu(s.recv)).numpy())
            lw = torch.full((max(1, s.recv.numel()),), 7.0)
            std.be[r].linear_gather(_cpu(s.recv), None, lw)
            assert np.array_equal(_np(s.lw), lw.numpy()[:s.recv.numel()])
            ref = onehot_rows(full, ids[r])
            assert np.array_equal(_np(s.out).reshape(s.B, F * K), ref), (P, partitions, "exact", r)
            if s.B:
                assert np.array_equal(_np(s.fm)[:, 0], O.fm_second_order(ref, F, K))
            assert np.array_equal(_np(s.lin), want_lin[r])


# ---- f / g. bags ------------------------------------------------------------------------------------------------------------------------
def _csr(bags, F, fmaj):
    return [tuple(None if a is None else torch.from_numpy(a) for a in to_csr(b, F, fmaj)) for b in bags]


def check_bags_bucket(std_be, s, csr, combiner, flags, P, F, cap_e, cap_b):
    """bags_bucket of one rank against the stand-in on the same CSR.  -> (mask as uint64 [B*F], longest run)."""
    nb = s.B * F
    v, o, w = csr
    S = dict(slabs=torch.zeros(P * (cap_e + 1) * 2, dtype=torch.int64), pos=torch.full((max(1, nb * P),), -7, dtype=torch.int32),
             mask=torch.zeros(max(1, nb), dtype=torch.int64), denom=torch.zeros(max(1, nb)))
    std_be.bags_bucket(v, o, w, s.B, s.sb, s.sf, combiner, flags, cap_e, cap_b, S["slabs"], S["pos"], S["mask"], S["denom"], None)
    mask, pos = _np(s.mask)[:nb], _np(s.pos)[:nb * P].reshape(nb, P)
    assert np.array_equal(mask, S["mask"].numpy()[:nb])
    codes = np.tile(np.array(std_be._codes(combiner)), s.B)
    dn, sdn = _np(s.denom)[:nb], S["denom"].numpy()[:nb]
    assert np.array_equal(dn[codes != 2], sdn[codes != 2]) and (_ulps(dn[codes == 2], sdn[codes == 2]) <= 1).all()
    rec, srec = _np(s.send).reshape(P, cap_e + 1, 2), S["slabs"].numpy().reshape(P, cap_e + 1, 2)
    assert np.array_equal(rec[:, 0], srec[:, 0])                              # counts and demands
    ne, npairs = rec[:, 0, 0] & 0xffffffff, rec[:, 0, 0] >> 32
    de, db = int(rec[0, 0, 1] & 0xffffffff), int(rec[0, 0, 1] >> 32)
    bits = (mask.astype(np.uint64)[:, None] >> np.arange(P, dtype=np.uint64)[None, :]) & np.uint64(1)
    assert (pos[bits == 0].view(np.int32) == JUNK32).all() if nb else True    # owners without an entry: not written
    fits = pos[bits == 1]
    assert ((fits >= 0) | (fits == -1)).all()
    if db <= cap_b:
        assert (fits >= 0).all()
    gi, oi = np.nonzero((bits == 1) & (pos >= 0))
    assert np.array_equal(pos[gi, oi] // cap_b, oi) and (pos[gi, oi] % cap_b < npairs[oi]).all()
    assert np.unique(pos[gi, oi]).size == gi.size
    assert np.array_equal(np.bincount(oi, minlength=P), npairs)               # exactly min(pairs, cap_b) partial rows per owner
    # runs: per owner the records of one return position are contiguous; their payload / weight sequence is the stand-in's for that pair
    longest = 0
    want_runs = {}
    for o_ in range(P):
        for j in range(int(srec[o_, 0, 0] & 0xffffffff)):
            want_runs.setdefault((o_, int(srec[o_, 1 + j, 1] >> 32)), []).append((int(srec[o_, 1 + j, 0]), int(srec[o_, 1 + j, 1] & 0xffffffff)))
    spos = S["pos"].numpy()[:nb * P].reshape(nb, P)
    for o_ in range(P):
        runs, prev = {}, None
        for j in range(int(ne[o_])):
            ret = int(rec[o_, 1 + j, 1] >> 32)
            if ret != prev:
                assert ret == -1 or ret not in runs, "the records of one (bag, owner) pair form ONE contiguous run"
                prev = ret
            runs.setdefault(ret, []).append((int(rec[o_, 1 + j, 0]), int(rec[o_, 1 + j, 1] & 0xffffffff)))
        for ret, run in runs.items():
            longest = max(longest, len(run))
            assert -1 <= ret < int(npairs[o_])
        if de <= cap_e and db <= cap_b:                                       # nothing overflowed: every pair's run, in CSR entry order
            for g in np.nonzero(bits[:, o_] == 1)[0]:
                assert runs[int(pos[g, o_]) % cap_b] == want_runs[(o_, int(spos[g, o_]) % cap_b)], (o_, g)
        assert sum(len(r_) for r_ in runs.values()) == int(ne[o_])
    return mask.astype(np.uint64), longest


@pytest.mark.parametrize("P,K", PK)
def test_bags_lookup_against_standin_and_float64(built_lib, P, K):
    """All five CASES (weights, per-slot combiners, field_major, the prune flag), default and custom layouts: bags_bucket against the
    stand-in (mask, denom, headers, pos, runs), the stat words of bags_pool, and emb against bags_ref in float64 within
    (L_max + P_live + 8) * 2^-24 * scale -- one rounding per accumulated term plus the clip and the division.  The linear term over the
    same bags within the bar of tests/test_gpu_shard_bags_linear.py (1e-5 relative to 1 + |ref|).
    Measured on an MI355X, worst |got - ref| / scale (the bound at that rank and case): P = 1: 2.1e-07 (1.8e-06), P = 2: 1.8e-07 (1.7e-06),
    P = 3: 2.7e-07 (2.0e-06), P = 8: 2.4e-07 (2.4e-06), P = 33: 2.4e-07 (2.3e-06), P = 64: 3.3e-07 (2.4e-06); P = 8 at K = 6: 2.2e-07
    (2.1e-06), at K = 64: 3.3e-07 (2.2e-06)."""
    from dir_amd import ops
    vocab = BAG_VOCAB
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rng = np.random.default_rng(60 + P)
    worst, bound_of_worst, high, upper = 0.0, 0.0, 0, 0
    for partitions in _layouts(P, BAG_PARTS):
        hip, std = _pair(full, lin, P, partitions)
        for c, (wmode, comb, mn, fmaj, prune) in enumerate(CASES):
            Bs = sizes(P)
            bags = [draw_bags(rng, B, vocab, BAG_MAXLEN, wmode) for B in Bs]
            csr = _csr(bags, F, fmaj)
            lc = ("sum", "mean", "sqrtn")[c % 3]
            flags = ops.PRUNE_NONPOSITIVE_WEIGHTS if prune else 0
            R = hip.bags_lookup(csr, Bs, comb, mn, fmaj, flags, CAP_E, CAP_B, want_fm=True, lin=(lc, torch.tensor([0.5])))
            for r, s in enumerate(R):
                mask, L_max = check_bags_bucket(std.be[r], s, csr[r], comb, flags, P, F, CAP_E, CAP_B)
                high += int((mask >> np.uint64(63)).astype(bool).sum())
                upper += int(((mask >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(bool).sum())
                stat = torch.zeros(3, dtype=torch.int64)
                std.be[r].bags_pool(_cpu(s.recv), CAP_E, CAP_B, mn, torch.zeros((P * CAP_B, K)), stat=stat)
                assert torch.equal(_cpu(s.stat), stat) and int(stat[0]) == 0
                if not s.B:
                    continue
                ref, scale = bags_ref(full, bags[r], comb, mn, prune)
                P_live = max(bin(int(m)).count("1") for m in mask)
                L_drawn = max(len(i_) for row in bags[r] for i_, _ in row)
                bound = (L_drawn + P_live + 8) * 2.0 ** -24
                err = np.abs(_np(s.out).astype(np.float64) - ref)
                rel = float((err / np.maximum(scale, 1e-30))[scale > 0].max()) if (scale > 0).any() else 0.0
                if rel > worst:
                    worst, bound_of_worst = rel, bound
                assert L_max <= L_drawn and (err <= bound * scale).all(), (P, K, c, r, rel, bound)
                fmv = _np(ops.fm_logit(s.out, F, K))
                assert (np.abs(_np(s.fm) - fmv) <= 2e-5 * (1 + np.abs(fmv))).all()
                want = lin_forward64(lin, lin_entries(bags[r], vocab, lc, prune), s.B) + 0.5
                assert _close(_np(s.lin)[:, 0], want) <= 1e-5
    print("bags P=%d K=%d: worst |got - ref| / scale = %.3g (bound there %.3g)" % (P, K, worst, bound_of_worst))
    if P == 64:
        assert high > 0 and upper > 0             # bags with owner 63 (the sign bit of the int64 mask) and with owners 32..62


@pytest.mark.parametrize("P", OWNERS)
def test_bags_one_owner_per_bag_is_bitwise_the_unsharded_bag(built_lib, P):
    """Every bag's live entries on ONE owner, the owners cycling over all P: emb = ops.embedding_bag on the full tables, FM = ops.fm_logit
    of it, the linear term = ops.linear_logit over the unsharded weights, all bit for bit.  The second draw puts runs of 7, 8, 9, 16, 17
    and 40 entries on one owner: they end at, just past and far past the pool kernel's 8-record chunks."""
    from dir_amd import ops
    from dir_amd.shard import div_range
    vocab, K = BAG_VOCAB, 16
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    ts = ops.TableSet([torch.from_numpy(t).to(DEV) for t in full])
    full_w = [torch.from_numpy(w).to(DEV) for w in lin]
    hip, _ = _pair(full, lin, P, None)
    rng = np.random.default_rng(70 + P)
    Bs = sizes(P)
    comb, mn = ["mean", "sqrtn", "sum"], [None, 0.9, None]
    cycled = [_one_owner_bags(rng, B, vocab, P, 20, lambda b, f, r=r: (b + f + 7 * r) % P) for r, B in enumerate(Bs)]
    s0, e0 = div_range(vocab[0], P, P - 1)                                   # the LAST owner's rows of table 0
    lens = [7, 8, 9, 16, 17, 40]
    chunks = [[[(rng.integers(s0, e0, size=L).astype(np.int64) if f == 0 else np.zeros(0, np.int64), rng.uniform(0.1, 2.0, size=L if f == 0 else 0).astype(np.float32))
                for f in range(F)] for L in lens] if r == 0 else [] for r in range(P)]
    for bags, sz, fmaj, lc in ((cycled, Bs, False, "mean"), (chunks, [len(b) for b in chunks], True, "sum")):
        csr = _csr(bags, F, fmaj)
        R = hip.bags_lookup(csr, sz, comb, mn, fmaj, 0, CAP_E, CAP_B, want_fm=True, lin=(lc, None))
        owners = set()
        for r, s in enumerate(R):
            m = _np(s.mask)[:s.B * F].astype(np.uint64)
            assert all(bin(int(x)).count("1") <= 1 for x in m)
            owners |= {int(x).bit_length() - 1 for x in m if x}
            if not s.B:
                continue
            v, o, w = (None if t is None else t.to(DEV) for t in csr[r])
            ref = ops.embedding_bag(ts, v, o, w, combiner=comb, field_major=fmaj, flags=0, max_norm=mn)
            assert torch.equal(s.out, ref), (P, r)
            assert torch.equal(s.fm, ops.fm_logit(ref, F, K))
            assert torch.equal(s.lin, ops.linear_logit(full_w, v, o, w, combiner=lc, field_major=fmaj))
        assert owners == (set(range(P)) if bags is cycled else {P - 1}), sorted(owners)


@pytest.mark.parametrize("P", [3, 8, 64])
def test_bags_bucket_overflow(built_lib, P):
    """cap_e too small alone, cap_b too small alone, both: the demands in the headers are the true ones, nothing is written past cap_e
    records (the guard words and the untouched slots say so), and pos = -1 / return position -1 mark the pairs that did not fit."""
    from dir_amd import ops
    vocab, K = BAG_VOCAB, 16
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rng = np.random.default_rng(80 + P)
    hip, std = _pair(full, lin, P, None)
    Bs = [30] + [0] * (P - 1)
    bags = [draw_bags(rng, B, vocab, BAG_MAXLEN, "pos") for B in Bs]
    csr = _csr(bags, F, False)
    s0 = hip.bags_lookup(csr, Bs, "mean", None, False, 0, CAP_E, CAP_B, want_fm=False)[0]
    rec = _np(s0.send).reshape(P, CAP_E + 1, 2)
    de, db = int(rec[0, 0, 1] & 0xffffffff), int(rec[0, 0, 1] >> 32)
    true_e, true_b = rec[:, 0, 0] & 0xffffffff, rec[:, 0, 0] >> 32              # nothing overflowed here: the headers hold the true counts
    assert de == true_e.max() and db == true_b.max() and de > 4 and db > 2
    for cap_e, cap_b in ((de // 2, CAP_B), (CAP_E, db // 2), (de // 2, db // 2)):
        G = Guards(DEV)
        nb = Bs[0] * F
        send = G.alloc("send", 0, P * (cap_e + 1) * 2, torch.int64, (cap_e + 1) * 2)
        pos, mask, denom = G.alloc("pos", 0, nb * P, torch.int32, P), G.alloc("mask", 0, nb, torch.int64, 64), G.alloc("denom", 0, nb, torch.float32, 64)
        v, o, w = (None if t is None else t.to(DEV) for t in csr[0])
        hip.be[0].bags_bucket(v, o, w, Bs[0], F, 1, "mean", 0, cap_e, cap_b, send, pos, mask, denom, hip.be[0].new_bags_workspace(DEV))
        G.check("bags_bucket (cap_e %d, cap_b %d)" % (cap_e, cap_b))
        got = _np(send).reshape(P, cap_e + 1, 2)
        assert np.array_equal(got[:, 0, 0] & 0xffffffff, np.minimum(true_e, cap_e)) and np.array_equal(got[:, 0, 0] >> 32, np.minimum(true_b, cap_b))
        assert (got[:, 0, 1] == (de | (db << 32))).all()                        # the demands are the true ones, in every header
        assert np.array_equal(_np(mask), _np(s0.mask)[:nb])
        ps = _np(pos).reshape(nb, P)
        bits = (_np(mask).astype(np.uint64)[:, None] >> np.arange(P, dtype=np.uint64)[None, :]) & np.uint64(1)
        fits = ps[bits == 1]
        assert ((fits >= 0) | (fits == -1)).all()
        assert np.array_equal(np.bincount(np.nonzero((bits == 1) & (ps >= 0))[1], minlength=P), np.minimum(true_b, cap_b))
        assert np.array_equal(np.bincount(np.nonzero((bits == 1) & (ps < 0))[1], minlength=P), true_b - np.minimum(true_b, cap_b))
        for o_ in range(P):
            n_ = int(min(true_e[o_], cap_e))
            ret = got[o_, 1:1 + n_, 1] >> 32
            assert ((ret >= -1) & (ret < cap_b)).all()
            if true_b[o_] > cap_b and true_e[o_] <= cap_e:
                assert (ret == -1).any()                                       # the entries of a pair without a partial row still travel, marked
            if true_b[o_] <= cap_b:
                assert (ret >= 0).all()


# ---- h. one training step each ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K", PK)
def test_onehot_training_step(built_lib, P, K):
    """linear_grad against the stand-in (a copy: exact), then apply_adagrad and apply_ftrl(sorted_by=) on every owner; the shards put
    back together against one synchronous float64 step on the full tables over all ranks' batches: within 1e-5 relative to 1 + |want|,
    rows nobody touched bitwise unchanged.  Row 3 of slot 0 is hit twice by every rank."""
    vocab = VOCAB
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rng = np.random.default_rng(90 + P)
    for partitions in _layouts(P, PARTS):
        hip, std = _pair(full, lin, P, partitions)
        hip.enable_training(LR, ACC0)
        Bs = sizes(P)
        ids = [draw_ids(rng, vocab, B) for B in Bs]
        G = [rng.standard_normal((B, F * K)).astype(np.float32) for B in Bs]
        g = [rng.standard_normal((B, 1)).astype(np.float32) for B in Bs]
        R = hip.onehot_train([torch.from_numpy(i) for i in ids], [torch.from_numpy(x) for x in G], CAP, [torch.from_numpy(x) for x in g], FTRL)
        for r, s in enumerate(R):
            send = torch.full((P * CAP,), 7.0)
            std.be[r].linear_grad(torch.from_numpy(g[r]), _cpu(s.inv).view(s.B, F), send)
            assert np.array_equal(_np(s.lgrad_send), send.numpy())
        ref = Reference(full, lin)
        ref.step(np.concatenate(ids), np.concatenate(G), np.concatenate(g), dict(lr=FTRL[0], l1=FTRL[1], l2=FTRL[2]))
        got, (w, n, z) = hip.assembled(), hip.assembled_linear()
        allids = ref.clean(np.concatenate(ids))
        for f in range(F):
            assert _close(got[f], ref.T[f]) <= 1e-5, (P, K, partitions, f, _close(got[f], ref.T[f]))
            for name, a, b in (("w", w, ref.w), ("n", n, ref.n), ("z", z, ref.z)):
                assert _close(a[f], b[f][:, 0]) <= 1e-5, (P, K, partitions, f, name)
            untouched = np.ones(vocab[f], bool)
            untouched[allids[allids[:, f] >= 0, f]] = False
            assert np.array_equal(got[f][untouched].astype(np.float32), full[f][untouched])
            assert np.array_equal(w[f][untouched].astype(np.float32), lin[f][untouched])


@pytest.mark.parametrize("P,K", PK)
def test_bags_training_step(built_lib, P, K):
    """bags_grad and bags_linear_grad against the stand-in on identical inputs (copies exact, divisions within 1 ulp), then bags_adagrad
    and bags_ftrl(sorted_by=) on every owner; the reassembled shards against one synchronous float64 step over all ranks' bags (1e-5
    relative to 1 + |want|), untouched rows bitwise unchanged.  Row 5 of slot 0 sits twice in many bags on every rank; slot 1 has a
    max_norm."""
    from dir_amd import ops
    vocab = BAG_VOCAB
    F = len(vocab)
    full, lin = draw_tables(vocab, K)
    rng = np.random.default_rng(95 + P)
    for partitions in _layouts(P, BAG_PARTS):
        for c, lc in ((2, "mean"), (1, "sqrtn")):       # per-slot combiners + per-slot max_norm + the prune flag; field-major + weights
            wmode, comb, mn, fmaj, prune = CASES[c]
            hip, std = _pair(full, lin, P, partitions)
            hip.enable_training(LR, ACC0)
            Bs = sizes(P)
            bags = [draw_bags(rng, B, vocab, BAG_MAXLEN, wmode) for B in Bs]
            for bl in bags:
                for row in bl:
                    if len(row[0][0]) > 1:
                        row[0][0][:2] = 5
                        row[0][1][:2] = np.abs(row[0][1][:2]) + 0.1
            csr = _csr(bags, F, fmaj)
            G = [rng.standard_normal((B, F * K)).astype(np.float32) for B in Bs]
            g = [rng.standard_normal((B, 1)).astype(np.float32) for B in Bs]
            flags = ops.PRUNE_NONPOSITIVE_WEIGHTS if prune else 0
            R = hip.bags_train(csr, Bs, [torch.from_numpy(x) for x in G], comb, mn, fmaj, flags, CAP_E, CAP_B,
                               g_lin=[torch.from_numpy(x) for x in g], lin_comb=lc, ftrl=FTRL)
            for r, s in enumerate(R):
                nb = s.B * F
                m = _np(s.mask)[:nb].astype(np.uint64)
                bits = (m[:, None] >> np.arange(P, dtype=np.uint64)[None, :]) & np.uint64(1)
                gi, oi = np.nonzero(bits == 1)
                where = _np(s.pos)[:nb * P].reshape(nb, P)[gi, oi]
                copied = np.array(std.be[r]._codes(comb))[gi % F] == 0              # sum slots: c_bag = 1, a copy
                send = torch.full((P * CAP_B, K), 7.0)
                std.be[r].bags_grad(torch.from_numpy(G[r]), CAP_B, _cpu(s.pos), _cpu(s.mask), _cpu(s.denom), s.B, comb, send)
                assert (_ulps(_np(s.rows)[where], send.numpy()[where]) <= 1).all(), (P, K, c, r)
                assert np.array_equal(_np(s.rows)[where[copied]], send.numpy()[where[copied]])
                lsend = torch.full((P * CAP_B,), 7.0)
                std.be[r].bags_linear_grad(torch.from_numpy(g[r]), CAP_B, _cpu(s.pos), _cpu(s.mask), _cpu(s.lden), s.B, lc, lsend)
                assert (_ulps(_np(s.lrows)[where], lsend.numpy()[where]) <= 1).all(), (P, K, c, r)
            allb = [b for bl in bags for b in bl]
            T, acc = [t.astype(np.float64) for t in full], [np.full(t.shape, ACC0) for t in full]
            ref_step(T, acc, allb, np.concatenate(G), comb, mn, prune, LR)
            w, n, z = ([x.astype(np.float64).reshape(-1, 1) for x in lin], [np.full((v, 1), ACC0) for v in vocab], [np.zeros((v, 1)) for v in vocab])
            ents = lin_entries(allb, vocab, lc, prune)
            lin_ftrl64(w, n, z, ents, np.concatenate(g), *FTRL)
            got, (gw, gn, gz) = hip.assembled(), hip.assembled_linear()
            for f in range(F):
                assert _close(got[f], T[f]) <= 1e-5, (P, K, partitions, c, f, _close(got[f], T[f]))
                for name, a, b in (("w", gw, w), ("n", gn, n), ("z", gz, z)):
                    assert _close(a[f], b[f][:, 0]) <= 1e-5, (P, K, partitions, c, f, name)
                untouched = np.ones(vocab[f], bool)
                untouched[ents[f][1]] = False
                assert np.array_equal(got[f][untouched].astype(np.float32), full[f][untouched])
                assert np.array_equal(gw[f][untouched].astype(np.float32), lin[f][untouched])
