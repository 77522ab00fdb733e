"""The 'div' routing (csrc/shard_route.hpp: route_fd's 32-bit branch for V < 2^31 - 1, div_owner's 64-bit one from there on) over
vocabularies 2^31 - 2, 2^31 - 1, 2^31, 2^31 + 1, 2^32 + 5 and 2^40, at 1, 3, 8 and 64 owners, with every table cut P ways and with a
`parts` list whose slices start on a rank other than 0: ops.shard_route, shard_bucket, shard_bucket_cap, shard_bucket_cap_dedup and
shard_bags_bucket.  The ids (tests/index_range_inputs.route_ids) hold 0, V - 1, V, pruned ids, both sides of make_fielddiv's thr, both
ends of every slice and ids at and above 2^32; owners, local rows, slab counts, payload words and inverse positions are bit for bit what
the NumPy stand-ins give (oracle.np_ref.shard_div_owner, tests/shard_standin.NumpyBackend.route / bucket and the invariants of
tests/test_gpu_shard_loopback), which tests/test_index_range_inputs.py holds to Python's unbounded integers.  A payload word is
local_row * F + slot: with F = 6 every word of the 2^40-row table's upper slices is past 2^31 and past 2^32, and decodes exactly.

tests/test_gpu_shard_loopback.py::test_routing_at_the_32_bit_boundary already routes five such vocabularies at 3, 8 and 64 owners in the
default layout through three of these entries; what is new here is one owner, the parts / first layouts, shard_bucket,
shard_bucket_cap_dedup, the 2^32 + 5 vocabulary and ids above 2^32 inside a vocabulary.  No table is allocated: the module needs no
device memory to speak of."""
import numpy as np
import pytest
import torch

from tests import index_range_inputs as X
from tests.shard_loopback import Guards
from tests.test_gpu_shard_loopback import _bucket_buffers, _router, check_bucket_dedup, check_bucket_plain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOCAB = list(X.ROUTE_VOCAB)
F = len(VOCAB)
CASES = [(P, None) for P in X.ROUTE_OWNERS] + [(P, list(X.ROUTE_PARTS[P])) for P in X.ROUTE_OWNERS if P in X.ROUTE_PARTS]


def _np(t):
    return t.detach().cpu().numpy()


def _case(P, partitions):
    router = _router(VOCAB, P, partitions)
    ids = np.array(X.route_ids(router.parts, seed=P))                      # (a writable copy: the builder's arrays are read-only)
    own, loc = X.route_exact(ids, router.parts, router.first, P)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)      # noqa: E731
    parts, first = (None, None) if partitions is None else (i32(router.parts), i32(router.first))
    return router, ids, own, loc, parts, first, torch.tensor(VOCAB, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("P", X.ROUTE_OWNERS)
def test_shard_route(built_lib, P):
    from dir_amd import ops
    from oracle import np_ref as R
    router, ids, own, loc, _, _, vocab_dev = _case(P, None)
    o, l = ops.shard_route(torch.from_numpy(ids).to(DEV).reshape(-1), vocab_dev, P)
    o, l = _np(o).reshape(ids.shape), _np(l).reshape(ids.shape)
    live = own >= 0
    assert o.dtype == np.int32 and l.dtype == np.int64
    assert np.array_equal(o[live], own[live]) and np.array_equal(l[live], loc[live])
    pruned = ids < 0                                                        # (the entry checks no vocabulary: an id >= V is the caller's to drop)
    assert (l[pruned] == -1).all() and np.array_equal(o.reshape(-1)[pruned.reshape(-1)], (np.arange(ids.size) % P)[pruned.reshape(-1)])
    for f, V in enumerate(VOCAB):
        wo, wl = R.shard_div_owner(np.where(live[:, f], ids[:, f], 0), V, P)
        assert np.array_equal(o[live[:, f], f], wo[live[:, f]]) and np.array_equal(l[live[:, f], f], wl[live[:, f]])


@pytest.mark.parametrize("P,partitions", CASES, ids=lambda v: "parts" if isinstance(v, list) else str(v))
def test_shard_bucket_variable_form(built_lib, P, partitions):
    from dir_amd import ops
    router, ids, own, loc, parts, first, vocab_dev = _case(P, partitions)
    flat = ids.reshape(-1)
    payload, inv, counts, starts = (_np(t) for t in ops.shard_bucket(torch.from_numpy(flat).to(DEV), vocab_dev, P, parts=parts, first=first))
    sp, si, sc, ss = (t.numpy() for t in router.bucket(torch.from_numpy(flat.copy())))
    assert np.array_equal(counts, sc) and np.array_equal(starts, ss)
    n = flat.size
    o, l = own.reshape(-1), loc.reshape(-1)
    dest = np.where(o < 0, np.arange(n) % P, o)                             # a pruned entry travels as a -1 word to owner i % P
    assert sorted(inv.tolist()) == list(range(n))
    want = np.where(l < 0, -1, l * F + np.arange(n) % F)
    assert np.array_equal(payload[inv], want) and np.array_equal(sp[si], want)
    assert ((inv >= starts[dest]) & (inv < starts[dest] + counts[dest])).all()
    for p in range(P):                                                      # the same words per owner as the stand-in's counting sort
        assert np.array_equal(np.sort(payload[starts[p]:starts[p] + counts[p]]), np.sort(sp[ss[p]:ss[p] + sc[p]]))
    assert int((want >= 2 ** 31).sum()) >= 4 and int((want >= 2 ** 32).sum()) >= 2      # the decode past 31 and 32 bits
    assert np.array_equal(want[want >= 0] // F, l[l >= 0]) and np.array_equal(want[want >= 0] % F, (np.arange(n) % F)[l >= 0])


@pytest.mark.parametrize("P,partitions", CASES, ids=lambda v: "parts" if isinstance(v, list) else str(v))
def test_shard_bucket_cap_and_its_dedup_form(built_lib, P, partitions):
    from dir_amd import ops
    router, ids, own, loc, parts, first, vocab_dev = _case(P, partitions)
    n = ids.size
    tid = torch.from_numpy(ids).to(DEV)
    live = own >= 0
    want_counts = np.bincount(own[live], minlength=P)
    for cap in (n, max(1, int(np.sort(want_counts)[(P - 1) // 2]))):        # ample; the median demand: the upper half overflows
        G = Guards(DEV)
        send, inv, counts, flags, cstat, ws = _bucket_buffers(G, P, cap, n)
        ops.shard_bucket_cap(tid.reshape(-1), vocab_dev, P, cap, send, inv, counts, flags, ws, parts=parts, first=first, stat=cstat)
        G.check("shard_bucket_cap")
        got = check_bucket_plain(router, ids.reshape(-1), F, P, cap, _np(send), _np(inv), _np(counts), _np(flags)[0], _np(cstat))
        assert np.array_equal(got, want_counts) and bool((ws == 0).all())
        if cap == n:
            iv, sl = _np(inv).reshape(ids.shape), _np(send).reshape(P, cap + 1)
            word = sl[iv[live] // cap, 1 + iv[live] % cap]
            assert np.array_equal(iv[live] // cap, own[live]) and np.array_equal(word // F, loc[live])
            assert np.array_equal(word % F, np.broadcast_to(np.arange(F), ids.shape)[live]) and int((word >= 2 ** 32).sum()) >= 2
    # the de-duplicating form: every row three times over (duplicates inside one tile share a position; ids >= 2^32 - 1 are sent once each)
    ids3 = np.concatenate([ids, ids[::-1], ids])
    own3, loc3 = (np.concatenate([a, a[::-1], a]) for a in (own, loc))
    B = ids3.shape[0]
    cap = B * F
    G = Guards(DEV)
    send, inv, counts, flags, cstat, ws = _bucket_buffers(G, P, cap, B * F)
    ops.shard_bucket_cap_dedup(torch.from_numpy(ids3).to(DEV), vocab_dev, P, cap, send, inv, counts, flags, ws, parts=parts, first=first,
                               stat=cstat)
    G.check("shard_bucket_cap_dedup")
    inv2d = _np(inv.view(F, B).t())
    check_bucket_dedup(router, ids3, P, cap, _np(send), inv2d, _np(counts), _np(flags)[0], _np(cstat), 2048)
    live3 = own3 >= 0
    sl = _np(send).reshape(P, cap + 1)
    word = sl[inv2d[live3] // cap, 1 + inv2d[live3] % cap]
    assert np.array_equal(inv2d[live3] // cap, own3[live3]) and np.array_equal(word // F, loc3[live3]) and bool((ws == 0).all())
    narrow = live3 & (ids3 < 0xffffffff)
    assert int(_np(counts).sum()) < int(live3.sum()) and len(np.unique(inv2d[narrow])) < int(narrow.sum())      # duplicates did share


@pytest.mark.parametrize("P,partitions", CASES, ids=lambda v: "parts" if isinstance(v, list) else str(v))
def test_shard_bags_bucket(built_lib, P, partitions):
    """One entry per bag: the mask bit is the owner, the record's payload the local row, the return position the bag's."""
    from dir_amd import ops
    router, ids, own, loc, parts, first, vocab_dev = _case(P, partitions)
    n = ids.shape[0]
    live = own >= 0
    G = Guards(DEV)
    cap_e = cap_b = n * F
    slabs = G.alloc("bag slabs", 0, P * (cap_e + 1) * 2, torch.int64, (cap_e + 1) * 2)
    pos = G.alloc("pos", 0, n * F * P, torch.int32, P)
    mask = G.alloc("mask", 0, n * F, torch.int64, 64)
    denom = G.alloc("denom", 0, n * F, torch.float32, 64)
    offs = torch.arange(n * F + 1, dtype=torch.int64, device=DEV)
    ops.shard_bags_bucket(torch.from_numpy(ids).to(DEV).reshape(-1), offs, None, n, F, 1, vocab_dev, P, None, 0, 0, cap_e, cap_b, slabs, pos,
                          mask, denom, torch.zeros(256, dtype=torch.int32, device=DEV), parts=parts, first=first)
    G.check("shard_bags_bucket")
    mk = _np(mask).reshape(n, F).astype(np.uint64)
    assert (mk[~live] == 0).all()
    assert np.array_equal(mk[live], np.uint64(1) << own[live].astype(np.uint64))
    ps = _np(pos).reshape(n, F, P)
    rec = _np(slabs).reshape(P, cap_e + 1, 2)
    hdr_e = rec[:, 0, 0] & 0xffffffff
    assert np.array_equal(hdr_e, np.bincount(own[live], minlength=P))
    found = {}
    for o_ in range(P):
        for j in range(int(hdr_e[o_])):
            found[(o_, int(rec[o_, 1 + j, 1] >> 32))] = int(rec[o_, 1 + j, 0])
    for b, f in zip(*np.nonzero(live)):
        p = int(ps[b, f, own[b, f]])
        assert p >= 0 and p // cap_b == own[b, f]
        assert found[(int(own[b, f]), p % cap_b)] == int(loc[b, f]) * F + f
