"""Every kernel that forms base + id * row_stride, on tables whose last rows lie past element 2^31 (tests/index_range_inputs.py builds the row
counts, the probe ids and the rows a narrow address would wrap to, and checks them on the CPU).  One layout and one consumer per case:

  plain [V, 16], V = 2^27 + 64      dir_gather_fm_fused_f32, dir_embedding_bag_ex2_f32 (one-hot; CSR sum / mean / sqrtn, weights, max_norm),
                                    dir_gather_fm_rows_bits_f32 (want_bits), dir_gather_rows_f32, dir_gather_packed_f32, dir_gather_slabs_f32,
                                    dir_shard_bags_pool_f32, dir_sparse_adagrad_sorted_f32, dir_sparse_adagrad_f32 (chains),
                                    dir_sparse_adagrad_sorted_payload_f32, dir_sparse_adagrad_sorted_bags_f32, dir_sparse_adam_f32,
                                    dir_sparse_adam_payload_norm_f32 + _apply_f32, the multi-hot bag backward through autograd
  PackedTables, ld 32, 2^26 + 64    dir_gather_fm_linear_packed_f32 (with and without emb), dir_deepfm_tower_cs_f16x2_f32 and
                                    dir_deepfm_tower_f16x2_f32 (ops.TOWER_KERNEL "cs" / "rows") at ops.TOWER_MIN_ROWS rows,
                                    dir_deepfm_tower_bf16x3_f32
  train_rows, ld 32, 2^26 + 64      dir_gather_fm_rows_f32 (fsum), dir_gather_fm_rows_bits_f32, dir_sparse_adagrad_sorted_rows_f32 (step, step_fm)
  weights [V], V = 2^31 + 64        dir_linear_sparse_sum_f32 (one-hot, bags), dir_sparse_ftrl_sorted_f32 (sort keys past 2^31)
  ftrl_rows, ld 4, 2^29 + 64        dir_linear_onehot_rows_f32, dir_sparse_ftrl_rows_sorted_f32, dir_sparse_ftrl_rows_sorted_payload_f32,
                                    dir_sparse_ftrl_rows_units_sorted_payload_f32 and dir_shard_linear_gather_units_f32 (rows of one unit),
                                    dir_shard_linear_gather_f32 (flat and slabs), dir_shard_bags_linear_pool_f32,
                                    dir_sparse_ftrl_rows_sorted_bags_f32
  DIN goods [V, 64], 2^25 + 64      dir_din_attention_pool_packed_f32, dir_din_attention_pool_arith_f32 (f16x2 on the wave kernel, bf16x3, f32;
                                    normalize on and off, one Dice case), dir_din_feat_rows_f32, dir_din_feat_rows_backward_f32,
                                    dir_din_attention_pool_save_arith_f32, dir_din_attention_pool_backward_f32 / _rows_f32 / _saved_f32

Readers that copy rows are bit for bit the rows, read back through narrow slices table[r:r + 1] (the slices are cross-checked once against
a flat view at the computed element offset).  Everything else is compared with the reference and bar of the entry's small-shape test, on a
compacted host copy of the touched rows with the ids renamed: the C oracle bit for bit where that test is bit for bit, float64 at 1e-5
scaled otherwise.  Writers: touched rows within 1e-5 of float64, a second run on fresh state bitwise equal on them, and EVERY other row of
every state tensor -- the wrap targets among them -- unchanged, compared on the device.

What a 32-bit id * ld would do here (argued from the builder's wrap targets, tests/test_index_range_inputs.py): row V - 1 starts at
element 2^31 + 63 ld.  As a signed 32-bit element offset it is negative (the address leaves the allocation); cut to 31 bits, or as an
unsigned 32-bit byte offset, it is row 63.  A reader then returns row 63's values, which differ from row V - 1's (the tables are random):
the bitwise row comparison fails.  A writer updates row 63, which is not touched: the untouched-rows comparison fails, and row V - 1 keeps
its start value, more than ten bars away from the float64 result.

A table is built once per layout (torch.empty, filled on the device in chunks) and shared by that layout's cases; only one layout's table
is alive at a time.  A case skips only when the device has less free memory than it needs (the peak measured for it plus 2 GiB); none
does on an idle MI355X.

Measured on an MI355X: every case takes under 2 s (the whole module 10 s: an 8 GiB table is filled in milliseconds); the largest peak is
the FTRL step on the [2^31 + 64] columns, 56 GiB (w, its clone, n and z at 8 GiB each plus the temporaries of the whole-tensor
comparisons), then the packed FTRL rows (48 GiB) and the Adam step on the plain table (40 GiB)."""
import time

import numpy as np
import pytest
import torch

from tests import index_range_inputs as X

pytestmark = pytest.mark.gpu
BAR = X.BAR
GIB = 1 << 30
_ALIVE = {}


def _need_memory(nbytes):
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if free < nbytes:
        pytest.skip("needs %d bytes of device memory, %d free" % (nbytes, free))


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                   # (a copy: the builder's arrays are read-only)


def _fill(t, seed, scale=0.25, uniform=False):
    """Fill a contiguous tensor on the device in chunks of 2^28 elements."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    flat = t.view(-1)
    for s in range(0, flat.numel(), 1 << 28):
        part = flat[s:s + (1 << 28)]
        part.uniform_(-scale, scale, generator=g) if uniform else part.normal_(0.0, scale, generator=g)
    return t


def _layout(name, build):
    """The layout's table(s), built once; the previous layout's are dropped first."""
    if name not in _ALIVE:
        _ALIVE.clear()
        torch.cuda.empty_cache()
        t0 = time.time()
        _ALIVE[name] = build()
        torch.cuda.synchronize()
        print("built layout %s in %.1f s" % (name, time.time() - t0))
    return _ALIVE[name]


def _rows(t, ids):
    """Rows `ids` of t [V, w] (any row stride) through narrow slices -> fp32 [n, w]; ids outside [0, V) give zeros."""
    V = t.shape[0]
    out = torch.zeros((len(ids), t.shape[1]), device=t.device)
    for i, r in enumerate(ids):
        r = int(r)
        if 0 <= r < V:
            out[i] = t[r:r + 1][0]
    return out.cpu().numpy()


def _reader_ids(ld, with_past=True):
    """ids [B, 2]: slot 0 the 97-row table, slot 1 every probe of the big table, a pruned id and (with_past) one id == V."""
    V = X.rows_past(ld)
    big = list(X.probes(ld)) + [-1] + ([V] if with_past else [])
    rng = np.random.default_rng(ld + 7)
    big = np.asarray(big, np.int64)[rng.permutation(len(big))]
    small = rng.integers(0, X.SMALL_V, size=big.size)
    small[:2] = (0, X.SMALL_V - 1)
    return np.stack([small, big], 1).astype(np.int64)


def _compact(tables, ids_by_slot):
    """Host copies of the rows each slot's ids name, and the renaming: -> (host tables [n_f, w], rename(f, ids)).  A pruned id stays
    pruned, an id >= V becomes one past the compact table."""
    touched, host = [], []
    for t, ids in zip(tables, ids_by_slot):
        ids = np.asarray(ids).reshape(-1)
        u = np.unique(ids[(ids >= 0) & (ids < t.shape[0])])
        touched.append(u)
        host.append(_rows(t, u))

    def rename(f, ids):
        ids = np.asarray(ids, np.int64)
        V = tables[f].shape[0]
        return np.where(ids < 0, ids, np.where(ids >= V, len(touched[f]) + (ids - V), np.searchsorted(touched[f], np.minimum(ids, V - 1))))
    return host, rename, touched


def _scaled(got, ref):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (1 + np.abs(ref))).max())


# ---- plain [V, 16] -------------------------------------------------------------------------------------------------------------------
K16 = 16


def _plain():
    def build():
        _need_memory(9 * GIB)
        V = X.rows_past(16)
        big = _fill(torch.empty((V, K16), device="cuda"), 16)
        small = _fill(torch.empty((X.SMALL_V, K16), device="cuda"), 17)
        return small, big
    return _layout("plain16", build)


def test_narrow_slices_agree_with_a_flat_view_at_the_computed_offset(built_lib):
    small, big = _plain()
    ids = X.probes(16)
    flat = big.view(-1)
    want = np.stack([flat[r * K16:(r + 1) * K16].cpu().numpy() for r in ids])
    got = _rows(big, ids)
    assert np.array_equal(got, want)
    assert len({row.tobytes() for row in got}) == len(ids) and np.abs(got).max() > 0       # random rows: a wrapped read returns other data
    for r in ids:
        for tgt in X.wrap_targets(16, r):
            assert not np.array_equal(_rows(big, [tgt])[0], got[ids.index(r)])


def test_plain_onehot_readers_return_the_rows_bit_for_bit(built_lib, oracle):
    from dir_amd import ops
    small, big = _plain()
    ts = ops.TableSet([small, big])
    ids = _reader_ids(16)
    B, F = ids.shape
    want = np.concatenate([_rows(small, ids[:, 0]), _rows(big, ids[:, 1])], 1)
    dids = _cuda(ids)
    emb, fm = ops.gather_fm(ts, dids)
    assert np.array_equal(emb.cpu().numpy(), want), "gather_fm"
    assert np.array_equal(fm.cpu().numpy()[:, 0], oracle.fm_second_order(want, F, K16))
    assert np.array_equal(ops.embedding_bag(ts, dids).cpu().numpy(), want), "embedding_bag one-hot"
    bits = ops.embedding_bag(ts, dids, want_bits=True)
    assert np.array_equal(bits.cpu().numpy(), want), "gather_fm_rows_bits"
    assert np.array_equal(ops.embedding_bag(ts, dids.t().contiguous().t()).cpu().numpy(), want), "field-major ids"
    # the owner-side readers check no vocabulary: probes and pruned entries only
    own = _reader_ids(16, with_past=False)
    n = own.size
    want_o = np.stack([_rows(small, own[:, 0]), _rows(big, own[:, 1])], 1).reshape(n, K16)
    slot = _cuda(np.tile(np.arange(F, dtype=np.int32), own.shape[0]))
    assert np.array_equal(ops.gather_rows(ts, slot, _cuda(own.reshape(-1))).cpu().numpy(), want_o), "gather_rows"
    pay = np.where(own >= 0, own * F + np.arange(F)[None, :], -1).reshape(-1).astype(np.int64)
    assert np.array_equal(ops.gather_packed(ts, _cuda(pay)).cpu().numpy(), want_o), "gather_packed"
    # two slabs of cap words: the first holds the live words and is full but for three, the second is empty
    live = pay[pay >= 0]
    P, cap = 2, live.size + 3
    recv = np.full((P, cap + 1), -7, np.int64)
    recv[0, 0], recv[0, 1:1 + live.size] = live.size | (live.size << 32), live
    recv[1, 0] = 0 | (live.size << 32)
    out = torch.full((P * cap, K16), float("nan"), device="cuda")
    ops.gather_slabs(ts, _cuda(recv.reshape(-1)), P, cap, out)
    got = out.cpu().numpy()
    assert np.array_equal(got[:live.size], want_o[pay >= 0]), "gather_slabs"
    assert np.isnan(got[live.size:]).all(), "rows behind a slab's count must stay untouched"


def _bag_inputs(ld, rng):
    """CSR bags over the two slots: lengths 0 .. 4, bag (b, 1) b's probe alone for the first bags (a `sum` of one entry is the row)."""
    V = X.rows_past(ld)
    probes = list(X.probes(ld))
    B = len(probes) + 6
    vals, offs = [], [0]
    for b in range(B):
        n0 = int(rng.integers(0, 4))
        vals += list(rng.integers(0, X.SMALL_V, size=n0))
        offs.append(len(vals))
        if b < len(probes):
            mine = [probes[b]]
        else:
            mine = list(rng.choice(probes, size=int(rng.integers(0, 5)))) + ([-1, V] if b % 2 else [])
        vals += mine
        offs.append(len(vals))
    vals, offs = np.asarray(vals, np.int64), np.asarray(offs, np.int64)
    slot_of = np.repeat(np.arange(2 * B) % 2, np.diff(offs))
    w = rng.uniform(0.1, 2.0, size=vals.size).astype(np.float32)
    return B, vals, offs, slot_of, w


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_plain_csr_bags_are_the_oracles_bit_for_bit(built_lib, oracle, combiner):
    from dir_amd import ops
    small, big = _plain()
    ts = ops.TableSet([small, big])
    B, vals, offs, slot_of, w = _bag_inputs(16, np.random.default_rng(3))
    host, rename, _ = _compact([small, big], [vals[slot_of == 0], vals[slot_of == 1]])
    cvals = np.where(slot_of == 0, rename(0, vals), rename(1, vals))
    code = {"sum": 0, "mean": 1, "sqrtn": 2}[combiner]
    for mn in (None, 0.75):
        for wts in (None, w):
            ref = oracle.embedding_bag(host, cvals, offsets=offs, weights=wts, combiner=code, B=B, vocab=True, max_norm=mn or 0.0)
            got = ops.embedding_bag(ts, _cuda(vals), _cuda(offs), None if wts is None else _cuda(wts), combiner=combiner, max_norm=mn)
            assert np.array_equal(got.cpu().numpy(), ref), (combiner, mn, wts is not None)
            if combiner == "sum" and mn is None and wts is None:
                n1 = len(X.probes(16))
                assert np.array_equal(got.cpu().numpy()[:n1, K16:], _rows(big, X.probes(16))), "a sum of one entry is the row itself"


def _bag_slab(entries, cap_e, cap_b, n_bags, F=2):
    """One owner's slab of bag records (csrc/shard_wire.hpp): entries = [(local_row, slot, weight, return position)] -> int64 [(cap_e + 1) * 2]."""
    sl = np.zeros((cap_e + 1, 2), np.int64)
    sl[0, 0] = len(entries) | (n_bags << 32)
    sl[0, 1] = len(entries) | (n_bags << 32)
    for j, (row, slot, wt, ret) in enumerate(entries):
        sl[1 + j, 0] = row * F + slot
        sl[1 + j, 1] = int(np.float32(wt).view(np.uint32)) | (ret << 32)
    return sl


def _bag_entries(ld, rng):
    """Owner-side bag records over the two tables: bag q (return position q) holds 1 .. 3 entries; the first bags one probe each."""
    probes = list(X.write_ids(ld)[0])
    entries = []
    n_bags = len(probes) + 4
    for q in range(n_bags):
        if q < len(probes):
            entries.append((probes[q], 1, float(rng.uniform(0.5, 1.5)), q))
        else:
            for j in range(int(rng.integers(1, 4))):
                slot = int(rng.integers(0, 2)) if j else q % 2          # (both slots get entries)
                row = int(rng.integers(0, X.SMALL_V)) if slot == 0 else int(rng.choice([probes[-1], probes[-2], probes[0]]))
                entries.append((row, slot, float(rng.uniform(0.5, 1.5)), q))
    return entries, n_bags


def test_plain_owner_side_bag_pool_is_the_stand_ins_bit_for_bit(built_lib):
    from dir_amd import ops
    from tests.shard_standin import NumpyBackend
    small, big = _plain()
    ts = ops.TableSet([small, big])
    entries, n_bags = _bag_entries(16, np.random.default_rng(5))
    cap_e, cap_b = len(entries) + 2, n_bags + 1
    host, rename, _ = _compact([small, big], [[e[0] for e in entries if e[1] == 0], [e[0] for e in entries if e[1] == 1]])
    centries = [(int(rename(s, [r])[0]), s, w, q) for r, s, w, q in entries]
    std = NumpyBackend([torch.from_numpy(h) for h in host], [h.shape[0] for h in host], [1, 1], [0, 0], 1, K16)
    for mn in (0.0, 0.75):
        want = torch.full((cap_b, K16), float("nan"))
        std.bags_pool(torch.from_numpy(_bag_slab(centries, cap_e, cap_b, n_bags).reshape(-1)), cap_e, cap_b, mn, want)
        out = torch.full((cap_b, K16), float("nan"), device="cuda")
        ops.shard_bags_pool(ts, _cuda(_bag_slab(entries, cap_e, cap_b, n_bags).reshape(-1)), 1, cap_e, cap_b, None, mn, out)
        got, want = out.cpu().numpy(), want.numpy()
        assert np.array_equal(got[:n_bags], want[:n_bags]), mn
        assert np.isnan(got[n_bags:]).all()


def _check_writer(what, c, starts, run, ref, whole=None, repeatable=True):
    """starts: per state tensor its per-slot start values -- device tensors [V_f, w] that are never written, or a number (the closed
    form).  run() -> per state tensor a list of per-slot device tensors after ONE step on fresh copies.  ref(start rows per state per
    slot) -> float64 results.  Touched rows within BAR; a second run bitwise equal on them (repeatable=False: the chains method adds a
    row's entries in chain order, which its small-shape tests do not hold to bitwise equality past two entries; the second run is then
    held to BAR as well); every other row unchanged (whole(): a further comparison once the touched rows are put back, e.g. of the arena
    the state tensors are views of)."""
    t0 = time.time()
    idx = [_cuda(t) for t in c.touched]
    start_rows = [[_rows(st[f], c.touched[f]) if torch.is_tensor(st[f]) else np.full((len(c.touched[f]), c.width), st[f], np.float32)
                   for f in range(2)] for st in starts]
    want = ref(*start_rows)
    firsts = None
    for attempt in range(2):
        state = run()
        rows = [[_rows(s[f], c.touched[f]) for f in range(2)] for s in state]
        if attempt == 0:
            firsts = rows
            errs = {"state%d" % i: max(X.scaled(rows[i][f], want[i][f]) for f in range(2)) for i in range(len(state))}
            for i, s in enumerate(state):
                for f in range(2):
                    st = starts[i][f]
                    if torch.is_tensor(st):
                        s[f][idx[f]] = st[idx[f]]
                        assert torch.equal(s[f], st), "%s: an untouched row moved (state %d, slot %d)" % (what, i, f)
                    else:
                        s[f][idx[f]] = st
                        assert bool((s[f] == st).all()), "%s: an untouched row moved from %g (state %d, slot %d)" % (what, st, i, f)
            if whole is not None:
                whole()
        else:
            for i in range(len(state)):
                for f in range(2):
                    if repeatable:
                        assert np.array_equal(rows[i][f], firsts[i][f]), "%s: two runs on fresh state differ (state %d, slot %d)" % (what, i, f)
                    else:
                        assert X.scaled(rows[i][f], want[i][f]) <= BAR, "%s: second run (state %d, slot %d)" % (what, i, f)
        del state
    torch.cuda.synchronize()
    print("%s: %s  (%.1f s, peak %.1f GiB)" % (what, "  ".join("%s %.2e" % kv for kv in errs.items()), time.time() - t0,
                                               torch.cuda.max_memory_allocated() / GIB))
    bad = {k: v for k, v in errs.items() if not v <= BAR}
    assert not bad, "%s: %s above %.0e of float64" % (what, bad, BAR)


PLAIN_WRITERS = ("adagrad_sorted", "adagrad_chains", "adagrad_payload", "adam", "adam_payload")


@pytest.mark.parametrize("name", PLAIN_WRITERS)
def test_plain_optimiser_steps(built_lib, name):
    import types
    from dir_amd import ops
    from dir_amd.shard import ShardedTables
    small, big = _plain()
    c = X.case("plain16")
    ids, grad = _cuda(c.ids), _cuda(c.grad)
    pay, pgrad = (_cuda(a) for a in X.payload_of(c))
    _need_memory((42 if name.startswith("adam") else 34) * GIB)
    torch.cuda.reset_peak_memory_stats()

    def run():
        tabs = [small.clone(), big.clone()]
        if name.startswith("adagrad"):
            opt = ops.SparseAdagrad(tabs, lr=X.ADAGRAD_LR, initial_accumulator_value=0.1, method="chains" if name.endswith("chains") else "sorted")
            if name.endswith("payload"):
                opt.step_payload(pay, pgrad)
            else:
                opt.step(ids, grad)
            return tabs, opt.accums
        opt = ops.SparseAdam(ops.TableSet(tabs), X.ADAM["b1"], X.ADAM["b2"], X.ADAM["eps"], X.CLIP)
        opt.lr_t = X.lr_t_of()
        if name.endswith("payload"):
            share = opt.norm_payload(pay, pgrad)
            opt.step_payload(pay, pgrad, ShardedTables._sum_norm_shares(types.SimpleNamespace(_collective=lambda: False), share))
        else:
            opt.step(ids, grad)
        return tabs, opt.ms, opt.vs
    if name.startswith("adagrad"):
        _check_writer(name, c, [[small, big], [0.1, 0.1]], run, lambda w0, a0: X.ref_adagrad(c, w0, a0), repeatable=not name.endswith("chains"))
    else:
        # Adam decays every row: var of an untouched row stays exact only because its m and v are zero (one step from zero state)
        _check_writer(name, c, [[small, big], [0.0, 0.0], [0.0, 0.0]], run, lambda w0, m0, v0: X.ref_adam(c, w0, m0, v0))


def test_plain_adagrad_step_over_bag_slabs(built_lib):
    from dir_amd import ops
    from tests.shard_standin import NumpyBackend
    small, big = _plain()
    rng = np.random.default_rng(8)
    entries, n_bags = _bag_entries(16, rng)
    cap_e, cap_b = len(entries) + 2, n_bags + 1
    g_rows = (rng.standard_normal((cap_b, K16)) * 0.5).astype(np.float32)
    touched = [np.unique([e[0] for e in entries if e[1] == f]) for f in range(2)]
    c = X.Case("bags", 16, K16, (X.SMALL_V, big.shape[0]), None, None, touched, None)
    host, rename, _ = _compact([small, big], touched)
    centries = [(int(rename(s, [r])[0]), s, w, q) for r, s, w, q in entries]
    _need_memory(34 * GIB)
    torch.cuda.reset_peak_memory_stats()

    def ref(w0, a0):
        std = NumpyBackend([torch.from_numpy(np.asarray(w, np.float64).copy()) for w in w0], [w.shape[0] for w in w0], [1, 1], [0, 0], 1, K16)
        opt = std.make_optimizer(X.ADAGRAD_LR, 0.1)
        std.bags_adagrad(opt, torch.from_numpy(_bag_slab(centries, cap_e, cap_b, n_bags).reshape(-1)), cap_e, cap_b, torch.from_numpy(g_rows), 0.0)
        return [t.numpy() for t in std.local], opt["acc"]

    def run():
        tabs = [small.clone(), big.clone()]
        opt = ops.SparseAdagrad(tabs, lr=X.ADAGRAD_LR, initial_accumulator_value=0.1)
        opt.step_bags(_cuda(_bag_slab(entries, cap_e, cap_b, n_bags).reshape(-1)), 1, cap_e, cap_b, _cuda(g_rows))
        return tabs, opt.accums
    _check_writer("adagrad_bags", c, [[small, big], [0.1, 0.1]], run, ref)


def test_plain_multi_hot_bag_backward_through_autograd(built_lib):
    """autograd.EmbeddingBag's sparse table gradient over the big table: every entry's coefficient times its bag's gradient, summed per
    row in float64, at the rows the entries name and nowhere else."""
    from dir_amd import autograd as A, ops
    small, big = _plain()
    B, vals, offs, slot_of, w = _bag_inputs(16, np.random.default_rng(3))
    ps, pb = small.clone().requires_grad_(True), big.detach().requires_grad_(True)
    ts = ops.TableSet([ps.data, pb.data])
    out = A.embedding_bag(ts, _cuda(vals), (ps, pb), _cuda(offs), _cuda(w), combiner="mean")
    g = (np.random.default_rng(4).standard_normal((B, 2 * K16)) * 0.5).astype(np.float32)
    out.backward(_cuda(g))
    gb = pb.grad.coalesce()
    V = big.shape[0]
    bag_of = np.repeat(np.arange(2 * B), np.diff(offs))
    ok = (vals >= 0) & (vals < np.where(slot_of == 0, X.SMALL_V, V))
    den = np.zeros(2 * B)
    np.add.at(den, bag_of[ok], w[ok].astype(np.float64))
    sel = ok & (slot_of == 1)
    rows, inv = np.unique(vals[sel], return_inverse=True)
    want = np.zeros((rows.size, K16))
    np.add.at(want, inv, (w[sel] / den[bag_of[sel]])[:, None] * g[bag_of[sel] // 2, K16:].astype(np.float64))
    got_idx, got_val = gb.indices()[0].cpu().numpy(), gb.values().cpu().numpy()
    keep = np.abs(got_val).max(1) > 0                      # (pruned entries arrive as zeros on row 0)
    assert np.array_equal(got_idx[keep], rows)
    assert _scaled(got_val[keep], want) <= BAR
    pb.grad = None


def _region(arena, ts0):
    """The rows of an arena laid out like ts0's (the first row may sit at different offsets of the two allocations)."""
    ld = ts0.ld
    n = sum(ts0.vocab) * ld
    off = (-(arena.data_ptr() // 4)) % (32 if ld == 32 else 4)
    return arena[off:off + n]


def _same_region(arena, ts0, what):
    """With the touched rows put back, the whole arena -- the columns no state tensor views among them -- is the start arena."""
    assert torch.equal(_region(arena, ts0), _region(ts0.arena, ts0)), "%s: the arena differs outside the touched rows" % what


# ---- PackedTables, ld = 32 -----------------------------------------------------------------------------------------------------------
def _packed():
    def build():
        from dir_amd import ops
        _need_memory(22 * GIB)
        V = X.rows_past(32)
        big = _fill(torch.empty((V, K16), device="cuda"), 32)
        small = _fill(torch.empty((X.SMALL_V, K16), device="cuda"), 33)
        lw = [_fill(torch.empty(X.SMALL_V, device="cuda"), 34, 0.1), _fill(torch.empty(V, device="cuda"), 35, 0.1)]
        pt = ops.PackedTables([small, big], lw)
        del big, lw
        return (pt,)
    return _layout("packed32", build)[0]


def _packed_reference(pt, ids, oracle, bias):
    emb_t = [r[:, :K16] for r in pt.rows]
    lin_t = [r[:, K16:K16 + 1] for r in pt.rows]
    want = np.concatenate([_rows(emb_t[f], ids[:, f]) for f in range(2)], 1)
    hostw, rename, _ = _compact(lin_t, [ids[:, 0], ids[:, 1]])
    cids = np.stack([rename(f, ids[:, f]) for f in range(2)], 1)
    cids = np.where(cids >= np.asarray([h.shape[0] for h in hostw])[None, :], -1, cids)      # the oracle's linear sum checks no vocabulary
    return want, oracle.fm_second_order(want, 2, K16), oracle.linear_sparse_sum([h[:, 0] for h in hostw], cids, bias=bias)


def test_packed_rows_gather_fm_linear(built_lib, oracle):
    from dir_amd import ops
    pt = _packed()
    assert pt.ld == 32 and pt.vocab[1] == X.rows_past(32) and pt.absmax() > 0.5
    ids = _reader_ids(32)
    bias = np.array([0.25], np.float32)
    want, fm_ref, lin_ref = _packed_reference(pt, ids, oracle, bias)
    emb, fm, lin = ops.gather_fm_linear(pt, _cuda(ids), bias=_cuda(bias))
    assert np.array_equal(emb.cpu().numpy(), want)
    assert np.array_equal(fm.cpu().numpy()[:, 0], fm_ref) and np.array_equal(lin.cpu().numpy()[:, 0], lin_ref)
    _, fm2, lin2 = ops.gather_fm_linear(pt, _cuda(ids.T.copy()).t(), bias=_cuda(bias), want_emb=False)
    assert torch.equal(fm2, fm) and torch.equal(lin2, lin)


@pytest.mark.parametrize("kernel,split", [("cs", None), ("rows", None), ("cs", "bf16x3")])
def test_packed_rows_fused_tower_looks_up_the_same_rows(built_lib, oracle, monkeypatch, kernel, split):
    """The tower with the lookup inside at the smallest batch that takes that route: bit for bit the tower on the rows (read through
    narrow slices) with the FM and first-order logits as addends -- its small-shape test's bar -- and within 1e-5 of float64."""
    from dir_amd import ops
    pt = _packed()
    monkeypatch.setattr(ops, "TOWER_KERNEL", kernel)
    M = ops.TOWER_MIN_ROWS
    base = _reader_ids(32)
    ids = np.tile(base, (-(-M // base.shape[0]), 1))[:M]
    ids[:, 0] = np.random.default_rng(9).integers(0, X.SMALL_V, size=M)
    bias = np.array([0.125], np.float32)
    want, fm_ref, lin_ref = _packed_reference(pt, ids, oracle, bias)
    torch.manual_seed(11)
    ws = [torch.randn(64, 32, device="cuda") / 32 ** 0.5, torch.randn(20, 64, device="cuda") / 8]
    bs = [torch.randn(64, device="cuda") * 0.1, torch.randn(20, device="cuda") * 0.1]
    head = (torch.randn(20, device="cuda") / 20 ** 0.5, torch.full((1,), 0.5, device="cuda"))
    assert ops.tower_gather_covers(pt, ws)
    one = ops.tower(None, ws, bs, head=head, gather=(pt, _cuda(ids), _cuda(bias)), split=split)
    two = ops.tower(_cuda(want), ws, bs, head=head, adds=(_cuda(fm_ref), _cuda(lin_ref)), split=split)
    assert torch.equal(one, two)
    x = want.astype(np.float64)
    for w_, b_ in zip(ws, bs):
        x = np.maximum(x @ w_.double().cpu().numpy().T + b_.double().cpu().numpy(), 0)
    ref = x @ head[0].double().cpu().numpy() + 0.5 + fm_ref.astype(np.float64) + lin_ref.astype(np.float64)
    err = _scaled(one.cpu().numpy()[:, 0], ref)
    print("fused tower (%s, %s) over packed rows past 2^31 elements: %.2e" % (kernel, split, err))
    assert err <= 1e-5


# ---- TableSet.train_rows, ld = 32 ------------------------------------------------------------------------------------------------------
def _train():
    def build():
        from dir_amd import ops
        _need_memory(14 * GIB)
        V = X.rows_past(32)
        big = _fill(torch.empty((V, K16), device="cuda"), 36)
        small = _fill(torch.empty((X.SMALL_V, K16), device="cuda"), 37)
        ts = ops.TableSet.train_rows([small, big], 0.1)
        del big
        return (ts,)
    return _layout("train32", build)[0]


def _train_copy(ts):
    """A fresh TableSet.train_rows over a copy of ts's arena (the constructor's layout, without the [V, K] sources)."""
    from dir_amd import ops
    ld, K = ts.ld, ts.K
    n = sum(ts.vocab) * ld
    arena = torch.empty_like(ts.arena)
    off0, off = (-(ts.arena.data_ptr() // 4)) % 32, (-(arena.data_ptr() // 4)) % 32
    arena[off:off + n].copy_(ts.arena[off0:off0 + n])
    rows = []
    for v in ts.vocab:
        rows.append(arena[off:off + v * ld].view(v, ld))
        off += v * ld
    new = ops.TableSet([r[:, :K] for r in rows], ld=ld)
    new.accums = [r[:, K:] for r in rows]
    new.arena, new.rows = arena, rows
    return new


def test_train_rows_gather_fm_with_field_sums_and_row_maxima(built_lib, oracle):
    from dir_amd import ops
    ts = _train()
    assert ts.ld == 32 and ts.vocab[1] == X.rows_past(32) and ts.absmax() > 0.5
    ids = _reader_ids(32)
    B = ids.shape[0]
    want = np.concatenate([_rows(ts.tables[f], ids[:, f]) for f in range(2)], 1)
    fsum = torch.full((B, K16), float("nan"), device="cuda")
    emb, fm = ops.gather_fm(ts, _cuda(ids), fsum=fsum)
    assert np.array_equal(emb.cpu().numpy(), want)
    assert np.array_equal(fm.cpu().numpy()[:, 0], oracle.fm_second_order(want, 2, K16))
    assert np.array_equal(fsum.cpu().numpy(), want[:, :K16] + want[:, K16:])             # f-ascending fp32 sums
    fsum2 = torch.empty_like(fsum)
    emb2, fm2 = ops.gather_fm(ts, _cuda(ids), fsum=fsum2, want_bits=True)
    assert torch.equal(emb2, emb) and torch.equal(fm2, fm) and torch.equal(fsum2, fsum)
    rb, ab = emb2._dir_bits[:2]
    row_max = np.abs(want).max(1).astype(np.float32)
    assert np.array_equal(rb.cpu().numpy(), row_max.view(np.int32)) and int(ab.item()) == int(row_max.max().view(np.int32))
    _, fm3 = ops.gather_fm(ts, _cuda(ids), want_emb=False)
    assert torch.equal(fm3, fm)


@pytest.mark.parametrize("name", ["step", "step_fm"])
def test_train_rows_adagrad_steps(built_lib, name):
    from dir_amd import ops
    ts0 = _train()
    c = X.case("train32")
    ids, grad = _cuda(c.ids), _cuda(c.grad)
    B = c.ids.shape[0]
    _need_memory(34 * GIB)
    torch.cuda.reset_peak_memory_stats()
    fm_g = _cuda((np.random.default_rng(12).standard_normal(B) * 0.5).astype(np.float32))
    fsum = torch.empty((B, K16), device="cuda")
    emb, _ = ops.gather_fm(ts0, ids, fsum=fsum)
    # step_fm's small-shape test: bit for bit fm_logit_backward(add_in=grad) followed by step(); the float64 reference takes that gradient
    d = ops.fm_logit_backward(emb, fm_g, 2, K16, add_in=grad) if name == "step_fm" else grad
    cc = c._replace(grad=d.cpu().numpy())

    def run(fused=True):
        ts = _train_copy(ts0)
        opt = ops.SparseAdagrad(ts, lr=X.ADAGRAD_LR)
        if name == "step_fm" and fused:
            opt.step_fm(ids, grad, fm_g, fsum)
        else:
            opt.step(ids, d)
        run.arena = ts.arena
        return ts.tables, ts.accums
    _check_writer("train_rows " + name, cc, [ts0.tables, ts0.accums], run, lambda w0, a0: X.ref_adagrad(cc, w0, a0),
                  whole=lambda: _same_region(run.arena, ts0, "train_rows " + name))
    if name == "step_fm":
        run(True)
        fused = run.arena
        run(False)
        assert torch.equal(_region(fused, ts0), _region(run.arena, ts0)), "step_fm must equal fm_logit_backward + step bit for bit"


# ---- first-order weights [V], V = 2^31 + 64 ----------------------------------------------------------------------------------------------
def _linear():
    def build():
        _need_memory(9 * GIB)
        V = X.rows_past(1)
        return _fill(torch.empty(X.SMALL_V, device="cuda"), 38, 0.1), _fill(torch.empty(V, device="cuda"), 39, 0.1)
    return _layout("linear1", build)


def test_linear_weights_onehot_and_bags(built_lib, oracle):
    from dir_amd import ops
    small, big = _linear()
    ts = ops.TableSet([small, big])
    cols = [small.view(-1, 1), big.view(-1, 1)]
    ids = _reader_ids(1, with_past=False)
    bias = np.array([0.25], np.float32)
    host, rename, _ = _compact(cols, [ids[:, 0], ids[:, 1]])
    cids = np.stack([rename(f, ids[:, f]) for f in range(2)], 1)
    hw = [h[:, 0] for h in host]
    got = ops.linear_logit(ts, _cuda(ids), bias=_cuda(bias)).cpu().numpy()[:, 0]
    assert np.array_equal(got, oracle.linear_sparse_sum(hw, cids, bias=bias))
    only = np.stack([np.full(ids.shape[0], -1), ids[:, 1]], 1)                             # the big column alone: the weight itself
    alone = ops.linear_logit(ts, _cuda(only)).cpu().numpy()[:, 0]
    assert np.array_equal(alone, _rows(cols[1], ids[:, 1])[:, 0])
    past = np.asarray([[0, big.shape[0]], [-1, big.shape[0] + 5]], np.int64)               # ids at and past V contribute nothing
    assert np.array_equal(ops.linear_logit(ts, _cuda(past)).cpu().numpy()[:, 0], [_rows(cols[0], [0])[0, 0], 0.0])
    B, vals, offs, slot_of, w = _bag_inputs(1, np.random.default_rng(6))
    live = (vals >= 0) & (vals < np.where(slot_of == 0, X.SMALL_V, big.shape[0]))
    vals = np.where(live, vals, -1)                                                         # (the oracle's linear sum checks no vocabulary)
    host, rename, _ = _compact(cols, [vals[slot_of == 0], vals[slot_of == 1]])
    cvals = np.where(slot_of == 0, rename(0, vals), rename(1, vals))
    hw = [h[:, 0] for h in host]
    for code, comb in enumerate(("sum", "mean", "sqrtn")):
        ref = oracle.linear_sparse_sum(hw, cvals, offsets=offs, entry_weights=w, combiner=code, bias=bias, B=B)
        got = ops.linear_logit(ts, _cuda(vals), offsets=_cuda(offs), entry_weights=_cuda(w), combiner=comb, bias=_cuda(bias))
        assert np.array_equal(got.cpu().numpy()[:, 0], ref), comb


def test_linear_weights_ftrl_step_with_sort_keys_past_2_31(built_lib):
    from dir_amd import ops
    small, big = _linear()
    c = X.case("linear1")
    assert X.SMALL_V + int(c.touched[1][-1]) >= 2 ** 31
    ids, grad = _cuda(c.ids), _cuda(c.grad)
    _need_memory(58 * GIB)
    torch.cuda.reset_peak_memory_stats()
    cols = [small.view(-1, 1), big.view(-1, 1)]

    def run():
        tabs = [small.clone(), big.clone()]
        opt = ops.SparseFtrl(tabs, **X.FTRL, initial_accumulator_value=0.1)
        assert not opt.packed
        opt.step(ids, grad)
        return [t.view(-1, 1) for t in tabs], [a.view(-1, 1) for a in opt.accums], [z.view(-1, 1) for z in opt.linears]
    _check_writer("ftrl on [V] columns", c, [cols, [0.1, 0.1], [0.0, 0.0]], run, lambda w0, n0, z0: X.ref_ftrl(c, w0, n0, z0))


# ---- TableSet.ftrl_rows, ld = 4 ----------------------------------------------------------------------------------------------------------
def _ftrl_rows():
    def build():
        from dir_amd import ops
        _need_memory(11 * GIB)
        V = X.rows_past(4)
        w = [_fill(torch.empty(X.SMALL_V, device="cuda"), 40, 0.1), _fill(torch.empty(V, device="cuda"), 41, 0.1)]
        ts = ops.TableSet.ftrl_rows(w, 0.1)
        z = [_fill(torch.empty(X.SMALL_V, device="cuda"), 42, 0.2, uniform=True), _fill(torch.empty(V, device="cuda"), 43, 0.2, uniform=True)]
        for f in range(2):
            ts.linears[f].copy_(z[f].view(-1, 1))
        del w, z
        return (ts,)
    return _layout("ftrl4", build)[0]


def _ftrl_copy(ts):
    from dir_amd import ops
    n = sum(ts.vocab) * 4
    arena = torch.empty_like(ts.arena)
    off0, off = (-(ts.arena.data_ptr() // 4)) % 4, (-(arena.data_ptr() // 4)) % 4
    arena[off:off + n].copy_(ts.arena[off0:off0 + n])
    rows = []
    for v in ts.vocab:
        rows.append(arena[off:off + v * 4].view(v, 4))
        off += v * 4
    new = ops.TableSet([r[:, 0:1] for r in rows], ld=4)
    new.accums = [r[:, 1:2] for r in rows]
    new.linears = [r[:, 2:3] for r in rows]
    new.arena, new.rows = arena, rows
    return new


def test_ftrl_rows_first_order_readers(built_lib, oracle):
    from dir_amd import ops
    ts = _ftrl_rows()
    assert ts.ld == 4 and ts.vocab[1] == X.rows_past(4)
    ids = _reader_ids(4)
    bias = np.array([0.25], np.float32)
    host, rename, _ = _compact(ts.tables, [ids[:, 0], ids[:, 1]])
    cids = np.stack([rename(f, ids[:, f]) for f in range(2)], 1)
    cids = np.where(cids >= np.asarray([h.shape[0] for h in host])[None, :], -1, cids)
    got = ops.linear_logit(ts, _cuda(ids), bias=_cuda(bias)).cpu().numpy()[:, 0]
    assert np.array_equal(got, oracle.linear_sparse_sum([h[:, 0] for h in host], cids, bias=bias))
    # the owner side: one weight per payload word, 0.0 for a pruned word and for a row past the owner's rows
    F = 2
    pay = np.where(ids >= 0, ids * F + np.arange(F)[None, :], -1).reshape(-1).astype(np.int64)
    want = np.stack([_rows(ts.tables[f], ids[:, f])[:, 0] for f in range(2)], 1).reshape(-1)
    n = pay.size
    # ops.shard_linear_gather goes through dir_shard_linear_gather_units_f32 (rows of one unit); the plain entry, which forwards to the
    # same body with its own row stride, is called through the loaded library: both exported symbols stay exercised past 2^31
    from dir_amd import _lib
    from dir_amd._abi import _ptr, _stream

    def plain_entry(ts, recv, P, cap, out):
        _lib.check(_lib.load().dir_shard_linear_gather_f32(_ptr(ts._ptrs), ts.ld, _ptr(ts.vocab_dev), ts.F, _ptr(recv), P, cap or 0,
                                                           0 if cap else recv.numel(), _ptr(out), _stream()))
    P, cap = 2, n + 3
    recv = np.full((P, cap + 1), -1, np.int64)
    recv[0, 0], recv[0, 1:1 + n] = n | (n << 32), pay
    recv[1, 0] = 0 | (n << 32)
    for fn in (ops.shard_linear_gather, plain_entry):
        out = torch.full((n,), float("nan"), device="cuda")
        fn(ts, _cuda(pay), 1, None, out)
        assert np.array_equal(out.cpu().numpy(), want), fn.__name__ + " (flat)"
        out = torch.full((P * cap,), float("nan"), device="cuda")
        fn(ts, _cuda(recv.reshape(-1)), P, cap, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want) and not got[n:].any(), fn.__name__ + " (slabs): every word is written, 0.0 behind the count"


# the ids name the C entry a case drives: dir_sparse_ftrl_rows_sorted_f32, ..._sorted_payload_f32, ..._units_sorted_payload_f32
@pytest.mark.parametrize("name", ["step", "step_payload", "step_payload_units"])
def test_ftrl_rows_steps(built_lib, name):
    from dir_amd import ops
    ts0 = _ftrl_rows()
    c = X.case("ftrl4")
    ids, grad = _cuda(c.ids), _cuda(c.grad)
    pay, pgrad = X.payload_of(c)
    pay, pgrad = _cuda(pay), _cuda(pgrad.reshape(-1))
    _need_memory(50 * GIB)
    torch.cuda.reset_peak_memory_stats()

    def run():
        ts = _ftrl_copy(ts0)
        opt = ops.SparseFtrl(ts, **X.FTRL, initial_accumulator_value=0.1)
        assert opt.packed
        if name == "step":
            opt.step(ids, grad)
        elif name == "step_payload_units":                                  # dir_sparse_ftrl_rows_units_sorted_payload_f32 (rows of one unit)
            opt.step_payload(pay, pgrad.view(-1, 1))
        else:                                                               # the plain entry, through the loaded library
            from dir_amd import _lib
            from dir_amd._abi import _ptr, _stream
            lib = _lib.load()
            ws, need, _ = opt._sort_area("step_payload", lib.dir_sparse_adagrad_sorted_workspace_bytes, pay.numel(), 1, 1)
            _lib.check(lib.dir_sparse_ftrl_rows_sorted_payload_f32(_ptr(ts._ptrs), ts.F, _ptr(pay), pay.numel(), _ptr(pgrad), opt.lr, opt.l1,
                                                                   opt.l2, _ptr(opt.row_base), opt.total_rows, ws, need, None, _stream()))
        run.arena = ts.arena
        return ts.tables, ts.accums, ts.linears
    _check_writer("ftrl_rows " + name, c, [ts0.tables, ts0.accums, ts0.linears], run, lambda w0, n0, z0: X.ref_ftrl(c, w0, n0, z0),
                  whole=lambda: _same_region(run.arena, ts0, "ftrl_rows " + name))


def test_ftrl_rows_bag_slabs_pool_and_step(built_lib):
    """The first-order term over bag slabs on the owner: the pool bit for bit the stand-in's (fp32 in entry order), the FTRL step over
    the same slabs within BAR of its float64 rule."""
    from dir_amd import ops
    from tests.shard_standin_bags_linear import BagsLinearBackend
    ts0 = _ftrl_rows()
    rng = np.random.default_rng(44)
    entries, n_bags = _bag_entries(4, rng)
    cap_e, cap_b = len(entries) + 2, n_bags + 1
    touched = [np.unique([e[0] for e in entries if e[1] == f]) for f in range(2)]
    c = X.Case("bags", 4, 1, tuple(ts0.vocab), None, None, touched, None)
    host, rename, _ = _compact(ts0.rows, touched)                         # whole [w | n | z | -] rows
    centries = [(int(rename(s, [r])[0]), s, w, q) for r, s, w, q in entries]
    recv, crecv = _bag_slab(entries, cap_e, cap_b, n_bags).reshape(-1), torch.from_numpy(_bag_slab(centries, cap_e, cap_b, n_bags).reshape(-1))
    std = BagsLinearBackend(None, [h.shape[0] for h in host], [1, 1], [0, 0], 1, 1)
    std.attach_linear([torch.from_numpy(h.copy()) for h in host], None)
    want = torch.full((cap_b,), float("nan"))
    std.bags_linear_pool(crecv, cap_e, cap_b, want)
    out = torch.full((cap_b,), float("nan"), device="cuda")
    ops.shard_bags_linear_pool(ts0, _cuda(recv), 1, cap_e, cap_b, out)
    assert np.array_equal(out.cpu().numpy(), want.numpy()), "shard_bags_linear_pool"
    dlin = (rng.standard_normal(cap_b) * 0.5).astype(np.float32)
    _need_memory(50 * GIB)
    torch.cuda.reset_peak_memory_stats()

    def ref(w0, n0, z0):
        ref_std = BagsLinearBackend(None, [h.shape[0] for h in host], [1, 1], [0, 0], 1, 1)
        rows64 = [np.concatenate([w0[f], n0[f], z0[f], np.zeros_like(w0[f])], 1).astype(np.float64) for f in range(2)]
        ref_std.attach_linear([torch.from_numpy(r) for r in rows64], None)
        ref_std.bags_ftrl(crecv, cap_e, cap_b, torch.from_numpy(dlin), X.FTRL["lr"], X.FTRL["l1"], X.FTRL["l2"])
        return tuple([r.numpy()[:, i:i + 1] for r in ref_std.lin] for i in range(3))

    def run():
        ts = _ftrl_copy(ts0)
        ops.SparseFtrl(ts, **X.FTRL, initial_accumulator_value=0.1).step_bags(_cuda(recv), 1, cap_e, cap_b, _cuda(dlin))
        run.arena = ts.arena
        return ts.tables, ts.accums, ts.linears
    _check_writer("ftrl_rows step_bags", c, [ts0.tables, ts0.accums, ts0.linears], run, ref,
                  whole=lambda: _same_region(run.arena, ts0, "ftrl_rows step_bags"))


# ---- the DIN goods table [V, 64] ---------------------------------------------------------------------------------------------------------
K64 = 64


def _din():
    def build():
        _need_memory(9 * GIB)
        return (_fill(torch.empty((X.rows_past(64), K64), device="cuda"), 64),)
    return _layout("din64", build)[0]


def _din_inputs():
    rng = np.random.default_rng(64)
    probes = np.asarray(X.probes(64), np.int64)
    B, T = len(probes) + 3, 9
    hist = rng.choice(probes, size=(B, T))
    hist[np.arange(len(probes)), 0] = probes                 # every probe is some sample's first position ...
    cand = rng.choice(probes, size=B)
    cand[:len(probes)] = probes[::-1]                        # ... and some sample's candidate
    hist[1, 3], cand[B - 1] = -1, -1
    lens = rng.integers(1, T + 1, size=B).astype(np.int32)
    lens[B - 2] = 0
    H1, H2 = 80, 40
    W = dict(W1=rng.standard_normal((4 * K64, H1)) / 16, b1=rng.standard_normal(H1) * 0.1, W2=rng.standard_normal((H1, H2)) / 9,
             b2=rng.standard_normal(H2) * 0.1, W3=rng.standard_normal(H2) / 6, b3=rng.standard_normal(1) * 0.1)
    W = {k: v.astype(np.float32) for k, v in W.items()}
    ap = np.concatenate([rng.uniform(0.05, 0.3, H1), rng.uniform(0.5, 1.5, H1), rng.standard_normal(H1) * 0.1,
                         rng.uniform(0.05, 0.3, H2), rng.uniform(0.5, 1.5, H2), rng.standard_normal(H2) * 0.1]).astype(np.float32)
    return hist, lens, cand, W, ap


@pytest.mark.parametrize("arith,packed,normalize,activation", [("f16x2", True, False, "sigmoid"), ("f16x2", True, True, "sigmoid"),
                                                               ("f16x2", True, False, "dice"), ("f16x2", False, True, "sigmoid"),
                                                               ("bf16x3", True, False, "sigmoid"), ("bf16x3", True, True, "sigmoid"),
                                                               ("f32", True, False, "sigmoid"), ("f32", True, True, "sigmoid")])
def test_din_unit_over_the_goods_table(built_lib, monkeypatch, arith, packed, normalize, activation):
    from dir_amd import ops
    from oracle import np_ref as R
    table = _din()
    monkeypatch.setattr(ops, "DIN_PACKED", packed)
    hist, lens, cand, W, ap = _din_inputs()
    host, rename, _ = _compact([table], [np.concatenate([hist.reshape(-1), cand])])
    ref, _ = R.din_attention_pool(host[0], rename(0, hist), lens, rename(0, cand), W["W1"], W["b1"], W["W2"], W["b2"], W["W3"], W["b3"],
                                  normalize=normalize, activation=activation, act_params=ap if activation != "sigmoid" else None)
    dw = {k: _cuda(v) for k, v in W.items()}
    got = ops.din_attention_pool(table, _cuda(hist), _cuda(lens), _cuda(cand), dw["W1"], dw["b1"], dw["W2"], dw["b2"], dw["W3"], dw["b3"],
                                 normalize=normalize, activation=activation, act_params=_cuda(ap) if activation != "sigmoid" else None, arith=arith)
    err = _scaled(got.cpu().numpy(), ref)
    print("din unit %s packed=%s normalize=%s %s over [2^25 + 64, 64]: %.2e" % (arith, packed, normalize, activation, err))
    assert err <= 1e-5
    if arith == "f16x2" and packed and not normalize and activation == "sigmoid":
        assert ops.din_arith(table, [dw["W1"], dw["W2"], dw["W3"]]) == ops.DIN_ARITHS["f16x2"]      # what the router picks for this table


def test_din_feature_rows_and_their_backward(built_lib):
    from dir_amd import ops
    table = _din()
    hist, lens, cand, _, _ = _din_inputs()
    B, T = hist.shape
    valid = (np.arange(T)[None, :] < lens[:, None]) & (hist >= 0)
    b_idx, pos = np.nonzero(valid)
    ids_h = hist[b_idx, pos]
    counts = valid.sum(1)
    row_off = (np.cumsum(counts) - counts).astype(np.int64)
    N = ids_h.size
    h32 = _rows(table, ids_h)
    a32 = _rows(table, cand)[b_idx]
    X_, Hc = ops.din_feat_rows(table, _cuda(ids_h), _cuda(b_idx.astype(np.int64)), _cuda(cand))
    assert np.array_equal(X_.cpu().numpy(), np.concatenate([h32, h32 * a32, a32], 1)) and np.array_equal(Hc.cpu().numpy(), h32)
    rng = np.random.default_rng(65)
    dX = rng.standard_normal((N, 3 * K64)).astype(np.float32)
    dH = rng.standard_normal((N, K64)).astype(np.float32)
    grows = ops.din_feat_rows_backward(table, _cuda(ids_h), _cuda(row_off), _cuda(cand), _cuda(dX), _cuda(dH)).cpu().numpy()
    h, a = h32.astype(np.float64), a32.astype(np.float64)
    gh = dX[:, :K64].astype(np.float64) + dX[:, K64:2 * K64] * a + dH
    ga = np.zeros((B, K64))
    np.add.at(ga, b_idx, dX[:, K64:2 * K64].astype(np.float64) * h + dX[:, 2 * K64:])
    ga[cand < 0] = 0
    assert np.abs(grows[:N] - gh).max() <= 1e-5 * (1 + np.abs(gh).max()) and np.abs(grows[N:] - ga).max() <= 2e-5 * (1 + np.abs(ga).max())


@pytest.mark.parametrize("normalize", [False, True])
def test_din_unit_training_forward_and_backward(built_lib, monkeypatch, normalize):
    """dir_din_attention_pool_save_arith_f32 and the three backward entries (single kernel, row pass, row pass on the saved activations)
    over the goods table, against the single-kernel backward on a compacted copy of the looked-up rows with the ids renamed, at the bar
    their small-shape tests hold them to each other (tests/test_gpu_backward.py: 2e-4 on the cancellation-aware scale, 5e-3 for d b3
    under the softmax); the saving forward bit for bit the plain one on the same kernel (the wave kernel: the packed one, which the plain
    forward would take for this table, orders its sums differently); ids_h the looked-up ids."""
    from dir_amd import ops
    table = _din()
    monkeypatch.setattr(ops, "DIN_PACKED", False)
    hist, lens, cand, W, _ = _din_inputs()
    host, rename, _ = _compact([table], [np.concatenate([hist.reshape(-1), cand])])
    small = _cuda(host[0])
    Ws = [_cuda(W[k]) for k in ("W1", "b1", "W2", "b2", "W3", "b3")]
    big_in = (_cuda(hist), _cuda(lens), _cuda(cand))
    small_in = (_cuda(rename(0, hist)), _cuda(lens), _cuda(rename(0, cand)))
    gout = _cuda((np.random.default_rng(66).standard_normal((hist.shape[0], K64))).astype(np.float32))
    out0, sc0 = ops.din_attention_pool(table, *big_in, *Ws, normalize=normalize, want_scores=True, arith="f16x2")
    out1, sc1, saved = ops.din_attention_pool_save(table, *big_in, *Ws, normalize=normalize, arith="f16x2")
    assert torch.equal(out0, out1) and torch.equal(sc0, sc1)
    ref = ops.din_attention_pool_backward(small, *small_in, *Ws, gout, normalize=normalize)
    got = {"single": ops.din_attention_pool_backward(table, *big_in, *Ws, gout, normalize=normalize),
           "rows": ops.din_attention_pool_backward(table, *big_in, *Ws, gout, normalize=normalize, scores=sc0),
           "saved": ops.din_attention_pool_backward(table, *big_in, *Ws, gout, normalize=normalize, scores=sc1, saved=saved)}
    valid = (np.arange(hist.shape[1])[None, :] < lens[:, None]) & (hist >= 0)
    for name, r in got.items():
        assert np.array_equal(r["ids_h"].cpu().numpy(), hist[valid]), name
        assert np.array_equal(rename(0, r["ids_h"].cpu().numpy()), ref["ids_h"].cpu().numpy()), name
        for k in ("gh", "ga", "gW1", "gb1", "gW2", "gb2", "gW3", "gb3"):
            a, b = ref[k].double(), r[k].double()
            err = ((a - b).abs() / (1e-3 + 0.05 * a.abs().max() + a.abs())).max().item()
            assert err < (5e-3 if (k == "gb3" and normalize) else 2e-4), (name, k, err)


def test_release_the_last_layout():
    _ALIVE.clear()
    torch.cuda.empty_cache()
