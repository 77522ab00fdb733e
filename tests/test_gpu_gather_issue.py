"""The one-hot gather's quad issue phase (csrc/embedding_bag.hip: issue_quad_rows -- K = 16, F = 26, ids [B, F] with unit field stride,
every table holds a row) against the oracle, bit for bit, at the small shapes where it can go wrong: tail waves, pruned ids, id and
output strides, the DIR_GATHER_TABLES_NONEMPTY flag and its fallback, a launch whose waves take a second unit, and the shapes that
stay on the predicated kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F, K = 26, 16
VOCAB = [1000] * F
VOCAB[3], VOCAB[17] = 1, 3          # a one-row and a three-row slot among the 1 000-row ones


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ops(built_lib):
    assert torch.cuda.is_available()
    from dir_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def tabs(ops):
    rng = np.random.default_rng(7)
    tables = [(rng.standard_normal((v, K)) * 0.25).astype(np.float32) for v in VOCAB]
    ts = ops.TableSet([_dev(t) for t in tables])
    assert ts.gather_flags() & ops.TABLES_NONEMPTY
    return tables, ts


def _ids(rng, B, vocab=VOCAB, lo=-1):
    return np.stack([rng.integers(lo, v, size=B) for v in vocab], axis=1).astype(np.int64)


def _route(ts, ids_dev, out=None, flags=None):
    """1: a one-hot launch with these arguments takes the quad issue phase, 0: the predicated kernel (the launcher's own decision)."""
    from dir_amd import _lib
    from dir_amd._abi import _ptr
    F_, K_ = ts.F, ts.K
    if out is None:
        out = torch.empty((1, F_ * K_), dtype=torch.float32, device="cuda")
    return _lib.load().dir_gather_onehot_route(F_, K_, ids_dev.stride(0), ids_dev.stride(1), _ptr(out), out.stride(0),
                                               ts.gather_flags() if flags is None else flags)


def _check(ops, oracle, tables, ts, ids_np, ids_dev=None, quad=None):
    """fm+out, fm-only and out-only launches against the oracle (ids >= vocab_f pruned, as the kernels do with TableSet's vocabulary).
    quad: which issue phase the launches must have taken (None: either)."""
    ids_dev = _dev(ids_np) if ids_dev is None else ids_dev
    if quad is not None:
        assert _route(ts, ids_dev) == int(quad)
    ref = oracle.embedding_bag(tables, ids_np, vocab=True)
    ref_fm = oracle.fm_second_order(ref, len(tables), K)
    emb, fm = ops.gather_fm(ts, ids_dev)
    assert np.array_equal(emb.cpu().numpy(), ref)
    assert np.array_equal(fm.cpu().numpy()[:, 0], ref_fm)
    _, fm2 = ops.gather_fm(ts, ids_dev, want_emb=False)
    assert np.array_equal(fm2.cpu().numpy()[:, 0], ref_fm)
    assert np.array_equal(ops.embedding_bag(ts, ids_dev).cpu().numpy(), ref)
    return ref, ref_fm


@pytest.mark.parametrize("B", [1, 15, 16, 17, 63, 64, 65, 4099])     # a partial quad group, wave, block; many blocks
def test_tail_handling(ops, oracle, tabs, B):
    tables, ts = tabs
    _check(ops, oracle, tables, ts, _ids(np.random.default_rng(B), B), quad=True)


def _pruned_ids(rng, B, kinds):
    """In-range ids with `kinds` of pruned ones in slot 0, slot 25, every slot of sample 7 and every sample of slot 11."""
    ids = _ids(rng, B, lo=0)
    def bad(f, n):
        vals = [k(VOCAB[f]) for k in kinds]
        return np.array([vals[i % len(vals)] for i in range(n)], np.int64)
    rows = rng.choice(B, size=B // 3, replace=False)
    ids[rows, 0] = bad(0, len(rows))
    rows = rng.choice(B, size=B // 3, replace=False)
    ids[rows, 25] = bad(25, len(rows))
    ids[7, :] = [bad(f, f + 1)[f] for f in range(F)]
    ids[:, 11] = bad(11, B)
    return ids


def test_pruned_ids_with_vocabulary(ops, oracle, tabs):
    tables, ts = tabs
    kinds = [lambda v: -1, lambda v: v, lambda v: 1 << 40, lambda v: v + 1]
    ids = _pruned_ids(np.random.default_rng(11), 69, kinds)
    ref, _ = _check(ops, oracle, tables, ts, ids, quad=True)
    assert not ref[7].any() and not ref[:, 11 * K:12 * K].any()


@pytest.mark.parametrize("flags", ["quad", "fallback"])
def test_pruned_ids_without_vocabulary(ops, oracle, tabs, flags):
    """vocab = NULL through the C ABI: the kernel trusts every non-negative id, so only -1 and in-range ids are valid inputs."""
    from dir_amd import _lib
    from dir_amd._abi import _ptr, _stream
    tables, ts = tabs
    B = 69
    ids = _pruned_ids(np.random.default_rng(12), B, [lambda v: -1])
    ref = oracle.embedding_bag(tables, ids)
    ref_fm = oracle.fm_second_order(ref, F, K)
    d = _dev(ids)
    fl = ops.STREAM_ROWS | (ops.TABLES_NONEMPTY if flags == "quad" else 0)
    assert _route(ts, d, flags=fl) == int(flags == "quad")
    emb = torch.full((B, F * K), 7.0, device="cuda")
    fm = torch.full((B, 1), 7.0, device="cuda")
    _lib.check(_lib.load().dir_gather_fm_fused_f32(_ptr(ts.ptrs), None, F, K, _ptr(d), d.stride(0), d.stride(1), fl, B, _ptr(emb), emb.stride(0),
                                                   _ptr(fm), _stream()))
    assert np.array_equal(emb.cpu().numpy(), ref)
    assert np.array_equal(fm.cpu().numpy()[:, 0], ref_fm)


@pytest.mark.parametrize("storage", ["contiguous", "field_major", "wide_view"])
def test_id_storage(ops, oracle, tabs, storage):
    tables, ts = tabs
    B = 259
    ids = _ids(np.random.default_rng(21), B)
    if storage == "contiguous":
        d = _dev(ids)
    elif storage == "field_major":
        d = _dev(ids.T.copy()).t()
        assert d.stride() == (1, B)
    else:       # [B, F] inside [B, F + 3]: unit field stride, sample stride F + 3; the 3 trailing columns hold ids that change the result
        wide = np.empty((B, F + 3), np.int64)       # if they are read as part of the next sample (or the next sample's as this one's)
        wide[:, F:] = np.array([0, 1 << 41, -1])
        wide[:, :F] = ids
        d = _dev(wide)[:, :F]
        assert d.stride() == (F + 3, 1)
    _check(ops, oracle, tables, ts, ids, d, quad=storage != "field_major")      # (field-major ids: the predicated kernel)


@pytest.mark.parametrize("policy", ["stream", "reuse"])          # non-temporal row loads on and off
def test_output_variants(ops, oracle, policy):
    rng = np.random.default_rng(31)
    tables = [(rng.standard_normal((v, K)) * 0.25).astype(np.float32) for v in VOCAB]
    ts = ops.TableSet([_dev(t) for t in tables])
    ts.row_policy = policy
    assert bool(ts.gather_flags() & ops.STREAM_ROWS) == (policy == "stream")
    B = 131
    ids = _ids(rng, B)
    ref, ref_fm = _check(ops, oracle, tables, ts, ids, quad=True)          # out_ld = F * K: fm+out, fm-only, out-only
    # out_ld > F * K: a 16-byte aligned view into a wider buffer; nothing outside the view is written
    ld = F * K + 8
    for call in ("fm_out", "out"):
        buf = torch.full((B, ld), -3.0, device="cuda")
        view = buf[:, 4:4 + F * K]
        assert view.data_ptr() % 16 == 0 and view.stride(0) == ld
        assert _route(ts, _dev(ids), out=view) == 1
        if call == "fm_out":
            _, fm = ops.gather_fm(ts, _dev(ids), out=view)
            assert np.array_equal(fm.cpu().numpy()[:, 0], ref_fm)
        else:
            ops.embedding_bag(ts, _dev(ids), out=view)
        got = buf.cpu().numpy()
        assert np.array_equal(got[:, 4:4 + F * K], ref)
        assert (got[:, :4] == -3.0).all() and (got[:, 4 + F * K:] == -3.0).all()


def test_flag_and_fallback(ops, oracle):
    """An empty table (0 rows: every id of its slot is pruned) takes the flag away and the launch to the predicated kernel; the same
    tables with one row there set it.  Both agree with the oracle."""
    rng = np.random.default_rng(41)
    B = 77
    for v9 in (0, 1):
        vocab = list(VOCAB)
        vocab[9] = v9
        tables = [(rng.standard_normal((v, K)) * 0.25).astype(np.float32) for v in vocab]
        ts = ops.TableSet([_dev(t) if t.size else torch.empty((0, K), device="cuda") for t in tables])
        assert bool(ts.gather_flags() & ops.TABLES_NONEMPTY) == (v9 == 1)
        ids = _ids(rng, B, [max(v, 1) for v in vocab])
        ids[::2, 9] = 0                 # row 0 of slot 9: pruned when the table is empty, looked up when it has its one row
        ids[1::2, 9] = 5
        ref, _ = _check(ops, oracle, tables, ts, ids, quad=v9 == 1)
        assert ref[::2, 9 * K:10 * K].any() == (v9 == 1) and not ref[1::2, 9 * K:10 * K].any()


def test_second_unit_per_wave(ops, oracle):
    """B = 65 536 + 64 + 3: 1 025 work blocks and a partial one on at most 1 024 resident ones, so some waves take a second unit (the
    loop, the tail clamp and the per-unit state once more).  Checked on a fixed sample of rows and on the last 67."""
    rng = np.random.default_rng(51)
    B = 65536 + 64 + 3
    tables = [(rng.standard_normal((1000, K)) * 0.25).astype(np.float32) for _ in range(F)]
    ts = ops.TableSet([_dev(t) for t in tables])
    ids = rng.integers(-1, 1000, size=(B, F)).astype(np.int64)
    assert _route(ts, _dev(ids[:1])) == 1
    emb, fm = ops.gather_fm(ts, _dev(ids))
    sel = np.concatenate([np.sort(rng.choice(B - 67, size=4096, replace=False)), np.arange(B - 67, B)])
    ref = oracle.embedding_bag(tables, ids[sel], vocab=True)
    tsel = torch.from_numpy(sel).cuda()
    assert np.array_equal(emb[tsel].cpu().numpy(), ref)
    assert np.array_equal(fm[tsel].cpu().numpy()[:, 0], oracle.fm_second_order(ref, F, K))


@pytest.mark.parametrize("Fx,Kx", [(13, 16), (27, 16), (52, 16), (26, 8), (26, 32), (8, 16), (4, 16), (2, 16)])
def test_other_shapes(ops, oracle, Fx, Kx):
    """Shapes beside the flagship one, tail wave included: F = 8 at K = 16 takes the quad issue phase (one unit of 8), the others the
    predicated kernel."""
    rng = np.random.default_rng(Fx * 100 + Kx)
    B = 1031
    vocab = [1000] * Fx
    vocab[Fx // 2] = 1
    tables = [(rng.standard_normal((v, Kx)) * 0.25).astype(np.float32) for v in vocab]
    ts = ops.TableSet([_dev(t) for t in tables])
    ids = _ids(rng, B, vocab)
    ids[5, :] = vocab                   # a sample of ids == vocab_f
    assert _route(ts, _dev(ids)) == int((Fx, Kx) == (8, 16))
    ref = oracle.embedding_bag(tables, ids, vocab=True)
    emb, fm = ops.gather_fm(ts, _dev(ids))
    assert np.array_equal(emb.cpu().numpy(), ref)
    assert np.array_equal(fm.cpu().numpy()[:, 0], oracle.fm_second_order(ref, Fx, Kx))
    assert np.array_equal(ops.embedding_bag(ts, _dev(ids.T.copy()).t()).cpu().numpy(), ref)


def test_field_sums_of_the_rows_kernel(ops, oracle, tabs):
    """gather_fm(fsum=...) runs gather_packed_rows_k, which keeps its own issue phase: out, fm and fsum stay what they were."""
    tables, ts = tabs
    B = 67
    ids = _ids(np.random.default_rng(61), B)
    ref = oracle.embedding_bag(tables, ids, vocab=True)
    fsum = torch.empty((B, K), device="cuda")
    emb, fm = ops.gather_fm(ts, _dev(ids), fsum=fsum)
    want = np.zeros((B, K), np.float32)
    for f in range(F):                  # f-ascending fp32 sums
        want = want + ref[:, f * K:(f + 1) * K]
    assert np.array_equal(emb.cpu().numpy(), ref)
    assert np.array_equal(fm.cpu().numpy()[:, 0], oracle.fm_second_order(ref, F, K))
    assert np.array_equal(fsum.cpu().numpy(), want)
