"""Every consumer of the in-tree radix sort (csrc/radix_sort.hip) at every digit plan of rs_layout, at the table edges and with dropped
entries mixed in (tests/sort_plan_inputs.py builds the inputs and the float64 references, and checks them on the CPU):

  A  ops.rows_scatter_sum, the payload forms SparseAdagrad.step_payload / SparseFtrl.step_payload / SparseAdam.norm_payload +
     step_payload and the id forms SparseAdagrad(method="sorted").step / SparseFtrl.step / SparseAdam.step over PLANS x (300, 20 000
     entries): touched rows within BAR of float64, a row named once by the scatter-sum bit for bit, two calls on fresh state bitwise
     equal, every other row untouched (checked on the device against a clone or the closed form of the start state).
  B  the C entries through raw ctypes with a workspace of EXACTLY the bytes their size query reports between two 4 KiB guard bands
     of 0xA5: both bands unchanged, results bitwise the Python wrapper's.
  C  the Adam clip norm from 50 to 1e7, spread over the rows and concentrated in one hot row, through SparseAdam.step and through
     norm_payload -> ShardedTables._sum_norm_shares -> step_payload; the norm share itself is held to 1e-6 of float64.
  D  ops.adagrad_dense_multi_ over 1, 16, 17 and 33 variables: bitwise adagrad_dense_ one variable at a time, 2e-6 of float64, and an
     autograd.Adagrad step over a 20-parameter group against torch.optim.Adagrad.

Memory: a state tensor is 16 bytes per row (K = 4): 268 MB at 2^24 rows, 2.1 GB at 2^27; the 2^27 cases run for the scatter-sum and the
FTRL packed rows only.  Cases of >= 2^24 rows skip when the device has less free memory than they need, no other case skips."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import sort_plan_inputs as S

pytestmark = pytest.mark.gpu
K, F, BAR = S.K, S.F, S.BAR
BIG_TOTAL = 1 << 24                    # from here on a case may skip for lack of device memory
ONLY_NARROW = 1 << 27                  # ... and from here on only the scatter-sum and the FTRL rows run
CONSUMERS = ("scatter", "adagrad_payload", "ftrl_payload", "adam_payload", "adagrad_ids", "ftrl_ids", "adam_ids")
NARROW = ("scatter", "ftrl_payload", "ftrl_ids")


def _need_memory(total, bytes_needed):
    if total < BIG_TOTAL:
        return
    free = torch.cuda.mem_get_info()[0]
    if free < bytes_needed:
        pytest.skip("needs %d bytes of device memory, %d free" % (bytes_needed, free))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _draw(vocab, width, seed, scale=0.1, uniform=False):
    """Start values drawn on the device (a table of 2^27 rows never crosses the bus): per table [v, width] fp32."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = []
    for v in vocab:
        t = torch.empty((v, width), device="cuda")
        out.append(t.uniform_(-scale, scale, generator=g) if uniform else t.normal_(0.0, scale, generator=g))
    return out


def _rows(t, idx):
    return t[idx].cpu().numpy()


def _check_state(what, c, run, refs):
    """run() -> (states, starts): states = per state tensor a list of per-table device tensors [v, width] after ONE step on fresh
    state; starts = per state tensor a list of per-table start values (a device tensor the step did not touch, or a number: the closed
    form).  refs(touched start values as fp32 arrays, per state tensor per table) -> the float64 results in the same layout."""
    s1, starts = run()
    s2, _ = run()
    idx = [_cuda(t) for t in c.touched]
    for i, (a, b) in enumerate(zip(s1, s2)):
        for f in range(F):
            assert torch.equal(a[f], b[f]), "%s: two calls on fresh state differ (state %d, table %d)" % (what, i, f)
    start_rows = [[_rows(st[f], idx[f]) if torch.is_tensor(st[f]) else np.full((len(c.touched[f]), s1[i][f].shape[1]), st[f], np.float32)
                   for f in range(F)] for i, st in enumerate(starts)]
    ref = refs(*start_rows)
    errs = {}
    for i in range(len(s1)):
        errs["state%d" % i] = max(S.scaled(_rows(s1[i][f], idx[f]), ref[i][f]) for f in range(F))
    print("%s total=%d n=%d: %s" % (what, c.total, c.n, "  ".join("%s %.2e" % kv for kv in errs.items())))
    # every other row is what it was: the touched rows are put back and the whole tensor is compared on the device
    for i in range(len(s1)):
        for f in range(F):
            t, st = s1[i][f], starts[i][f]
            if torch.is_tensor(st):
                t[idx[f]] = st[idx[f]]
                assert torch.equal(t, st), "%s: an untouched row moved (state %d, table %d)" % (what, i, f)
            else:
                t[idx[f]] = st
                assert bool((t == st).all()), "%s: an untouched row moved from %g (state %d, table %d)" % (what, st, i, f)
    bad = {k: v for k, v in errs.items() if not v <= BAR}
    assert not bad, "%s: %s above %.0e of float64" % (what, bad, BAR)
    return errs


def _sum_shares(share):
    """ShardedTables._sum_norm_shares' arithmetic at world 1 (no process group: the collective is skipped)."""
    from dir_amd.shard import ShardedTables
    return ShardedTables._sum_norm_shares(types.SimpleNamespace(_collective=lambda: False), share)


def _ftrl_rows(vocab, seed):
    """TableSet.ftrl_rows with drawn w and z, n = 0.1; -> (rows, clones of the start w and z)."""
    from dir_amd import ops
    w0 = _draw(vocab, 1, seed)
    rows = ops.TableSet.ftrl_rows([w.reshape(-1) for w in w0], 0.1)
    z0 = _draw(vocab, 1, seed + 1, scale=0.2, uniform=True)
    for f in range(F):
        rows.linears[f].copy_(z0[f])
    return rows, w0, z0


def _run_consumer(name, total, n):
    from dir_amd import ops
    ids_form = name.endswith("_ids")
    c = S.ids_entries(total, n) if ids_form else S.entries(total, n)
    what = "%s" % name
    if name == "scatter":
        _need_memory(total, int(2.5 * total * K * 4))
        pos, vals = _cuda(S.positions_of(c)), _cuda(c.grad)
        out = torch.full((total, K), float("nan"), device="cuda")
        ops.rows_scatter_sum(pos, vals, total, out=out)
        again = ops.rows_scatter_sum(pos.clone(), vals.clone(), total)
        assert torch.equal(out, again), "two calls differ"
        del again
        tp, want, counts = S.ref_scatter(c)
        got = out[_cuda(tp)].cpu().numpy()
        err = S.scaled(got, want)
        print("scatter total=%d n=%d: %.2e" % (total, n, err))
        live_e = np.flatnonzero(c.live)
        uk, first = np.unique(c.key[live_e], return_index=True)
        once = counts == 1
        assert np.array_equal(uk, tp) and once.any()
        assert np.array_equal(got[once], c.grad[live_e[first[once]]]), "a row named once must hold its entry bit for bit"
        assert np.isfinite(got).all() and int(out.count_nonzero()) == int(np.count_nonzero(got)), "rows nobody names must be zeros"
        assert err <= BAR, "scatter: %.3e" % err
        return
    if name.startswith("adagrad"):
        _need_memory(total, int(5.5 * total * K * 4))
        w_start = _draw(c.vocab, K, 100 + total % 97)

        def run():
            tabs = [w.clone() for w in w_start]
            opt = ops.SparseAdagrad(tabs, lr=S.ADAGRAD_LR, initial_accumulator_value=0.1, method="sorted")
            if ids_form:
                ids, grad = S.ids_of(c)
                opt.step(_cuda(ids), _cuda(grad))
            else:
                opt.step_payload(_cuda(S.payload_of(c)), _cuda(c.grad))
            return (tabs, opt.accums), (w_start, [0.1] * F)
        return _check_state(what, c, run, lambda w0, a0: S.ref_adagrad(c, w0, a0))
    if name.startswith("ftrl"):
        _need_memory(total, int(total * (2 * 16 + 4 * 4) * 1.3))

        def run():
            rows, w0, z0 = _ftrl_rows(c.vocab, 200 + total % 97)
            opt = ops.SparseFtrl(rows, **S.FTRL, initial_accumulator_value=0.1)
            assert opt.packed
            g1 = np.ascontiguousarray(c.grad[:, 0])
            if ids_form:
                opt.step(_cuda(S.ids_of(c)[0]), _cuda(g1.reshape(-1, F)))
            else:
                opt.step_payload(_cuda(S.payload_of(c)), _cuda(g1))
            return (rows.tables, rows.accums, rows.linears), (w0, [0.1] * F, z0)
        return _check_state(what, c, run, lambda w0, n0, z0: S.ref_ftrl(c, w0, n0, z0))
    assert name.startswith("adam")
    _need_memory(total, int(7.5 * total * K * 4) + 2 * total)
    w_start = _draw(c.vocab, K, 300 + total % 97)

    def run():
        tabs = [w.clone() for w in w_start]
        opt = ops.SparseAdam(ops.TableSet(tabs), S.ADAM["b1"], S.ADAM["b2"], S.ADAM["eps"], S.CLIP)
        opt.lr_t = S.lr_t_of()
        if ids_form:
            ids, grad = S.ids_of(c)
            opt.step(_cuda(ids), _cuda(grad))
        else:
            pay, grad = _cuda(S.payload_of(c)), _cuda(c.grad)
            opt.step_payload(pay, grad, _sum_shares(opt.norm_payload(pay, grad)))
        return (tabs, opt.ms, opt.vs), (w_start, [0.0] * F, [0.0] * F)       # untouched rows: m = v = 0 and var exact
    return _check_state(what, c, run, lambda w0, m0, v0: S.ref_adam(c, w0, m0, v0))


@pytest.mark.parametrize("name,total,n", [(name, total, n) for total in S.TOTALS for n in S.NS for name in CONSUMERS
                                          if total < ONLY_NARROW or name in NARROW],
                         ids=lambda v: str(v))
def test_consumer_at_every_sort_plan(built_lib, name, total, n):
    _run_consumer(name, total, n)


# ---- B: the workspace guard --------------------------------------------------------------------------------------------------------
GUARD = 4096


class _Guarded:
    """need bytes, 256-byte aligned, in the middle of one buffer of 0xA5 with at least 4 KiB on either side."""

    def __init__(self, need):
        self.need = need
        self.buf = torch.full((need + 2 * GUARD + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.off)
        assert self.off >= GUARD and self.buf.numel() - self.off - need >= GUARD

    def check(self, what):
        torch.cuda.synchronize()
        lo, hi = self.buf[:self.off], self.buf[self.off + self.need:]
        assert bool((lo == 0xA5).all()), "%s wrote below its workspace" % what
        assert bool((hi == 0xA5).all()), "%s wrote past the %d bytes its size query reports" % (what, self.need)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _ptrs(tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device="cuda")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.dir_last_error()


@pytest.mark.parametrize("name,total", [(name, total) for total in S.distinct_plan_totals()
                                        for name in ("scatter", "adagrad_payload", "ftrl_payload", "adam_payload")
                                        if total < ONLY_NARROW or name in NARROW], ids=lambda v: str(v))
def test_entry_stays_inside_the_workspace_it_reports(built_lib, name, total):
    from dir_amd import ops
    lib = built_lib
    n = S.BIG
    c = S.entries(total, n)
    base = _cuda(c.row_base)
    if name == "scatter":
        _need_memory(total, int(2.5 * total * K * 4))
        need = int(lib.dir_rows_scatter_sum_workspace_bytes(n, K, total))
        assert need > 0
        g = _Guarded(need)
        pos, vals = _cuda(S.positions_of(c)), _cuda(c.grad)
        out = torch.full((total, K), float("nan"), device="cuda")
        _ok(lib, lib.dir_rows_scatter_sum_f32(_p(pos), _p(vals), K, n, K, total, _p(out), g.ptr, need, _stream()))
        g.check("dir_rows_scatter_sum_f32")
        assert torch.equal(out, ops.rows_scatter_sum(pos, vals, total))
        return
    if name == "adagrad_payload":
        _need_memory(total, int(5.5 * total * K * 4))
        need = int(lib.dir_sparse_adagrad_sorted_workspace_bytes(n, 1, K, total))
        assert need > 0
        g = _Guarded(need)
        w_start = _draw(c.vocab, K, 400)
        tabs, accs = [w.clone() for w in w_start], [torch.full_like(w, 0.1) for w in w_start]
        pay, grad = _cuda(S.payload_of(c)), _cuda(c.grad)
        tp, ap = _ptrs(tabs), _ptrs(accs)
        _ok(lib, lib.dir_sparse_adagrad_sorted_payload_f32(_p(tp), _p(ap), F, K, _p(pay), n, _p(grad), S.ADAGRAD_LR, _p(base), total, g.ptr, need,
                                                           _stream()))
        g.check("dir_sparse_adagrad_sorted_payload_f32")
        opt = ops.SparseAdagrad([w.clone() for w in w_start], lr=S.ADAGRAD_LR, initial_accumulator_value=0.1)
        opt.step_payload(pay, grad)
        for f in range(F):
            assert torch.equal(tabs[f], opt.ts.tables[f]) and torch.equal(accs[f], opt.accums[f]), f
        return
    if name == "ftrl_payload":
        _need_memory(total, int(total * (2 * 16 + 4 * 4) * 1.3))
        need = int(lib.dir_sparse_adagrad_sorted_workspace_bytes(n, 1, 1, total))
        assert need > 0
        g = _Guarded(need)
        rows, _, _ = _ftrl_rows(c.vocab, 500)
        pay, grad = _cuda(S.payload_of(c)), _cuda(np.ascontiguousarray(c.grad[:, 0]))
        rp = _ptrs(rows.rows)
        _ok(lib, lib.dir_sparse_ftrl_rows_sorted_payload_f32(_p(rp), F, _p(pay), n, _p(grad), S.FTRL["lr"], S.FTRL["l1"], S.FTRL["l2"], _p(base),
                                                             total, g.ptr, need, None, _stream()))
        g.check("dir_sparse_ftrl_rows_sorted_payload_f32")
        rows2, _, _ = _ftrl_rows(c.vocab, 500)
        ops.SparseFtrl(rows2, **S.FTRL, initial_accumulator_value=0.1).step_payload(pay, grad)
        for f in range(F):
            assert torch.equal(rows.rows[f][:, :3], rows2.rows[f][:, :3]), f
        return
    _need_memory(total, int(7.5 * total * K * 4) + 2 * total)
    need = int(lib.dir_sparse_adam_payload_workspace_bytes(n, F, K, total))
    assert need > 0
    g = _Guarded(need)
    w_start = _draw(c.vocab, K, 600)
    tabs, ms, vs = [w.clone() for w in w_start], [torch.zeros_like(w) for w in w_start], [torch.zeros_like(w) for w in w_start]
    pay, grad = _cuda(S.payload_of(c)), _cuda(c.grad)
    opt = ops.SparseAdam(ops.TableSet([w.clone() for w in w_start]), S.ADAM["b1"], S.ADAM["b2"], S.ADAM["eps"], S.CLIP)
    opt.lr_t = S.lr_t_of()
    share = opt.norm_payload(pay, grad)
    words = torch.full((128,), -1, dtype=torch.int64, device="cuda")      # the entry's norm words: 64 low, 64 high (zeroed by the entry)
    _ok(lib, lib.dir_sparse_adam_payload_norm_f32(F, K, _p(pay), n, _p(grad), _p(base), total, _p(words), g.ptr, need, _stream()))
    g.check("dir_sparse_adam_payload_norm_f32")
    assert _share_value(words.view(2, 64)[:, :F]) == _share_value(share), "the norm words differ from the wrapper's"
    assert not bool(words.view(2, 64)[:, F:].any()), "words of tables that do not exist must stay zero"
    norms = _sum_shares(share)
    marks = torch.empty((total + 255) // 256 * 256, dtype=torch.uint8, device="cuda")
    tp, mp, vp = _ptrs(tabs), _ptrs(ms), _ptrs(vs)
    _ok(lib, lib.dir_sparse_adam_payload_apply_f32(_p(tp), _p(mp), _p(vp), F, K, _p(pay), n, _p(grad), S.lr_t_of(), S.ADAM["b1"], S.ADAM["b2"],
                                                   S.ADAM["eps"], S.CLIP, _p(norms), _p(base), total, _p(marks), g.ptr, need, 1, 1, _stream()))
    g.check("dir_sparse_adam_payload_apply_f32")
    opt.step_payload(pay, grad, norms)
    for f in range(F):
        assert torch.equal(tabs[f], opt.ts.tables[f]) and torch.equal(ms[f], opt.ms[f]) and torch.equal(vs[f], opt.vs[f]), f


# ---- C: the Adam clip norm across its range ------------------------------------------------------------------------------------------
def _share_value(share):
    """The norm words of SparseAdam.norm_payload -> per table the exact integer ||g||^2 * 2^32 they stand for."""
    rows = share.cpu().numpy().astype(np.uint64).reshape(2, F)          # [low word, high word] per table
    return [int(lo) + (int(hi) << 32) for lo, hi in zip(rows[0], rows[1])]


@pytest.mark.parametrize("form", ["ids", "payload"])
@pytest.mark.parametrize("shape", S.CLIP_SHAPES)
@pytest.mark.parametrize("norm", S.CLIP_NORMS, ids=lambda v: "%g" % v)
def test_adam_clip_norm_across_its_range(built_lib, norm, shape, form):
    """Measured on an MI355X while the norm was ONE u64 word per table in 2^-32 fixed point: 14 of these 24 cases failed -- every case of
    norm >= 7e4, spread and concentrated alike (the word wraps at ||g||^2 = 2^32: m off by 1.4 ... 450 scaled, the share by 88 % ... 100 %),
    and "concentrated" from 6e4 on (one row-lane contribution above the 4.0e18 clamp: m off by 0.14, the share by 26 %); the cases up to
    6e4 spread held 2.4e-7.  With two words per table all 24 hold the bar: DESIGN.md 5.4."""
    from dir_amd import ops
    c = S.clip_case(norm, shape)
    w0, _, _ = S.clip_start(norm, shape)
    tabs = [_cuda(w) for w in w0]
    opt = ops.SparseAdam(ops.TableSet(tabs), S.ADAM["b1"], S.ADAM["b2"], S.ADAM["eps"], S.CLIP)
    opt.lr_t = S.lr_t_of()
    share_err = None
    if form == "ids":
        opt.step(_cuda(c["ids"]), _cuda(c["grad"]))
    else:
        pay, grad = S.clip_payload(norm, shape)
        pay, grad = _cuda(pay), _cuda(grad)
        share = opt.norm_payload(pay, grad)
        got = _share_value(share)
        share_err = max(abs(g / (n2 * 4294967296.0) - 1.0) for g, n2 in zip(got, c["norm2"]))
        opt.step_payload(pay, grad, _sum_shares(share))
    ref = S.clip_ref(norm, shape)
    state = (tabs, opt.ms, opt.vs)
    errs = {name: max(S.scaled(state[i][f].cpu().numpy(), ref[i][f]) for f in range(F)) for i, name in enumerate("wmv")}
    print("adam clip norm %g %s %s: %s  share %s" % (norm, shape, form, "  ".join("%s %.2e" % kv for kv in errs.items()),
                                                     "-" if share_err is None else "%.2e" % share_err))
    assert share_err is None or share_err <= 1e-6, "the norm share is %.3e off float64 ||g||^2 * 2^32" % share_err
    bad = {k: v for k, v in errs.items() if not v <= BAR}
    assert not bad, "adam clip norm %g %s %s: %s above %.0e of float64" % (norm, shape, form, bad, BAR)


# ---- D: the dense Adagrad multi-launch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-7])
@pytest.mark.parametrize("n_vars", S.DENSE_GROUPS)
def test_dense_adagrad_multi_equals_single_launches_and_float64(built_lib, n_vars, eps):
    from dir_amd import ops
    sizes = S.dense_sizes(n_vars)
    rng = np.random.default_rng(1000 + n_vars)
    lr, steps = 0.05, 3
    w0 = [(rng.standard_normal(s) * 0.3).astype(np.float32) for s in sizes]
    grads = [[(rng.standard_normal(s) * 0.5).astype(np.float32) for s in sizes] for _ in range(steps)]
    wm, am = [_cuda(w) for w in w0], [torch.full((s,), 0.1, device="cuda") for s in sizes]
    ws, as_ = [_cuda(w) for w in w0], [torch.full((s,), 0.1, device="cuda") for s in sizes]
    for g in grads:
        dg = [_cuda(x) for x in g]
        ops.adagrad_dense_multi_(wm, am, dg, lr, eps)
        for v in range(n_vars):
            ops.adagrad_dense_(ws[v], as_[v], dg[v], lr, eps)
    worst = 0.0
    for v in range(n_vars):
        assert torch.equal(wm[v], ws[v]) and torch.equal(am[v], as_[v]), "variable %d of %d (size %d) differs from the single launch" % (
            v, n_vars, sizes[v])
        rw, ra = S.dense_ref(w0[v], np.full(sizes[v], 0.1, np.float32), [g[v] for g in grads], lr, eps)
        worst = max(worst, S.scaled(wm[v].cpu().numpy(), rw), S.scaled(am[v].cpu().numpy(), ra))
    print("adagrad_dense_multi_ %d variables eps=%g: worst scaled error %.2e" % (n_vars, eps, worst))
    assert worst <= S.DENSE_BAR


def test_autograd_adagrad_steps_a_group_of_twenty_like_torch(built_lib):
    from dir_amd import autograd as A
    rng = np.random.default_rng(20)
    sizes = [3, 257, 100003, 1, 256] * 4
    w0 = [(rng.standard_normal(s) * 0.3).astype(np.float32) for s in sizes]
    g0 = [(rng.standard_normal(s) * 0.5).astype(np.float32) for s in sizes]
    mine = [torch.nn.Parameter(_cuda(w)) for w in w0]
    theirs = [torch.nn.Parameter(torch.from_numpy(w.copy())) for w in w0]
    opt = A.Adagrad(mine, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    ref = torch.optim.Adagrad(theirs, lr=0.05, initial_accumulator_value=0.1, eps=0.0)
    for p, q, g in zip(mine, theirs, g0):
        p.grad, q.grad = _cuda(g), torch.from_numpy(g.copy())
    opt.step()
    ref.step()
    worst = max(max(S.scaled(p.detach().cpu().numpy(), q.detach().numpy()), S.scaled(opt.state[p]["sum"].cpu().numpy(), ref.state[q]["sum"].numpy()))
                for p, q in zip(mine, theirs))
    print("autograd.Adagrad, 20 parameters: worst scaled difference from torch.optim.Adagrad %.2e" % worst)
    assert worst <= S.DENSE_BAR
