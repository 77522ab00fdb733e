"""The sharded first-order term has ONE implementation per step, and U = 1 is a value of U: for U in {2, 3, 8} every step over U-unit
packed rows (csrc/shard_linear.hip: linear_gather_k, linear_finish_k, linear_grad_k; csrc/backward.hip: the payload-driven FTRL) equals,
column by column and BIT FOR BIT, the U = 1 call on that column's own packed rows.  Every output is filled with NaN before a call: a
word that a kernel leaves unwritten fails the comparison on either side.

Shapes, the smallest at which each kernel can go wrong: F in {1, 5, 29} (three idle lanes of a quad; one past a quad; one past the 28
fields of one round of the finish's field loop), B in {1, 65} (one past a block's 64 samples), slot vocabularies 7 / 300 / 20; flat
payloads of 0, 1, 513 and 1025 words (one past 256 lanes x 2 and x 4 entries per lane) and slabs with P = 3, cap = 37 and header counts
0 / 17 / 37, pruned words and rows at or beyond the slot's local rows in both; inv as the row-major [B, F] view and as the field-major
transposed view of a de-duplicated bucket, pruned positions, n = 0, with and without bias; an FTRL payload of 1025 words with rows
repeated many times, sorting for itself and on the sort an Adagrad step has just left."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
UNITS = [2, 3, 8]
FS = [1, 5, 29]
VOCAB = [7, 300, 20]
ACC0 = 0.1
NAN = float("nan")
# The two forms of the payload-driven FTRL this file's last test compares agreed bitwise before they were merged (measured on an MI355X
# with the former two entry points): the one form is held to that, not to a tolerance.
FTRL_BITWISE = True


def _vocab(F):
    return [VOCAB[f % 3] for f in range(F)]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _packed(ws):
    """ws[f]: [V_f, U] float32 -> the TableSet over [V_f, 4 U] rows of U blocks [w | n | z | -] (HipBackend.attach_linear's layout)."""
    from dir_amd import ops
    U = ws[0].shape[1]
    n_rows = [w.shape[0] for w in ws]
    arena = torch.zeros(sum(n_rows) * 4 * U + 4, dtype=torch.float32, device="cuda")
    off = (-(arena.data_ptr() // 4)) % 4
    rows = []
    for w, v in zip(ws, n_rows):
        blk = arena[off:off + v * 4 * U].view(v, 4 * U)
        blk[:, 0::4] = _cuda(w)
        blk[:, 1::4] = ACC0
        rows.append(blk)
        off += v * 4 * U
    ts = ops.TableSet([r[:, 0:1] for r in rows], ld=4 * U)
    ts.accums, ts.linears = [r[:, 1:2] for r in rows], [r[:, 2:3] for r in rows]
    ts.arena, ts.rows, ts.units = arena, rows, U
    return ts


def _columns(ws):
    """The same weights as U independent one-unit row sets (TableSet.ftrl_rows)."""
    from dir_amd import ops
    return [ops.TableSet.ftrl_rows([_cuda(w[:, u]) for w in ws], ACC0) for u in range(ws[0].shape[1])]


def _weights(rng, F, U):
    return [(0.3 * rng.standard_normal((v, U))).astype(np.float32) for v in _vocab(F)]


def _payload(rng, F, n, beyond=True):
    """n payload words local_row * F + slot: most inside the slot's rows, some pruned (-1) and -- beyond: what the gather must answer
    with 0.0; an owner's update never receives one -- some at or beyond the local rows."""
    vocab = np.asarray(_vocab(F))
    slot = rng.integers(0, F, size=n)
    row = rng.integers(0, vocab[slot])
    kind = rng.integers(0, 8, size=n)
    if beyond:
        row = np.where(kind == 0, vocab[slot] + rng.integers(0, 3, size=n), row)
    return np.where(kind == 1, -1, row * F + slot).astype(np.int64)


@pytest.mark.parametrize("U", UNITS)
def test_gather_columns_equal_the_one_unit_gather(built_lib, U):
    from dir_amd import ops
    rng = np.random.default_rng(100 + U)
    for F in FS:
        ws = _weights(rng, F, U)
        ts, cols = _packed(ws), _columns(ws)
        for n in (0, 1, 513, 1025):                                                     # flat payloads
            pay = _cuda(_payload(rng, F, n))
            out = torch.full((n * U,), NAN, device="cuda")
            ops.shard_linear_gather(ts, pay, 1, None, out)
            for u in range(U):
                one = torch.full((n,), NAN, device="cuda")
                ops.shard_linear_gather(cols[u], pay, 1, None, one)
                assert torch.equal(out.view(n, U)[:, u], one), (F, n, u)
        P, cap = 3, 37                                                                  # slabs: words behind the count are not read
        recv = _payload(rng, F, P * (cap + 1)).reshape(P, cap + 1)
        for s, cnt in enumerate((0, 17, 37)):
            recv[s, 0] = cnt | (cnt << 32)
        recv = _cuda(recv.reshape(-1))
        out = torch.full((P * cap * U,), NAN, device="cuda")
        ops.shard_linear_gather(ts, recv, P, cap, out)
        o = out.view(P, cap, U)
        assert not bool(o[0].any()) and not bool(o[1, 17:].any()), "0.0 behind the header's count"
        for u in range(U):
            one = torch.full((P * cap,), NAN, device="cuda")
            ops.shard_linear_gather(cols[u], recv, P, cap, one)
            assert torch.equal(o[:, :, u].reshape(-1), one), (F, "slabs", u)


def _inv_views(inv):
    """inv [B, F] int64 -> (the row-major view, the field-major transposed view a de-duplicated bucket returns)"""
    B, F = inv.shape
    fm = inv.t().contiguous().view(-1)
    return (("row-major", inv), ("field-major", fm.view(F, B).t()))


@pytest.mark.parametrize("U", UNITS)
def test_finish_columns_equal_the_one_unit_finish(built_lib, U):
    from dir_amd import ops
    rng = np.random.default_rng(200 + U)
    for F in FS:
        for B in (1, 65):
            for n in (B * F + 3, 0):                                                    # n = 0: nothing came back, every sum is 0.0 + bias
                wback = _cuda(rng.standard_normal(n * U).astype(np.float32))
                pos = rng.integers(0, max(n, 1), size=(B, F))
                inv = _cuda(np.where(rng.integers(0, 6, size=(B, F)) == 0, -1, pos).astype(np.int64))      # pruned positions
                bias = _cuda(rng.standard_normal(U).astype(np.float32))
                for what, iv in _inv_views(inv):
                    for b in (bias, None):
                        out = torch.full((B, U), NAN, device="cuda")
                        ops.shard_linear_finish(wback, iv, b, out, units=U)
                        for u in range(U):
                            one = torch.full((B, 1), NAN, device="cuda")
                            ops.shard_linear_finish(wback.view(n, U)[:, u].contiguous(), iv, None if b is None else b[u:u + 1], one)
                            assert torch.equal(out[:, u:u + 1], one), (F, B, n, what, b is not None, u)


@pytest.mark.parametrize("U", UNITS)
def test_grad_columns_equal_the_one_unit_grad(built_lib, U):
    from dir_amd import ops
    rng = np.random.default_rng(300 + U)
    for F in FS:
        for B in (1, 65):
            for n in (B * F + 5, 0):                                                    # n = 0: an empty send buffer, nothing is written
                pos = rng.permutation(max(n, B * F))[:B * F].reshape(B, F)              # one writer per position
                inv = _cuda(np.where(rng.integers(0, 6, size=(B, F)) == 0, -1, pos).astype(np.int64))
                g = _cuda(rng.standard_normal((B, U)).astype(np.float32))
                for what, iv in _inv_views(inv):
                    send = torch.full((n * U,), NAN, device="cuda")
                    ops.shard_linear_grad(g, iv, send, units=U)
                    for u in range(U):
                        one = torch.full((n,), NAN, device="cuda")
                        ops.shard_linear_grad(g[:, u:u + 1], iv, one)
                        assert torch.equal(send.view(n, U)[:, u], one), (F, B, n, what, u)


@pytest.mark.parametrize("reuse", [False, True], ids=["own_sort", "adagrad_sort"])
@pytest.mark.parametrize("U", UNITS)
def test_ftrl_columns_equal_the_one_unit_ftrl(built_lib, U, reuse):
    """w, n and z of every unit after one payload-driven FTRL step over the U-unit rows against the one-unit step on that column's rows.
    The two entry points this one replaced agreed bitwise on this payload: FTRL_BITWISE above."""
    from dir_amd import ops
    rng = np.random.default_rng(400 + U)
    F, n, K = 3, 1025, 4
    ws = _weights(rng, F, U)
    pay = _payload(rng, F, n, beyond=False)
    pay[:400] = 11 * F + 1                                                              # one row of the 300-row slot 400 times,
    pay[400:700] = rng.integers(0, 7, size=300) * F + 0                                 # the 7-row slot about 43 times per row
    pay = _cuda(pay[rng.permutation(n)])
    g = _cuda(rng.standard_normal((n, U)).astype(np.float32))
    grows = _cuda(rng.standard_normal((n, K)).astype(np.float32))
    hp = dict(lr=0.2, l1=0.01, l2=0.02)

    def step(ts, grad):
        opt = ops.SparseFtrl(ts, **hp)
        if reuse:                                                                       # the co-located embedding rows' Adagrad sorts first
            ada = ops.SparseAdagrad(ops.TableSet([torch.zeros((v, K), device="cuda") for v in _vocab(F)]), 0.1)
            ada.step_payload(pay, grows)
            opt.step_payload(pay, grad, sorted_by=ada)
        else:
            opt.step_payload(pay, grad)
        torch.cuda.synchronize()
        return ts.rows

    rows = step(_packed(ws), g)
    moved = 0
    for u, col in enumerate(_columns(ws)):
        one = step(col, g[:, u].contiguous())
        for f in range(F):
            got, want = rows[f][:, 4 * u:4 * u + 3], one[f][:, 0:3]
            moved += int((want[:, 0].cpu() != torch.from_numpy(ws[f][:, u])).sum())
            if FTRL_BITWISE:
                assert torch.equal(got, want), (U, reuse, u, f)
            else:
                err = float(((got.double() - want.double()).abs() / (1 + want.double().abs())).max())
                assert err <= 1e-5, (U, reuse, u, f, err)
    assert moved > 0, "the step moved some weights"
