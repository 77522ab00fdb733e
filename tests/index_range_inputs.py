"""Inputs and float64 references of tests/test_gpu_index_range.py (host side, NumPy only): for a table whose rows lie `ld` floats apart,
the smallest row count whose last rows lie past element 2^31, the probe ids on either side of every offset at which a narrow address
wraps, and the rows such a wrap would land in.

  rows_past(ld)     ceil(2^31 / ld) + 64 rows: the last 64 rows start at or past element 2^31 (byte 2^33).
  probes(ld)        the last row wholly below and the first row at or after each of the element offsets 2^29, 2^30 and 2^31 (byte offsets
                    2^31, 2^32 and 2^33: a signed and an unsigned 32-bit byte offset and a signed 32-bit element offset end there), row 0,
                    row 4099 (below every line), row V - 1 and five random rows between the 2^31 line and V - 1.  What the READERS look up.
  wrap_targets(ld, p)  the rows that p's element offset e = p * ld or byte offset 4 e, cut to 31 or to 32 bits, lands in.
  write_ids(ld)     what the WRITERS update.  The lines are powers of two, so a cut probe often IS another probe (the first row at 2^31 cut
                    to 31 bits is row 0; the last row below 2^31, its byte offset cut to 32 bits, is the last row below 2^30).  A step that
                    went to the wrong one of two touched rows could then hide behind the other's update, so the probes are taken from the
                    top of the table down and one that is a wrap target of a probe already taken is left OUT of the update and checked as
                    an untouched row instead.  The rows on both sides of the 2^31 line, the random rows and V - 1 always stay.
  case(name)        one small batch over two tables, ids [B, 2]: slot 0 a 97-row table (so the big table's sort keys start at 97, and
                    reach past 2^31 for the first-order weights), slot 1 the big table named by write_ids with V - 1 five times and the
                    first row at the line three times, one pruned id and one id == V (dropped).

The references run oracle.np_ref's float64 rules on a compacted copy of the touched rows only (the big table never exists on the host).
route_ids / route_exact are the inputs of tests/test_gpu_route_wide_vocab.py: ids over vocabularies from 2^31 - 2 to 2^40 and their owners
and local rows in Python's unbounded integers, to which the CPU test holds the NumPy stand-ins.
All of this is asserted on the CPU (tests/test_index_range_inputs.py), never on a kernel."""
import collections
import functools

import numpy as np

from oracle import np_ref as R
from tests.hot_rows_inputs import BAR, scaled  # noqa: F401  (re-exported)

LINES = (1 << 29, 1 << 30, 1 << 31)                       # element offsets
LOW_ROW = 4099                                            # an interior row below every line (element 4099 * 64 < 2^29)
SMALL_V = 97                                              # slot 0 of every writer case
# layout -> (row stride in floats, floats of a row that the consumers read or write as the embedding / weight)
LAYOUTS = collections.OrderedDict([("plain16", (16, 16)), ("packed32", (32, 16)), ("train32", (32, 16)), ("linear1", (1, 1)),
                                   ("ftrl4", (4, 1)), ("din64", (64, 64))])
HOT_LAST, HOT_LINE = 5, 3                                 # how often V - 1 and the first row at the 2^31 line are named

ADAGRAD_LR = 0.05
FTRL = dict(lr=0.2, l1=0.01, l2=0.05)
ADAM = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-4)
CLIP = 100.0


def rows_past(ld):
    return -(-(1 << 31) // ld) + 64


def line_rows(ld):
    """Per line: (the last row wholly below it, the first row at or after it)."""
    return [(line // ld - 1, -(-line // ld)) for line in LINES]


@functools.lru_cache(maxsize=None)
def probes(ld):
    V = rows_past(ld)
    first_past = line_rows(ld)[-1][1]
    rng = np.random.default_rng(ld)
    rand = rng.choice(np.arange(first_past + 1, V - 1), size=5, replace=False)
    out = sorted({0, LOW_ROW, V - 1, *[r for pair in line_rows(ld) for r in pair], *[int(r) for r in rand]})
    assert out[0] == 0 and out[-1] == V - 1
    return tuple(out)


def wrap_targets(ld, p):
    """The rows a 31-bit or 32-bit cut of p's element or byte offset lands in, p itself (no wrap) left out."""
    e = p * ld
    cuts = {e % (1 << 31), e % (1 << 32), (4 * e) % (1 << 31) // 4, (4 * e) % (1 << 32) // 4}
    return sorted({c // ld for c in cuts} - {p})


@functools.lru_cache(maxsize=None)
def write_ids(ld):
    """-> (kept probes, ascending; every wrap target of a kept probe, ascending)."""
    kept, targets = [], set()
    for p in sorted(probes(ld), reverse=True):
        if p in targets:
            continue
        kept.append(p)
        targets.update(wrap_targets(ld, p))
    return tuple(sorted(kept)), tuple(sorted(targets))


Case = collections.namedtuple("Case", "name ld width vocab ids grad touched compact")


@functools.lru_cache(maxsize=None)
def case(name):
    ld, width = LAYOUTS[name]
    V = rows_past(ld)
    kept, _ = write_ids(ld)
    first_past = line_rows(ld)[-1][1]
    rng = np.random.default_rng(1000 + ld)
    big = list(kept) + [V - 1] * (HOT_LAST - 1) + [first_past] * (HOT_LINE - 1) + [-1, V]
    big = np.asarray(big, np.int64)[rng.permutation(len(big))]
    small = rng.integers(0, SMALL_V, size=big.size)
    small[:3] = (0, SMALL_V - 1, SMALL_V - 1)
    ids = np.stack([small, big], 1).astype(np.int64)
    grad = (rng.standard_normal((big.size, 2 * width)) * 0.5).astype(np.float32)
    vocab = (SMALL_V, V)
    live = (ids >= 0) & (ids < np.asarray(vocab)[None, :])
    touched = [np.unique(ids[live[:, f], f]) for f in range(2)]
    compact = np.full(ids.shape, -1, np.int64)
    for f in range(2):
        compact[live[:, f], f] = np.searchsorted(touched[f], ids[live[:, f], f])
    for a in (ids, grad, compact):
        a.setflags(write=False)
    return Case(name, ld, width, vocab, ids, grad, touched, compact)


def payload_of(c):
    """[B * 2] int64: local_row * F + slot of entry b * 2 + f, < 0 for a pruned id (an id == V is past the owner's rows: dropped by the key
    pass), and its gradient rows [B * 2, width]."""
    F = 2
    pay = np.where(c.ids >= 0, c.ids * F + np.arange(F)[None, :], -1).reshape(-1).astype(np.int64)
    return pay, c.grad.reshape(-1, c.width).copy()


def _f64(state):
    return [[np.asarray(a, np.float64).copy() for a in s] for s in state]


def ref_adagrad(c, w0, a0):
    """w0 / a0: per table the fp32 start values of its TOUCHED rows [len(touched_f), width] -> float64 (w, accum)."""
    w, a = _f64((w0, a0))
    R.sparse_adagrad_step(w, a, c.compact, c.grad, ADAGRAD_LR)
    return w, a


def ref_ftrl(c, w0, n0, z0):
    """width 1: slot f's gradient is column f of the case's gradient -> float64 (w, n, z)."""
    assert c.width == 1
    w, n, z = _f64((w0, n0, z0))
    R.sparse_ftrl_step(w, n, z, c.compact, c.grad, FTRL["lr"], FTRL["l1"], FTRL["l2"])
    return w, n, z


def lr_t_of(t=1):
    return ADAM["lr"] * np.sqrt(1 - ADAM["b2"] ** t) / (1 - ADAM["b1"] ** t)


def ref_adam(c, w0, m0, v0):
    """One step (t = 1) on zero m / v.  Rows outside the touched ones carry a zero gradient: the norms are the compacted copies'."""
    w, m, v = _f64((w0, m0, v0))
    R.sparse_adam_step(w, m, v, c.compact, c.grad, t=1, clip=CLIP, **ADAM)
    return w, m, v


def start_state(c, seed):
    """fp32 start values of the touched rows for the CPU checks: w in N(0, 0.1), n = 0.1, z in U(-0.2, 0.2)."""
    rng = np.random.default_rng(seed)
    w = [(rng.standard_normal((len(t), c.width)) * 0.1).astype(np.float32) for t in c.touched]
    a = [np.full((len(t), c.width), 0.1, np.float32) for t in c.touched]
    z = [rng.uniform(-0.2, 0.2, size=(len(t), c.width)).astype(np.float32) for t in c.touched]
    return w, a, z


# ---- 'div' routing over vocabularies on both sides of 2^31 and of 2^32 (tests/test_gpu_route_wide_vocab.py) -------------------------
ROUTE_VOCAB = (2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 + 5, 2 ** 40)
ROUTE_OWNERS = (1, 3, 8, 64)
ROUTE_PARTS = {3: (2, 3, 1, 3, 2, 3), 8: (3, 8, 1, 5, 8, 2), 64: (64, 33, 7, 64, 1, 50)}      # slices per table: fewer than P, so first != 0


def route_ids(parts, seed=0):
    """ids [n, F] over ROUTE_VOCAB for tables cut into parts[f] slices: 0, both sides of make_fielddiv's thr, the first and last row of
    every slice, V - 1, V and V + 2^32 (out of range), a pruned id, ids at and above 2^32 where the table has them, random ids to fill."""
    rng = np.random.default_rng(seed)
    cols = []
    for V, Pf in zip(ROUTE_VOCAB, parts):
        q, r = divmod(V, Pf)
        thr = r * (q + 1)
        col = [0, V - 1, V, V + 2 ** 32, -1, -5] + [x for x in (thr - 1, thr, thr + 1) if 0 <= x]
        for o in range(Pf):
            lo = o * (q + 1) if o < r else thr + (o - r) * q
            col += [lo, lo + (q if o < r else q - 1)]
        col += [x for x in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 4, 2 ** 32 + 123, 2 ** 39 + 1) if x < V]
        cols.append(col)
    n = max(len(c) for c in cols) + 5
    for V, col in zip(ROUTE_VOCAB, cols):
        col += [int(x) for x in rng.integers(0, V, size=n - len(col))]
    ids = np.asarray(cols, np.int64).T.copy()
    ids.setflags(write=False)
    return ids


def route_exact(ids, parts, first, P):
    """Owner rank and local row of ids [n, F] in Python's unbounded integers (-1, -1 for a pruned or out-of-range id)."""
    own, loc = np.full(ids.shape, -1, np.int64), np.full(ids.shape, -1, np.int64)
    for f, (V, Pf) in enumerate(zip(ROUTE_VOCAB, parts)):
        q, r = divmod(V, Pf)
        thr = r * (q + 1)
        for i, x in enumerate(ids[:, f].tolist()):
            if 0 <= x < V:
                o = x // (q + 1) if x < thr else r + (x - thr) // q
                start = o * (q + 1) if o < r else thr + (o - r) * q
                own[i, f], loc[i, f] = (o + first[f]) % P, x - start
    return own, loc
