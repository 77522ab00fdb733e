"""Inputs and float64 references of tests/test_gpu_sort_plans.py (host side, NumPy only): entry lists that take every consumer of the
in-tree radix sort (csrc/radix_sort.hip) -- the sorted scatter-sum and the payload and id forms of the sparse Adagrad, FTRL and Adam
steps -- through every digit plan of rs_layout, with the table edges, the dropped entries and the run lengths at which the wiring each
consumer redoes by hand can go wrong: the key width taken from total_rows / R, the input buffer chosen by pass parity, the workspace
carve and the table search from the key.

PLANS is the plan table (rule: sort_plan).  entries(total, n) builds one entry list over three tables; ids_entries(total, big) the same
pattern as ids [B, F] with B < 4096 (the plain sort, not the slot-major one).  The references run oracle.np_ref's float64 rules on a
compacted copy of the touched rows only (a table of 2^27 rows never exists on the host): ref_adagrad, ref_ftrl, ref_adam, ref_scatter.
emu_* are the fp32-faithful emulations (tests/hot_rows_inputs: adagrad_f32, ftrl_f32, adam_f32 on kahan_sum run sums); the CPU tests
hold them to ROOM of float64, so a GPU failure at BAR is the kernel's doing and not fp32's.  clip_case builds the inputs of the Adam
clip-norm range test (table gradient norms from 50 to 1e7, spread over the rows or concentrated in one hot row).

All are asserted on the emulation, never on the kernel."""
import collections
import functools

import numpy as np

from oracle import np_ref as R
from tests.hot_rows_inputs import BAR, ROOM, TILE, adagrad_f32, adam_f32, ftrl_f32, kahan_sum, scaled  # noqa: F401  (re-exported)

K = 4                                  # the 16-byte path
F = 3
SORT_TILE = 8192                       # entries per tile of the sort (RS_TILE)
SMALL, BIG = 300, 20000                # entries: inside one sort tile / three sort tiles
NS = (SMALL, BIG)
RUN_LOW, RUN_HIGH = 257, 3000          # the run on the lowest row of table 0 / on the highest row of table 2 (BIG only)
# The id forms: ids [B, F] with B < 4096 (at 4096 rows the slot-major sort takes over), every column filled to B.  A column must hold its
# table's run, so the small list has B = 300 (900 entries, one sort tile) and the large one B = 4095 (12 285 entries, two sort tiles).
IDS_B = {SMALL: 300, BIG: 4095}

# total_rows / R, key bits, digit bits, passes, the buffer the input pairs go to (sorted pairs always land in buffer 1)
PLANS = [(255, 8, 8, 1, 0), (256, 9, 9, 1, 0), (511, 9, 9, 1, 0), (512, 10, 8, 2, 1), (65535, 16, 8, 2, 1), (65536, 17, 9, 2, 1),
         ((1 << 18) - 1, 18, 9, 2, 1), (1 << 18, 19, 8, 3, 0), ((1 << 24) - 1, 24, 8, 3, 0), (1 << 24, 25, 9, 3, 0), (1 << 27, 28, 8, 4, 1)]
TOTALS = [p[0] for p in PLANS]


def sort_plan(total):
    """rs_layout's rule (csrc/radix_sort.hip) for keys 0 ... total (total = the key of a dropped entry) -> (bits, digit, passes, in)."""
    bits = 1
    while (1 << bits) <= total:
        bits += 1
    p8, p9 = (bits + 7) // 8, (bits + 8) // 9
    digit, passes = (9, p9) if p9 < p8 else (8, p8)
    return bits, digit, passes, 0 if passes & 1 else 1


def distinct_plan_totals():
    """One total per distinct (digit, passes) plan: the first of PLANS that has it."""
    seen, out = set(), []
    for total, _, digit, passes, _ in PLANS:
        if (digit, passes) not in seen:
            seen.add((digit, passes))
            out.append(total)
    return out


def vocab_of(total):
    """Three tables whose edges fall inside the key range: (7, total - 307, 300).  The two smallest totals (255, 256) have no room for a
    300-row last table: theirs has 100 rows, (7, total - 107, 100)."""
    last = 300 if total >= 511 else 100
    return (7, total - 7 - last, last)


Entries = collections.namedtuple("Entries", "total n vocab row_base slot row grad key live touched compact dropped_at_vocab negatives")


def _build(total, n, cap, seed, interleave):
    """The entry list: per entry its slot, its local row (-1 ... -9: a negative payload; == vocab_f: one past the table, dropped) and
    its gradient [K].  cap: at most this many entries per slot, every slot filled to exactly cap with negatives (the id form's columns);
    interleave: entry e belongs to slot e % F (ids [B, F] flattened), else the whole list is shuffled."""
    rng = np.random.default_rng(seed)
    vocab = vocab_of(total)
    assert sum(vocab) == total and min(vocab) >= 7
    big = n > SORT_TILE or (cap is not None and cap * F > SORT_TILE)
    per = [[], [], []]                                       # local rows per slot
    per[0] += [0] * RUN_LOW + [vocab[0] - 1]                 # the run on the lowest key of the sort; row 0 of table 0 is that run
    per[1] += [0, vocab[1] - 1]
    per[2] += [0] + ([vocab[2] - 1] * RUN_HIGH if big else [vocab[2] - 1])
    n_vocab = 6 if big else 2                                # row == vocab_f, per table: dropped, never row 0 of the next table
    for f in range(F):
        per[f] += [vocab[f]] * n_vocab
    fixed = sum(len(p) for p in per)
    min_neg = 13 if big else 5
    room = [(cap if cap is not None else n) - len(p) for p in per]
    left = n - fixed - min_neg
    assert left > 0 and min(room) >= 0
    fill = [0, 0, 0]
    fill[0] = min(room[0], left // 10, 150)
    fill[2] = min(room[2], left // 10, 400)
    fill[1] = min(room[1], left - fill[0] - fill[2])
    if big:
        # the run on the highest live key starts where all other live entries end: it must start mid-tile and end one entry past a
        # 256-entry tile edge
        others = lambda: fixed - F * n_vocab - RUN_HIGH + sum(fill)      # noqa: E731
        while (others() + RUN_HIGH) % TILE != 1:
            fill[1] -= 1
        assert fill[1] > 0 and others() % TILE != 0
    for f in range(F):
        per[f] += list(rng.integers(1, vocab[f] - 1, size=fill[f]))       # interior rows: the edge rows keep their single entries
    if cap is not None:
        for f in range(F):
            per[f] += list(-rng.integers(1, 10, size=cap - len(per[f])))
            assert len(per[f]) == cap
        cols = [np.asarray(p, np.int64)[rng.permutation(cap)] for p in per]
        if interleave:
            row = np.stack(cols, 1).reshape(-1)
            slot = np.tile(np.arange(F), cap)
        else:
            row, slot = np.concatenate(cols), np.repeat(np.arange(F), cap)
    else:
        negs = n - sum(len(p) for p in per)
        assert negs >= min_neg
        row = np.concatenate([np.asarray(p, np.int64) for p in per] + [-rng.integers(1, 10, size=negs)])
        slot = np.concatenate([np.full(len(p), f) for f, p in enumerate(per)] + [rng.integers(0, F, size=negs)])
        order = rng.permutation(row.size)
        row, slot = row[order], slot[order]
    assert row.size == (n if cap is None else cap * F)
    grad = (rng.standard_normal((row.size, K)) * 0.5).astype(np.float32)
    row_base = np.concatenate([[0], np.cumsum(vocab)[:-1]]).astype(np.int64)
    vf = np.asarray(vocab)[slot]
    live = (row >= 0) & (row < vf)
    key = np.where(live, row_base[slot] + row, total).astype(np.int64)
    touched = [np.unique(row[live & (slot == f)]) for f in range(F)]
    compact = np.full(row.size, -1, np.int64)                # the entry's row among its table's touched rows
    for f in range(F):
        sel = live & (slot == f)
        compact[sel] = np.searchsorted(touched[f], row[sel])
    for a in (slot, row, grad, key, live, compact):
        a.setflags(write=False)
    return Entries(total, row.size, vocab, row_base, slot, row, grad, key, live, touched, compact,
                   int((row == vf).sum()), int((row < 0).sum()))


@functools.lru_cache(maxsize=None)
def entries(total, n):
    """The payload form's list: n entries, shuffled."""
    return _build(total, n, None, 7 * total + n, False)


@functools.lru_cache(maxsize=None)
def ids_entries(total, n):
    """The id form's list for the case of n entries: ids [B, F] with B = IDS_B[n], entry e = b * F + f in slot f."""
    return _build(total, IDS_B[n] * F, IDS_B[n], 11 * total + n, True)


def payload_of(c):
    """[n] int64: local_row * F + slot; negative rows give negative words."""
    return np.where(c.row >= 0, c.row * F + c.slot, c.row).astype(np.int64)


def ids_of(c):
    """ids [B, F] int64 and grad [B, F * K] of an ids_entries list (a row == vocab_f is an id one past its table: pruned)."""
    return c.row.reshape(-1, F).copy(), c.grad.reshape(-1, F * K).copy()


def positions_of(c):
    """The scatter-sum's positions in [0, R), R = total: the same keys, the dropped entries as -1, R and R + 5 in turn."""
    drop = np.asarray([-1, c.total, c.total + 5], np.int64)[np.arange(c.n) % 3]
    return np.where(c.live, c.key, drop).astype(np.int64)


def run_report(c):
    """What the CPU test asserts of every list -> dict: the run lengths on the lowest row of table 0 and the highest of table 2, the
    sorted position where the latter starts, the singles on the edge rows, the dropped entries."""
    order = np.argsort(c.key, kind="stable")
    skey = c.key[order]
    hi_key = c.row_base[F - 1] + c.vocab[F - 1] - 1
    edge = {}
    for f in range(F):
        for r in (0, c.vocab[f] - 1):
            edge[(f, r)] = int((c.live & (c.slot == f) & (c.row == r)).sum())
    return dict(low_run=int((c.key == 0).sum()), high_run=int((c.key == hi_key).sum()), high_start=int(np.searchsorted(skey, hi_key)),
                high_end=int(np.searchsorted(skey, hi_key, side="right")), edge=edge, negatives=c.negatives,
                at_vocab=[int(((c.row == c.vocab[f]) & (c.slot == f)).sum()) for f in range(F)],
                dropped_key=int((c.key == c.total).sum()), live=int(c.live.sum()))


# ---- the float64 rules on the touched rows -----------------------------------------------------------------------------------------
def _compact_ids(c, width):
    """ids [n, F] (the entry's compacted row in its slot's column, -1 elsewhere) and grad [n, F * width] for oracle.np_ref."""
    ids = np.full((c.n, F), -1, np.int64)
    ids[np.arange(c.n), c.slot] = c.compact
    grad = np.zeros((c.n, F * width), np.float32)
    g = c.grad[:, :width]
    for f in range(F):
        sel = c.slot == f
        grad[sel, f * width:(f + 1) * width] = g[sel]
    return ids, grad


def _f64(state):
    return [[np.asarray(a, np.float64).copy() for a in s] for s in state]


ADAGRAD_LR = 0.05
FTRL = dict(lr=0.2, l1=0.01, l2=0.05)
ADAM = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-4)
CLIP = 100.0


def lr_t_of(t=1):
    return ADAM["lr"] * np.sqrt(1 - ADAM["b2"] ** t) / (1 - ADAM["b1"] ** t)


def ref_adagrad(c, w0, a0):
    """w0 / a0: per table the fp32 start values of its TOUCHED rows [len(touched_f), K] -> the float64 results (w, accum)."""
    w, a = _f64((w0, a0))
    ids, grad = _compact_ids(c, K)
    R.sparse_adagrad_step(w, a, ids, grad, ADAGRAD_LR)
    return w, a


def ref_ftrl(c, w0, n0, z0):
    """First-order rows (K = 1; the gradient is column 0 of the entry's gradient): per table [len(touched_f), 1] -> (w, n, z)."""
    w, n, z = _f64((w0, n0, z0))
    ids, grad = _compact_ids(c, 1)
    R.sparse_ftrl_step(w, n, z, ids, grad, FTRL["lr"], FTRL["l1"], FTRL["l2"])
    return w, n, z


def ref_adam(c, w0, m0, v0, clip=CLIP):
    """One step (t = 1).  Rows outside the touched ones carry a zero gradient, so the tables' norms are those of the compacted copies."""
    w, m, v = _f64((w0, m0, v0))
    ids, grad = _compact_ids(c, K)
    R.sparse_adam_step(w, m, v, ids, grad, t=1, clip=clip, **ADAM)
    return w, m, v


def ref_scatter(c):
    """float64 sums per touched position (sorted) -> (positions [T], sums [T, K], entries per position [T])."""
    pos, inv, counts = np.unique(c.key[c.live], return_inverse=True, return_counts=True)
    out = np.zeros((pos.size, K))
    np.add.at(out, inv, c.grad[c.live].astype(np.float64))
    return pos, out, counts


# ---- the fp32-faithful emulations --------------------------------------------------------------------------------------------------
def run_sums_f32(c, width=K):
    """Per table [len(touched_f), width] fp32: every row's entries summed as the kernels' run_sum does (the first entry as it is, the
    others Kahan-compensated), in entry order -- the order the stable sort leaves."""
    out = []
    for f in range(F):
        e = np.flatnonzero(c.live & (c.slot == f))
        e = e[np.argsort(c.compact[e], kind="stable")]
        cuts = np.flatnonzero(np.diff(c.compact[e])) + 1
        g = c.grad[:, :width]
        out.append(np.stack([kahan_sum(g[part]) for part in np.split(e, cuts)]) if e.size else np.zeros((0, width), np.float32))
    return out


def emu_adagrad(c, w0, a0):
    gs = run_sums_f32(c)
    res = [adagrad_f32(a0[f], w0[f], gs[f], ADAGRAD_LR) for f in range(F)]
    return [r[1] for r in res], [r[0] for r in res]


def emu_ftrl(c, w0, n0, z0):
    gs = run_sums_f32(c, 1)
    res = [ftrl_f32(n0[f], z0[f], w0[f], gs[f], FTRL["lr"], FTRL["l1"], FTRL["l2"]) for f in range(F)]
    return [r[2] for r in res], [r[0] for r in res], [r[1] for r in res]


def emu_adam(c, w0, m0, v0, clip=CLIP, gs=None):
    """adam_f32 on the run sums with the EXACT norm: the float64 norm of the float64 row sums."""
    gs = run_sums_f32(c) if gs is None else gs
    ids, grad = _compact_ids(c, K)
    w, m, v = [], [], []
    for f in range(F):
        g64, _ = R._dedup_sum(ids[:, f], grad[:, f * K:(f + 1) * K], len(c.touched[f]))
        den = max(float(np.sqrt((g64 ** 2).sum())), clip)
        m1, v1, w1 = adam_f32(m0[f], v0[f], w0[f], gs[f], den, lr_t_of(), ADAM["b1"], ADAM["b2"], ADAM["eps"], clip)
        w.append(w1), m.append(m1), v.append(v1)
    return w, m, v


def start_state(c, seed, width=K, n_init=0.1):
    """fp32 start values of the touched rows for the CPU checks (the GPU tests draw whole tables on the device and read the touched rows
    back): w in N(0, 0.1), the accumulator n_init, z in U(-0.2, 0.2)."""
    rng = np.random.default_rng(seed)
    w = [(rng.standard_normal((len(t), width)) * 0.1).astype(np.float32) for t in c.touched]
    a = [np.full((len(t), width), n_init, np.float32) for t in c.touched]
    z = [rng.uniform(-0.2, 0.2, size=(len(t), width)).astype(np.float32) for t in c.touched]
    return w, a, z


def worst(got, ref):
    """The largest scaled error over the tables of every state tensor: got / ref are tuples (state) of lists (table)."""
    return max(scaled(g, r) for gs, rs in zip(got, ref) for g, r in zip(gs, rs))


# ---- the Adam clip norm across its range ----------------------------------------------------------------------------------------
CLIP_K = 16
CLIP_VOCAB = (50, 7, 3000)
CLIP_B = 4000                          # < 4096: the plain sort
CLIP_NORMS = (50.0, 150.0, 6.0e4, 7.0e4, 3.0e5, 1.0e7)
CLIP_SHAPES = ("spread", "concentrated")
CLIP_HOT = 3000                        # entries of the hot row (the last row of table 2)


@functools.lru_cache(maxsize=None)
def clip_case(norm, shape):
    """ids [B, 3], grad [B, 3 * 16] whose summed gradient has norm `norm` (to fp32 rounding of the entries) in EVERY table.  "spread":
    uniform ids, no row holds more than a small share of its table's ||g||^2 (table 1 has 7 rows: a seventh or so each);
    "concentrated": 3000 entries of table 2 name its last row and their sum carries over 99 % of that table's ||g||^2.
    -> Entries (the id form: entry b * F + f in slot f, K = 16), ids, grad, the tables' float64 ||g||^2 and the hot row's share."""
    rng = np.random.default_rng(int(norm) * 2 + (shape == "concentrated"))
    B, Kc = CLIP_B, CLIP_K
    ids = np.stack([rng.integers(-1, v, size=B) for v in CLIP_VOCAB], 1).astype(np.int64)
    g = rng.standard_normal((B, F, Kc))
    hot = CLIP_VOCAB[2] - 1
    if shape == "concentrated":
        ids[ids[:, 2] == hot, 2] = -1
        at = rng.permutation(B)[:CLIP_HOT]
        ids[at, 2] = hot
        g[at, 2] = rng.standard_normal(Kc) * 3.0 + rng.standard_normal((CLIP_HOT, Kc)) * 0.3      # a common direction: the sum grows with the count
    share = 0.0
    for f, v in enumerate(CLIP_VOCAB):
        gs, _ = R._dedup_sum(ids[:, f], g[:, f], v)
        g[:, f] *= norm / np.sqrt((gs ** 2).sum())
    grad = g.reshape(B, F * Kc).astype(np.float32)
    norm2 = []
    for f, v in enumerate(CLIP_VOCAB):
        gs, _ = R._dedup_sum(ids[:, f], grad[:, f * Kc:(f + 1) * Kc], v)
        norm2.append(float((gs ** 2).sum()))
        if f == 2:
            share = float((gs[hot] ** 2).sum()) / norm2[-1]
            top = float((gs ** 2).sum(1).max()) / norm2[-1]
    for a in (ids, grad):
        a.setflags(write=False)
    return dict(ids=ids, grad=grad, norm2=norm2, hot_share=share, top_share=top)


def clip_start(norm, shape):
    rng = np.random.default_rng(31 + int(norm))
    w0 = [(rng.standard_normal((v, CLIP_K)) * 0.1).astype(np.float32) for v in CLIP_VOCAB]
    return w0, [np.zeros_like(w) for w in w0], [np.zeros_like(w) for w in w0]


@functools.lru_cache(maxsize=None)
def clip_ref(norm, shape):
    """One oracle.np_ref.sparse_adam_step (t = 1, clip 100) on zero m / v -> float64 (w, m, v), whole tables."""
    c = clip_case(norm, shape)
    w, m, v = _f64(clip_start(norm, shape))
    R.sparse_adam_step(w, m, v, c["ids"], c["grad"], t=1, clip=CLIP, **ADAM)
    return w, m, v


def clip_payload(norm, shape):
    """The same entries as the owner of ALL rows receives them (world 1): payload [B * F] = id * F + slot (-1: pruned), grad [B * F, K]."""
    c = clip_case(norm, shape)
    ids = c["ids"]
    pay = np.where(ids >= 0, ids * F + np.arange(F)[None, :], -1).reshape(-1).astype(np.int64)
    return pay, c["grad"].reshape(-1, CLIP_K).copy()


def clip_emu(norm, shape):
    """adam_f32 on kahan_sum run sums with the exact norm -> fp32 (w, m, v), whole tables."""
    c = clip_case(norm, shape)
    w0, m0, v0 = clip_start(norm, shape)
    out = ([], [], [])
    for f, vsz in enumerate(CLIP_VOCAB):
        gf = c["grad"][:, f * CLIP_K:(f + 1) * CLIP_K]
        gs = np.zeros((vsz, CLIP_K), np.float32)
        idf = c["ids"][:, f]
        for r in np.unique(idf[idf >= 0]):
            gs[r] = kahan_sum(gf[idf == r])
        den = max(float(np.sqrt(c["norm2"][f])), CLIP)
        m1, v1, w1 = adam_f32(m0[f], v0[f], w0[f], gs, den, lr_t_of(), ADAM["b1"], ADAM["b2"], ADAM["eps"], CLIP)
        out[0].append(w1), out[1].append(m1), out[2].append(v1)
    return out


# ---- the dense Adagrad multi-launch ----------------------------------------------------------------------------------------------
DENSE_SIZES = (1, 255, 256, 257, 100003)
DENSE_GROUPS = (1, 16, 17, 33)
DENSE_BAR = 2e-6                       # the bar of test_dense_adagrad_step_matches_torch_adagrad


def dense_sizes(n_vars):
    """Sizes of a group's variables from DENSE_SIZES: every chunk of 16 holds the largest size, never as its first variable (a group of one
    variable, and a last chunk of one, cannot but lead with it: theirs is 257, more than one workgroup)."""
    rng = np.random.default_rng(n_vars)
    sizes = []
    for v0 in range(0, n_vars, 16):
        nv = min(16, n_vars - v0)
        if nv == 1:
            sizes.append(257)
            continue
        s = [int(x) for x in rng.choice(DENSE_SIZES[:4], size=nv)]
        s[int(rng.integers(1, nv))] = DENSE_SIZES[4]
        sizes += s
    return sizes


def dense_ref(w, acc, grads, lr, eps):
    """float64 Adagrad: acc += g^2; w -= lr * g / (sqrt(acc) + eps), one step per entry of grads."""
    w, acc = np.asarray(w, np.float64).copy(), np.asarray(acc, np.float64).copy()
    lr, eps = float(np.float32(lr)), float(np.float32(eps))
    for g in grads:
        g = np.asarray(g, np.float64)
        acc += g * g
        w -= lr * g / (np.sqrt(acc) + eps)
    return w, acc
