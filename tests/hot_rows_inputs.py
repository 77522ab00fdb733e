"""Inputs of tests/test_gpu_hot_rows.py (host side, NumPy only): batches in which one row of one slot collects hundreds or thousands of
entries of a single step, the optimiser state that makes the update cancel, the fp32 emulations of the per-row rules (csrc/backward.hip:
FtrlUpd::one, AdagradUpd::apply, AdamUpd::one) and the two conditions every committed seed must meet:

  (a) the emulation fed the CORRECTLY ROUNDED run sum np.float32(float64 sum) is within 4e-6 of the float64 rule on every state value
      (measure |got - ref| / (1 + |ref|)): the 1e-5 bar of the GPU tests has 2x room over what fp32 itself costs on these inputs;
  (b) for the FTRL cases of >= 3000 hits, the same emulation fed a run sum formed the old way misses 1e-5 on z by >= 2x, so the inputs
      tell that sum from a compensated one.  The old ways, in batch order (the order the stable sort leaves: csrc/radix_sort.hip):
        seq    one sequential fp32 sum over the whole run;
        tiles  what the kernels did before the compensation: the sorted entries are cut into tiles of 256 from entry 0 of the sort (the
               run starts wherever the smaller keys end), a sequential fp32 sum per tile, the tile partials added in fp32 in tile order;
        fix    (the case of 20 000 hits, 79 tiles) Kahan-compensated tile sums, as run_sum forms them, with the partials still added
               plainly in fp32: adagrad_tile_k's half of the change without adagrad_fix_k's.
      FTRL_PICKS names, per case and K, the seed and the ways it is picked for; with K = 4 a way is met by at least one column, and
      ftrl_case reports which (the GPU test prints them).  `fix` is held to 1e-5 + 4e-6 -- the bar plus all the room of (a).  The
      single-GPU sort is deterministic, so `tiles` predicts what a kernel with plain sums reads and `fix` what one with plain adds in
      adagrad_fix_k reads.

All are asserted on the emulation, never on the kernel."""
import collections
import functools

import numpy as np

from oracle import np_ref as R

VOCAB = (50, 7, 5000)                  # slot 0 holds the lowest keys, slot 2 the highest; the 7-row slot is all long runs
F = len(VOCAB)
BAR, ROOM = 1e-5, 4e-6

# n: hits of the hot row; pos: "low" = the lowest key of the sort (slot 0, id 0: its run starts at a tile start), "high" = the highest live
# key (slot 2, id 4999: its run starts mid-tile); n2 > 0: the next row of the same slot is hot too (an open-left and an open-right run in
# one tile); sigma: spread of the hot entries' gradients.  B = 4000 takes the plain sort, B = 32 768 the slot-major one.  The seeds of the
# cases of >= 3000 hits are picked for condition (b): at 3000 hits about every second seed qualifies, at 20 000 nearly all do.
Case = collections.namedtuple("Case", "n B pos seed sigma n2 tag", defaults=(0, ""))
TILE = 256
CASES = [Case(140, 4000, "low", 1, 0.5), Case(255, 4000, "low", 2, 0.5), Case(255, 4000, "high", 3, 0.5), Case(256, 4000, "low", 4, 0.5),
         Case(256, 4000, "high", 5, 0.5), Case(257, 4000, "low", 6, 0.5), Case(257, 4000, "high", 7, 0.5), Case(513, 4000, "low", 8, 0.5),
         Case(513, 4000, "high", 9, 0.5), Case(700, 4000, "high", 10, 0.5), Case(3000, 4000, "low", 16, 0.5),
         Case(3000, 4000, "high", 19, 0.5), Case(20000, 32768, "low", 12, 0.1), Case(300, 4000, "low", 14, 0.5, 400),
         Case(20000, 32768, "low", 12, 0.1, 0, "fix")]
SUBSET = [c for c in CASES if c.n in (257, 700, 3000, 20000) and c.pos == ("low" if c.n in (257, 3000, 20000) else "high") and not c.tag]


# The FTRL tests' cases of >= 3000 hits, per (hits, position, tag, K): the seed of the batch and the old ways of summing that condition (b)
# demands of it (the Adagrad and Adam tests draw from the case's own seed).  Picked by search: `seq` holds for every second seed at 3000
# hits and nearly all at 20 000; `tiles` reaches 2e-5 for one seed in a hundred or more (the tiles keep every plain sum short); `fix` -- 78
# fp32 adds of partials, each off by at most 1.9e-6 while the sum is in 32 ... 64, some 6e-6 in all -- reached 1.9e-5 at best in 1200 seeds,
# so it gets a case of its own (tag "fix") and the margin BAR + ROOM: the emulation repeats the kernel's sum bit for bit, and ROOM is all
# that the rest of the rule's fp32 arithmetic can give back.
FTRL_PICKS = {(3000, "low", "", 1): (356, ("seq", "tiles")), (3000, "low", "", 4): (3, ("seq", "tiles")),
              (3000, "high", "", 1): (19, ("seq",)), (3000, "high", "", 4): (47, ("seq", "tiles")),
              (20000, "low", "", 1): (697, ("seq", "tiles")), (20000, "low", "", 4): (429, ("seq", "tiles")),
              (20000, "low", "fix", 1): (615, ("seq", "fix")), (20000, "low", "fix", 4): (3, ("seq", "fix"))}
MARGIN = {"seq": 2 * BAR, "tiles": 2 * BAR, "fix": BAR + ROOM}


def case_id(c):
    return "%d%s-%s-B%d%s" % (c.n, "+%d" % c.n2 if c.n2 else "", c.pos, c.B, "-" + c.tag if c.tag else "")


def scaled(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max()) if got.size else 0.0


@functools.lru_cache(maxsize=None)
def batch(case, K, shared):
    """-> ids [B, F] int64 (uniform, -1 = pruned mixed in, the hot rows planted), grad [B, K] (shared by the slots) or [B, F*K] fp32, the hot
    slot, the hot ids and per hot id its batch positions and float64 column sums S (30 <= |S| <= 60 by a small drift of the entries)."""
    rng = np.random.default_rng(1000 * FTRL_PICKS.get((case.n, case.pos, case.tag, K), (case.seed,))[0] + K)
    B = case.B
    ids = np.stack([rng.integers(-1, v, size=B) for v in VOCAB], 1).astype(np.int64)
    f, hid = (0, 0) if case.pos == "low" else (F - 1, VOCAB[F - 1] - 1 - (1 if case.n2 else 0))
    grad = (rng.standard_normal((B, K if shared else F * K)) * 0.5).astype(np.float32)
    cols = slice(0, K) if shared else slice(f * K, (f + 1) * K)
    perm = rng.permutation(B)
    hot, at = [], 0
    for j, n in enumerate([case.n] + ([case.n2] if case.n2 else [])):
        ids[ids[:, f] == hid + j, f] = -1                  # exactly n hits: chance hits of the uniform draw are pruned
    for j, n in enumerate([case.n] + ([case.n2] if case.n2 else [])):
        pos = np.sort(perm[at:at + n])
        at += n
        ids[pos, f] = hid + j
        g = rng.standard_normal((n, K)) * case.sigma
        target = rng.uniform(35.0, 55.0, size=K) * rng.choice([-1.0, 1.0], size=K)
        grad[pos, cols] = (g + (target - g.sum(0)) / n).astype(np.float32)
        hot.append((hid + j, pos))
    sums = [grad[pos, cols].astype(np.float64).sum(0) for _, pos in hot]
    for (i, _), S in zip(hot, sums):
        assert int((ids[:, f] == i).sum()) in (case.n, case.n2) and (np.abs(S) >= 30).all() and (np.abs(S) <= 60).all(), (case, S)
    for a in (ids, grad):
        a.setflags(write=False)
    return ids, grad, f, hot, sums


def run_sums(ids, grad, K):
    """Per slot: the float64 sum of every row's gradients and the rows touched."""
    out = []
    for f, v in enumerate(VOCAB):
        gf = grad if grad.shape[1] == K else grad[:, f * K:(f + 1) * K]
        out.append(R._dedup_sum(ids[:, f], gf, v))
    return out


def plain_sum(grad_rows):
    """The sequential fp32 sum of the rows in the order given (np.cumsum adds one after the other)."""
    return np.cumsum(grad_rows.astype(np.float32), axis=0, dtype=np.float32)[-1]


def run_start(ids, f, hid):
    """Where the run of (slot f, id hid) starts among the sorted entries: the live entries with a smaller key (pruned ids sort last)."""
    return sum(int((ids[:, s] >= 0).sum()) for s in range(f)) + int(((ids[:, f] >= 0) & (ids[:, f] < hid)).sum())


def kahan_sum(rows):
    """run_sum of csrc/backward.hip over rows [n, K] fp32: the first entry as it is, the others Kahan-compensated."""
    acc = rows[0].copy()
    comp = np.zeros_like(acc)
    for x in rows[1:]:
        y = x - comp
        t = acc + y
        comp = (t - acc) - y
        acc = t
    return acc


def tiled_sum(rows, start, inner):
    """The run's sum as the tile pass and the fix pass form it: pieces cut where the sorted position (start + i) crosses a multiple of
    TILE, each piece summed by `inner` (plain_sum or kahan_sum), the pieces added in fp32 in order."""
    rows = rows.astype(np.float32)
    cuts = [0] + list(range(TILE - start % TILE, len(rows), TILE)) + [len(rows)]
    parts = np.stack([inner(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a])
    return np.cumsum(parts, axis=0, dtype=np.float32)[-1]


f32 = np.float32


def ftrl_f32(n, z, w, g, lr, l1, l2):
    """FtrlUpd::one in fp32, elementwise."""
    lr, l1, l2 = f32(lr), f32(l1), f32(l2)
    n_new = n + g * g
    sigma = (np.sqrt(n_new) - np.sqrt(n)) / lr
    z_new = (z + g) - sigma * w
    quad = np.sqrt(n_new) / lr + f32(2) * l2
    w_new = np.where(np.abs(z_new) > l1, (np.sign(z_new) * l1 - z_new) / quad, f32(0)).astype(np.float32)
    return n_new, z_new, w_new


def adagrad_f32(acc, w, g, lr):
    acc = acc + g * g
    return acc, w - (f32(lr) * g) / np.sqrt(acc)


def adam_f32(m, v, w, g, den, lr_t, b1, b2, eps, clip):
    lr_t, b1, b2, eps, clip = f32(lr_t), f32(b1), f32(b2), f32(eps), f32(clip)
    if clip > 0:
        g = (g * clip) / f32(den)
    m = m * b1 + g * (f32(1) - b1)
    v = v * b2 + (g * g) * (f32(1) - b2)
    return m, v, w - (lr_t * m) / (np.sqrt(v) + eps)


# ---- FTRL ---------------------------------------------------------------------------------------------------------------------------
FTRL_LR = 0.2


@functools.lru_cache(maxsize=None)
def ftrl_case(case, K, l1, l2):
    """-> dict: the batch, the fp32 start state (w, n, z per slot, [V, K]; the hot rows' set so that z + S cancels: n = 0.1 + S^2,
    z = -fp32(S) + u, u in U(-0.2, 0.2), w in N(0, 0.01)) and the float64 result of one oracle.np_ref.sparse_ftrl_step.  Conditions (a) and
    (b) are asserted here."""
    ids, grad, f, hot, sums = batch(case, K, K == 1)
    rng = np.random.default_rng(77 + case.seed)
    w0 = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in VOCAB]
    n0 = [np.full((v, K), 0.1, np.float32) for v in VOCAB]
    z0 = [np.zeros((v, K), np.float32) for v in VOCAB]
    for (i, _), S in zip(hot, sums):
        n0[f][i] = (0.1 + S * S).astype(np.float32)
        z0[f][i] = (-S.astype(np.float32).astype(np.float64) + rng.uniform(-0.2, 0.2, size=K)).astype(np.float32)
        w0[f][i] = (rng.standard_normal(K) * 0.01).astype(np.float32)
    ref = [[a.astype(np.float64) for a in s] for s in (w0, n0, z0)]
    R.sparse_ftrl_step(ref[0], ref[1], ref[2], ids, grad, FTRL_LR, l1, l2)
    gs = run_sums(ids, grad, K)
    room = 0.0
    for s in range(F):
        g32, t = gs[s][0].astype(np.float32), gs[s][1]
        n1, z1, w1 = ftrl_f32(n0[s][t], z0[s][t], w0[s][t], g32[t], FTRL_LR, l1, l2)
        room = max(room, scaled(w1, ref[0][s][t]), scaled(n1, ref[1][s][t]), scaled(z1, ref[2][s][t]))
    assert room <= ROOM, "(a) fp32 on the correctly rounded sums is %.2e off float64: the inputs leave no room under 1e-5" % room
    teeth = ftrl_teeth(case, K, l1, l2, ids, grad, f, hot, n0, z0, w0, ref) if case.n >= 3000 else None
    return dict(ids=ids, grad=grad, w0=w0, n0=n0, z0=z0, ref=ref, room=room, teeth=teeth, hot_slot=f, hot=hot)


def ftrl_teeth(case, K, l1, l2, ids, grad, f, hot, n0, z0, w0, ref, check=True):
    """Condition (b): per old way of summing, the hot row's z error per column -> {name: (worst, the columns at or above MARGIN[name])};
    the ways FTRL_PICKS names for the case must each have such a column."""
    want = FTRL_PICKS[(case.n, case.pos, case.tag, K)][1] if check else ()
    i, pos = hot[0]
    cols = slice(0, K) if grad.shape[1] == K else slice(f * K, (f + 1) * K)
    rows, start = grad[pos, cols], run_start(ids, f, i)
    ways = {"seq": plain_sum(rows), "tiles": tiled_sum(rows, start, plain_sum)}
    if case.n >= 20000:
        ways["fix"] = tiled_sum(rows, start, kahan_sum)
    out = {}
    for name, g in ways.items():
        _, z1, _ = ftrl_f32(n0[f][i], z0[f][i], w0[f][i], g, FTRL_LR, l1, l2)
        err = np.abs(z1.astype(np.float64) - ref[2][f][i]) / (1.0 + np.abs(ref[2][f][i]))
        out[name] = (float(err.max()), [int(c) for c in np.nonzero(err >= MARGIN[name])[0]])
        assert out[name][1] or name not in want, "(b) the run sum formed the '%s' way leaves z only %.2e off: this seed would not notice it" % (
            name, out[name][0])
    return out


# ---- Adagrad ------------------------------------------------------------------------------------------------------------------------
ADAGRAD_LR = 0.05


def adagrad_check(ids, grad, K, w0, a0, ref_w, ref_a):
    """Condition (a) for one Adagrad step."""
    gs = run_sums(ids, grad, K)
    room = 0.0
    for s in range(F):
        g32, t = gs[s][0].astype(np.float32), gs[s][1]
        a1, w1 = adagrad_f32(a0[s][t], w0[s][t], g32[t], ADAGRAD_LR)
        room = max(room, scaled(w1, ref_w[s][t]), scaled(a1, ref_a[s][t]))
    assert room <= ROOM, "(a) fp32 on the correctly rounded sums is %.2e off float64" % room
    return room


@functools.lru_cache(maxsize=None)
def adagrad_case(case, K, big_prior):
    """big_prior: the hot rows start from an accumulator of 1e4 instead of 0.1."""
    ids, grad, f, hot, sums = batch(case, K, False)
    rng = np.random.default_rng(177 + case.seed)
    w0 = [(rng.standard_normal((v, K)) * 0.25).astype(np.float32) for v in VOCAB]
    a0 = [np.full((v, K), 0.1, np.float32) for v in VOCAB]
    if big_prior:
        for i, _ in hot:
            a0[f][i] = 1e4
    ref_w, ref_a = [a.astype(np.float64) for a in w0], [a.astype(np.float64) for a in a0]
    R.sparse_adagrad_step(ref_w, ref_a, ids, grad, ADAGRAD_LR)
    room = adagrad_check(ids, grad, K, w0, a0, ref_w, ref_a)
    return dict(ids=ids, grad=grad, w0=w0, a0=a0, ref_w=ref_w, ref_a=ref_a, room=room, hot_slot=f, hot=hot)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
ADAM = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-4)


@functools.lru_cache(maxsize=None)
def adam_case(case, K, clip, big_prior):
    """One tf.train.AdamOptimizer step (t = 1) on zero m / v; big_prior: the hot rows start from v = 50, m = 2."""
    ids, grad, f, hot, sums = batch(case, K, False)
    rng = np.random.default_rng(277 + case.seed)
    w0 = [(rng.standard_normal((v, K)) * 0.1).astype(np.float32) for v in VOCAB]
    m0 = [np.zeros((v, K), np.float32) for v in VOCAB]
    v0 = [np.zeros((v, K), np.float32) for v in VOCAB]
    if big_prior:
        for i, _ in hot:
            m0[f][i], v0[f][i] = 2.0, 50.0
    ref = [[a.astype(np.float64) for a in s] for s in (w0, m0, v0)]
    R.sparse_adam_step(ref[0], ref[1], ref[2], ids, grad, t=1, clip=clip, **ADAM)
    lr_t = ADAM["lr"] * np.sqrt(1 - ADAM["b2"]) / (1 - ADAM["b1"])
    gs = run_sums(ids, grad, K)
    room = 0.0
    for s in range(F):
        g32 = gs[s][0].astype(np.float32)                  # rows never looked up: a zero gradient (every row of m, v and var moves)
        den = max(float(np.sqrt((g32.astype(np.float64) ** 2).sum())), clip)
        m1, v1, w1 = adam_f32(m0[s], v0[s], w0[s], g32, den, lr_t, ADAM["b1"], ADAM["b2"], ADAM["eps"], clip)
        room = max(room, scaled(w1, ref[0][s]), scaled(m1, ref[1][s]), scaled(v1, ref[2][s]))
    assert room <= ROOM, "(a) fp32 on the correctly rounded sums is %.2e off float64" % room
    return dict(ids=ids, grad=grad, w0=w0, m0=m0, v0=v0, ref=ref, lr_t=lr_t, room=room)
