"""Inputs of the packed DIN unit's edge tests in tests/test_gpu_din_pack.py (host side, NumPy only): named cases for din_pack_k
(csrc/din_pack.hip) and a plain restatement of the host-side geometry that decides which code a case reaches -- the chunk size and count of
the partition's first level, the waves of the launch, each wave's sample range, its blocks of up to 16 samples, their passes of 32 rows.
The restatement is written from the kernel's text and imports nothing from the library; tests/test_din_pack_inputs.py uses it to prove
that every case reaches the edge it is named for, and holds every case to the conditioning check (fp32 NumPy within a tenth of the GPU
bar of float64) that keeps the 1e-5 bar a statement about the kernel.

What the geometry says about small batches (and the cases follow it): the launch has about one wave per TWO samples (G = 8 ceil(ceil(B / 2)
/ 8) up to 2048), each taking an equal share of the weight sum_b (len_b + 5).  A wave therefore holds a block of 16 samples only when 16
samples together weigh no more than about W / G, i.e. when a few samples of the batch are much longer than the rest.  At (B = 40, T = 20)
and (B = 3, T = 20) no wave can hold more than three samples (W / G <= 1000 / 24), so the `no_candidate` and `lengths_out_of_range`
cases each come in the small form and in a DENSE form, with a larger T and a few full-length samples at the batch's end that soak up most
waves, in which wave 0 walks whole 16-sample blocks.  For the same reason a block of `long_history` is one sample (T = 65 535 rows, 2048
passes): the 2^15 passes of a block of 16 such samples would need 16 of them to weigh one wave's share, which no batch reaches (G grows
with B).  What T = 65 535 does exercise is the top bit of the 16-bit position field and the 32-bit row offsets of a 2048-pass block; the
forms beyond it (T = 65 536 and T = 2^20, on the kernel's instantiations with a 20-bit field) reach a block of 2^15 passes with one sample."""
import collections
import functools

import numpy as np

K, V = 64, 3000
BAR = 1e-5
ROOM = BAR / 10                  # what fp32 itself may cost on a case's operands
ACTIVATIONS = ("sigmoid", "prelu", "dice")

# ---- the host-side geometry of csrc/din_pack.hip, restated ------------------------------------------------------------------------------
CUS, WAVES, BLK, PASS, W0 = 256, 8, 16, 32, 5          # kCUs, DP_WAVES, DP_BLK, rows of a pass (two 16-row tiles), launch_din_pack's w0
MAX_CHUNKS, MAX_T, MAX_T_WIDE = 1024, 65535, 1 << 20


def covers(Kk, T, H1, H2):
    """din_pack_covers."""
    return Kk == 64 and 1 <= T <= MAX_T and 0 < H1 <= 80 and 0 < H2 <= 48 and H1 % 4 == 0 and H2 % 4 == 0


def long_covers(Kk, T, H1, H2):
    """din_pack_long_covers: the histories beyond the 16-bit position field, on the instantiations with a field of 20 bits."""
    return MAX_T < T <= MAX_T_WIDE and covers(Kk, 1, H1, H2)


def chunks(B):
    """din_pack_chunks: -> (samples per chunk, chunks): 64 per chunk while that needs at most 1024 chunks, doubled until it does."""
    chunk = 64
    while (B + chunk - 1) // chunk > MAX_CHUNKS:
        chunk *= 2
    return chunk, max(1, (B + chunk - 1) // chunk)


def launch(B):
    """launch_din_pack: -> (workgroups, waves): a wave per two samples, eight waves per workgroup, one workgroup per CU at most."""
    nwg = min(CUS, max(1, ((B + 1) // 2 + WAVES - 1) // WAVES))
    return nwg, nwg * WAVES


def clamped(hist_len, T, B):
    """A sample's rows: its length held to [0, T] (len_of, block_len_of, din_pack_sums_k); no vector: T."""
    if hist_len is None:
        return np.full(B, T, np.int64)
    return np.clip(np.asarray(hist_len, np.int64), 0, T)


def partition(hist_len, T, B):
    """-> [(s_lo, s_hi)] per wave: wave g of G takes the samples whose exclusive weight prefix P(b) lies in [ceil(g W / G), ceil((g + 1) W /
    G)) -- first_at: the least b with P(b) >= t, B when there is none; the last wave ends at B."""
    wgt = clamped(hist_len, T, B) + W0
    P = np.concatenate([[0], np.cumsum(wgt)[:-1]])
    W = int(wgt.sum())
    G = launch(B)[1]
    first_at = lambda t: int(np.searchsorted(P, t, side="left"))      # noqa: E731
    out = []
    for g in range(G):
        lo = first_at((g * W + G - 1) // G)
        hi = B if g + 1 == G else first_at(((g + 1) * W + G - 1) // G)
        out.append((lo, hi))
    return out


Block = collections.namedtuple("Block", "wave sb ns lens rows passes")


def blocks(hist_len, T, B):
    """Every block the launch computes: consecutive runs of up to 16 samples from the wave's first one; rows = the samples' clamped lengths
    end to end, passes = ceil(rows / 32), one (without rows) for a block of empty samples."""
    lens = clamped(hist_len, T, B)
    out = []
    for g, (lo, hi) in enumerate(partition(hist_len, T, B)):
        for sb in range(lo, hi, BLK):
            ns = min(BLK, hi - sb)
            R = int(lens[sb:sb + ns].sum())
            out.append(Block(g, sb, ns, lens[sb:sb + ns].copy(), R, (R + PASS - 1) // PASS if R else 1))
    return out


def block_rows(blk):
    """-> (sample, position) of the block's rows in order: row q is row q % 32 of pass q // 32."""
    s = np.repeat(np.arange(blk.ns), blk.lens)
    ends = np.cumsum(blk.lens)
    p = np.arange(blk.rows) - np.repeat(ends - blk.lens, blk.lens)
    return blk.sb + s, p


def pass_rows(hist_len, T, B):
    """The row count of every pass of the launch (a block without rows: one pass of 0)."""
    out = []
    for blk in blocks(hist_len, T, B):
        out += [min(PASS, blk.rows - PASS * i) if blk.rows else 0 for i in range(blk.passes)]
    return out


def boundaries_in_second_half_of_a_chunk(hist_len, T, B):
    """Wave ranges that start at a sample beyond the first 64 of its chunk: first_at reaches it on a later trip, with a live carry."""
    chunk = chunks(B)[0]
    return [lo for lo, hi in partition(hist_len, T, B) if lo < B and lo % chunk >= 64]


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name table hist hist_plain hist_len cand unit act_params T H1 H2 combos")
# hist_len: None = the call passes no length vector (the references take T).  combos: the (activation, normalize) pairs the case runs for.
# hist_plain: the ids of the runs with normalize = False -- hist with all but PLAIN_KEEP valid positions per sample masked (id -1; the first
# and the last valid position stay).  A masked position inside the length is still a row of the block, so the geometry is the same; but
# the plain sum over a sample's rows is the one quantity whose fp32 cost grows with the row count (the softmax output is a convex
# combination), and at the weight scales of the existing tests 50 valid rows leave fp32 itself up to 1.9e-6 off float64, 8 up to 1.2e-6,
# 6 under 1e-6 on every case (the PReLU / Dice scores alone cost fp32 up to 9e-7 at H1 = 80).
PLAIN_KEEP = 6
ALL = tuple((a, n) for a in ACTIVATIONS for n in (False, True))
PAPER = tuple((a, n) for a in ("prelu", "dice") for n in (False, True))


def unit_weights(rng, H1, H2):
    """tests/test_gpu_din_model.py: _unit_case's scales."""
    W1 = (rng.standard_normal((4 * K, H1)) * 0.08).astype(np.float32)
    b1 = (rng.standard_normal(H1) * 0.1).astype(np.float32)
    W2 = (rng.standard_normal((H1, H2)) * 0.2).astype(np.float32)
    b2 = (rng.standard_normal(H2) * 0.1).astype(np.float32)
    W3 = (rng.standard_normal(H2) * 0.3).astype(np.float32)
    return W1, b1, W2, b2, W3, np.array([0.05], np.float32)


def unit_act_params(rng, H1, H2):
    """alpha in [-0.2, 0.6) (negative values included), Dice scale in [0.3, 3), shift ~ N(0, 0.5), per layer."""
    return np.concatenate([rng.uniform(-0.2, 0.6, H1), rng.uniform(0.3, 3.0, H1), rng.standard_normal(H1) * 0.5,
                           rng.uniform(-0.2, 0.6, H2), rng.uniform(0.3, 3.0, H2), rng.standard_normal(H2) * 0.5]).astype(np.float32)


def thinned(rng, hist, hist_len, keep):
    """hist with at most `keep` valid positions per sample: the first and the last valid one and a random choice of the others."""
    B, T = hist.shape
    lens = clamped(hist_len, T, B)
    valid = (np.arange(T)[None, :] < lens[:, None]) & (hist >= 0)
    out = hist.copy()
    for b in np.flatnonzero(valid.sum(1) > keep):
        idx = np.flatnonzero(valid[b])
        stay = np.concatenate([idx[[0, -1]], rng.choice(idx[1:-1], size=keep - 2, replace=False)])
        out[b, np.setdiff1d(idx, stay)] = -1
    return out


def _case(name, rng, hist, hist_len, cand, H1=80, H2=40, combos=ALL, keep=PLAIN_KEEP):
    table = (rng.standard_normal((V, K)) * 0.3).astype(np.float32)
    unit, ap = unit_weights(rng, H1, H2), unit_act_params(rng, H1, H2)
    hist = np.ascontiguousarray(hist, np.int64)
    plain = thinned(rng, hist, hist_len, keep) if keep else hist
    cand = np.ascontiguousarray(cand, np.int64)
    hist_len = None if hist_len is None else np.ascontiguousarray(hist_len, np.int32)
    for a in (table, hist, plain, cand, ap) + unit + (() if hist_len is None else (hist_len,)):
        a.setflags(write=False)
    return Case(name, table, hist, plain, hist_len, cand, unit, ap, hist.shape[1], H1, H2, combos)


def ids(case, normalize):
    """The history ids of a run."""
    return case.hist if normalize else case.hist_plain


def ref_len(case):
    """The length vector the references take."""
    return np.full(case.hist.shape[0], case.T, np.int32) if case.hist_len is None else case.hist_len


def valid_mask(case, normalize=True):
    """[B, T]: the positions that take part (j < hist_len[b], id >= 0): the oracle's definition."""
    B, T = case.hist.shape
    return (np.arange(T)[None, :] < ref_len(case).astype(np.int64)[:, None]) & (ids(case, normalize) >= 0)


def _lengths(rng, B, T, kind):
    """tests/test_gpu_din_pack.py: _lengths."""
    if kind == "uniform":
        hl = rng.integers(0, T + 1, size=B)
    elif kind == "full":
        hl = np.full(B, T)
    elif kind == "empty_runs":
        hl = rng.integers(1, T + 1, size=B)
        hl[:min(B, 21)] = 0
        hl[B // 2:B // 2 + 40] = 0
        hl[-19:] = 0
    elif kind == "all_empty":
        hl = np.zeros(B)
    elif kind == "multiples":
        hl = np.full(B, 32 if T >= 32 else T)
        hl[1::2] = 0
    else:
        raise ValueError(kind)
    return hl.astype(np.int32)


# (B, T, H1, H2, length kind): test_packed_din_matches_oracle's grid cut down to the shapes that differ in code path
ACT_SHAPES = [(1, 50, 80, 40, "full"), (2, 7, 80, 40, "uniform"), (9, 1, 80, 40, "uniform"), (40, 33, 16, 4, "uniform"),
              (25, 40, 48, 48, "uniform"), (20, 17, 72, 36, "uniform"), (1, 1, 4, 4, "uniform"), (130, 64, 80, 48, "uniform"),
              (1500, 50, 80, 40, "empty_runs"), (64, 50, 80, 40, "all_empty"), (96, 50, 80, 40, "multiples"), (4099, 50, 80, 40, "uniform")]


def _act_shape(i):
    B, T, H1, H2, kind = ACT_SHAPES[i]
    rng = np.random.default_rng(9000 + B * 131 + T * 7 + H1)
    hist = rng.integers(-1, V, size=(B, T))
    hl = _lengths(rng, B, T, kind)
    if (B, T) == (1, 1):
        hl[:] = 1                                              # the one row there is
    return _case("act_shapes-%dx%d-%d-%d-%s" % (B, T, H1, H2, kind), rng, hist, hl, rng.integers(0, V, size=B), H1, H2, PAPER)


NO_CAND = (0, 15) + tuple(range(16, 32)) + (32, 39)          # first and last lane of a block, a whole block, first lane of a part block, the last sample


def _no_candidate(form):
    rng = np.random.default_rng(41 + len(form))
    if form == "40x20":
        B, T = 40, 20
        hl = rng.integers(1, T + 1, size=B)
        hl[[0, 18, 25, 39]] = 0                              # missing candidates on empty samples ...
        hl[[15, 16, 31, 32]] = T                             # ... and on full ones
        miss = NO_CAND
    elif form == "3x20":
        B, T = 3, 20
        hl = np.array([T, 0, 7])
        miss = (0, 1)
    elif form == "40-dense":                                 # wave 0: blocks [0, 16), [16, 32) and a part block from 32
        B, T = 40, 1500
        hl = rng.integers(1, 5, size=B)
        hl[[0, 18, 25, 33]] = 0
        hl[34:] = T                                          # "full" here: the six samples that soak up the other waves
        hl[[15, 16, 31, 32]] = 4
        miss = NO_CAND
    elif form == "3-dense":                                  # one wave holds all three samples: a 3-sample block, 13 idle lanes
        B, T = 3, 100
        hl = np.array([2, 0, T])
        miss = (0, 1)
    else:
        raise ValueError(form)
    hist = rng.integers(-1, V, size=(B, T))
    cand = rng.integers(0, V, size=B)
    cand[list(miss)] = -1
    return _case("no_candidate-" + form, rng, hist, hl, cand)


I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _lengths_out_of_range(form):
    dense = "dense" in form
    # (the forms without a length vector: the same operands.  The dense seed is the first of 72 .. 76 that leaves fp32 the most room:
    # 7.1e-7; the five give 7.1e-7 .. 1.06e-6, the largest from one score of the PReLU unit.)
    rng = np.random.default_rng(73 if dense else 71)
    B, T = 70, (2000 if dense else 9)
    hist = rng.integers(-1, V, size=(B, T))
    if dense:                                                # wave 0 holds samples 0 .. 60: block edges at 16, 32, 48 inside one wave
        hl = rng.integers(0, 4, size=B).astype(np.int64)
        hl[60:] = T
        hl[[0, 15, 16, 31, 32]] = [-1, I32_MIN, -7, -1, I32_MIN]        # out of range on both sides of the edges at 16 and 32 ...
        hl[[47, 48]] = [I32_MIN, -1]
        hl[[66, 67, 69]] = [T + 1, I32_MAX, I32_MAX]                    # ... and above T on the long samples, the last one included
        hl[5] = 0
    else:
        hl = rng.integers(0, T + 1, size=B).astype(np.int64)
        hl[0], hl[B - 1] = -1, I32_MAX                       # first and last sample
        hl[15:17] = [T + 1, I32_MIN]                         # both sides of sample 16 ...
        hl[30:38] = [-1, T + 1, I32_MIN, I32_MAX, -1, I32_MAX, T + 1, I32_MIN]      # ... and a run that several waves' ranges cut
        hl[40] = 0
    return _case("lengths_out_of_range-" + form, rng, hist, None if form.endswith("none") else hl, rng.integers(0, V, size=B))


def _all_masked():
    B, T = 50, 40
    rng = np.random.default_rng(23)
    hist = rng.integers(-1, V, size=(B, T))
    hl = rng.integers(1, T + 1, size=B)
    for b, n in ((0, T), (7, 1), (8, 33), (21, 16), (49, T)):      # positive length, every position masked (first and last sample included)
        hl[b] = n
        hist[b] = -1
    hl[3] = T; hist[3, 1:] = -1; hist[3, 0] = 5                    # valid at position 0 only
    hl[12] = T; hist[12, :T - 1] = -1; hist[12, T - 1] = 6         # valid at its last position only
    for b in (16, 17, 30, 31):                                     # positions 0 .. 31 masked, valid rows behind: whichever of them starts
        hl[b] = T; hist[b, :32] = -1; hist[b, 32:] = rng.integers(0, V, size=T - 32)      # its block has a pass of 32 masked rows
    return _case("all_masked", rng, hist, hl, rng.integers(0, V, size=B))


def masked_passes(case):
    """Passes of 32 rows that are all masked positions inside the length."""
    B, T = case.hist.shape
    n = 0
    for blk in blocks(case.hist_len, T, B):
        s, p = block_rows(blk)
        m = case.hist[s, p] < 0
        n += sum(1 for i in range(blk.rows // PASS) if m[PASS * i:PASS * (i + 1)].all())
    return n


def _past_one_chunk_size():
    B, T = 65536 + 200, 2
    rng = np.random.default_rng(65)
    return _case("past_one_chunk_size", rng, rng.integers(-1, V, size=(B, T)), rng.integers(0, T + 1, size=B), rng.integers(0, V, size=B))


LONG_KEPT = (0, 31, 32, 65533, 65534)


def _long_history(form):
    """full: every position valid (normalize only: a convex combination); sparse: all but a dozen positions masked (a hundred leave fp32
    1.6e-6 off float64 in the plain sum), so that the index arithmetic runs over the whole length while the plain sum stays short;
    beyond: T = 65 536, one past din_pack_covers; widest: T = 2^20, the longest history the wide position field holds (one sample: a block
    of 32 768 passes)."""
    rng = np.random.default_rng({"full": 604, "sparse": 606, "beyond": 606, "widest": 611}[form])
    B, T = {"beyond": (2, MAX_T + 1), "widest": (1, MAX_T_WIDE)}.get(form, (3, MAX_T))
    if form == "full":
        hist = rng.integers(0, V, size=(B, T))
        combos = (("sigmoid", True), ("dice", True))
    else:
        hist = np.full((B, T), -1, np.int64)
        for b in range(B):
            keep = np.unique(np.concatenate([[j for j in LONG_KEPT + (32767, 32768, 65535, 65536, 1 << 19, T - 2) if j < T] + [T - 1],
                                             rng.integers(0, T, size=4 if T <= MAX_T + 1 else 2)]))
            hist[b, keep] = rng.integers(0, V, size=keep.size)
        combos = (("sigmoid", True), ("dice", False)) if form == "widest" else (("sigmoid", False), ("sigmoid", True), ("dice", False), ("dice", True))
    hl = np.full(B, T)
    if form == "sparse":
        hl[1] = T - 1                                          # one sample a row short: the next block's rows start off a tile edge
    return _case("long_history-" + form, rng, hist, hl, rng.integers(0, V, size=B), combos=combos, keep=0)


def _null_image():
    B, T = 257, 30
    rng = np.random.default_rng(3)
    cand = rng.integers(0, V, size=B)
    cand[[0, 100, 256]] = -1
    return _case("null_image", rng, rng.integers(-1, V, size=(B, T)), rng.integers(0, T + 1, size=B), cand, combos=PAPER)


BUILDERS = collections.OrderedDict()
for _i, _s in enumerate(ACT_SHAPES):
    BUILDERS["act_shapes-%dx%d-%d-%d-%s" % _s] = functools.partial(_act_shape, _i)
for _f in ("40x20", "3x20", "40-dense", "3-dense"):
    BUILDERS["no_candidate-" + _f] = functools.partial(_no_candidate, _f)
BUILDERS["past_one_chunk_size"] = _past_one_chunk_size
for _f in ("small", "small-none", "dense", "dense-none"):
    BUILDERS["lengths_out_of_range-" + _f] = functools.partial(_lengths_out_of_range, _f)
BUILDERS["all_masked"] = _all_masked
for _f in ("full", "sparse", "beyond", "widest"):
    BUILDERS["long_history-" + _f] = functools.partial(_long_history, _f)
BUILDERS["null_image"] = _null_image
NAMES = list(BUILDERS)
BEYOND = ["long_history-beyond", "long_history-widest"]
# the cases of the parametrised GPU test (the packed kernel through ops.din_attention_pool); the others have tests of their own
PACKED = [n for n in NAMES if n not in BEYOND + ["null_image"]]


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


def grid(names):
    """-> [(case name, activation, normalize)]: every case at the combinations it runs for."""
    return [(n, a, z) for n in names for a, z in case(n).combos]


def scaled(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max()) if got.size else 0.0


def subsample(c, stride):
    """Every stride-th sample of a case (the references are per-sample: a subsample's rows are the whole batch's rows)."""
    sl = slice(0, None, stride)
    return c._replace(hist=c.hist[sl], hist_plain=c.hist_plain[sl], hist_len=None if c.hist_len is None else c.hist_len[sl], cand=c.cand[sl])
