"""Inputs of tests/test_gpu_shared_embedding.py (host side, NumPy only): one sorted Adagrad step over three slots of which slots 0 and 2
read ONE 7-row table (feature_column.shared_embedding_columns) and slot 1, between them, a 50-row table of its own -- so the sharing
slots' keys straddle slot 1's --, the float64 result of oracle.np_ref.sparse_adagrad_step with the shared table fed as ONE table, and
the two conditions every committed seed meets:

  (a) the float64 update moves every row of the shared table by more than 1e-3 (no row can pass by standing still);
  (b) stepping the two slots one after the other on the shared table -- two Adagrad steps with two partial gradients, what a kernel that
      merely aliases the pointers does -- misses the 1e-5 bar of the GPU test by at least 2x, on the table and on the accumulator.

Both are asserted on the inputs, never on the kernel."""
import functools

import numpy as np

from oracle import np_ref as R
from tests.hot_rows_inputs import BAR, scaled      # noqa: F401  (the project's bar: max |got - ref| / (1 + |ref|) <= 1e-5)

VOCAB = (7, 50, 7)                     # per slot; slots 0 and 2 are one table
SLOT_TABLE = (0, 1, 0)
TABLE_VOCAB = (7, 50)
F = len(VOCAB)
LR = 0.05
SEED = 20


def prune(ids, V):
    """ids as the oracle takes them: everything outside [0, V) is -1 (the kernel prunes id < 0 and id >= V alike)."""
    return np.where((ids >= 0) & (ids < V), ids, -1)


def gathered(tables, ids):
    """The rows the forward reads: [B, F*K] fp32, zero rows for pruned ids; tables per SLOT."""
    B, K = ids.shape[0], tables[0].shape[1]
    emb = np.zeros((B, len(tables), K), np.float32)
    for f, t in enumerate(tables):
        ok = (ids[:, f] >= 0) & (ids[:, f] < t.shape[0])
        emb[ok, f] = t[ids[ok, f]]
    return emb.reshape(B, -1)


@functools.lru_cache(maxsize=None)
def case(B, K, fm):
    """-> dict.  ids [B, 3] uniform over [-1, V] (-1 and V are pruned; every table row is hit from both sharing slots; every fifth sample
    has the same id in both), grad [B, 3K] fp32, tables / accumulators per DISTINCT table (accumulators from U(0.1, 1)); fm: fm_g [B]
    and the entry gradient is np_ref.fm_logit_backward's over the gathered rows, plus grad.  ref_w / ref_a: float64, per distinct table."""
    rng = np.random.default_rng(1000 * SEED + 10 * K + B % 7 + (1 if fm else 0))
    ids = np.stack([rng.integers(-1, v + 1, size=B) for v in VOCAB], 1).astype(np.int64)
    ids[::5, 2] = ids[::5, 0]
    grad = (rng.standard_normal((B, F * K)) * 0.5).astype(np.float32)
    w0 = [(rng.standard_normal((v, K)) * 0.25).astype(np.float32) for v in TABLE_VOCAB]
    a0 = [rng.uniform(0.1, 1.0, size=(v, K)).astype(np.float32) for v in TABLE_VOCAB]
    fm_g = (rng.standard_normal(B) * 0.1).astype(np.float32) if fm else None
    if fm:
        emb = gathered([w0[t] for t in SLOT_TABLE], ids)
        total = R.fm_logit_backward(emb, fm_g, F, K, add_in=grad)                  # float64 [B, F*K]
    else:
        total = grad.astype(np.float64)
    for v in (-1, 7):
        assert (ids[:, 0] == v).any() and (ids[:, 2] == v).any()
    for r in range(7):
        assert (ids[:, 0] == r).any() and (ids[:, 2] == r).any(), "row %d is not hit from both slots" % r
    sh = (0, 2)
    ids_sh = prune(ids[:, sh], 7).reshape(-1, 1)                                    # entry order e = b*2 + j
    g_sh = np.stack([total[:, f * K:(f + 1) * K] for f in sh], 1).reshape(-1, K)   # the matching [2B, K] rows
    ref_w, ref_a = [a.astype(np.float64) for a in w0], [a.astype(np.float64) for a in a0]
    R.sparse_adagrad_step(ref_w[0:1], ref_a[0:1], ids_sh, g_sh, LR)
    R.sparse_adagrad_step(ref_w[1:2], ref_a[1:2], prune(ids[:, 1:2], 50), total[:, K:2 * K], LR)
    moved = np.abs(ref_w[0] - w0[0]).max(1)
    assert (moved > 1e-3).all(), "(a) a row of the shared table moves by %.2e only" % moved.min()
    seq_w, seq_a = [w0[0].astype(np.float64)], [a0[0].astype(np.float64)]
    for f in sh:                                                                     # the failure guarded against: one step per slot
        R.sparse_adagrad_step(seq_w, seq_a, prune(ids[:, f:f + 1], 7), total[:, f * K:(f + 1) * K], LR)
    miss = (scaled(seq_w[0], ref_w[0]), scaled(seq_a[0], ref_a[0]))
    assert min(miss) >= 2 * BAR, "(b) stepping slot by slot is only %.2e / %.2e off: these inputs would not notice it" % miss
    for a in [ids, grad] + w0 + a0 + ([fm_g] if fm else []):
        a.setflags(write=False)
    return dict(ids=ids, grad=grad, w0=w0, a0=a0, fm_g=fm_g, ref_w=ref_w, ref_a=ref_a, miss=miss)
