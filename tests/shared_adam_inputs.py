"""Inputs of tests/test_gpu_shared_adam.py (host side, NumPy only): five tf.train.AdamOptimizer steps over three slots of which slots 0
and 2 read ONE 7-row table (feature_column.shared_embedding_columns) and slot 1, between them, a 50-row table of its own -- the geometry
of tests/shared_embedding_inputs.py --, the float64 restatement of the TF sparse Adam with the shared table as the ONE variable it is, and
what each of the three per-slot formulations of that step would give instead:

  norm    the clip norm taken per slot, sqrt(sum_r ||S_a,r||^2 + ||S_b,r||^2) instead of ||S_a + S_b|| (the cross term dropped);
  steps   a touched row stepped once per slot with that slot's part of the gradient (m and v are not linear in g);
  sweep   the rows no entry names decayed and stepped once per SLOT of their table, i.e. twice on the shared table.

Ids are uniform over [-1, V] (both pruned edges occur), every fifth sample has the same id in both sharing slots, and every row of the
shared table is hit from both slots in steps 1, 3 and 5.  Steps 2 and 4 leave row 3 of the shared table and rows 40..49 of the 50-row
table without an entry (their ids become -1), so that the sweep has rows to visit whose m and v are not zero.  The sharing slots'
gradients have a common part per row (2 u_r + noise): the summed gradient's norm is about sqrt(2) times the per-slot one.

clip modes: "zero" (clip_norm 0), "idle" (10 x the largest norm of any step) and "active": the geometric mean of the largest per-slot
norm and the smallest summed norm of the shared table over the five steps -- ||g|| > clip ONLY through the cross term between the
slots, a per-slot norm never clips.  (The 50-row table's own norm is far below it: one clipped and one unclipped table per step.)

Conditions every case meets, asserted on the inputs and never on the kernel: each formulation above misses the float64 reference by at
least 100 x BAR on var, m or v of the shared table (`norm` in the active mode only: where no clip acts the norm does not matter).  The
measure is the GPU test's: max |got - ref| / max |ref| per array, BAR = 1e-5 (tests/test_gpu_backward.py:
test_sparse_adam_matches_tf_semantics_over_steps)."""
import functools

import numpy as np

VOCAB = (7, 50, 7)                     # per slot; slots 0 and 2 are one table
SLOT_TABLE = (0, 1, 0)
TABLE_VOCAB = (7, 50)
F = len(VOCAB)
SHARING = (0, 2)
STEPS = 5
SPARSE_STEPS = (2, 4)                  # the steps that leave REST_SHARED / REST_OWN without an entry
REST_SHARED, REST_OWN = 3, np.arange(40, 50)
B1, B2, EPS, LR = 0.9, 0.999, 1e-4, 0.01
BAR = 1e-5
MODES = ("zero", "active", "idle")
SEED = 31


def array_err(got, ref):
    """max |got - ref| as a fraction of the array's scale (m and v are orders of magnitude smaller than var)"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-30))


def lr_t_of(t):
    return LR * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)


class Adam64:
    """tf.train.AdamOptimizer._apply_sparse on ONE variable in float64, the hyper-parameters as the fp32 graph sees them (oracle.np_ref.
    sparse_adam_step's convention: 1 - beta is formed in fp32).  step(parts, ...): parts = the dense [V, K] gradient of every slot that
    reads the variable; how = None (the variable's one step), or one of the three per-slot formulations."""

    def __init__(self, w0, clip, how=None):
        self.w, self.m, self.v = w0.astype(np.float64), np.zeros(w0.shape), np.zeros(w0.shape)
        self.clip, self.how = float(np.float32(clip)), how
        self.b1, self.b2, self.eps = float(np.float32(B1)), float(np.float32(B2)), float(np.float32(EPS))
        self.omb1, self.omb2 = float(np.float32(1) - np.float32(B1)), float(np.float32(1) - np.float32(B2))
        self.norms = []                # per step: (the variable's ||g||, the per-slot norm)

    def _rows(self, rows, g, lr_t):
        self.m[rows] = self.m[rows] * self.b1 + g[rows] * self.omb1
        self.v[rows] = self.v[rows] * self.b2 + g[rows] * g[rows] * self.omb2
        self.w[rows] = self.w[rows] - lr_t * self.m[rows] / (np.sqrt(self.v[rows]) + self.eps)

    def step(self, parts, touched, t):
        """touched: per part, the bool [V] mask of the rows its entries name"""
        lr_t = float(np.float32(lr_t_of(t)))
        g = sum(parts)
        norm = float(np.sqrt((g * g).sum()))
        per_slot = float(np.sqrt(sum((p * p).sum() for p in parts)))
        self.norms.append((norm, per_slot))
        scale = 1.0
        if self.clip > 0:
            scale = self.clip / max(per_slot if self.how == "norm" else norm, self.clip)
        any_touched = np.logical_or.reduce(touched)
        if self.how == "steps":
            for p, rows in zip(parts, touched):
                self._rows(rows, p * scale, lr_t)
            self._rows(~any_touched, g * 0.0, lr_t)
            return
        self._rows(np.ones(len(g), bool), g * scale, lr_t)
        if self.how == "sweep":
            for _ in parts[1:]:
                self._rows(~any_touched, g * 0.0, lr_t)


def _dense(V, K, ids, grad):
    g = np.zeros((V, K))
    ok = (ids >= 0) & (ids < V)
    np.add.at(g, ids[ok], grad[ok].astype(np.float64))
    touched = np.zeros(V, bool)
    touched[ids[ok]] = True
    return g, touched


@functools.lru_cache(maxsize=None)
def case(B, K, mode):
    """-> dict: ids [STEPS][B, 3] int64, grad [STEPS][B, 3K] fp32, w0 per DISTINCT table, clip, ref = {"var", "m", "v"} per distinct
    table in float64 after the five steps, own_rest = the rows of the 50-row table that steps 2 and 4 leave alone, miss = what each
    per-slot formulation is off by on the shared table, norms = per step (summed, per-slot) of the shared table."""
    assert mode in MODES
    rng = np.random.default_rng(1000 * SEED + 10 * K + B % 7)           # (the three modes of one (B, K) see the same batches)
    u = rng.standard_normal((TABLE_VOCAB[0], K))
    gscale = 30.0 / B
    w0 = [(rng.standard_normal((v, K)) * 0.25).astype(np.float32) for v in TABLE_VOCAB]
    ids_t, grad_t = [], []
    for t in range(1, STEPS + 1):
        ids = np.stack([rng.integers(-1, v + 1, size=B) for v in VOCAB], 1).astype(np.int64)
        ids[::5, 2] = ids[::5, 0]
        for v in (-1, 7):
            assert (ids[:, 0] == v).any() and (ids[:, 2] == v).any()
        assert (ids[:, 1] == -1).any() and (ids[:, 1] == 50).any()
        if t in SPARSE_STEPS:
            for f in SHARING:
                ids[ids[:, f] == REST_SHARED, f] = -1
            ids[np.isin(ids[:, 1], REST_OWN), 1] = -1
        for r in range(7):
            hit = (ids[:, 0] == r).any() and (ids[:, 2] == r).any()
            assert hit != (t in SPARSE_STEPS and r == REST_SHARED), "step %d row %d" % (t, r)
        assert (ids[::5, 2] == ids[::5, 0]).all() and (ids[::5, 0] >= 0).any()
        grad = rng.standard_normal((B, F * K)) * 0.5
        for f in SHARING:
            ok = (ids[:, f] >= 0) & (ids[:, f] < 7)
            grad[ok, f * K:(f + 1) * K] += 2.0 * u[ids[ok, f]]
        ids_t.append(ids)
        grad_t.append((grad * gscale).astype(np.float32))

    def run(clip, how=None):
        """-> (the shared table's Adam64, the 50-row table's)"""
        sh, own = Adam64(w0[0], clip, how), Adam64(w0[1], clip)
        for t, (ids, grad) in enumerate(zip(ids_t, grad_t), 1):
            parts = [_dense(7, K, ids[:, f], grad[:, f * K:(f + 1) * K]) for f in SHARING]
            sh.step([p[0] for p in parts], [p[1] for p in parts], t)
            g, touched = _dense(50, K, ids[:, 1], grad[:, K:2 * K])
            own.step([g], [touched], t)
        return sh, own

    probe_sh, probe_own = run(0.0)
    summed, per_slot = [n[0] for n in probe_sh.norms], [n[1] for n in probe_sh.norms]
    if mode == "zero":
        clip = 0.0
    elif mode == "idle":
        clip = 10.0 * max(summed + [n[0] for n in probe_own.norms])
    else:
        clip = float(np.sqrt(max(per_slot) * min(summed)))
        assert max(per_slot) * 1.05 < clip < min(summed) / 1.05, "no room for a clip between the per-slot norms %s and the summed ones %s" \
            % (per_slot, summed)
        assert max(n[0] for n in probe_own.norms) < clip                   # the 50-row table is not clipped in the same call
    clip = float(np.float32(clip))
    sh, own = run(clip)
    ref = {"var": [sh.w, own.w], "m": [sh.m, own.m], "v": [sh.v, own.v]}
    assert np.abs(ref["m"][0][REST_SHARED]).min() > 0 and np.abs(ref["m"][1][REST_OWN]).max() > 0
    assert float(np.abs(sh.w - w0[0]).min()) > 1e-3                        # no element of the shared table can pass by standing still
    miss = {}
    for how in ("norm", "steps", "sweep"):
        bad = run(clip, how)[0]
        miss[how] = max(array_err(bad.w, sh.w), array_err(bad.m, sh.m), array_err(bad.v, sh.v))
        if how != "norm" or mode == "active":
            assert miss[how] >= 100 * BAR, "%s is only %.2e off at B=%d K=%d %s: these inputs would not notice it" % (how, miss[how], B, K, mode)
    for a in ids_t + grad_t + w0:
        a.setflags(write=False)
    return dict(ids=ids_t, grad=grad_t, w0=w0, clip=clip, ref=ref, miss=miss, norms=sh.norms, own_norms=[n[0] for n in own.norms])
