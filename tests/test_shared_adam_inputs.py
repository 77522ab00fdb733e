"""The inputs of tests/test_gpu_shared_adam.py meet their conditions (no GPU): tests/shared_adam_inputs.py asserts, while it builds a
case, that each per-slot formulation of the shared Adam step misses the float64 reference by at least 100 x the bar; here every case the
GPU test uses is built, the reference is held against oracle.np_ref.sparse_adam_step fed the shared table as ONE table, and the clip
modes are what they claim to be."""
import numpy as np
import pytest

from oracle import np_ref as R
from tests import shared_adam_inputs as SA

CASES = [(B, K, mode) for K in (4, 16) for B in (300, 4096, 8192) for mode in SA.MODES]


@pytest.mark.parametrize("B,K,mode", CASES)
def test_case_conditions(B, K, mode):
    c = SA.case(B, K, mode)                                              # (asserts the hit pattern and the three misses)
    print("B=%d K=%d %s: clip %.4g, shared norms summed %.4g..%.4g per-slot %.4g..%.4g, own <= %.4g; per-slot formulations are off by "
          "norm %.2e steps %.2e sweep %.2e" % (B, K, mode, c["clip"], min(n[0] for n in c["norms"]), max(n[0] for n in c["norms"]),
                                                min(n[1] for n in c["norms"]), max(n[1] for n in c["norms"]), max(c["own_norms"]),
                                                c["miss"]["norm"], c["miss"]["steps"], c["miss"]["sweep"]))
    assert c["miss"]["steps"] >= 100 * SA.BAR and c["miss"]["sweep"] >= 100 * SA.BAR
    summed, per_slot = [n[0] for n in c["norms"]], [n[1] for n in c["norms"]]
    if mode == "active":
        assert c["miss"]["norm"] >= 100 * SA.BAR
        assert max(per_slot) < c["clip"] < min(summed)                   # over the clip only through the cross term between the slots
        assert max(c["own_norms"]) < c["clip"]
    elif mode == "idle":
        assert c["clip"] > max(summed + c["own_norms"])
    else:
        assert c["clip"] == 0.0
    # the same three (B, K) batches under every mode; steps 2 and 4 leave their rows alone, the others hit every shared row from both slots
    for t, ids in enumerate(c["ids"], 1):
        rest = t in SA.SPARSE_STEPS
        for f in SA.SHARING:
            assert bool((ids[:, f] == SA.REST_SHARED).any()) != rest
        assert bool(np.isin(ids[:, 1], SA.REST_OWN).any()) != rest
        assert ids.min() == -1 and ids[:, 1].max() == 50 and ids[:, 0].max() == 7 and ids[:, 2].max() == 7


@pytest.mark.parametrize("B,K,mode", [(300, 4, "active"), (4096, 16, "idle"), (300, 16, "zero")])
def test_reference_is_the_oracle_on_the_one_table(B, K, mode):
    """The shared table's reference is oracle.np_ref.sparse_adam_step with both slots' entries fed as ONE slot of ONE table, entry
    order e = b*2 + j; the 50-row table's is the plain call."""
    c = SA.case(B, K, mode)
    w = [a.astype(np.float64) for a in c["w0"]]
    m, v = [np.zeros_like(a) for a in w], [np.zeros_like(a) for a in w]
    for t, (ids, grad) in enumerate(zip(c["ids"], c["grad"]), 1):
        ids_sh = ids[:, SA.SHARING].reshape(-1, 1)
        g_sh = np.stack([grad[:, f * K:(f + 1) * K] for f in SA.SHARING], 1).reshape(-1, K)
        R.sparse_adam_step(w[0:1], m[0:1], v[0:1], ids_sh, g_sh, SA.LR, SA.B1, SA.B2, SA.EPS, c["clip"], t)
        R.sparse_adam_step(w[1:2], m[1:2], v[1:2], ids[:, 1:2], grad[:, K:2 * K], SA.LR, SA.B1, SA.B2, SA.EPS, c["clip"], t)
    for i in range(2):
        for name, got in (("var", w), ("m", m), ("v", v)):
            assert SA.array_err(got[i], c["ref"][name][i]) <= 1e-12, (i, name)
