"""Hot rows through the sorted sparse updates (csrc/backward.hip: sparse_sorted_update -- adagrad_tile_k's run sums, adagrad_fix_k for runs
that cross 256-entry tiles): ONE step of every rule, with one row of one slot hit 140 ... 20 000 times, against the float64 rule
(oracle.np_ref: sparse_ftrl_step, sparse_adagrad_step, sparse_adam_step) at the project's bar: max |got - ref| / (1 + |ref|) <= 1e-5 on
every state tensor.

The hit counts 255 / 256 / 257 / 513 put run ends on, before and after tile edges, with the hot row as the lowest key of the sort (its run
starts at a tile start) and as the highest live key (it starts mid-tile); one case has two adjacent hot rows, so that one tile carries an
open-left and an open-right run; B = 4000 takes the plain sort, B = 32 768 the slot-major one.  For FTRL the hot row's state is set so
that z + S cancels (n = 0.1 + S^2, z = -S + u): z_new is O(1) and carries the run sum's ABSOLUTE error at full size.  tests/hot_rows_inputs.py
builds the inputs and asserts on the CPU that fp32 itself leaves room under the bar and that the run sums formed the old ways (one
sequential sum; plain sums per tile; compensated tiles with plain adds across them) would miss it.

Measured on an MI355X, with plain run sums and with the compensated ones: see DESIGN.md 5.2."""
import numpy as np
import pytest
import torch

from tests import hot_rows_inputs as H

pytestmark = pytest.mark.gpu
BAR = H.BAR


def _cuda(a):
    return torch.tensor(np.asarray(a)).cuda()              # (a copy: the cached inputs are read-only)


def _report(what, errs):
    print("%s: %s" % (what, "  ".join("%s %.2e" % kv for kv in errs.items())))
    bad = {k: v for k, v in errs.items() if not v <= BAR}
    assert not bad, "%s: %s above %.0e of float64" % (what, bad, BAR)


@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (0.01, 0.05)])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_ftrl_hot_row_matches_float64(built_lib, case, K, l1, l2):
    """ops.SparseFtrl, three-array form: K = 1 with one [B, 1] gradient shared by the slots, K = 4 with per-slot gradients (the VEC = 4
    apply).  K = 1 also runs the packed rows (TableSet.ftrl_rows, dir_sparse_ftrl_rows_sorted_f32): bitwise the three-array result."""
    from dir_amd import ops
    c = H.ftrl_case(case, K, l1, l2)
    shape = (lambda v: (v,)) if K == 1 else (lambda v: (v, K))
    tabs = [_cuda(c["w0"][f].reshape(shape(v))) for f, v in enumerate(H.VOCAB)]
    opt = ops.SparseFtrl(tabs, lr=H.FTRL_LR, initial_accumulator_value=0.1, l1=l1, l2=l2)
    for f, v in enumerate(H.VOCAB):                        # the state that cancels, written in place
        opt.accums[f].copy_(_cuda(c["n0"][f].reshape(shape(v))))
        opt.linears[f].copy_(_cuda(c["z0"][f].reshape(shape(v))))
    ids, grad = _cuda(c["ids"]), _cuda(c["grad"])
    opt.step(ids, grad)
    got = [[t.cpu().numpy().reshape(v, K) for t, v in zip(s, H.VOCAB)] for s in (tabs, opt.accums, opt.linears)]
    errs = {name: max(H.scaled(got[i][f], c["ref"][i][f]) for f in range(H.F)) for i, name in enumerate("wnz")}
    if K == 1:
        rows = ops.TableSet.ftrl_rows([_cuda(c["w0"][f].reshape(-1)) for f in range(H.F)], 0.1)
        opt_p = ops.SparseFtrl(rows, lr=H.FTRL_LR, initial_accumulator_value=0.1, l1=l1, l2=l2)
        assert opt_p.packed
        for f in range(H.F):
            rows.accums[f].copy_(_cuda(c["n0"][f]).reshape_as(rows.accums[f]))
            rows.linears[f].copy_(_cuda(c["z0"][f]).reshape_as(rows.linears[f]))
        opt_p.step(ids, grad)
        for f in range(H.F):
            assert torch.equal(rows.tables[f].reshape(-1), tabs[f]) and torch.equal(rows.accums[f].reshape(-1), opt.accums[f]) \
                and torch.equal(rows.linears[f].reshape(-1), opt.linears[f]), "packed rows differ from the three-array form (slot %d)" % f
    teeth = " ".join("%s %.1e %s" % (k, v[0], v[1]) for k, v in c["teeth"].items()) if c["teeth"] else "-"
    _report("ftrl %s K=%d l1=%g (fp32 room %.1e; emulated old sums, worst z and the columns that would miss: %s)" % (
        H.case_id(case), K, l1, c["room"], teeth), errs)


@pytest.mark.parametrize("K,big_prior,case", [(16, False, c) for c in H.CASES] + [(16, True, c) for c in H.SUBSET] +
                         [(64, False, c) for c in H.SUBSET if c.B == 4000] + [(4, False, H.SUBSET[2])],
                         ids=lambda v: H.case_id(v) if isinstance(v, H.Case) else str(v))
def test_adagrad_hot_row_matches_float64(built_lib, K, big_prior, case):
    """ops.SparseAdagrad(method="sorted") on split tables: K = 16 and 4 stage the hot tiles' gradients in LDS (the tiles of the 5000-row
    slot take the fast path of nearly distinct rows), K = 64 sums from global memory."""
    from dir_amd import ops
    c = H.adagrad_case(case, K, big_prior)
    tabs = [_cuda(w) for w in c["w0"]]
    opt = ops.SparseAdagrad(tabs, lr=H.ADAGRAD_LR, initial_accumulator_value=0.1, method="sorted")
    for f in range(H.F):
        opt.accums[f].copy_(_cuda(c["a0"][f]))
    opt.step(_cuda(c["ids"]), _cuda(c["grad"]))
    errs = {"w": max(H.scaled(tabs[f].cpu().numpy(), c["ref_w"][f]) for f in range(H.F)),
            "accum": max(H.scaled(opt.accums[f].cpu().numpy(), c["ref_a"][f]) for f in range(H.F))}
    _report("adagrad %s K=%d prior=%s (fp32 room %.1e)" % (H.case_id(case), K, big_prior, c["room"]), errs)


@pytest.mark.parametrize("big_prior", [False, True])
@pytest.mark.parametrize("case", H.SUBSET, ids=H.case_id)
def test_adagrad_packed_rows_and_folded_fm_hot_row(built_lib, case, big_prior):
    """ops.SparseAdagrad on TableSet.train_rows with the FM backward folded into the entry gradient (step_fm), beside the split tables fed
    fm_logit_backward's rows: bitwise equal, and both within the bar of float64 Adagrad on those rows."""
    from dir_amd import ops
    K = 16
    c = H.adagrad_case(case, K, big_prior)
    B = case.B
    split = ops.TableSet([_cuda(w) for w in c["w0"]])
    packed = ops.TableSet.train_rows([_cuda(w) for w in c["w0"]], 0.1)
    o_split, o_packed = ops.SparseAdagrad(split, lr=H.ADAGRAD_LR), ops.SparseAdagrad(packed, lr=H.ADAGRAD_LR)
    for f in range(H.F):
        o_split.accums[f].copy_(_cuda(c["a0"][f]))
        o_packed.accums[f].copy_(_cuda(c["a0"][f]))
    ids, gdnn = _cuda(c["ids"]), _cuda(c["grad"])
    gfm = _cuda((np.random.default_rng(case.seed).standard_normal((B, 1)) * 0.01).astype(np.float32))
    emb, _ = ops.gather_fm(split, ids)
    fsum = torch.empty((B, K), device="cuda")
    ops.gather_fm(packed, ids, fsum=fsum)
    demb = ops.fm_logit_backward(emb, gfm, H.F, K, add_in=gdnn)
    o_split.step(ids, demb)
    o_packed.step_fm(ids, gdnn, gfm, fsum)
    for f in range(H.F):
        assert torch.equal(split.tables[f], packed.tables[f]) and torch.equal(o_split.accums[f], o_packed.accums[f]), f
    rows = demb.cpu().numpy()                              # the entry gradients both paths sum: the float64 rule on exactly these
    ref_w, ref_a = [w.astype(np.float64) for w in c["w0"]], [a.astype(np.float64) for a in c["a0"]]
    H.R.sparse_adagrad_step(ref_w, ref_a, c["ids"], rows, H.ADAGRAD_LR)
    room = H.adagrad_check(c["ids"], rows, K, c["w0"], c["a0"], ref_w, ref_a)
    errs = {"w": max(H.scaled(split.tables[f].cpu().numpy(), ref_w[f]) for f in range(H.F)),
            "accum": max(H.scaled(o_split.accums[f].cpu().numpy(), ref_a[f]) for f in range(H.F))}
    _report("adagrad rows + fm %s prior=%s (fp32 room %.1e)" % (H.case_id(case), big_prior, room), errs)


@pytest.mark.parametrize("K,clip,big_prior,case", [(16, clip, False, c) for clip in (0.0, 100.0) for c in H.SUBSET] +
                         [(16, 100.0, True, H.SUBSET[2]), (64, 100.0, False, H.SUBSET[2]), (64, 0.0, False, H.SUBSET[0])],
                         ids=lambda v: H.case_id(v) if isinstance(v, H.Case) else str(v))
def test_adam_hot_row_matches_float64(built_lib, K, clip, big_prior, case):
    """ops.SparseAdam, clip_norm idle and active (the norm pass adds up ||S_r||^2 of the same run sums); K = 64 sums from global memory."""
    from dir_amd import ops
    c = H.adam_case(case, K, clip, big_prior)
    tabs = [_cuda(w) for w in c["w0"]]
    opt = ops.SparseAdam(ops.TableSet(tabs), H.ADAM["b1"], H.ADAM["b2"], H.ADAM["eps"], clip)
    for f in range(H.F):
        opt.ms[f].copy_(_cuda(c["m0"][f]))
        opt.vs[f].copy_(_cuda(c["v0"][f]))
    opt.lr_t = c["lr_t"]
    opt.step(_cuda(c["ids"]), _cuda(c["grad"]))
    got = (tabs, opt.ms, opt.vs)
    errs = {name: max(H.scaled(got[i][f].cpu().numpy(), c["ref"][i][f]) for f in range(H.F)) for i, name in enumerate("wmv")}
    _report("adam %s K=%d clip=%g prior=%s (fp32 room %.1e)" % (H.case_id(case), K, clip, big_prior, c["room"]), errs)
