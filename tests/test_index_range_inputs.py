"""CPU self-checks of tests/index_range_inputs.py: every layout's table ends just past element 2^31, the probes sit on both sides of every
line, a probe above the 2^31 line has a wrap target that is another row, no wrap target of an updated row is itself updated, the hot
rows are named several times, and one float64 step of every optimiser moves the touched rows by more than ten times the comparison bar -- a
step that a kernel dropped, or applied to another row, cannot pass for one that was made."""
import numpy as np
import pytest

from tests import index_range_inputs as X

OPTIMISERS = {"plain16": ("adagrad", "adam"), "train32": ("adagrad",), "linear1": ("ftrl",), "ftrl4": ("ftrl",), "packed32": (), "din64": ()}


def test_row_counts_are_the_smallest_past_the_line():
    assert [X.rows_past(ld) for ld in (16, 32, 1, 4, 64)] == [2 ** 27 + 64, 2 ** 26 + 64, 2 ** 31 + 64, 2 ** 29 + 64, 2 ** 25 + 64]
    assert X.rows_past(3) == (2 ** 31 + 2) // 3 + 64                       # a stride that does not divide the line
    assert set(OPTIMISERS) == set(X.LAYOUTS)
    for ld, _ in X.LAYOUTS.values():
        V = X.rows_past(ld)
        assert (V - 64) * ld >= 2 ** 31 > (V - 65) * ld                    # exactly 64 rows start at or past element 2^31
        assert V * ld * 4 < 2 ** 34 and V < 2 ** 32 - 1 - X.SMALL_V        # (the sorted updates' keys are 32 bits wide)


@pytest.mark.parametrize("name", list(X.LAYOUTS))
def test_probes_sit_on_both_sides_of_every_line(name):
    ld, width = X.LAYOUTS[name]
    V, P = X.rows_past(ld), X.probes(ld)
    assert width <= ld and P[0] == 0 and P[-1] == V - 1 and len(set(P)) == len(P) == 14 and X.LOW_ROW in P
    for line, (below, at) in zip(X.LINES, X.line_rows(ld)):
        assert below in P and at in P and at == below + 1
        assert (below + 1) * ld <= line <= at * ld and below * ld + width <= line      # wholly below / at or after
    above = [p for p in P if p * ld >= 2 ** 31]
    assert len(above) == 7                                                 # the first row at the line, five random rows, V - 1
    for p in P:
        t = X.wrap_targets(ld, p)
        assert p not in t and all(0 <= r < p for r in t)
        if p * ld >= 2 ** 31:
            assert t, "a probe above the line must have somewhere else to wrap to"
        if p * ld * 4 < 2 ** 31:
            assert not t                                                   # below every line nothing wraps


@pytest.mark.parametrize("name", list(X.LAYOUTS))
def test_no_wrap_target_of_an_updated_row_is_updated(name):
    ld, _ = X.LAYOUTS[name]
    V = X.rows_past(ld)
    kept, targets = X.write_ids(ld)
    below, at = X.line_rows(ld)[-1]
    assert not set(kept) & set(targets)
    dropped = set(X.probes(ld)) - set(kept)
    assert dropped <= set(targets) and 0 in dropped                        # what is left out of the update is watched as a wrap target
    assert {below, at, V - 1} <= set(kept) and sum(p * ld >= 2 ** 31 for p in kept) == 7
    assert X.LOW_ROW in kept and (X.LOW_ROW + 1) * ld * 4 < 2 ** 31                             # a row below every line is updated too
    for p in kept:
        if p * ld >= 2 ** 31:
            assert set(X.wrap_targets(ld, p)) <= set(targets) and X.wrap_targets(ld, p)
    # the mutation argument of the GPU tests: V - 1 starts at element 2^31 + 63 ld.  Cut to 31 bits (a signed element offset with its sign
    # dropped) or, as a byte offset, to 32 bits (an unsigned 32-bit byte offset) it is row 63: a target, never touched
    assert X.wrap_targets(ld, V - 1) == [63] and 63 in targets and 63 not in kept
    # ... and the last row below the 2^31 line, whose byte offset alone is past 2^32, lands 2^30 elements lower
    assert below - 2 ** 30 // ld in X.wrap_targets(ld, below)


@pytest.mark.parametrize("name", list(X.LAYOUTS))
def test_case_names_the_hot_rows_and_the_dropped_ids(name):
    c = X.case(name)
    ld, width = X.LAYOUTS[name]
    V = X.rows_past(ld)
    kept, targets = X.write_ids(ld)
    big = c.ids[:, 1]
    assert c.vocab == (X.SMALL_V, V) and c.grad.shape == (big.size, 2 * width) and c.ids.dtype == np.int64
    assert int((big == V - 1).sum()) == X.HOT_LAST and int((big == X.line_rows(ld)[-1][1]).sum()) == X.HOT_LINE
    assert int((big == -1).sum()) == 1 and int((big == V).sum()) == 1
    assert list(c.touched[1]) == list(kept) and not set(c.touched[1]) & set(targets)
    assert int((c.ids[:, 0] == X.SMALL_V - 1).sum()) >= 2 and 0 in c.ids[:, 0]
    assert (c.compact[:, 1] == -1).sum() == 2 and (c.compact[:, 0] >= 0).all()
    assert np.array_equal(c.touched[1][c.compact[big == V - 1, 1]], [V - 1] * X.HOT_LAST)
    pay, g = X.payload_of(c)
    assert pay.shape == (big.size * 2,) and g.shape == (big.size * 2, width) and int((pay < 0).sum()) == 1
    assert int(pay.max()) == V * 2 + 1 and np.array_equal(g[1], c.grad[0, width:])
    if name == "linear1":
        assert X.SMALL_V + int(kept[-1]) >= 2 ** 31                        # the first consumer run with sort keys at or above 2^31


@pytest.mark.parametrize("name,rule", [(n, r) for n, rules in OPTIMISERS.items() for r in rules])
def test_one_float64_step_moves_every_touched_row_past_the_bar(name, rule):
    c = X.case(name)
    w0, a0, z0 = X.start_state(c, 5)
    zeros = [np.zeros_like(w) for w in w0]
    if rule == "adagrad":
        start, ref = (w0, a0), X.ref_adagrad(c, w0, a0)
    elif rule == "ftrl":
        start, ref = (w0, a0, z0), X.ref_ftrl(c, w0, a0, z0)
    else:
        start, ref = (w0, zeros, zeros), X.ref_adam(c, w0, zeros, zeros)
    for s, (st, rf) in enumerate(zip(start, ref)):
        for f in range(2):
            assert np.isfinite(rf[f]).all() and rf[f].shape == st[f].shape
            moved = np.abs(rf[f] - st[f]) / (1 + np.abs(st[f]))
            per_row = moved.max(1)
            print("%s %s state %d table %d: least-moved touched row %.2e" % (name, rule, s, f, per_row.min()))
            assert per_row.min() > 10 * X.BAR, (name, rule, s, f)


@pytest.mark.parametrize("P", X.ROUTE_OWNERS)
def test_route_stand_ins_compute_in_64_bits(P):
    """oracle.np_ref.shard_div_owner and the stand-in's route() against Python's unbounded integers, on the ids of the GPU routing test."""
    from dir_amd.shard import partition_layout
    from oracle import np_ref as R
    from tests.shard_standin import NumpyBackend
    F = len(X.ROUTE_VOCAB)
    for partitions in [None] + ([list(X.ROUTE_PARTS[P])] if P in X.ROUTE_PARTS else []):
        parts, first, _ = partition_layout(list(X.ROUTE_VOCAB), 1, P, 0, partitions)
        ids = X.route_ids(parts, seed=P)
        own, loc = X.route_exact(ids, parts, first, P)
        live = own >= 0
        assert partitions is None or any(first)
        assert np.array_equal(live, (ids >= 0) & (ids < np.asarray(X.ROUTE_VOCAB)[None, :]))
        for f, V in enumerate(X.ROUTE_VOCAB):
            assert {int(o) for o in own[live[:, f], f]} == {(first[f] + j) % P for j in range(parts[f])}      # every slice is somebody's
            o, l = R.shard_div_owner(np.where(live[:, f], ids[:, f], 0), V, parts[f])
            assert o.dtype == np.int64 and l.dtype == np.int64
            assert np.array_equal(((o + first[f]) % P)[live[:, f]], own[live[:, f], f]) and np.array_equal(l[live[:, f]], loc[live[:, f], f])
        so, sl = NumpyBackend(None, list(X.ROUTE_VOCAB), parts, first, P, 1).route(ids.reshape(-1))
        assert np.array_equal(so.reshape(ids.shape), own) and np.array_equal(sl.reshape(ids.shape), loc)
        assert int((ids >= 2 ** 32).sum()) >= 6 and int((loc * F >= 2 ** 31).sum()) >= 4                    # payload words past 31 bits
        assert int(loc.max()) * F + F - 1 < 2 ** 63
