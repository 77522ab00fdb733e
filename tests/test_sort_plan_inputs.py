"""CPU self-checks of tests/sort_plan_inputs.py: the plan table follows rs_layout's rule, every entry list holds the runs, the edge rows
and the dropped entries it is built for, and the fp32-faithful emulation of every rule on those inputs stays within ROOM (4e-6) of the
float64 references -- so the GPU tests' bar (1e-5) measures the kernels and not fp32."""
import numpy as np
import pytest

from tests import sort_plan_inputs as S

EMU_TOTALS = S.TOTALS               # (the references and emulations work on the touched rows only: 2^27 rows cost what 255 do)


def test_plan_table_matches_the_rule():
    assert len(S.PLANS) == 11
    for total, bits, digit, passes, inbuf in S.PLANS:
        assert S.sort_plan(total) == (bits, digit, passes, inbuf), total
        assert (1 << bits) > total >= (1 << (bits - 1))
        assert digit * passes >= bits and inbuf == (0 if passes % 2 else 1)
    # every pass structure of the sort is there, and both sides of every change of plan
    assert {(d, p) for _, _, d, p, _ in S.PLANS} == {(8, 1), (9, 1), (8, 2), (9, 2), (8, 3), (9, 3), (8, 4)}
    assert len(S.distinct_plan_totals()) == 7
    for lo, hi in ((255, 256), (511, 512), (65535, 65536), ((1 << 18) - 1, 1 << 18), ((1 << 24) - 1, 1 << 24)):
        assert lo in S.TOTALS and hi in S.TOTALS and S.sort_plan(lo)[1:3] != S.sort_plan(hi)[1:3]


@pytest.mark.parametrize("form", ["payload", "ids"])
@pytest.mark.parametrize("n", S.NS)
@pytest.mark.parametrize("total", S.TOTALS)
def test_entry_lists_hold_the_runs_edges_and_dropped_entries(total, n, form):
    c = S.entries(total, n) if form == "payload" else S.ids_entries(total, n)
    big = n == S.BIG
    assert sum(c.vocab) == total and c.vocab[0] == 7 and c.vocab[2] == (300 if total >= 511 else 100)
    assert c.n == (n if form == "payload" else 3 * S.IDS_B[n]) and (form == "payload" or S.IDS_B[n] < 4096)
    assert (c.n > 2 * S.SORT_TILE) == (big and form == "payload") and (c.n > S.SORT_TILE) == big
    r = S.run_report(c)
    assert r["low_run"] == S.RUN_LOW                                        # ends one entry past a 256-entry tile edge, from position 0
    if big:
        assert r["high_run"] == S.RUN_HIGH and r["high_start"] % S.TILE != 0 and r["high_end"] % S.TILE == 1
        assert r["high_end"] == r["live"]                                   # the highest live key: only dropped entries sort behind it
    for (f, row), count in r["edge"].items():
        want = S.RUN_LOW if (f, row) == (0, 0) else (S.RUN_HIGH if big and (f, row) == (2, c.vocab[2] - 1) else 1)
        assert count == want, (f, row, count)
    assert r["negatives"] >= 5 and min(r["at_vocab"]) >= 2
    assert r["dropped_key"] == r["negatives"] + sum(r["at_vocab"]) == c.n - r["live"]
    # an entry one past table f is dropped: it is NOT row 0 of table f + 1 (key row_base[f + 1]), and one past the last table is the
    # dropped key itself
    past = c.row == np.asarray(c.vocab)[c.slot]
    assert (c.key[past] == total).all() and c.row_base[2] + c.vocab[2] == total
    for f in range(2):
        assert int((c.key == c.row_base[f + 1]).sum()) == 1                 # row 0 of the next table: its single entry only
    if form == "payload":
        pay = S.payload_of(c)
        assert (pay[c.row < 0] < 0).all() and ((pay[c.row >= 0] % S.F) == c.slot[c.row >= 0]).all()
        assert not np.array_equal(c.key, np.sort(c.key))                    # shuffled
        pos = S.positions_of(c)
        assert {-1, total, total + 5} <= set(pos[~c.live].tolist()) and np.array_equal(pos[c.live], c.key[c.live])
    else:
        ids, grad = S.ids_of(c)
        assert ids.shape == (S.IDS_B[n], S.F) and grad.shape == (S.IDS_B[n], S.F * S.K)
        assert np.array_equal(ids.reshape(-1), c.row) and (c.slot.reshape(-1, S.F) == np.arange(S.F)).all()


@pytest.mark.parametrize("form", ["payload", "ids"])
@pytest.mark.parametrize("n", S.NS)
@pytest.mark.parametrize("total", EMU_TOTALS)
def test_fp32_emulation_of_every_rule_leaves_room_under_the_bar(total, n, form):
    c = S.entries(total, n) if form == "payload" else S.ids_entries(total, n)
    w0, a0, z0 = S.start_state(c, 5)
    room = {"adagrad": S.worst(S.emu_adagrad(c, w0, a0), S.ref_adagrad(c, w0, a0))}
    zeros = [np.zeros_like(w) for w in w0]
    room["adam"] = S.worst(S.emu_adam(c, w0, zeros, zeros), S.ref_adam(c, w0, zeros, zeros))
    w1, n1, z1 = S.start_state(c, 6, width=1)
    room["ftrl"] = S.worst(S.emu_ftrl(c, w1, n1, z1), S.ref_ftrl(c, w1, n1, z1))
    pos, sums, counts = S.ref_scatter(c)
    order = np.argsort(c.key, kind="stable")
    order = order[c.live[order]]
    cuts = np.flatnonzero(np.diff(c.key[order])) + 1
    got = np.stack([S.kahan_sum(c.grad[part]) for part in np.split(order, cuts)])
    assert got.shape == sums.shape and np.array_equal(counts, [len(p) for p in np.split(order, cuts)])
    room["scatter"] = S.scaled(got, sums)
    print("total %d n %d %s: fp32 room %s" % (total, n, form, "  ".join("%s %.2e" % kv for kv in room.items())))
    bad = {k: v for k, v in room.items() if not v <= S.ROOM}
    assert not bad, "fp32 on these inputs is %s off float64: no room under %.0e" % (bad, S.BAR)


@pytest.mark.parametrize("shape", S.CLIP_SHAPES)
@pytest.mark.parametrize("norm", S.CLIP_NORMS)
def test_clip_range_cases_have_their_norms_and_fp32_room(norm, shape):
    c = S.clip_case(norm, shape)
    assert c["ids"].shape == (S.CLIP_B, S.F) and S.CLIP_B < 4096
    for n2 in c["norm2"]:
        assert abs(np.sqrt(n2) / norm - 1) < 1e-5                           # "about": the entries are rounded to fp32 after scaling
    if shape == "concentrated":
        assert int((c["ids"][:, 2] == S.CLIP_VOCAB[2] - 1).sum()) == S.CLIP_HOT and c["hot_share"] > 0.99
    else:
        assert c["top_share"] < 0.02
    assert (norm > S.CLIP) == (norm > 100)
    room = S.worst(S.clip_emu(norm, shape), S.clip_ref(norm, shape))
    print("clip case %g %s: hot share %.4f, fp32 room (exact norm) %.2e" % (norm, shape, c["hot_share"], room))
    assert room <= S.ROOM
    pay, grad = S.clip_payload(norm, shape)
    assert pay.shape == (S.CLIP_B * S.F,) and grad.shape == (S.CLIP_B * S.F, S.CLIP_K) and int((pay < 0).sum()) == int((c["ids"] < 0).sum())


def test_dense_groups_never_lead_a_chunk_with_its_largest_variable():
    for n_vars in S.DENSE_GROUPS:
        sizes = S.dense_sizes(n_vars)
        assert len(sizes) == n_vars and set(sizes) <= set(S.DENSE_SIZES)
        for v0 in range(0, n_vars, 16):
            chunk = sizes[v0:v0 + 16]
            if len(chunk) > 1:
                assert max(chunk) == S.DENSE_SIZES[-1] and chunk[0] != max(chunk) and chunk.count(max(chunk)) == 1
    assert len(S.dense_sizes(33)) == 33 and len(S.dense_sizes(17)[16:]) == 1      # a second and a third launch
    w, acc = S.dense_ref(np.ones(3, np.float32), np.full(3, 0.1, np.float32), [np.full(3, 2.0, np.float32)], 0.5, 0.0)
    assert np.allclose(acc, 4.1) and np.allclose(w, 1 - 0.5 * 2 / np.sqrt(4.1))
