"""The fused sparse Adam over tables shared between slots (feature_column.shared_embedding_columns; include/dir_hip.h:
dir_sparse_adam_shared_f32) on the GPU: the kernel against the float64 restatement of the TF step on the ONE variable (1), the export
without a map and with an identity map against dir_sparse_adam_f32 (2, 3), its argument checks (4), a DCN with a shared pair under
train_spec.TrainStep against the dense torch formulation (5), a captured step (6) and the optimiser state saved once per table (7).
The inputs of (1) and the conditions they meet: tests/shared_adam_inputs.py."""
import os

import numpy as np
import pytest
import torch

from tests import shared_adam_inputs as SA

pytestmark = pytest.mark.gpu
BAR = SA.BAR


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the kernel against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", SA.MODES)
@pytest.mark.parametrize("B", [300, 4096, 8192])
@pytest.mark.parametrize("K", [4, 16])
def test_shared_adam_matches_float64_over_steps(built_lib, K, B, mode):
    """Five steps, lr_t of t = 1..5, slots 0 and 2 on one 7-row table and slot 1 (50 rows) between them.  300 takes the plain sort, 4096 is
    where a set without sharing would switch sort plans, 8192 gives every shared row some 1 800 entries per step: runs across many
    256-entry tiles.  active: the shared table's ||g|| exceeds the clip only through the cross term between its slots.  var, m and v of
    both tables within 1e-5 of each array's scale; the rows that steps 2 and 4 leave alone -- one of the shared table, ten of the other --
    are held on their own (the sweep visits a table once); a second optimiser fed the same data ends bitwise equal."""
    from dir_amd import ops
    c = SA.case(B, K, mode)
    runs = []
    for rep in range(2):
        tabs = [_dev(w) for w in c["w0"]]
        ts = ops.TableSet([tabs[t] for t in SA.SLOT_TABLE])
        assert ts.shared and ts.T == 2 and ts.total_rows == 57
        opt = ops.SparseAdam(ts, SA.B1, SA.B2, SA.EPS, c["clip"], shared=True)
        assert opt.ms[0] is opt.ms[2] and opt.vs[0] is opt.vs[2] and opt.ms[0] is not opt.ms[1]
        for t in range(1, SA.STEPS + 1):
            opt.lr_t = SA.lr_t_of(t)
            opt.step(_dev(c["ids"][t - 1]), _dev(c["grad"][t - 1]))
        torch.cuda.synchronize()
        assert ts.tables[0].data_ptr() == ts.tables[2].data_ptr() == tabs[0].data_ptr() and torch.equal(ts.tables[0], ts.tables[2])
        runs.append({"var": [tabs[0].cpu().numpy(), tabs[1].cpu().numpy()], "m": [opt.ms[0].cpu().numpy(), opt.ms[1].cpu().numpy()],
                     "v": [opt.vs[0].cpu().numpy(), opt.vs[1].cpu().numpy()]})
    got, ref = runs[0], c["ref"]
    errs, rest = {}, {}
    for name in ("var", "m", "v"):
        for i, rows in enumerate((slice(SA.REST_SHARED, SA.REST_SHARED + 1), SA.REST_OWN)):
            errs[name, i] = SA.array_err(got[name][i], ref[name][i])
            rest[name, i] = float(np.abs(got[name][i][rows] - ref[name][i][rows]).max() / np.abs(ref[name][i]).max())
    print("shared adam K=%d B=%d %s (clip %.4g): errors of the array's scale, shared var %.2e m %.2e v %.2e, own var %.2e m %.2e v %.2e; "
          "rows left alone in steps 2 and 4: %.2e; per-slot formulations would be off by norm %.2e steps %.2e sweep %.2e"
          % (K, B, mode, c["clip"], errs["var", 0], errs["m", 0], errs["v", 0], errs["var", 1], errs["m", 1], errs["v", 1],
             max(rest.values()), c["miss"]["norm"], c["miss"]["steps"], c["miss"]["sweep"]))
    assert max(errs.values()) <= BAR, errs
    assert max(rest.values()) <= BAR, rest
    for name in got:
        for a, b in zip(got[name], runs[1][name]):
            assert np.array_equal(a, b), name


# ---- raw calls of the two exports ---------------------------------------------------------------------------------------------------
class _Raw:
    """Tables, m, v and a workspace of their own for raw calls of dir_sparse_adam_f32 / dir_sparse_adam_shared_f32."""

    def __init__(self, w_slots, table_vocab, K, B):
        from dir_amd import _lib
        self.lib = _lib.load()
        self.K, self.F = K, len(w_slots)
        self.tabs = w_slots                                             # per slot (the slots of a table hold the same tensor)
        uniq = {}
        for w in w_slots:
            uniq.setdefault(w.data_ptr(), (torch.zeros_like(w), torch.zeros_like(w)))
        self.ms, self.vs = [uniq[w.data_ptr()][0] for w in w_slots], [uniq[w.data_ptr()][1] for w in w_slots]
        ptrs = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")      # noqa: E731
        self.p_w, self.p_m, self.p_v = ptrs(self.tabs), ptrs(self.ms), ptrs(self.vs)
        self.total_rows = int(sum(table_vocab))
        self.row_base = torch.tensor(np.concatenate([[0], np.cumsum(table_vocab)[:-1]]), dtype=torch.int64, device="cuda")
        self.need = int(self.lib.dir_sparse_adam_workspace_bytes(B, self.F, K, self.total_rows))
        assert self.need > 0
        self.buf = torch.zeros(self.need + 256, dtype=torch.uint8, device="cuda")
        self.first = 1

    def ws(self):
        from dir_amd.sparse_opt import _aligned
        return _aligned(self.buf)[0]

    def call(self, shared, ids, grad, lr_t, clip, slot_table=None, n_tables=None, F=None, K=None, B=None, bytes_=None, first=None):
        """-> rc.  shared: dir_sparse_adam_shared_f32 with (slot_table, n_tables), else dir_sparse_adam_f32."""
        from dir_amd._abi import _ptr, _stream
        F = self.F if F is None else F
        B = (ids.shape[0] if ids is not None else 0) if B is None else B
        args = (_ptr(self.p_w), _ptr(self.p_m), _ptr(self.p_v), F, self.K if K is None else K, _ptr(ids), ids.stride(0) if ids is not None else 0,
                ids.stride(1) if ids is not None else 0, _ptr(grad), grad.stride(0) if grad is not None else 0, lr_t, SA.B1, SA.B2, SA.EPS, clip, B,
                _ptr(self.row_base), self.total_rows, self.ws(), self.need if bytes_ is None else bytes_, self.first if first is None else first,
                _stream())
        if shared:
            rc = self.lib.dir_sparse_adam_shared_f32(*args, _ptr(slot_table), F if n_tables is None else n_tables)
        else:
            rc = self.lib.dir_sparse_adam_f32(*args)
        if rc == 0:
            self.first = 0
        return rc

    def state(self):
        return [t.clone() for t in self.tabs + self.ms + self.vs]


def _batches(rng, vocab, B, K, pruned, steps=2):
    lo, hi = (-1, 1) if pruned else (0, 0)
    return [(_dev(np.stack([rng.integers(lo, v + hi, size=B) for v in vocab], 1).astype(np.int64)),
             _dev((rng.standard_normal((B, len(vocab) * K)) * 0.5).astype(np.float32))) for _ in range(steps)]


# ---- 2. no map: the unshared call, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [300, 4096])
def test_no_map_is_the_existing_export_bit_for_bit(built_lib, B):
    K, vocab = 16, (7, 50, 23)
    rng = np.random.default_rng(B + 2)
    w0 = [_dev((rng.standard_normal((v, K)) * 0.25).astype(np.float32)) for v in vocab]
    a, b = _Raw([w.clone() for w in w0], vocab, K, B), _Raw([w.clone() for w in w0], vocab, K, B)
    for t, (ids, grad) in enumerate(_batches(rng, vocab, B, K, True), 1):          # clip 1.0: active on every table
        assert a.call(False, ids, grad, SA.lr_t_of(t), 1.0) == 0
        assert b.call(True, ids, grad, SA.lr_t_of(t), 1.0, None, 3) == 0
    torch.cuda.synchronize()
    assert not any(torch.equal(x, w) for x, w in zip(a.tabs, w0))
    for x, y in zip(a.state(), b.state()):
        assert torch.equal(x, y)


# ---- 3. an identity map against the existing export -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruned", [False, True], ids=["in_range", "pruned_ids"])
@pytest.mark.parametrize("B", [300, 4096])
def test_identity_map_against_the_existing_export(built_lib, B, pruned):
    """Three distinct tables, map (0, 1, 2): the same keys through the global sort.  Bitwise equal -- except at B >= 4096 WITH pruned ids,
    where the existing export's slot-major sort leaves a slot's pruned entries at the end of that slot's segment, the tiles cut the later
    slots' runs elsewhere and the compensated sums round differently (include/dir_hip.h, the caveat of
    dir_sparse_adagrad_sorted_shared_f32): held to the 1e-5 bar, figure printed."""
    K, vocab = 16, (7, 50, 23)
    rng = np.random.default_rng(B + 3)
    w0 = [_dev((rng.standard_normal((v, K)) * 0.25).astype(np.float32)) for v in vocab]
    ident = torch.arange(3, dtype=torch.int32, device="cuda")
    a, b = _Raw([w.clone() for w in w0], vocab, K, B), _Raw([w.clone() for w in w0], vocab, K, B)
    for t, (ids, grad) in enumerate(_batches(rng, vocab, B, K, pruned), 1):
        assert a.call(False, ids, grad, SA.lr_t_of(t), 1.0) == 0
        assert b.call(True, ids, grad, SA.lr_t_of(t), 1.0, ident, 3) == 0
    torch.cuda.synchronize()
    assert not any(torch.equal(x, w) for x, w in zip(a.tabs, w0))
    if not (pruned and B >= 4096):
        for x, y in zip(a.state(), b.state()):
            assert torch.equal(x, y)
        return
    err = max(SA.array_err(y.cpu().numpy(), x.double().cpu().numpy()) for x, y in zip(a.state(), b.state()))
    print("identity map, B=%d, pruned ids: global sort against slot-major sort %.2e of the array's scale" % (B, err))
    assert err <= BAR, err


# ---- 4. argument checks ------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_touch_nothing(built_lib):
    """Every rejected argument returns its code before the first HIP call: the workspace (filled with 0xFF, first_call = 1: the first HIP
    call would zero the marks), the tables, m and v are untouched.  A map value outside [0, n_tables) prunes its slot's entries; B == 0
    runs the sweep alone."""
    K, B = 16, 300
    c = SA.case(B, K, "active")
    tabs = [_dev(w) for w in c["w0"]]
    r = _Raw([tabs[t] for t in SA.SLOT_TABLE], SA.TABLE_VOCAB, K, B)
    smap = torch.tensor(SA.SLOT_TABLE, dtype=torch.int32, device="cuda")
    ids, grad = _dev(c["ids"][0]), _dev(c["grad"][0])
    r.buf.fill_(0xFF)
    before = r.state()
    lr_t = SA.lr_t_of(1)
    cases = [("a NULL map with n_tables < F", dict(slot_table=None, n_tables=2), -1, b"n_tables"),
             ("n_tables > F", dict(slot_table=smap, n_tables=4), -1, b"n_tables"),
             ("n_tables < 1", dict(slot_table=smap, n_tables=0), -1, b"n_tables"),
             ("F > 64", dict(slot_table=None, n_tables=65, F=65), -4, b"F <= 64"),
             ("K = 6", dict(slot_table=smap, n_tables=2, K=6), -4, b"K"),
             ("K = 12", dict(slot_table=smap, n_tables=2, K=12), -4, b"K"),
             ("a short workspace", dict(slot_table=smap, n_tables=2, bytes_=r.need - 1), -1, b"workspace"),
             ("a negative clip", dict(slot_table=smap, n_tables=2, clip=-1.0), -1, b"hyper")]
    for what, kw, code, word in cases:
        clip = kw.pop("clip", c["clip"])
        rc = r.call(True, ids, grad, lr_t, clip, first=1, **kw)
        assert rc == code and word in r.lib.dir_last_error(), (what, rc, r.lib.dir_last_error())
    torch.cuda.synchronize()
    assert bool((r.buf == 0xFF).all()), "a rejected call wrote the workspace"
    for x, y in zip(before, r.state()):
        assert torch.equal(x, y)
    # a map value outside [0, n_tables): slot 1's entries are pruned, exactly as if its ids were -1
    a_t = [tabs[0].clone(), tabs[1].clone()]
    a = _Raw([a_t[0], a_t[1], a_t[0]], SA.TABLE_VOCAB, K, B)
    b_t = [tabs[0].clone(), tabs[1].clone()]
    b = _Raw([b_t[0], b_t[1], b_t[0]], SA.TABLE_VOCAB, K, B)
    bad_map = torch.tensor([0, 5, 0], dtype=torch.int32, device="cuda")
    ids_off = ids.clone()
    ids_off[:, 1] = -1
    assert a.call(True, ids, grad, lr_t, c["clip"], bad_map, 2) == 0
    assert b.call(True, ids_off, grad, lr_t, c["clip"], smap, 2) == 0
    torch.cuda.synchronize()
    assert not torch.equal(a.tabs[0], tabs[0]) and torch.equal(a.tabs[1], tabs[1])       # (m = v = 0: a zero-gradient step moves nothing)
    for x, y in zip(a.state(), b.state()):
        assert torch.equal(x, y)
    # B == 0: the sweep alone, once per table -- m *= b1, v *= b2, var -= lr_t m / (sqrt(v) + eps) on every row of both tables
    m0, v0, w0 = [x.double().cpu().numpy() for x in (a.ms[0], a.vs[0], a.tabs[0])]
    lr2 = SA.lr_t_of(2)
    assert a.call(True, None, None, lr2, c["clip"], smap, 2, B=0) == 0
    torch.cuda.synchronize()
    b1, b2, eps = float(np.float32(SA.B1)), float(np.float32(SA.B2)), float(np.float32(SA.EPS))
    m1, v1 = m0 * b1, v0 * b2
    w1 = w0 - float(np.float32(lr2)) * m1 / (np.sqrt(v1) + eps)
    errs = [SA.array_err(a.ms[0].cpu().numpy(), m1), SA.array_err(a.vs[0].cpu().numpy(), v1), SA.array_err(a.tabs[0].cpu().numpy(), w1)]
    print("B == 0: the shared table after the sweep alone, m %.2e v %.2e var %.2e of the array's scale" % tuple(errs))
    assert max(errs) <= BAR and float(np.abs(w1 - w0).max()) > 1e-4
    assert a.tabs[0].data_ptr() == a.tabs[2].data_ptr()


# ---- 5. models ----------------------------------------------------------------------------------------------------------------------------
V, KM, BM = 300, 16, 2048
SPEC = dict(optimizer="Adam", optimizer_spec={"epsilon": 1e-4},
            learning_rate_spec={"learning_rate": 0.01, "decay_method": "cosine_decay", "decay_steps": 100, "alpha": 0.5})


def _dcn(straddle=False):
    """6 identity columns of 300 ids, C02 / C03 one shared_embedding_columns pair, K = 16, 3 numeric columns, 2 cross layers, [64, 32],
    Adam with the reference's spec.  straddle: the pair is C00 / C05 and the four columns between them are 8 wide, so the pair's two
    columns are not adjacent in the name-sorted concat and no group owns the shared table."""
    from dir_amd import feature_column as fc
    from dir_amd.dcn import DeepCrossNetwork
    torch.manual_seed(5)
    cats = [fc.categorical_column_with_identity("C%02d" % i, V) for i in range(6)]
    pair = (0, 5) if straddle else (2, 3)
    shared = fc.shared_embedding_columns([cats[i] for i in pair], KM)
    cols = [fc.embedding_column(cats[i], 8 if straddle else KM) for i in range(6) if i not in pair] + shared
    cols += [fc.numeric_column("I%02d" % i) for i in range(3)]
    return DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[64, 32], batch_norm=False, **SPEC).cuda()


def _model_batches(n, multihot=False, pair=(2, 3)):
    from dir_amd import feature_column as fc
    gen = torch.Generator(device="cuda").manual_seed(1)
    out = []
    for _ in range(n):
        ids = torch.randint(0, V, (BM, 6), generator=gen, device="cuda")
        ids[::5, pair[1]] = ids[::5, pair[0]]                            # the same id in both sharing columns
        f = {"C%02d" % i: ids[:, i].contiguous() for i in range(6)}
        if multihot:
            lens = torch.randint(0, 4, (BM,), generator=gen, device="cuda")
            offs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), lens.cumsum(0)])
            f["C%02d" % pair[0]] = fc.Ragged(torch.randint(0, V, (int(offs[-1]),), generator=gen, device="cuda"), offs)
        f.update({"I%02d" % i: torch.rand((BM,), generator=gen, device="cuda") for i in range(3)})
        out.append((f, (torch.rand((BM, 1), generator=gen, device="cuda") < 0.3).float()))
    return out


def _bce(model, f, y):
    return torch.nn.functional.binary_cross_entropy_with_logits(model(f), y)


def _train(hip, batches, straddle=False, watch=None):
    os.environ["DIR_TRAIN_HIP_ADAM"] = "1" if hip else "0"
    try:
        model = _dcn(straddle)
        op = model.train_step()
        if watch is not None:
            watch(model, op)
        for f, y in batches:
            op(_bce(model, f, y))
        torch.cuda.synchronize()
        return model, op, [p.detach().clone() for p in model.parameters()]
    finally:
        del os.environ["DIR_TRAIN_HIP_ADAM"]


def _shared_param(model):
    il = model.input_layer
    (t,) = [t for t in set(il._col_table) if il._col_table.count(t) > 1]
    return il.embedding_weights[t]


def test_dcn_with_a_shared_pair_keeps_the_hip_adam(built_lib):
    batches = _model_batches(3)
    seen = {}

    def watch(model, op):
        shared = _shared_param(model)
        (opt,) = op.sparse_adam                                          # six 16-wide columns, adjacent: one group, one optimiser
        assert opt.ts.shared and opt.ts.F == 6 and opt.ts.T == 5
        assert sum(p is shared for p in opt.owned) == 1 and len(opt.owned) == 5 and len({id(p) for p in opt.owned}) == 5
        assert [opt.ts.slot_table[f] for f in opt.owned_slots] == list(range(5))
        assert all(p is not q for p in op.params for q in opt.owned)     # the torch Adam holds none of the tables
        seen["w0"] = shared.detach().clone()

    model, op, a = _train(True, batches, watch=watch)
    assert all(p.grad is None for p in model.input_layer.embedding_weights), "an owned table kept a .grad"
    assert float((_shared_param(model).detach() - seen["w0"]).abs().max()) > 1e-3
    _, op0, b = _train(False, batches)
    assert op0.sparse_adam == []
    err = max(float((x - y).abs().max()) for x, y in zip(a, b))
    print("DCN with a shared pair, 3 steps at B = %d: HIP Adam against the dense torch formulation, max |difference| %.2e" % (BM, err))
    assert err <= 1e-5


def test_multihot_shared_column_takes_one_table_step(built_lib):
    """The pair's first column multi-hot: the group's lookups take the CSR path, every table's gradient arrives as its sparse .grad --
    the shared table's as the SUM of both columns' -- and TrainStep steps each table once through step_table_grad."""
    batches = _model_batches(3, multihot=True)
    calls = []

    def watch(model, op):
        (opt,) = op.sparse_adam
        inner = opt.step_table_grad

        def counted(f, grad):
            calls.append(opt.ts.slot_table[f])
            return inner(f, grad)

        opt.step_table_grad = counted

    model, _, a = _train(True, batches, watch=watch)
    assert sorted(calls) == sorted(list(range(5)) * 3), calls              # per step: every distinct table once, the shared one included
    assert all(p.grad is None for p in model.input_layer.embedding_weights)
    _, _, b = _train(False, batches)
    err = max(float((x - y).abs().max()) for x, y in zip(a, b))
    print("DCN, multi-hot shared column, 3 steps: step_table_grad against the dense torch formulation, max |difference| %.2e" % err)
    assert err <= 1e-5


def test_straddling_shared_table_still_trains_through_grad(built_lib):
    batches = _model_batches(3, pair=(0, 5))
    seen = {}

    def watch(model, op):
        shared = _shared_param(model)
        assert len(op.sparse_adam) == 1 and not op.sparse_adam[0].ts.shared and op.sparse_adam[0].ts.K == 8
        assert all(p is not shared for o in op.sparse_adam for p in o.owned) and any(p is shared for p in op.params)
        seen["w0"] = shared.detach().clone()

    model, _, a = _train(True, batches, straddle=True, watch=watch)
    assert float((_shared_param(model).detach() - seen["w0"]).abs().max()) > 1e-3
    _, _, b = _train(False, batches, straddle=True)
    err = max(float((x - y).abs().max()) for x, y in zip(a, b))
    print("DCN, straddling shared table, 3 steps: max |difference| to the dense torch formulation %.2e" % err)
    assert err <= 1e-5


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_bitwise_the_eager_step(built_lib):
    """Forward, loss and backward of the DCN with the fused shared Adam inside (the embedding update IS part of backward), captured after
    eager warm-up steps: two replays from one state and the eager step from that state end bitwise equal -- tables, m and v."""
    from dir_amd import ops
    (feats, y), = _model_batches(1)
    model = _dcn().train()
    (opt,), owned = model.input_layer.fused_sparse_adam(SA.B1, SA.B2, SA.EPS, 100.0, shared=True)
    assert opt.ts.shared and len(owned) == 5
    opt.lr_t = SA.lr_t_of(3)
    dense = [p for p in model.parameters() if all(p is not q for q in owned)]

    def step():
        for p in dense:
            p.grad = None
        loss = _bce(model, feats, y)
        loss.backward()
        return loss.detach()

    first = [opt.ts.slots_of(t)[0] for t in range(opt.ts.T)]
    state = [opt.ts.tables[f] for f in first] + [opt.ms[f] for f in first] + [opt.vs[f] for f in first]
    graph = ops.CapturedStep(step, written=ops.written_of(model), warmup=1)
    saved = [t.clone() for t in state]

    def run(fn):
        with torch.no_grad():
            for t, s in zip(state, saved):
                t.copy_(s)
        fn()
        torch.cuda.synchronize()
        return [t.clone() for t in state]

    r1, r2, eager = run(graph.replay), run(graph.replay), run(step)
    assert not any(torch.equal(a, s) for a, s in zip(r1[:5], saved[:5]))
    for a, b, c in zip(r1, r2, eager):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert all(p.grad is None for p in owned)


# ---- 7. the state of a shared table is saved once ---------------------------------------------------------------------------------------------
def test_state_round_trip_saves_a_shared_table_once(built_lib):
    from dir_amd import ops
    K, B = 16, 300
    c = SA.case(B, K, "active")

    def fresh(w):
        tabs = [w[0].clone(), w[1].clone()]
        return tabs, ops.SparseAdam(ops.TableSet([tabs[t] for t in SA.SLOT_TABLE]), SA.B1, SA.B2, SA.EPS, c["clip"], shared=True)

    def step(opt, t):
        opt.lr_t = SA.lr_t_of(t)
        opt.step(_dev(c["ids"][t - 1]), _dev(c["grad"][t - 1]))

    ta, A = fresh([_dev(w) for w in c["w0"]])
    step(A, 1), step(A, 2)
    state = A.state_dict()
    assert len(state["m"]) == len(state["v"]) == 2 and state["steps"] == 2          # one m / v per distinct table
    assert [tuple(m.shape) for m in state["m"]] == [(7, K), (50, K)]
    tb, Bo = fresh(ta)                                                    # the tables as they stand after step 2, zero m / v
    Bo.load_state_dict(state)
    assert Bo.ms[0] is Bo.ms[2] and torch.equal(Bo.ms[0], A.ms[0]) and torch.equal(Bo.vs[1], A.vs[1]) and Bo.steps == 2
    step(A, 3), step(Bo, 3)
    torch.cuda.synchronize()
    assert not torch.equal(state["m"][0], A.ms[0])                        # (the saved state is a copy)
    for x, z in zip(ta + [A.ms[0], A.ms[1], A.vs[0], A.vs[1]], tb + [Bo.ms[0], Bo.ms[1], Bo.vs[0], Bo.vs[1]]):
        assert torch.equal(x, z)
    with pytest.raises(ValueError, match="tables"):
        Bo.load_state_dict({"m": state["m"][:1], "v": state["v"][:1], "steps": 0})
