"""Tables shared between slots (feature_column.shared_embedding_columns) on the GPU: the sorted Adagrad step over a sharing TableSet
against float64 (a), bit for bit against the one-slot form of the same entries (b), the new export on a set without sharing (c), the
forward of models that share a table against twins that duplicate it (d), one fused training step of a shared DeepFM (e) and
InputLayer's grouping around a shared table (f).  The inputs of (a) and their conditions: tests/shared_embedding_inputs.py."""
import numpy as np
import pytest
import torch

from tests import shared_embedding_inputs as SI
from tests.hot_rows_inputs import BAR, scaled

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- (a) the kernel against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["plain", "packed_fm"])
@pytest.mark.parametrize("B", [300, 4096, 8192])
@pytest.mark.parametrize("K", [4, 16])
def test_shared_adagrad_step_matches_float64(built_lib, K, B, layout):
    """Slots 0 and 2 on one 7-row table, slot 1 (50 rows) between them: every row of the shared table collects entries from both slots
    (B = 8192: some 2 300 per row, runs across many 256-entry tiles), and takes ONE Adagrad step with their sum.  300 takes the plain
    sort, 4096 is where a set without sharing switches to the slot-major sort.  packed_fm: packed [embedding | accumulator] rows with
    the FM backward folded into the update."""
    from dir_amd import ops
    fm = layout == "packed_fm"
    c = SI.case(B, K, fm)                                                # (asserts the two conditions on the inputs)
    tabs = [_dev(w) for w in c["w0"]]
    per_slot = [tabs[t] for t in SI.SLOT_TABLE]
    ids, grad = _dev(c["ids"]), _dev(c["grad"])
    if fm:
        ts = ops.TableSet.train_rows(per_slot, 0.1)
        assert ts.shared and ts.slot_table == list(SI.SLOT_TABLE) and ts.tables[0].data_ptr() == ts.tables[2].data_ptr()
        assert ts.arena.numel() == sum(SI.TABLE_VOCAB) * 2 * K + 32        # the shared table's rows lie in the arena once
        for t, slot in enumerate((0, 1)):
            ts.accums[slot].copy_(_dev(c["a0"][t]))
        opt = ops.SparseAdagrad(ts, lr=SI.LR)
        fsum = torch.empty((B, K), device="cuda")
        emb, _ = ops.gather_fm(ts, ids, fsum=fsum)
        assert np.array_equal(emb.cpu().numpy(), SI.gathered([c["w0"][t] for t in SI.SLOT_TABLE], c["ids"]))
        opt.step_fm(ids, grad, _dev(c["fm_g"]), fsum)
    else:
        ts = ops.TableSet(per_slot)
        assert ts.shared and ts.T == 2 and ts.total_rows == 57 and ts.nbytes == 57 * K * 4
        opt = ops.SparseAdagrad(ts, lr=SI.LR)
        assert opt.accums[0] is opt.accums[2]
        for t, slot in enumerate((0, 1)):
            opt.accums[slot].copy_(_dev(c["a0"][t]))
        opt.step(ids, grad)
    torch.cuda.synchronize()
    errs = []
    for t, slot in enumerate((0, 1)):
        errs += [scaled(ts.tables[slot].cpu().numpy(), c["ref_w"][t]), scaled(opt.accums[slot].cpu().numpy(), c["ref_a"][t])]
    print("shared adagrad K=%d B=%d %s: scaled errors (w, a) shared %.2e %.2e, own %.2e %.2e; slot-by-slot would be %.2e %.2e off"
          % ((K, B, layout) + tuple(errs) + c["miss"]))
    assert max(errs) <= BAR, errs
    assert torch.equal(ts.tables[0], ts.tables[2])


def test_chains_refuse_a_sharing_set(built_lib):
    from dir_amd import ops
    t = torch.zeros((7, 4), device="cuda")
    with pytest.raises(ValueError, match="shared"):
        ops.SparseAdagrad(ops.TableSet([t, t]), lr=0.1, method="chains")
    with pytest.raises(ValueError, match="shared"):
        ops.SparseAdam(ops.TableSet([t, t]))


# ---- (b) bit for bit the one-slot form of the same entries ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [300, 4096])
def test_shared_step_is_bitwise_the_one_slot_step(built_lib, B):
    """F = 2, both slots on one table: entry e = b*2 + f of the shared call is entry e of the one-slot call on ids.reshape(2B, 1) --
    the same keys, the same stable order, the same tiles, the same compensated sums."""
    from dir_amd import ops
    K, V = 16, 37
    rng = np.random.default_rng(B)
    ids = _dev(rng.integers(-1, V + 1, size=(B, 2)).astype(np.int64))
    grad = _dev((rng.standard_normal((B, 2 * K)) * 0.5).astype(np.float32))
    w0 = _dev((rng.standard_normal((V, K)) * 0.25).astype(np.float32))
    a0 = _dev(rng.uniform(0.1, 1.0, size=(V, K)).astype(np.float32))
    ws, w1 = w0.clone(), w0.clone()
    shared = ops.SparseAdagrad(ops.TableSet([ws, ws]), lr=0.05)
    one = ops.SparseAdagrad(ops.TableSet([w1]), lr=0.05)
    shared.accums[0].copy_(a0)
    one.accums[0].copy_(a0)
    shared.step(ids, grad)
    one.step(ids.reshape(2 * B, 1), grad.reshape(2 * B, K))
    torch.cuda.synchronize()
    assert not torch.equal(ws, w0)
    assert torch.equal(ws, w1) and torch.equal(shared.accums[0], one.accums[0])


# ---- (c) a set without sharing through the new export ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pruned", [False, True], ids=["in_range", "pruned_ids"])
@pytest.mark.parametrize("B", [300, 4096])
def test_identity_map_against_the_existing_export(built_lib, B, pruned):
    """A set without sharing through the new export -- with an identity map, then with no map -- against the existing export.  No map
    is the existing call (same sort) and is bitwise equal always.  An identity map takes the global sort: the same keys in the same stable
    order, so bitwise equal too -- except at B >= RSS_MIN_B = 4096 WITH pruned ids, where the existing export's slot-major sort leaves a
    slot's pruned entries at the end of that slot's segment (csrc/radix_sort.hip) while the global sort puts them behind every row: the
    live entries of the later slots stand at other positions, the 256-entry tiles cut their runs elsewhere, and the compensated sums of
    a run's pieces round differently.  Both results are then the same sums to about an ulp: held to the 1e-5 bar, figure printed."""
    from dir_amd import ops, _lib
    from dir_amd._abi import _ptr, _stream
    K, vocab = 16, (7, 50, 23)
    rng = np.random.default_rng(B + 1)
    ids = _dev(np.stack([rng.integers(-1 if pruned else 0, v + 1 if pruned else v, size=B) for v in vocab], 1).astype(np.int64))
    grad = _dev((rng.standard_normal((B, 3 * K)) * 0.5).astype(np.float32))
    w0 = [_dev((rng.standard_normal((v, K)) * 0.25).astype(np.float32)) for v in vocab]
    lib = _lib.load()
    for ident in (torch.arange(3, dtype=torch.int32, device="cuda"), None):
        a = ops.SparseAdagrad(ops.TableSet([w.clone() for w in w0]), lr=0.05)
        b = ops.SparseAdagrad(ops.TableSet([w.clone() for w in w0]), lr=0.05)
        assert not a.ts.shared and a.ts.slot_table_dev is None
        a.step(ids, grad)
        ts = b.ts
        ws, need, _ = b._sort_area("test", lib.dir_sparse_adagrad_sorted_workspace_bytes, B, ts.F, ts.K)
        _lib.check(lib.dir_sparse_adagrad_sorted_shared_f32(_ptr(ts.ptrs), _ptr(b.acc_ptrs), ts.F, ts.K, _ptr(ids), ids.stride(0), ids.stride(1),
                                                            _ptr(grad), grad.stride(0), b.lr, B, _ptr(b.row_base), b.total_rows, _ptr(ident), 3,
                                                            ws, need, _stream()))
        torch.cuda.synchronize()
        exact = ident is None or not (pruned and B >= 4096)
        for f in range(3):
            assert not torch.equal(a.ts.tables[f], w0[f])
            if exact:
                assert torch.equal(a.ts.tables[f], b.ts.tables[f]) and torch.equal(a.accums[f], b.accums[f]), f
            else:
                err = max(scaled(b.ts.tables[f].cpu().numpy(), a.ts.tables[f].cpu().numpy()), scaled(b.accums[f].cpu().numpy(), a.accums[f].cpu().numpy()))
                print("identity map, B=%d, pruned ids, table %d: global sort against slot-major sort %.2e" % (B, f, err))
                assert err <= BAR, (f, err)
    rc = lib.dir_sparse_adagrad_sorted_shared_f32(_ptr(b.ts.ptrs), _ptr(b.acc_ptrs), 3, K, _ptr(ids), ids.stride(0), ids.stride(1), _ptr(grad),
                                                  grad.stride(0), b.lr, B, _ptr(b.row_base), b.total_rows, None, 2, ws, need, _stream())
    assert rc == -1 and b"n_tables" in lib.dir_last_error()


# ---- models on [user, pos, neg], pos / neg on one table ----------------------------------------------------------------------------------
KM, V_USER, V_ITEM = 16, 20, 30


def _model(kind, shared, names=("user", "pos", "neg"), user_dim=KM):
    """DeepFM (fm_embedding_size 16, hidden [32, 32]) or DCN over the three columns; shared: pos / neg through shared_embedding_columns,
    else every column its own table (the twin).  Linear weights and biases are drawn so that no term is zero."""
    from dir_amd import feature_column as fc
    from dir_amd.dcn import DeepCrossNetwork
    from dir_amd.deepfm import DeepFM
    cats = [fc.categorical_column_with_identity(names[0], V_USER), fc.categorical_column_with_identity(names[1], V_ITEM),
            fc.categorical_column_with_identity(names[2], V_ITEM)]
    items = fc.shared_embedding_columns(cats[1:], KM) if shared else [fc.embedding_column(c, KM) for c in cats[1:]]
    cols = [fc.embedding_column(cats[0], user_dim)] + items
    if kind == "deepfm":
        model = DeepFM(linear_feature_columns=cats, dnn_feature_columns=cols, dnn_hidden_units=[32, 32], fm_embedding_size=KM)
    else:
        model = DeepCrossNetwork(columns=cols, cross_layer_num=2, dnn_hidden_units=[32, 32])
    return model.cuda()


def _slot_params(model):
    """The embedding parameters per column, in the model's own column order."""
    return model._slot_weights() if hasattr(model, "_slot_weights") else model.input_layer._col_weights()


def _twin_of(model, kind, **kw):
    """The same model with the shared table duplicated into two parameters: every other parameter and buffer copied."""
    twin = _model(kind, False, **kw)
    src, dst = model.state_dict(), twin.state_dict()
    with torch.no_grad():
        for k, v in dst.items():
            if "embedding_weights" not in k:
                v.copy_(src[k])
        for p, q in zip(_slot_params(twin), _slot_params(model)):
            p.copy_(q)
    return twin


def _randomize(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "linear" in n or n.endswith("bias") or n.startswith("cross"):
                p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(p.device))


def _features(B, multihot, seed, names=("user", "pos", "neg")):
    from dir_amd import feature_column as fc
    rng = np.random.default_rng(seed)
    user = rng.integers(0, V_USER, size=B)
    neg = rng.integers(0, V_ITEM, size=B)
    neg[::7] = -1                                                       # pruned (B = 1: its only id)
    feats = {names[0]: _dev(user.astype(np.int64)), names[2]: _dev(neg.astype(np.int64))}
    if multihot:
        lens = rng.integers(0, 4, size=B)
        lens[0] = 3
        vals = rng.integers(-1, V_ITEM, size=int(lens.sum()))
        offs = np.concatenate([[0], np.cumsum(lens)])
        feats[names[1]] = fc.Ragged(_dev(vals.astype(np.int64)), _dev(offs.astype(np.int64)))
    else:
        pos = rng.integers(0, V_ITEM, size=B)
        pos[::5] = neg[::5]                                             # the same id in both sharing columns
        feats[names[1]] = _dev(pos.astype(np.int64))
    return feats


# ---- (d) forward: a shared table reads like a duplicated one ----------------------------------------------------------------------------
@pytest.mark.parametrize("multihot", [False, True], ids=["onehot", "multihot_pos"])
@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("kind", ["deepfm", "dcn"])
def test_shared_forward_is_bitwise_the_duplicated_twin(built_lib, kind, B, multihot):
    model = _model(kind, True)
    _randomize(model, 3)
    twin = _twin_of(model, kind)
    assert len(list(model.parameters())) + 1 == len(list(twin.parameters()))
    feats = _features(B, multihot, 11 + B)
    model.eval(), twin.eval()
    outs = []
    for m in (model, twin):
        got = {}
        pred = m.predict(feats)                                          # DeepFM one-hot: packed serving rows / the one-launch tower
        got["predict"] = [pred[k].clone() for k in sorted(pred)]
        if kind == "deepfm" and not multihot:
            assert m._packed is not None, "the packed serving layout was not built"
        with torch.no_grad():
            m.hparams["serving_layout"] = None                           # the reference layout's kernels
            got["no_grad"] = [m(feats).clone()]
            m.hparams.pop("serving_layout")
        m.train()
        got["grad"] = [m(feats).detach().clone()]
        m.eval()
        outs.append(got)
    torch.cuda.synchronize()
    for k in outs[0]:
        for a, b in zip(outs[0][k], outs[1][k]):
            assert a.shape[0] == B and bool(torch.isfinite(a.float()).all())
            assert torch.equal(a, b), k
    assert float(outs[0]["grad"][0].abs().max()) > 0


def test_shared_forward_with_max_norm_and_gather_fm(built_lib):
    """The remaining forward entries on a sharing TableSet against the set with the table duplicated: embedding_bag with max_norm, one-hot
    and multi-hot, and gather_fm."""
    from dir_amd import ops
    rng = np.random.default_rng(5)
    B, K = 257, 16
    user, item = _dev((rng.standard_normal((V_USER, K))).astype(np.float32)), _dev((rng.standard_normal((V_ITEM, K))).astype(np.float32))
    shared, dup = ops.TableSet([user, item, item]), ops.TableSet([user, item, item.clone()])
    assert shared.shared and not dup.shared and shared.nbytes < dup.nbytes and shared.range_ok() == dup.range_ok()
    ids = _dev(np.stack([rng.integers(-1, v, size=B) for v in (V_USER, V_ITEM, V_ITEM)], 1).astype(np.int64))
    for a, b in zip(ops.gather_fm(shared, ids), ops.gather_fm(dup, ids)):
        assert torch.equal(a, b)
    assert torch.equal(ops.embedding_bag(shared, ids, max_norm=0.8), ops.embedding_bag(dup, ids, max_norm=0.8))
    lens = rng.integers(0, 4, size=3 * B)
    vals = _dev(rng.integers(-1, V_USER, size=int(lens.sum())).astype(np.int64))
    offs = _dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    kw = dict(combiner=["sum", "mean", "sqrtn"], field_major=True, max_norm=[None, 0.8, 0.5])
    assert torch.equal(ops.embedding_bag(shared, vals, offs, **kw), ops.embedding_bag(dup, vals, offs, **kw))


# ---- (e) one fused training step of the shared DeepFM --------------------------------------------------------------------------------------
LR, ACC0 = 0.05, 0.1


def _adagrad64(w0, grad, lr=LR, acc0=ACC0):
    """The float64 Adagrad rule on a summed (coalesced) sparse gradient: -> (table, accumulator), untouched rows as they were."""
    g = grad.coalesce()
    rows = g.indices()[0].cpu().numpy()
    G = g.values().double().cpu().numpy()
    w, acc = w0.detach().double().cpu().numpy().copy(), np.full(tuple(w0.shape), acc0, np.float64)
    acc[rows] += G * G
    w[rows] -= lr * G / np.sqrt(acc[rows])
    return w, acc


def _loss(model, feats, y):
    return torch.nn.functional.binary_cross_entropy_with_logits(model(feats), y, reduction="sum")


@pytest.mark.parametrize("packed", [False, True], ids=["split", "packed"])
def test_shared_deepfm_fused_step_and_graph_replay(built_lib, packed):
    import copy
    from dir_amd import ops
    B = 257
    model = _model("deepfm", True)
    _randomize(model, 7)
    plain = copy.deepcopy(model)                                        # the same model without a fused optimiser: the summed .grad
    feats = _features(B, False, 23)
    y = (_dev(np.random.default_rng(1).random((B, 1)).astype(np.float32)) < 0.4).float()
    _loss(plain.train(), feats, y).backward()
    torch.cuda.synchronize()
    w0 = [p.detach().clone() for p in plain.embedding_weights]
    assert len(w0) == 2 and plain.embedding_weights[1].grad.is_sparse
    ref = [_adagrad64(w, p.grad) for w, p in zip(w0, plain.embedding_weights)]
    assert float(np.abs(ref[1][0] - w0[1].double().cpu().numpy()).max()) > 1e-3          # the shared table does move

    opt = model.train().fused_sparse_adagrad(LR, ACC0, packed=packed)
    ts = opt.ts
    assert ts.shared and ts.slot_table == [0, 1, 1]
    if packed:
        assert ts.arena.numel() == (V_USER + V_ITEM) * 2 * KM + 32       # the shared table's rows lie in the arena once
        assert ts.tables[1].data_ptr() == ts.tables[2].data_ptr() and ts.accums[1].data_ptr() == ts.accums[2].data_ptr()
        assert ts.tables[1].untyped_storage().data_ptr() == ts.arena.untyped_storage().data_ptr()
        assert model.embedding_weights[1].data_ptr() == ts.tables[1].data_ptr()
    dense = [p for n, p in model.named_parameters() if "embedding_weights" not in n]

    def step():
        for p in dense:
            p.grad = None
        loss = _loss(model, feats, y)
        loss.backward()
        return loss.detach()

    step()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in model.embedding_weights)          # the fused update took the gradients
    errs = []
    for t, slot in enumerate((0, 1)):
        errs += [scaled(ts.tables[slot].cpu().numpy(), ref[t][0]), scaled(opt.accums[slot].cpu().numpy(), ref[t][1])]
    print("shared DeepFM step (%s): scaled errors user w %.2e a %.2e, shared w %.2e a %.2e" % (("packed" if packed else "split",) + tuple(errs)))
    assert max(errs) <= BAR, errs

    # the same step from a captured graph, replayed twice from one state, and eagerly from that state: bitwise equal
    # (packed: the row blocks [embedding | accumulator], not the arena -- its alignment gap and tail are never written and may hold NaN bit
    # patterns left by the allocator, which torch.equal tells apart from themselves)
    state = [ts.rows[0], ts.rows[1]] if packed else [ts.tables[0], ts.tables[1], opt.accums[0], opt.accums[1]]
    graph = ops.CapturedStep(step, written=ops.written_of(model))

    def run(fn):
        with torch.no_grad():
            for t, s in zip(state, saved):
                t.copy_(s)
        fn()
        torch.cuda.synchronize()
        return [t.clone() for t in state]

    saved = [t.clone() for t in state]
    r1, r2, eager = run(graph.replay), run(graph.replay), run(step)
    assert not any(torch.equal(a, s) for a, s in zip(r1[:2], saved[:2]))
    for a, b, c in zip(r1, r2, eager):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---- (f) InputLayer: a shared table whose columns are not adjacent keeps its sparse .grad --------------------------------------------------
def test_input_layer_leaves_a_straddling_shared_table_to_autograd(built_lib):
    import copy
    from dir_amd import autograd as ag
    names = ("b_user", "a_item", "c_item")            # sorted concat: a_item_shared_embedding, b_user_embedding (8 wide), c_item_shared_embedding
    B = 257
    model = _model("dcn", True, names=names, user_dim=8)
    _randomize(model, 9)
    il = model.input_layer
    assert [c.name for c in il.emb_cols] == ["a_item_shared_embedding", "b_user_embedding", "c_item_shared_embedding"]
    assert il._col_table == [0, 1, 0] and len(il.embedding_weights) == 2
    plain = copy.deepcopy(model)
    feats = _features(B, False, 31, names=names)
    y = (_dev(np.random.default_rng(2).random((B, 1)).astype(np.float32)) < 0.4).float()
    _loss(plain.train(), feats, y).backward()
    shared_p, user_p = il.embedding_weights[0], il.embedding_weights[1]
    ref_shared = _adagrad64(shared_p, plain.input_layer.embedding_weights[0].grad)
    ref_user = _adagrad64(user_p, plain.input_layer.embedding_weights[1].grad)

    opts = il.fused_sparse_adagrad(LR, ACC0)
    assert len(il._tablesets()) == 3 and len(opts) == 1                  # the two 16-wide columns are not adjacent: three groups
    assert all(t.data_ptr() != shared_p.data_ptr() for o in opts for t in o.ts.tables)      # no fused optimiser owns the shared table
    assert opts[0].ts.tables[0].data_ptr() == user_p.data_ptr()
    rest = ag.Adagrad([shared_p], lr=LR, initial_accumulator_value=ACC0, eps=0.0)
    _loss(model.train(), feats, y).backward()
    assert user_p.grad is None and shared_p.grad is not None and shared_p.grad.is_sparse
    rest.step()
    torch.cuda.synchronize()
    errs = [scaled(shared_p.detach().cpu().numpy(), ref_shared[0]), scaled(rest.state[shared_p]["sum"].cpu().numpy(), ref_shared[1]),
            scaled(user_p.detach().cpu().numpy(), ref_user[0]), scaled(opts[0].accums[0].cpu().numpy(), ref_user[1])]
    print("InputLayer step: scaled errors shared w %.2e a %.2e, user w %.2e a %.2e" % tuple(errs))
    assert max(errs) <= BAR, errs
    assert float(np.abs(ref_shared[0] - plain.input_layer.embedding_weights[0].detach().double().cpu().numpy()).max()) > 1e-3
    # adjacent sharing columns ARE one group, owned by one fused optimiser
    adj = _model("dcn", True).input_layer                                # neg_..., pos_..., user_...: all 16 wide, one run
    got = adj.fused_sparse_adagrad(LR, ACC0)
    assert len(got) == 1 and got[0].ts.shared and got[0].ts.slot_table == [0, 0, 1]
    assert adj.fused_sparse_adam()[0] == []                              # the HIP Adam skips a group that shares a table
