"""Host side of the fused sparse Adam over tables shared between slots (no GPU): the new export is declared, documented, exported and
bound with the header's argument count; it rejects every bad argument before any HIP call (on a machine without a GPU a HIP call would
return DIR_E_HIP, not the argument's code); InputLayer.fused_sparse_adam's bookkeeping around a shared table, with stand-ins for the
device parts as in tests/test_shared_embedding_host.py; TrainStep's loop visits a shared parameter once."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dir_amd import feature_column as fc
from dir_amd import input_layer as IL
from dir_amd import ops, sparse_opt
from dir_amd.dcn import DeepCrossNetwork

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dir_sparse_adam_shared_f32"
BADARG, UNSUPPORTED = -1, -4
f32 = ctypes.c_float


def _err(lib):
    return lib.dir_last_error().decode()


def test_header_export_and_binding_agree(built_lib):
    from dir_amd import _lib
    src = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {n: re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % n, code) for n in (NAME, "dir_sparse_adam_f32")}
    assert decl[NAME], "%s is not declared in include/dir_hip.h" % NAME
    assert hasattr(built_lib, NAME), "libdir_hip.so does not export %s" % NAME
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == decl[NAME].group(1).count(",") + 1
    # dir_sparse_adam_f32 with two TRAILING arguments: the same parameter list, then the map and the table count
    norm = lambda s: [re.sub(r"\s+", " ", a).strip() for a in s.split(",")]      # noqa: E731
    assert norm(decl[NAME].group(1)) == norm(decl["dir_sparse_adam_f32"].group(1)) + ["const int32_t* slot_table", "int n_tables"]
    assert list(argtypes) == list(_lib.SIGNATURES["dir_sparse_adam_f32"][1]) + [ctypes.c_void_p, ctypes.c_int32]
    assert NAME in src.split(decl[NAME].group(0))[0], "%s is not documented above its declaration" % NAME
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_rejected_arguments_return_before_any_hip_call(built_lib):
    lib = built_lib
    buf = np.zeros(1 << 16, np.int64)                 # a stand-in address: every call below fails before it is dereferenced
    p = ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)

    def call(**kw):
        a = dict(tables=p, ms=p, vs=p, F=3, K=16, ids=p, sb=3, sf=1, grad=p, grad_ld=48, lr_t=f32(0.01), b1=f32(0.9), b2=f32(0.999),
                 eps=f32(1e-4), clip=f32(100.0), B=32, rb=p, total=57, ws=p, ws_bytes=1 << 19, first=1, stream=None, slot_table=p,
                 n_tables=2)
        a.update(kw)
        return lib.dir_sparse_adam_shared_f32(*a.values())
    need = lib.dir_sparse_adam_workspace_bytes(32, 3, 16, 57)
    assert 0 < need <= 1 << 19
    assert call(slot_table=None) == BADARG and NAME in _err(lib) and "n_tables" in _err(lib)       # no map, yet fewer tables than slots
    assert call(n_tables=4) == BADARG and NAME in _err(lib) and "n_tables=4" in _err(lib)
    assert call(n_tables=0) == BADARG and "n_tables=0" in _err(lib)
    assert call(F=65, n_tables=65, slot_table=None) == UNSUPPORTED and NAME in _err(lib) and "F=65" in _err(lib)
    assert call(F=65, n_tables=2) == UNSUPPORTED and "F=65" in _err(lib)
    assert call(F=0, n_tables=0) == BADARG and NAME in _err(lib)
    for K in (6, 12, 0, 48):
        assert call(K=K, grad_ld=3 * K) in (UNSUPPORTED, BADARG) and NAME in _err(lib), K
    assert call(K=6, grad_ld=18) == UNSUPPORTED and call(K=48, grad_ld=144) == UNSUPPORTED
    assert call(ws_bytes=need - 1) == BADARG and "workspace" in _err(lib) and NAME in _err(lib)
    assert call(ws=ctypes.c_void_p(p.value + 16)) == BADARG and "256-byte" in _err(lib)
    for arg in ("tables", "ms", "vs", "rb", "ws", "ids", "grad"):
        assert call(**{arg: None}) == BADARG and NAME in _err(lib), arg
    assert call(grad_ld=47) == BADARG and call(B=-1) == BADARG
    assert call(clip=f32(-1.0)) == BADARG and "hyper" in _err(lib)
    assert call(b1=f32(1.0)) == BADARG and call(eps=f32(0.0)) == BADARG
    assert call(total=0) == BADARG and call(total=(1 << 32) - 1) == BADARG                          # (no workspace size for such a key range)
    assert not buf.any()


def _layer(names=("user", "pos", "neg"), user_dim=8):
    cats = [fc.categorical_column_with_identity(names[0], 20), fc.categorical_column_with_identity(names[1], 30),
            fc.categorical_column_with_identity(names[2], 30)]
    cols = [fc.embedding_column(cats[0], user_dim)] + fc.shared_embedding_columns(cats[1:], 8)
    return DeepCrossNetwork(columns=cols, cross_layer_num=1, dnn_hidden_units=[8]).input_layer


class _FakeDevice:
    type = "cuda"


class _StandIn:
    """What fused_sparse_adam builds per group, without a device: records the set it was given."""

    def __init__(self, ts, *hyper, shared=False):
        self.ts, self.hyper, self.shared = ts, hyper, shared

    def attach(self):
        self.ts.grad_sink = "adam"
        return self

    @staticmethod
    def covers(ts):
        return sparse_opt.SparseAdam.covers(ts)


@pytest.fixture
def on_host(monkeypatch):
    """CPU tensors through ops.TableSet (its device check off), the groups' device reported as a GPU, SparseAdam replaced by _StandIn."""
    monkeypatch.setattr(ops, "_dev", lambda t, dtype, name: t)
    monkeypatch.setattr(ops, "SparseAdam", _StandIn)
    real = IL.InputLayer._tablesets

    def tablesets(self):
        groups = real(self)
        for g in groups:
            g[0].device = _FakeDevice()
        return groups

    monkeypatch.setattr(IL.InputLayer, "_tablesets", tablesets)


def test_fused_sparse_adam_owns_a_shared_parameter_once(on_host):
    il = _layer()                                       # sorted concat: neg_shared, pos_shared, user -- all 8 wide: one group
    assert il._col_table == [0, 0, 1] and il._owns_its_tables([0, 1, 2])
    assert il.fused_sparse_adam(0.9, 0.999, 1e-4, 100.0) == ([], [])      # a sharing group is opted into
    opts, owned = il.fused_sparse_adam(0.9, 0.999, 1e-4, 100.0, shared=True)
    assert len(opts) == 1 and opts[0].hyper == (0.9, 0.999, 1e-4, 100.0) and opts[0].shared
    ts = opts[0].ts
    assert ts.shared and ts.slot_table == [0, 0, 1] and ts.T == 2 and ts.total_rows == 50
    shared_p, user_p = il.embedding_weights[0], il.embedding_weights[1]
    assert len(owned) == 2 and owned[0] is shared_p and owned[1] is user_p
    assert opts[0].owned == owned and opts[0].owned_slots == [0, 2]
    assert ts.grad_sink == "adam" and len(ts.owners) == 2


def test_a_straddling_shared_table_keeps_its_grad(on_host):
    il = _layer(names=("b_user", "a_item", "c_item"), user_dim=4)       # a_item_shared (8), b_user (4), c_item_shared (8): three groups
    assert il._col_table == [0, 1, 0]
    opts, owned = il.fused_sparse_adam(shared=True)
    assert len(il._tablesets()) == 3 and len(opts) == 1
    assert owned == [il.embedding_weights[1]] and opts[0].owned_slots == [0] and not opts[0].ts.shared
    assert all(g[0].grad_sink is None for g in il._tablesets() if g[0] is not opts[0].ts)


def test_unshared_layer_lists_every_slot(on_host):
    cats = [fc.categorical_column_with_identity("C%d" % i, 10 + i) for i in range(3)]
    il = DeepCrossNetwork(columns=[fc.embedding_column(c, 8) for c in cats], cross_layer_num=1, dnn_hidden_units=[8]).input_layer
    opts, owned = il.fused_sparse_adam()
    assert len(opts) == 1 and opts[0].owned_slots == [0, 1, 2] and len(owned) == 3 and not opts[0].ts.shared


def test_sparse_adam_accepts_a_sharing_set_and_steps_a_shared_table_once(monkeypatch):
    """The constructor on CPU tensors (device checks off): one m / v per table, the halves refuse by name; step_table_grad with the summed
    sparse .grad of a shared table is ONE tf.train.AdamOptimizer step, and TrainStep's loop calls it once per table."""
    monkeypatch.setattr(ops, "_dev", lambda t, dtype, name: t)
    K = 4
    g = torch.Generator().manual_seed(3)
    item, user = torch.randn((7, K), generator=g), torch.randn((5, K), generator=g)
    ts = ops.TableSet([item, user, item])
    assert ts.shared and ts.slot_table == [0, 1, 0]
    with pytest.raises(ValueError, match="shared"):
        sparse_opt.SparseAdam(ts, 0.9, 0.999, 1e-4, 1.0)               # a sharing set is opted into
    opt = sparse_opt.SparseAdam(ts, 0.9, 0.999, 1e-4, 1.0, shared=True)
    assert opt.ms[0] is opt.ms[2] and opt.vs[0] is opt.vs[2] and opt.ms[1] is not opt.ms[0] and len(opt._slots) == 4
    assert opt.total_rows == 12 and sparse_opt.SparseAdam.covers(ts)
    for half in (opt.norm_payload, opt.step_payload):
        with pytest.raises(ValueError, match="SparseAdam.*shared"):
            half(None, None)
    for half in (opt.norm_bags, opt.step_bags):
        with pytest.raises(ValueError, match="SparseAdam.*shared"):
            half(None, 1, 1, 1, None)
    state = opt.state_dict()
    assert len(state["m"]) == len(state["v"]) == 2
    # one step of the shared table from the SUM of its two columns' sparse gradients
    rows = torch.tensor([[1, 3, 1, 6]])
    vals = torch.randn((4, K), generator=g)
    grad = torch.sparse_coo_tensor(rows, vals, (7, K))
    opt.lr_t = 0.01
    w0 = item.clone().double()
    opt.step_table_grad(2, grad)                        # through its second slot: the same table, m and v
    dense = grad.to_dense().double()
    dense = dense * (1.0 / max(float(dense.norm()), 1.0))
    m = dense * (1.0 - float(np.float32(0.9)))
    v = dense * dense * (1.0 - float(np.float32(0.999)))
    want = w0 - 0.01 * m / (v.sqrt() + 1e-4)
    assert float((item.double() - want).abs().max()) <= 1e-6 and float((opt.ms[0].double() - m).abs().max()) <= 1e-7
    assert float((item.double() - w0).abs().max()) > 1e-3

    # TrainStep's loop: owned lists the shared parameter once, with the slot to step it through
    from dir_amd import train_spec
    calls = []
    p_item, p_user = torch.nn.Parameter(item), torch.nn.Parameter(user)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

    step = train_spec.TrainStep(Model(), optimizer="Adam")
    opt.owned, opt.owned_slots = [p_item, p_user], [0, 1]
    opt.step_table_grad = lambda f, grad: calls.append(f)
    step.sparse_adam = [opt]
    p_item.grad, p_user.grad = grad, None
    step((step.params[0] * 2.0).sum())
    assert calls == [0] and p_item.grad is None and opt.lr_t > 0
