"""CPU tests of the C-ABI boundary of row groups and units > 1 on the sharded lookup (include/dir_hip.h: dir_shard_finish_groups_f32,
dir_shard_grad_groups_f32, dir_shard_linear_gather_units_f32, dir_shard_linear_finish_units_f32, dir_shard_linear_grad_units_f32,
dir_sparse_ftrl_rows_units_sorted_payload_f32): the six exports are declared, documented, exported and bound, and each checks its
arguments before any HIP call -- null pointers, F <= 0, G <= 0, K % 4 != 0, units outside 1..8, P > 64, P * cap >= 2^31, a negative n, a
short or misaligned workspace, lr <= 0 -- returns the error code and names itself and the argument in dir_last_error."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -4
NAMES = ("dir_shard_finish_groups_f32", "dir_shard_grad_groups_f32", "dir_shard_linear_gather_units_f32", "dir_shard_linear_finish_units_f32",
         "dir_shard_linear_grad_units_f32", "dir_sparse_ftrl_rows_units_sorted_payload_f32")


def _err(lib):
    return lib.dir_last_error().decode()


def _buf():
    buf = np.zeros(1 << 16, np.int64)                 # a stand-in address: every call below fails before it is dereferenced
    return buf, ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)


def _ptrs(p, n=2, shift=0):
    """A HOST array of n stand-in device pointers (the grouped entries take their G buffers this way)."""
    return (ctypes.c_void_p * n)(*[p.value + shift + 1024 * i for i in range(n)])


def test_header_exports_and_bindings_agree(built_lib):
    from dir_amd import _lib
    src = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % n, code)
        assert decl, "%s is not declared in include/dir_hip.h" % n
        assert hasattr(built_lib, n), "libdir_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES, "%s has no row in _lib.SIGNATURES" % n
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is ctypes.c_int and len(argtypes) == decl.group(1).count(",") + 1, n
        assert n in src.split(decl.group(0))[0], "%s is not documented above its declaration" % n


def test_finish_groups_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_finish_groups_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(back=p, n_back=32, G=2, K=4, inv=p, sb=3, sf=1, F=3, B=4, outs=_ptrs(p), out_ld=12)
        a.update(kw)
        return lib.dir_shard_finish_groups_f32(*a.values(), None)
    for arg in ("back", "inv", "outs"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib)
    assert call(outs=(ctypes.c_void_p * 2)(p.value, None)) == BADARG and name in _err(lib) and "outs[1]" in _err(lib)
    assert call(outs=_ptrs(p, shift=4)) == BADARG and "16-byte" in _err(lib)
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(B=-1) == BADARG and "B=-1" in _err(lib)
    assert call(G=0) == BADARG and name in _err(lib) and "G=0" in _err(lib)
    assert call(G=-2) == BADARG and "G=-2" in _err(lib)
    assert call(G=17) == BADARG and "G=17" in _err(lib)
    assert call(K=6, out_ld=18) == BADARG and name in _err(lib) and "K=6" in _err(lib)
    assert call(K=0) == BADARG and "K=0" in _err(lib)
    assert call(out_ld=8) == BADARG and "out_ld=8" in _err(lib)                                # < F * K
    assert call(out_ld=14) == BADARG and "out_ld=14" in _err(lib)                              # not a multiple of 4
    assert call(n_back=-1) == BADARG and "n_back=-1" in _err(lib)
    assert call(n_back=1 << 31) == BADARG and "2^31" in _err(lib)
    assert call(B=1 << 30) == BADARG and name in _err(lib) and "2^31" in _err(lib)             # B * F * G * K / 4
    assert call(B=0, back=None, inv=None, outs=None) == 0                                      # an empty batch carries no buffers


def test_grad_groups_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_grad_groups_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(grads=_ptrs(p), g_ld=12, G=2, K=4, inv=p, sb=3, sf=1, F=3, B=4, send=p, n_send=32)
        a.update(kw)
        return lib.dir_shard_grad_groups_f32(*a.values(), None)
    for arg in ("grads", "inv", "send"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib)
    assert call(grads=(ctypes.c_void_p * 2)(None, p.value)) == BADARG and name in _err(lib) and "grads[0]" in _err(lib)
    assert call(send=ctypes.c_void_p(p.value + 8)) == BADARG and "16-byte" in _err(lib)
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(B=-1) == BADARG and "B=-1" in _err(lib)
    assert call(G=0) == BADARG and name in _err(lib) and "G=0" in _err(lib)
    assert call(G=17) == BADARG and "G=17" in _err(lib)
    assert call(K=10, g_ld=30) == BADARG and name in _err(lib) and "K=10" in _err(lib)
    assert call(g_ld=8) == BADARG and "g_ld=8" in _err(lib)
    assert call(n_send=-1) == BADARG and "n_send=-1" in _err(lib)
    assert call(n_send=1 << 31) == BADARG and "2^31" in _err(lib)
    assert call(B=1 << 30) == BADARG and "2^31" in _err(lib)
    assert call(B=0, grads=None, inv=None, send=None, n_send=0) == 0


def test_gather_units_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_linear_gather_units_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(rows=p, units=2, local=None, F=2, recv=p, P=2, cap=16, n=0, out=p)
        a.update(kw)
        return lib.dir_shard_linear_gather_units_f32(*a.values(), None)
    for arg in ("rows", "recv", "out"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib)
        assert call(**{arg: None}, cap=0, n=8) == BADARG and name in _err(lib) and "null" in _err(lib)      # the flat form too
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(units=0) == BADARG and name in _err(lib) and "units=0" in _err(lib)
    assert call(units=9) == BADARG and "units=9" in _err(lib)
    assert call(units=-1) == BADARG and "units=-1" in _err(lib)
    assert call(P=65) == BADARG and name in _err(lib) and "P=65" in _err(lib)
    assert call(P=0) == BADARG and "P=0" in _err(lib)
    assert call(cap=1 << 30) == BADARG and name in _err(lib) and "2^31" in _err(lib)          # P * cap
    assert call(cap=-1) == BADARG and "cap=-1" in _err(lib)
    assert call(cap=0, n=-1) == BADARG and name in _err(lib) and "n=-1" in _err(lib)
    assert call(cap=0, n=1 << 31) == BADARG and "2^31" in _err(lib)
    assert call(cap=0, n=0, rows=None, recv=None, out=None) == 0                              # an empty payload carries no buffers


def test_finish_units_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_linear_finish_units_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(wback=p, n_back=32, units=2, inv=p, sb=2, sf=1, F=2, bias=None, B=4, out=p, out_ld=2)
        a.update(kw)
        return lib.dir_shard_linear_finish_units_f32(*a.values(), None)
    for arg in ("wback", "inv", "out"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib)
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(B=-1) == BADARG and "B=-1" in _err(lib)
    assert call(units=0) == BADARG and name in _err(lib) and "units=0" in _err(lib)
    assert call(units=9, out_ld=9) == BADARG and "units=9" in _err(lib)
    assert call(n_back=-1) == BADARG and "n_back=-1" in _err(lib)
    assert call(n_back=1 << 30) == BADARG and "2^31" in _err(lib)                             # n_back * units
    assert call(out_ld=1) == BADARG and "out_ld=1" in _err(lib)                               # < units
    assert call(B=0, wback=None, inv=None, out=None) == 0


def test_grad_units_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_linear_grad_units_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(g=p, g_ld=2, units=2, inv=p, sb=2, sf=1, F=2, B=4, send=p, n_send=32)
        a.update(kw)
        return lib.dir_shard_linear_grad_units_f32(*a.values(), None)
    for arg in ("g", "inv", "send"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib)
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(B=-1) == BADARG and "B=-1" in _err(lib)
    assert call(units=0) == BADARG and name in _err(lib) and "units=0" in _err(lib)
    assert call(units=9, g_ld=9) == BADARG and "units=9" in _err(lib)
    assert call(B=1 << 29, F=2) == BADARG and "2^31" in _err(lib)                             # B * F * units
    assert call(n_send=-1) == BADARG and "n_send=-1" in _err(lib)
    assert call(n_send=1 << 30) == BADARG and "2^31" in _err(lib)
    assert call(g_ld=1) == BADARG and "g_ld=1" in _err(lib)
    assert call(B=0, g=None, inv=None, send=None, n_send=0) == 0


def test_ftrl_units_payload_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_sparse_ftrl_rows_units_sorted_payload_f32"
    buf, p = _buf()
    big = 1 << 19
    f32 = ctypes.c_float

    def call(**kw):
        a = dict(rows=p, F=2, units=2, payload=p, n=32, grad=p, lr=f32(0.1), l1=f32(0.0), l2=f32(0.0), rb=p, total=100, ws=p, ws_bytes=big,
                 src=None)
        a.update(kw)
        return lib.dir_sparse_ftrl_rows_units_sorted_payload_f32(*a.values(), None)
    for arg in ("rows", "payload", "grad", "rb", "ws"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib)
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(n=-1) == BADARG and name in _err(lib) and "n=-1" in _err(lib)
    assert call(units=0) == BADARG and name in _err(lib) and "units=0" in _err(lib)
    assert call(units=9) == BADARG and "units=9" in _err(lib)
    assert call(lr=f32(0.0)) == BADARG and name in _err(lib) and "lr=0" in _err(lib)
    assert call(lr=f32(-0.5)) == BADARG and "lr=-0.5" in _err(lib)
    assert call(l1=f32(-1.0)) == BADARG and name in _err(lib) and "l1=-1" in _err(lib)
    assert call(l2=f32(-2.0)) == BADARG and name in _err(lib) and "l2=-2" in _err(lib)
    assert call(total=1 << 32) == UNSUPPORTED and "total_rows" in _err(lib)
    assert call(total=0) == UNSUPPORTED and "total_rows" in _err(lib)
    # the workspace: dir_sparse_adagrad_sorted_workspace_bytes(n, 1, units, total_rows) bytes, 256-byte aligned -- for itself and for sorted_from
    need = lib.dir_sparse_adagrad_sorted_workspace_bytes(32, 1, 2, 100)
    assert 0 < need <= big
    assert call(ws_bytes=need - 1) == BADARG and "workspace" in _err(lib) and name in _err(lib)
    assert call(ws_bytes=64) == BADARG and "workspace" in _err(lib)
    assert call(ws=ctypes.c_void_p(p.value + 16)) == BADARG and "256-byte" in _err(lib) and name in _err(lib)
    assert call(src=ctypes.c_void_p(p.value + 16)) == BADARG and "sorted_from" in _err(lib) and "256-byte" in _err(lib)
    assert call(n=0, payload=None, grad=None, rb=None, ws=None) == 0                          # nothing received: nothing to do
