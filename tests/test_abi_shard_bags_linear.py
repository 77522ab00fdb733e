"""CPU tests of the C-ABI boundary of the first-order term over row-sharded multi-hot bags (include/dir_hip.h:
dir_shard_bags_linear_pool_f32, dir_shard_bags_linear_combine_f32, dir_shard_bags_linear_grad_f32, dir_sparse_ftrl_rows_sorted_bags_f32):
the four exports are declared, documented, exported and bound, and each checks its arguments before any HIP call -- null pointers, F <= 0,
P outside 1..64, P * cap_b >= 2^31, cap_e out of range, a bad combiner, lr <= 0, negative l1 / l2, a short or misaligned workspace --
returns the error code and names itself and the argument in dir_last_error."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -4
NAMES = ("dir_shard_bags_linear_pool_f32", "dir_shard_bags_linear_combine_f32", "dir_shard_bags_linear_grad_f32",
         "dir_sparse_ftrl_rows_sorted_bags_f32")


def _err(lib):
    return lib.dir_last_error().decode()


def _buf():
    buf = np.zeros(1 << 16, np.int64)                 # a stand-in address: every call below fails before it is dereferenced
    return buf, ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)


def _bad(lib, name, rc, *words, code=BADARG):
    msg = _err(lib)
    assert rc == code and name in msg and all(w in msg for w in words), (rc, msg, words)


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


def test_pool_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_bags_linear_pool_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(rows=p, ld=4, local=p, F=2, recv=p, P=2, cap_e=16, cap_b=16, out=p)
        a.update(kw)
        return lib.dir_shard_bags_linear_pool_f32(*a.values(), None)
    for arg in ("rows", "local", "recv", "out"):
        _bad(lib, name, call(**{arg: None}), "null")
    _bad(lib, name, call(F=0), "F=0")
    _bad(lib, name, call(F=-3), "F=-3")
    _bad(lib, name, call(ld=0), "row_ld=0")
    _bad(lib, name, call(P=65), "P=65")
    _bad(lib, name, call(P=0), "P=0")
    _bad(lib, name, call(cap_e=0), "cap_e=0")
    _bad(lib, name, call(cap_e=1 << 31), "cap_e=", "2^31")
    _bad(lib, name, call(cap_b=0), "cap_b=0")
    _bad(lib, name, call(cap_b=1 << 30), "cap_b=", "2^31")                                     # P * cap_b


def test_combine_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_bags_linear_combine_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(lback=p, P=2, cap_b=16, pos=p, mask=p, ids=p, offsets=p, weights=None, nnz=8, sb=2, sf=1, vocab=p, flags=0, B=4, F=2,
                 combiner=1, lden=p, bias=None, out=p, out_ld=1)
        a.update(kw)
        return lib.dir_shard_bags_linear_combine_f32(*a.values(), None)
    for arg in ("lback", "pos", "mask", "out", "ids", "offsets", "vocab", "lden"):            # (mean: the CSR and lden are read)
        _bad(lib, name, call(**{arg: None}), "null")
    for arg in ("lback", "pos", "mask", "out"):
        _bad(lib, name, call(**{arg: None}, combiner=0), "null")
    _bad(lib, name, call(F=0), "F=0")
    _bad(lib, name, call(B=-1), "B=-1")
    _bad(lib, name, call(B=1 << 30), "2^31")                                                   # B * F
    _bad(lib, name, call(P=65), "P=65")
    _bad(lib, name, call(P=0), "P=0")
    _bad(lib, name, call(cap_b=0), "cap_b=0")
    _bad(lib, name, call(cap_b=1 << 30), "cap_b=", "2^31")
    _bad(lib, name, call(combiner=3), "combiner=3")
    _bad(lib, name, call(combiner=-1), "combiner=-1")
    _bad(lib, name, call(nnz=-1), "nnz=-1")
    _bad(lib, name, call(out_ld=0), "out_ld=0")
    assert call(B=0, lback=None, pos=None, mask=None, out=None, ids=None, offsets=None, vocab=None, lden=None) == 0      # an empty batch


def test_grad_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_shard_bags_linear_grad_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(g=p, g_ld=1, P=2, cap_b=16, pos=p, mask=p, lden=p, B=4, F=2, combiner=2, send=p)
        a.update(kw)
        return lib.dir_shard_bags_linear_grad_f32(*a.values(), None)
    for arg in ("g", "pos", "mask", "lden", "send"):
        _bad(lib, name, call(**{arg: None}), "null")
    _bad(lib, name, call(F=0), "F=0")
    _bad(lib, name, call(B=-1), "B=-1")
    _bad(lib, name, call(B=1 << 30), "2^31")
    _bad(lib, name, call(P=65), "P=65")
    _bad(lib, name, call(cap_b=0), "cap_b=0")
    _bad(lib, name, call(cap_b=1 << 30), "cap_b=", "2^31")
    _bad(lib, name, call(combiner=7), "combiner=7")
    _bad(lib, name, call(g_ld=0), "g_ld=0")
    assert call(B=0, g=None, pos=None, mask=None, lden=None) == 0


def test_ftrl_bags_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_sparse_ftrl_rows_sorted_bags_f32"
    buf, p = _buf()
    big = 1 << 19
    f32 = ctypes.c_float

    def call(**kw):
        a = dict(rows=p, F=2, recv=p, P=2, cap_e=16, cap_b=8, grecv=p, lr=f32(0.1), l1=f32(0.0), l2=f32(0.0), rb=p, total=100, ws=p,
                 ws_bytes=big, src=None)
        a.update(kw)
        return lib.dir_sparse_ftrl_rows_sorted_bags_f32(*a.values(), None)
    for arg in ("rows", "recv", "grecv", "rb", "ws"):
        _bad(lib, name, call(**{arg: None}), "null")
    _bad(lib, name, call(F=0), "F=0")
    _bad(lib, name, call(P=65), "P=65")
    _bad(lib, name, call(P=0), "P=0")
    _bad(lib, name, call(cap_e=0), "cap_e=0")
    _bad(lib, name, call(cap_e=1 << 31), "cap_e=", "2^31")
    _bad(lib, name, call(cap_b=1 << 30), "cap_b=", "2^31")
    _bad(lib, name, call(lr=f32(0.0)), "lr=0")
    _bad(lib, name, call(lr=f32(-0.5)), "lr=-0.5")
    _bad(lib, name, call(l1=f32(-1.0)), "l1=-1")
    _bad(lib, name, call(l2=f32(-2.0)), "l2=-2")
    _bad(lib, name, call(cap_e=1 << 29), "2^30", code=UNSUPPORTED)                             # P * cap_e entry slots
    _bad(lib, name, call(total=1 << 32), "total_rows", code=UNSUPPORTED)
    # the workspace: dir_sparse_adagrad_sorted_workspace_bytes(P * cap_e, 1, 1, total_rows) bytes, 256-byte aligned -- its own and sorted_from
    need = lib.dir_sparse_adagrad_sorted_workspace_bytes(32, 1, 1, 100)
    assert 0 < need <= big
    _bad(lib, name, call(ws_bytes=need - 1), "workspace")
    _bad(lib, name, call(ws_bytes=64), "workspace")
    _bad(lib, name, call(ws=ctypes.c_void_p(p.value + 16)), "256-byte")
    _bad(lib, name, call(src=ctypes.c_void_p(p.value + 16)), "sorted_from", "256-byte")
    assert call(total=0) == 0                                                                  # a rank without rows: nothing to do
