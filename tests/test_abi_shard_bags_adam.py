"""CPU tests of the C-ABI boundary of the owner-side sparse Adam over bag records (include/dir_hip.h:
dir_sparse_adam_bags_workspace_bytes, dir_sparse_adam_bags_norm_f32, dir_sparse_adam_bags_apply_f32): the three exports are declared,
documented, exported and bound, and the two entries check every argument before any HIP call -- null pointers, F = 0 or 65, K = 12 or 6,
a misaligned grecv / norm2 / workspace, a short workspace, bad slab geometry, P * cap_e >= 2^30, total_rows >= 2^32 - 1, beta outside
[0, 1), eps <= 0, clip_norm > 0 without norm2_global (and the reverse) -- return the error code and name themselves and the argument in
dir_last_error.  The workspace query returns 0 exactly for the unsupported sizes."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -4
NAMES = ("dir_sparse_adam_bags_workspace_bytes", "dir_sparse_adam_bags_norm_f32", "dir_sparse_adam_bags_apply_f32")
f32 = ctypes.c_float


def _err(lib):
    return lib.dir_last_error().decode()


def _buf():
    buf = np.zeros(1 << 16, np.int64)                 # a stand-in address: every call below fails before it is dereferenced
    return buf, ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)


def test_header_exports_and_bindings_agree(built_lib):
    from dir_amd import _lib
    src = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        decl = re.search(r"\b(int|int64_t)\s+%s\s*\(([^;]*)\)\s*;" % n, code)
        assert decl, "%s is not declared in include/dir_hip.h" % n
        assert hasattr(built_lib, n), "libdir_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES, "%s has no row in _lib.SIGNATURES" % n
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is (ctypes.c_int if decl.group(1) == "int" else ctypes.c_int64), n
        assert len(argtypes) == decl.group(2).count(",") + 1, n
        assert n in src.split(decl.group(0))[0], "%s is not documented above its declaration" % n
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert n in doc, "%s is missing from INTEGRATION.md" % n


def test_workspace_bytes(built_lib):
    ws = built_lib.dir_sparse_adam_bags_workspace_bytes          # (P, cap_e, F, K, total_rows)
    need = ws(4, 250, 3, 16, 457)
    assert need > 0 and need == built_lib.dir_sparse_adam_payload_workspace_bytes(1000, 3, 16, 457)      # the payload form's for n = P * cap_e
    assert need == built_lib.dir_sparse_adagrad_sorted_workspace_bytes(1000, 1, 32, 457)                 # ... with carry rows of K doubles
    assert ws(4, 250, 3, 64, 457) >= need
    assert ws(2, 16, 3, 16, 0) > 0                                      # an owner without rows (every vocab < P) is legal
    assert ws(64, (1 << 24) - 1, 3, 16, 100) > 0                        # the largest sort: P * cap_e = 2^30 - 64
    for bad in ((0, 16, 3, 16, 100), (65, 16, 3, 16, 100), (2, 0, 3, 16, 100), (2, 1 << 31, 3, 16, 100), (64, 1 << 24, 3, 16, 100),
                (1, 1 << 30, 3, 16, 100), (2, 16, 0, 16, 100), (2, 16, 65, 16, 100), (2, 16, 3, 6, 100), (2, 16, 3, 12, 100),
                (2, 16, 3, 0, 100), (2, 16, 3, 48, 100), (2, 16, 3, 16, -1), (2, 16, 3, 16, (1 << 32) - 1)):
        assert ws(*bad) == 0, bad
    for K in (4, 8, 16, 32, 64, 128, 256):
        assert ws(2, 16, 64, K, (1 << 32) - 2) > 0, K


def _shared_checks(lib, name, call, p):
    """What both entries reject alike: the arguments of adam_bags_check."""
    for arg in ("recv", "grecv", "rb", "ws"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib), (arg, _err(lib))
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(F=65) == BADARG and name in _err(lib) and "F=65" in _err(lib)
    assert call(K=6) == BADARG and name in _err(lib) and "K=6" in _err(lib)
    assert call(K=12) == BADARG and name in _err(lib) and "K=12" in _err(lib)                 # K / 4 = 3 does not divide 64
    assert call(K=0) == BADARG and "K=0" in _err(lib)
    assert call(P=0) == BADARG and name in _err(lib) and "P=0" in _err(lib)
    assert call(P=65) == BADARG and "P=65" in _err(lib)
    assert call(cap_e=0) == BADARG and name in _err(lib) and "cap_e=0" in _err(lib)
    assert call(cap_b=0) == BADARG and name in _err(lib) and "cap_b=0" in _err(lib)
    assert call(P=64, cap_e=1 << 24) == UNSUPPORTED and name in _err(lib) and "2^30" in _err(lib)
    assert call(P=1, cap_e=1 << 30) == UNSUPPORTED and "2^30" in _err(lib)
    assert call(total=(1 << 32) - 1) == UNSUPPORTED and name in _err(lib) and "total_rows" in _err(lib)
    assert call(total=1 << 32) == UNSUPPORTED and "total_rows" in _err(lib)
    assert call(total=-1) == UNSUPPORTED and "total_rows" in _err(lib)
    assert call(mn=f32(-1.0)) == BADARG and name in _err(lib) and "max_norm=-1" in _err(lib)
    for off in (4, 8):
        assert call(grecv=ctypes.c_void_p(p.value + off)) == UNSUPPORTED and name in _err(lib) and "grecv" in _err(lib) and "16-byte" in _err(lib)
    need = lib.dir_sparse_adam_bags_workspace_bytes(2, 16, 2, 8, 100)
    assert 0 < need <= 1 << 19
    assert call(ws_bytes=need - 1) == BADARG and "workspace" in _err(lib) and name in _err(lib)
    assert call(ws_bytes=0) == BADARG and "workspace" in _err(lib)
    assert call(ws=ctypes.c_void_p(p.value + 16)) == BADARG and "256-byte" in _err(lib) and name in _err(lib)


def test_norm_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_sparse_adam_bags_norm_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(tables=p, F=2, K=8, recv=p, P=2, cap_e=16, cap_b=16, grecv=p, slot_mn=None, mn=f32(0.0), rb=p, total=100, norm2=p, ws=p,
                 ws_bytes=1 << 19)
        a.update(kw)
        return lib.dir_sparse_adam_bags_norm_f32(*a.values(), None)
    _shared_checks(lib, name, call, p)
    assert call(norm2=None) == BADARG and name in _err(lib) and "null" in _err(lib) and "norm2" in _err(lib)
    assert call(norm2=None, total=0) == BADARG and "norm2" in _err(lib)                       # an owner without rows still zeroes norm2
    assert call(norm2=ctypes.c_void_p(p.value + 4)) == BADARG and "norm2" in _err(lib) and "8-byte" in _err(lib)
    # tables may be NULL only when no slot has a max_norm
    assert call(tables=None, mn=f32(0.5)) == BADARG and name in _err(lib) and "tables" in _err(lib)
    assert call(tables=None, slot_mn=p) == BADARG and "tables" in _err(lib)
    assert call(tables=None, norm2=None) == BADARG and "norm2" in _err(lib)                   # (tables = NULL alone is accepted: the next check speaks)


def test_apply_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_sparse_adam_bags_apply_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(tables=p, ms=p, vs=p, F=2, K=8, recv=p, P=2, cap_e=16, cap_b=16, grecv=p, slot_mn=None, mn=f32(0.0), lr_t=f32(0.01),
                 b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8), clip=f32(100.0), norm2=p, rb=p, total=100, marks=p, ws=p, ws_bytes=1 << 19,
                 sorted=0, first=1)
        a.update(kw)
        return lib.dir_sparse_adam_bags_apply_f32(*a.values(), None)
    _shared_checks(lib, name, call, p)
    for arg in ("tables", "ms", "vs", "marks"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib), (arg, _err(lib))
    assert call(b1=f32(1.0)) == BADARG and name in _err(lib) and "beta1=1" in _err(lib)
    assert call(b2=f32(-0.5)) == BADARG and "beta2=-0.5" in _err(lib)
    assert call(eps=f32(0.0)) == BADARG and name in _err(lib) and "eps=0" in _err(lib)
    assert call(clip=f32(-1.0), norm2=None) == BADARG and name in _err(lib) and "clip_norm=-1" in _err(lib)
    assert call(lr_t=f32(-0.5)) == BADARG and "lr_t=-0.5" in _err(lib)
    assert call(norm2=None) == BADARG and name in _err(lib) and "norm2_global" in _err(lib)              # clip_norm > 0 without the norms
    assert call(clip=f32(0.0)) == BADARG and "norm2_global" in _err(lib)                                  # ... and norms without a clip
    assert call(norm2=ctypes.c_void_p(p.value + 4)) == BADARG and "norm2_global" in _err(lib) and "8-byte" in _err(lib)
    assert call(norm2=None, total=0) == BADARG and "norm2_global" in _err(lib)                            # checked before the no-rows return
