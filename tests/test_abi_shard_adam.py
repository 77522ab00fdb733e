"""CPU tests of the C-ABI boundary of the owner-side sparse Adam on row-sharded tables (include/dir_hip.h:
dir_sparse_adam_payload_workspace_bytes, dir_sparse_adam_payload_norm_f32, dir_sparse_adam_payload_apply_f32): the three exports are
declared, documented, exported and bound, and the two entries check every argument before any HIP call -- null pointers, F <= 0 or > 64,
K not a multiple of 4, n < 0 or >= 2^31, a short or misaligned workspace, beta outside [0, 1), eps <= 0, a negative clip, clip_norm > 0
without norm2_global (and the reverse) -- return the error code and name themselves and the argument in dir_last_error."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -4
NAMES = ("dir_sparse_adam_payload_workspace_bytes", "dir_sparse_adam_payload_norm_f32", "dir_sparse_adam_payload_apply_f32")
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
    ws = built_lib.dir_sparse_adam_payload_workspace_bytes
    assert ws(0, 3, 16, 100) > 0                                        # nothing received is legal
    assert ws(0, 3, 16, 0) > 0 and ws(32, 3, 16, 0) > 0                 # ... and so is an owner without rows (every vocab < P)
    need = ws(1000, 3, 16, 457)
    assert need == built_lib.dir_sparse_adagrad_sorted_workspace_bytes(1000, 1, 32, 457)       # the sort area of n flat entries, carry rows of K doubles
    assert ws(1000, 3, 64, 457) >= need
    for bad in ((-1, 3, 16, 100), (1 << 31, 3, 16, 100), (10, 0, 16, 100), (10, 65, 16, 100), (10, 3, 6, 100), (10, 3, 0, 100),
                (10, 3, 48, 100), (10, 3, 16, -1), (10, 3, 16, (1 << 32) - 1)):
        assert ws(*bad) == 0, bad


def test_norm_words_are_two_per_table(built_lib):
    """The norm words' size is part of the ABI: 128 u64 (low [f], high [64 + f]) at the head of dir_sparse_adam_f32's workspace and in
    dir_sparse_adam_payload_norm_f32's norm2, stated in the header, bound in _lib and documented."""
    from dir_amd import _lib
    assert _lib.ADAM_NORM_WORDS == 128
    B, F, K, total = 1000, 3, 16, 457
    sort_area = built_lib.dir_sparse_adagrad_sorted_workspace_bytes(B, F, K, total)
    assert built_lib.dir_sparse_adam_workspace_bytes(B, F, K, total) == sort_area + 8 * _lib.ADAM_NORM_WORDS + (total + 255) // 256 * 256
    src = open(os.path.join(ROOT, "include", "dir_hip.h")).read()
    assert "128 x u64" in src and "norm2[64 + f]" in src and "2^62" in src
    assert "128 x u64" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _shared_checks(lib, name, call, p):
    """What both entries reject alike: the arguments of adam_payload_check."""
    for arg in ("payload", "grad", "rb", "ws"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib), (arg, _err(lib))
    assert call(F=0) == BADARG and name in _err(lib) and "F=0" in _err(lib)
    assert call(F=-3) == BADARG and "F=-3" in _err(lib)
    assert call(F=65) == BADARG and name in _err(lib) and "F=65" in _err(lib)
    assert call(K=6) == BADARG and name in _err(lib) and "K=6" in _err(lib)
    assert call(K=0) == BADARG and "K=0" in _err(lib)
    assert call(K=48) == BADARG and "K=48" in _err(lib)                                       # K / 4 = 12 does not divide 64
    assert call(n=-1) == BADARG and name in _err(lib) and "n=-1" in _err(lib)
    assert call(n=1 << 31) == BADARG and name in _err(lib) and "2^31" in _err(lib)
    assert call(n=(1 << 31) - 1) == BADARG and "2^31" in _err(lib)
    assert call(total=1 << 32) == UNSUPPORTED and name in _err(lib) and "total_rows" in _err(lib)
    assert call(total=-1) == UNSUPPORTED and "total_rows" in _err(lib)
    need = lib.dir_sparse_adam_payload_workspace_bytes(32, 2, 8, 100)
    assert 0 < need <= 1 << 19
    assert call(ws_bytes=need - 1) == BADARG and "workspace" in _err(lib) and name in _err(lib)
    assert call(ws_bytes=64) == BADARG and "workspace" in _err(lib)
    assert call(ws_bytes=0) == BADARG and "workspace" in _err(lib)
    assert call(ws=ctypes.c_void_p(p.value + 16)) == BADARG and "256-byte" in _err(lib) and name in _err(lib)


def test_norm_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_sparse_adam_payload_norm_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(F=2, K=8, payload=p, n=32, grad=p, rb=p, total=100, norm2=p, ws=p, ws_bytes=1 << 19)
        a.update(kw)
        return lib.dir_sparse_adam_payload_norm_f32(*a.values(), None)
    _shared_checks(lib, name, call, p)
    assert call(norm2=None) == BADARG and name in _err(lib) and "null" in _err(lib) and "norm2" in _err(lib)
    assert call(norm2=None, n=0, payload=None, grad=None, ws=None) == BADARG and "norm2" in _err(lib)      # n == 0 still zeroes norm2
    assert call(norm2=ctypes.c_void_p(p.value + 4)) == BADARG and "norm2" in _err(lib) and "8-byte" in _err(lib)
    assert call(n=0, rb=None) == BADARG and "row_base" in _err(lib)


def test_apply_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_sparse_adam_payload_apply_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(tables=p, ms=p, vs=p, F=2, K=8, payload=p, n=32, grad=p, lr_t=f32(0.01), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8),
                 clip=f32(100.0), norm2=p, rb=p, total=100, marks=p, ws=p, ws_bytes=1 << 19, sorted=0, first=1)
        a.update(kw)
        return lib.dir_sparse_adam_payload_apply_f32(*a.values(), None)
    _shared_checks(lib, name, call, p)
    for arg in ("tables", "ms", "vs", "marks"):
        lib.dir_last_error()
        assert call(**{arg: None}) == BADARG, arg
        assert name in _err(lib) and "null" in _err(lib), (arg, _err(lib))
        assert call(**{arg: None}, n=0, payload=None, grad=None, ws=None) == BADARG and "null" in _err(lib), arg     # the decay pass needs them too
    assert call(b1=f32(1.0)) == BADARG and name in _err(lib) and "beta1=1" in _err(lib)
    assert call(b1=f32(-0.1)) == BADARG and "beta1=-0.1" in _err(lib)
    assert call(b2=f32(1.0)) == BADARG and name in _err(lib) and "beta2=1" in _err(lib)
    assert call(b2=f32(-0.5)) == BADARG and "beta2=-0.5" in _err(lib)
    assert call(eps=f32(0.0)) == BADARG and name in _err(lib) and "eps=0" in _err(lib)
    assert call(eps=f32(-1.0)) == BADARG and "eps=-1" in _err(lib)
    assert call(clip=f32(-1.0), norm2=None) == BADARG and name in _err(lib) and "clip_norm=-1" in _err(lib)
    assert call(lr_t=f32(-0.5)) == BADARG and "lr_t=-0.5" in _err(lib)
    assert call(norm2=None) == BADARG and name in _err(lib) and "norm2_global" in _err(lib)              # clip_norm > 0 without the norms
    assert call(clip=f32(0.0)) == BADARG and "norm2_global" in _err(lib)                                  # ... and norms without a clip
    assert call(norm2=ctypes.c_void_p(p.value + 4)) == BADARG and "norm2_global" in _err(lib) and "8-byte" in _err(lib)
    assert call(norm2=None, n=0, payload=None, grad=None, ws=None) == BADARG and "norm2_global" in _err(lib)
