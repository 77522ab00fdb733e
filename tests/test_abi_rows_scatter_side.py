"""CPU tests of the C-ABI boundary of the scatter-sum with a side sum (include/dir_hip.h: dir_rows_scatter_sum_side_workspace_bytes,
dir_rows_scatter_sum_side_f32): the two exports are declared, documented, exported and bound; the size query answers -1 outside the
supported shapes and never less than the plain entry's size; and the entry checks every argument before any HIP call -- U outside 1..4,
side_div < 1, side_ld < U, ld < K, a null side or out_side, a short or misaligned workspace, K wider than a wave covers -- returning the
error code and naming itself and the argument in dir_last_error."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, UNSUPPORTED = -1, -4
NAMES = ("dir_rows_scatter_sum_side_workspace_bytes", "dir_rows_scatter_sum_side_f32")


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
    # the plain entry keeps its signature
    assert len(_lib.SIGNATURES["dir_rows_scatter_sum_f32"][1]) == 10 and len(_lib.SIGNATURES["dir_rows_scatter_sum_workspace_bytes"][1]) == 3


def test_workspace_bytes(built_lib):
    ws, plain = built_lib.dir_rows_scatter_sum_side_workspace_bytes, built_lib.dir_rows_scatter_sum_workspace_bytes
    for n, K, R in ((0, 8, 5), (1, 4, 1), (9079, 16, 40), (9079, 256, 40), (65536 * 26, 16, 1 << 21), (300, 6, 1_000_003), (10, 8, 0)):
        for U in (1, 2, 4):
            assert ws(n, K, U, R) >= plain(n, K, R) >= 0, (n, K, U, R)
            assert ws(n, K, U, R) % 256 == 0
    # the carry grows from K to K + U floats per slot: two slots per 256-entry tile
    n, K, R = 1 << 20, 16, 1000
    assert ws(n, K, 4, R) - plain(n, K, R) == (n // 256) * 2 * 4 * 4
    # outside scat_shape_ok, or U outside 1..4
    for bad in ((-1, 8, 1, 5), (1 << 30, 8, 1, 5), (4, 0, 1, 5), (4, -8, 1, 5), (4, 8, 1, -1), (4, 8, 1, (1 << 32) - 1), (4, 8, 1, 1 << 32),
                (4, 8, 0, 5), (4, 8, 5, 5), (4, 8, -1, 5)):
        assert ws(*bad) == -1, bad


def test_entry_rejects_bad_arguments(built_lib):
    lib, name = built_lib, "dir_rows_scatter_sum_side_f32"
    buf, p = _buf()

    def call(**kw):
        a = dict(idx=p, vals=p, ld=8, side=p, side_ld=1, side_div=3, n=32, K=8, U=1, R=100, out=p, out_side=p, ws=p, ws_bytes=1 << 19)
        a.update(kw)
        return lib.dir_rows_scatter_sum_side_f32(*a.values(), None)
    assert 0 < lib.dir_rows_scatter_sum_side_workspace_bytes(32, 8, 1, 100) <= 1 << 19
    assert call(U=0) == BADARG and name in _err(lib) and "U=0" in _err(lib)
    assert call(U=5) == BADARG and name in _err(lib) and "U=5" in _err(lib)
    assert call(U=5, side_ld=5) == BADARG and "U=5" in _err(lib)
    assert call(side_div=0) == BADARG and name in _err(lib) and "side_div=0" in _err(lib)
    assert call(side_div=-2) == BADARG and "side_div=-2" in _err(lib)
    assert call(U=2, side_ld=1) == BADARG and name in _err(lib) and "side_ld=1" in _err(lib)
    assert call(U=4, side_ld=3) == BADARG and "side_ld=3" in _err(lib)
    assert call(ld=7) == BADARG and name in _err(lib) and "ld=7" in _err(lib)
    assert call(side=None) == BADARG and name in _err(lib) and "null" in _err(lib) and "(side)" in _err(lib)
    assert call(out_side=None) == BADARG and name in _err(lib) and "null" in _err(lib) and "out_side" in _err(lib)
    assert call(out_side=None, n=0, idx=None, vals=None, side=None, ws=None) == BADARG and "out_side" in _err(lib)     # n == 0 still zero-fills it
    for arg in ("idx", "vals", "out"):
        assert call(**{arg: None}) == BADARG and name in _err(lib) and "null" in _err(lib), arg
    need = lib.dir_rows_scatter_sum_side_workspace_bytes(32, 8, 1, 100)
    assert call(ws_bytes=need - 1) == BADARG and name in _err(lib) and "workspace" in _err(lib)
    assert call(ws_bytes=0) == BADARG and "workspace" in _err(lib)
    assert call(ws=None) == BADARG and "workspace" in _err(lib)
    assert call(ws=ctypes.c_void_p(p.value + 16)) == BADARG and name in _err(lib) and "256-byte" in _err(lib)
    assert call(K=260, ld=260) == UNSUPPORTED and name in _err(lib) and "K=260" in _err(lib) and "wave" in _err(lib)
    assert call(K=65, ld=65) == UNSUPPORTED and "K=65" in _err(lib)                   # the scalar path: one lane per float
    assert call(n=-1) == BADARG and name in _err(lib) and "n=-1" in _err(lib)
    assert call(n=1 << 30) == BADARG and "2^30" in _err(lib)
    assert call(R=-1) == BADARG and "R=-1" in _err(lib)
    assert call(K=0, ld=0) == BADARG and "K=0" in _err(lib)
    # R == 0: nothing to write -- as the plain entry, also with null outputs
    assert call(R=0, out=None, out_side=None) == 0
    # the plain entry's checks are what they were
    plain = lib.dir_rows_scatter_sum_f32
    assert plain(p, p, 7, 32, 8, 100, p, p, 1 << 19, None) == BADARG and "dir_rows_scatter_sum_f32" in _err(lib) and "ld=7" in _err(lib)
    assert plain(p, p, 260, 32, 260, 100, p, p, 1 << 19, None) == UNSUPPORTED and "dir_rows_scatter_sum_f32:" in _err(lib)
