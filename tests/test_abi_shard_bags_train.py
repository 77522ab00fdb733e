"""CPU tests of the C-ABI boundary of the sharded bags' backward (include/dir_hip.h: dir_shard_bags_grad_f32,
dir_sparse_adagrad_sorted_bags_f32): both exports check their arguments before any HIP call -- null pointers, K outside the range one
wave covers, P > 64, capacities past 2^31, a short or misaligned workspace -- return the error code and name themselves in
dir_last_error."""
import ctypes

import numpy as np

BADARG, UNSUPPORTED = -1, -4


def _err(lib):
    return lib.dir_last_error().decode()


def _buf():
    buf = np.zeros(1 << 16, np.int64)                 # a stand-in address: every call below fails before it is dereferenced
    return buf, ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)


def test_grad_rejects_bad_arguments_and_k(built_lib):
    lib = built_lib
    buf, p = _buf()

    def call(**kw):
        a = dict(g=p, ld=32, K=16, P=2, pos=p, mask=p, denom=p, B=4, F=2, sc=None, comb=1, cap_b=16, send=p)
        a.update(kw)
        return lib.dir_shard_bags_grad_f32(*a.values(), None)
    for name in ("g", "pos", "mask", "denom", "send"):
        lib.dir_last_error()
        assert call(**{name: None}) == BADARG, name
        assert "dir_shard_bags_grad_f32" in _err(lib) and "null" in _err(lib)
    assert call(K=0) == BADARG and "dir_shard_bags_grad_f32" in _err(lib) and "K=0" in _err(lib)
    assert call(K=65, ld=130) == UNSUPPORTED and "K=65" in _err(lib)              # not a multiple of 4: one float per lane, at most 64
    assert call(K=260, ld=520) == UNSUPPORTED and "K=260" in _err(lib)            # 65 float4 chunks: wider than one wave
    assert call(P=65) == BADARG and "P <= 64" in _err(lib)
    assert call(cap_b=1 << 30) == BADARG and "2^31" in _err(lib)                  # P * cap_b
    assert call(cap_b=0) == BADARG and "cap_b" in _err(lib)
    assert call(ld=31) == BADARG and "g_ld" in _err(lib)
    assert call(comb=3) == BADARG and "combiner" in _err(lib)
    assert call(F=0) == BADARG
    assert call(g=None, pos=None, mask=None, denom=None, B=0) == 0                # an empty batch carries no buffers


def test_adagrad_bags_rejects_bad_arguments_and_k(built_lib):
    lib = built_lib
    buf, p = _buf()
    big = 1 << 20

    def call(**kw):
        a = dict(tables=p, accums=p, F=2, K=16, recv=p, P=2, cap_e=16, cap_b=16, grecv=p, smn=None, mn=0.0, lr=0.1, rb=p, total=100,
                 ws=p, ws_bytes=big)
        a.update(kw)
        return lib.dir_sparse_adagrad_sorted_bags_f32(*a.values(), None)
    for name in ("tables", "accums", "recv", "grecv", "rb", "ws"):
        lib.dir_last_error()
        assert call(**{name: None}) == BADARG, name
        assert "dir_sparse_adagrad_sorted_bags_f32" in _err(lib) and "null" in _err(lib)
    assert call(K=0) == BADARG and "dir_sparse_adagrad_sorted_bags_f32" in _err(lib) and "K=0" in _err(lib)
    assert call(K=65) == UNSUPPORTED and "K=65" in _err(lib)
    assert call(K=260) == UNSUPPORTED and "K=260" in _err(lib)
    assert call(P=65) == BADARG and "P <= 64" in _err(lib)
    assert call(P=0) == BADARG
    assert call(cap_e=1 << 31) == BADARG and "2^31" in _err(lib)
    assert call(cap_b=1 << 30) == BADARG and "2^31" in _err(lib)                  # P * cap_b
    assert call(cap_e=1 << 29, P=2) == UNSUPPORTED and "2^30" in _err(lib)        # the sort's entry limit
    assert call(mn=-1.0) == BADARG and "max_norm" in _err(lib)
    assert call(total=1 << 32) == UNSUPPORTED and "total_rows" in _err(lib)
    # the workspace: dir_sparse_adagrad_sorted_workspace_bytes(P * cap_e, 1, K, total_rows) bytes, 256-byte aligned
    need = lib.dir_sparse_adagrad_sorted_workspace_bytes(2 * 16, 1, 16, 100)
    assert 0 < need <= big
    assert call(ws_bytes=64) == BADARG and "workspace" in _err(lib) and "dir_sparse_adagrad_sorted_bags_f32" in _err(lib)
    assert call(ws=ctypes.c_void_p(p.value + 16)) == BADARG and "256-byte" in _err(lib)
