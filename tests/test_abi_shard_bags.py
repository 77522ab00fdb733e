"""CPU tests of the C-ABI boundary of the row-sharded bags (include/dir_hip.h: dir_shard_bags_*): every export checks its arguments
before any HIP call -- null pointers, K outside the range one wave covers, capacities past 2^31, P > 64 -- returns the error code and
leaves a message in dir_last_error."""
import ctypes

import numpy as np

BADARG, UNSUPPORTED = -1, -4


def _err(lib):
    return lib.dir_last_error().decode()


def test_workspace_bytes(built_lib):
    assert built_lib.dir_shard_bags_workspace_bytes(8) >= 64 * 8 + 4
    assert built_lib.dir_shard_bags_workspace_bytes(0) == 0
    assert built_lib.dir_shard_bags_workspace_bytes(65) == 0


def test_bucket_rejects_bad_arguments(built_lib):
    lib = built_lib
    buf = np.zeros(4096, np.int64)                    # a stand-in address: every call below fails before it is dereferenced
    p = ctypes.c_void_p(buf.ctypes.data)

    def call(**kw):
        a = dict(ids=p, offsets=p, weights=None, nnz=4, sb=2, sf=1, B=2, vocab=p, parts=None, first=None, F=2, P=2, sc=None, comb=1,
                 flags=0, cap_e=16, cap_b=16, slabs=p, pos=p, mask=p, denom=p, stat=None, ws=p)
        a.update(kw)
        return lib.dir_shard_bags_bucket(*a.values(), None)
    for name in ("vocab", "slabs", "ws", "offsets", "pos", "mask", "denom", "ids"):
        lib.dir_last_error()
        assert call(**{name: None}) == BADARG, name
        assert "dir_shard_bags_bucket" in _err(lib) and "null" in _err(lib)
    assert call(P=65) == BADARG and "P <= 64" in _err(lib)
    assert call(cap_e=1 << 31) == BADARG and "2^31" in _err(lib)
    assert call(cap_b=1 << 30) == BADARG and "2^31" in _err(lib)          # P * cap_b
    assert call(comb=3) == BADARG and "combiner" in _err(lib)
    assert call(F=0) == BADARG


def test_pool_rejects_bad_arguments_and_k(built_lib):
    lib = built_lib
    buf = np.zeros(4096, np.int64)
    p = ctypes.c_void_p((buf.ctypes.data + 15) // 16 * 16)

    def call(**kw):
        a = dict(tables=p, lv=p, F=2, K=16, recv=p, P=2, cap_e=16, cap_b=16, smn=None, mn=0.0, flags=0, out=p, stat=None)
        a.update(kw)
        return lib.dir_shard_bags_pool_f32(*a.values(), None)
    for name in ("tables", "lv", "recv", "out"):
        assert call(**{name: None}) == BADARG, name
        assert "dir_shard_bags_pool_f32" in _err(lib) and "null" in _err(lib)
    assert call(K=0) == BADARG and "K=0" in _err(lib)
    assert call(K=260) == UNSUPPORTED and "K=260" in _err(lib)            # 65 float4 chunks: wider than one wave
    assert call(K=65) == UNSUPPORTED and "K=65" in _err(lib)              # not a multiple of 4: one float per lane, at most 64
    assert call(mn=-1.0) == BADARG and "max_norm" in _err(lib)
    assert call(P=65) == BADARG


def test_combine_rejects_bad_arguments_and_k(built_lib):
    lib = built_lib
    buf = np.zeros(4096, np.int64)
    p = ctypes.c_void_p((buf.ctypes.data + 15) // 16 * 16)

    def call(**kw):
        a = dict(back=p, K=16, P=2, pos=p, mask=p, denom=p, B=4, F=2, sc=None, comb=1, out=p, ld=32, fm=None)
        a.update(kw)
        return lib.dir_shard_bags_combine_f32(*a.values(), None)
    for name in ("back", "pos", "mask", "denom", "out"):
        assert call(**{name: None}) == BADARG, name
        assert "dir_shard_bags_combine_f32" in _err(lib) and "null" in _err(lib)
    assert call(K=0) == BADARG
    assert call(K=260, ld=520) == UNSUPPORTED and "K=260" in _err(lib)
    assert call(K=65, ld=130) == UNSUPPORTED and "K=65" in _err(lib)
    assert call(ld=31) == BADARG and "out_ld" in _err(lib)
    assert call(comb=7) == BADARG and "combiner" in _err(lib)
