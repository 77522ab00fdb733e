"""CPU tests of the grouped ranking metrics' C ABI: argument validation happens before any HIP call, so it is testable without a GPU."""
import ctypes

import pytest


def _p(v=64):
    return ctypes.c_void_p(v)


def test_group_rank_limits(built_lib):
    from dir_amd import ops
    w, t = ctypes.c_int(), ctypes.c_int()
    assert built_lib.dir_group_rank_limits(ctypes.byref(w), ctypes.byref(t)) == 0
    assert w.value >= 64 and w.value % 64 == 0                   # whole waves' worth of entries
    assert t.value > w.value and t.value % 4 == 0                # 16-byte LDS reads
    assert ops.group_rank_limits() == (w.value, t.value)
    assert built_lib.dir_group_rank_limits(None, ctypes.byref(t)) == -1 and b"null pointer" in built_lib.dir_last_error()


def test_group_rank_stats_argument_errors_without_gpu(built_lib):
    f = built_lib.dir_group_rank_stats_f32
    ok = [_p(), _p(), None, _p(), 1] + [_p()] * 7 + [None]        # scores, labels, weights (NULL is legal), offsets, G, seven outputs, stream
    rc = f(*(ok[:4] + [-1] + ok[5:]))
    assert rc == -1 and b"G=-1" in built_lib.dir_last_error()
    for k in [0, 1, 3] + list(range(5, 12)):                     # every pointer but weights
        args = list(ok)
        args[k] = None
        assert f(*args) == -1 and b"null pointer" in built_lib.dir_last_error(), k
    # G == 0 is a no-op (no launch: this machine has no GPU to launch on); offsets is still required
    assert f(None, None, None, _p(), 0, None, None, None, None, None, None, None, None) == 0
    assert f(None, None, None, None, 0, None, None, None, None, None, None, None, None) == -1


def test_ops_group_rank_stats_refuses_cpu_tensors(built_lib):
    import torch
    from dir_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.group_rank_stats(torch.zeros(4), torch.zeros(4), None, torch.tensor([0, 4]))
