"""CPU tests of the matrix-factorisation entry points' C ABI (csrc/mf.hip): argument validation happens before any HIP call, so it is
testable without a GPU."""
import ctypes

import pytest


def _p(v=64):
    return ctypes.c_void_p(v)


def _score_args(**kw):
    a = dict(P=_p(), Q=_p(), bu=_p(), bi=_p(), b0=_p(), ids=_p(), sb=3, sf=1, B=5, C=2, K=16, logits=_p(), stream=None)
    a.update(kw)
    return [a[k] for k in ("P", "Q", "bu", "bi", "b0", "ids", "sb", "sf", "B", "C", "K", "logits", "stream")]


def _bwd_args(**kw):
    a = dict(P=_p(), Q=_p(), bu=_p(), bi=_p(), ids=_p(), sb=3, sf=1, dl=_p(), l2=0.0, B=5, C=2, K=16, grad=_p(), gbias=_p(), stream=None)
    a.update(kw)
    return [a[k] for k in ("P", "Q", "bu", "bi", "ids", "sb", "sf", "dl", "l2", "B", "C", "K", "grad", "gbias", "stream")]


def _neg_args(**kw):
    a = dict(users=_p(), B=5, offsets=_p(), items=_p(), num_items=10, n_neg=2, state=_p(), stream_id=0, first=0, out=_p(), status=_p(), stream=None)
    a.update(kw)
    return [a[k] for k in ("users", "B", "offsets", "items", "num_items", "n_neg", "state", "stream_id", "first", "out", "status", "stream")]


@pytest.mark.parametrize("entry,make", [("dir_mf_score_f32", _score_args), ("dir_mf_score_backward_f32", _bwd_args)])
def test_mf_score_argument_errors_without_gpu(built_lib, entry, make):
    f = getattr(built_lib, entry)
    for bad, text in ((dict(K=6), b"K=6"), (dict(K=260), b"K=260"), (dict(K=0), b"K=0"), (dict(C=0), b"C=0"), (dict(B=-1), b"B=-1"),
                      (dict(P=None), b"null pointer"), (dict(Q=None), b"null pointer"), (dict(ids=None), b"null pointer"),
                      (dict(bi=None), b"bu and bi go together"), (dict(bu=None), b"bu and bi go together"), (dict(P=_p(68)), b"16-byte aligned")):
        assert f(*make(**bad)) == -1 and text in built_lib.dir_last_error(), bad
    # B == 0 is a no-op (no launch: this machine has no GPU to launch on), with or without biases
    assert f(*make(B=0)) == 0
    assert f(*make(B=0, bu=None, bi=None)) == 0


def test_mf_score_output_pointers(built_lib):
    assert built_lib.dir_mf_score_f32(*_score_args(logits=None)) == -1 and b"null pointer" in built_lib.dir_last_error()
    assert built_lib.dir_mf_score_backward_f32(*_bwd_args(grad=None)) == -1 and b"null pointer" in built_lib.dir_last_error()
    assert built_lib.dir_mf_score_backward_f32(*_bwd_args(dl=None)) == -1 and b"null pointer" in built_lib.dir_last_error()
    assert built_lib.dir_mf_score_backward_f32(*_bwd_args(grad=_p(72))) == -1 and b"16-byte aligned" in built_lib.dir_last_error()
    assert built_lib.dir_mf_score_backward_f32(*_bwd_args(l2=-0.5)) == -1 and b"l2=" in built_lib.dir_last_error()


def test_neg_sample_argument_errors_without_gpu(built_lib):
    f = built_lib.dir_neg_sample_i64
    for bad, text in ((dict(n_neg=0), b"n_neg=0"), (dict(num_items=0), b"num_items=0"), (dict(num_items=-3), b"num_items=-3"), (dict(B=-1), b"B=-1"),
                      (dict(first=-1), b"first=-1"), (dict(first=(1 << 63) - 5), b"overflows"), (dict(offsets=None), b"null pointer"),
                      (dict(state=None), b"null pointer"), (dict(users=None), b"null pointer"), (dict(out=None), b"null pointer"),
                      (dict(status=None), b"null pointer")):
        assert f(*_neg_args(**bad)) == -1 and text in built_lib.dir_last_error(), bad
    assert f(*_neg_args(B=0)) == 0
    assert f(*_neg_args(B=0, users=None, items=None, out=None, status=None)) == 0


def test_ops_mf_refuse_cpu_tensors_and_bad_shapes(built_lib):
    import torch
    from dir_amd import ops
    P, Q, ids = torch.zeros(4, 8), torch.zeros(5, 8), torch.zeros(3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mf_score(P, Q, ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mf_score_backward(P, Q, ids, torch.zeros(3, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.neg_sample(torch.zeros(3, dtype=torch.int64), ops.UserItems(torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 4), 2, None)
