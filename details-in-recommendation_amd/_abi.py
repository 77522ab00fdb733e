"""_abi.py -- how torch tensors and streams go through the C ABI (include/dir_hip.h): the helpers ops.py and sparse_opt.py share.
A leaf module: it imports neither of them."""
import ctypes

import torch


def _stream():
    """The current HIP stream of the current device as the C ABI takes it.  (torch.cuda.current_stream() builds a Stream object per call:
    5.7 us, 30 times per DeepFM training step; the raw query is 0.3 us.)"""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (ROCm) tensor: the HIP path has no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _onehot_strides(ids, F):
    """ids [B,F] (any strides) or [F,B] given as transposed view -> (B, stride_b, stride_f)."""
    if ids.dim() != 2 or ids.shape[1] != F:
        raise ValueError("one-hot ids must be [B, F=%d], got %s" % (F, tuple(ids.shape)))
    return ids.shape[0], ids.stride(0), ids.stride(1)
