"""CPU tests of the dropout generator: the library's Philox4x32-10 and the NumPy restatement the GPU tests compare with both reproduce the
published Random123 known answers, and the host-side argument checks of the dropout entry points."""
import ctypes

import numpy as np

from tests import dropout_ref as R

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, result)
KATS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _lib_block(lib, ctr, key):
    c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    lib.dir_philox4x32_10(c, k, o)
    return tuple(o)


def test_library_philox_matches_published_vectors(built_lib):
    for ctr, key, exp in KATS:
        assert _lib_block(built_lib, ctr, key) == exp


def test_reference_philox_matches_published_vectors():
    for ctr, key, exp in KATS:
        assert tuple(int(w) for w in R.philox4x32_10([np.uint64(c) for c in ctr], key)) == exp


def test_library_and_reference_agree_on_the_dropout_counters(built_lib):
    # the counter layout of the kernels: (q low, q high, stream_id, draw), key = the seed's halves
    seed = 0x0123456789abcdef
    for q, sid, draw in [(0, 0, 0), (5, 7, 3), ((1 << 32) - 8, 1, 0xffffffff), (1 << 33, 2, 9)]:
        ctr = (q & 0xffffffff, q >> 32, sid, draw)
        key = (seed & 0xffffffff, seed >> 32)
        assert _lib_block(built_lib, ctr, key) == tuple(int(w) for w in R.philox4x32_10([np.uint64(c) for c in ctr], key))


def test_reference_mask_layout():
    # four consecutive elements share one block; `first` shifts the element index, not the block contents
    m = R.mask(64, 0.5, seed=11, draw=2, stream_id=3)
    assert np.array_equal(R.mask(40, 0.5, seed=11, draw=2, stream_id=3, first=24), m[24:])
    assert np.array_equal(R.mask(13, 0.5, seed=11, draw=2, stream_id=3, first=5), m[5:18])
    assert not np.array_equal(R.mask(64, 0.5, seed=11, draw=3, stream_id=3), m)
    assert not np.array_equal(R.mask(64, 0.5, seed=11, draw=2, stream_id=4), m)
    assert R.mask(4096, 0.0, seed=1).all()


def test_dropout_argument_errors_without_gpu(built_lib):
    st = ctypes.c_void_p(16)
    for rate in (1.0, -0.1, float("nan")):
        rc = built_lib.dir_dropout_f32(ctypes.c_void_p(16), ctypes.c_void_p(16), 4, 0, rate, st, 0, None, None, None)
        assert rc == -1 and b"rate" in built_lib.dir_last_error()
        rc = built_lib.dir_dropout_mask_u8(4, 0, rate, st, 0, None, ctypes.c_void_p(16), None)
        assert rc == -1 and b"rate" in built_lib.dir_last_error()
    assert built_lib.dir_dropout_f32(ctypes.c_void_p(16), ctypes.c_void_p(16), 4, 0, 0.5, None, 0, None, None, None) == -1
    assert built_lib.dir_dropout_f32(ctypes.c_void_p(16), ctypes.c_void_p(16), -1, 0, 0.5, st, 0, None, None, None) == -1
    assert built_lib.dir_dropout_advance(None, None) == -1
    rc = built_lib.dir_bn_affine_dropout_f32(ctypes.c_void_p(16), 6, ctypes.c_void_p(16), ctypes.c_void_p(16), 8, 6, ctypes.c_void_p(16), 6, 0.5, st, 0,
                                             None, None, None)
    assert rc == -4
