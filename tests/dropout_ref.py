"""The dropout mask layout of csrc/dropout.hip restated in NumPy: Philox4x32-10 as published (Salmon et al., SC'11) and the element -> counter
map of include/dir_hip.h.  The reference of tests/test_dropout_host.py and tests/test_gpu_dropout.py."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(c, k):
    """c: four uint64 arrays holding 32-bit counter words, k: two 32-bit key words -> four uint64 arrays of 32-bit results."""
    c = [np.asarray(w, dtype=np.uint64) for w in c]
    k0, k1, lo32 = np.uint64(k[0]), np.uint64(k[1]), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]              # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & lo32]
        k0, k1 = (k0 + np.uint64(W0)) & lo32, (k1 + np.uint64(W1)) & lo32
    return c


def mask(n, rate, seed, draw=0, stream_id=0, first=0):
    """uint8 [n]: 1 where element first + i is kept."""
    e = np.uint64(first) + np.arange(n, dtype=np.uint64)
    q = e >> np.uint64(2)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full(n, stream_id, np.uint64), np.full(n, draw & 0xFFFFFFFF, np.uint64)],
                      [seed & 0xFFFFFFFF, seed >> 32])
    word = np.choose((e & np.uint64(3)).astype(np.int64), r)
    u = (word >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(rate)).astype(np.uint8)
