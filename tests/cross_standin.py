"""A pure-Python restatement of crossed_column's semantics as the project states them ([TF-upstream] _CrossedColumn / SparseCross with
hashed output; DESIGN.md section 2: stated, not verified): the FingerprintCat64 chain and the product order of ragged keys.  Strings go
through oracle/np_ref.py's FarmHash64.  Shared by tests/test_cross_host.py and tests/test_gpu_cross.py; nothing here touches the library."""
import numpy as np

M64 = (1 << 64) - 1
KMUL = 0xc6a4a7935bd1e995
HASH_KEY = 0xDECAFCAFFE


def shift_mix(v):
    return v ^ (v >> 47)


def cat64(a, b):
    a, b = int(a) & M64, int(b) & M64
    r = a ^ KMUL
    r ^= (shift_mix((b * KMUL) & M64) * KMUL) & M64
    r = (r * KMUL) & M64
    r = (shift_mix(r) * KMUL) & M64
    return shift_mix(r)


def contribution(v):
    """64 bits of one entry: an integer as it is (two's complement), a string's Fingerprint64."""
    if isinstance(v, (bytes, str)):
        from oracle import np_ref as R
        return int(R.fingerprint64(v.encode("utf-8") if isinstance(v, str) else v)) & M64
    return int(v) & M64


def cross_id(entries, hash_bucket_size, hash_key=HASH_KEY):
    h = int(hash_key) & M64
    for v in entries:
        h = cat64(h, contribution(v))
    return h % int(hash_bucket_size)


def cross_onehot(columns, hash_bucket_size, hash_key=HASH_KEY):
    """columns: one sequence [B] per key, in hashing order -> int64 ids [B]."""
    return np.array([cross_id(row, hash_bucket_size, hash_key) for row in zip(*columns)], dtype=np.uint64).astype(np.int64)


def cross_ragged(keys, hash_bucket_size, hash_key=HASH_KEY):
    """keys: per key either a sequence [B] (one entry per row) or (values, offsets [B+1]).  -> (ids, offsets [B+1]): row b holds the
    cartesian product of the keys' entries of row b, the LAST key fastest; a row in which a key is empty has no entries."""
    def rows_of(k):
        if isinstance(k, tuple):
            v, o = k
            return [list(v[int(o[b]):int(o[b + 1])]) for b in range(len(o) - 1)]
        return [[x] for x in k]

    per_key = [rows_of(k) for k in keys]
    B = len(per_key[0])
    out, offs = [], [0]
    for b in range(B):
        combos = [[]]
        for rows in per_key:                     # extending on the right makes the last key the fastest
            combos = [c + [e] for c in combos for e in rows[b]]
        out += [cross_id(c, hash_bucket_size, hash_key) for c in combos]
        offs.append(len(out))
    return np.array(out, dtype=np.uint64).astype(np.int64), np.array(offs, dtype=np.int64)
