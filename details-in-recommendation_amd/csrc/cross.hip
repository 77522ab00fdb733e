// cross.hip -- feature crosses on the device: crossed_column's ids (bit-exact integer work).
//
// Replaces (reference):
//   tf.feature_column.crossed_column(["workclass", "education"], 128)      models/ESMM/train.py:94
//     [TF-upstream] _CrossedColumn -> SparseCross with hashed output: every leaf key contributes 64 bits per entry (an integer as it is, a
//     string's FarmHash Fingerprint64, a categorical column's id), chained through FingerprintCat64 from hash_key, modulo hash_bucket_size
//     (unsigned).  Stated from TensorFlow 1.x, not verified; the known answers in tests/ pin the formula as stated.
//
// One-hot keys: cross_onehot_k forms up to 16 crosses over up to 32 source columns in one launch.  Ragged keys: cross_ragged_count_k gives
// the per-row product sizes, the caller turns them into offsets, cross_ragged_fill_k is parallel over the OUTPUT entries.
#include "common.hpp"

namespace dir {

// [TF-upstream] FingerprintCat64(fp1, fp2) = FarmHash's Hash128to64 (Murmur-inspired) of the pair.  Host and device run this one function.
__host__ __device__ inline uint64_t fingerprint_cat64(uint64_t a, uint64_t b) {
    constexpr uint64_t kMul = 0xc6a4a7935bd1e995ULL;
    uint64_t r = a ^ kMul;
    uint64_t m = b * kMul;
    m ^= m >> 47;
    r ^= m * kMul;
    r *= kMul;
    r ^= r >> 47;
    r *= kMul;
    return r ^ (r >> 47);
}

constexpr int kCrossMaxKeys = 8;       // leaf keys per cross
constexpr int kCrossMax = 16;          // crosses per launch
constexpr int kCrossMaxSrc = 32;       // distinct source columns per launch (256 threads x 32 x 8 B = the 64 KB of LDS a workgroup may take)
constexpr int64_t kCrossSaturate = (int64_t)1 << 40;       // a row's product clamps here: 8.8 TB of ids, above any real capacity, and
                                                           // 2^22 such rows still sum inside int64

// The tables travel BY VALUE in the kernel arguments (as finish_groups_k's GroupPtrs): nothing to upload, nothing to keep alive.
struct CrossSources {
    const int64_t* p[kCrossMaxSrc];
    int64_t stride[kCrossMaxSrc];      // in elements: a column of a [B, F] id matrix is read in place
};
struct CrossPlan {
    uint64_t hash_key[kCrossMax];
    uint64_t buckets[kCrossMax];
    uint8_t nkeys[kCrossMax];
    uint8_t key[kCrossMax][kCrossMaxKeys];      // indices into CrossSources, in hashing order
};

// A thread takes a sample: its n_src source values go through LDS (slot [s][thread]: each is loaded from memory ONCE however many
// crosses use it; only the owning thread touches a slot, so there is no barrier), then every cross chains its keys from there.  The plan is
// indexed uniformly: scalar loads from the kernel arguments.  out is field-major [nx, B].
__global__ __launch_bounds__(256) void cross_onehot_k(CrossSources src, CrossPlan plan, int n_src, int nx, int64_t B,
                                                      int64_t* __restrict__ out) {
    extern __shared__ uint64_t cross_vals[];      // [n_src][256]
    uint64_t* mine = cross_vals + threadIdx.x;
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < B; b += (int64_t)gridDim.x * 256) {
        for (int s = 0; s < n_src; ++s) mine[s * 256] = (uint64_t)src.p[s][b * src.stride[s]];
        for (int x = 0; x < nx; ++x) {
            uint64_t h = plan.hash_key[x];
            const int nk = plan.nkeys[x];
            for (int k = 0; k < nk; ++k) h = fingerprint_cat64(h, mine[(int)plan.key[x][k] * 256]);
            out[(int64_t)x * B + b] = (int64_t)(h % plan.buckets[x]);
        }
    }
}

// One cross over ragged keys.  Key k: offsets[k] != nullptr -> row b holds values[k][offsets[k][b] .. offsets[k][b+1]);
// offsets[k] == nullptr -> the one entry values[k][b * stride[k]].
struct CrossRaggedKeys {
    const int64_t* values[kCrossMaxKeys];
    const int64_t* offsets[kCrossMaxKeys];
    int64_t stride[kCrossMaxKeys];
};

__global__ __launch_bounds__(256) void cross_ragged_count_k(CrossRaggedKeys keys, int nk, int64_t B, int64_t* __restrict__ counts) {
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < B; b += (int64_t)gridDim.x * 256) {
        int64_t prod = 1;
        for (int k = 0; k < nk; ++k) {
            if (!keys.offsets[k]) continue;
            int64_t len = keys.offsets[k][b + 1] - keys.offsets[k][b];
            if (len < 0) len = 0;
            if (len > kCrossSaturate) len = kCrossSaturate;      // (the comparison below runs before the multiply: no overflow)
            prod = (len != 0 && prod > kCrossSaturate / len) ? kCrossSaturate : prod * len;
        }
        counts[b] = prod;
    }
}

// A thread takes an OUTPUT entry e: its row is the last b with out_offsets[b] <= e (binary search; rows without entries are stepped over
// because their offset equals the next one's), the remainder decodes into per-key positions with the last key fastest, then the chain.
// out_offsets[B] must equal capacity, the number of words behind out: otherwise status = 1 and nothing is written.
__global__ __launch_bounds__(256) void cross_ragged_fill_k(CrossRaggedKeys keys, int nk, uint64_t hash_key, uint64_t buckets, int64_t B,
                                                           const int64_t* __restrict__ out_offsets, int64_t capacity,
                                                           int64_t* __restrict__ out, int32_t* __restrict__ status) {
    const bool ok = out_offsets[B] == capacity && out_offsets[0] == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = ok ? 0 : 1;
    if (!ok) return;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < capacity; e += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = B;                 // invariant: out_offsets[lo] <= e < out_offsets[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (out_offsets[mid] <= e) lo = mid; else hi = mid;
        }
        const int64_t b = lo;
        int64_t r = e - out_offsets[b];
        int64_t at[kCrossMaxKeys];              // where key k's entry lies in values[k]
        bool live = r >= 0;
#pragma unroll
        for (int k = kCrossMaxKeys - 1; k >= 0; --k) {
            at[k] = 0;
            if (k >= nk) continue;
            if (!keys.offsets[k]) {
                at[k] = b * keys.stride[k];
                continue;
            }
            const int64_t o0 = keys.offsets[k][b];
            const int64_t len = keys.offsets[k][b + 1] - o0;
            if (len <= 0) {                     // offsets that do not belong to these keys: read nothing, write nothing
                live = false;
                continue;
            }
            const int64_t q = r / len;
            at[k] = o0 + (r - q * len);
            r = q;
        }
        if (!live || r != 0) continue;
        uint64_t h = hash_key;
#pragma unroll
        for (int k = 0; k < kCrossMaxKeys; ++k)
            if (k < nk) h = fingerprint_cat64(h, (uint64_t)keys.values[k][at[k]]);
        out[e] = (int64_t)(h % buckets);
    }
}

}  // namespace dir

using namespace dir;

extern "C" uint64_t dir_fingerprint_cat64(uint64_t a, uint64_t b) { return fingerprint_cat64(a, b); }

extern "C" int dir_cross_onehot_i64(const int64_t* const* src_ptrs, const int64_t* src_strides, int n_src, const int32_t* key_index,
                                    const int32_t* key_count, const uint64_t* hash_keys, const int64_t* buckets, int nx, int64_t B,
                                    int64_t* out, dir_stream_t stream) {
    DIR_CHECK_ARG(n_src >= 1 && n_src <= kCrossMaxSrc, "dir_cross_onehot_i64: n_src=%d (1..%d source columns per launch)", n_src, kCrossMaxSrc);
    DIR_CHECK_ARG(nx >= 1 && nx <= kCrossMax, "dir_cross_onehot_i64: nx=%d (1..%d crosses per launch)", nx, kCrossMax);
    DIR_CHECK_ARG(B >= 0, "dir_cross_onehot_i64: B=%lld", (long long)B);
    DIR_CHECK_ARG(src_ptrs && src_strides && key_index && key_count && hash_keys && buckets, "dir_cross_onehot_i64: null pointer");
    CrossSources src;
    CrossPlan plan;
    memset(&src, 0, sizeof(src));
    memset(&plan, 0, sizeof(plan));
    int at = 0;
    for (int x = 0; x < nx; ++x) {
        DIR_CHECK_ARG(key_count[x] >= 2 && key_count[x] <= kCrossMaxKeys, "dir_cross_onehot_i64: cross %d has %d keys (2..%d)", x, key_count[x],
                      kCrossMaxKeys);
        DIR_CHECK_ARG(buckets[x] >= 1, "dir_cross_onehot_i64: cross %d: hash_bucket_size=%lld < 1", x, (long long)buckets[x]);
        plan.hash_key[x] = hash_keys[x];
        plan.buckets[x] = (uint64_t)buckets[x];
        plan.nkeys[x] = (uint8_t)key_count[x];
        for (int k = 0; k < key_count[x]; ++k, ++at) {
            DIR_CHECK_ARG(key_index[at] >= 0 && key_index[at] < n_src, "dir_cross_onehot_i64: cross %d key %d: source %d of %d", x, k,
                          key_index[at], n_src);
            plan.key[x][k] = (uint8_t)key_index[at];
        }
    }
    if (B == 0) return DIR_OK;
    DIR_CHECK_ARG(out, "dir_cross_onehot_i64: null pointer");
    for (int s = 0; s < n_src; ++s) {
        DIR_CHECK_ARG(src_ptrs[s], "dir_cross_onehot_i64: source %d is null", s);
        src.p[s] = src_ptrs[s];
        src.stride[s] = src_strides[s];
    }
    hipLaunchKernelGGL(cross_onehot_k, dim3(grid_for((B + 255) / 256)), dim3(256), (size_t)n_src * 256 * sizeof(uint64_t), as_stream(stream),
                       src, plan, n_src, nx, B, out);
    DIR_CHECK_LAUNCH("cross_onehot");
    return DIR_OK;
}

// the checks the two ragged entries share; -> DIR_OK and `keys` filled
static int cross_ragged_keys(const char* who, const int64_t* const* values, const int64_t* const* offsets, const int64_t* strides, int nk,
                             bool need_values, CrossRaggedKeys* keys) {
    DIR_CHECK_ARG(nk >= 2 && nk <= kCrossMaxKeys, "%s: %d keys (2..%d)", who, nk, kCrossMaxKeys);
    DIR_CHECK_ARG(offsets && (!need_values || (values && strides)), "%s: null pointer", who);
    memset(keys, 0, sizeof(*keys));
    for (int k = 0; k < nk; ++k) {
        DIR_CHECK_ARG(!need_values || values[k], "%s: key %d has no values", who, k);
        keys->values[k] = need_values ? values[k] : nullptr;
        keys->offsets[k] = offsets[k];
        keys->stride[k] = strides ? strides[k] : 1;
    }
    return DIR_OK;
}

extern "C" int dir_cross_ragged_count_i64(const int64_t* const* offsets, int nk, int64_t B, int64_t* counts, dir_stream_t stream) {
    CrossRaggedKeys keys;
    const int rc = cross_ragged_keys("dir_cross_ragged_count_i64", nullptr, offsets, nullptr, nk, false, &keys);
    if (rc != DIR_OK) return rc;
    DIR_CHECK_ARG(B >= 0, "dir_cross_ragged_count_i64: B=%lld", (long long)B);
    if (B == 0) return DIR_OK;
    DIR_CHECK_ARG(counts, "dir_cross_ragged_count_i64: null pointer");
    hipLaunchKernelGGL(cross_ragged_count_k, dim3(grid_for((B + 255) / 256)), dim3(256), 0, as_stream(stream), keys, nk, B, counts);
    DIR_CHECK_LAUNCH("cross_ragged_count");
    return DIR_OK;
}

extern "C" int dir_cross_ragged_fill_i64(const int64_t* const* values, const int64_t* const* offsets, const int64_t* strides, int nk,
                                         uint64_t hash_key, int64_t buckets, int64_t B, const int64_t* out_offsets, int64_t capacity,
                                         int64_t* out, int32_t* status, dir_stream_t stream) {
    CrossRaggedKeys keys;
    const int rc = cross_ragged_keys("dir_cross_ragged_fill_i64", values, offsets, strides, nk, true, &keys);
    if (rc != DIR_OK) return rc;
    DIR_CHECK_ARG(B >= 0 && capacity >= 0 && buckets >= 1, "dir_cross_ragged_fill_i64: B=%lld capacity=%lld hash_bucket_size=%lld", (long long)B,
                  (long long)capacity, (long long)buckets);
    DIR_CHECK_ARG(out_offsets && status && (out || capacity == 0), "dir_cross_ragged_fill_i64: null pointer");
    // (capacity == 0 still launches: the status word is the kernel's to write)
    hipLaunchKernelGGL(cross_ragged_fill_k, dim3(grid_for((capacity + 255) / 256)), dim3(256), 0, as_stream(stream), keys, nk, hash_key,
                       (uint64_t)buckets, B, out_offsets, capacity, out, status);
    DIR_CHECK_LAUNCH("cross_ragged_fill");
    return DIR_OK;
}
