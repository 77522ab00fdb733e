// dropout.hip -- dropout of the DNN towers in TRAIN mode, with masks from a counter-based generator: no mask is ever stored.
//
// Reference: core_layers.dropout(net, rate, training=True) after the hidden layers (models/DeepFM/deepFM.py:301-302,
// models/DeepCrossNetwork/DeepCrossNetwork.py:405-408, models/ESMM/ESMM.py:143-144); [TF-upstream] nn.dropout computes
// out = (x / keep_prob) * m with m in {0, 1}, keep_prob = 1 - rate.  The division is the correctly rounded one and m multiplies, so a dropped
// NaN / inf stays NaN as there.  The masks are THIS library's stream, not TensorFlow's:
//
//   Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85), one 128-bit block per four
//   consecutive elements.  Element e = first + (flat index into the contiguous tensor):  q = e >> 2, lane = e & 3,
//   counter = (q & 0xffffffff, q >> 32, stream_id, draw), key = (seed & 0xffffffff, seed >> 32), u = float(r[lane] >> 8) * 2^-24, keep iff u >= rate.
//
// state is a device int64[2] = (seed, draw): the host never reads it on the training path.  The forward takes both words from state and one
// thread leaves them in used_out (16 bytes: all the backward needs); the backward takes BOTH from used_in and does not look at state, so the
// gradient gets the forward's mask whatever has happened to state since (an advance, a manual_seed, a set_state).  dir_dropout_advance adds 1
// to draw (one thread).  Everything is a kernel launch: capturable in a HIP graph.
//
// Elementwise: 8 B of traffic and ten Philox rounds (two 32 x 32 -> 64 multiplies each) per four elements; what a site costs inside a training
// step is in profiles/NOTES.md R9.1 (the kernels alone have not been timed against the copy ceiling).  Compiled without packed fp32 VALU
// instructions (build.py: NO_PACKED_FP32): the kernels may share a SIMD with another stream's bf16-MFMA kernel.
#include "common.hpp"
#include "philox.hpp"      // Philox4, philox4x32_10 (shared with csrc/mf.hip's negative sampler)

namespace dir {

// What every kernel of this file needs to make the mask of element e
struct DropCtx {
    uint32_t k0, k1, stream_id, draw;
    float rate;
};

__device__ __forceinline__ DropCtx drop_ctx(const int64_t* __restrict__ state, const int64_t* __restrict__ used_in, uint32_t stream_id, float rate) {
    DropCtx c;
    const int64_t* __restrict__ src = used_in ? used_in : state;      // (seed, draw): the forward's own words in the backward
    const uint64_t seed = (uint64_t)src[0];
    c.k0 = (uint32_t)seed;
    c.k1 = (uint32_t)(seed >> 32);
    c.stream_id = stream_id;
    c.draw = (uint32_t)(uint64_t)src[1];
    c.rate = rate;
    return c;
}

__device__ __forceinline__ bool drop_keep_word(uint32_t r, float rate) { return (float)(r >> 8) * 0x1p-24f >= rate; }

__device__ __forceinline__ Philox4 drop_block(const DropCtx& c, uint64_t q) {
    return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), c.stream_id, c.draw, c.k0, c.k1);
}

// keep[k] for the four elements e0 .. e0 + 3 of ONE block (e0 a multiple of 4: the host sends a `first` that is not to the one-element path,
// so no word is ever picked by a run-time index -- that put the block into scratch memory)
__device__ __forceinline__ void drop_keep4(const DropCtx& c, uint64_t e0, bool keep[4]) {
    const Philox4 a = drop_block(c, e0 >> 2);
#pragma unroll
    for (int k = 0; k < 4; ++k) keep[k] = drop_keep_word(a.v[k], c.rate);
}

__device__ __forceinline__ bool drop_keep1(const DropCtx& c, uint64_t e) {
    const Philox4 a = drop_block(c, e >> 2);
    const uint32_t l = (uint32_t)(e & 3);
    return drop_keep_word(l == 0 ? a.v[0] : (l == 1 ? a.v[1] : (l == 2 ? a.v[2] : a.v[3])), c.rate);
}

// (x / keep_prob) * m, the division correctly rounded (no reciprocal), m = 0 multiplies: NaN / inf inputs stay non-finite as in the reference
__device__ __forceinline__ float drop_apply(float x, float keep_prob, bool keep) { return __fdiv_rn(x, keep_prob) * (keep ? 1.0f : 0.0f); }

// out[i] = dropout(x[i]), i < n; element i is e = first + i.  VEC: x and out are 16-byte aligned and first is a multiple of 4 -- quads i = 4 j .. 4 j + 3 move as one
// load / store, the tail of n % 4 elements (and everything when !VEC) one element per thread.  rate == 0: a copy.  out may alias x.
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_k(const float* x, float* out, int64_t n, int64_t first, float rate, const int64_t* __restrict__ state,
                                                  uint32_t stream_id, const int64_t* __restrict__ used_in, int64_t* __restrict__ used_out) {
    const DropCtx c = drop_ctx(state, used_in, stream_id, rate);
    const float keep_prob = 1.0f - rate;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    if (used_out && tid == 0) {
        used_out[0] = (int64_t)(((uint64_t)c.k1 << 32) | c.k0);
        used_out[1] = (int64_t)c.draw;
    }
    const int64_t nvec = VEC ? (n >> 2) : 0;
    for (int64_t j = tid; j < nvec; j += nthr) {
        const float4 v = *reinterpret_cast<const float4*>(x + 4 * j);
        float4 o = v;
        if (rate != 0.0f) {
            bool keep[4];
            drop_keep4(c, (uint64_t)(first + 4 * j), keep);
            o.x = drop_apply(v.x, keep_prob, keep[0]);
            o.y = drop_apply(v.y, keep_prob, keep[1]);
            o.z = drop_apply(v.z, keep_prob, keep[2]);
            o.w = drop_apply(v.w, keep_prob, keep[3]);
        }
        *reinterpret_cast<float4*>(out + 4 * j) = o;
    }
    for (int64_t i = 4 * nvec + tid; i < n; i += nthr) {
        const float v = x[i];
        out[i] = rate != 0.0f ? drop_apply(v, keep_prob, drop_keep1(c, (uint64_t)(first + i))) : v;
    }
}

// out[i] = 1 if element first + i is kept, else 0 (tests and diagnostics); four bytes per thread where out is 4-byte aligned and first % 4 == 0
__global__ __launch_bounds__(256) void dropout_mask_k(uint8_t* __restrict__ out, int64_t n, int64_t first, float rate, const int64_t* __restrict__ state,
                                                       uint32_t stream_id, const int64_t* __restrict__ used_in, int vec) {
    const DropCtx c = drop_ctx(state, used_in, stream_id, rate);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const int64_t nvec = vec ? (n >> 2) : 0;
    for (int64_t j = tid; j < nvec; j += nthr) {
        bool keep[4];
        drop_keep4(c, (uint64_t)(first + 4 * j), keep);
        const uint32_t w = (keep[0] ? 1u : 0u) | (keep[1] ? 0x100u : 0u) | (keep[2] ? 0x10000u : 0u) | (keep[3] ? 0x1000000u : 0u);
        *reinterpret_cast<uint32_t*>(out + 4 * j) = w;
    }
    for (int64_t i = 4 * nvec + tid; i < n; i += nthr) out[i] = drop_keep1(c, (uint64_t)(first + i)) ? 1 : 0;
}

// out[r, c] = dropout(y[r, c] * scale[c] + shift[c]): the batch-norm affine and the dropout behind it (DCN's order) in one pass.  N a multiple
// of 4, so a quad never crosses a row; element index e = r N + c (out's values as a contiguous [B, N] tensor).
__global__ __launch_bounds__(256) void bn_affine_dropout_k(const float* __restrict__ y, int64_t y_ld, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, int64_t B, int N, float* __restrict__ out, int64_t out_ld,
                                                            float rate, const int64_t* __restrict__ state, uint32_t stream_id,
                                                            const int64_t* __restrict__ used_in, int64_t* __restrict__ used_out) {
    const DropCtx c = drop_ctx(state, used_in, stream_id, rate);
    const float keep_prob = 1.0f - rate;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    if (used_out && tid == 0) {
        used_out[0] = (int64_t)(((uint64_t)c.k1 << 32) | c.k0);
        used_out[1] = (int64_t)c.draw;
    }
    const int nv = N >> 2;
    const int64_t total = B * (int64_t)nv;
    for (int64_t j = tid; j < total; j += nthr) {
        const int64_t r = j / nv;
        const int cq = (int)(j - r * nv);
        const float4 v = *reinterpret_cast<const float4*>(y + r * y_ld + 4 * cq);
        const float4 sc = *reinterpret_cast<const float4*>(scale + 4 * cq), sh = *reinterpret_cast<const float4*>(shift + 4 * cq);
        float4 o;
        o.x = fmaf(v.x, sc.x, sh.x); o.y = fmaf(v.y, sc.y, sh.y); o.z = fmaf(v.z, sc.z, sh.z); o.w = fmaf(v.w, sc.w, sh.w);
        if (rate != 0.0f) {
            bool keep[4];
            drop_keep4(c, (uint64_t)(4 * j), keep);
            o.x = drop_apply(o.x, keep_prob, keep[0]);
            o.y = drop_apply(o.y, keep_prob, keep[1]);
            o.z = drop_apply(o.z, keep_prob, keep[2]);
            o.w = drop_apply(o.w, keep_prob, keep[3]);
        }
        *reinterpret_cast<float4*>(out + r * out_ld + 4 * cq) = o;
    }
}

__global__ void dropout_advance_k(int64_t* __restrict__ state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] = (int64_t)(((uint64_t)state[1] + 1u) & 0xffffffffull);
}

static int drop_check(const char* name, int64_t n, int64_t first, float rate, const void* state) {
    DIR_CHECK_ARG(n >= 0 && first >= 0, "%s: n=%lld first=%lld", name, (long long)n, (long long)first);
    DIR_CHECK_ARG(rate >= 0.0f && rate < 1.0f, "%s: rate=%g must lie in [0, 1)", name, (double)rate);
    DIR_CHECK_ARG(state != nullptr, "%s: null pointer (state)", name);
    DIR_CHECK_ARG(first <= INT64_MAX - n, "%s: first + n overflows", name);
    return DIR_OK;
}

}  // namespace dir

using namespace dir;

extern "C" void dir_philox4x32_10(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4) {
    const Philox4 r = philox4x32_10(counter4[0], counter4[1], counter4[2], counter4[3], key2[0], key2[1]);
    for (int i = 0; i < 4; ++i) out4[i] = r.v[i];
}

extern "C" int dir_dropout_f32(const float* x, float* out, int64_t n, int64_t first, float rate, const int64_t* state, uint32_t stream_id,
                               const int64_t* used_in, int64_t* used_out, dir_stream_t stream) {
    const char* name = "dir_dropout_f32";
    if (int rc = drop_check(name, n, first, rate, state)) return rc;
    DIR_CHECK_ARG(n == 0 || (x && out), "%s: null pointer", name);
    DIR_CHECK_ARG(((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 3u) == 0, "%s: x / out must be 4-byte aligned", name);
    if (n == 0 && !used_out) return DIR_OK;
    const bool vec = aligned16(x) && aligned16(out) && (first & 3) == 0;
    const int grid = grid_for(((vec ? (n + 3) / 4 : n) + 255) / 256);
    if (vec)
        hipLaunchKernelGGL(dropout_k<true>, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x, out, n, first, rate, state, stream_id, used_in, used_out);
    else
        hipLaunchKernelGGL(dropout_k<false>, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x, out, n, first, rate, state, stream_id, used_in, used_out);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_dropout_mask_u8(int64_t n, int64_t first, float rate, const int64_t* state, uint32_t stream_id, const int64_t* used,
                                   uint8_t* out, dir_stream_t stream) {
    const char* name = "dir_dropout_mask_u8";
    if (int rc = drop_check(name, n, first, rate, state)) return rc;
    DIR_CHECK_ARG(n == 0 || out, "%s: null pointer", name);
    if (n == 0) return DIR_OK;
    const int vec = (((uintptr_t)out & 3u) == 0 && (first & 3) == 0) ? 1 : 0;
    const int grid = grid_for(((vec ? (n + 3) / 4 : n) + 255) / 256);
    hipLaunchKernelGGL(dropout_mask_k, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), out, n, first, rate, state, stream_id, used, vec);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_dropout_advance(int64_t* state, dir_stream_t stream) {
    const char* name = "dir_dropout_advance";
    DIR_CHECK_ARG(state != nullptr, "%s: null pointer", name);
    hipLaunchKernelGGL(dropout_advance_k, dim3(1), dim3(64), 0, as_stream(stream), state);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_bn_affine_dropout_f32(const float* y, int64_t y_ld, const float* scale, const float* shift, int64_t B, int N, float* out,
                                         int64_t out_ld, float rate, const int64_t* state, uint32_t stream_id, const int64_t* used_in,
                                         int64_t* used_out, dir_stream_t stream) {
    const char* name = "dir_bn_affine_dropout_f32";
    DIR_CHECK_ARG(B > 0 && N > 0, "%s: B=%lld N=%d", name, (long long)B, N);
    if (int rc = drop_check(name, B, 0, rate, state)) return rc;
    DIR_CHECK_ARG(y && scale && shift && out, "%s: null pointer", name);
    if (N % 4 || y_ld % 4 || out_ld % 4) return fail(DIR_E_UNSUPPORTED, "%s: N=%d and the row strides must be multiples of 4", name, N);
    DIR_CHECK_ARG(y_ld >= N && out_ld >= N, "%s: row strides smaller than N", name);
    if (!(aligned16(y) && aligned16(out) && aligned16(scale) && aligned16(shift)))
        return fail(DIR_E_BADARG, "%s: y / out / scale / shift must be 16-byte aligned", name);
    const int grid = grid_for((B * (int64_t)(N / 4) + 255) / 256);
    hipLaunchKernelGGL(bn_affine_dropout_k, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), y, y_ld, scale, shift, B, N, out, out_ld, rate, state,
                       stream_id, used_in, used_out);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}
