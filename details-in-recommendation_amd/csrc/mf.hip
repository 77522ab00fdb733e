// mf.hip -- the matrix-factorisation family (BiasedMF / Svd / BPR): fused gather-and-score, its backward, and the negative sampler.
//
// Reference: models/LFM/Mixture_1/MF_model.py:164-194 (_logit_fn: reduce_sum(user_emb * item_emb, 1) + (user_bias + item_bias) + global_bias)
// and :196-206 (reg_pen * l2_loss of the LOOKED-UP rows: per occurrence); models/LFM/Mixture_2/model.py:74-90 (no biases);
// models/BPR/bpr_sampler.py:102-111 (a negative redrawn until the user has not interacted with it).
//
// ids [B, 1 + C] int64 (any strides): column 0 the row of P [U, K], columns 1 .. C rows of Q [I, K]; 0 <= id < vocab is the caller's
// precondition (ops.check_ids is the debugging aid).  K % 4 == 0, 4 <= K <= 256.  A sample is handled by L lanes, L the smallest power of two
// >= K / 4 (lanes past K / 4 are masked: they load nothing and add zeros); lane l holds floats 4 l .. 4 l + 3 of a row as ONE 16-byte load;
// a wave handles 64 / L samples, a workgroup 256 / L; grid-stride over those groups of samples.
//
//   score     logits[b, c] = sum_k P[u, k] Q[i_c, k] (+ (bu[u] + bi[i_c]) + b0).  The user row is loaded once and stays in registers over
//             the C candidates; the candidates go four at a time: four ids, then four independent row loads, before the first is consumed.
//             The dot: ((p0 q0 + p1 q1) + p2 q2) + p3 q3 in a lane (no contraction: -ffp-contract=off), then the xor butterfly over the L
//             lanes (offsets L/2 .. 1): a fixed tree, so two runs give the same bits.  Of a quad of candidates lane j stores result j.
//   backward  grad [B, (1 + C) K]: slot 0 = sum_c dl[b, c] Q[i_c] (+ l2 P[u]), added in c order; slot 1 + c = dl[b, c] P[u] (+ l2 Q[i_c]).
//             gbias [B, 1 + C]: sum_c dl[b, c] (+ l2 bu[u]) and dl[b, c] (+ l2 bi[i_c]).  These are the slabs the sorted sparse optimisers take
//             with the same ids matrix.  The rows are re-read: no [B, C, K] tensor is saved.  l2 == 0 skips the l2 terms.  No cross-lane op.
//   sampler   out[b, c] = an item drawn uniformly from the num_items - n_u items user users[b] has NOT interacted with, without rejection:
//             offsets [U + 1] / items: a CSR of every user's items, ascending and distinct.  k uniform in [0, num_items - n_u); p = the
//             smallest position with items[p] - p > k (n_u if none: a binary search of at most 64 steps); the item is k + p.
//             One Philox4x32-10 block (philox.hpp) per draw.  Draw e = first + b n_neg + c (64 bits):
//                 counter = (e & 0xffffffff, e >> 32, stream_id, draw), key = (seed & 0xffffffff, seed >> 32)
//             with (seed, draw) the two words of state (device int64[2], the same pair as dropout.hip's: ops.DropoutState);
//             w = r[0] | r[1] << 32, k = mulhi64(w, num_items - n_u) = floor(w (num_items - n_u) / 2^64).  Bias: an item's probability differs
//             from 1 / (num_items - n_u) by less than 2^-64, i.e. relatively by at most (num_items - n_u) / 2^64.
//             A user with n_u >= num_items has no negative: out = -1 and status[0] = 1 (a plain store of the same value by every such thread;
//             the caller zeroes status).
//
// All three are launch-only: no host read, no atomics, no spin; every loop's trip count is bounded by the arguments.  Capturable in a HIP graph.
// Compiled without packed fp32 VALU instructions (build.py: NO_PACKED_FP32): a training or evaluation stream may share a SIMD with another
// stream's bf16-MFMA kernel.
#include "common.hpp"
#include "philox.hpp"

namespace dir {

constexpr int kMfQuad = 4;      // candidate rows in flight per lane

__device__ __forceinline__ float4 mf_row4(const float* __restrict__ T, int64_t row, int K, int l, bool on) {
    return on ? *reinterpret_cast<const float4*>(T + row * (int64_t)K + 4 * l) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

template <int L>
__global__ __launch_bounds__(256) void mf_score_k(const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ bu,
                                                   const float* __restrict__ bi, const float* __restrict__ b0, const int64_t* __restrict__ ids,
                                                   int64_t sb, int64_t sf, int64_t B, int C, int K, float* __restrict__ logits) {
    constexpr int SPB = 256 / L;                    // samples per workgroup
    const int l = (int)threadIdx.x & (L - 1), sub = (int)threadIdx.x / L;
    const bool on = 4 * l < K;
    const int64_t nblk = (B + SPB - 1) / SPB;
    const float g0 = b0 ? b0[0] : 0.0f;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t s = blk * SPB + sub;
        const bool valid = s < B;                   // (a sample past the end reads sample B - 1 and stores nothing: all lanes stay in the butterfly)
        const int64_t* __restrict__ row = ids + (valid ? s : B - 1) * sb;
        const int64_t u = row[0];
        const float4 p = mf_row4(P, u, K, l, on);
        const float bub = bu ? bu[u] : 0.0f;
        for (int c0 = 0; c0 < C; c0 += kMfQuad) {
            int64_t it[kMfQuad];
            float4 q[kMfQuad];
            float bb[kMfQuad];
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) it[j] = row[(int64_t)(1 + min(c0 + j, C - 1)) * sf];
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) q[j] = mf_row4(Q, it[j], K, l, on);
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) bb[j] = bi ? bi[it[j]] : 0.0f;
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) {
                float d = p.x * q[j].x;
                d = d + p.y * q[j].y;
                d = d + p.z * q[j].z;
                d = d + p.w * q[j].w;
                d = group_sum<L>(d);
                if (bu) {
                    float t = bub + bb[j];          // (bu + bi) + b0: MF_model.py:184
                    if (b0) t = t + g0;
                    d = d + t;
                } else if (b0) {
                    d = d + g0;
                }
                if (valid && c0 + j < C && l == (j & (L - 1))) logits[s * (int64_t)C + c0 + j] = d;
            }
        }
    }
}

template <int L>
__global__ __launch_bounds__(256) void mf_score_bwd_k(const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ bu,
                                                       const float* __restrict__ bi, const int64_t* __restrict__ ids, int64_t sb, int64_t sf,
                                                       const float* __restrict__ dlogits, float l2, int64_t B, int C, int K,
                                                       float* __restrict__ grad, float* __restrict__ gbias) {
    constexpr int SPB = 256 / L;
    const int l = (int)threadIdx.x & (L - 1), sub = (int)threadIdx.x / L;
    const bool on = 4 * l < K;
    const bool reg = l2 != 0.0f;
    const int64_t nblk = (B + SPB - 1) / SPB;
    const int64_t ldg = (int64_t)(1 + C) * K;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t s = blk * SPB + sub;
        if (s >= B) continue;                       // (no cross-lane operation in this kernel)
        const int64_t* __restrict__ row = ids + s * sb;
        const int64_t u = row[0];
        const float4 p = mf_row4(P, u, K, l, on);
        float* __restrict__ g = grad + s * ldg + 4 * l;
        float* __restrict__ gb = gbias ? gbias + s * (int64_t)(1 + C) : nullptr;
        float4 gu = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float sdl = 0.0f;
        for (int c0 = 0; c0 < C; c0 += kMfQuad) {
            int64_t it[kMfQuad];
            float4 q[kMfQuad];
            float d[kMfQuad];
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) it[j] = row[(int64_t)(1 + min(c0 + j, C - 1)) * sf];
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) q[j] = mf_row4(Q, it[j], K, l, on);
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) d[j] = dlogits[s * (int64_t)C + min(c0 + j, C - 1)];
#pragma unroll
            for (int j = 0; j < kMfQuad; ++j) {
                if (c0 + j < C) {
                    const float dl = d[j];
                    gu.x = gu.x + dl * q[j].x;
                    gu.y = gu.y + dl * q[j].y;
                    gu.z = gu.z + dl * q[j].z;
                    gu.w = gu.w + dl * q[j].w;
                    sdl = sdl + dl;
                    float4 gi = make_float4(dl * p.x, dl * p.y, dl * p.z, dl * p.w);
                    if (reg) {
                        gi.x = gi.x + l2 * q[j].x;
                        gi.y = gi.y + l2 * q[j].y;
                        gi.z = gi.z + l2 * q[j].z;
                        gi.w = gi.w + l2 * q[j].w;
                    }
                    if (on) *reinterpret_cast<float4*>(g + (int64_t)(1 + c0 + j) * K) = gi;
                    if (gb && l == (j & (L - 1))) gb[1 + c0 + j] = (reg && bi) ? dl + l2 * bi[it[j]] : dl;
                }
            }
        }
        if (reg) {
            gu.x = gu.x + l2 * p.x;
            gu.y = gu.y + l2 * p.y;
            gu.z = gu.z + l2 * p.z;
            gu.w = gu.w + l2 * p.w;
        }
        if (on) *reinterpret_cast<float4*>(g) = gu;
        if (gb && l == 0) gb[0] = (reg && bu) ? sdl + l2 * bu[u] : sdl;
    }
}

__global__ __launch_bounds__(256) void neg_sample_k(const int64_t* __restrict__ users, int64_t B, const int64_t* __restrict__ offsets,
                                                     const int64_t* __restrict__ items, int64_t num_items, int n_neg,
                                                     const int64_t* __restrict__ state, uint32_t stream_id, int64_t first,
                                                     int64_t* __restrict__ out, int32_t* __restrict__ status) {
    const uint64_t seed = (uint64_t)state[0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), draw = (uint32_t)(uint64_t)state[1];
    const int64_t total = B * (int64_t)n_neg;
    const int64_t nthr = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += nthr) {
        const int64_t b = i / n_neg;
        const int64_t u = users[b];
        const int64_t base = offsets[u], n_u = offsets[u + 1] - base;
        const int64_t m = num_items - n_u;          // the items left to draw from
        if (m <= 0) {
            out[i] = -1;
            status[0] = 1;
            continue;
        }
        const uint64_t e = (uint64_t)first + (uint64_t)i;
        const Philox4 r = philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), stream_id, draw, k0, k1);
        const uint64_t w = (uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32);
        const int64_t k = (int64_t)__umul64hi(w, (uint64_t)m);
        // the smallest p in [0, n_u] with items[p] - p > k (items[p] - p = the non-members below items[p]: non-decreasing in p)
        int64_t lo = 0, hi = n_u;
        const int64_t* __restrict__ mine = items + base;
        for (int step = 0; step < 64; ++step) {
            if (lo >= hi) break;
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (mine[mid] - mid > k) hi = mid;
            else lo = mid + 1;
        }
        out[i] = k + lo;
    }
}

static int mf_lanes(int K) {
    int L = 1;
    while (L < K / 4) L <<= 1;
    return L;
}

// f(integral_constant<int, L>) for L = mf_lanes(K)
template <class Fn>
static void mf_dispatch(int L, Fn&& f) {
    switch (L) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 32: f(std::integral_constant<int, 32>{}); break;
        default: f(std::integral_constant<int, 64>{}); break;
    }
}

static int mf_check(const char* name, const void* P, const void* Q, const void* bu, const void* bi, const void* ids, int64_t B, int C, int K) {
    DIR_CHECK_ARG(B >= 0 && C >= 1, "%s: B=%lld C=%d", name, (long long)B, C);
    DIR_CHECK_ARG(K >= 4 && K <= 256 && K % 4 == 0, "%s: K=%d (a multiple of 4 in [4, 256])", name, K);
    DIR_CHECK_ARG((bu == nullptr) == (bi == nullptr), "%s: bu and bi go together", name);
    DIR_CHECK_ARG(P && Q && ids, "%s: null pointer", name);
    DIR_CHECK_ARG(aligned16(P) && aligned16(Q), "%s: P / Q must be 16-byte aligned", name);
    DIR_CHECK_ARG((int64_t)(1 + C) * K < 0x7fffffffll, "%s: (1 + C) * K must fit int32", name);
    return DIR_OK;
}

}  // namespace dir

using namespace dir;

extern "C" int dir_mf_score_f32(const float* P, const float* Q, const float* bu, const float* bi, const float* b0, const int64_t* ids, int64_t sb,
                                int64_t sf, int64_t B, int C, int K, float* logits, dir_stream_t stream) {
    const char* name = "dir_mf_score_f32";
    if (int rc = mf_check(name, P, Q, bu, bi, ids, B, C, K)) return rc;
    if (B == 0) return DIR_OK;
    DIR_CHECK_ARG(logits != nullptr, "%s: null pointer (logits)", name);
    const int L = mf_lanes(K);
    const int grid = grid_for((B + 256 / L - 1) / (256 / L));
    mf_dispatch(L, [&](auto l) {
        hipLaunchKernelGGL((mf_score_k<decltype(l)::value>), dim3((unsigned)grid), dim3(256), 0, as_stream(stream), P, Q, bu, bi, b0, ids, sb, sf, B, C, K,
                           logits);
    });
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_mf_score_backward_f32(const float* P, const float* Q, const float* bu, const float* bi, const int64_t* ids, int64_t sb, int64_t sf,
                                         const float* dlogits, float l2, int64_t B, int C, int K, float* grad, float* gbias, dir_stream_t stream) {
    const char* name = "dir_mf_score_backward_f32";
    if (int rc = mf_check(name, P, Q, bu, bi, ids, B, C, K)) return rc;
    DIR_CHECK_ARG(l2 >= 0.0f, "%s: l2=%g", name, (double)l2);
    if (B == 0) return DIR_OK;
    DIR_CHECK_ARG(dlogits && grad, "%s: null pointer (dlogits / grad)", name);
    DIR_CHECK_ARG(aligned16(grad), "%s: grad must be 16-byte aligned", name);
    const int L = mf_lanes(K);
    const int grid = grid_for((B + 256 / L - 1) / (256 / L));
    mf_dispatch(L, [&](auto l) {
        hipLaunchKernelGGL((mf_score_bwd_k<decltype(l)::value>), dim3((unsigned)grid), dim3(256), 0, as_stream(stream), P, Q, bu, bi, ids, sb, sf,
                           dlogits, l2, B, C, K, grad, gbias);
    });
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_neg_sample_i64(const int64_t* users, int64_t B, const int64_t* offsets, const int64_t* items, int64_t num_items, int n_neg,
                                  const int64_t* state, uint32_t stream_id, int64_t first, int64_t* out, int32_t* status, dir_stream_t stream) {
    const char* name = "dir_neg_sample_i64";
    DIR_CHECK_ARG(B >= 0 && n_neg >= 1, "%s: B=%lld n_neg=%d", name, (long long)B, n_neg);
    DIR_CHECK_ARG(num_items >= 1, "%s: num_items=%lld", name, (long long)num_items);
    DIR_CHECK_ARG(first >= 0 && B <= (INT64_MAX - first) / n_neg, "%s: first=%lld: first + B * n_neg overflows", name, (long long)first);
    DIR_CHECK_ARG(offsets && state, "%s: null pointer (offsets / state)", name);
    if (B == 0) return DIR_OK;
    DIR_CHECK_ARG(users && items && out && status, "%s: null pointer", name);      // (items: any valid address when no user has an item)
    const int grid = grid_for((B * (int64_t)n_neg + 255) / 256);
    hipLaunchKernelGGL(neg_sample_k, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), users, B, offsets, items, num_items, n_neg, state, stream_id,
                       first, out, status);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}
