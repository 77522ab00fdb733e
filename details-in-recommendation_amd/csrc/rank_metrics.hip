// rank_metrics.hip -- per-group pair statistics behind the grouped ranking metrics (GAUC, HR / NDCG / MRR@K, the per-user weighted loss).
//
// Reference: metrics/NCF_evaluation/ndcg_hr_mrr.py:14-44,58-84 (one positive among 99 sampled negatives, the top 10 of argsort(-pred)) and
// metrics/weighted_loss/weighted_loss.py:27-50,80-81 (per user: the weight of the (pos, neg) pairs with preds[i] <= preds[j] over the weight
// of all pairs), both O(n^2) Python loops there; GAUC is the DIN paper's user-weighted AUC (arXiv:1706.06978 section 6.2).  All of them are
// functions of the same counts.  A group g is the entries offsets[g] .. offsets[g + 1] - 1 of scores / labels / weights, in their given order;
// P = {e : labels[e] > 0.5}, N the rest (a NaN label is a negative), and for i in P
//     a_i = |{j in N : s_j > s_i}|,  e_i = |{j in N : s_j == s_i}|          (fp32 compares of the scores as they are)
// Per group: n_pos, n_neg, gt = sum_i (n_neg - a_i - e_i), eq = sum_i e_i, mis_w = sum_i w_i (a_i + e_i), tot_w = sum_i w_i n_neg (float64, the
// weights widened exactly, every term one IEEE product) and, where n_pos == 1, rank = 1 + |{j != i : s_j > s_i}| + |{j < i : s_j == s_i}| -- the
// positive's place in a STABLE descending sort, from 1 -- else 0.  A NaN score is above, below and equal to nothing, as the compares give.
//
// One launch, routed on the device from the group's own offsets (no host-declared maximum is trusted; n <= 0 is an empty group):
//   n <= kRankWaveMax: ONE WAVE per group, four groups per workgroup, no LDS and no barrier.  Lane l holds entries l, l + 64, ... in registers.
//     The wave walks the positives in entry order (the bits of a ballot); per positive, a readlane broadcasts its score and every lane
//     compares its own negatives: a_i and e_i are popcounts of two ballots per 64 entries.  The cost is n_pos * ceil(n / 64) ballot pairs --
//     the reference's block of 100 with one positive is four compares per lane.  The float64 sums run in entry order in every lane alike.
//   n >  kRankWaveMax: ONE WORKGROUP per group, after the wave phase of the same four groups.  The entries are walked in chunks of 4 x 256
//     (thread t holds entries c + t, c + 256 + t, ...: the positives strided over the threads; a chunk without a positive is skipped); for
//     each chunk the negatives' side goes through LDS in tiles of kRankTile scores (a positive's slot holds NaN, which no compare counts) that
//     every thread reads as broadcast 16-byte loads.  O(n^2 / 256) compares per thread for any n; one huge group is not split over workgroups.
//     Each thread adds its terms in entry order; the block sum is a fixed tree (xor butterfly in the wave, then (w0 + w1) + (w2 + w3)).
// Integer counters are exact; there is no floating-point atomic, so two runs give the same bits.  Compiled without packed fp32 VALU
// instructions (build.py: NO_PACKED_FP32): an evaluation stream may share a SIMD with another stream's bf16-MFMA kernel.
#include "common.hpp"

namespace dir {

constexpr int kRankWaveMax = 256;                 // largest group of the wave route
constexpr int kRankRounds = kRankWaveMax / 64;    // entries per lane there, and per thread and chunk in the workgroup route
constexpr int kRankTile = 512;                    // scores per LDS tile of the workgroup route (a multiple of 4)
constexpr int kRankGroupsPerBlock = 4;

struct RankStats {
    long long n_pos, n_neg, gt, eq, rank;
    double mis_w, tot_w;
};

struct RankOut {
    int64_t *n_pos, *n_neg, *gt, *eq;
    double *mis_w, *tot_w;
    int64_t* rank;
};

__device__ __forceinline__ void rank_store(const RankOut& o, int64_t g, const RankStats& r) {
    o.n_pos[g] = r.n_pos;
    o.n_neg[g] = r.n_neg;
    o.gt[g] = r.gt;
    o.eq[g] = r.eq;
    o.mis_w[g] = r.mis_w;
    o.tot_w[g] = r.tot_w;
    o.rank[g] = r.n_pos == 1 ? r.rank : 0;
}

// The wave route: 0 < n <= kRankWaveMax, all 64 lanes active; every lane returns the same statistics.
__device__ __forceinline__ RankStats rank_wave(const float* __restrict__ scores, const float* __restrict__ labels, const float* __restrict__ weights,
                                               int64_t base, int n, int lane) {
    float s[kRankRounds], w[kRankRounds];
    bool neg[kRankRounds];
    unsigned long long pm[kRankRounds];
    int n_pos = 0;
#pragma unroll
    for (int r = 0; r < kRankRounds; ++r) {
        const int j = lane + 64 * r;
        const bool valid = j < n;
        s[r] = valid ? scores[base + j] : 0.0f;
        const bool p = valid && labels[base + j] > 0.5f;
        neg[r] = valid && !p;
        w[r] = (p && weights) ? weights[base + j] : 1.0f;
        pm[r] = __ballot(p);
        n_pos += __popcll(pm[r]);
    }
    RankStats st = {n_pos, n - n_pos, 0, 0, 0, 0.0, 0.0};
    const int n_neg = n - n_pos;
    if (n_neg == 0 && n_pos != 1) return st;                      // no pair and no rank to report
#pragma unroll
    for (int ri = 0; ri < kRankRounds; ++ri) {
        unsigned long long m = pm[ri];                            // wave-uniform: the positives of this round, walked in entry order
        while (m) {
            const int li = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float si = lane_bcast(s[ri], li), wi = lane_bcast(w[ri], li);
            int a = 0, e = 0, eb = 0;
#pragma unroll
            for (int r = 0; r < kRankRounds; ++r) {
                if (64 * r < n) {
                    const unsigned long long gm = __ballot(neg[r] && s[r] > si), em = __ballot(neg[r] && s[r] == si);
                    a += __popcll(gm);
                    e += __popcll(em);
                    const unsigned long long before = r < ri ? ~0ull : (r == ri ? ((1ull << li) - 1ull) : 0ull);      // entries j < i
                    eb += __popcll(em & before);
                }
            }
            st.gt += n_neg - a - e;
            st.eq += e;
            st.mis_w = st.mis_w + (double)wi * (double)(a + e);
            st.tot_w = st.tot_w + (double)wi * (double)n_neg;
            st.rank = 1 + a + eb;                                 // kept only where n_pos == 1: then every other entry is a negative
        }
    }
    return st;
}

// Sum over the 256 threads in a fixed order: xor butterfly inside each wave, then (w0 + w1) + (w2 + w3).  red: 4 slots; called by all threads.
template <typename T>
__device__ __forceinline__ T rank_block_sum(T v, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    __syncthreads();                                              // the slots' previous readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One tile against the thread's four entries.  RANK: also count the equal negatives in front of the entry (only a group with one positive asks)
template <bool RANK>
__device__ __forceinline__ void rank_tile_pass(const float4* __restrict__ tile4, int m4, int64_t t0, const float (&s)[kRankRounds],
                                               const int64_t (&idx)[kRankRounds], unsigned (&a)[kRankRounds], unsigned (&e)[kRankRounds],
                                               unsigned (&eb)[kRankRounds]) {
    for (int k4 = 0; k4 < m4; ++k4) {
        const float4 q = tile4[k4];                               // the same address in every lane: a broadcast read
        const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < kRankRounds; ++r) {
                a[r] += v[c] > s[r] ? 1u : 0u;
                e[r] += v[c] == s[r] ? 1u : 0u;
                if (RANK) eb[r] += (v[c] == s[r] && t0 + 4 * k4 + c < idx[r]) ? 1u : 0u;
            }
        }
    }
}

// The workgroup route: n > kRankWaveMax, all 256 threads (block-uniform arguments).  Thread 0's result is stored.
__device__ __forceinline__ void rank_block(const float* __restrict__ scores, const float* __restrict__ labels, const float* __restrict__ weights,
                                           int64_t base, int64_t n, int64_t g, const RankOut& out, float4* tile4, long long* red_i, double* red_d) {
    const int tid = threadIdx.x;
    float* tile = reinterpret_cast<float*>(tile4);
    long long cnt = 0;
    for (int64_t j = tid; j < n; j += 256) cnt += labels[base + j] > 0.5f ? 1 : 0;
    const long long n_pos = rank_block_sum<long long>(cnt, red_i), n_neg = n - n_pos;
    long long t_gt = 0, t_eq = 0, t_rank = 0;
    double t_mis = 0.0, t_tot = 0.0;
    if (n_pos > 0 && n_neg > 0) {                                 // block-uniform
        const float nan = __builtin_nanf("");
        for (int64_t c0 = 0; c0 < n; c0 += 256 * kRankRounds) {
            float s[kRankRounds], w[kRankRounds];
            int64_t idx[kRankRounds];
            bool pos[kRankRounds], any = false;
#pragma unroll
            for (int r = 0; r < kRankRounds; ++r) {
                idx[r] = c0 + 256 * r + tid;
                const bool valid = idx[r] < n;
                s[r] = valid ? scores[base + idx[r]] : 0.0f;
                pos[r] = valid && labels[base + idx[r]] > 0.5f;
                w[r] = (pos[r] && weights) ? weights[base + idx[r]] : 1.0f;
                any = any || pos[r];
            }
            if (!__syncthreads_or(any ? 1 : 0)) continue;         // block-uniform: no positive in this chunk
            long long a64[kRankRounds] = {}, e64[kRankRounds] = {}, eb64[kRankRounds] = {};
            for (int64_t t0 = 0; t0 < n; t0 += kRankTile) {
                __syncthreads();                                  // the previous tile has been read
                for (int k = tid; k < kRankTile; k += 256) {
                    const int64_t j = t0 + k;
                    tile[k] = (j < n && !(labels[base + j] > 0.5f)) ? scores[base + j] : nan;      // positives and the padding count nowhere
                }
                __syncthreads();
                const int64_t left = n - t0;
                const int m4 = (int)((left < kRankTile ? left : kRankTile) + 3) >> 2;
                unsigned a[kRankRounds] = {}, e[kRankRounds] = {}, eb[kRankRounds] = {};
                if (n_pos == 1) rank_tile_pass<true>(tile4, m4, t0, s, idx, a, e, eb);
                else rank_tile_pass<false>(tile4, m4, t0, s, idx, a, e, eb);
#pragma unroll
                for (int r = 0; r < kRankRounds; ++r) {
                    a64[r] += a[r];
                    e64[r] += e[r];
                    eb64[r] += eb[r];
                }
            }
#pragma unroll
            for (int r = 0; r < kRankRounds; ++r) {               // the thread's terms in entry order
                if (pos[r]) {
                    t_gt += n_neg - a64[r] - e64[r];
                    t_eq += e64[r];
                    t_mis = t_mis + (double)w[r] * (double)(a64[r] + e64[r]);
                    t_tot = t_tot + (double)w[r] * (double)n_neg;
                    t_rank = 1 + a64[r] + eb64[r];
                }
            }
        }
    }
    RankStats st;
    st.n_pos = n_pos;
    st.n_neg = n_neg;
    st.gt = rank_block_sum<long long>(t_gt, red_i);
    st.eq = rank_block_sum<long long>(t_eq, red_i);
    st.rank = rank_block_sum<long long>(t_rank, red_i);           // at most one thread holds one where it is kept (n_pos == 1)
    st.mis_w = rank_block_sum<double>(t_mis, red_d);
    st.tot_w = rank_block_sum<double>(t_tot, red_d);
    if (tid == 0) rank_store(out, g, st);
}

__global__ __launch_bounds__(256) void group_rank_stats_k(const float* __restrict__ scores, const float* __restrict__ labels,
                                                           const float* __restrict__ weights, const int64_t* __restrict__ offsets, int64_t G,
                                                           RankOut out) {
    __shared__ float4 tile4[kRankTile / 4];
    __shared__ long long red_i[4];
    __shared__ double red_d[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t g0 = (int64_t)blockIdx.x * kRankGroupsPerBlock; g0 < G; g0 += (int64_t)gridDim.x * kRankGroupsPerBlock) {
        const int64_t gw = g0 + wave;                             // wave phase: no barrier inside
        if (gw < G) {
            const int64_t lo = offsets[gw], n = offsets[gw + 1] - lo;
            if (n <= 0) {
                const RankStats zero = {0, 0, 0, 0, 0, 0.0, 0.0};
                if (lane == 0) rank_store(out, gw, zero);
            } else if (n <= kRankWaveMax) {
                const RankStats st = rank_wave(scores, labels, weights, lo, (int)n, lane);
                if (lane == 0) rank_store(out, gw, st);
            }
        }
        for (int q = 0; q < kRankGroupsPerBlock; ++q) {           // workgroup phase: every thread reads the same offsets, so the branch is block-uniform
            const int64_t g = g0 + q;
            if (g >= G) break;
            const int64_t lo = offsets[g], n = offsets[g + 1] - lo;
            if (n > kRankWaveMax) rank_block(scores, labels, weights, lo, n, g, out, tile4, red_i, red_d);
        }
    }
}

}  // namespace dir

using namespace dir;

extern "C" int dir_group_rank_limits(int* wave_max, int* tile) {
    DIR_CHECK_ARG(wave_max && tile, "dir_group_rank_limits: null pointer");
    *wave_max = kRankWaveMax;
    *tile = kRankTile;
    return DIR_OK;
}

extern "C" int dir_group_rank_stats_f32(const float* scores, const float* labels, const float* weights, const int64_t* offsets, int64_t G,
                                        int64_t* n_pos, int64_t* n_neg, int64_t* gt, int64_t* eq, double* mis_w, double* tot_w, int64_t* rank,
                                        dir_stream_t stream) {
    const char* name = "dir_group_rank_stats_f32";
    DIR_CHECK_ARG(G >= 0, "%s: G=%lld", name, (long long)G);
    DIR_CHECK_ARG(offsets != nullptr, "%s: null pointer (offsets)", name);
    DIR_CHECK_ARG(G == 0 || (scores && labels && n_pos && n_neg && gt && eq && mis_w && tot_w && rank), "%s: null pointer", name);
    if (G == 0) return DIR_OK;
    const RankOut out = {n_pos, n_neg, gt, eq, mis_w, tot_w, rank};
    const int grid = grid_for((G + kRankGroupsPerBlock - 1) / kRankGroupsPerBlock, 16);
    hipLaunchKernelGGL(group_rank_stats_k, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), scores, labels, weights, offsets, G, out);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}
