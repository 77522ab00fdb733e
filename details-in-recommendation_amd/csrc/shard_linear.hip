// shard_linear.hip -- the first-order (linear) term of DeepFM over ROW-SHARDED weights, gfx950.
//
// Replaces (reference): linear_logits under the embedding tables' input_layer_partitioner, models/DeepFM/deepFM.py:199-223, 255-275.
//
// The first-order weights of slot f live beside the embedding rows of slot f, on the rank that owns them, as packed 16-byte training rows
// [w | n | z | -] (TableSet.ftrl_rows' layout).  The linear term rides on the embedding lookup's id exchange: the owner already holds the
// (slot, local row) payload of every entry it serves, so
//   linear_gather_k   owner:      one w per received payload word -> one float per slab slot (4 bytes per entry travel back)
//   linear_finish_k   requester:  lin[b] = bias + sum_f wback[inv[b, f]], in linear_onehot4_k's order and arithmetic (bit for bit)
//   linear_grad_k     requester:  the transpose of the finish: send[inv[b, f]] = d logit[b]
// The owner's update is dir_sparse_ftrl_rows_sorted_payload_f32 (backward.hip).
//
// All three are request-rate-bound (one 4-byte read or write per entry, no reuse): one lane per entry, the payload read coalesced, several
// independent loads in flight per lane, nothing staged through LDS.
#include "common.hpp"

namespace dir {

__device__ __forceinline__ int64_t lin_slab_count(int64_t header) { return (int64_t)(uint32_t)header; }

// Owner side.  Slab form (cap > 0): recv = P slabs of [header | cap slots] (header: low 32 bits = valid slots), out[s * cap + j].  Flat form
// (cap == 0): recv = n payload words, out[i].  p = local_row * F + slot; p < 0, a slot behind the header, or a row outside the slot's
// local rows (local_rows, optional) writes 0.0f: every output word is written, nothing uninitialised goes back over the wire.
template <int EPT>
__global__ __launch_bounds__(256) void linear_gather_k(const float* const* __restrict__ rows, int64_t ld, const int64_t* __restrict__ local_rows,
                                                       int F, const int64_t* __restrict__ recv, int64_t cap, int64_t total,
                                                       float* __restrict__ out) {
    const int64_t per_grid = (int64_t)gridDim.x * 256 * EPT;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 * EPT; i0 < total; i0 += per_grid) {
        int64_t p[EPT];
        const float* src[EPT];
        float v[EPT];
#pragma unroll
        for (int u = 0; u < EPT; ++u) {                        // the payload words: consecutive lanes read consecutive words
            const int64_t i = i0 + u * 256 + threadIdx.x;
            p[u] = -1;
            if (i < total) {
                if (cap > 0) {
                    const int64_t sl = (int64_t)((uint32_t)i / (uint32_t)cap);       // total < 2^31
                    const int64_t j = i - sl * cap;
                    const int64_t* slab = recv + sl * (cap + 1);
                    if (j < lin_slab_count(slab[0])) p[u] = slab[1 + j];
                } else {
                    p[u] = recv[i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < EPT; ++u) {                        // decode as gather_slabs_k does (32-bit division when it fits)
            src[u] = nullptr;
            if (p[u] >= 0) {
                int slot;
                int64_t row;
                if (p[u] < (int64_t)0x7fffffff) {
                    const uint32_t r32 = (uint32_t)p[u] / (uint32_t)F;
                    slot = (int)((uint32_t)p[u] - r32 * (uint32_t)F);
                    row = r32;
                } else {
                    row = p[u] / F;
                    slot = (int)(p[u] - row * F);
                }
                if (!local_rows || row < local_rows[slot]) src[u] = rows[slot] + row * ld;
            }
        }
#pragma unroll
        for (int u = 0; u < EPT; ++u) v[u] = src[u] ? *src[u] : 0.f;      // EPT independent 4-byte reads in flight per lane
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            const int64_t i = i0 + u * 256 + threadIdx.x;
            if (i < total) out[i] = v[u];
        }
    }
}

// Requester side: FOUR lanes per sample, lane c reads the weights of fields 4 j + c through the inverse positions, and the quad adds them
// up in FIELD order through quad broadcasts -- linear_onehot4_k's sum (linear_cross.hip), add for add: acc = 0; acc += v_f for f = 0..F-1
// (a pruned entry adds 0.0f); r = acc + (bias ? bias[0] : 0.0f).
template <int UFL>
__global__ __launch_bounds__(256) void linear_finish_k(const float* __restrict__ wback, int64_t n_back, const int64_t* __restrict__ inv,
                                                       int64_t sb, int64_t sf, int F, const float* __restrict__ bias, int64_t B,
                                                       float* __restrict__ out, int64_t out_ld) {
    const int c = threadIdx.x & 3;
    const int64_t per_grid = ((int64_t)gridDim.x * blockDim.x) >> 2;
    for (int64_t b0 = ((int64_t)blockIdx.x * blockDim.x) >> 2; b0 < B; b0 += per_grid) {      // (block-uniform trip count: the DPP reads see live lanes)
        const int64_t b = b0 + (threadIdx.x >> 2);
        const bool live = b < B;
        const int64_t* ip = inv + (live ? b : 0) * sb;
        float acc = 0.f;
        for (int f0 = 0; f0 < F; f0 += 4 * UFL) {
            int64_t pos[UFL];
            float v[UFL];
#pragma unroll
            for (int j = 0; j < UFL; ++j) {
                const int f = f0 + 4 * j + c;
                pos[j] = (live && f < F) ? ip[(int64_t)f * sf] : (int64_t)-1;
            }
#pragma unroll
            for (int j = 0; j < UFL; ++j) v[j] = (uint64_t)pos[j] < (uint64_t)n_back ? wback[pos[j]] : 0.f;     // inv < 0: pruned
#pragma unroll
            for (int j = 0; j < UFL; ++j) {
                const int vi = __builtin_bit_cast(int, v[j]);
                const float q0 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(vi, 0x00, 0xf, 0xf, true));   // quad_perm [0,0,0,0]
                const float q1 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(vi, 0x55, 0xf, 0xf, true));   // [1,1,1,1]
                const float q2 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(vi, 0xaa, 0xf, 0xf, true));   // [2,2,2,2]
                const float q3 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(vi, 0xff, 0xf, 0xf, true));   // [3,3,3,3]
                const int f = f0 + 4 * j;
                if (f < F) acc = acc + q0;
                if (f + 1 < F) acc = acc + q1;
                if (f + 2 < F) acc = acc + q2;
                if (f + 3 < F) acc = acc + q3;
            }
        }
        if (live && c == 0) out[b * out_ld] = acc + (bias ? bias[0] : 0.f);
    }
}

// Requester side of the backward: entry (b, f) writes d logit[b] where its weight came back from.  Training lookups are never de-duplicated:
// every position has exactly one writer (plain stores); `send` was zero-filled by the caller of the kernel (the C entry).
__global__ __launch_bounds__(256) void linear_grad_k(const float* __restrict__ g, int64_t g_ld, const int64_t* __restrict__ inv, int64_t sb,
                                                     int64_t sf, int F, int64_t n /* B * F */, float* __restrict__ send, int64_t n_send) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = (int64_t)((uint32_t)i / (uint32_t)F);          // n < 2^31
        const int f = (int)(i - b * F);
        const int64_t pos = inv[b * sb + (int64_t)f * sf];
        if ((uint64_t)pos < (uint64_t)n_send) send[pos] = g[b * g_ld];
    }
}

}  // namespace dir

using namespace dir;

extern "C" int dir_shard_linear_gather_f32(const float* const* rows, int64_t row_ld, const int64_t* local_rows, int F, const int64_t* recv,
                                           int P, int64_t cap, int64_t n, float* out, dir_stream_t stream) {
    const char* name = "dir_shard_linear_gather_f32";
    DIR_CHECK_ARG(F > 0 && row_ld >= 1, "%s: F=%d row_ld=%lld", name, F, (long long)row_ld);
    int64_t total;
    if (cap > 0) {                                             // the P fixed-capacity slabs
        DIR_CHECK_ARG(P > 0 && P <= 64, "%s: P=%d (1 <= P <= 64)", name, P);
        DIR_CHECK_ARG((int64_t)P * cap < ((int64_t)1 << 31), "%s: cap=%lld (P*cap < 2^31)", name, (long long)cap);
        total = (int64_t)P * cap;
    } else {                                                   // a flat payload of n words
        DIR_CHECK_ARG(cap == 0, "%s: cap=%lld (> 0: slabs, 0: a flat payload of n words)", name, (long long)cap);
        DIR_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "%s: n=%lld (0 <= n < 2^31)", name, (long long)n);
        total = n;
    }
    if (total == 0) return DIR_OK;
    DIR_CHECK_ARG(rows && recv && out, "%s: null pointer", name);
    constexpr int EPT = 4;
    dim3 grid(grid_for((total + 256 * EPT - 1) / (256 * EPT)));
    hipLaunchKernelGGL((linear_gather_k<EPT>), grid, dim3(256), 0, as_stream(stream), rows, row_ld, local_rows, F, recv, cap, total, out);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_shard_linear_finish_f32(const float* wback, int64_t n_back, const int64_t* inv, int64_t stride_b, int64_t stride_f, int F,
                                           const float* bias, int64_t B, float* out, int64_t out_ld, dir_stream_t stream) {
    const char* name = "dir_shard_linear_finish_f32";
    DIR_CHECK_ARG(F > 0 && B >= 0, "%s: F=%d B=%lld", name, F, (long long)B);
    DIR_CHECK_ARG(n_back >= 0 && n_back < ((int64_t)1 << 31), "%s: n_back=%lld (0 <= n_back < 2^31)", name, (long long)n_back);
    DIR_CHECK_ARG(out_ld >= 1, "%s: out_ld=%lld", name, (long long)out_ld);
    if (B == 0) return DIR_OK;
    DIR_CHECK_ARG(inv && out && (wback || n_back == 0), "%s: null pointer", name);
    hipLaunchKernelGGL((linear_finish_k<7>), dim3(grid_for((B + 63) / 64)), dim3(256), 0, as_stream(stream), wback, n_back, inv, stride_b,
                       stride_f, F, bias, B, out, out_ld);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_shard_linear_grad_f32(const float* g, int64_t g_ld, const int64_t* inv, int64_t stride_b, int64_t stride_f, int F, int64_t B,
                                         float* send, int64_t n_send, dir_stream_t stream) {
    const char* name = "dir_shard_linear_grad_f32";
    DIR_CHECK_ARG(F > 0 && B >= 0 && B * F < ((int64_t)1 << 31), "%s: F=%d B=%lld (B*F < 2^31)", name, F, (long long)B);
    DIR_CHECK_ARG(n_send >= 0 && n_send < ((int64_t)1 << 31), "%s: n_send=%lld (0 <= n_send < 2^31)", name, (long long)n_send);
    DIR_CHECK_ARG(g_ld >= 1, "%s: g_ld=%lld", name, (long long)g_ld);
    DIR_CHECK_ARG(send || n_send == 0, "%s: null pointer", name);
    DIR_CHECK_ARG(B == 0 || (g && inv), "%s: null pointer", name);
    hipStream_t st = as_stream(stream);
    if (n_send > 0 && hipMemsetAsync(send, 0, (size_t)n_send * sizeof(float), st) != hipSuccess)
        return fail(DIR_E_HIP, "%s: zero-fill of send failed", name);
    if (B == 0 || n_send == 0) return DIR_OK;
    const int64_t n = B * F;
    hipLaunchKernelGGL(linear_grad_k, dim3(grid_for((n + 255) / 256)), dim3(256), 0, st, g, g_ld, inv, stride_b, stride_f, F, n, send, n_send);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}
