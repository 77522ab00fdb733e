// rows_scatter.hip -- sparse rows summed into a dense slab, deterministically (gfx950).
//
//   out[r, :] = sum of vals[i, :K] over the entries i with idx[i] == r        (rows nobody names: zeros)
//
// The requester-side transpose of a sharded lookup (ShardedTables.lookup_train / lookup_rows_train): every entry of a micro-batch holds the
// gradient of one received row, `idx` is the entry's position in the slab of received rows (the lookup's `inv`), and a DE-DUPLICATED lookup
// names one position from many entries.  The (idx, i) pairs are sorted with the in-tree stable radix sort (radix_sort.hip), so the entries
// of a row are summed in ascending entry order, and the sums go through the sorted optimiser steps' run_sum (run_sum.hpp): compensated
// inside a 256-entry sort tile, a long run's tile partials added in double and rounded once (scat_fix_k, as adagrad_fix_k).  No float
// atomics: two calls over the same input are the same bits, and a run of ONE entry is that entry's row bit for bit.
// Kernel launches only -- the zero fill of `out` rides on the key pass -- so a call can sit inside a HIP-graph capture.
// Plain loads, adds and stores: no matrix instructions in this translation unit.
//
// dir_rows_scatter_sum_side_f32: the same call with a SIDE sum on the same sort -- out_side[r, :U] = sum of side[i / side_div, :U] over the
// same entries (the first-order term of a de-duplicated training lookup: entry i of a [Bc * F] entry list belongs to sample i / F, so d lin
// [Bc, U] is read in place).  One key pass (which also zero-fills out_side), one sort, one run discovery; the side sums go through the same
// run_sum (BV<1> per unit) with the same tile cuts and the same carry-then-fix combine in double, so out_side is bit for bit what the plain
// entry gives at K = U on the expanded side rows.  The kernels are templated on SIDE; without it every side statement is compiled out.
#include "common.hpp"
#include "run_sum.hpp"

namespace dir {

constexpr int SCAT_TILE = 256;

// the side sum's arguments (SIDE kernels only): side [.., ld] read at row entry / div, out [R, U], carry [tiles][2][U] behind the rows' carry
struct ScatSide { const float* side; int64_t ld; uint32_t div; int U; float* out; float* carry; };

// keys[i] = idx[i] (entries that name no row of the slab -- idx < 0 or idx >= R -- get R and sort behind every row), vals[i] = i; and
// the zero fill of out [n_out floats]: 16-byte stores over the aligned body (n_out4 float4s), scalar stores over what is left
// (SIDE: and of out_side [n_side floats], scalar stores)
template <bool SIDE>
__global__ __launch_bounds__(256) void scat_keys_k(const int64_t* __restrict__ idx, int64_t n, uint32_t R, uint32_t* __restrict__ keys,
                                                   uint32_t* __restrict__ vals, float* __restrict__ out, int64_t n_out4, int64_t n_out,
                                                   float* __restrict__ out_side, int64_t n_side) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t e = i0; e < n; e += step) {
        const int64_t id = idx[e];
        keys[e] = (uint64_t)id < (uint64_t)R ? (uint32_t)id : R;
        vals[e] = (uint32_t)e;
    }
    float4* o4 = reinterpret_cast<float4*>(out);
    for (int64_t i = i0; i < n_out4; i += step) o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = n_out4 * 4 + i0; i < n_out; i += step) out[i] = 0.f;
    if constexpr (SIDE)
        for (int64_t i = i0; i < n_side; i += step) out_side[i] = 0.f;
}

// One workgroup per tile of 256 sorted entries: the runs of equal keys inside the tile are found as in adagrad_tile_k, a group of LPS
// lanes sums a run through run_sum and writes the row -- or, for a run that crosses a tile border, leaves the tile's partial in `carry`
// ([tiles][2][K]: slot 0 = the run that came in from the left, slot 1 = the run that goes out to the right; a run open on both sides
// goes to slot 0).
// SIDE: the run's side sums are formed by the lanes that sum its row -- lane c takes the units c, c + kv, ... (kv = the lanes a row
// occupies), so a group without an idle lane (K = 16 in float4s: 4 lanes; K = 4: one lane, which then takes every unit) and a padded
// group (K = 6: 6 of 8 lanes) are served alike -- through the same run_sum over the same entries, into out_side or the side carry.
template <int LPS, int VEC, bool SIDE>
__global__ __launch_bounds__(256) void scat_tile_k(int K, int64_t n, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                   const float* __restrict__ rows, int64_t ld, uint32_t R, float* __restrict__ out,
                                                   float* __restrict__ carry, ScatSide sd) {
    using V = BV<VEC>;
    using T = typename V::T;
    constexpr int NG = 256 / LPS;
    __shared__ uint32_t skey[SCAT_TILE], sval[SCAT_TILE];
    __shared__ int rstart[SCAT_TILE + 1];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t = blockIdx.x, e0 = t * SCAT_TILE;
    const int ne = (int)((n - e0) < SCAT_TILE ? (n - e0) : SCAT_TILE);
    const bool in = tid < ne;
    const uint32_t key = in ? keys[e0 + tid] : 0xffffffffu;
    skey[tid] = key;
    sval[tid] = in ? vals[e0 + tid] : 0u;
    const bool start = in && (tid == 0 || key != keys[e0 + tid - 1]);
    const unsigned long long m = __ballot(start);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int woff = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) woff += (w < wave) ? wcnt[w] : 0;
    const int nruns = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (start) rstart[woff + __popcll(m & ((1ull << lane) - 1ull))] = tid;
    if (tid == 0) rstart[nruns] = ne;
    __syncthreads();
    const bool cont_l = t > 0 && keys[e0 - 1] == skey[0];
    const bool cont_r = e0 + ne < n && keys[e0 + ne] == skey[ne - 1];
    const int g = tid / LPS, c = tid - g * LPS, kv = K / VEC;
    if (c >= kv) return;                                   // idle lanes of a padded group (no barrier follows)
    for (int r = g; r < nruns; r += NG) {
        const int s = rstart[r], e = rstart[r + 1];
        const uint32_t rk = skey[s];
        if (rk >= R) continue;                             // entries that name no row
        const T sum = run_sum<VEC>(s, e, [&](int i) { return V::ld(rows + (int64_t)sval[i] * ld + c * VEC); });
        const bool open_l = r == 0 && cont_l, open_r = r == nruns - 1 && cont_r;
        if (!open_l && !open_r) V::st(out + (int64_t)rk * K + c * VEC, sum);
        else V::st(carry + (t * 2 + (open_l ? 0 : 1)) * K + c * VEC, sum);
        if constexpr (SIDE) {
            for (int u = c; u < sd.U; u += kv) {
                const float ss = run_sum<1>(s, e, [&](int i) { return sd.side[(int64_t)(sval[i] / sd.div) * sd.ld + u]; });
                if (!open_l && !open_r) sd.out[(int64_t)rk * sd.U + u] = ss;
                else sd.carry[(t * 2 + (open_l ? 0 : 1)) * sd.U + u] = ss;
            }
        }
    }
}

// One thread group per tile: if a run STARTS in this tile and continues to the right, its tiles' partials -- each good to an ulp
// (run_sum) -- are added in tile order in double and the total is rounded once (adagrad_fix_k's arithmetic), then the row is written.
// SIDE: the same combine over the side carry, by the lanes and units of scat_tile_k.
template <int LPS, int VEC, bool SIDE>
__global__ __launch_bounds__(256) void scat_fix_k(int K, int64_t n, int64_t ntiles, const uint32_t* __restrict__ keys, uint32_t R,
                                                  const float* __restrict__ carry, float* __restrict__ out, ScatSide sd) {
    using V = BV<VEC>;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = q / LPS;
    const int c = (int)(q - t * LPS), kv = K / VEC;
    if (t >= ntiles || c >= kv) return;
    const int64_t e0 = t * SCAT_TILE;
    const int64_t e1 = (e0 + SCAT_TILE < n) ? e0 + SCAT_TILE : n;    // first entry of the next tile
    if (e1 >= n) return;
    const uint32_t kl = keys[e1 - 1];
    if (kl >= R || keys[e1] != kl) return;                            // not open to the right
    if (t > 0 && keys[e0] == kl && keys[e0 - 1] == kl) return;        // the run started in an earlier tile
    typename V::D wide = V::widen(V::ld(carry + (t * 2 + 1) * K + c * VEC));
    for (int64_t u = t + 1; u < ntiles; ++u) {
        wide = V::addw(wide, V::ld(carry + (u * 2) * K + c * VEC));
        const int64_t u1 = (u + 1) * SCAT_TILE;
        if (!(u1 < n && keys[u1] == kl)) break;                       // the run ends inside tile u
    }
    V::st(out + (int64_t)kl * K + c * VEC, V::narrow(wide));
    if constexpr (SIDE) {
        for (int u = c; u < sd.U; u += kv) {
            double ws = (double)sd.carry[(t * 2 + 1) * sd.U + u];
            for (int64_t v = t + 1; v < ntiles; ++v) {
                ws += (double)sd.carry[(v * 2) * sd.U + u];
                const int64_t v1 = (v + 1) * SCAT_TILE;
                if (!(v1 < n && keys[v1] == kl)) break;
            }
            sd.out[(int64_t)kl * sd.U + u] = (float)ws;
        }
    }
}

struct ScatPlan { size_t n, ntiles, off_keys[2], off_vals[2], off_carry, off_tmp, total; unsigned bits; };
// U: the side sum's units (0: none) -- the carry holds K + U floats per slot, the rows' [tiles][2][K] first, the side's [tiles][2][U] behind
static void scat_plan(int64_t n, int K, int U, int64_t R, ScatPlan& p) {
    p.n = (size_t)n;
    p.ntiles = (p.n + SCAT_TILE - 1) / SCAT_TILE;
    unsigned bits = 1;
    while (bits < 32 && (((uint64_t)1 << bits) <= (uint64_t)R)) ++bits;     // keys go up to R (entries that name no row)
    p.bits = bits;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    p.off_keys[0] = take(p.n * 4); p.off_keys[1] = take(p.n * 4);
    p.off_vals[0] = take(p.n * 4); p.off_vals[1] = take(p.n * 4);
    p.off_carry = take(p.ntiles * 2 * (size_t)(K + U) * 4);
    const size_t tmp = radix_sort_temp_bytes(p.n, bits);
    p.off_tmp = take(tmp ? tmp : 256);
    p.total = off;
}

static bool scat_shape_ok(int64_t n, int K, int64_t R) {
    return n >= 0 && n < ((int64_t)1 << 30) && K > 0 && R >= 0 && R < 0xffffffffll;
}

}  // namespace dir

using namespace dir;

// Both entries: the checks (all of them before any HIP call), the key pass, the sort, the tile and fix kernels.  sd == nullptr: no side sum.
static int scat_sum(const char* name, const int64_t* idx, const float* vals, int64_t ld, int64_t n, int K, int64_t R, float* out,
                    const ScatSide* side, int64_t side_div, void* workspace, int64_t workspace_bytes, dir_stream_t stream) {
    DIR_CHECK_ARG(scat_shape_ok(n, K, R), "%s: n=%lld (0 <= n < 2^30) K=%d R=%lld (0 <= R < 2^32-1)", name, (long long)n, K, (long long)R);
    DIR_CHECK_ARG(ld >= K, "%s: ld=%lld < K=%d", name, (long long)ld, K);
    const int U = side ? side->U : 0;
    if (side) {
        DIR_CHECK_ARG(U >= 1 && U <= 4, "%s: U=%d (1 <= U <= 4)", name, U);
        DIR_CHECK_ARG(side_div >= 1, "%s: side_div=%lld < 1", name, (long long)side_div);
        DIR_CHECK_ARG(side->ld >= U, "%s: side_ld=%lld < U=%d", name, (long long)side->ld, U);
    }
    if (R == 0) return DIR_OK;                             // no row to write, and no entry can name one
    DIR_CHECK_ARG(out && (n == 0 || (idx && vals)), "%s: null pointer", name);
    if (side) {
        DIR_CHECK_ARG(side->out, "%s: null pointer (out_side)", name);
        DIR_CHECK_ARG(n == 0 || side->side, "%s: null pointer (side)", name);
    }
    const bool vec = (K % 4 == 0) && (ld % 4 == 0) && aligned16(vals) && aligned16(out);
    int lps = 1;
    while (lps < (vec ? K / 4 : K)) lps <<= 1;
    if (lps > 64) return fail(DIR_E_UNSUPPORTED, "%s: K=%d is wider than one wave covers (max %d)", name, K, vec ? 256 : 64);
    ScatPlan p;
    scat_plan(n, K, U, R, p);
    DIR_CHECK_ARG(n == 0 || (workspace && (int64_t)p.total <= workspace_bytes && !(reinterpret_cast<uintptr_t>(workspace) & 255u)),
                  "%s: workspace needs %lld bytes, 256-byte aligned", name, (long long)p.total);
    hipStream_t st = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    uint32_t* k0 = n ? reinterpret_cast<uint32_t*>(ws + p.off_keys[0]) : nullptr;
    uint32_t* k1 = n ? reinterpret_cast<uint32_t*>(ws + p.off_keys[1]) : nullptr;
    uint32_t* v0 = n ? reinterpret_cast<uint32_t*>(ws + p.off_vals[0]) : nullptr;
    uint32_t* v1 = n ? reinterpret_cast<uint32_t*>(ws + p.off_vals[1]) : nullptr;
    const bool second = n && radix_sort_input_buffer((size_t)n, p.bits) == 1;
    const int64_t n_out = R * (int64_t)K;
    const int64_t n_out4 = aligned16(out) ? n_out / 4 : 0;
    const int64_t fill = n_out4 ? n_out4 : n_out;          // (grid-stride loops: the grid only has to be large enough to be quick)
    const int64_t work = n > fill ? n : fill;
    if (side)
        hipLaunchKernelGGL(scat_keys_k<true>, dim3(grid_for((work + 255) / 256)), dim3(256), 0, st, idx, n, (uint32_t)R, second ? k1 : k0,
                           second ? v1 : v0, out, n_out4, n_out, side->out, R * (int64_t)U);
    else
        hipLaunchKernelGGL(scat_keys_k<false>, dim3(grid_for((work + 255) / 256)), dim3(256), 0, st, idx, n, (uint32_t)R, second ? k1 : k0,
                           second ? v1 : v0, out, n_out4, n_out, (float*)nullptr, (int64_t)0);
    DIR_CHECK_LAUNCH(name);
    if (n == 0) return DIR_OK;
    if (radix_sort_pairs_u32(ws + p.off_tmp, k0, k1, v0, v1, (size_t)n, p.bits, st) != hipSuccess) return fail(DIR_E_HIP, "%s: radix sort failed", name);
    float* carry = reinterpret_cast<float*>(ws + p.off_carry);
    const int64_t ntiles = (int64_t)p.ntiles;
    ScatSide sd = side ? *side : ScatSide{nullptr, 0, 1u, 0, nullptr, nullptr};
    if (side) {
        sd.div = side_div > 0xffffffffll ? 0xffffffffu : (uint32_t)side_div;     // (entry numbers are below 2^30: the quotient is 0 either way)
        sd.carry = carry + ntiles * 2 * (int64_t)K;
    }
    dispatch_lps(vec, lps, [&](auto L, auto V) {
        constexpr int LPS = decltype(L)::value, VEC = decltype(V)::value;
        const dim3 gt((unsigned)ntiles), gf((unsigned)((ntiles * LPS + 255) / 256));
        if (side) {
            hipLaunchKernelGGL((scat_tile_k<LPS, VEC, true>), gt, dim3(256), 0, st, K, n, k1, v1, vals, ld, (uint32_t)R, out, carry, sd);
            hipLaunchKernelGGL((scat_fix_k<LPS, VEC, true>), gf, dim3(256), 0, st, K, n, ntiles, k1, (uint32_t)R, carry, out, sd);
        } else {
            hipLaunchKernelGGL((scat_tile_k<LPS, VEC, false>), gt, dim3(256), 0, st, K, n, k1, v1, vals, ld, (uint32_t)R, out, carry, sd);
            hipLaunchKernelGGL((scat_fix_k<LPS, VEC, false>), gf, dim3(256), 0, st, K, n, ntiles, k1, (uint32_t)R, carry, out, sd);
        }
    });
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int64_t dir_rows_scatter_sum_workspace_bytes(int64_t n, int K, int64_t R) {
    if (!scat_shape_ok(n, K, R)) return -1;
    ScatPlan p;
    scat_plan(n, K, 0, R, p);
    return (int64_t)p.total;
}

extern "C" int dir_rows_scatter_sum_f32(const int64_t* idx, const float* vals, int64_t ld, int64_t n, int K, int64_t R, float* out,
                                        void* workspace, int64_t workspace_bytes, dir_stream_t stream) {
    return scat_sum("dir_rows_scatter_sum_f32", idx, vals, ld, n, K, R, out, nullptr, 1, workspace, workspace_bytes, stream);
}

extern "C" int64_t dir_rows_scatter_sum_side_workspace_bytes(int64_t n, int K, int U, int64_t R) {
    if (!scat_shape_ok(n, K, R) || U < 1 || U > 4) return -1;
    ScatPlan p;
    scat_plan(n, K, U, R, p);
    return (int64_t)p.total;
}

extern "C" int dir_rows_scatter_sum_side_f32(const int64_t* idx, const float* vals, int64_t ld, const float* side, int64_t side_ld,
                                             int64_t side_div, int64_t n, int K, int U, int64_t R, float* out, float* out_side,
                                             void* workspace, int64_t workspace_bytes, dir_stream_t stream) {
    const ScatSide sd{side, side_ld, 1u, U, out_side, nullptr};
    return scat_sum("dir_rows_scatter_sum_side_f32", idx, vals, ld, n, K, R, out, &sd, side_div, workspace, workspace_bytes, stream);
}
