// shard_linear.hip -- the first-order (linear) term of DeepFM over ROW-SHARDED weights, gfx950.
//
// Replaces (reference): linear_logits under the embedding tables' input_layer_partitioner, models/DeepFM/deepFM.py:199-223, 255-275.
//
// The first-order weights of slot f live beside the embedding rows of slot f, on the rank that owns them, as packed training rows: U
// 16-byte blocks [w | n | z | -], one per unit, side by side (unit u's weight at float 4 u; U = 1: TableSet.ftrl_rows' layout, DeepFM and
// xDeepFM; U = 2: ESMM_W_D's two linear models over the same ids, ShardedTables.attach_linear([rows, U])).  The linear term rides on the
// embedding lookup's id exchange: the owner already holds the (slot, local row) payload of every entry it serves, and the U weights of
// an entry travel behind ONE payload word, so
//   linear_gather_k   owner:      out[i * U + u] = unit u's weight of payload word i -> U floats per slab slot travel back
//   linear_finish_k   requester:  lin[b, u] = bias[u] + sum_f wback[inv[b, f] * U + u], per unit in linear_onehot4_k's order and arithmetic
//                                 (bit for bit)
//   linear_grad_k     requester:  the transpose of the finish: send[inv[b, f] * U + u] = d logit[b, u]
// The owner's update is dir_sparse_ftrl_rows_units_sorted_payload_f32 (backward.hip).  U = 1 is a value of U like any other: the plain
// C entries below are the units entries at units = 1.
//
// All three are request-rate-bound (4-byte reads or writes, no reuse): one lane per entry (the grad: per entry and unit), the payload
// read coalesced, several independent loads in flight per lane, nothing staged through LDS.
#include "common.hpp"
#include "shard_wire.hpp"

namespace dir {

constexpr int DIR_MAX_UNITS = 8;

// Owner side.  Slab form (cap > 0): recv = P one-hot slabs (shard_wire.hpp), out[(s * cap + j) * U + u].  Flat form (cap == 0): recv = n
// payload words, out[i * U + u].  p < 0, a slot behind the header, or a row outside the slot's local rows (local_rows, optional) writes
// 0.0f: every output word is written, nothing uninitialised goes back over the wire.  ONE lane takes a row and issues its U reads
// together (they fall into the row's one 16 U-byte piece: for U = 2 one 32-byte segment holds both).
template <int U, int EPT>
__global__ __launch_bounds__(256) void linear_gather_k(const float* const* __restrict__ rows, int64_t ld, const int64_t* __restrict__ local_rows,
                                                       int F, const int64_t* __restrict__ recv, int64_t cap, int64_t total,
                                                       float* __restrict__ out) {
    const int64_t per_grid = (int64_t)gridDim.x * 256 * EPT;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 * EPT; i0 < total; i0 += per_grid) {
        int64_t p[EPT];
        const float* src[EPT];
        float v[EPT][U];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {                        // the payload words: consecutive lanes read consecutive words
            const int64_t i = i0 + e * 256 + threadIdx.x;
            p[e] = -1;
            if (i < total) {
                if (cap > 0) {
                    const int64_t sl = (int64_t)((uint32_t)i / (uint32_t)cap);       // total < 2^31
                    const int64_t j = i - sl * cap;
                    const int64_t* slab = slab_of(recv, sl, cap);
                    if (j < slab_count(slab[0])) p[e] = slab[1 + j];
                } else {
                    p[e] = recv[i];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            src[e] = nullptr;
            if (p[e] >= 0) {
                int slot;
                int64_t row;
                unpack_payload(p[e], F, slot, row);
                if (!local_rows || row < local_rows[slot]) src[e] = rows[slot] + row * ld;
            }
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e)
#pragma unroll
            for (int u = 0; u < U; ++u) v[e][u] = src[e] ? src[e][4 * u] : 0.f;     // EPT * U independent 4-byte reads in flight per lane
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t i = i0 + e * 256 + threadIdx.x;
            if (i < total) {
#pragma unroll
                for (int u = 0; u < U; ++u) out[i * U + u] = v[e][u];
            }
        }
    }
}

// Requester side: FOUR lanes per sample and unit (blockIdx.y = the unit), lane c reads the weights of fields 4 j + c through the inverse
// positions, and the quad adds them up in FIELD order through quad broadcasts -- linear_onehot4_k's sum (linear_cross.hip), add for add:
// acc = 0; acc += v_f for f = 0..F-1 (a pruned entry adds 0.0f); r = acc + (bias ? bias[unit] : 0.0f).
// ONE: U == 1 known at compile time (the flagship DeepFM term): no multiply in the address of a weight.
template <int UFL, bool ONE>
__global__ __launch_bounds__(256) void linear_finish_k(const float* __restrict__ wback, int64_t n_back, int units, const int64_t* __restrict__ inv,
                                                       int64_t sb, int64_t sf, int F, const float* __restrict__ bias, int64_t B,
                                                       float* __restrict__ out, int64_t out_ld) {
    const int c = threadIdx.x & 3;
    const int U = ONE ? 1 : units;
    const int unit = ONE ? 0 : (int)blockIdx.y;
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
            for (int j = 0; j < UFL; ++j) v[j] = (uint64_t)pos[j] < (uint64_t)n_back ? wback[pos[j] * U + unit] : 0.f;     // inv < 0: pruned
#pragma unroll
            for (int j = 0; j < UFL; ++j) acc = quad_add_in_order(v[j], f0 + 4 * j, F, acc);
        }
        if (live && c == 0) out[b * out_ld + unit] = acc + (bias ? bias[unit] : 0.f);
    }
}

// Requester side of the backward, one lane per (entry, unit): entry (b, f) writes d logit[b, u] where its weights came back from --
// consecutive lanes write the U consecutive floats of a position.  Training lookups are never de-duplicated: every position has exactly
// one writer (plain stores); `send` was zero-filled by the C entry.  ONE: as in linear_finish_k.
template <bool ONE>
__global__ __launch_bounds__(256) void linear_grad_k(const float* __restrict__ g, int64_t g_ld, int units, const int64_t* __restrict__ inv,
                                                     int64_t sb, int64_t sf, int F, int64_t n /* B * F * U */, float* __restrict__ send,
                                                     int64_t n_send) {
    const int U = ONE ? 1 : units;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t e = ONE ? (uint32_t)i : (uint32_t)i / (uint32_t)U;                    // n < 2^31
        const int u = ONE ? 0 : (int)((uint32_t)i - e * (uint32_t)U);
        const int64_t b = (int64_t)(e / (uint32_t)F);
        const int f = (int)(e - (uint32_t)b * (uint32_t)F);
        const int64_t pos = inv[b * sb + (int64_t)f * sf];
        if ((uint64_t)pos < (uint64_t)n_send) send[pos * U + u] = g[b * g_ld + u];
    }
}

// ------------------------------------------------------------------------------------------------
// the term over multi-hot bags (ShardedTables.lookup_bags(want_lin=True) / lookup_bags_train(with_linear=True))
// ------------------------------------------------------------------------------------------------
// The bag lookup's owner holds every entry's 16-byte record (shard_wire.hpp), so it pools the first-order weights of each run beside the
// embedding rows: one float per partial-row position travels back behind the partial rows, the requester adds a bag's partials in
// ascending owner order, applies the model's ONE linear_sparse_combiner (independent of the per-slot embedding combiners: its
// denominators are computed from the CSR entries with the lookup's liveness rule) and sums the sample's F bags in slot order --
// linear_csr_k's operations in its order (linear_cross.hip), so with one owner per bag and flags = 0 the result is
// dir_linear_sparse_sum_f32's bit for bit.
//   bags_linear_pool_k     owner:      lout[src * cap_b + ret] = sum over the run of w_e * lw[row_e], in entry order, from 0.0f
//   bags_linear_denom_k    requester:  lden[g] of every bag (mean / sqrtn only), kept in the plan for the backward
//   bags_linear_combine_k  requester:  lin[b] = sum_f (sum_o partial) [/ lden] + bias
//   bags_linear_grad_k     requester:  the transpose of the combine: send[pos[g * P + o]] = d lin[b] [/ lden[g]]
// The owner's update is dir_sparse_ftrl_rows_sorted_bags_f32 (backward.hip).
constexpr int SBL_U = 8;      // entry slots per lane (bags_pool_k's chunk)

// Owner side.  ONE lane takes a chunk of SBL_U entry slots of the received slabs -- bags_pool_k's walk with a lane where that kernel has a
// lane group: the chunk's records (consecutive lanes read consecutive 128-byte pieces of the slab: every line a wave touches is used whole)
// and then its SBL_U weights are in flight together; the lane pools every run that STARTS inside its chunk, acc + w * lw in entry order,
// and writes each position once; a run that goes on past the chunk is walked to its end, SBL_U records at a time, and a leading run that
// began in the previous chunk is left to that chunk's lane.  bags_pool_k's record checks (read_bag_record, row < the slot's local
// rows): an entry that kernel drops is dropped here.  Positions no run names keep the zero the C entry filled lout with.
__global__ __launch_bounds__(256) void bags_linear_pool_k(const float* const* __restrict__ rows, int64_t ld, const int64_t* __restrict__ lvocab,
                                                          int F, const int4* __restrict__ recv, int P, int64_t cap_e, int64_t cap_b,
                                                          float* __restrict__ lout) {
    constexpr int U = SBL_U;
    const int64_t cpb = (cap_e + U - 1) / U;                          // chunks per slab
    const int64_t n = (int64_t)P * cpb;
    // record j of a slab -> return position, the address of its weight (nullptr: none / outside the local rows), entry weight
    auto load = [&](const int4* slab, int64_t j, int64_t ne, int& ret, const float*& src, float& w) {
        src = nullptr;
        int sl;
        int64_t rr;
        if (read_bag_record(slab, j, ne, F, cap_b, ret, w, sl, rr) && rr < lvocab[sl]) src = rows[sl] + rr * ld;
    };
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < n; it += (int64_t)gridDim.x * 256) {
        const int s = n < ((int64_t)1 << 31) ? (int)((uint32_t)it / (uint32_t)cpb) : (int)(it / cpb);
        const int64_t c0 = (it - (int64_t)s * cpb) * U;
        const int4* slab = bag_slab_of(recv, s, cap_e);
        const int64_t ne = bag_entries(slab, cap_e);
        if (c0 >= ne) continue;
        const int prev = c0 > 0 ? bag_record_ret(slab[c0]) : -3;
        int ret[U];
        const float* src[U];
        float w[U], v[U];
        bool cont = true;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load(slab, c0 + u, ne, ret[u], src[u], w[u]);
            cont = cont && ret[u] == prev;
            if (cont) {
                ret[u] = -2;
                src[u] = nullptr;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = src[u] ? *src[u] : 0.f;        // U independent 4-byte reads in flight
        float acc = 0.f;
        int cur = -2;
        auto store = [&](int r, float a) {
            if (r >= 0 && (int64_t)r < cap_b) lout[(int64_t)s * cap_b + r] = a;
        };
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ret[u] == -2) continue;
            if (ret[u] != cur) {
                store(cur, acc);
                acc = 0.f;
                cur = ret[u];
            }
            if (src[u]) acc = acc + w[u] * v[u];
        }
        if (cur >= 0 && (int64_t)cur < cap_b) {                            // the chunk's last run may go on past it
            for (int64_t j0 = c0 + U; j0 < ne && bag_record_ret(slab[1 + j0]) == cur; j0 += U) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    load(slab, j0 + u, ne, ret[u], src[u], w[u]);
                    if (ret[u] != cur) src[u] = nullptr;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = src[u] ? *src[u] : 0.f;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (src[u]) acc = acc + w[u] * v[u];
                if (ret[U - 1] != cur) break;
            }
        }
        store(cur, acc);
    }
}

// Requester side: the linear combiner's denominator of every bag g = b * F + f, from the CSR entries: bags_bucket_k's liveness rule and
// sums (bag_entry_live, BagDenom), which are linear_csr_k's arithmetic.  A bag without a live entry gets a value nobody divides by.
__global__ __launch_bounds__(256) void bags_linear_denom_k(const int64_t* __restrict__ ids, const int64_t* __restrict__ offsets,
                                                           const float* __restrict__ weights, int64_t sb, int64_t sf, int64_t nb, int F,
                                                           const int64_t* __restrict__ vocab, int flags, int combiner,
                                                           float* __restrict__ lden) {
    const bool prune_w = weights && (flags & DIR_BAG_PRUNE_NONPOSITIVE_WEIGHTS);
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nb; g += (int64_t)gridDim.x * 256) {
        const int64_t b = (int64_t)((uint32_t)g / (uint32_t)F);          // nb < 2^31
        const int f = (int)(g - b * F);
        const int64_t bag = b * sb + (int64_t)f * sf;
        const int64_t beg = offsets[bag], end = offsets[bag + 1];
        const int64_t V = vocab[f];
        BagDenom den;
        for (int64_t e = beg; e < end; ++e) {
            const float w = weights ? weights[e] : 1.0f;
            if (bag_entry_live(ids[e], w, V, prune_w)) den.add(w);
        }
        lden[g] = den.value(combiner, weights != nullptr);
    }
}

// Requester side: linear_finish_k's quads -- lane c of a sample's four computes the bags of slots 4 j + c (v = 0; v += the partial of every
// owner in mask[g], ascending; v /= lden[g] when the bag had a live entry and the combiner is mean or sqrtn), and the quad adds them up in
// SLOT order through quad broadcasts: acc = 0; acc += v_f for f = 0..F-1; r = acc + (bias ? bias[0] : 0.0f).  lden == nullptr: sum.
template <int UFL>
__global__ __launch_bounds__(256) void bags_linear_combine_k(const float* __restrict__ lback, int64_t n_back, int P,
                                                             const int32_t* __restrict__ pos, const uint64_t* __restrict__ mask,
                                                             const float* __restrict__ lden, int F, const float* __restrict__ bias, int64_t B,
                                                             float* __restrict__ out, int64_t out_ld) {
    const int c = threadIdx.x & 3;
    const int64_t per_grid = ((int64_t)gridDim.x * blockDim.x) >> 2;
    for (int64_t b0 = ((int64_t)blockIdx.x * blockDim.x) >> 2; b0 < B; b0 += per_grid) {      // (block-uniform trip count: the DPP reads see live lanes)
        const int64_t b = b0 + (threadIdx.x >> 2);
        const bool live = b < B;
        float acc = 0.f;
        for (int f0 = 0; f0 < F; f0 += 4 * UFL) {
            uint64_t m[UFL];
            float v[UFL];
#pragma unroll
            for (int j = 0; j < UFL; ++j) {
                const int f = f0 + 4 * j + c;
                m[j] = (live && f < F) ? mask[b * F + f] : 0ull;
            }
#pragma unroll
            for (int j = 0; j < UFL; ++j) {
                v[j] = 0.f;
                if (m[j]) {
                    const int64_t g = b * F + f0 + 4 * j + c;
                    for_each_owner(m[j], [&](int o) {
                        const int32_t p = pos[g * P + o];
                        if (p >= 0 && (int64_t)p < n_back) v[j] = v[j] + lback[p];
                    });
                    if (lden) v[j] = v[j] / lden[g];
                }
            }
#pragma unroll
            for (int j = 0; j < UFL; ++j) acc = quad_add_in_order(v[j], f0 + 4 * j, F, acc);
        }
        if (live && c == 0) out[b * out_ld] = acc + (bias ? bias[0] : 0.f);
    }
}

// Requester side of the backward, one lane per bag: every owner o in mask[g] gets c_g * d lin[b] (c_g = 1 / lden[g] for mean and sqrtn:
// lden != nullptr) at position pos[g * P + o] of `send` -- where the forward received that partial.  bags_grad_k's rule: positions no
// partial came back from are not written (the owners never read them).
__global__ __launch_bounds__(256) void bags_linear_grad_k(const float* __restrict__ g, int64_t g_ld, int P, const int32_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ mask, const float* __restrict__ lden, int64_t nb, int F,
                                                          float* __restrict__ send, int64_t n_send) {
    for (int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x; gi < nb; gi += (int64_t)gridDim.x * 256) {
        const uint64_t m = mask[gi];
        if (!m) continue;
        const int64_t b = (int64_t)((uint32_t)gi / (uint32_t)F);         // nb < 2^31
        float d = g[b * g_ld];
        if (lden) d = d / lden[gi];
        for_each_owner(m, [&](int o) {
            const int32_t p = pos[gi * P + o];
            if (p >= 0 && (int64_t)p < n_send) send[p] = d;
        });
    }
}

}  // namespace dir

using namespace dir;

// ---- one body per step: the plain entry is the units entry at units = 1 (the gather's plain entry brings its own row stride) --------------
static int check_units(const char* name, int units) {
    DIR_CHECK_ARG(units >= 1 && units <= DIR_MAX_UNITS, "%s: units=%d (1 <= units <= %d)", name, units, DIR_MAX_UNITS);
    return DIR_OK;
}

static int linear_gather(const char* name, const float* const* rows, int units, int64_t row_ld, const int64_t* local_rows, int F,
                         const int64_t* recv, int P, int64_t cap, int64_t n, float* out, dir_stream_t stream) {
    DIR_CHECK_ARG(F > 0, "%s: F=%d", name, F);
    if (int rc = check_units(name, units)) return rc;
    DIR_CHECK_ARG(row_ld >= 1, "%s: row_ld=%lld", name, (long long)row_ld);
    int64_t total;
    if (cap > 0) {                                             // the P fixed-capacity slabs
        if (int rc = check_owners(name, P)) return rc;
        DIR_CHECK_ARG((int64_t)P * cap * units < ((int64_t)1 << 31), "%s: cap=%lld (P*cap*units < 2^31)", name, (long long)cap);
        total = (int64_t)P * cap;
    } else {                                                   // a flat payload of n words
        DIR_CHECK_ARG(cap == 0, "%s: cap=%lld (> 0: slabs, 0: a flat payload of n words)", name, (long long)cap);
        DIR_CHECK_ARG(n >= 0 && n * units < ((int64_t)1 << 31), "%s: n=%lld (0 <= n, n*units < 2^31)", name, (long long)n);
        total = n;
    }
    if (total == 0) return DIR_OK;
    DIR_CHECK_ARG(rows && recv && out, "%s: null pointer", name);
    const int ept = units == 1 ? 4 : 2;                        // entries per lane: ept * units reads in flight
    dim3 grid(grid_for((total + 256 * ept - 1) / (256 * ept)));
    hipStream_t st = as_stream(stream);
#define DIR_LG(UN, EPT) \
    case UN: hipLaunchKernelGGL((linear_gather_k<UN, EPT>), grid, dim3(256), 0, st, rows, row_ld, local_rows, F, recv, cap, total, out); break;
    switch (units) { DIR_LG(1, 4) DIR_LG(2, 2) DIR_LG(3, 2) DIR_LG(4, 2) DIR_LG(5, 2) DIR_LG(6, 2) DIR_LG(7, 2) DIR_LG(8, 2) }
#undef DIR_LG
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

static int linear_finish(const char* name, const float* wback, int64_t n_back, int units, const int64_t* inv, int64_t stride_b, int64_t stride_f,
                         int F, const float* bias, int64_t B, float* out, int64_t out_ld, dir_stream_t stream) {
    DIR_CHECK_ARG(F > 0 && B >= 0, "%s: F=%d B=%lld", name, F, (long long)B);
    if (int rc = check_units(name, units)) return rc;
    DIR_CHECK_ARG(n_back >= 0 && n_back * units < ((int64_t)1 << 31), "%s: n_back=%lld (0 <= n_back, n_back*units < 2^31)", name, (long long)n_back);
    DIR_CHECK_ARG(out_ld >= units, "%s: out_ld=%lld (>= units)", name, (long long)out_ld);
    if (B == 0) return DIR_OK;
    DIR_CHECK_ARG(inv && out && (wback || n_back == 0), "%s: null pointer", name);
    const dim3 grid(grid_for((B + 63) / 64), (unsigned)units);
    hipStream_t st = as_stream(stream);
    if (units == 1)
        hipLaunchKernelGGL((linear_finish_k<7, true>), grid, dim3(256), 0, st, wback, n_back, units, inv, stride_b, stride_f, F, bias, B, out, out_ld);
    else
        hipLaunchKernelGGL((linear_finish_k<7, false>), grid, dim3(256), 0, st, wback, n_back, units, inv, stride_b, stride_f, F, bias, B, out, out_ld);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

static int linear_grad(const char* name, const float* g, int64_t g_ld, int units, const int64_t* inv, int64_t stride_b, int64_t stride_f, int F,
                       int64_t B, float* send, int64_t n_send, dir_stream_t stream) {
    DIR_CHECK_ARG(F > 0 && B >= 0, "%s: F=%d B=%lld", name, F, (long long)B);
    if (int rc = check_units(name, units)) return rc;
    DIR_CHECK_ARG(B * F * units < ((int64_t)1 << 31), "%s: B=%lld (B*F*units < 2^31)", name, (long long)B);
    DIR_CHECK_ARG(n_send >= 0 && n_send * units < ((int64_t)1 << 31), "%s: n_send=%lld (0 <= n_send, n_send*units < 2^31)", name, (long long)n_send);
    DIR_CHECK_ARG(g_ld >= units, "%s: g_ld=%lld (>= units)", name, (long long)g_ld);
    DIR_CHECK_ARG(send || n_send == 0, "%s: null pointer", name);
    DIR_CHECK_ARG(B == 0 || (g && inv), "%s: null pointer", name);
    hipStream_t st = as_stream(stream);
    // a kernel's zero-fill (a memset node would end a graph capture: DESIGN 7.1)
    if (n_send > 0 && zero_async(send, (size_t)n_send * (size_t)units * sizeof(float), st) != hipSuccess)
        return fail(DIR_E_HIP, "%s: zero-fill of send failed", name);
    if (B == 0 || n_send == 0) return DIR_OK;
    const int64_t n = B * F * units;
    const dim3 grid(grid_for((n + 255) / 256));
    if (units == 1)
        hipLaunchKernelGGL(linear_grad_k<true>, grid, dim3(256), 0, st, g, g_ld, units, inv, stride_b, stride_f, F, n, send, n_send);
    else
        hipLaunchKernelGGL(linear_grad_k<false>, grid, dim3(256), 0, st, g, g_ld, units, inv, stride_b, stride_f, F, n, send, n_send);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_shard_linear_gather_f32(const float* const* rows, int64_t row_ld, const int64_t* local_rows, int F, const int64_t* recv,
                                           int P, int64_t cap, int64_t n, float* out, dir_stream_t stream) {
    return linear_gather("dir_shard_linear_gather_f32", rows, 1, row_ld, local_rows, F, recv, P, cap, n, out, stream);
}

extern "C" int dir_shard_linear_gather_units_f32(const float* const* rows, int units, const int64_t* local_rows, int F, const int64_t* recv,
                                                 int P, int64_t cap, int64_t n, float* out, dir_stream_t stream) {
    return linear_gather("dir_shard_linear_gather_units_f32", rows, units, (int64_t)4 * units, local_rows, F, recv, P, cap, n, out, stream);
}

extern "C" int dir_shard_linear_finish_f32(const float* wback, int64_t n_back, const int64_t* inv, int64_t stride_b, int64_t stride_f, int F,
                                           const float* bias, int64_t B, float* out, int64_t out_ld, dir_stream_t stream) {
    return linear_finish("dir_shard_linear_finish_f32", wback, n_back, 1, inv, stride_b, stride_f, F, bias, B, out, out_ld, stream);
}

extern "C" int dir_shard_linear_finish_units_f32(const float* wback, int64_t n_back, int units, const int64_t* inv, int64_t stride_b,
                                                 int64_t stride_f, int F, const float* bias, int64_t B, float* out, int64_t out_ld,
                                                 dir_stream_t stream) {
    return linear_finish("dir_shard_linear_finish_units_f32", wback, n_back, units, inv, stride_b, stride_f, F, bias, B, out, out_ld, stream);
}

extern "C" int dir_shard_linear_grad_f32(const float* g, int64_t g_ld, const int64_t* inv, int64_t stride_b, int64_t stride_f, int F, int64_t B,
                                         float* send, int64_t n_send, dir_stream_t stream) {
    return linear_grad("dir_shard_linear_grad_f32", g, g_ld, 1, inv, stride_b, stride_f, F, B, send, n_send, stream);
}

extern "C" int dir_shard_linear_grad_units_f32(const float* g, int64_t g_ld, int units, const int64_t* inv, int64_t stride_b, int64_t stride_f,
                                               int F, int64_t B, float* send, int64_t n_send, dir_stream_t stream) {
    return linear_grad("dir_shard_linear_grad_units_f32", g, g_ld, units, inv, stride_b, stride_f, F, B, send, n_send, stream);
}

// ---- the term over multi-hot bags ---------------------------------------------------------------------------------------------------
extern "C" int dir_shard_bags_linear_pool_f32(const float* const* rows, int64_t row_ld, const int64_t* local_rows, int F, const int64_t* recv,
                                              int P, int64_t cap_e, int64_t cap_b, float* lout, dir_stream_t stream) {
    const char* name = "dir_shard_bags_linear_pool_f32";
    DIR_CHECK_ARG(F > 0 && row_ld >= 1, "%s: F=%d row_ld=%lld", name, F, (long long)row_ld);
    if (int rc = check_slab_geometry(name, P, cap_e, cap_b)) return rc;
    DIR_CHECK_ARG(rows && local_rows && recv && lout, "%s: null pointer", name);
    hipStream_t st = as_stream(stream);
    // every word crosses the wire: a kernel's zero-fill (a memset node would end the world-1 lookup's graph capture: DESIGN 7.1)
    if (zero_async(lout, (size_t)P * (size_t)cap_b * sizeof(float), st) != hipSuccess) return fail(DIR_E_HIP, "%s: zero-fill of lout failed", name);
    const int64_t n = (int64_t)P * ((cap_e + SBL_U - 1) / SBL_U);      // one lane per chunk of SBL_U entry slots
    hipLaunchKernelGGL(bags_linear_pool_k, dim3(grid_for((n + 255) / 256)), dim3(256), 0, st, rows, row_ld, local_rows, F,
                       reinterpret_cast<const int4*>(recv), P, cap_e, cap_b, lout);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_shard_bags_linear_combine_f32(const float* lback, int P, int64_t cap_b, const int32_t* pos, const int64_t* mask,
                                                 const int64_t* ids, const int64_t* offsets, const float* weights, int64_t nnz,
                                                 int64_t stride_b, int64_t stride_f, const int64_t* vocab, int flags, int64_t B, int F,
                                                 int combiner, float* lden, const float* bias, float* out, int64_t out_ld,
                                                 dir_stream_t stream) {
    const char* name = "dir_shard_bags_linear_combine_f32";
    DIR_CHECK_ARG(F > 0 && B >= 0 && B * F < ((int64_t)1 << 31), "%s: F=%d B=%lld (B*F < 2^31)", name, F, (long long)B);
    if (int rc = check_partial_geometry(name, P, cap_b)) return rc;
    DIR_CHECK_ARG(combiner >= DIR_COMBINER_SUM && combiner <= DIR_COMBINER_SQRTN, "%s: combiner=%d", name, combiner);
    DIR_CHECK_ARG(nnz >= 0 && out_ld >= 1, "%s: nnz=%lld out_ld=%lld", name, (long long)nnz, (long long)out_ld);
    if (B == 0) return DIR_OK;                                 // an empty batch carries no buffers
    DIR_CHECK_ARG(lback && pos && mask && out, "%s: null pointer", name);
    const bool div = combiner != DIR_COMBINER_SUM;
    DIR_CHECK_ARG(!div || (lden && offsets && vocab && (ids || nnz == 0)), "%s: null pointer (mean / sqrtn: ids, offsets, vocab, lden)", name);
    hipStream_t st = as_stream(stream);
    if (div) {
        const int64_t nb = B * F;
        hipLaunchKernelGGL(bags_linear_denom_k, dim3(grid_for((nb + 255) / 256)), dim3(256), 0, st, ids, offsets, weights, stride_b, stride_f,
                           nb, F, vocab, flags, combiner, lden);
    }
    hipLaunchKernelGGL((bags_linear_combine_k<4>), dim3(grid_for((B + 63) / 64)), dim3(256), 0, st, lback, (int64_t)P * cap_b, P, pos,
                       reinterpret_cast<const uint64_t*>(mask), div ? lden : nullptr, F, bias, B, out, out_ld);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}

extern "C" int dir_shard_bags_linear_grad_f32(const float* g, int64_t g_ld, int P, int64_t cap_b, const int32_t* pos, const int64_t* mask,
                                              const float* lden, int64_t B, int F, int combiner, float* send, dir_stream_t stream) {
    const char* name = "dir_shard_bags_linear_grad_f32";
    DIR_CHECK_ARG(F > 0 && B >= 0 && B * F < ((int64_t)1 << 31), "%s: F=%d B=%lld (B*F < 2^31)", name, F, (long long)B);
    if (int rc = check_partial_geometry(name, P, cap_b)) return rc;
    DIR_CHECK_ARG(combiner >= DIR_COMBINER_SUM && combiner <= DIR_COMBINER_SQRTN, "%s: combiner=%d", name, combiner);
    DIR_CHECK_ARG(g_ld >= 1, "%s: g_ld=%lld", name, (long long)g_ld);
    DIR_CHECK_ARG(send, "%s: null pointer", name);
    const bool div = combiner != DIR_COMBINER_SUM;
    DIR_CHECK_ARG(B == 0 || (g && pos && mask && (lden || !div)), "%s: null pointer", name);
    if (B == 0) return DIR_OK;
    const int64_t nb = B * F;
    hipLaunchKernelGGL(bags_linear_grad_k, dim3(grid_for((nb + 255) / 256)), dim3(256), 0, as_stream(stream), g, g_ld, P, pos,
                       reinterpret_cast<const uint64_t*>(mask), div ? lden : nullptr, nb, F, send, (int64_t)P * cap_b);
    DIR_CHECK_LAUNCH(name);
    return DIR_OK;
}
