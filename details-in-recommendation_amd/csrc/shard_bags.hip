// shard_bags.hip -- multi-hot embedding bags over ROW-SHARDED tables (ShardedTables.lookup_bags), pooled on the owning rank.
//
// Replaces (reference, /root/reference): the multi-hot columns of myself_input_layer (models/DeepFM/deepFM.py:53,77,84, a user's
// history as one bag) over tables row-partitioned with partition_strategy='div' (deepFM.py:163-167) -- [TF-upstream]
// embedding_lookup_sparse over a partitioned variable.
//
// One lookup, per rank:
//   bucket  (requester, bags_bucket_k)  every live CSR entry goes to the owner of its row; each (bag, owner) pair gets ONE return
//           position (a partial row) and a contiguous run of entry slots in that owner's slab, in entry order
//   exchange (equal-split all-to-all of the slabs)
//   pool    (owner, bags_pool_k)        per run: gather the rows, clip (max_norm), accumulate w * row in entry order -> partial row
//   exchange (equal-split all-to-all of the partial rows)
//   combine (requester, bags_combine_k) per bag: the partials in ascending owner order, then the slot's combiner; optional fused FM
// A bag of L entries over P owners sends L entries out and brings at most min(L, P) rows back.  With one owner (world size 1, or all of
// a bag's live entries on one rank) the arithmetic is bag_csr_k's operation for operation: the result is bit for bit the single-GPU
// embedding bag.
#include "common.hpp"
#include "bag_row.hpp"
#include "shard_route.hpp"
#include "shard_wire.hpp"

namespace dir {

// The slabs of 16-byte records that travel: shard_wire.hpp (BAG SLAB).
constexpr int SB_NT = 128;       // threads of the bucketing kernel's workgroup (one bag per thread per step)
constexpr int SB_MAXF = 256;     // slots whose 'div' constants are staged in LDS

__device__ __forceinline__ FieldDiv bag_fielddiv(const int64_t* __restrict__ vocab, const int32_t* __restrict__ parts,
                                                 const int32_t* __restrict__ first, int P, int f) {
    return make_fielddiv(vocab[f], parts ? parts[f] : P, first ? first[f] : 0);
}

// ------------------------------------------------------------------------------------------------
// requester: bucketing of CSR entries into fixed-capacity slabs
// ------------------------------------------------------------------------------------------------
// One thread walks one bag at a time (bag g = logical b * F + f; its entries at offsets[b * sb + f * sf]).  A workgroup takes
// SB_NT * bpt bags in two passes over them:
//   pass 1  counts the live entries and the distinct (bag, owner) pairs per owner (LDS atomics), then reserves both ranges of every
//           owner with ONE global 64-bit atomic per owner and workgroup (entries in the low, pairs in the high word) -- same-address
//           returning atomics retire at ~90 per us, so the count of reservations is what bounds such a kernel
//   pass 2  walks each bag again: per-owner entry counts in a lane-private LDS column, the combiner's denominator in entry order
//           (bag_csr_k's sums), then one run of entry slots and one partial row per owner present (LDS cursors inside the workgroup's
//           reservation), then a third walk scatters the entries into their runs in entry order.
// Where a run sits inside the slab depends on LDS atomic order; what is computed from it does not (each partial row is the sum of
// its own run, in entry order, and the requester finds it through pos[]).  The last workgroup to arrive writes the slab headers.
__global__ __launch_bounds__(SB_NT) void bags_bucket_k(const int64_t* __restrict__ ids, const int64_t* __restrict__ offsets,
                                                       const float* __restrict__ weights, int64_t sb, int64_t sf, int64_t B, int F,
                                                       const int64_t* __restrict__ vocab, const int32_t* __restrict__ parts,
                                                       const int32_t* __restrict__ first, int P, int flags,
                                                       const int32_t* __restrict__ slot_combiner, int combiner, int64_t cap_e,
                                                       int64_t cap_b, int bpt, int4* __restrict__ slabs, int32_t* __restrict__ pos,
                                                       uint64_t* __restrict__ mask, float* __restrict__ denom,
                                                       unsigned long long* __restrict__ gcount, int64_t* __restrict__ stat) {
    extern __shared__ int cnt[];          // [P][SB_NT]: this lane's entries of the current bag per owner; then its run cursor
    __shared__ unsigned int wg_e[64], wg_b[64];
    __shared__ FieldDiv fd[SB_MAXF];
    __shared__ int s_last;
    const int t = threadIdx.x;
    for (int i = t; i < P * SB_NT; i += SB_NT) cnt[i] = 0;
    if (t < 64) {
        wg_e[t] = 0;
        wg_b[t] = 0;
    }
    for (int f = t; f < F && f < SB_MAXF; f += SB_NT) fd[f] = bag_fielddiv(vocab, parts, first, P, f);
    __syncthreads();
    const int64_t nbags = B * F;
    const int64_t g0 = (int64_t)blockIdx.x * SB_NT * bpt;
    const bool prune_w = weights && (flags & DIR_BAG_PRUNE_NONPOSITIVE_WEIGHTS);
    // entry e of a bag of slot f: live (bag_csr_k's pruning: bag_entry_live) -> owner o, local row l
    auto route = [&](int64_t e, const FieldDiv& d, int& o, int64_t& l, float& w) -> bool {
        const int64_t id = ids[e];
        w = weights ? weights[e] : 1.0f;
        if (!bag_entry_live(id, w, d.V, prune_w)) return false;
        route_fd(id, d, &o, &l);
        o += d.first;
        if (o >= P) o -= P;
        return true;
    };
    auto bag_of = [&](int64_t g, int& f, int64_t& beg, int64_t& end) {
        const int64_t b = g / F;
        f = (int)(g - b * F);
        const int64_t bag = b * sb + (int64_t)f * sf;
        beg = offsets[bag];
        end = offsets[bag + 1];
    };
    // ---- pass 1: the workgroup's demand per owner ----
    for (int k = 0; k < bpt; ++k) {
        const int64_t g = g0 + (int64_t)k * SB_NT + t;
        if (g >= nbags) break;
        int f;
        int64_t beg, end;
        bag_of(g, f, beg, end);
        const FieldDiv d = f < SB_MAXF ? fd[f] : bag_fielddiv(vocab, parts, first, P, f);
        uint64_t m = 0;
        for (int64_t e = beg; e < end; ++e) {
            int o;
            int64_t l;
            float w;
            if (!route(e, d, o, l, w)) continue;
            atomicAdd(&wg_e[o], 1u);
            if (!((m >> o) & 1ull)) {
                m |= 1ull << o;
                atomicAdd(&wg_b[o], 1u);
            }
        }
    }
    __syncthreads();
    if (t < P) {           // the reservation: one returning atomic per owner and workgroup
        const unsigned long long add = ((unsigned long long)wg_b[t] << 32) | wg_e[t];
        const unsigned long long old = add ? atomicAdd(&gcount[t], add) : 0ull;
        wg_e[t] = (unsigned int)old;       // from here on: the workgroup's cursors
        wg_b[t] = (unsigned int)(old >> 32);
    }
    __syncthreads();
    // ---- pass 2: denominators, runs, scatter ----
    for (int k = 0; k < bpt; ++k) {
        const int64_t g = g0 + (int64_t)k * SB_NT + t;
        if (g >= nbags) break;
        int f;
        int64_t beg, end;
        bag_of(g, f, beg, end);
        const FieldDiv d = f < SB_MAXF ? fd[f] : bag_fielddiv(vocab, parts, first, P, f);
        uint64_t m = 0;
        BagDenom den;                      // bag_csr_k's sums, in entry order (w = 1 without weights)
        for (int64_t e = beg; e < end; ++e) {
            int o;
            int64_t l;
            float w;
            if (!route(e, d, o, l, w)) continue;
            cnt[o * SB_NT + t] += 1;
            m |= 1ull << o;
            den.add(w);
        }
        mask[g] = m;
        // (applied by the combine step only when the bag has a live entry and the combiner is not SUM)
        denom[g] = den.value(slot_combiner ? slot_combiner[f] : combiner, weights != nullptr);
        for_each_owner(m, [&](int o) {
            const unsigned int start = atomicAdd(&wg_e[o], (unsigned int)cnt[o * SB_NT + t]);
            const unsigned int q = atomicAdd(&wg_b[o], 1u);
            cnt[o * SB_NT + t] = (int)start;
            pos[g * P + o] = (int64_t)q < cap_b ? (int32_t)((int64_t)o * cap_b + q) : -1;
        });
        if (m) {
            for (int64_t e = beg; e < end; ++e) {
                int o;
                int64_t l;
                float w;
                if (!route(e, d, o, l, w)) continue;
                const int64_t p = (unsigned int)cnt[o * SB_NT + t];
                cnt[o * SB_NT + t] = (int)(p + 1);
                if (p < cap_e) {
                    const int32_t r = pos[g * P + o];
                    bag_slab_of(slabs, o, cap_e)[1 + p] = make_bag_record(pack_payload(l, F, f), w, r >= 0 ? (int)(r - (int64_t)o * cap_b) : -1);
                }
            }
            for_each_owner(m, [&](int o) { cnt[o * SB_NT + t] = 0; });
        }
    }
    // arrival: the last workgroup writes the headers (no fence: the counters are device-scope atomics whose results every workgroup
    // consumed before it arrives; slabs / pos / mask / denom are for LATER kernels -- see common.hpp)
    __syncthreads();
    if (t == 0) s_last = atomicAdd(reinterpret_cast<unsigned int*>(gcount + 64), 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (s_last && t < 64) {
        const unsigned long long c = t < P ? atomicExch(&gcount[t], 0ull) : 0ull;
        const unsigned int ce = (unsigned int)c, cb = (unsigned int)(c >> 32);
        unsigned int me = ce, mb = cb;
        bag_demand_stat(me, mb, cap_e, cap_b, stat);
        if (t < P) bag_slab_of(slabs, t, cap_e)[0] = make_bag_header(ce, cb, cap_e, cap_b, me, mb);
        if (t == 0) __hip_atomic_store(reinterpret_cast<unsigned int*>(gcount + 64), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------
// owner: gather + partial pool
// ------------------------------------------------------------------------------------------------
// LPS lanes take a chunk of U = 8 entry slots of the received slabs (bag_csr_k's lane mapping: lane c owns the 16-byte chunk c of every
// row): its U records and U rows are in flight together, and it pools every run that starts inside the chunk -- clip_row with the slot's
// max_norm, acc + w * row in entry order, the per-entry operations of bag_csr_k -- writing each partial row once; a run that goes on past
// the chunk is walked to its end, U records at a time, and a run that began in the previous chunk is left to that chunk's group.
// Received records are checked (read_bag_record, then row < the local table's rows) before they are used.
// Block 0 also reads the P received headers into stat (bag_demand_stat).
template <int LPS, int VEC, bool CLIP>
__global__ __launch_bounds__(256) void bags_pool_k(const float* const* __restrict__ tables, const int64_t* __restrict__ lvocab, int F,
                                                   int K, const int4* __restrict__ recv, int P, int64_t cap_e, int64_t cap_b,
                                                   const float* __restrict__ slot_max_norm, float max_norm, int flags,
                                                   float* __restrict__ out, int64_t* __restrict__ stat) {
    using V = typename VecT<VEC>::T;
    constexpr int SPW = 64 / LPS;
    constexpr int U = 8;
    const int lane = threadIdx.x & 63;
    const int c = lane & (LPS - 1);
    const int s = lane / LPS;
    const int kv = (K + VEC - 1) / VEC;
    const bool cact = c < kv;
    const bool nt = (flags & DIR_GATHER_STREAM_ROWS) != 0;
    __shared__ const float* s_tab[SB_MAXF];           // per-slot table base and row count: one LDS read per entry, not two global ones
    __shared__ int64_t s_rows[SB_MAXF];
    for (int f = threadIdx.x; f < F && f < SB_MAXF; f += blockDim.x) {
        s_tab[f] = tables[f];
        s_rows[f] = lvocab[f];
    }
    __syncthreads();
    if (stat && blockIdx.x == 0 && threadIdx.x < 64) {
        unsigned int me = 0, mb = 0;
        for (int o = threadIdx.x; o < P; o += 64) {
            const int4 h = bag_slab_of(recv, o, cap_e)[0];
            me = max(me, (unsigned int)h.z);
            mb = max(mb, (unsigned int)h.w);
        }
        bag_demand_stat(me, mb, cap_e, cap_b, stat);
    }
    const int64_t cpb = (cap_e + U - 1) / U;                          // chunks of U entry slots per slab
    const int64_t n = (int64_t)P * cpb;
    const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
    // record j of a slab -> return position, row (-1: none / outside the local table), slot, weight
    auto load = [&](const int4* slab, int64_t j, int64_t ne, int& ret, int64_t& row, int& sl, float& w) {
        row = -1;
        sl = 0;
        int64_t rr;
        if (read_bag_record(slab, j, ne, F, cap_b, ret, w, sl, rr) && rr < (sl < SB_MAXF ? s_rows[sl] : lvocab[sl])) row = rr;
    };
    // U rows in flight, then clip_row with the slot's max_norm and acc + w * row in entry order (bag_csr_k's per-entry operations)
    auto rows_of = [&](const int64_t (&row)[U], const int (&sl)[U], V (&v)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = vzero((V*)nullptr);
            if (row[u] >= 0 && cact) {
                const float* tp = (sl[u] < SB_MAXF ? s_tab[sl[u]] : tables[sl[u]]) + row[u] * K + c * VEC;
                v[u] = nt ? ldv_nt(tp, (V*)nullptr) : ldv(tp, (V*)nullptr);
            }
        }
        if (CLIP) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float mn = slot_max_norm ? slot_max_norm[sl[u]] : max_norm;      // (group-uniform: one record per group)
                if (row[u] >= 0 && mn > 0.f) v[u] = clip_row<LPS>(v[u], mn, lane, c);
            }
        }
    };
    auto store = [&](int src, int ret, const V& acc) {
        if (ret >= 0 && (int64_t)ret < cap_b && cact) stv(out + ((int64_t)src * cap_b + ret) * K + c * VEC, acc);
    };
    for (int64_t gw = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gw * SPW < n; gw += nwave) {
        const int64_t it = gw * SPW + s;
        if (it >= n) continue;
        const int src = n < ((int64_t)1 << 31) ? (int)((uint32_t)it / (uint32_t)cpb) : (int)(it / cpb);     // 32-bit division when it fits
        const int64_t c0 = (it - (int64_t)src * cpb) * U;
        const int4* slab = bag_slab_of(recv, src, cap_e);
        const int64_t ne = bag_entries(slab, cap_e);
        if (c0 >= ne) continue;
        // the chunk's U records; a leading run that began in the previous chunk belongs to that chunk's group
        const int prev = c0 > 0 ? bag_record_ret(slab[c0]) : -3;
        int ret[U], sl[U];
        int64_t row[U];
        float w[U];
        bool cont = true;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load(slab, c0 + u, ne, ret[u], row[u], sl[u], w[u]);
            cont = cont && ret[u] == prev;
            if (cont) {
                ret[u] = -2;
                row[u] = -1;
            }
        }
        V v[U];
        rows_of(row, sl, v);
        V acc = vzero((V*)nullptr);
        int cur = -2;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (ret[u] == -2) continue;
            if (ret[u] != cur) {
                store(src, cur, acc);
                acc = vzero((V*)nullptr);
                cur = ret[u];
            }
            if (row[u] >= 0) acc = vadd(acc, vscale(v[u], w[u]));
        }
        // the chunk's last run may go on past it: walk the rest of it, U records at a time
        if (cur >= 0 && (int64_t)cur < cap_b) {
            for (int64_t j0 = c0 + U; j0 < ne && bag_record_ret(slab[1 + j0]) == cur; j0 += U) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    load(slab, j0 + u, ne, ret[u], row[u], sl[u], w[u]);
                    if (ret[u] != cur) row[u] = -1;
                }
                rows_of(row, sl, v);
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (row[u] >= 0 && ret[u] == cur) acc = vadd(acc, vscale(v[u], w[u]));
                if (ret[U - 1] != cur) break;
            }
        }
        store(src, cur, acc);
    }
}

// ------------------------------------------------------------------------------------------------
// requester: combine the partial rows of every bag
// ------------------------------------------------------------------------------------------------
// bag_csr_k's lane mapping and final step: acc = sum of the bag's partials in ascending owner order (from 0), then / denom for mean and
// sqrtn when the bag had a live entry.  DO_FM: fm_k's sums over the slots of the sample, on the values written -- the logit is
// dir_fm_second_order_f32 of out bit for bit.
template <int LPS, int VEC, bool DO_FM>
__global__ __launch_bounds__(256) void bags_combine_k(const float* __restrict__ back, int K, int P, const int32_t* __restrict__ pos,
                                                      const uint64_t* __restrict__ mask, const float* __restrict__ denom,
                                                      const int32_t* __restrict__ slot_combiner, int combiner, int64_t B, int F,
                                                      float* __restrict__ out, int64_t out_ld, float* __restrict__ fm) {
    using V = typename VecT<VEC>::T;
    constexpr int SPW = 64 / LPS;
    const int lane = threadIdx.x & 63;
    const int c = lane & (LPS - 1);
    const int s = lane / LPS;
    const int kv = (K + VEC - 1) / VEC;
    const bool cact = c < kv;
    const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t gw = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gw * SPW < B; gw += nwave) {
        const int64_t b = gw * SPW + s;
        const bool sact = b < B;
        const bool act = cact && sact;
        V sum = vzero((V*)nullptr), sq = vzero((V*)nullptr);
        for (int f = 0; f < F; ++f) {
            V acc = vzero((V*)nullptr);
            if (sact) {
                const int64_t g = b * F + f;
                const uint64_t m = mask[g];
                for_each_owner(m, [&](int o) {
                    const int32_t p = pos[g * P + o];
                    if (p >= 0 && cact) acc = vadd(acc, ldv(back + (int64_t)p * K + c * VEC, (V*)nullptr));
                });
                const int comb = slot_combiner ? slot_combiner[f] : combiner;
                if (m && comb != DIR_COMBINER_SUM) acc = vdiv(acc, denom[g]);
                if (act) stv(out + b * out_ld + (int64_t)f * K + c * VEC, acc);
            }
            if (DO_FM) {
                sum = vadd(sum, acc);
                sq = vadd(sq, vmul(acc, acc));
            }
        }
        if (DO_FM) {
            const float r = fm_tail<LPS>(sum, sq, lane, c);
            if (c == LPS - 1 && sact) fm[b] = r;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// requester, backward: scatter the bag gradients to the partial rows they came from
// ------------------------------------------------------------------------------------------------
// The transpose of bags_combine_k with its lane mapping: every owner o in mask[g] gets c_bag * g[b, f*K..] (c_bag = 1 / denom for mean
// and sqrtn, 1 for sum) at row pos[g*P + o] of `send` -- the row where the forward received that partial.  Rows no partial came back
// from are not written (the owners never read them).  The buffer then travels the partial-row exchange in reverse.
template <int LPS, int VEC>
__global__ __launch_bounds__(256) void bags_grad_k(const float* __restrict__ g, int64_t g_ld, int K, int P, const int32_t* __restrict__ pos,
                                                   const uint64_t* __restrict__ mask, const float* __restrict__ denom,
                                                   const int32_t* __restrict__ slot_combiner, int combiner, int64_t B, int F,
                                                   float* __restrict__ send, int64_t n_rows) {
    using V = typename VecT<VEC>::T;
    constexpr int SPW = 64 / LPS;
    const int lane = threadIdx.x & 63;
    const int c = lane & (LPS - 1);
    const int s = lane / LPS;
    const int kv = (K + VEC - 1) / VEC;
    const bool cact = c < kv;
    const int64_t nwave = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t gw = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gw * SPW < B; gw += nwave) {
        const int64_t b = gw * SPW + s;
        if (b >= B) continue;
        for (int f = 0; f < F; ++f) {
            const int64_t gi = b * F + f;
            const uint64_t m = mask[gi];
            if (!m) continue;
            const int comb = slot_combiner ? slot_combiner[f] : combiner;
            V gv = ldv(g + b * g_ld + (int64_t)f * K + (cact ? c * VEC : 0), (V*)nullptr);
            if (comb != DIR_COMBINER_SUM) gv = vdiv(gv, denom[gi]);
            for_each_owner(m, [&](int o) {
                const int32_t p = pos[gi * P + o];
                if (p >= 0 && (int64_t)p < n_rows && cact) stv(send + (int64_t)p * K + c * VEC, gv);
            });
        }
    }
}

static int next_pow2_sb(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace dir

using namespace dir;

// 64 packed (pairs << 32 | entries) counters + the arrival counter (+ padding): zero before the first call, left zero by every call
extern "C" int64_t dir_shard_bags_workspace_bytes(int P) { return P > 0 && P <= 64 ? 1024 : 0; }

extern "C" int dir_shard_bags_bucket(const int64_t* ids, const int64_t* offsets, const float* weights, int64_t nnz, int64_t stride_b,
                                     int64_t stride_f, int64_t B, const int64_t* vocab, const int32_t* parts, const int32_t* first, int F,
                                     int P, const int32_t* slot_combiner, int combiner, int flags, int64_t cap_e, int64_t cap_b,
                                     int64_t* slabs, int32_t* pos, int64_t* mask, float* denom, int64_t* stat, void* workspace,
                                     dir_stream_t stream) {
    DIR_CHECK_ARG(F > 0 && B >= 0 && nnz >= 0 && nnz < ((int64_t)1 << 31), "dir_shard_bags_bucket: F=%d B=%lld nnz=%lld (nnz < 2^31)", F,
                  (long long)B, (long long)nnz);
    if (int rc = check_slab_geometry("dir_shard_bags_bucket", P, cap_e, cap_b)) return rc;
    DIR_CHECK_ARG(combiner >= DIR_COMBINER_SUM && combiner <= DIR_COMBINER_SQRTN, "dir_shard_bags_bucket: combiner=%d", combiner);
    DIR_CHECK_ARG(vocab && slabs && workspace, "dir_shard_bags_bucket: null pointer");
    DIR_CHECK_ARG(B == 0 || (offsets && pos && mask && denom && (nnz == 0 || ids)), "dir_shard_bags_bucket: null pointer");
    const int64_t nbags = B * F;
    // bags per thread: at most ~2048 workgroups of 2 waves (2 per SIMD: the walks are latency-bound; 2048 reservations per owner
    // counter queue for ~23 us at ~90 per us, spread over the launch)
    int bpt = 1;
    while (bpt < 64 && (nbags + (int64_t)SB_NT * bpt - 1) / ((int64_t)SB_NT * bpt) > 2048) bpt <<= 1;
    const int64_t grid = nbags > 0 ? (nbags + (int64_t)SB_NT * bpt - 1) / ((int64_t)SB_NT * bpt) : 1;
    hipLaunchKernelGGL(bags_bucket_k, dim3((unsigned)grid), dim3(SB_NT), (size_t)P * SB_NT * sizeof(int), as_stream(stream), ids, offsets,
                       weights, stride_b, stride_f, B, F, vocab, parts, first, P, flags, slot_combiner, combiner, cap_e, cap_b, bpt,
                       reinterpret_cast<int4*>(slabs), pos, reinterpret_cast<uint64_t*>(mask), denom,
                       static_cast<unsigned long long*>(workspace), stat);
    DIR_CHECK_LAUNCH("shard_bags_bucket");
    return DIR_OK;
}

extern "C" int dir_shard_bags_pool_f32(const float* const* tables, const int64_t* local_vocab, int F, int K, const int64_t* recv, int P,
                                       int64_t cap_e, int64_t cap_b, const float* slot_max_norm, float max_norm, int flags, float* out,
                                       int64_t* stat, dir_stream_t stream) {
    DIR_CHECK_ARG(F > 0 && K > 0 && cap_e > 0 && cap_b > 0, "dir_shard_bags_pool_f32: F=%d K=%d cap_e=%lld cap_b=%lld", F, K, (long long)cap_e,
                  (long long)cap_b);
    if (int rc = check_owners("dir_shard_bags_pool_f32", P)) return rc;
    DIR_CHECK_ARG(!(max_norm < 0.f), "dir_shard_bags_pool_f32: max_norm=%g", max_norm);
    DIR_CHECK_ARG(tables && local_vocab && recv && out, "dir_shard_bags_pool_f32: null pointer");
    const bool vec = (K % 4 == 0) && aligned16(out);
    const int lps = next_pow2_sb(vec ? K / 4 : K);
    if (lps > 64) return fail(DIR_E_UNSUPPORTED, "dir_shard_bags_pool_f32: K=%d is wider than one wave covers (max %d)", K, vec ? 256 : 64);
    const int spw = 64 / lps;
    const int64_t waves = ((int64_t)P * ((cap_e + 7) / 8) + spw - 1) / spw;     // one lane group per chunk of 8 entry slots
    dim3 grid(grid_for((waves + 3) / 4));
    hipStream_t st = as_stream(stream);
    const int4* r = reinterpret_cast<const int4*>(recv);
    const bool clip = max_norm > 0.f || slot_max_norm;
    dispatch_lps(vec, lps, [&](auto L, auto V) {
        auto k = clip ? bags_pool_k<decltype(L)::value, decltype(V)::value, true> : bags_pool_k<decltype(L)::value, decltype(V)::value, false>;
        hipLaunchKernelGGL(k, grid, dim3(256), 0, st, tables, local_vocab, F, K, r, P, cap_e, cap_b, slot_max_norm, max_norm, flags, out, stat);
    });
    DIR_CHECK_LAUNCH("shard_bags_pool");
    return DIR_OK;
}

extern "C" int dir_shard_bags_combine_f32(const float* back, int K, int P, const int32_t* pos, const int64_t* mask, const float* denom,
                                          int64_t B, int F, const int32_t* slot_combiner, int combiner, float* out, int64_t out_ld,
                                          float* fm, dir_stream_t stream) {
    DIR_CHECK_ARG(F > 0 && K > 0 && B >= 0, "dir_shard_bags_combine_f32: F=%d K=%d B=%lld", F, K, (long long)B);
    if (int rc = check_owners("dir_shard_bags_combine_f32", P)) return rc;
    DIR_CHECK_ARG(combiner >= DIR_COMBINER_SUM && combiner <= DIR_COMBINER_SQRTN, "dir_shard_bags_combine_f32: combiner=%d", combiner);
    DIR_CHECK_ARG(out_ld >= (int64_t)F * K, "dir_shard_bags_combine_f32: out_ld=%lld < F*K=%lld", (long long)out_ld, (long long)F * K);
    // the FM step's lane layout follows dir_fm_second_order_f32's choice on `out`, so that the fused logit is that kernel's bit for bit
    const bool vec = (K % 4 == 0) && (out_ld % 4 == 0) && aligned16(out);
    const int lps = next_pow2_sb(vec ? K / 4 : K);
    if (lps > 64) return fail(DIR_E_UNSUPPORTED, "dir_shard_bags_combine_f32: K=%d is wider than one wave covers (max %d)", K, vec ? 256 : 64);
    if (B == 0) return DIR_OK;  // an empty batch carries no buffers
    DIR_CHECK_ARG(back && pos && mask && denom && out, "dir_shard_bags_combine_f32: null pointer");
    if (vec && !aligned16(back)) return fail(DIR_E_UNSUPPORTED, "dir_shard_bags_combine_f32: back must be 16-byte aligned");
    const int spw = 64 / lps;
    const int64_t waves = (B + spw - 1) / spw;
    dim3 grid(grid_for((waves + 3) / 4));
    hipStream_t st = as_stream(stream);
    const uint64_t* m = reinterpret_cast<const uint64_t*>(mask);
    dispatch_lps(vec, lps, [&](auto L, auto V) {
        auto k = fm ? bags_combine_k<decltype(L)::value, decltype(V)::value, true> : bags_combine_k<decltype(L)::value, decltype(V)::value, false>;
        hipLaunchKernelGGL(k, grid, dim3(256), 0, st, back, K, P, pos, m, denom, slot_combiner, combiner, B, F, out, out_ld, fm);
    });
    DIR_CHECK_LAUNCH("shard_bags_combine");
    return DIR_OK;
}

extern "C" int dir_shard_bags_grad_f32(const float* g, int64_t g_ld, int K, int P, const int32_t* pos, const int64_t* mask, const float* denom,
                                       int64_t B, int F, const int32_t* slot_combiner, int combiner, int64_t cap_b, float* send,
                                       dir_stream_t stream) {
    const char* name = "dir_shard_bags_grad_f32";
    DIR_CHECK_ARG(F > 0 && K > 0 && B >= 0, "%s: F=%d K=%d B=%lld", name, F, K, (long long)B);
    if (int rc = check_partial_geometry(name, P, cap_b)) return rc;
    DIR_CHECK_ARG(combiner >= DIR_COMBINER_SUM && combiner <= DIR_COMBINER_SQRTN, "%s: combiner=%d", name, combiner);
    DIR_CHECK_ARG(g_ld >= (int64_t)F * K, "%s: g_ld=%lld < F*K=%lld", name, (long long)g_ld, (long long)F * K);
    DIR_CHECK_ARG(send, "%s: null pointer", name);
    DIR_CHECK_ARG(B == 0 || (g && pos && mask && denom), "%s: null pointer", name);
    const bool vec = (K % 4 == 0) && (g_ld % 4 == 0) && aligned16(g) && aligned16(send);
    const int lps = next_pow2_sb(vec ? K / 4 : K);
    if (lps > 64) return fail(DIR_E_UNSUPPORTED, "%s: K=%d is wider than one wave covers (max %d)", name, K, vec ? 256 : 64);
    if (B == 0) return DIR_OK;
    const int spw = 64 / lps;
    const int64_t waves = (B + spw - 1) / spw;
    dim3 grid(grid_for((waves + 3) / 4));
    hipStream_t st = as_stream(stream);
    const uint64_t* m = reinterpret_cast<const uint64_t*>(mask);
    const int64_t n_rows = (int64_t)P * cap_b;
    dispatch_lps(vec, lps, [&](auto L, auto V) {
        hipLaunchKernelGGL((bags_grad_k<decltype(L)::value, decltype(V)::value>), grid, dim3(256), 0, st, g, g_ld, K, P, pos, m, denom,
                           slot_combiner, combiner, B, F, send, n_rows);
    });
    DIR_CHECK_LAUNCH("shard_bags_grad");
    return DIR_OK;
}
