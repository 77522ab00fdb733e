// shard_wire.hpp -- what travels between the ranks of a row-sharded lookup, defined once: the payload word, the one-hot slab, the bag
// slab and its 16-byte records, the walk over a bag's owners, and a bag's liveness rule and denominator.  Shared by ids.hip (one-hot
// bucketing and gathers), shard_bags.hip (multi-hot bags), shard_linear.hip (the first-order term on both) and backward.hip (the
// owner-side updates): a kernel that packs, unpacks or checks a record calls these, so "drops the same entries as the other path" and
// "rounds like the other path" are properties of the code.
//
// PAYLOAD WORD (int64): p = local_row * F + slot -- the row of slot `slot` on its owner.  p < 0: pruned, nobody owns it.
//
// ONE-HOT SLAB (the fixed-capacity, sync-free lookup): owner o gets cap payload words behind a one-word header, slabs (cap + 1) words
// apart:
//   word 0        header: low 32 bits = number of valid slots (<= cap); high 32 bits = the SENDER's largest per-owner demand of the
//                 micro-batch (may exceed cap).  Every rank learns every other rank's demand from the id exchange itself (slab_stat_k):
//                 the global overflow verdict needs no collective of its own.
//   word 1 + pos  payload word of the element at slab position pos.  inv[i] = o * cap + pos is the row of element i in the [P * cap, K]
//                 row buffer that comes back; pruned / out-of-range ids and elements that do not fit get inv = -1.
// The order inside a slab is arbitrary (atomics); inv is its exact inverse, so the looked-up values do not depend on it.
//
// BAG SLAB (multi-hot bags): (cap_e + 1) records of 16 bytes (int4), record 0 = header, records 1..cap_e = entries:
//   entry   x, y = payload word (little-endian halves), z = entry weight (fp32 bits), w = return position (-1: none): the partial row
//           of the entry's (bag, owner) pair among the owner's cap_b partial rows for this sender
//   header  x = entries in this slab (<= cap_e), y = partial rows asked for (<= cap_b), z, w = the SENDER's largest per-owner demand of
//           entries / partial rows (may exceed the capacities): every receiver reads every sender's demand off the exchange itself
// The entries of one (bag, owner) pair form one contiguous run, in entry order, all with the same return position.
#pragma once
#include "common.hpp"

namespace dir {

// ---- host: the geometry checks of the entries that take slabs (one wording each; DIR_OK or the failure code, dir_last_error set) ----
inline int check_owners(const char* name, int P) {
    DIR_CHECK_ARG(P > 0 && P <= 64, "%s: P=%d (1 <= P <= 64)", name, P);
    return DIR_OK;
}
inline int check_partial_geometry(const char* name, int P, int64_t cap_b) {        // the [P * cap_b] partial rows
    if (int rc = check_owners(name, P)) return rc;
    DIR_CHECK_ARG(cap_b > 0 && (int64_t)P * cap_b < ((int64_t)1 << 31), "%s: cap_b=%lld (cap_b > 0, P*cap_b < 2^31)", name, (long long)cap_b);
    return DIR_OK;
}
inline int check_slab_geometry(const char* name, int P, int64_t cap_e, int64_t cap_b) {      // P bag slabs and their partial rows
    if (int rc = check_owners(name, P)) return rc;
    DIR_CHECK_ARG(cap_e > 0 && cap_e < ((int64_t)1 << 31), "%s: cap_e=%lld (0 < cap_e < 2^31)", name, (long long)cap_e);
    return check_partial_geometry(name, P, cap_b);
}

#if defined(__HIPCC__)
// ---- payload word ----
__host__ __device__ __forceinline__ int64_t pack_payload(int64_t local, int F, int slot) { return local * F + slot; }
// p >= 0 -> (slot, row); the 32-bit division when it fits (~4x cheaper than the 64-bit software division)
__host__ __device__ __forceinline__ void unpack_payload(int64_t p, int F, int& slot, int64_t& row) {
    if (p < (int64_t)0x7fffffff) {
        const uint32_t r32 = (uint32_t)p / (uint32_t)F;
        slot = (int)((uint32_t)p - r32 * (uint32_t)F);
        row = r32;
    } else {
        row = p / F;
        slot = (int)(p - row * F);
    }
}

// ---- one-hot slab ----
template <class T>
__host__ __device__ __forceinline__ T* slab_of(T* recv, int64_t s, int64_t cap) { return recv + s * (cap + 1); }
__host__ __device__ __forceinline__ int64_t slab_count(int64_t header) { return (int64_t)(uint32_t)header; }
__host__ __device__ __forceinline__ int slab_demand(int64_t header) { return (int)(header >> 32); }
__host__ __device__ __forceinline__ int64_t make_slab_header(int64_t count, int64_t cap, int demand32) {
    return (count < cap ? count : cap) | ((int64_t)demand32 << 32);
}

// ---- bag slab ----
__host__ __device__ __forceinline__ const int4* bag_slab_of(const int4* recv, int64_t s, int64_t cap_e) { return recv + s * (cap_e + 1); }
__host__ __device__ __forceinline__ int4* bag_slab_of(int4* recv, int64_t s, int64_t cap_e) { return recv + s * (cap_e + 1); }
// the header's entry count, clamped: a record index below it lies inside the slab whatever was received
__host__ __device__ __forceinline__ int64_t bag_entries(const int4* slab, int64_t cap_e) {
    const int64_t ne = (int64_t)(unsigned int)slab[0].x;
    return ne < cap_e ? ne : cap_e;
}
__device__ __forceinline__ int4 make_bag_record(int64_t packed, float weight, int ret) {
    int4 r;
    r.x = (int)(uint32_t)(uint64_t)packed;
    r.y = (int)(uint32_t)((uint64_t)packed >> 32);
    r.z = __float_as_int(weight);
    r.w = ret;
    return r;
}
__device__ __forceinline__ int64_t bag_record_payload(const int4& r) { return (int64_t)(((uint64_t)(uint32_t)r.y << 32) | (uint32_t)r.x); }
__device__ __forceinline__ float bag_record_weight(const int4& r) { return __int_as_float(r.z); }
__device__ __forceinline__ int bag_record_ret(const int4& r) { return r.w; }
__device__ __forceinline__ int4 make_bag_header(unsigned int entries, unsigned int pairs, int64_t cap_e, int64_t cap_b,
                                                unsigned int demand_e, unsigned int demand_b) {
    int4 h;
    h.x = (int)((int64_t)entries < cap_e ? entries : (unsigned int)cap_e);
    h.y = (int)((int64_t)pairs < cap_b ? pairs : (unsigned int)cap_b);
    h.z = (int)demand_e;
    h.w = (int)demand_b;
    return h;
}
// bag_record_payload and bag_record_valid have one caller, read_bag_record, and must STAY separate functions: with the two written
// out inside read_bag_record -- the same operations -- the compiler allocates bags_pool_k's registers differently, and that build's
// bags_pool_k<16,4,false> measured 3-4 % slower than the parent commit's (profiles/NOTES.md R7.3).  Do not inline them by hand.
// The check on a received record before its payload is decoded; what is left is the consumer's own `row < the slot's local rows`
// (slot < F holds by the decode).
__device__ __forceinline__ bool bag_record_valid(int64_t p, int ret, int64_t cap_b) { return p >= 0 && ret >= 0 && (int64_t)ret < cap_b; }
// Record j of a received slab with ne = bag_entries(slab): ret = its return position (-2 at or past ne) and w = its weight; true iff
// it is valid, and then (slot, row) is its decoded payload.  The pool, the linear pool and the key pass of the update all read records
// through this, so they drop the same entries by construction.
__device__ __forceinline__ bool read_bag_record(const int4* slab, int64_t j, int64_t ne, int F, int64_t cap_b, int& ret, float& w, int& slot,
                                                int64_t& row) {
    ret = -2;
    w = 0.f;
    if (j >= ne) return false;
    const int4 r = slab[1 + j];
    ret = bag_record_ret(r);
    const int64_t p = bag_record_payload(r);
    w = bag_record_weight(r);
    if (!bag_record_valid(p, ret, cap_b)) return false;
    unpack_payload(p, F, slot, row);
    return true;
}

// One wave (all 64 lanes): the largest demands me / mb of the headers its lanes hold -> every lane; lane 0 writes
// stat = {some demand > its capacity, largest entry demand, largest pair demand} when stat != nullptr.
__device__ __forceinline__ void bag_demand_stat(unsigned int& me, unsigned int& mb, int64_t cap_e, int64_t cap_b, int64_t* __restrict__ stat) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        me = max(me, (unsigned int)__shfl_xor((int)me, o, 64));
        mb = max(mb, (unsigned int)__shfl_xor((int)mb, o, 64));
    }
    if (stat && (threadIdx.x & 63) == 0) {
        stat[0] = ((int64_t)me > cap_e || (int64_t)mb > cap_b) ? 1 : 0;
        stat[1] = me;
        stat[2] = mb;
    }
}

// ---- the owners of a bag: bit o of mask[g] = owner o holds a live entry of bag g; walked in ascending owner order ----
// (lowest_bit is a name of its own because wave_agg_rank in ids.hip picks a wave's leader lane with it: one spelling of the ffs idiom)
__device__ __forceinline__ int lowest_bit(unsigned long long m) { return __ffsll((long long)m) - 1; }
template <class Fn>
__device__ __forceinline__ void for_each_owner(uint64_t mask, Fn&& fn) {
    for (uint64_t mm = mask; mm; mm &= mm - 1ull) fn(lowest_bit(mm));
}

// ---- liveness and denominator of a bag (bag_csr_k's / linear_csr_k's rule and sums) ----
// An entry counts iff its id lies inside [0, V) and, under PRUNE_NONPOSITIVE_WEIGHTS (prune_w), its weight is > 0.
__device__ __forceinline__ bool bag_entry_live(int64_t id, float w, int64_t V, bool prune_w) {
    return (uint64_t)id < (uint64_t)V && !(prune_w && !(w > 0.0f));
}
// wsum, w2sum and the count over the live entries in entry order (w = 1 without weights); value(): what mean / sqrtn divide by (sum: 1)
struct BagDenom {
    float wsum = 0.f, w2sum = 0.f;
    int n = 0;
    __device__ __forceinline__ void add(float w) {
        wsum = wsum + w;
        w2sum = w2sum + w * w;
        ++n;
    }
    __device__ __forceinline__ float value(int combiner, bool weighted) const {
        if (combiner == DIR_COMBINER_MEAN) return weighted ? wsum : (float)n;
        if (combiner == DIR_COMBINER_SQRTN) return weighted ? sqrtf(w2sum) : sqrtf((float)n);
        return 1.f;
    }
};

#endif  // __HIPCC__

}  // namespace dir
