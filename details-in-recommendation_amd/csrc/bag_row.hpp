// bag_row.hpp -- the per-row arithmetic of the embedding-bag kernels (16-byte row chunks per lane, LPS lanes per row), shared by
// embedding_bag.hip (bag_csr_k, the one-hot gathers, fm_k) and shard_bags.hip (the row-sharded bags): one definition, so the
// sharded path rounds exactly like the single-GPU one.
#pragma once
#include "common.hpp"

namespace dir {

template <int VEC> struct VecT;
template <> struct VecT<4> { using T = float4; };
template <> struct VecT<1> { using T = float; };

__device__ __forceinline__ float4 ldv(const float* p, float4*) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float ldv(const float* p, float*) { return *p; }
// non-temporal (streaming) row loads: a table row is read once per launch, so it should not displace
// the output / id lines in L2 and the Infinity Cache
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ldv_nt(const float* p, float4*) {
    f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float ldv_nt(const float* p, float*) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void stv(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void stv(float* p, float v) { *p = v; }
__device__ __forceinline__ float4 vzero(float4*) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float vzero(float*) { return 0.f; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vmul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float vmul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 vscale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float vscale(float a, float s) { return a * s; }
__device__ __forceinline__ float4 vdiv(float4 a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }
__device__ __forceinline__ float vdiv(float a, float s) { return a / s; }
// ordered horizontal add: acc + v.x + v.y + v.z + v.w, left to right
__device__ __forceinline__ float hadd_into(float acc, float4 v) { return (((acc + v.x) + v.y) + v.z) + v.w; }
__device__ __forceinline__ float hadd_into(float acc, float v) { return acc + v; }

// Exclusive upper bound of the ids of slot f as an unsigned value: ids are looked up iff (uint64_t)id < bound, which prunes
// id < 0 always and id >= vocab_f when the caller passed the vocabulary sizes (DEVICE [F]; NULL = precondition unchecked).
__device__ __forceinline__ uint64_t id_bound(const int64_t* __restrict__ vocab, int f) {
    return vocab ? (uint64_t)vocab[f] : (uint64_t)1 << 63;
}

// FM tail shared by the fused gather and the standalone kernel.  sum/sq hold this lane's chunk of
// sum_f e and sum_f e^2; returns 0.5 * sum_k (sum^2 - sq) in lane LPS-1 of the group.
template <int LPS, typename V>
__device__ __forceinline__ float fm_tail(V sum, V sq, int lane, int c) {
    V sm = vmul(sum, sum);
    V d;
    if constexpr (sizeof(V) == 16) {
        d = make_float4(sm.x - sq.x, sm.y - sq.y, sm.z - sq.z, sm.w - sq.w);
    } else {
        d = sm - sq;
    }
    float acc = 0.f;
    const int gbase = lane & ~(LPS - 1);
#pragma unroll
    for (int cc = 0; cc < LPS; ++cc) {
        float carry = __shfl(acc, gbase + (cc > 0 ? cc - 1 : 0), 64);
        if (c == cc) acc = hadd_into(cc == 0 ? 0.f : carry, d);
    }
    return 0.5f * acc;
}

// [TF-upstream] embedding_lookup(..., max_norm): every looked-up row is clipped to l2-norm max_norm BEFORE it is weighted
// (clip_ops.clip_by_norm, r1.10+ form):  row * max_norm / max(||row||, max_norm),  ||row|| = sqrt(sum_k row_k^2) (0 when
// the sum is 0).  The sum of squares runs k-ascending through the LPS lanes of the group (lane c -> c+1), so it is the
// oracle's sequential fp32 sum bit for bit.
template <int LPS, typename V>
__device__ __forceinline__ V clip_row(V row, float max_norm, int lane, int c) {
    V sq = vmul(row, row);
    float acc = 0.f;
    const int gbase = lane & ~(LPS - 1);
#pragma unroll
    for (int cc = 0; cc < LPS; ++cc) {
        float carry = __shfl(acc, gbase + (cc > 0 ? cc - 1 : 0), 64);
        if (c == cc) acc = hadd_into(cc == 0 ? 0.f : carry, sq);
    }
    const float l2sum = __shfl(acc, gbase + LPS - 1, 64);
    const float l2norm = l2sum > 0.f ? sqrtf(l2sum) : l2sum;
    return vdiv(vscale(row, max_norm), fmaxf(l2norm, max_norm));
}

}  // namespace dir
