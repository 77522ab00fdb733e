// run_sum.hpp -- the row-chunk vector type of the sorted sparse kernels (BV) and the compensated sum of one run of sorted entries
// (run_sum), shared by the sorted optimiser steps (backward.hip) and the sorted scatter-sum of rows (rows_scatter.hip): one definition,
// so that every sum over the same sorted entries is the same bits wherever it is formed.
#pragma once
#include "common.hpp"

#if defined(__HIPCC__)
namespace dir {

template <int VEC> struct BV;
template <> struct BV<4> {
    using T = float4;
    static __device__ __forceinline__ T ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
    static __device__ __forceinline__ void st(float* p, T v) { *reinterpret_cast<float4*>(p) = v; }
    static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
    static __device__ __forceinline__ T sub(T a, T b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
    static __device__ __forceinline__ T scale(T a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
    static __device__ __forceinline__ T fma(T a, float s, T c) { return make_float4(fmaf(a.x, s, c.x), fmaf(a.y, s, c.y), fmaf(a.z, s, c.z), fmaf(a.w, s, c.w)); }
    static __device__ __forceinline__ float dot(T a, T b, float acc) {
        acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
        return acc;
    }
    static __device__ __forceinline__ T upd(T x0, float xw, T b, T xl) {
        return make_float4(((x0.x * xw) + b.x) + xl.x, ((x0.y * xw) + b.y) + xl.y, ((x0.z * xw) + b.z) + xl.z, ((x0.w * xw) + b.w) + xl.w);
    }
    using D = double4;                                     // T in double: adagrad_fix_k's sum of a long run's tile partials
    static __device__ __forceinline__ D widen(T a) { return make_double4((double)a.x, (double)a.y, (double)a.z, (double)a.w); }
    static __device__ __forceinline__ D addw(D a, T b) { return make_double4(a.x + (double)b.x, a.y + (double)b.y, a.z + (double)b.z, a.w + (double)b.w); }
    static __device__ __forceinline__ T narrow(D a) { return make_float4((float)a.x, (float)a.y, (float)a.z, (float)a.w); }
    static __device__ __forceinline__ D addd(D a, D b) { return make_double4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
    static __device__ __forceinline__ D ldw(const double* p) { return *reinterpret_cast<const double4*>(p); }       // 32-byte aligned
    static __device__ __forceinline__ void stw(double* p, D v) { *reinterpret_cast<double4*>(p) = v; }
};
template <> struct BV<1> {
    using T = float;
    static __device__ __forceinline__ T ld(const float* p) { return *p; }
    static __device__ __forceinline__ void st(float* p, T v) { *p = v; }
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
    static __device__ __forceinline__ T sub(T a, T b) { return a - b; }
    static __device__ __forceinline__ T scale(T a, float s) { return a * s; }
    static __device__ __forceinline__ T fma(T a, float s, T c) { return fmaf(a, s, c); }
    static __device__ __forceinline__ float dot(T a, T b, float acc) { return fmaf(a, b, acc); }
    static __device__ __forceinline__ T upd(T x0, float xw, T b, T xl) { return ((x0 * xw) + b) + xl; }
    using D = double;
    static __device__ __forceinline__ D widen(T a) { return (double)a; }
    static __device__ __forceinline__ D addw(D a, T b) { return a + (double)b; }
    static __device__ __forceinline__ T narrow(D a) { return (float)a; }
    static __device__ __forceinline__ D addd(D a, D b) { return a + b; }
    static __device__ __forceinline__ D ldw(const double* p) { return *p; }
    static __device__ __forceinline__ void stw(double* p, D v) { *p = v; }
};

// The gradient sum of one run inside a tile, COMPENSATED (Kahan), for every rule.  A plain sequential fp32 sum of a row hit by hundreds
// or thousands of entries of one step (the head of a Zipf slot, a 7-row table under any batch) is off by 1e-5 ... 3e-4 absolute in an
// order-dependent way, and FTRL's z = z_prev + g - sigma * w can cancel to O(0.1) against summands of O(10): z, and w through it, then
// miss 1e-5 of float64.  With the compensation the sum is good to an ulp whatever the order -- which on the sharded paths is the order
// the slab's atomics left, different from run to run.  get(i): the gradient chunk of sorted entry i.  A run of ONE entry -- nearly every
// run under uniform ids over large tables -- is its own sum and pays nothing.  Longer runs keep four entries' loads in flight before
// their (ordered) adds.  Every loop of adagrad_tile_k sums through here, so two paths over the same sorted entries (packed and split
// rows, FM folded in or not, own sort or borrowed) agree bit for bit.
template <int VEC, class Get>
__device__ __forceinline__ typename BV<VEC>::T run_sum(int s, int e, Get get) {
    using V = BV<VEC>;
    using T = typename V::T;
    T sum = get(s);
    if (e - s == 1) return sum;
    T comp = V::zero();                                    // the low-order part the adds so far have lost
    auto kahan = [&](T x) {
        const T y = V::sub(x, comp), t = V::add(sum, y);
        comp = V::sub(V::sub(t, sum), y);
        sum = t;
    };
    int i = s + 1;
    for (; i + 4 <= e; i += 4) {
        const T d0 = get(i), d1 = get(i + 1), d2 = get(i + 2), d3 = get(i + 3);
        kahan(d0); kahan(d1); kahan(d2); kahan(d3);
    }
    for (; i < e; ++i) kahan(get(i));
    return sum;
}

}  // namespace dir
#endif
