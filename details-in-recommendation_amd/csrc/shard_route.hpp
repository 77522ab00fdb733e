// shard_route.hpp -- the 'div' partition rule of the row-sharded tables ([TF-upstream] embedding_lookup partition_strategy='div',
// models/DeepFM/deepFM.py:163-167): owner and local row of an id.  Shared by ids.hip (the one-hot bucketing) and shard_bags.hip
// (the multi-hot bags).
#pragma once
#include "common.hpp"

namespace dir {

__host__ __device__ inline void div_owner(int64_t id, int64_t q, int64_t r, int64_t thr, int* owner, int64_t* local) {
    if (id < thr) {
        const int64_t o = id / (q + 1);
        *owner = (int)o;
        *local = id - o * (q + 1);
    } else {
        const int64_t o = r + (q > 0 ? (id - thr) / q : 0);
        *owner = (int)o;
        *local = id - (thr + (o - r) * q);
    }
}

// per-field 'div' constants q = V / Pf, thr = (V % Pf) * (q + 1), r = V % Pf, staged once per workgroup.  Pf = the number of
// row slices of the table (parts[f]; P when parts == NULL) and first = the rank holding slice 0 (slice j lives on rank
// (first + j) % P): the reference's min_max_variable_partitioner cuts a table into <= P slices of >= min_slice_size bytes
// (models/DeepFM/deepFM.py:163-167) and [TF-upstream] replica_device_setter deals the slices round-robin over the ps tasks.
struct FieldDiv { int64_t q, thr, V; int r; int small; int first; };

__device__ __forceinline__ FieldDiv make_fielddiv(int64_t V, int Pf, int first = 0) {
    FieldDiv d;
    d.q = V / Pf;
    d.r = (int)(V % Pf);
    d.thr = (int64_t)d.r * (d.q + 1);
    d.V = V;
    d.small = V < (int64_t)0x7fffffff ? 1 : 0;   // every quotient fits 32-bit unsigned arithmetic
    d.first = first;
    return d;
}

__device__ __forceinline__ void route_fd(int64_t id, const FieldDiv& d, int* owner, int64_t* local) {
    if (d.small) {   // 32-bit divisions (ids < vocab < 2^31): ~4x cheaper than the 64-bit software division
        const uint32_t u = (uint32_t)id, q = (uint32_t)d.q, thr = (uint32_t)d.thr;
        if (u < thr) {
            const uint32_t o = u / (q + 1);
            *owner = (int)o;
            *local = (int64_t)(u - o * (q + 1));
        } else {
            const uint32_t o = (uint32_t)d.r + (q > 0 ? (u - thr) / q : 0u);
            *owner = (int)o;
            *local = (int64_t)(u - (thr + (o - (uint32_t)d.r) * q));
        }
    } else {
        div_owner(id, d.q, d.r, d.thr, owner, local);
    }
}

}  // namespace dir
