// The one-wave-per-node row sum that node_neighbour.hip (forward) and node_neighbour_bwd.hip (backward) share: ONE copy of the lane
// mapping and of the association, so that the backward kernel without its epilogue leaves the bits the forward kernel leaves on the
// reversed graph.  Both are stated in node_neighbour.hip's header.
#pragma once
#include "common.h"

namespace gnnome {

constexpr int kNbrThreads = 256;
constexpr int kNbrHubThreshold = 4096;   // items above which a list is summed in two levels
constexpr int kNbrHubBlock = 128;        // items per first-level block of such a list (a multiple of the 64-item batch)
constexpr int kNbrInFlight = 4;          // row requests per lane group in flight

template <int H>
__device__ __forceinline__ float nbr_group_sum(float v) {
    // all-reduce over the lane groups (lanes with equal lane % (H/4)): node_aggregate_in.hip's in_group_sum
    constexpr int LPR = H / 4;
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// acc += sum over items [lo, hi) of one list (idx: the list's first neighbour id; NULL only for an empty list) of sscale[j] * h[j,:],
// lane group g taking every G-th item of every 64-item batch.  The bounds are wave-uniform (scalar loops).
template <int H, bool SS>
__device__ __forceinline__ void accumulate_rows(const float* __restrict__ h, int ldh, const float* __restrict__ sscale,
                                                const int32_t* __restrict__ idx, int lo, int hi, int lane, int group, int c, f32x4& acc) {
    constexpr int LPR = H / 4, G = 64 / LPR, U = kNbrInFlight;
    // the value lane `it` holds: `it` is uniform inside a lane group, so with one group (H = 256) it is a scalar read
    auto pick = [&](int v, int it) -> int {
        if (G == 1) return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(it));
        return __builtin_amdgcn_ds_bpermute(it << 2, v);
    };
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;   // lane l owns item base + l
        int my_n = 0;
        float my_s = 1.0f;
        if (j < hi) {
            my_n = idx[j];
            if (SS) my_s = sscale[my_n];
        }
        const int m = min(64, hi - base);
        for (int j0 = 0; j0 < m; j0 += G * U) {
            f32x4 a[U];
            float s[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int it = j0 + u * G + group;
                live[u] = it < m;
                const int sel = live[u] ? it : j0;   // (a dead slot reads item j0, which exists)
                a[u] = *reinterpret_cast<const f32x4*>(h + (int64_t)pick(my_n, sel) * ldh + c);
                s[u] = SS ? __int_as_float(pick(__float_as_int(my_s), sel)) : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (live[u]) {
                    if (SS) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[k] = fmaf(s[u], a[u][k], acc[k]);
                    } else {
                        acc += a[u];
                    }
                }
            }
        }
    }
}

// one list of `len` items into the node's accumulators: one block, or fixed 128-item blocks above the hub threshold
template <int H, bool SS>
__device__ __forceinline__ void accumulate_list(const float* __restrict__ h, int ldh, const float* __restrict__ sscale,
                                                const int32_t* __restrict__ idx, int len, int lane, int group, int c, f32x4& acc) {
    const int blk = len > kNbrHubThreshold ? kNbrHubBlock : len;   // (wave-uniform)
    for (int blo = 0; blo < len; blo += blk) {
        f32x4 part = {0.f, 0.f, 0.f, 0.f};
        accumulate_rows<H, SS>(h, ldh, sscale, idx, blo, min(len, blo + blk), lane, group, c, part);
        acc += part;
    }
}

// The whole sum of one node, in every lane: sscale[node] h[node,:] (lane group 0's start), then the list (ptr_a, idx_a), then - ptr_b
// not NULL - the list (ptr_b, idx_b), then the tree over the lane groups.  `node` is wave-uniform; lane = group * (H/4) + c / 4.
template <int H, bool SS>
__device__ __forceinline__ f32x4 nbr_node_sum(const float* __restrict__ h, int ldh, const float* __restrict__ sscale, int64_t node,
                                              const int32_t* __restrict__ ptr_a, const int32_t* __restrict__ idx_a,
                                              const int32_t* __restrict__ ptr_b, const int32_t* __restrict__ idx_b, int lane, int group, int c) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (group == 0) {   // the loop edge of g': the node's own row
        acc = *reinterpret_cast<const f32x4*>(h + node * ldh + c);
        if (SS) acc *= sscale[node];
    }
    const int ab = ptr_a[node], da = ptr_a[node + 1] - ab;
    accumulate_list<H, SS>(h, ldh, sscale, idx_a + ab, da, lane, group, c, acc);
    if (ptr_b != nullptr) {   // directed=False: the reverse copies of the node's other list
        const int bb = ptr_b[node], db = ptr_b[node + 1] - bb;
        accumulate_list<H, SS>(h, ldh, sscale, idx_b + bb, db, lane, group, c, acc);
    }
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = nbr_group_sum<H>(acc[k]);
    return v;
}

}  // namespace gnnome
