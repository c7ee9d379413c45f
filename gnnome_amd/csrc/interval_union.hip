// Union of read intervals per group (utils/labels.py:5-20, interval_union), on intervals the caller has ordered by (group, start).
//
// The statement (tests/interval_statement.py): walking a group in start order with R = the largest end seen so far in the group,
// interval i opens a new island iff it is the group's first or start[i] > R; start[i] == R touches and merges.  An island is
// [start of its head, R at its last member].  With end >= start for every interval - the Python wrapper refuses anything else - R at
// an island's last member is the largest end of the island's own members, because a head's end is >= its start > every earlier end
// of the group: the reference's result[-1][1].  The reference has one group; a group per chromosome is this project's addition.
//
// Two segmented scans over fixed tiles of kIuTile positions, each in three launches (per-tile reduce, ONE workgroup over the tile
// summaries, per-tile apply); the second scan's reduce needs the first scan's result, so the launches are, in order:
//   k_iu_reduce_max   per tile: the segmented summary (a group starts in the tile, largest end after the last group start)
//   k_iu_carry<IuMax> ONE workgroup: exclusive segmented scan of the summaries -> the running maximum that enters every tile
//   k_iu_reduce_cnt   per tile: redo the max-scan inside the tile, flag the heads, and sum (heads, group starts) plus, segmented by
//                     group, the heads and the covered length
//   k_iu_carry<IuCnt> ONE workgroup: exclusive scan of those -> island index, group index and group sums that enter every tile; K, G
//   k_iu_apply        per tile: the same in-tile scans on top of the carries; a head writes its island's group and start, an island's
//                     last member its end, a group's last member the group's code, island count and covered length
// The scan operators are (value, segment-flag) pairs combined with __shfl_up inside a wavefront, through LDS across the four
// wavefronts of a workgroup.  No kernel waits on another workgroup, every output slot has exactly one writer (plain vector stores,
// no atomics), everything is integer: the output is a pure function of the input and does not depend on the grid.
// The covered length of a group is the sum over its positions of (R if the position ends an island) - (start if it heads one), in
// 64-bit wrap-around arithmetic: exact whenever the true figure fits int64, whatever the partial sums do.
#include "common.h"

namespace gnnome {

constexpr int kIuThreads = 256;
constexpr int kIuItems = 4;                        // consecutive positions per thread
constexpr int kIuTile = kIuThreads * kIuItems;     // positions per tile
constexpr int kIuWaves = kIuThreads / kWave;

typedef unsigned long long u64;

// running maximum of `end` inside a group; `f`: a group starts at or before this position (within what was combined)
struct IuMax {
    int64_t v;
    int f;
    __device__ static IuMax identity() { return IuMax{INT64_MIN, 0}; }
    __device__ static IuMax combine(const IuMax& a, const IuMax& b) { return IuMax{b.f ? b.v : (a.v > b.v ? a.v : b.v), a.f | b.f}; }
    __device__ static IuMax shfl_up(const IuMax& a, int o) { return IuMax{(int64_t)__shfl_up((u64)a.v, o), __shfl_up(a.f, o)}; }
};

// tot = (heads << 32) | group starts, over everything (each < 2^31); cov and seg = covered length and heads of the current group
struct IuCnt {
    u64 tot, cov;
    unsigned seg;
    int f;
    __device__ static IuCnt identity() { return IuCnt{0ull, 0ull, 0u, 0}; }
    __device__ static IuCnt combine(const IuCnt& a, const IuCnt& b) {
        return IuCnt{a.tot + b.tot, b.f ? b.cov : a.cov + b.cov, b.f ? b.seg : a.seg + b.seg, a.f | b.f};
    }
    __device__ static IuCnt shfl_up(const IuCnt& a, int o) {
        return IuCnt{__shfl_up(a.tot, o), __shfl_up(a.cov, o), __shfl_up(a.seg, o), __shfl_up(a.f, o)};
    }
};

struct IuLayout {
    size_t info, max_sums, cnt_sums, total;
};

static inline size_t iu_align(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ static inline int64_t iu_tiles(int64_t n) { return (n + kIuTile - 1) / kIuTile; }

static IuLayout iu_layout(int64_t M) {
    IuLayout L;
    size_t o = 0;
    L.info = o;     o = iu_align(o + sizeof(IuCnt));   // the combination of all tiles: K and G
    L.max_sums = o; o = iu_align(o + (size_t)iu_tiles(M) * sizeof(IuMax));
    L.cnt_sums = o; o = iu_align(o + (size_t)iu_tiles(M) * sizeof(IuCnt));
    L.total = o;
    return L;
}

static unsigned iu_grid(int64_t tiles) { return (unsigned)(tiles < 1 ? 1 : tiles < kNumCUs * 8 ? tiles : kNumCUs * 8); }

// the combination of the aggregates of all earlier threads of the workgroup (exclusive), and of all its threads
template <class T>
__device__ __forceinline__ T iu_block_scan(const T agg, T* __restrict__ wave_s, T& total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    T inc = agg;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T up = T::shfl_up(inc, o);
        if (lane >= o) inc = T::combine(up, inc);
    }
    const T prev = T::shfl_up(inc, 1);
    __syncthreads();   // wave_s may still be read by the previous call
    if (lane == kWave - 1) wave_s[wave] = inc;
    __syncthreads();
    T before = T::identity(), all = T::identity();
#pragma unroll
    for (int w = 0; w < kIuWaves; ++w) {
        const T s = wave_s[w];
        if (w < wave) before = T::combine(before, s);
        all = T::combine(all, s);
    }
    total = all;
    return lane == 0 ? before : T::combine(before, prev);
}

// A thread's kIuItems positions of tile t.  f[a]: position a starts a group (a = kIuItems: the position after the thread's last).
struct IuItems {
    int64_t i0, s[kIuItems + 1], e[kIuItems];
    int32_t g[kIuItems];
    int f[kIuItems + 1];
};

__device__ __forceinline__ void iu_load(const int64_t* __restrict__ start, const int64_t* __restrict__ end, const int32_t* __restrict__ group,
                                        int64_t M, int64_t t, IuItems& it) {
    it.i0 = t * kIuTile + (int64_t)threadIdx.x * kIuItems;
    int32_t before = it.i0 > 0 && it.i0 - 1 < M ? group[it.i0 - 1] : 0;
#pragma unroll
    for (int a = 0; a <= kIuItems; ++a) {
        const int64_t i = it.i0 + a;
        const bool in = i < M;
        const int32_t g = in ? group[i] : 0;
        it.s[a] = in ? start[i] : 0;
        it.f[a] = in && (i == 0 || g != before);
        if (a < kIuItems) {
            it.e[a] = in ? end[i] : 0;
            it.g[a] = g;
        }
        before = g;
    }
}

__device__ __forceinline__ IuMax iu_max_aggregate(const IuItems& it, int64_t M) {
    IuMax agg = IuMax::identity();
#pragma unroll
    for (int a = 0; a < kIuItems; ++a)
        if (it.i0 + a < M) agg = IuMax::combine(agg, IuMax{it.e[a], it.f[a]});
    return agg;
}

// The max-scan inside tile t on top of the running maximum `carry` that enters it.  head[a]: position a heads an island; last[a]: it is
// the last member of one; r[a]: the running maximum of its group at and including it.  cnt[a]: its element of the second scan.
__device__ __forceinline__ void iu_tile_heads(const IuItems& it, int64_t M, const IuMax carry, IuMax* __restrict__ wave_s, int (&head)[kIuItems],
                                              int (&last)[kIuItems], int64_t (&r)[kIuItems], IuCnt (&cnt)[kIuItems]) {
    IuMax total;
    IuMax run = IuMax::combine(carry, iu_block_scan(iu_max_aggregate(it, M), wave_s, total));
#pragma unroll
    for (int a = 0; a < kIuItems; ++a) {
        const bool in = it.i0 + a < M;
        head[a] = in && (it.f[a] || it.s[a] > run.v);
        if (in) run = IuMax::combine(run, IuMax{it.e[a], it.f[a]});
        r[a] = run.v;
    }
    const int head_after = it.i0 + kIuItems < M && (it.f[kIuItems] || it.s[kIuItems] > run.v);
#pragma unroll
    for (int a = 0; a < kIuItems; ++a) {
        const int64_t i = it.i0 + a;
        last[a] = i < M && (i == M - 1 || (a + 1 < kIuItems ? head[a + 1] : head_after));
        const u64 cov = (last[a] ? (u64)r[a] : 0ull) - (head[a] ? (u64)it.s[a] : 0ull);
        cnt[a] = IuCnt{((u64)head[a] << 32) | (u64)it.f[a], cov, (unsigned)head[a], it.f[a]};
    }
}

__global__ void __launch_bounds__(kIuThreads) k_iu_reduce_max(const int64_t* __restrict__ end, const int32_t* __restrict__ group, int64_t M,
                                                              IuMax* __restrict__ sums) {
    __shared__ IuMax wave_s[kIuWaves];
    const int64_t tiles = iu_tiles(M);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i0 = t * kIuTile + (int64_t)threadIdx.x * kIuItems;
        int32_t before = i0 > 0 && i0 - 1 < M ? group[i0 - 1] : 0;
        IuMax agg = IuMax::identity(), total;
#pragma unroll
        for (int a = 0; a < kIuItems; ++a) {
            const int64_t i = i0 + a;
            if (i < M) {
                const int32_t g = group[i];
                agg = IuMax::combine(agg, IuMax{end[i], i == 0 || g != before});
                before = g;
            }
        }
        iu_block_scan(agg, wave_s, total);
        if (threadIdx.x == 0) sums[t] = total;
    }
}

// launched with ONE workgroup: sums[t] becomes the combination of the tiles before t; the combination of all tiles goes to total_out[0]
template <class T>
__global__ void __launch_bounds__(kIuThreads) k_iu_carry(T* __restrict__ sums, int64_t tiles, T* __restrict__ total_out) {
    __shared__ T wave_s[kIuWaves];
    T carry = T::identity();
    for (int64_t c0 = 0; c0 < tiles; c0 += kIuTile) {
        const int64_t i0 = c0 + (int64_t)threadIdx.x * kIuItems;
        T v[kIuItems], agg = T::identity(), total;
#pragma unroll
        for (int a = 0; a < kIuItems; ++a) {
            v[a] = i0 + a < tiles ? sums[i0 + a] : T::identity();
            agg = T::combine(agg, v[a]);
        }
        T run = T::combine(carry, iu_block_scan(agg, wave_s, total));
#pragma unroll
        for (int a = 0; a < kIuItems; ++a) {
            if (i0 + a < tiles) sums[i0 + a] = run;
            run = T::combine(run, v[a]);
        }
        carry = T::combine(carry, total);
    }
    if (threadIdx.x == 0 && total_out) total_out[0] = carry;
}

__global__ void __launch_bounds__(kIuThreads) k_iu_reduce_cnt(const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                              const int32_t* __restrict__ group, int64_t M, const IuMax* __restrict__ max_sums,
                                                              IuCnt* __restrict__ cnt_sums) {
    __shared__ IuMax wave_m[kIuWaves];
    __shared__ IuCnt wave_c[kIuWaves];
    const int64_t tiles = iu_tiles(M);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        IuItems it;
        int head[kIuItems], last[kIuItems];
        int64_t r[kIuItems];
        IuCnt cnt[kIuItems], total;
        iu_load(start, end, group, M, t, it);
        iu_tile_heads(it, M, max_sums[t], wave_m, head, last, r, cnt);
        IuCnt agg = IuCnt::identity();
#pragma unroll
        for (int a = 0; a < kIuItems; ++a) agg = IuCnt::combine(agg, cnt[a]);
        iu_block_scan(agg, wave_c, total);
        if (threadIdx.x == 0) cnt_sums[t] = total;
    }
}

__global__ void __launch_bounds__(kIuThreads) k_iu_apply(const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                                                         const int32_t* __restrict__ group, int64_t M, const IuMax* __restrict__ max_sums,
                                                         const IuCnt* __restrict__ cnt_sums, uint8_t* __restrict__ head_out,
                                                         int32_t* __restrict__ isl_group, int64_t* __restrict__ isl_start,
                                                         int64_t* __restrict__ isl_end, int64_t max_groups, int32_t* __restrict__ grp_code,
                                                         int64_t* __restrict__ grp_covered, int64_t* __restrict__ grp_count) {
    __shared__ IuMax wave_m[kIuWaves];
    __shared__ IuCnt wave_c[kIuWaves];
    const int64_t tiles = iu_tiles(M);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        IuItems it;
        int head[kIuItems], last[kIuItems];
        int64_t r[kIuItems];
        IuCnt cnt[kIuItems], total;
        iu_load(start, end, group, M, t, it);
        iu_tile_heads(it, M, max_sums[t], wave_m, head, last, r, cnt);
        IuCnt agg = IuCnt::identity();
#pragma unroll
        for (int a = 0; a < kIuItems; ++a) agg = IuCnt::combine(agg, cnt[a]);
        IuCnt run = IuCnt::combine(cnt_sums[t], iu_block_scan(agg, wave_c, total));
#pragma unroll
        for (int a = 0; a < kIuItems; ++a) {
            const int64_t i = it.i0 + a;
            if (i >= M) break;
            run = IuCnt::combine(run, cnt[a]);
            const int64_t k = (int64_t)(run.tot >> 32) - 1;              // the island of position i: heads up to and including i, less one
            const int64_t grp = (int64_t)(run.tot & 0xFFFFFFFFull) - 1;  // its group, counted from 0 in input order
            if (head_out) head_out[i] = (uint8_t)head[a];
            if (k < 0 || k >= M) continue;                               // position 0 is a head: never taken
            if (head[a]) {
                isl_group[k] = it.g[a];
                isl_start[k] = it.s[a];
            }
            if (last[a]) isl_end[k] = r[a];
            if ((i == M - 1 || it.f[a + 1]) && grp >= 0 && grp < max_groups) {   // the group's last position
                grp_code[grp] = it.g[a];
                grp_covered[grp] = (int64_t)run.cov;
                grp_count[grp] = (int64_t)run.seg;
            }
        }
    }
}

}  // namespace gnnome

extern "C" int gnnome_interval_union_tile_size(int* tile_host) {
    GN_REQUIRE(tile_host, "interval_union_tile_size: null pointer");
    *tile_host = gnnome::kIuTile;
    return GNNOME_OK;
}

extern "C" int gnnome_interval_union_workspace_bytes(int64_t num_intervals, size_t* bytes_host) {
    GN_REQUIRE(num_intervals >= 0 && num_intervals < ((int64_t)1 << 31) && bytes_host,
               "interval_union_workspace_bytes: bad argument (num_intervals=%lld)", (long long)num_intervals);
    *bytes_host = gnnome::iu_layout(num_intervals).total;
    return GNNOME_OK;
}

extern "C" int gnnome_interval_union(const int64_t* start, const int64_t* end, const int32_t* group, int64_t num_intervals, uint8_t* head,
                                     int32_t* isl_group, int64_t* isl_start, int64_t* isl_end, int64_t max_groups, int32_t* grp_code,
                                     int64_t* grp_covered, int64_t* grp_count, int64_t* result_host, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    const int64_t M = num_intervals;
    GN_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "interval_union: num_intervals=%lld outside [0, 2^31)", (long long)M);
    GN_REQUIRE(result_host, "interval_union: null result_host");
    result_host[0] = result_host[1] = 0;
    if (M == 0) return GNNOME_OK;   // no interval, no island, nothing launched
    GN_REQUIRE(start && end && group && isl_group && isl_start && isl_end, "interval_union: null pointer");
    GN_REQUIRE(max_groups >= 1 && grp_code && grp_covered && grp_count, "interval_union: null group table or max_groups=%lld < 1",
               (long long)max_groups);
    GN_REQUIRE(workspace, "interval_union: null workspace");
    const IuLayout L = iu_layout(M);
    if (workspace_bytes < L.total) {
        set_error("interval_union: workspace %zu < %zu bytes", workspace_bytes, L.total);
        return GNNOME_EWORKSPACE;
    }
    IuCnt* info = (IuCnt*)((char*)workspace + L.info);
    IuMax* max_sums = (IuMax*)((char*)workspace + L.max_sums);
    IuCnt* cnt_sums = (IuCnt*)((char*)workspace + L.cnt_sums);
    hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = iu_tiles(M);
    const dim3 grid(iu_grid(tiles)), block(kIuThreads);
    hipLaunchKernelGGL(k_iu_reduce_max, grid, block, 0, s, end, group, M, max_sums);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_iu_carry<IuMax>, dim3(1), block, 0, s, max_sums, tiles, (IuMax*)nullptr);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_iu_reduce_cnt, grid, block, 0, s, start, end, group, M, (const IuMax*)max_sums, cnt_sums);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_iu_carry<IuCnt>, dim3(1), block, 0, s, cnt_sums, tiles, info);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_iu_apply, grid, block, 0, s, start, end, group, M, (const IuMax*)max_sums, (const IuCnt*)cnt_sums, head, isl_group,
                       isl_start, isl_end, max_groups, grp_code, grp_covered, grp_count);
    GN_LAUNCH_CHECK();
    IuCnt h;
    GN_HIP(hipMemcpyAsync(&h, info, sizeof(h), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    result_host[0] = (int64_t)(h.tot >> 32);
    result_host[1] = (int64_t)(h.tot & 0xFFFFFFFFull);
    GN_REQUIRE(result_host[1] <= max_groups, "interval_union: %lld groups, the group tables hold %lld (only those were written)",
               (long long)result_host[1], (long long)max_groups);
    return GNNOME_OK;
}
