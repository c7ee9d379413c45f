// Precision-recall curve and average precision of the edge scores (utils/metrics.py:51-80, which calls scikit-learn's
// precision_recall_curve and average_precision_score), for either class.
//
// With v the score of an edge (p, or 1.0f - p for the inverse pair) and `positive` its class bit, the statement is: sort by v
// descending; idx = the last position of every run of equal v; tp[j] = positives at positions <= idx[j], fp[j] = 1 + idx[j] - tp[j],
// thresholds[j] = v at idx[j]; precision = tp / (tp + fp), recall = tp / tp[-1]; both reversed and extended by (1, 0);
// AP = -sum(diff(recall) * precision[:-1]), clipped below at 0.
//
// The passes, in launch order:
//   k_pr_keys     per edge: v, the checks, key = (bits(v) << 1) | positive.  v lies in [0, 1], so bits(v) < 2^30 and is monotone in v:
//                 the class rides in the low bit and the sort needs no payload.
//   (the caller sorts the keys, descending)
//   k_pr_reduce   per tile of kPrTile sorted positions: (run ends, positives) summed as one 64-bit word (each count < 2^31)
//   k_pr_sums     ONE workgroup: exclusive scan of the tile sums, chunk by chunk with a carry -> M thresholds, P positives
//   (one host synchronisation: M, P and the check words)
//   k_pr_emit     per tile: the scan inside the tile on top of the tile's prefix; every run end j writes thresholds[j], tp[j], fp[j] and
//                 precision / recall at M-1-j; the last positive writes the cut index (its run is the first with tp = P)
//   k_pr_ap_tiles per tile of kPrTile terms (recall[r+1] - recall[r]) * precision[r]: a fixed tree;  k_pr_ap_sum  ONE workgroup: the
//                 tile partials in a fixed tree
// No kernel waits on another workgroup: the three phases of the scan are three launches.  Tiles are fixed, counts are integers and the
// only float sum is a fixed tree, so no bit depends on the grid; the only atomics are the integer minima of the check words.
// The file is compiled with -ffp-contract=off (Makefile): division, subtraction and multiplication stay separate IEEE operations.
#include "common.h"

namespace gnnome {

constexpr int kPrThreads = 256;
constexpr int kPrItems = 4;                        // consecutive positions per thread
constexpr int kPrTile = kPrThreads * kPrItems;     // sorted positions per tile
enum { kPrBadPred = 0, kPrBadLabel = 1, kPrThresholds = 2, kPrPositives = 3, kPrWords = 8 };

typedef unsigned long long u64;

struct PrLayout {
    size_t info, sums, partials, total;
};

static inline size_t pr_align(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ static inline int64_t pr_tiles(int64_t n) { return (n + kPrTile - 1) / kPrTile; }

static PrLayout pr_layout(int64_t E) {
    PrLayout L;
    size_t o = 0;
    L.info = o;     o = pr_align(o + kPrWords * sizeof(u64));
    L.partials = o; o = pr_align(o + (size_t)pr_tiles(E) * sizeof(double));   // M <= E terms; first, so that its place does not depend on E
    L.sums = o;     o = pr_align(o + (size_t)pr_tiles(E) * sizeof(u64));
    L.total = o;
    return L;
}

static unsigned pr_grid(int64_t tiles) { return (unsigned)(tiles < 1 ? 1 : tiles < kNumCUs * 8 ? tiles : kNumCUs * 8); }

// exclusive prefix of v over the workgroup's threads and the workgroup's total; integer, so the order of addition is immaterial
__device__ __forceinline__ u64 pr_block_scan(u64 v, u64* __restrict__ wave_s, u64& total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const u64 up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();   // wave_s may still be read by the previous call
    if (lane == kWave - 1) wave_s[wave] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kPrThreads / kWave; ++w) {
        const u64 s = wave_s[w];
        if (w < wave) before += s;
        all += s;
    }
    total = all;
    return before + inc - v;
}

// sum over the workgroup in a fixed tree (the same for every launch); the result is valid in thread 0
__device__ __forceinline__ double pr_block_tree(double v, double* __restrict__ r_s) {
    const int tid = threadIdx.x;
    __syncthreads();
    r_s[tid] = v;
    __syncthreads();
    for (int w = kPrThreads / 2; w > 0; w >>= 1) {
        if (tid < w) r_s[tid] += r_s[tid + w];
        __syncthreads();
    }
    return r_s[0];
}

__global__ void k_pr_keys(const float* __restrict__ preds, const float* __restrict__ labels, int64_t E, int apply_sigmoid, int inverse,
                          uint32_t* __restrict__ keys, float* __restrict__ probs_out, u64* __restrict__ info) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (int64_t)gridDim.x * blockDim.x) {
        float p = preds[i];
        if (apply_sigmoid) p = 1.0f / (1.0f + expf(-p));
        if (probs_out) probs_out[i] = p;
        const float y = labels[i];
        uint32_t key = 0;
        if (!(p >= 0.0f && p <= 1.0f)) {           // NaN included
            atomicMin(info + kPrBadPred, (u64)i);
        } else if (y != 0.0f && y != 1.0f) {       // NaN included
            atomicMin(info + kPrBadLabel, (u64)i);
        } else {
            const float v = (inverse ? 1.0f - p : p) + 0.0f;   // + 0.0f: -0.0 and 0.0 are one score
            key = (__float_as_uint(v) << 1) | (uint32_t)(inverse ? y == 0.0f : y == 1.0f);
        }
        keys[i] = key;
    }
}

// (run end << 32) | positive of sorted position i; keys descend, a run is a stretch of equal scores
__device__ __forceinline__ u64 pr_item(uint32_t k, uint32_t k_next, bool is_last) {
    const bool end = is_last || (k >> 1) != (k_next >> 1);
    return ((u64)end << 32) | (u64)(k & 1u);
}

// the thread's kPrItems items of tile t (zero past E)
__device__ __forceinline__ void pr_load(const uint32_t* __restrict__ keys, int64_t E, int64_t t, uint32_t (&k)[kPrItems + 1], u64 (&v)[kPrItems]) {
    const int64_t i0 = t * kPrTile + (int64_t)threadIdx.x * kPrItems;
#pragma unroll
    for (int a = 0; a <= kPrItems; ++a) k[a] = i0 + a < E ? keys[i0 + a] : 0u;
#pragma unroll
    for (int a = 0; a < kPrItems; ++a) v[a] = i0 + a < E ? pr_item(k[a], k[a + 1], i0 + a == E - 1) : 0ull;
}

__global__ void __launch_bounds__(kPrThreads) k_pr_reduce(const uint32_t* __restrict__ keys, int64_t E, u64* __restrict__ sums) {
    __shared__ u64 wave_s[kPrThreads / kWave];
    const int64_t tiles = pr_tiles(E);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t k[kPrItems + 1];
        u64 v[kPrItems], total;
        pr_load(keys, E, t, k, v);
        pr_block_scan(v[0] + v[1] + v[2] + v[3], wave_s, total);
        if (threadIdx.x == 0) sums[t] = total;
    }
}

// launched with ONE workgroup: sums[t] becomes the sum of the tiles before t; the grand total goes to the info words
__global__ void __launch_bounds__(kPrThreads) k_pr_sums(u64* __restrict__ sums, int64_t tiles, u64* __restrict__ info) {
    __shared__ u64 wave_s[kPrThreads / kWave];
    u64 carry = 0;
    for (int64_t c0 = 0; c0 < tiles; c0 += kPrTile) {
        const int64_t i0 = c0 + (int64_t)threadIdx.x * kPrItems;
        u64 v[kPrItems], total;
#pragma unroll
        for (int a = 0; a < kPrItems; ++a) v[a] = i0 + a < tiles ? sums[i0 + a] : 0ull;
        u64 run = carry + pr_block_scan(v[0] + v[1] + v[2] + v[3], wave_s, total);
#pragma unroll
        for (int a = 0; a < kPrItems; ++a) {
            if (i0 + a < tiles) sums[i0 + a] = run;
            run += v[a];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        info[kPrThresholds] = carry >> 32;
        info[kPrPositives] = carry & 0xFFFFFFFFull;
    }
}

__global__ void __launch_bounds__(kPrThreads) k_pr_emit(const uint32_t* __restrict__ keys, int64_t E, int64_t M, int64_t P,
                                                        const u64* __restrict__ sums, float* __restrict__ thresholds, int64_t* __restrict__ tp_out,
                                                        int64_t* __restrict__ fp_out, double* __restrict__ precision,
                                                        double* __restrict__ recall, int64_t* __restrict__ last) {
    __shared__ u64 wave_s[kPrThreads / kWave];
    const int64_t tiles = pr_tiles(E);
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the appended point
        if (precision) precision[M] = 1.0;
        if (recall) recall[M] = 0.0;
    }
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t k[kPrItems + 1];
        u64 v[kPrItems], total;
        pr_load(keys, E, t, k, v);
        u64 run = sums[t] + pr_block_scan(v[0] + v[1] + v[2] + v[3], wave_s, total);
        const int64_t i0 = t * kPrTile + (int64_t)threadIdx.x * kPrItems;
#pragma unroll
        for (int a = 0; a < kPrItems; ++a) {
            const int64_t j = (int64_t)(run >> 32);             // run ends before this position = the index of its run
            run += v[a];
            const int64_t i = i0 + a, tp = (int64_t)(run & 0xFFFFFFFFull);
            if (i >= E || j >= M) continue;                       // j < M always when M is what k_pr_sums counted
            if (last && (k[a] & 1u) && tp == P) last[0] = j;      // the last positive: its run is the first with tp = P
            if (!(v[a] >> 32)) continue;
            if (thresholds) thresholds[j] = __uint_as_float(k[a] >> 1);
            if (tp_out) tp_out[j] = tp;
            if (fp_out) fp_out[j] = 1 + i - tp;
            if (precision) precision[M - 1 - j] = (double)tp / (double)(1 + i);
            if (recall) recall[M - 1 - j] = (double)tp / (double)P;
        }
    }
}

// partials[t] = the sum of tile t's terms (recall[r+1] - recall[r]) * precision[r], r < M, in a fixed tree
__global__ void __launch_bounds__(kPrThreads) k_pr_ap_tiles(const double* __restrict__ precision, const double* __restrict__ recall, int64_t M,
                                                            double* __restrict__ partials) {
    __shared__ double r_s[kPrThreads];
    const int64_t tiles = pr_tiles(M);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * kPrTile + (int64_t)threadIdx.x * kPrItems;
        double term[kPrItems];
#pragma unroll
        for (int a = 0; a < kPrItems; ++a) {
            const int64_t r = r0 + a;
            term[a] = 0.0;
            if (r < M) {
                const double d = recall[r + 1] - recall[r];
                term[a] = d * precision[r];
            }
        }
        const double s = pr_block_tree((term[0] + term[1]) + (term[2] + term[3]), r_s);
        if (threadIdx.x == 0) partials[t] = s;
    }
}

// launched with ONE workgroup: thread i adds partials i, i + kPrThreads, ... in that order, then the fixed tree; ap = max(0, -sum)
__global__ void __launch_bounds__(kPrThreads) k_pr_ap_sum(const double* __restrict__ partials, int64_t tiles, double* __restrict__ ap) {
    __shared__ double r_s[kPrThreads];
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += kPrThreads) s += partials[t];
    s = pr_block_tree(s, r_s);
    if (threadIdx.x == 0) ap[0] = -s > 0.0 ? -s : 0.0;
}

static int pr_workspace(const char* what, int64_t E, void* workspace, size_t workspace_bytes, PrLayout& L) {
    GN_REQUIRE(E >= 1 && E < ((int64_t)1 << 31), "%s: num_edges=%lld outside [1, 2^31)", what, (long long)E);
    GN_REQUIRE(workspace, "%s: null workspace", what);
    L = pr_layout(E);
    if (workspace_bytes < L.total) {
        set_error("%s: workspace %zu < %zu bytes", what, workspace_bytes, L.total);
        return GNNOME_EWORKSPACE;
    }
    return GNNOME_OK;
}

}  // namespace gnnome

extern "C" int gnnome_pr_curve_tile_size(int* tile_host) {
    GN_REQUIRE(tile_host, "pr_curve_tile_size: null pointer");
    *tile_host = gnnome::kPrTile;
    return GNNOME_OK;
}

extern "C" int gnnome_pr_curve_workspace_bytes(int64_t num_edges, size_t* bytes_host) {
    GN_REQUIRE(num_edges >= 1 && num_edges < ((int64_t)1 << 31) && bytes_host, "pr_curve_workspace_bytes: bad argument (num_edges=%lld)",
               (long long)num_edges);
    *bytes_host = gnnome::pr_layout(num_edges).total;
    return GNNOME_OK;
}

extern "C" int gnnome_pr_curve_keys(const float* preds, const float* labels, int64_t num_edges, int apply_sigmoid, int inverse,
                                    uint32_t* keys, float* probs_out, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    PrLayout L;
    if (const int rc = pr_workspace("pr_curve_keys", num_edges, workspace, workspace_bytes, L)) return rc;
    GN_REQUIRE(preds && labels && keys, "pr_curve_keys: null pointer");
    u64* info = (u64*)((char*)workspace + L.info);
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(info, 0xFF, kPrWords * sizeof(u64), s));
    const int64_t blocks = (num_edges + kPrThreads - 1) / kPrThreads;
    hipLaunchKernelGGL(k_pr_keys, dim3((unsigned)(blocks < kNumCUs * 16 ? blocks : kNumCUs * 16)), dim3(kPrThreads), 0, s, preds, labels,
                       num_edges, apply_sigmoid, inverse, keys, probs_out, info);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_pr_curve_scan(const uint32_t* sorted_keys, int64_t num_edges, void* workspace, size_t workspace_bytes,
                                    int64_t* result_host, void* stream) {
    using namespace gnnome;
    PrLayout L;
    if (const int rc = pr_workspace("pr_curve_scan", num_edges, workspace, workspace_bytes, L)) return rc;
    GN_REQUIRE(sorted_keys && result_host, "pr_curve_scan: null pointer");
    u64* info = (u64*)((char*)workspace + L.info);
    u64* sums = (u64*)((char*)workspace + L.sums);
    hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = pr_tiles(num_edges);
    hipLaunchKernelGGL(k_pr_reduce, dim3(pr_grid(tiles)), dim3(kPrThreads), 0, s, sorted_keys, num_edges, sums);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pr_sums, dim3(1), dim3(kPrThreads), 0, s, sums, tiles, info);
    GN_LAUNCH_CHECK();
    u64 h[kPrWords];
    GN_HIP(hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    result_host[0] = (int64_t)h[kPrThresholds];
    result_host[1] = (int64_t)h[kPrPositives];
    result_host[2] = h[kPrBadPred] == ~0ull ? -1 : (int64_t)h[kPrBadPred];
    result_host[3] = h[kPrBadLabel] == ~0ull ? -1 : (int64_t)h[kPrBadLabel];
    return GNNOME_OK;
}

extern "C" int gnnome_pr_curve_emit(const uint32_t* sorted_keys, int64_t num_edges, int64_t num_thresholds, int64_t num_positives,
                                    float* thresholds, int64_t* tp, int64_t* fp, double* precision, double* recall, int64_t* last,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    PrLayout L;
    if (const int rc = pr_workspace("pr_curve_emit", num_edges, workspace, workspace_bytes, L)) return rc;
    GN_REQUIRE(sorted_keys, "pr_curve_emit: null pointer");
    GN_REQUIRE(num_thresholds >= 1 && num_thresholds <= num_edges && num_positives >= 1 && num_positives <= num_edges,
               "pr_curve_emit: %lld thresholds and %lld positives for %lld edges", (long long)num_thresholds, (long long)num_positives,
               (long long)num_edges);
    const u64* sums = (const u64*)((char*)workspace + L.sums);
    hipLaunchKernelGGL(k_pr_emit, dim3(pr_grid(pr_tiles(num_edges))), dim3(kPrThreads), 0, (hipStream_t)stream, sorted_keys, num_edges,
                       num_thresholds, num_positives, sums, thresholds, tp, fp, precision, recall, last);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_pr_curve_ap(const double* precision, const double* recall, int64_t num_thresholds, double* ap, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    PrLayout L;
    if (const int rc = pr_workspace("pr_curve_ap", num_thresholds, workspace, workspace_bytes, L)) return rc;
    GN_REQUIRE(precision && recall && ap, "pr_curve_ap: null pointer");
    double* partials = (double*)((char*)workspace + L.partials);
    hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = pr_tiles(num_thresholds);
    hipLaunchKernelGGL(k_pr_ap_tiles, dim3(pr_grid(tiles)), dim3(kPrThreads), 0, s, precision, recall, num_thresholds, partials);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pr_ap_sum, dim3(1), dim3(kPrThreads), 0, s, (const double*)partials, tiles, ap);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
