// Simple bubbles of the overlap graph: arm records, the judgement per source node, the node mark.  tests/bubble_statement.py
// states the rule; everything here is integer arithmetic, there are no atomics, every decision reads only the round's input and every slot
// has one writer (or every writer stores the same 1), so the bytes do not depend on the grid or on timing.  No lane walks along an arm:
// the chains, their heads, tails and lengths come from the ranking of unitigs.hip, the per-chain sums from prefix sums over chain_nodes.
//
// gnnome_bubble_arms   two launches.  One lane per edge: the edge is the in-edge of its target where that has in-degree 1 and the out-edge
//   of its source where that has out-degree 1 (one writer per slot).  Then one lane per chain: not circular, head of in-degree 1, tail of
//   out-degree 1, the in-edge from a node s of out-degree >= 2, the out-edge to a node t of in-degree >= 2, t != s, t != s ^ 1 make it an
//   arm; its 40-byte record holds s, t, the key node min(a_1, a_k ^ 1), the node count, weight, overlap and dist.  A chain that is no arm
//   has s = -1.
// gnnome_bubble_judge  one wavefront per source node v of out-degree >= 2.  An out-edge (v, x) leads into an arm iff the record of x's
//   chain names v as its source and x is that chain's head; parallel edges make x a join, so an arm is met once in the row.  The row is
//   staged in the wave's own LDS kBbTile entries at a time, already resolved through unitig[] and the records to (t, key, weight, overlap,
//   dist) planes; the lanes each hold one arm of the row and run over the staged entries wave-uniformly (every lane reads the same LDS
//   address: a broadcast), counting the arms of their t and keeping the best of them.  A row longer than 64 is done in passes of 64 arms, a
//   row longer than the tile tile by tile within each pass: a hub is slower and stays correct.  loser[chain] = 1 for an arm that is not
//   the best of >= 2 and meets the three distance bounds.
// gnnome_bubble_mark   one lane per node: mark[v] = loser[unitig[v]] | loser[unitig[v ^ 1]].
// Every index that comes out of a table is compared with its bound before it is used.
#include "common.h"

namespace gnnome {

constexpr int kBbThreads = 256;
constexpr int kBbWaves = kBbThreads / kWave;
constexpr int kBbTile = 128;   // row entries per LDS tile and wave: 2 planes x 512 B + 3 planes x 1 KiB
constexpr int kBbMaxGrid = kNumCUs * 16;

struct __attribute__((aligned(8))) BbArm {
    int32_t s, t;        // s < 0: the chain is no arm
    int32_t key, nodes;  // min(a_1, a_k ^ 1); k
    int64_t weight, overlap, dist;
};
static_assert(sizeof(BbArm) == 40, "the record the Python side reads");

static unsigned bb_grid(int64_t blocks, int grid) {
    const int64_t cap = grid > 0 && grid < kBbMaxGrid ? grid : kBbMaxGrid;
    return (unsigned)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

__global__ void __launch_bounds__(kBbThreads) k_bubble_edges(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                             const int32_t* __restrict__ in_deg, const int32_t* __restrict__ out_deg,
                                                             int64_t N, int64_t E, int32_t* __restrict__ in_edge,
                                                             int32_t* __restrict__ out_edge) {
    for (int64_t e = (int64_t)blockIdx.x * kBbThreads + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBbThreads) {
        const int64_t u = src[e], v = dst[e];
        if ((uint64_t)u >= (uint64_t)N || (uint64_t)v >= (uint64_t)N) continue;
        if (out_deg[u] == 1) out_edge[u] = (int32_t)e;
        if (in_deg[v] == 1) in_edge[v] = (int32_t)e;
    }
}

__global__ void __launch_bounds__(kBbThreads) k_bubble_arms(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                            const int64_t* __restrict__ overlap, const int32_t* __restrict__ in_deg,
                                                            const int32_t* __restrict__ out_deg, int64_t N, int64_t E,
                                                            const int64_t* __restrict__ chain_off, const int32_t* __restrict__ chain_nodes,
                                                            const uint8_t* __restrict__ circular, const int64_t* __restrict__ length,
                                                            const int64_t* __restrict__ cum_weight, const int64_t* __restrict__ cum_length,
                                                            int64_t U, const int32_t* __restrict__ in_edge,
                                                            const int32_t* __restrict__ out_edge, BbArm* __restrict__ arms) {
    for (int64_t j = (int64_t)blockIdx.x * kBbThreads + threadIdx.x; j < U; j += (int64_t)gridDim.x * kBbThreads) {
        BbArm r{-1, -1, -1, 0, 0, 0, 0};
        const int64_t a = chain_off[j], b = chain_off[j + 1];
        if (a >= 0 && a < b && b <= N && !circular[j]) {
            const int64_t first = chain_nodes[a], last = chain_nodes[b - 1];
            if ((uint64_t)first < (uint64_t)N && (uint64_t)last < (uint64_t)N && in_deg[first] == 1 && out_deg[last] == 1) {
                const int64_t e_in = in_edge[first], e_out = out_edge[last];
                if ((uint64_t)e_in < (uint64_t)E && (uint64_t)e_out < (uint64_t)E) {
                    const int64_t s = src[e_in], t = dst[e_out];
                    if ((uint64_t)s < (uint64_t)N && (uint64_t)t < (uint64_t)N && out_deg[s] >= 2 && in_deg[t] >= 2 && t != s && t != (s ^ 1)) {
                        const int64_t ends = overlap[e_in] + overlap[e_out];
                        const int64_t mate = last ^ 1;
                        r.s = (int32_t)s;
                        r.t = (int32_t)t;
                        r.key = (int32_t)(first < mate ? first : mate);
                        r.nodes = (int32_t)(b - a);
                        r.weight = cum_weight[b] - cum_weight[a];
                        r.dist = length[j] - ends;                                      // the summed read lengths less all k + 1 overlaps
                        r.overlap = cum_length[b] - cum_length[a] - r.dist;
                    }
                }
            }
        }
        arms[j] = r;
    }
}

// the arm that the row entry at position i of the (src, dst)-sorted edges leads into from v -> its chain, or -1
__device__ __forceinline__ int64_t bb_arm_of(int64_t i, int v, const int32_t* __restrict__ s_dst, const int32_t* __restrict__ unitig,
                                             const int32_t* __restrict__ rank, const BbArm* __restrict__ arms, int64_t N, int64_t U,
                                             BbArm* out) {
    const int64_t x = s_dst[i];
    if ((uint64_t)x >= (uint64_t)N || rank[x] != 0) return -1;
    const int64_t j = unitig[x];
    if ((uint64_t)j >= (uint64_t)U) return -1;
    const BbArm a = arms[j];
    if (a.s != v || (uint64_t)(int64_t)a.t >= (uint64_t)N) return -1;
    *out = a;
    return j;
}

__device__ __forceinline__ bool bb_better(int64_t w, int64_t o, int key, int64_t bw, int64_t bo, int bkey) {
    return w > bw || (w == bw && (o > bo || (o == bo && key < bkey)));
}

__global__ void __launch_bounds__(kBbThreads) k_bubble_judge(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ s_dst,
                                                             const int32_t* __restrict__ unitig, const int32_t* __restrict__ rank,
                                                             const BbArm* __restrict__ arms, int64_t N, int64_t E, int64_t U,
                                                             int64_t max_dist, int64_t max_diff, uint8_t* __restrict__ loser) {
    __shared__ int32_t t_s[kBbWaves][kBbTile], key_s[kBbWaves][kBbTile];
    __shared__ int64_t w_s[kBbWaves][kBbTile], o_s[kBbWaves][kBbTile], d_s[kBbWaves][kBbTile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int32_t* const ts = t_s[wave];
    int32_t* const keys = key_s[wave];
    int64_t* const ws = w_s[wave];
    int64_t* const os = o_s[wave];
    int64_t* const ds = d_s[wave];
    const int64_t first = (int64_t)blockIdx.x * kBbWaves + wave, step = (int64_t)gridDim.x * kBbWaves;
    for (int64_t v64 = first; v64 < N; v64 += step) {
        const int v = __builtin_amdgcn_readfirstlane((int)v64);   // N < 2^31
        const int64_t rs = row_ptr[v], re = row_ptr[v + 1];
        if (rs < 0 || re > E || re - rs < 2) continue;            // a bubble has two arms
        const bool one_tile = re - rs <= kBbTile;
        for (int64_t c0 = rs; c0 < re; c0 += kWave) {
            // this pass's arms, one per lane
            BbArm mine{-1, -1, -1, 0, 0, 0, 0};
            const int64_t my = c0 + lane < re ? bb_arm_of(c0 + lane, v, s_dst, unitig, rank, arms, N, U, &mine) : -1;
            int count = 0;
            int64_t bw = mine.weight, bo = mine.overlap, bd = mine.dist;
            int bkey = mine.key;
            for (int64_t t0 = rs; t0 < re; t0 += kBbTile) {
                const int n = re - t0 < kBbTile ? (int)(re - t0) : kBbTile;
                if (!(one_tile && c0 > rs)) {                     // a row of one tile is staged once
                    __builtin_amdgcn_wave_barrier();              // the tile is this wave's own: LDS keeps a wave's accesses in order
                    for (int i = lane; i < n; i += kWave) {
                        BbArm a{-1, -1, -1, 0, 0, 0, 0};
                        const bool arm = bb_arm_of(t0 + i, v, s_dst, unitig, rank, arms, N, U, &a) >= 0;
                        ts[i] = arm ? a.t : -1;
                        keys[i] = a.key;
                        ws[i] = a.weight;
                        os[i] = a.overlap;
                        ds[i] = a.dist;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                if (my >= 0) {
                    for (int i = 0; i < n; ++i) {
                        if (ts[i] != mine.t) continue;
                        ++count;
                        if (bb_better(ws[i], os[i], keys[i], bw, bo, bkey)) bw = ws[i], bo = os[i], bkey = keys[i], bd = ds[i];
                    }
                }
            }
            if (my >= 0 && count >= 2 && bkey != mine.key) {
                int64_t diff = mine.dist - bd;
                diff = diff < 0 ? -diff : diff;
                if (bd <= max_dist && mine.dist <= max_dist && diff <= max_diff) loser[my] = 1;
            }
        }
    }
}

__global__ void __launch_bounds__(kBbThreads) k_bubble_mark(const int32_t* __restrict__ unitig, const uint8_t* __restrict__ loser, int64_t N,
                                                            int64_t U, uint8_t* __restrict__ mark) {
    for (int64_t v = (int64_t)blockIdx.x * kBbThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kBbThreads) {
        const int64_t a = unitig[v], b = unitig[v ^ 1];           // N is even
        mark[v] = ((uint64_t)a < (uint64_t)U && loser[a]) || ((uint64_t)b < (uint64_t)U && loser[b]);
    }
}

}  // namespace gnnome

extern "C" int gnnome_bubble_tile_size(int* tile_host) {
    GN_REQUIRE(tile_host, "bubble_tile_size: null pointer");
    *tile_host = gnnome::kBbTile;
    return GNNOME_OK;
}

extern "C" int gnnome_bubble_arms(const int64_t* src, const int64_t* dst, const int64_t* overlap, const int32_t* in_deg, const int32_t* out_deg,
                                  int64_t num_nodes, int64_t num_edges, const int64_t* chain_off, const int32_t* chain_nodes,
                                  const uint8_t* circular, const int64_t* length, const int64_t* cum_weight, const int64_t* cum_length,
                                  int64_t num_unitigs, int32_t* in_edge, int32_t* out_edge, void* arms, int grid, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes, E = num_edges, U = num_unitigs;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && N % 2 == 0 && E >= 0 && E < ((int64_t)1 << 31) && U >= 0 && U <= N && grid >= 0,
               "bubble_arms: num_nodes=%lld (even, below 2^31) num_edges=%lld (below 2^31) num_unitigs=%lld (at most num_nodes) grid=%d",
               (long long)N, (long long)E, (long long)U, grid);
    if (N == 0 || U == 0) return GNNOME_OK;
    GN_REQUIRE(in_deg && out_deg && chain_off && chain_nodes && circular && length && cum_weight && cum_length && in_edge && out_edge && arms &&
                   ((src && dst && overlap) || E == 0), "bubble_arms: null pointer");
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(in_edge, 0xFF, (size_t)N * sizeof(int32_t), s));
    GN_HIP(hipMemsetAsync(out_edge, 0xFF, (size_t)N * sizeof(int32_t), s));
    if (E) {
        hipLaunchKernelGGL(k_bubble_edges, dim3(bb_grid((E + kBbThreads - 1) / kBbThreads, grid)), dim3(kBbThreads), 0, s, src, dst, in_deg,
                           out_deg, N, E, in_edge, out_edge);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_bubble_arms, dim3(bb_grid((U + kBbThreads - 1) / kBbThreads, grid)), dim3(kBbThreads), 0, s, src, dst, overlap, in_deg,
                       out_deg, N, E, chain_off, chain_nodes, circular, length, cum_weight, cum_length, U, (const int32_t*)in_edge,
                       (const int32_t*)out_edge, (BbArm*)arms);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_bubble_judge(const int64_t* row_ptr, const int32_t* dst, const int32_t* unitig, const int32_t* rank, const void* arms,
                                   int64_t num_nodes, int64_t num_edges, int64_t num_unitigs, int64_t max_dist, int64_t max_diff,
                                   uint8_t* loser, int grid, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes, E = num_edges, U = num_unitigs;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && E >= 0 && E < ((int64_t)1 << 31) && U >= 0 && U <= N && max_diff >= 0 && grid >= 0,
               "bubble_judge: num_nodes=%lld num_edges=%lld (below 2^31) num_unitigs=%lld (at most num_nodes) max_diff=%lld (>= 0) grid=%d",
               (long long)N, (long long)E, (long long)U, (long long)max_diff, grid);
    if (U == 0) return GNNOME_OK;
    GN_REQUIRE(loser, "bubble_judge: null pointer");
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(loser, 0, (size_t)U, s));
    if (E < 2) return GNNOME_OK;
    GN_REQUIRE(row_ptr && dst && unitig && rank && arms, "bubble_judge: null pointer");
    hipLaunchKernelGGL(k_bubble_judge, dim3(bb_grid((N + kBbWaves - 1) / kBbWaves, grid)), dim3(kBbThreads), 0, s, row_ptr, dst, unitig, rank,
                       (const BbArm*)arms, N, E, U, max_dist, max_diff, loser);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_bubble_mark(const int32_t* unitig, const uint8_t* loser, int64_t num_nodes, int64_t num_unitigs, uint8_t* mark, int grid,
                                  void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes, U = num_unitigs;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && N % 2 == 0 && U >= 0 && U <= N && grid >= 0,
               "bubble_mark: num_nodes=%lld (even, below 2^31) num_unitigs=%lld (at most num_nodes) grid=%d", (long long)N, (long long)U, grid);
    if (N == 0) return GNNOME_OK;
    GN_REQUIRE(unitig && loser && mark, "bubble_mark: null pointer");
    hipLaunchKernelGGL(k_bubble_mark, dim3(bb_grid((N + kBbThreads - 1) / kBbThreads, grid)), dim3(kBbThreads), 0, (hipStream_t)stream, unitig,
                       loser, N, U, mark);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
