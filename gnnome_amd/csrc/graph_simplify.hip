// Overlap-graph simplification: transitive edges and tips.  tests/graph_simplify_statement.py states both rules; everything
// here is integer arithmetic, there are no atomics, every decision reads only the input graph and every flag that is stored is 1, so the
// bytes do not depend on the grid or on timing.
//
// gnnome_transitive_edges   the rule is simultaneous (raven's, not Myers' sequential marking): edge e = (v, x) is transitive iff some
//   w != v, w != x has edges e1 = (v, w), e2 = (w, x) with |p(e1) + p(e2) - p(e)| <= fuzz.  One wavefront per source node v.  The edges
//   arrive sorted by (src, dst); a tile of kTrTile entries of out(v) is staged in the wave's own LDS as three planes (dst, p, edge id - a
//   binary search touches the dst plane only).  e1 runs over ALL of out(v), wave-uniformly; the lanes run over out(w), and each looks
//   its x' up in the staged tile by binary search (lower bound, then the run of equal dst: parallel edges are separate edges).  A hit
//   within fuzz stores 1 into mark[edge id] with a plain byte store; several lanes may store the same 1.  A row longer than the tile is
//   done tile by tile, the two-hop pairs being walked again for each: a hub is slower and stays correct.
// gnnome_tip_nodes          two launches, one lane per node, loops bounded by max_tip.  The first follows the chain from every tip start
//   (in-degree 0, out-degree 1) and leaves per start the junction (or -1), the summed p and the last chain node; the last node of a
//   candidate also gets its start (a chain node has in-degree <= 1, so it lies on one chain: one writer).  The second looks, per
//   candidate, at the in-edges of its junction: an in-edge that does not come from a candidate's last node makes every candidate there
//   a tip, otherwise all but the heaviest (ties: the smallest last node) are; a tip's lane walks its chain again and flags the nodes and
//   their complements.
#include "common.h"

namespace gnnome {

constexpr int kTrThreads = 256;
constexpr int kTrWaves = kTrThreads / kWave;
constexpr int kTrTile = 256;   // entries of out(v) per LDS tile and wave: 3 planes x 1 KiB

static unsigned gs_grid(int64_t blocks) { return (unsigned)(blocks < 1 ? 1 : blocks < kNumCUs * 16 ? blocks : kNumCUs * 16); }

__global__ void __launch_bounds__(kTrThreads) k_transitive(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ s_dst,
                                                           const int32_t* __restrict__ s_p, const int32_t* __restrict__ s_eid, int64_t N,
                                                           int64_t E, int64_t fuzz, uint8_t* __restrict__ mark) {
    __shared__ int32_t dst_s[kTrWaves][kTrTile], p_s[kTrWaves][kTrTile], eid_s[kTrWaves][kTrTile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int32_t* const dsts = dst_s[wave];
    int32_t* const ps = p_s[wave];
    int32_t* const eids = eid_s[wave];
    const int64_t first = (int64_t)blockIdx.x * kTrWaves + wave, step = (int64_t)gridDim.x * kTrWaves;
    for (int64_t v64 = first; v64 < N; v64 += step) {
        const int v = __builtin_amdgcn_readfirstlane((int)v64);   // N < 2^31
        const int64_t rs = row_ptr[v], re = row_ptr[v + 1];
        if (re - rs < 2) continue;   // e and e1 are two different out-edges of v
        for (int64_t t0 = rs; t0 < re; t0 += kTrTile) {
            const int n = re - t0 < kTrTile ? (int)(re - t0) : kTrTile;
            __builtin_amdgcn_wave_barrier();   // the tile is this wave's own: LDS keeps a wave's accesses in order
            for (int i = lane; i < n; i += kWave) {
                dsts[i] = s_dst[t0 + i];
                ps[i] = s_p[t0 + i];
                eids[i] = s_eid[t0 + i];
            }
            __builtin_amdgcn_wave_barrier();
            for (int64_t i = rs; i < re; ++i) {
                const int w = s_dst[i];
                if (w == v || (unsigned)w >= (uint64_t)N) continue;
                const int64_t p1 = s_p[i], ws = row_ptr[w], we = row_ptr[w + 1];
                for (int64_t j = ws + lane; j < we; j += kWave) {
                    const int x = s_dst[j];
                    if (x == w) continue;
                    const int64_t p12 = p1 + s_p[j];
                    int lo = 0, hi = n;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (dsts[mid] < x) lo = mid + 1; else hi = mid;
                    }
                    for (; lo < n && dsts[lo] == x; ++lo) {
                        int64_t d = p12 - ps[lo];
                        d = d < 0 ? -d : d;
                        const int64_t e = eids[lo];
                        if (d <= fuzz && (uint64_t)e < (uint64_t)E) mark[e] = 1;
                    }
                }
            }
        }
    }
}

constexpr int kTipThreads = 256;

__global__ void __launch_bounds__(kTipThreads) k_tip_chains(const int32_t* __restrict__ in_deg, const int32_t* __restrict__ out_deg,
                                                            const int32_t* __restrict__ succ, const int32_t* __restrict__ succ_p, int64_t N,
                                                            int max_tip, int32_t* __restrict__ cand_j, int64_t* __restrict__ cand_sum,
                                                            int32_t* __restrict__ cand_last, int32_t* __restrict__ last_start) {
    for (int64_t s = (int64_t)blockIdx.x * kTipThreads + threadIdx.x; s < N; s += (int64_t)gridDim.x * kTipThreads) {
        int j = -1, last = -1;
        int64_t sum = 0;
        if (in_deg[s] == 0 && out_deg[s] == 1) {
            int c = (int)s;
            for (int m = 1; m <= max_tip; ++m) {
                const int nxt = succ[c];
                if ((unsigned)nxt >= (uint64_t)N) break;
                sum += succ_p[c];
                if (in_deg[nxt] >= 2) {
                    j = nxt;
                    last = c;
                    break;
                }
                if (out_deg[nxt] != 1) break;
                c = nxt;
            }
        }
        cand_j[s] = j;
        cand_sum[s] = sum;
        cand_last[s] = last;
        if (j >= 0) last_start[last] = (int32_t)s;
    }
}

__global__ void __launch_bounds__(kTipThreads) k_tip_resolve(const int64_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src,
                                                             const int32_t* __restrict__ succ, int64_t N, int max_tip,
                                                             const int32_t* __restrict__ cand_j, const int64_t* __restrict__ cand_sum,
                                                             const int32_t* __restrict__ cand_last, const int32_t* __restrict__ last_start,
                                                             uint8_t* __restrict__ tip) {
    for (int64_t s = (int64_t)blockIdx.x * kTipThreads + threadIdx.x; s < N; s += (int64_t)gridDim.x * kTipThreads) {
        const int j = cand_j[s];
        if (j < 0) continue;
        const int mine = cand_last[s];
        bool all = true;
        int best_last = -1;
        int64_t best_sum = 0;
        for (int64_t q = in_ptr[j]; q < in_ptr[j + 1]; ++q) {
            const int u = in_src[q];
            const int t = (unsigned)u < (uint64_t)N ? last_start[u] : -1;
            if (t < 0 || cand_j[t] != j) {
                all = false;
                break;
            }
            const int64_t sm = cand_sum[t];
            if (best_last < 0 || sm > best_sum || (sm == best_sum && u < best_last)) best_sum = sm, best_last = u;
        }
        if (all && best_last == mine) continue;   // the survivor
        int c = (int)s;
        for (int m = 1; m <= max_tip; ++m) {
            tip[c] = 1;
            tip[c ^ 1] = 1;   // N is even
            if (c == mine) break;
            c = succ[c];
            if ((unsigned)c >= (uint64_t)N) break;
        }
    }
}

struct TipLayout {
    size_t cand_sum, cand_j, cand_last, last_start, total;
};
static TipLayout tip_layout(int64_t N) {
    TipLayout L;
    size_t o = 0;
    const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    L.cand_sum = o;   o = al(o + (size_t)N * sizeof(int64_t));
    L.cand_j = o;     o = al(o + (size_t)N * sizeof(int32_t));
    L.cand_last = o;  o = al(o + (size_t)N * sizeof(int32_t));
    L.last_start = o; o = al(o + (size_t)N * sizeof(int32_t));
    L.total = o;
    return L;
}

}  // namespace gnnome

extern "C" int gnnome_transitive_tile_size(int* tile_host) {
    GN_REQUIRE(tile_host, "transitive_tile_size: null pointer");
    *tile_host = gnnome::kTrTile;
    return GNNOME_OK;
}

extern "C" int gnnome_transitive_edges(const int64_t* row_ptr, const int32_t* dst, const int32_t* prefix, const int32_t* edge_id,
                                       int64_t num_nodes, int64_t num_edges, int fuzz, uint8_t* mark, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes >= 0 && num_nodes < ((int64_t)1 << 31) && num_edges >= 0 && num_edges < ((int64_t)1 << 31) && fuzz >= 0,
               "transitive_edges: num_nodes=%lld num_edges=%lld fuzz=%d out of range", (long long)num_nodes, (long long)num_edges, fuzz);
    if (num_edges == 0) return GNNOME_OK;
    GN_REQUIRE(row_ptr && dst && prefix && edge_id && mark, "transitive_edges: null pointer");
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(mark, 0, (size_t)num_edges, s));
    hipLaunchKernelGGL(k_transitive, dim3(gs_grid((num_nodes + kTrWaves - 1) / kTrWaves)), dim3(kTrThreads), 0, s, row_ptr, dst, prefix, edge_id,
                       num_nodes, num_edges, (int64_t)fuzz, mark);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_tip_nodes_workspace_bytes(int64_t num_nodes, size_t* bytes_host) {
    GN_REQUIRE(num_nodes >= 0 && num_nodes < ((int64_t)1 << 31) && bytes_host, "tip_nodes_workspace_bytes: bad argument (num_nodes=%lld)",
               (long long)num_nodes);
    *bytes_host = gnnome::tip_layout(num_nodes).total;
    return GNNOME_OK;
}

extern "C" int gnnome_tip_nodes(const int32_t* in_deg, const int32_t* out_deg, const int32_t* succ, const int32_t* succ_prefix,
                                const int64_t* in_ptr, const int32_t* in_src, int64_t num_nodes, int max_tip, uint8_t* tip, void* workspace,
                                size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && N % 2 == 0 && max_tip >= 1, "tip_nodes: num_nodes=%lld (even, below 2^31) max_tip=%d (>= 1)",
               (long long)N, max_tip);
    if (N == 0) return GNNOME_OK;
    GN_REQUIRE(in_deg && out_deg && succ && succ_prefix && in_ptr && in_src && tip && workspace, "tip_nodes: null pointer");
    const TipLayout L = tip_layout(N);
    if (workspace_bytes < L.total) {
        set_error("tip_nodes: workspace %zu < %zu bytes", workspace_bytes, L.total);
        return GNNOME_EWORKSPACE;
    }
    int64_t* cand_sum = (int64_t*)((char*)workspace + L.cand_sum);
    int32_t* cand_j = (int32_t*)((char*)workspace + L.cand_j);
    int32_t* cand_last = (int32_t*)((char*)workspace + L.cand_last);
    int32_t* last_start = (int32_t*)((char*)workspace + L.last_start);
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(tip, 0, (size_t)N, s));
    GN_HIP(hipMemsetAsync(last_start, 0xFF, (size_t)N * sizeof(int32_t), s));
    const dim3 grid(gs_grid((N + kTipThreads - 1) / kTipThreads)), block(kTipThreads);
    hipLaunchKernelGGL(k_tip_chains, grid, block, 0, s, in_deg, out_deg, succ, succ_prefix, N, max_tip, cand_j, cand_sum, cand_last, last_start);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tip_resolve, grid, block, 0, s, in_ptr, in_src, (const int32_t*)succ, N, max_tip, (const int32_t*)cand_j,
                       (const int64_t*)cand_sum, (const int32_t*)cand_last, (const int32_t*)last_start, tip);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
