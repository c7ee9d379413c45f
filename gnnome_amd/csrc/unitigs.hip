// Unitig compaction: links, list ranking of the chains, the scatter of the chain members.  tests/unitig_statement.py states
// the rule; everything here is integer arithmetic, there are no atomics, and every slot of every table has one writer, so the bytes do
// not depend on the grid or on timing.
//
// gnnome_unitig_links   one lane per edge: (u, v) is a link iff out_deg[u] == 1, in_deg[v] == 1 and u >> 1 != v >> 1.  A link writes
//   succ[u], pred[v], weight[u] = p and succ_edge[u] = its id: out_deg[u] == 1 and in_deg[v] == 1 make it the only writer of each.
// gnnome_unitig_rank    pointer jumping towards the head.  A node's jump state is one 16-byte record (ancestor, hops, bases), so a jump
//   is one dwordx4 gather; the records are double-buffered, a round reads one buffer and writes the other.  The ancestor is stored
//   complemented (~a < 0) once it is a head: such a record is final, and a round only copies it.  Each launch does ONE jump per node - no
//   lane follows a chain - and leaves the number of unfinished nodes per workgroup; a one-workgroup launch adds them and the host reads
//   the sum.  On paths the sum falls strictly, a chain of n nodes is done after ceil(log2 n) rounds.  When it stops falling the rest
//   lie on cycles: the same doubling over 8-byte records (ancestor, smallest read so far) until the jump distance reaches the number of
//   leftover nodes gives every node its cycle's smallest read r; the node 2r (or the successor of 2r + 1) drops its predecessor, its
//   predecessor drops its successor and the link flag of that edge, each lane writing its own slots only; the leftover nodes start
//   again from the cut tables and are ranked by the same rounds.  A graph without cycles never launches the cycle kernels.
// gnnome_unitig_scatter chain_nodes[chain_off[unitig[v]] + rank[v]] = v, one lane per node, both indices checked.
// Every index that comes out of a table is compared with its bound before it is used.
#include "common.h"

namespace gnnome {

constexpr int kUtThreads = 256;
constexpr int kUtMaxGrid = kNumCUs * 16;
constexpr int kUtMaxRounds = 40;   // 2^31 nodes need 31

struct __attribute__((aligned(16))) UtRec {
    int32_t anc;      // >= 0: the node `hops` links back; < 0: ~anc is the head, the record is final
    uint32_t hops;
    int64_t bases;    // the summed p of those links
};
struct __attribute__((aligned(8))) UtMin {
    int32_t anc, read;
};

static unsigned ut_grid(int64_t n, int grid) {
    const int64_t blocks = (n + kUtThreads - 1) / kUtThreads;
    const int64_t cap = grid > 0 && grid < kUtMaxGrid ? grid : kUtMaxGrid;
    return (unsigned)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_links(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                             const int64_t* __restrict__ prefix, const int32_t* __restrict__ out_deg,
                                                             const int32_t* __restrict__ in_deg, int64_t N, int64_t E,
                                                             int32_t* __restrict__ succ, int32_t* __restrict__ pred,
                                                             int32_t* __restrict__ weight, int32_t* __restrict__ succ_edge,
                                                             uint8_t* __restrict__ link) {
    for (int64_t e = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; e < E; e += (int64_t)gridDim.x * kUtThreads) {
        const int64_t u = src[e], v = dst[e];
        bool is_link = false;
        if ((uint64_t)u < (uint64_t)N && (uint64_t)v < (uint64_t)N) is_link = out_deg[u] == 1 && in_deg[v] == 1 && (u >> 1) != (v >> 1);
        link[e] = is_link;
        if (is_link) {
            succ[u] = (int32_t)v;
            pred[v] = (int32_t)u;
            weight[u] = (int32_t)prefix[e];
            succ_edge[u] = (int32_t)e;
        }
    }
}

// the workgroup's count into block_count[blockIdx.x]
__device__ __forceinline__ void ut_block_count(int cnt, int32_t* __restrict__ block_count) {
    __shared__ int wave_cnt[kUtThreads / kWave];
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_cnt[threadIdx.x / kWave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < kUtThreads / kWave; ++w) sum += wave_cnt[w];
        block_count[blockIdx.x] = sum;
    }
}

__device__ __forceinline__ UtRec ut_start(int64_t v, const int32_t* __restrict__ pred, const int32_t* __restrict__ weight, int64_t N) {
    const int p1 = pred[v];
    if ((uint64_t)(int64_t)p1 >= (uint64_t)N) return UtRec{~(int32_t)v, 0u, 0};
    const int p2 = pred[p1];
    return UtRec{(uint64_t)(int64_t)p2 >= (uint64_t)N ? ~p1 : p1, 1u, (int64_t)weight[p1]};
}

// only_cycle: the nodes flagged in `cyc` start again, the others keep their record
__global__ void __launch_bounds__(kUtThreads) k_unitig_start(const int32_t* __restrict__ pred, const int32_t* __restrict__ weight, int64_t N,
                                                             const uint8_t* __restrict__ cyc, int only_cycle, UtRec* __restrict__ rec,
                                                             int32_t* __restrict__ block_count) {
    int cnt = 0;
    for (int64_t v = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kUtThreads) {
        if (only_cycle && !cyc[v]) continue;
        const UtRec r = ut_start(v, pred, weight, N);
        rec[v] = r;
        cnt += r.anc >= 0;
    }
    ut_block_count(cnt, block_count);
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_jump(const UtRec* __restrict__ in, UtRec* __restrict__ out, int64_t N,
                                                            int32_t* __restrict__ block_count) {
    int cnt = 0;
    for (int64_t v = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kUtThreads) {
        UtRec r = in[v];
        if (r.anc >= 0) {
            if ((int64_t)r.anc < N) {
                const UtRec a = in[r.anc];
                r.anc = a.anc;
                r.hops += a.hops;
                r.bases += a.bases;
            } else {
                r = UtRec{~(int32_t)v, 0u, 0};   // no table the host lets through gets here
            }
        }
        out[v] = r;
        cnt += r.anc >= 0;
    }
    ut_block_count(cnt, block_count);
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_sum(const int32_t* __restrict__ block_count, int blocks, int64_t* __restrict__ total) {
    __shared__ int64_t part[kUtThreads];
    int64_t sum = 0;
    for (int i = threadIdx.x; i < blocks; i += kUtThreads) sum += block_count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = kUtThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = part[0];
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_min_start(const UtRec* __restrict__ rec, const int32_t* __restrict__ pred, int64_t N,
                                                                 UtMin* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kUtThreads)
        if (rec[v].anc >= 0) out[v] = UtMin{pred[v], (int32_t)(v >> 1)};
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_min_jump(const UtRec* __restrict__ rec, const UtMin* __restrict__ in,
                                                                UtMin* __restrict__ out, int64_t N) {
    for (int64_t v = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kUtThreads) {
        if (rec[v].anc < 0) continue;
        UtMin m = in[v];
        if ((uint64_t)(int64_t)m.anc < (uint64_t)N) {   // a leftover node's ancestors are leftover nodes: their records exist
            const UtMin a = in[m.anc];
            m.anc = a.anc;
            m.read = a.read < m.read ? a.read : m.read;
        }
        out[v] = m;
    }
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_cut(const UtRec* __restrict__ rec, const UtMin* __restrict__ mins, int64_t N, int64_t E,
                                                           int32_t* __restrict__ succ, int32_t* __restrict__ pred,
                                                           const int32_t* __restrict__ succ_edge, uint8_t* __restrict__ link,
                                                           uint8_t* __restrict__ cyc) {
    for (int64_t v = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kUtThreads) {
        if (rec[v].anc < 0) continue;
        const int64_t start = 2 * (int64_t)mins[v].read, end = start + 1;   // the cycle holds one of the two
        cyc[v] = 1;
        if (v == start || pred[v] == end) pred[v] = -1;
        if (succ[v] == start || v == end) {
            succ[v] = -1;
            const int64_t e = succ_edge[v];
            if ((uint64_t)e < (uint64_t)E) link[e] = 0;
        }
    }
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_result(const UtRec* __restrict__ rec, int64_t N, int32_t* __restrict__ head,
                                                              int32_t* __restrict__ rank, int64_t* __restrict__ offset) {
    for (int64_t v = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kUtThreads) {
        const UtRec r = rec[v];
        const int h = ~r.anc;
        const bool ok = r.anc < 0 && (int64_t)h < N;
        head[v] = ok ? h : (int32_t)v;
        rank[v] = ok ? (int32_t)r.hops : 0;
        offset[v] = ok ? r.bases : 0;
    }
}

__global__ void __launch_bounds__(kUtThreads) k_unitig_scatter(const int32_t* __restrict__ unitig, const int32_t* __restrict__ rank,
                                                               const int64_t* __restrict__ chain_off, int64_t N, int64_t U,
                                                               int32_t* __restrict__ chain_nodes) {
    for (int64_t v = (int64_t)blockIdx.x * kUtThreads + threadIdx.x; v < N; v += (int64_t)gridDim.x * kUtThreads) {
        const int64_t j = unitig[v];
        if ((uint64_t)j >= (uint64_t)U) continue;
        const int64_t at = chain_off[j] + rank[v];
        if ((uint64_t)at < (uint64_t)N) chain_nodes[at] = (int32_t)v;
    }
}

struct UtLayout {
    size_t rec[2], mins[2], block_count, total, bytes;
};
static UtLayout ut_layout(int64_t N) {
    UtLayout L;
    size_t o = 0;
    const auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    for (int i = 0; i < 2; ++i) L.rec[i] = o, o = al(o + (size_t)N * sizeof(UtRec));
    for (int i = 0; i < 2; ++i) L.mins[i] = o, o = al(o + (size_t)N * sizeof(UtMin));
    L.block_count = o; o = al(o + (size_t)kUtMaxGrid * sizeof(int32_t));
    L.total = o;       o = al(o + sizeof(int64_t));
    L.bytes = o;
    return L;
}

}  // namespace gnnome

extern "C" int gnnome_unitig_links(const int64_t* src, const int64_t* dst, const int64_t* prefix, const int32_t* out_deg, const int32_t* in_deg,
                                   int64_t num_nodes, int64_t num_edges, int32_t* succ, int32_t* pred, int32_t* weight, int32_t* succ_edge,
                                   uint8_t* link, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes, E = num_edges;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && N % 2 == 0 && E >= 0 && E < ((int64_t)1 << 31),
               "unitig_links: num_nodes=%lld (even, below 2^31) num_edges=%lld (below 2^31)", (long long)N, (long long)E);
    if (N == 0) return GNNOME_OK;
    GN_REQUIRE(succ && pred && weight && succ_edge, "unitig_links: null pointer");
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(succ, 0xFF, (size_t)N * sizeof(int32_t), s));
    GN_HIP(hipMemsetAsync(pred, 0xFF, (size_t)N * sizeof(int32_t), s));
    GN_HIP(hipMemsetAsync(weight, 0, (size_t)N * sizeof(int32_t), s));
    GN_HIP(hipMemsetAsync(succ_edge, 0xFF, (size_t)N * sizeof(int32_t), s));
    if (E == 0) return GNNOME_OK;
    GN_REQUIRE(src && dst && prefix && out_deg && in_deg && link, "unitig_links: null pointer");
    hipLaunchKernelGGL(k_unitig_links, dim3(ut_grid(E, 0)), dim3(kUtThreads), 0, s, src, dst, prefix, out_deg, in_deg, N, E, succ, pred, weight,
                       succ_edge, link);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_unitig_rank_workspace_bytes(int64_t num_nodes, size_t* bytes_host) {
    GN_REQUIRE(num_nodes >= 0 && num_nodes < ((int64_t)1 << 31) && bytes_host, "unitig_rank_workspace_bytes: bad argument (num_nodes=%lld)",
               (long long)num_nodes);
    *bytes_host = gnnome::ut_layout(num_nodes).bytes;
    return GNNOME_OK;
}

extern "C" int gnnome_unitig_rank(int32_t* succ, int32_t* pred, const int32_t* weight, const int32_t* succ_edge, int64_t num_nodes,
                                  int64_t num_edges, uint8_t* link, uint8_t* cyc, int32_t* head, int32_t* rank, int64_t* offset, int grid,
                                  int64_t* rounds_host, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes, E = num_edges;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && N % 2 == 0 && E >= 0 && E < ((int64_t)1 << 31) && grid >= 0,
               "unitig_rank: num_nodes=%lld (even, below 2^31) num_edges=%lld (below 2^31) grid=%d", (long long)N, (long long)E, grid);
    if (rounds_host) rounds_host[0] = rounds_host[1] = rounds_host[2] = rounds_host[3] = 0;
    if (N == 0) return GNNOME_OK;
    GN_REQUIRE(succ && pred && weight && succ_edge && cyc && head && rank && offset && workspace && (link || E == 0), "unitig_rank: null pointer");
    const UtLayout L = ut_layout(N);
    if (workspace_bytes < L.bytes) {
        set_error("unitig_rank: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
        return GNNOME_EWORKSPACE;
    }
    char* const ws = (char*)workspace;
    UtRec* rec[2] = {(UtRec*)(ws + L.rec[0]), (UtRec*)(ws + L.rec[1])};
    UtMin* mins[2] = {(UtMin*)(ws + L.mins[0]), (UtMin*)(ws + L.mins[1])};
    int32_t* const block_count = (int32_t*)(ws + L.block_count);
    int64_t* const total = (int64_t*)(ws + L.total);
    hipStream_t s = (hipStream_t)stream;
    const dim3 g(ut_grid(N, grid)), b(kUtThreads);
    int64_t left = 0;
    const auto read_count = [&]() -> int {
        hipLaunchKernelGGL(k_unitig_sum, dim3(1), b, 0, s, (const int32_t*)block_count, (int)g.x, total);
        GN_LAUNCH_CHECK();
        GN_HIP(hipMemcpyAsync(&left, total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        return GNNOME_OK;
    };
    int cur = 0;
    // rounds while the count falls -> GNNOME_OK with left == 0, or with left > 0 where it stopped falling
    const auto rank_rounds = [&](int64_t* rounds) -> int {
        while (left > 0) {
            if (*rounds >= kUtMaxRounds) break;
            const int64_t before = left;
            hipLaunchKernelGGL(k_unitig_jump, g, b, 0, s, (const UtRec*)rec[cur], rec[cur ^ 1], N, block_count);
            GN_LAUNCH_CHECK();
            cur ^= 1;
            ++*rounds;
            const int rc = read_count();
            if (rc != GNNOME_OK) return rc;
            if (left >= before) break;
        }
        return GNNOME_OK;
    };
    GN_HIP(hipMemsetAsync(cyc, 0, (size_t)N, s));
    hipLaunchKernelGGL(k_unitig_start, g, b, 0, s, (const int32_t*)pred, weight, N, (const uint8_t*)cyc, 0, rec[cur], block_count);
    GN_LAUNCH_CHECK();
    int rc = read_count();
    if (rc != GNNOME_OK) return rc;
    int64_t rounds[4] = {0, 0, 0, 0};   // path rounds, minimum rounds, rounds after the cut, nodes on cycles
    rc = rank_rounds(&rounds[0]);
    if (rc != GNNOME_OK) return rc;
    if (left > 0) {
        // what is left lies on cycles: every node's window of 2^k predecessors covers its cycle once 2^k >= left
        rounds[3] = left;
        int mc = 0;
        hipLaunchKernelGGL(k_unitig_min_start, g, b, 0, s, (const UtRec*)rec[cur], (const int32_t*)pred, N, mins[mc]);
        GN_LAUNCH_CHECK();
        for (int64_t dist = 1; dist < left; dist *= 2) {
            hipLaunchKernelGGL(k_unitig_min_jump, g, b, 0, s, (const UtRec*)rec[cur], (const UtMin*)mins[mc], mins[mc ^ 1], N);
            GN_LAUNCH_CHECK();
            mc ^= 1;
            ++rounds[1];
        }
        hipLaunchKernelGGL(k_unitig_cut, g, b, 0, s, (const UtRec*)rec[cur], (const UtMin*)mins[mc], N, E, succ, pred, succ_edge, link, cyc);
        GN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_unitig_start, g, b, 0, s, (const int32_t*)pred, weight, N, (const uint8_t*)cyc, 1, rec[cur], block_count);
        GN_LAUNCH_CHECK();
        rc = read_count();
        if (rc != GNNOME_OK) return rc;
        rc = rank_rounds(&rounds[2]);
        if (rc != GNNOME_OK) return rc;
        GN_REQUIRE(left == 0, "unitig_rank: %lld nodes are still without a head after the cut: succ and pred are not each other's inverse",
                   (long long)left);
    }
    hipLaunchKernelGGL(k_unitig_result, g, b, 0, s, (const UtRec*)rec[cur], N, head, rank, offset);
    GN_LAUNCH_CHECK();
    if (rounds_host)
        for (int i = 0; i < 4; ++i) rounds_host[i] = rounds[i];
    return GNNOME_OK;
}

extern "C" int gnnome_unitig_scatter(const int32_t* unitig, const int32_t* rank, const int64_t* chain_off, int64_t num_nodes,
                                     int64_t num_unitigs, int32_t* chain_nodes, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes, U = num_unitigs;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && U >= 0 && U <= N, "unitig_scatter: num_nodes=%lld (below 2^31) num_unitigs=%lld (at most that)",
               (long long)N, (long long)U);
    if (N == 0) return GNNOME_OK;
    GN_REQUIRE(unitig && rank && chain_off && chain_nodes, "unitig_scatter: null pointer");
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(chain_nodes, 0xFF, (size_t)N * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_unitig_scatter, dim3(ut_grid(N, 0)), dim3(kUtThreads), 0, s, unitig, rank, chain_off, N, U, chain_nodes);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
