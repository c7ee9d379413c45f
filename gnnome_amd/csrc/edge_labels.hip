// Ground-truth edge labels from read positions (utils/labels.py: create_correct_graphs[_combo], get_gt_for_single_strand,
// process_graph[_combo]; called from graph_parser.py:387-400 when training=True).
//
// An edge (u, v) is a class edge of problem (c, s) when chr[u] == chr[v] == c, strand[u] == strand[v] == s and, for s = +1,
// start[u] < start[v] < end[u] (for s = -1: start[v] < start[u] < end[v]).  Each problem's class edges are labelled by the
// reference's component loop, restated with one key per node, hk = end (s = +1) or ~start = -start - 1 (s = -1):
//   final = argmax_V hk;  reached = min_V hk;  alive = V
//   while alive:  a = first alive node in cursor order (start ascending for +1, end descending for -1)
//                 F = reachable from a in G[alive];  h = argmax_F hk;  C = nodes that reach h in G[F]
//                 if |C| >= 2 and hk[h] >= reached: reached = hk[h], the class edges inside C are labelled 1, stop if h == final
//                 alive -= F
// Every argmin / argmax takes the smallest node id among equal keys.
//
// The passes, in launch order:
//   k_lab_nodes     stamps to -1, the node-side input checks
//   k_lab_classify  one thread per edge: the edge-side checks, the class flag, member flags of the endpoints
//   k_lab_poskey    the cursor key of every node;  radix sort (key, id) -> node ids in cursor order, ties by id (stable)
//   k_lab_probkey   the problem key (chr, strand) of the sorted nodes;  stable radix sort -> problems are contiguous runs
//   k_lab_heads     the first position of every problem;  rocprim::select -> prob_start, and select the class edges
//   (one host synchronisation: the check results and the counts)
//   gnnome_build_graph_views over the class edges: successors (out_ptr / out_dst) and predecessors (in_ptr / srt_src)
//   k_lab_loop      one wavefront per problem runs the loop above
//   k_lab_write     y[e] = 1 iff e is a class edge whose endpoints carry the same accepted component stamp
//
// The loop keeps one stamp per node and direction, written once: fstamp[v] = the pass whose forward traversal claimed v
// (so "alive" is fstamp == -1 and F of pass p is fstamp == p), bstamp[v] likewise backwards.  A node enters each queue at most
// once over the whole problem, so each problem's two queues fit in its own slice [lo, hi) of two int32[N] buffers and every
// loop is bounded by the node count.  Problems share nothing: no communication between workgroups, no spin-wait.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"

namespace gnnome {

constexpr int kLabThreads = 256;
constexpr uint64_t kNoProblem = 1ull << 33;   // problem key of a node that is in no problem: sorts after every (chr, strand)
constexpr unsigned kProblemKeyBits = 34;
constexpr int kStatsCols = 8;
enum { kInfoBadEdge = 0, kInfoBadNode = 1, kInfoMembers = 2, kInfoProblems = 3, kInfoClassEdges = 4, kInfoWords = 8 };

static inline size_t lab_align(size_t x) { return (x + 255) & ~(size_t)255; }

static unsigned lab_grid(int64_t n) {
    int64_t b = (n + kLabThreads - 1) / kLabThreads;
    if (b < 1) b = 1;
    if (b > kNumCUs * 16) b = kNumCUs * 16;
    return (unsigned)b;
}

__device__ __forceinline__ uint64_t problem_key(int32_t chr, int32_t strand) {
    return ((uint64_t)((uint32_t)chr ^ 0x80000000u) << 1) | (strand > 0 ? 1u : 0u);   // chr ascending, then strand -1 before +1
}

// the key the loop maximises: end for s = +1, ~start (= -start - 1, order-reversing, no overflow) for s = -1
__device__ __forceinline__ int64_t h_key(int s, const int64_t* start, const int64_t* end, int32_t u) {
    return s > 0 ? end[u] : ~start[u];
}

__global__ void k_lab_nodes(const int32_t* __restrict__ strand, int64_t N, uint8_t* __restrict__ member, int32_t* __restrict__ iota,
                            int32_t* __restrict__ fstamp, int32_t* __restrict__ bstamp, int32_t* __restrict__ comp,
                            unsigned long long* __restrict__ info) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        member[i] = 0;
        iota[i] = (int32_t)i;
        fstamp[i] = bstamp[i] = comp[i] = -1;
        const int32_t s = strand[i];
        if (s != 1 && s != -1) atomicMin(info + kInfoBadNode, (unsigned long long)i);
    }
}

__global__ void k_lab_classify(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t E, int64_t N,
                               const int32_t* __restrict__ strand, const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                               const int32_t* __restrict__ chr, uint8_t* __restrict__ cls, uint8_t* __restrict__ member,
                               unsigned long long* __restrict__ info) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = src[e], v = dst[e];
        uint8_t c = 0;
        if (u < 0 || u >= N || v < 0 || v >= N) {
            atomicMin(info + kInfoBadEdge, (unsigned long long)e);
        } else if (chr[u] == chr[v] && strand[u] == strand[v]) {
            const int32_t s = strand[u];
            if (s == 1) c = start[u] < start[v] && start[v] < end[u];
            else if (s == -1) c = start[v] < start[u] && start[u] < end[v];
            if (c) member[u] = member[v] = 1;   // every writer stores the same byte
        }
        cls[e] = c;
    }
}

__global__ void k_lab_poskey(const int32_t* __restrict__ strand, const int64_t* __restrict__ start, const int64_t* __restrict__ end,
                             int64_t N, int64_t* __restrict__ key) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
        key[i] = strand[i] > 0 ? start[i] : ~end[i];   // the cursor: start ascending (+1), end descending (-1)
}

__global__ void k_lab_probkey(const int32_t* __restrict__ order, const uint8_t* __restrict__ member, const int32_t* __restrict__ strand,
                              const int32_t* __restrict__ chr, int64_t N, uint64_t* __restrict__ pk) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = order[i];
        pk[i] = member[u] ? problem_key(chr[u], strand[u]) : kNoProblem;
    }
}

__global__ void k_lab_heads(const uint64_t* __restrict__ pk, int64_t N, uint8_t* __restrict__ head, unsigned long long* __restrict__ info) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = pk[i];
        head[i] = k != kNoProblem && (i == 0 || pk[i - 1] != k);
        if (k != kNoProblem && (i + 1 == N || pk[i + 1] == kNoProblem)) info[kInfoMembers] = (unsigned long long)(i + 1);   // one writer
    }
}

__global__ void k_lab_take_edges(const int32_t* __restrict__ ceid, int64_t K, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                 int32_t* __restrict__ csrc, int32_t* __restrict__ cdst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t e = ceid[i];
        csrc[i] = src[e];
        cdst[i] = dst[e];
    }
}

// ---- the component loop: one wavefront per problem --------------------------------------------------------------------------

// Stamps and queue entries are read and written at agent scope (they bypass the CU's L1): a line of the queue or of a stamp
// array that one lane loaded must never be served stale to another lane of the same wave after an atomic or a store.
__device__ __forceinline__ int32_t ld_ag(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_ag(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool claim(int32_t* p, int32_t pass) {
    int32_t expected = -1;
    return __hip_atomic_compare_exchange_strong(p, &expected, pass, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (key, id) with the larger key, the smaller id among equal keys; id < 0 is "none"
__device__ __forceinline__ bool lab_better(int64_t ka, int32_t ia, int64_t kb, int32_t ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    return ka > kb || (ka == kb && ia < ib);
}

__device__ __forceinline__ void wave_argmax(int64_t& k, int32_t& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t k2 = __shfl_xor(k, o);
        const int32_t i2 = __shfl_xor(i, o);
        if (lab_better(k2, i2, k, i)) {
            k = k2;
            i = i2;
        }
    }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct LabLoop {
    const int32_t* order;        // node ids, grouped by problem, cursor order within one
    const int32_t* prob_start;   // [P]
    const int32_t *out_ptr, *out_dst, *in_ptr, *in_src;   // class-edge views
    const int32_t *strand, *chr;
    const int64_t *start, *end;
    int32_t *fstamp, *bstamp, *comp, *fq, *bq;
    int64_t* stats;              // NULL or [1 + rows * kStatsCols]
    int64_t stats_rows;
    int64_t members;             // prob_start[P] (the members are order[0, members))
    int num_problems;
};

// Breadth-first traversal from q[head, tail) over one CSR, one wavefront: a lane that has no edge left takes the next queued
// node (ranks by ballot), every lane with an edge examines one neighbour per step, and the claimed neighbours are appended by
// ballot prefix.  Forward: a neighbour is taken when it is alive (fstamp -1 -> pass); the fold keeps argmax hk of the popped
// nodes.  Backward: when it is in this pass's F (fstamp == pass) and not yet taken (bstamp -1 -> pass).  `cap` bounds the
// queue slice; the claims already bound it (a node is claimed once per direction), the test only keeps a broken input in it.
template <bool kForward>
__device__ void lab_traverse(const LabLoop& a, const int32_t* ptr, const int32_t* adj, int32_t* q, int32_t cap, int32_t head, int32_t& tail_io,
                             int32_t pass, int s, int64_t& best_k, int32_t& best_i) {
    const int lane = threadIdx.x;
    const uint64_t below = (1ull << lane) - 1;
    int32_t tail = tail_io, k = 0, kend = 0;
    while (true) {
        const bool idle = k >= kend;
        const uint64_t need = __ballot(idle);
        const int32_t avail = tail - head;
        const int32_t rank = __popcll(need & below);
        if (idle && rank < avail) {
            const int32_t u = ld_ag(q + head + rank);
            k = ptr[u];
            kend = ptr[u + 1];
            if (kForward) {
                const int64_t hk = h_key(s, a.start, a.end, u);
                if (lab_better(hk, u, best_k, best_i)) {
                    best_k = hk;
                    best_i = u;
                }
            }
        }
        const int32_t taken = __popcll(need);
        head += taken < avail ? taken : avail;
        if (__ballot(k < kend) == 0) {
            if (head >= tail) break;
            continue;
        }
        bool got = false;
        int32_t v = 0;
        if (k < kend) {
            v = adj[k++];
            if (kForward) got = ld_ag(a.fstamp + v) == -1 && claim(a.fstamp + v, pass);
            else got = ld_ag(a.fstamp + v) == pass && ld_ag(a.bstamp + v) == -1 && claim(a.bstamp + v, pass);
        }
        const uint64_t m = __ballot(got);
        if (m) {
            const int32_t pos = tail + __popcll(m & below);
            if (got && pos < cap) st_ag(q + pos, v);
            tail += __popcll(m);
            if (tail > cap) tail = cap;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the entries are in memory before any lane pops them
        }
    }
    tail_io = tail;
}

__global__ __launch_bounds__(64) void k_lab_loop(LabLoop a) {
    const int p = blockIdx.x;
    if (p >= a.num_problems) return;
    const int lane = threadIdx.x;
    const int32_t lo = a.prob_start[p];
    const int32_t hi = p + 1 < a.num_problems ? a.prob_start[p + 1] : (int32_t)a.members;
    const int32_t cap = hi - lo;
    const int32_t u0 = a.order[lo];
    const int s = a.strand[u0];

    // final = argmax_V hk, reached = min_V hk (argmax of ~hk), the problem's class edges
    int64_t fk = 0, rk = 0, edges = 0;
    int32_t fi = -1, ri = -1;
    for (int32_t i = lo + lane; i < hi; i += 64) {
        const int32_t u = a.order[i];
        const int64_t hk = h_key(s, a.start, a.end, u);
        if (lab_better(hk, u, fk, fi)) { fk = hk; fi = u; }
        if (lab_better(~hk, u, rk, ri)) { rk = ~hk; ri = u; }
        edges += a.out_ptr[u + 1] - a.out_ptr[u];
    }
    wave_argmax(fk, fi);
    wave_argmax(rk, ri);
    edges = wave_sum(edges);
    const int32_t final_node = fi;
    int64_t reached = ~rk;

    int32_t* fq = a.fq + lo;
    int32_t* bq = a.bq + lo;
    int32_t ftail = 0, btail = 0, pass = 0, accepted = 0, cursor = lo;
    while (cursor < hi) {
        const int32_t start_node = a.order[cursor];   // alive: the cursor only stops on fstamp == -1
        if (lane == 0) {
            st_ag(a.fstamp + start_node, pass);
            st_ag(fq + ftail, start_node);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int32_t fhead = ftail;
        ++ftail;
        int64_t hk = 0;
        int32_t h = -1;
        lab_traverse<true>(a, a.out_ptr, a.out_dst, fq, cap, fhead, ftail, pass, s, hk, h);
        wave_argmax(hk, h);
        bool stop = false;
        if (!(hk < reached)) {
            if (lane == 0) {
                st_ag(a.bstamp + h, pass);
                st_ag(bq + btail, h);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int32_t bhead = btail;
            ++btail;
            int64_t unused_k = 0;
            int32_t unused_i = -1;
            lab_traverse<false>(a, a.in_ptr, a.in_src, bq, cap, bhead, btail, pass, s, unused_k, unused_i);
            if (btail - bhead >= 2) {
                reached = hk;
                ++accepted;
                for (int32_t i = bhead + lane; i < btail; i += 64) a.comp[ld_ag(bq + i)] = pass;
                stop = h == final_node;
            }
        }
        ++pass;
        if (stop) break;
        // alive -= F: F is stamped already, so only the cursor moves, past every claimed node
        while (cursor < hi) {
            const int32_t idx = cursor + lane;
            const bool alive = idx < hi && ld_ag(a.fstamp + a.order[idx]) == -1;
            const uint64_t m = __ballot(alive);
            if (m) {
                cursor += __ffsll((long long)m) - 1;
                break;
            }
            cursor = hi - cursor > 64 ? cursor + 64 : hi;
        }
    }
    if (a.stats && lane == 0 && p < a.stats_rows) {
        int64_t* row = a.stats + 1 + (int64_t)p * kStatsCols;
        row[0] = a.chr[u0];
        row[1] = s;
        row[2] = cap;
        row[3] = edges;
        row[4] = pass;
        row[5] = accepted;
        row[6] = ftail;
        row[7] = btail;
    }
}

__global__ void k_lab_write(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, const uint8_t* __restrict__ cls, int64_t E,
                            const int32_t* __restrict__ comp, float* __restrict__ y, int64_t* __restrict__ stats, int64_t num_problems) {
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) stats[0] = num_problems;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
        float lab = 0.f;
        if (cls[e]) {
            const int32_t cu = comp[src[e]];
            lab = (cu != -1 && cu == comp[dst[e]]) ? 1.f : 0.f;
        }
        y[e] = lab;
    }
}

// ---- workspace -----------------------------------------------------------------------------------------------------------

struct LabLayout {
    size_t cls, ceid, csrc, cdst, srt_src, srt_dst, srt_eid, out_pos, out_dst, in_ptr, out_ptr, member, iota, order1, order2, key_a, key_b,
        pk_a, pk_b, head, prob_start, fstamp, bstamp, comp, fq, bq, info, sort_tmp, views_tmp, total;
    size_t sort_bytes, views_bytes;
};

static int lab_layout(int64_t N, int64_t E, LabLayout* L) {
    size_t sort_bytes = 0, b = 0;
    auto grow = [&](size_t x) { sort_bytes = x > sort_bytes ? x : sort_bytes; };
    const size_t n = (size_t)N, e = (size_t)E;
    if (N > 0) {
        GN_HIP(rocprim::radix_sort_pairs(nullptr, b, (const int64_t*)nullptr, (int64_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, n,
                                         0u, 64u, (hipStream_t)0));
        grow(b);
        GN_HIP(rocprim::radix_sort_pairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr,
                                         n, 0u, kProblemKeyBits, (hipStream_t)0));
        grow(b);
        GN_HIP(rocprim::select(nullptr, b, rocprim::counting_iterator<int32_t>(0), (const uint8_t*)nullptr, (int32_t*)nullptr,
                               (unsigned long long*)nullptr, n, (hipStream_t)0));
        grow(b);
    }
    if (E > 0) {
        GN_HIP(rocprim::select(nullptr, b, rocprim::counting_iterator<int32_t>(0), (const uint8_t*)nullptr, (int32_t*)nullptr,
                               (unsigned long long*)nullptr, e, (hipStream_t)0));
        grow(b);
    }
    size_t views_bytes = 0;
    {
        const int rc = gnnome_graph_views_workspace_bytes(N, E, &views_bytes);
        if (rc != GNNOME_OK) return rc;
    }
    size_t off = 0;
    auto put = [&](size_t bytes) { const size_t at = off; off += lab_align(bytes); return at; };
    L->cls = put(e);
    L->ceid = put(e * 4);
    L->csrc = put(e * 4);
    L->cdst = put(e * 4);
    L->srt_src = put(e * 4);
    L->srt_dst = put(e * 4);
    L->srt_eid = put(e * 4);
    L->out_pos = put(e * 4);
    L->out_dst = put(e * 4);
    L->in_ptr = put((n + 1) * 4);
    L->out_ptr = put((n + 1) * 4);
    L->member = put(n);
    L->iota = put(n * 4);
    L->order1 = put(n * 4);
    L->order2 = put(n * 4);
    L->key_a = put(n * 8);
    L->key_b = put(n * 8);
    L->pk_a = put(n * 8);
    L->pk_b = put(n * 8);
    L->head = put(n);
    L->prob_start = put(n * 4);
    L->fstamp = put(n * 4);
    L->bstamp = put(n * 4);
    L->comp = put(n * 4);
    L->fq = put(n * 4);
    L->bq = put(n * 4);
    L->info = put(kInfoWords * 8);
    L->sort_tmp = put(sort_bytes);
    L->views_tmp = put(views_bytes);
    L->total = off;
    L->sort_bytes = sort_bytes;
    L->views_bytes = views_bytes;
    return GNNOME_OK;
}

}  // namespace gnnome

extern "C" int gnnome_edge_labels_workspace_bytes(int64_t num_nodes, int64_t num_edges, size_t* bytes_host) {
    using namespace gnnome;
    GN_REQUIRE(bytes_host != nullptr, "edge_labels_workspace_bytes: null output");
    GN_REQUIRE(num_nodes >= 0 && num_edges >= 0 && num_nodes < (1ll << 31) && num_edges < (1ll << 31),
               "edge_labels: N=%lld E=%lld out of int32 range", (long long)num_nodes, (long long)num_edges);
    LabLayout L;
    const int rc = lab_layout(num_nodes, num_edges, &L);
    if (rc != GNNOME_OK) return rc;
    *bytes_host = L.total;
    return GNNOME_OK;
}

extern "C" int gnnome_edge_labels(const int32_t* src, const int32_t* dst, int64_t num_edges, int64_t num_nodes, const int32_t* read_strand,
                                  const int64_t* read_start, const int64_t* read_end, const int32_t* read_chr, float* y, int64_t* stats,
                                  int64_t stats_rows, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes, E = num_edges;
    GN_REQUIRE(N >= 0 && E >= 0 && N < (1ll << 31) && E < (1ll << 31), "edge_labels: N=%lld E=%lld out of int32 range", (long long)N,
               (long long)E);
    GN_REQUIRE(stats_rows >= 0, "edge_labels: stats_rows %lld < 0", (long long)stats_rows);
    GN_REQUIRE(N > 0 || E == 0, "edge_labels: %lld edges on a graph without nodes", (long long)E);
    GN_REQUIRE((E == 0 || (src && dst && y)) && (N == 0 || (read_strand && read_start && read_end && read_chr)) && workspace,
               "edge_labels: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        if (stats) GN_HIP(hipMemsetAsync(stats, 0, sizeof(int64_t), s));
        return GNNOME_OK;
    }
    LabLayout L;
    {
        const int rc = lab_layout(N, E, &L);
        if (rc != GNNOME_OK) return rc;
    }
    if (workspace_bytes < L.total) {
        set_error("edge_labels: workspace %zu < %zu bytes", workspace_bytes, L.total);
        return GNNOME_EWORKSPACE;
    }
    char* ws = (char*)workspace;
    auto at = [&](size_t o) { return (void*)(ws + o); };
    uint8_t* cls = (uint8_t*)at(L.cls);
    int32_t *ceid = (int32_t*)at(L.ceid), *csrc = (int32_t*)at(L.csrc), *cdst = (int32_t*)at(L.cdst);
    int32_t *in_ptr = (int32_t*)at(L.in_ptr), *out_ptr = (int32_t*)at(L.out_ptr);
    int32_t *srt_src = (int32_t*)at(L.srt_src), *srt_dst = (int32_t*)at(L.srt_dst), *srt_eid = (int32_t*)at(L.srt_eid);
    int32_t *out_pos = (int32_t*)at(L.out_pos), *out_dst = (int32_t*)at(L.out_dst);
    uint8_t* member = (uint8_t*)at(L.member);
    int32_t *iota = (int32_t*)at(L.iota), *order1 = (int32_t*)at(L.order1), *order2 = (int32_t*)at(L.order2);
    int64_t *key_a = (int64_t*)at(L.key_a), *key_b = (int64_t*)at(L.key_b);
    uint64_t *pk_a = (uint64_t*)at(L.pk_a), *pk_b = (uint64_t*)at(L.pk_b);
    uint8_t* head = (uint8_t*)at(L.head);
    int32_t* prob_start = (int32_t*)at(L.prob_start);
    int32_t *fstamp = (int32_t*)at(L.fstamp), *bstamp = (int32_t*)at(L.bstamp), *comp = (int32_t*)at(L.comp);
    int32_t *fq = (int32_t*)at(L.fq), *bq = (int32_t*)at(L.bq);
    unsigned long long* info = (unsigned long long*)at(L.info);
    void* sort_tmp = at(L.sort_tmp);

    // info: the two "first bad index" words start at all ones, the counts at zero
    GN_HIP(hipMemsetAsync(info, 0xFF, 2 * sizeof(unsigned long long), s));
    GN_HIP(hipMemsetAsync(info + 2, 0, (kInfoWords - 2) * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_lab_nodes, dim3(lab_grid(N)), dim3(kLabThreads), 0, s, read_strand, N, member, iota, fstamp, bstamp, comp, info);
    GN_LAUNCH_CHECK();
    if (E > 0) {
        hipLaunchKernelGGL(k_lab_classify, dim3(lab_grid(E)), dim3(kLabThreads), 0, s, src, dst, E, N, read_strand, read_start, read_end,
                           read_chr, cls, member, info);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_lab_poskey, dim3(lab_grid(N)), dim3(kLabThreads), 0, s, read_strand, read_start, read_end, N, key_a);
    GN_LAUNCH_CHECK();
    size_t sb = L.sort_bytes;
    GN_HIP(rocprim::radix_sort_pairs(sort_tmp, sb, (const int64_t*)key_a, key_b, (const int32_t*)iota, order1, (size_t)N, 0u, 64u, s));
    hipLaunchKernelGGL(k_lab_probkey, dim3(lab_grid(N)), dim3(kLabThreads), 0, s, (const int32_t*)order1, (const uint8_t*)member, read_strand,
                       read_chr, N, pk_a);
    GN_LAUNCH_CHECK();
    sb = L.sort_bytes;
    GN_HIP(rocprim::radix_sort_pairs(sort_tmp, sb, (const uint64_t*)pk_a, pk_b, (const int32_t*)order1, order2, (size_t)N, 0u, kProblemKeyBits, s));
    hipLaunchKernelGGL(k_lab_heads, dim3(lab_grid(N)), dim3(kLabThreads), 0, s, (const uint64_t*)pk_b, N, head, info);
    GN_LAUNCH_CHECK();
    sb = L.sort_bytes;
    GN_HIP(rocprim::select(sort_tmp, sb, rocprim::counting_iterator<int32_t>(0), (const uint8_t*)head, prob_start, info + kInfoProblems,
                           (size_t)N, s));
    if (E > 0) {
        sb = L.sort_bytes;
        GN_HIP(rocprim::select(sort_tmp, sb, rocprim::counting_iterator<int32_t>(0), (const uint8_t*)cls, ceid, info + kInfoClassEdges,
                               (size_t)E, s));
    }
    unsigned long long h[kInfoWords];
    GN_HIP(hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    if (h[kInfoBadEdge] != ~0ull) {
        const long long e = (long long)h[kInfoBadEdge];
        set_error("edge_labels: edge %lld has a node outside [0, %lld)", e, (long long)N);
        return GNNOME_EINVAL;
    }
    GN_REQUIRE(h[kInfoBadNode] == ~0ull, "edge_labels: node %lld has a strand other than -1 / +1", (long long)h[kInfoBadNode]);
    const int64_t members = (int64_t)h[kInfoMembers], P = (int64_t)h[kInfoProblems], K = (int64_t)h[kInfoClassEdges];

    if (K > 0) {
        hipLaunchKernelGGL(k_lab_take_edges, dim3(lab_grid(K)), dim3(kLabThreads), 0, s, (const int32_t*)ceid, K, src, dst, csrc, cdst);
        GN_LAUNCH_CHECK();
        size_t need = 0;
        int rc = gnnome_graph_views_workspace_bytes(N, K, &need);
        if (rc != GNNOME_OK) return rc;
        if (need > L.views_bytes) {
            set_error("edge_labels: graph views need %zu > %zu workspace bytes", need, L.views_bytes);
            return GNNOME_EWORKSPACE;
        }
        rc = gnnome_build_graph_views(csrc, cdst, N, K, in_ptr, srt_src, srt_dst, srt_eid, out_ptr, out_pos, out_dst, at(L.views_tmp),
                                      L.views_bytes, s);
        if (rc != GNNOME_OK) return rc;
        LabLoop a{order2, prob_start, out_ptr, out_dst, in_ptr, srt_src, read_strand, read_chr, read_start, read_end, fstamp, bstamp, comp,
                  fq, bq, stats, stats_rows, members, (int)P};
        hipLaunchKernelGGL(k_lab_loop, dim3((unsigned)P), dim3(64), 0, s, a);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_lab_write, dim3(lab_grid(E)), dim3(kLabThreads), 0, s, src, dst, (const uint8_t*)cls, E, (const int32_t*)comp, y,
                       stats, P);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
