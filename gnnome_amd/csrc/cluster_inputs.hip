// Every cluster's model inputs in one call (train.py:125-135 get_partition_ne_features, train.py:148-186 the gathers of
// get_bce_loss_partition / get_symmetry_loss_partition), for all k clusters of a graph at once.
//
// Clusters are packed: cluster c owns node positions [node_ptr[c], node_ptr[c+1]) of nid and edge positions
// [edge_ptr[c], edge_ptr[c+1]) of eid.  A node position p stands for the full-graph node g = outer_nid[nid[p]] (or nid[p]
// without an outer map), an edge position for the full-graph edge outer_eid[eid[p]] (or eid[p]).  Outputs, packed the same way:
//   x_org[p] = [z_in | z_out], x_rev[p] = [z_out | z_in], z = (d - mean_c) / std_c over the cluster's nodes, mean and UNBIASED std
//   e_sub[p] = e[edge], y_sub[p] = y[edge]
//
// The passes, in launch order:
//   k_ci_clusters   per cluster: the ptr checks, the shift (the degrees of its first node)
//   k_ci_partials   per tile of kTile node positions: the id checks, then a segmented scan of (d - shift, (d - shift)^2) in fp64;
//                   a cluster that lies inside the tile gets its sums, a cluster that crosses a tile border leaves one
//                   partial per tile it touches (F[t]: the tile's first segment, begun earlier; L[t]: its last, going on)
//   k_ci_edge_check per edge position: the id checks
//   (one host synchronisation: the check results; an error names the cluster and nothing is written)
//   k_ci_finalize   one workgroup per cluster: L[first tile] + the F[] of the later tiles in a fixed tree -> mean, std
//   k_ci_nodes      x_org / x_rev;  k_ci_edges  e_sub / y_sub
// Every sum is a function of the tile size and the workgroup size alone, both compile-time constants: the bits do not depend on
// the grid, and no float is accumulated with an atomic (the only atomics are the integer minima of the check words).
#include "common.h"

namespace gnnome {

constexpr int kCiThreads = 256;
constexpr int kTile = kCiThreads;   // node positions per tile of k_ci_partials
enum {
    kCiNodePtr = 0, kCiEdgePtr = 1,
    kCiNidC = 2, kCiNidP = 3, kCiOuterNidC = 4, kCiOuterNidP = 5,
    kCiEidC = 6, kCiEidP = 7, kCiOuterEidC = 8, kCiOuterEidP = 9,
    kCiWords = 16
};

struct CiLayout {
    size_t info, shift, stats, whole, first, last, total;
};

static inline size_t ci_align(size_t x) { return (x + 255) & ~(size_t)255; }

static CiLayout ci_layout(int64_t k, int64_t total_nodes) {
    const int64_t tiles = (total_nodes + kTile - 1) / kTile;
    CiLayout L;
    size_t o = 0;
    L.info = o;  o = ci_align(o + kCiWords * sizeof(unsigned long long));
    L.shift = o; o = ci_align(o + (size_t)k * 2 * sizeof(float));
    L.stats = o; o = ci_align(o + (size_t)k * 4 * sizeof(float));
    L.whole = o; o = ci_align(o + (size_t)k * 4 * sizeof(double));
    L.first = o; o = ci_align(o + (size_t)tiles * 4 * sizeof(double));
    L.last = o;  o = ci_align(o + (size_t)tiles * 4 * sizeof(double));
    L.total = o;
    return L;
}

static unsigned ci_grid(int64_t n) {
    int64_t b = (n + kCiThreads - 1) / kCiThreads;
    if (b < 1) b = 1;
    if (b > kNumCUs * 16) b = kNumCUs * 16;
    return (unsigned)b;
}

// the cluster that owns position p: the largest c in [0, k) with ptr[c] <= p (empty clusters own nothing); always in [0, k)
__device__ __forceinline__ int64_t ci_owner(const int64_t* __restrict__ ptr, int64_t k, int64_t p) {
    int64_t lo = 0, hi = k - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the full-graph id behind position p, or -1 (and the check words raised) when an id is out of range
__device__ __forceinline__ int64_t ci_resolve(const int64_t* __restrict__ ids, const int64_t* __restrict__ outer, int64_t n_outer, int64_t n,
                                              int64_t p, int64_t c, unsigned long long* __restrict__ info, int w_c, int w_p, int w_oc, int w_op) {
    const int64_t a = ids[p];
    if (a < 0 || a >= (outer ? n_outer : n)) {
        atomicMin(info + w_c, (unsigned long long)c);
        atomicMin(info + w_p, (unsigned long long)p);
        return -1;
    }
    if (!outer) return a;
    const int64_t g = outer[a];
    if (g < 0 || g >= n) {
        atomicMin(info + w_oc, (unsigned long long)c);
        atomicMin(info + w_op, (unsigned long long)p);
        return -1;
    }
    return g;
}

__device__ __forceinline__ bool ci_ptr_ok(const int64_t* __restrict__ ptr, int64_t k, int64_t total, int64_t c) {
    const int64_t lo = ptr[c], hi = ptr[c + 1];
    return !((c == 0 && lo != 0) || hi < lo || hi > total || (c == k - 1 && hi != total));
}

__global__ void k_ci_clusters(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr, int64_t k, int64_t total_nodes,
                              int64_t total_edges, const int64_t* __restrict__ nid, const int64_t* __restrict__ outer_nid, int64_t n_outer,
                              const float* __restrict__ in_deg, const float* __restrict__ out_deg, int64_t N, float* __restrict__ shift,
                              unsigned long long* __restrict__ info) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < k; c += (int64_t)gridDim.x * blockDim.x) {
        if (!ci_ptr_ok(node_ptr, k, total_nodes, c)) atomicMin(info + kCiNodePtr, (unsigned long long)c);
        if (!ci_ptr_ok(edge_ptr, k, total_edges, c)) atomicMin(info + kCiEdgePtr, (unsigned long long)c);
        float si = 0.f, so = 0.f;
        const int64_t p = node_ptr[c];
        if (p >= 0 && p < total_nodes && p < node_ptr[c + 1]) {   // the first node's degrees; a bad id is reported by k_ci_partials
            int64_t a = nid[p];
            if (a >= 0 && a < (outer_nid ? n_outer : N)) {
                if (outer_nid) a = outer_nid[a];
                if (a >= 0 && a < N) si = in_deg[a], so = out_deg[a];
            }
        }
        shift[2 * c] = si;
        shift[2 * c + 1] = so;
    }
}

__global__ void __launch_bounds__(kCiThreads) k_ci_partials(const int64_t* __restrict__ node_ptr, int64_t k, int64_t total_nodes,
                                                            const int64_t* __restrict__ nid, const int64_t* __restrict__ outer_nid, int64_t n_outer,
                                                            const float* __restrict__ in_deg, const float* __restrict__ out_deg, int64_t N,
                                                            const float* __restrict__ shift, double* __restrict__ whole, double* __restrict__ first,
                                                            double* __restrict__ last, unsigned long long* __restrict__ info) {
    __shared__ int64_t cid_s[kTile];
    __shared__ double v_s[4][kTile];
    const int tid = threadIdx.x;
    const int64_t tiles = (total_nodes + kTile - 1) / kTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t t0 = t * kTile, p = t0 + tid;
        int64_t c = -1;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (p < total_nodes) {
            c = ci_owner(node_ptr, k, p);
            const int64_t g = ci_resolve(nid, outer_nid, n_outer, N, p, c, info, kCiNidC, kCiNidP, kCiOuterNidC, kCiOuterNidP);
            if (g >= 0) {
                const double a = (double)in_deg[g] - (double)shift[2 * c], b = (double)out_deg[g] - (double)shift[2 * c + 1];
                v[0] = a, v[1] = a * a, v[2] = b, v[3] = b * b;
            }
        }
        cid_s[tid] = c;
        for (int j = 0; j < 4; ++j) v_s[j][tid] = v[j];
        __syncthreads();
        // inclusive segmented scan (Hillis-Steele): the ids are non-decreasing along the tile, so equal ids off positions apart
        // mean one segment in between
        for (int off = 1; off < kTile; off <<= 1) {
            const bool take = tid >= off && c >= 0 && cid_s[tid - off] == c;
            double add[4] = {0.0, 0.0, 0.0, 0.0};
            if (take)
                for (int j = 0; j < 4; ++j) add[j] = v_s[j][tid - off];
            __syncthreads();
            if (take)
                for (int j = 0; j < 4; ++j) v_s[j][tid] = v[j] += add[j];
            __syncthreads();
        }
        if (c >= 0 && (tid == kTile - 1 || cid_s[tid + 1] != c)) {   // the last position of a segment holds its sums
            const bool begun = node_ptr[c] < t0, goes_on = node_ptr[c + 1] - 1 > p;
            double* dst = begun ? first + 4 * t : goes_on ? last + 4 * t : whole + 4 * c;
            for (int j = 0; j < 4; ++j) dst[j] = v[j];
        }
        __syncthreads();
    }
}

__global__ void k_ci_edge_check(const int64_t* __restrict__ edge_ptr, int64_t k, int64_t total_edges, const int64_t* __restrict__ eid,
                                const int64_t* __restrict__ outer_eid, int64_t e_outer, int64_t E, unsigned long long* __restrict__ info) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total_edges; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = eid[p];
        const bool bad = a < 0 || a >= (outer_eid ? e_outer : E);
        const bool bad_outer = !bad && outer_eid && (outer_eid[a] < 0 || outer_eid[a] >= E);
        if (bad || bad_outer) {   // rare: only then is the owner looked up
            const int64_t c = ci_owner(edge_ptr, k, p);
            atomicMin(info + (bad ? kCiEidC : kCiOuterEidC), (unsigned long long)c);
            atomicMin(info + (bad ? kCiEidP : kCiOuterEidP), (unsigned long long)p);
        }
    }
}

__global__ void __launch_bounds__(kCiThreads) k_ci_finalize(const int64_t* __restrict__ node_ptr, int64_t k, const float* __restrict__ shift,
                                                            const double* __restrict__ whole, const double* __restrict__ first,
                                                            const double* __restrict__ last, float* __restrict__ stats) {
    __shared__ double r_s[4][kCiThreads];
    const int tid = threadIdx.x;
    for (int64_t c = blockIdx.x; c < k; c += gridDim.x) {
        const int64_t lo = node_ptr[c], hi = node_ptr[c + 1], n = hi - lo;
        if (n == 0) continue;   // uniform over the workgroup
        const int64_t ta = lo / kTile, tb = (hi - 1) / kTile;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (ta != tb) {
            for (int64_t t = ta + 1 + tid; t <= tb; t += kCiThreads)
                for (int j = 0; j < 4; ++j) s[j] += first[4 * t + j];
            for (int j = 0; j < 4; ++j) r_s[j][tid] = s[j];
            __syncthreads();
            for (int w = kCiThreads / 2; w > 0; w >>= 1) {
                if (tid < w)
                    for (int j = 0; j < 4; ++j) r_s[j][tid] += r_s[j][tid + w];
                __syncthreads();
            }
            for (int j = 0; j < 4; ++j) s[j] = last[4 * ta + j] + r_s[j][0];
            __syncthreads();
        } else {
            for (int j = 0; j < 4; ++j) s[j] = whole[4 * c + j];
        }
        if (tid == 0) {
            const double nd = (double)n;
            for (int col = 0; col < 2; ++col) {
                const double s1 = s[2 * col], s2 = s[2 * col + 1];
                const double mean = ((double)shift[2 * c + col] * nd + s1) / nd;
                double m2 = s2 - s1 * s1 / nd;
                if (m2 < 0.0) m2 = 0.0;                  // rounding only: the shifted moments give m2 >= 0 exactly
                const double var = m2 / (nd - 1.0);      // n = 1: 0 / 0 = NaN, as torch.std
                stats[4 * c + 2 * col] = (float)mean;
                stats[4 * c + 2 * col + 1] = (float)sqrt(var);
            }
        }
    }
}

__global__ void k_ci_nodes(const int64_t* __restrict__ node_ptr, int64_t k, int64_t total_nodes, const int64_t* __restrict__ nid,
                           const int64_t* __restrict__ outer_nid, const float* __restrict__ in_deg, const float* __restrict__ out_deg,
                           const float* __restrict__ stats, float2* __restrict__ x_org, float2* __restrict__ x_rev) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total_nodes; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = ci_owner(node_ptr, k, p);
        int64_t g = nid[p];
        if (outer_nid) g = outer_nid[g];
        const float4 st = reinterpret_cast<const float4*>(stats)[c];
        const float zi = (in_deg[g] - st.x) / st.y, zo = (out_deg[g] - st.z) / st.w;   // torch: (d - d.mean()) / d.std() in fp32
        x_org[p] = make_float2(zi, zo);
        if (x_rev) x_rev[p] = make_float2(zo, zi);
    }
}

__global__ void k_ci_edges(int64_t total_edges, const int64_t* __restrict__ eid, const int64_t* __restrict__ outer_eid,
                           const float2* __restrict__ e, const float* __restrict__ y, float2* __restrict__ e_sub, float* __restrict__ y_sub) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total_edges; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t g = eid[p];
        if (outer_eid) g = outer_eid[g];
        e_sub[p] = e[g];
        if (y_sub) y_sub[p] = y[g];
    }
}

}  // namespace gnnome

extern "C" int gnnome_cluster_inputs_workspace_bytes(int64_t num_clusters, int64_t total_nodes, size_t* bytes_host) {
    GN_REQUIRE(num_clusters >= 0 && total_nodes >= 0 && bytes_host, "cluster_inputs_workspace_bytes: bad argument");
    *bytes_host = gnnome::ci_layout(num_clusters, total_nodes).total;
    return GNNOME_OK;
}

extern "C" int gnnome_cluster_inputs_f32(const int64_t* node_ptr, const int64_t* nid, int64_t num_clusters, int64_t total_nodes,
                                         const int64_t* edge_ptr, const int64_t* eid, int64_t total_edges, const int64_t* outer_nid,
                                         int64_t outer_nodes, const int64_t* outer_eid, int64_t outer_edges, const float* in_deg,
                                         const float* out_deg, int64_t num_nodes, const float* e, const float* y, int64_t num_edges,
                                         float* x_org, float* x_rev, float* e_sub, float* y_sub, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    using namespace gnnome;
    const int64_t k = num_clusters, TN = total_nodes, TE = total_edges, N = num_nodes, E = num_edges;
    GN_REQUIRE(k >= 0 && TN >= 0 && TE >= 0 && N >= 0 && E >= 0 && outer_nodes >= 0 && outer_edges >= 0,
               "cluster_inputs: negative size (k=%lld nodes=%lld edges=%lld)", (long long)k, (long long)TN, (long long)TE);
    GN_REQUIRE(k > 0 || (TN == 0 && TE == 0), "cluster_inputs: %lld node and %lld edge positions without clusters", (long long)TN,
               (long long)TE);
    if (k == 0) return GNNOME_OK;
    GN_REQUIRE(node_ptr && edge_ptr && workspace, "cluster_inputs: null pointer");
    GN_REQUIRE(TN == 0 || (nid && in_deg && out_deg && x_org), "cluster_inputs: null node pointer");
    GN_REQUIRE(TE == 0 || (eid && e && e_sub), "cluster_inputs: null edge pointer");
    GN_REQUIRE((y == nullptr) == (y_sub == nullptr), "cluster_inputs: y and y_sub go together");
    const CiLayout L = ci_layout(k, TN);
    if (workspace_bytes < L.total) {
        set_error("cluster_inputs: workspace %zu < %zu bytes", workspace_bytes, L.total);
        return GNNOME_EWORKSPACE;
    }
    char* ws = (char*)workspace;
    unsigned long long* info = (unsigned long long*)(ws + L.info);
    float* shift = (float*)(ws + L.shift);
    float* stats = (float*)(ws + L.stats);
    double *whole = (double*)(ws + L.whole), *first = (double*)(ws + L.first), *last = (double*)(ws + L.last);
    hipStream_t s = (hipStream_t)stream;

    // pass 1: every check, and the node sums (workspace only)
    GN_HIP(hipMemsetAsync(info, 0xFF, kCiWords * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_ci_clusters, dim3(ci_grid(k)), dim3(kCiThreads), 0, s, node_ptr, edge_ptr, k, TN, TE, nid, outer_nid, outer_nodes,
                       in_deg, out_deg, N, shift, info);
    GN_LAUNCH_CHECK();
    const int64_t tiles = (TN + kTile - 1) / kTile;
    if (tiles > 0) {
        hipLaunchKernelGGL(k_ci_partials, dim3((unsigned)(tiles < kNumCUs * 8 ? tiles : kNumCUs * 8)), dim3(kCiThreads), 0, s, node_ptr, k, TN,
                           nid, outer_nid, outer_nodes, in_deg, out_deg, N, (const float*)shift, whole, first, last, info);
        GN_LAUNCH_CHECK();
    }
    if (TE > 0) {
        hipLaunchKernelGGL(k_ci_edge_check, dim3(ci_grid(TE)), dim3(kCiThreads), 0, s, edge_ptr, k, TE, eid, outer_eid, outer_edges, E, info);
        GN_LAUNCH_CHECK();
    }
    unsigned long long h[kCiWords];
    GN_HIP(hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    GN_REQUIRE(h[kCiNodePtr] == ~0ull, "cluster_inputs: cluster %lld: node_ptr is not monotone from 0 to %lld", (long long)h[kCiNodePtr],
               (long long)TN);
    GN_REQUIRE(h[kCiEdgePtr] == ~0ull, "cluster_inputs: cluster %lld: edge_ptr is not monotone from 0 to %lld", (long long)h[kCiEdgePtr],
               (long long)TE);
    GN_REQUIRE(h[kCiNidC] == ~0ull, "cluster_inputs: cluster %lld: nid[%lld] out of range [0, %lld)", (long long)h[kCiNidC],
               (long long)h[kCiNidP], (long long)(outer_nid ? outer_nodes : N));
    GN_REQUIRE(h[kCiOuterNidC] == ~0ull, "cluster_inputs: cluster %lld: outer_nid[nid[%lld]] out of range [0, %lld)",
               (long long)h[kCiOuterNidC], (long long)h[kCiOuterNidP], (long long)N);
    GN_REQUIRE(h[kCiEidC] == ~0ull, "cluster_inputs: cluster %lld: eid[%lld] out of range [0, %lld)", (long long)h[kCiEidC],
               (long long)h[kCiEidP], (long long)(outer_eid ? outer_edges : E));
    GN_REQUIRE(h[kCiOuterEidC] == ~0ull, "cluster_inputs: cluster %lld: outer_eid[eid[%lld]] out of range [0, %lld)",
               (long long)h[kCiOuterEidC], (long long)h[kCiOuterEidP], (long long)E);

    // pass 2: the statistics and the outputs
    if (TN > 0) {
        hipLaunchKernelGGL(k_ci_finalize, dim3((unsigned)(k < kNumCUs * 16 ? k : kNumCUs * 16)), dim3(kCiThreads), 0, s, node_ptr, k,
                           (const float*)shift, (const double*)whole, (const double*)first, (const double*)last, stats);
        GN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_ci_nodes, dim3(ci_grid(TN)), dim3(kCiThreads), 0, s, node_ptr, k, TN, nid, outer_nid, in_deg, out_deg,
                           (const float*)stats, (float2*)x_org, (float2*)x_rev);
        GN_LAUNCH_CHECK();
    }
    if (TE > 0) {
        hipLaunchKernelGGL(k_ci_edges, dim3(ci_grid(TE)), dim3(kCiThreads), 0, s, TE, eid, outer_eid, (const float2*)e, y, (float2*)e_sub, y_sub);
        GN_LAUNCH_CHECK();
    }
    return GNNOME_OK;
}
