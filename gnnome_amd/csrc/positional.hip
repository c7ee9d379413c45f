// Positional encodings of the dataset path (utils/data_utils.py:53-90, add_positional_encoding with nb_pos_enc > 0), as
// tests/positional_statement.py states them: the k-step PageRank features (:74-90) and the k-step random-walk return
// probabilities (:59-72).  Everything is fp64 until one final cast; no atomics of any kind, every output slot has one writer, every
// sum a fixed association: the result is a pure function of the input and does not depend on the grid.
//
// PageRank (type_pos_enc = 'PR').  x_0 = 1/n, x_{t+1}[v] = 0.95 * sum_{u -> v} x_t[u] * dinv[u] + (1 - 0.95)/n, dinv[u] = 1/(outdeg(u) + 1e-9),
// 0 where outdeg(u) < 1e-9 - the reference's expressions, the 1e-9 included.  A parallel edge is one term per copy (scipy sums the
// duplicate entries of A), a self-loop is an ordinary edge.  One launch per step, a gather over the destination-sorted in-list: a
// thread owns a destination and adds its terms in list order; a list longer than a wavefront is summed by the whole wavefront, lane l
// taking entries l, l + 64, ... in order and the 64 partial sums meeting in the xor butterfly 32, 16, ..., 1.  Each step leaves
// y_{t+1} = x_{t+1} * dinv next to column t of the table, so an edge costs one 8-byte read.
//
// Random-walk return (type_pos_enc = 'RW').  PE[i, t-1] = (M^t)[i, i], M[u, v] = mult(u -> v) / max(indeg(v), 1).  Which axis DGL's
// adjacency_matrix puts the sources on does not matter: (M^t)[i, i] is the sum, over the closed walks of length t through i, of the
// product of 1/max(indeg, 1) over the walk's nodes (i counted once), and a closed walk of the graph read backwards is a closed walk
// of the transposed convention with the same nodes - the same sum, term for term.  No matrix power is formed.  One workgroup owns
// node i and keeps the sparse row r_t = e_i^T M^t as (node id ascending, fp64 value) pairs in LDS.  A step
//   1. scans the out-degrees of the row's nodes (wavefront 0, __shfl_up): the offsets of their out-lists in the expansion and its
//      size T; T > capacity ends the node: it records T and raises the status word, nothing was written past a buffer;
//      T = 0 ends it too - the row is empty and every later column is 0;
//   2. expands: entry k writes, for its q-th out-edge u -> v, the key (v << 32 | position) and the value r_t[u] * inv[v];
//   3. sorts the keys (bitonic, in LDS): by node id, then by position = (row order, edge order) - keys are distinct, so the order
//      does not depend on the sorting network;
//   4. marks the first key of every run of equal ids and ranks it (wavefront 0, __ballot + popcount);
//   5. the thread of a run's head adds the run's values left to right - the fixed association - and writes (id, sum) at its rank:
//      the next row, ids ascending.  The run of id i is column t of the output.
// capacity counts the pairs of ONE expansion, sum of outdeg over the row's nodes; the merged row is never longer.
// LDS per workgroup: 8 * pow2ceil(capacity) + 24 * capacity + 4 bytes (keys, expanded values, row values, row ids, offsets/ranks):
// 32 KiB + 4 at the default capacity of 1024, with the kernel's 32 bytes of scalars four workgroups per CU (a fifth misses the 160 KiB by
// 180 bytes).  Up to 1024 a workgroup is ONE wavefront (its barriers are free and four nodes share a CU); a larger capacity leaves room for one or two workgroups per CU, which then get four wavefronts
// each for the expansion, the sort and the run sums (the two scans stay with wavefront 0: they are O(T), the sort O(T log^2 T)).
#include "common.h"

namespace gnnome {

typedef unsigned long long u64;

constexpr int kPeThreads = 256;
constexpr double kPrAlpha = 0.95;          // data_utils.py:85
constexpr int kRwOneWaveCapacity = 1024;   // up to here a node is owned by one wavefront
constexpr size_t kRwMaxLds = 160 * 1024;

// data_utils.py:77-78
__device__ __forceinline__ double pr_dinv(int32_t outdeg) {
    const double d = (double)outdeg;
    return d < 1e-9 ? 0.0 : 1.0 / (d + 1e-9);
}

__global__ void __launch_bounds__(kPeThreads) k_pr_init(const int32_t* __restrict__ out_deg, int64_t N, double* __restrict__ y) {
    const int64_t v = (int64_t)blockIdx.x * kPeThreads + threadIdx.x;
    if (v < N) y[v] = (1.0 / (double)N) * pr_dinv(out_deg[v]);   // :81-83: x = One / n
}

// one step (:87): column t of the table and y_next = x_{t+1} * dinv from y = x_t * dinv
__global__ void __launch_bounds__(kPeThreads) k_pr_step(const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src,
                                                        const int32_t* __restrict__ out_deg, int64_t N, int pe_dim, int t,
                                                        const double* __restrict__ y, double* __restrict__ y_next,
                                                        double* __restrict__ table) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t v = (int64_t)blockIdx.x * kPeThreads + threadIdx.x;
    const bool in = v < N;
    const int32_t b = in ? in_ptr[v] : 0, e = in ? in_ptr[v + 1] : 0;
    const bool wide = e - b > kWave;
    double s = 0.0;
    if (!wide)
        for (int32_t p = b; p < e; ++p) s += y[in_src[p]];
    u64 todo = __ballot(wide);
    while (todo) {   // the lists longer than a wavefront, one after the other, by all 64 lanes
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int32_t wb = __shfl(b, l), we = __shfl(e, l);
        double part = 0.0;
        for (int32_t p = wb + lane; p < we; p += kWave) part += y[in_src[p]];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if (lane == l) s = part;
    }
    if (in) {
        const double x = kPrAlpha * s + (1.0 - kPrAlpha) / (double)N;
        table[v * pe_dim + t] = x;
        y_next[v] = x * pr_dinv(out_deg[v]);
    }
}

// the one cast (:88 / :70, .float()) or copy of the fp64 table into the caller's output; does nothing where `status` says a row overflowed
__global__ void __launch_bounds__(kPeThreads) k_pe_finish(const double* __restrict__ table, int64_t count, const int32_t* __restrict__ status,
                                                          float* __restrict__ out_f32, double* __restrict__ out_f64) {
    if (status && status[0] != 0) return;
    for (int64_t k = (int64_t)blockIdx.x * kPeThreads + threadIdx.x; k < count; k += (int64_t)gridDim.x * kPeThreads) {
        if (out_f32) out_f32[k] = (float)table[k];
        if (out_f64) out_f64[k] = table[k];
    }
}

static unsigned pe_grid(int64_t count) {
    const int64_t blocks = (count + kPeThreads - 1) / kPeThreads;
    return (unsigned)(blocks < 1 ? 1 : blocks < kNumCUs * 16 ? blocks : kNumCUs * 16);
}

// data_utils.py:62: in_degrees().clip(1) ** -1.0
__global__ void __launch_bounds__(kPeThreads) k_rw_inv(const int32_t* __restrict__ in_deg, int64_t N, double* __restrict__ inv) {
    const int64_t v = (int64_t)blockIdx.x * kPeThreads + threadIdx.x;
    if (v < N) inv[v] = 1.0 / (double)(in_deg[v] > 1 ? in_deg[v] : 1);
}

static inline int rw_pow2ceil(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}
static inline size_t rw_lds_bytes(int capacity) { return (size_t)8 * rw_pow2ceil(capacity) + (size_t)24 * capacity + 4; }

__global__ void __launch_bounds__(kPeThreads) k_rw_return(const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                                          const double* __restrict__ inv, int pe_dim, int C, int Cpad,
                                                          double* __restrict__ table, int32_t* __restrict__ info, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rw_lds[];
    u64* keys = reinterpret_cast<u64*>(rw_lds);        // [Cpad] (node id << 32) | position in the expansion
    double* evals = reinterpret_cast<double*>(keys + Cpad);   // [C] expanded values, by position
    double* rvals = evals + C;                         // [C] the row's values
    int32_t* rids = reinterpret_cast<int32_t*>(rvals + C);    // [C] the row's node ids, ascending
    int32_t* aux = rids + C;                           // [C + 1] step 1: offsets of the out-lists; step 4: rank of a run's head, -1 elsewhere
    __shared__ long long s_total;
    __shared__ int s_len;
    __shared__ double s_diag;

    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & (kWave - 1);
    const int64_t i = blockIdx.x;
    if (tid == 0) {
        rids[0] = (int32_t)i;
        rvals[0] = 1.0;
    }
    int L = 1, steps = 0;
    long long need = 0;
    bool over = false;
    __syncthreads();
    for (int t = 0; t < pe_dim; ++t) {
        // 1. offsets of the out-lists and the size of the expansion
        if (tid < kWave) {
            long long base = 0;
            for (int c = 0; c < L; c += kWave) {
                const int k = c + lane;
                long long d = 0;
                if (k < L) {
                    const int32_t u = rids[k];
                    d = out_ptr[u + 1] - out_ptr[u];
                }
                long long inc = d;
#pragma unroll
                for (int o = 1; o < kWave; o <<= 1) {
                    const long long up = __shfl_up(inc, o);
                    if (lane >= o) inc += up;
                }
                if (k < L) aux[k] = (int32_t)(base + inc - d <= C ? base + inc - d : C);   // only read when the total fits
                base += __shfl(inc, kWave - 1);
            }
            if (tid == 0) s_total = base;
        }
        __syncthreads();
        const long long T64 = s_total;
        if (T64 > need) need = T64;
        if (T64 > C) {
            over = true;
            break;
        }
        if (T64 == 0) break;   // the row is empty: every later column is 0
        const int T = (int)T64;
        steps = t + 1;
        int P = 1;
        while (P < T) P <<= 1;   // <= Cpad
        // 2. expand
        for (int k = tid; k < L; k += nt) {
            const int32_t u = rids[k];
            const double val = rvals[k];
            int o = aux[k];
            for (int32_t q = out_ptr[u], qe = out_ptr[u + 1]; q < qe; ++q, ++o) {
                const int32_t v = out_dst[q];
                keys[o] = ((u64)(uint32_t)v << 32) | (u64)(uint32_t)o;
                evals[o] = val * inv[v];
            }
        }
        for (int j = T + tid; j < P; j += nt) keys[j] = ~0ull;
        __syncthreads();
        // 3. sort
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int x = tid; x < (P >> 1); x += nt) {
                    const int i1 = ((x & ~(j - 1)) << 1) | (x & (j - 1)), i2 = i1 | j;
                    const u64 a = keys[i1], b = keys[i2];
                    if ((a > b) == ((i1 & k) == 0)) {
                        keys[i1] = b;
                        keys[i2] = a;
                    }
                }
                __syncthreads();
            }
        // 4. heads of the runs of equal ids, ranked
        if (tid < kWave) {
            int base = 0;
            for (int c = 0; c < T; c += kWave) {
                const int j = c + lane;
                const bool head = j < T && (j == 0 || (keys[j] >> 32) != (keys[j - 1] >> 32));
                const u64 m = __ballot(head);
                if (j < T) aux[j] = head ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
                base += __popcll(m);
            }
            if (tid == 0) {
                s_len = base;
                s_diag = 0.0;
            }
        }
        __syncthreads();
        // 5. run sums, left to right
        for (int j = tid; j < T; j += nt) {
            const int r = aux[j];
            if (r < 0) continue;
            const u64 id = keys[j] >> 32;
            double s = evals[(uint32_t)keys[j]];
            for (int jj = j + 1; jj < T && (keys[jj] >> 32) == id; ++jj) s += evals[(uint32_t)keys[jj]];
            rids[r] = (int32_t)id;
            rvals[r] = s;
            if ((int64_t)id == i) s_diag = s;
        }
        __syncthreads();
        L = s_len;
        if (tid == 0) table[i * pe_dim + t] = s_diag;
    }
    for (int c = steps + tid; c < pe_dim; c += nt) table[i * pe_dim + c] = 0.0;
    if (tid == 0) {
        info[2 * i] = (int32_t)(need < 0x7FFFFFFFll ? need : 0x7FFFFFFFll);
        info[2 * i + 1] = steps;
        if (over) status[0] = 1;   // every overflowing node stores the same word
    }
}

}  // namespace gnnome

extern "C" int gnnome_pagerank_workspace_bytes(int64_t num_nodes, size_t* bytes_host) {
    GN_REQUIRE(num_nodes >= 0 && num_nodes < ((int64_t)1 << 31) && bytes_host, "pagerank_workspace_bytes: bad argument (num_nodes=%lld)",
               (long long)num_nodes);
    *bytes_host = (size_t)2 * (size_t)num_nodes * sizeof(double);
    return GNNOME_OK;
}

extern "C" int gnnome_pagerank_steps_f64(const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_deg, int64_t num_nodes, int pe_dim,
                                         double* table, float* out_f32, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "pagerank_steps: num_nodes=%lld outside [0, 2^31)", (long long)N);
    GN_REQUIRE(pe_dim >= 1 && pe_dim <= 1024, "pagerank_steps: pe_dim=%d outside [1, 1024]", pe_dim);
    if (N == 0) return GNNOME_OK;
    GN_REQUIRE(in_ptr && out_deg && table && workspace, "pagerank_steps: null pointer");
    if (workspace_bytes < (size_t)2 * (size_t)N * sizeof(double)) {
        set_error("pagerank_steps: workspace %zu < %zu bytes", workspace_bytes, (size_t)2 * (size_t)N * sizeof(double));
        return GNNOME_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* y[2] = {(double*)workspace, (double*)workspace + N};
    const dim3 grid((unsigned)((N + kPeThreads - 1) / kPeThreads)), block(kPeThreads);
    hipLaunchKernelGGL(k_pr_init, grid, block, 0, s, out_deg, N, y[0]);
    GN_LAUNCH_CHECK();
    for (int t = 0; t < pe_dim; ++t) {
        hipLaunchKernelGGL(k_pr_step, grid, block, 0, s, in_ptr, in_src, out_deg, N, pe_dim, t, (const double*)y[t & 1], y[(t + 1) & 1], table);
        GN_LAUNCH_CHECK();
    }
    if (out_f32) {
        hipLaunchKernelGGL(k_pe_finish, dim3(pe_grid(N * pe_dim)), block, 0, s, (const double*)table, N * pe_dim, (const int32_t*)nullptr, out_f32,
                           (double*)nullptr);
        GN_LAUNCH_CHECK();
    }
    return GNNOME_OK;
}

extern "C" int gnnome_rw_return_lds_bytes(int capacity, size_t* bytes_host) {
    GN_REQUIRE(capacity >= 1 && capacity <= (1 << 20) && bytes_host, "rw_return_lds_bytes: bad argument (capacity=%d)", capacity);
    *bytes_host = gnnome::rw_lds_bytes(capacity);
    return GNNOME_OK;
}

extern "C" int gnnome_rw_return_workspace_bytes(int64_t num_nodes, int pe_dim, size_t* bytes_host) {
    GN_REQUIRE(num_nodes >= 0 && num_nodes < ((int64_t)1 << 31) && pe_dim >= 1 && pe_dim <= 1024 && bytes_host,
               "rw_return_workspace_bytes: bad argument (num_nodes=%lld, pe_dim=%d)", (long long)num_nodes, pe_dim);
    *bytes_host = (size_t)num_nodes * sizeof(double) * ((size_t)pe_dim + 1);
    return GNNOME_OK;
}

extern "C" int gnnome_rw_return_f64(const int32_t* out_ptr, const int32_t* out_dst, const int32_t* in_deg, int64_t num_nodes, int pe_dim,
                                    int capacity, void* out, int out_is_f64, int32_t* info, int32_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    const int64_t N = num_nodes;
    GN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "rw_return: num_nodes=%lld outside [0, 2^31)", (long long)N);
    GN_REQUIRE(pe_dim >= 1 && pe_dim <= 1024, "rw_return: pe_dim=%d outside [1, 1024]", pe_dim);
    GN_REQUIRE(capacity >= 1 && capacity <= (1 << 20) && rw_lds_bytes(capacity) <= kRwMaxLds,
               "rw_return: capacity=%d needs %zu bytes of LDS per workgroup, a CU has %zu", capacity,
               capacity >= 1 && capacity <= (1 << 20) ? rw_lds_bytes(capacity) : (size_t)0, kRwMaxLds);
    GN_REQUIRE(status, "rw_return: null status");
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (N == 0) return GNNOME_OK;
    GN_REQUIRE(out_ptr && in_deg && out && info && workspace, "rw_return: null pointer");
    const size_t need = (size_t)N * sizeof(double) * ((size_t)pe_dim + 1);
    if (workspace_bytes < need) {
        set_error("rw_return: workspace %zu < %zu bytes", workspace_bytes, need);
        return GNNOME_EWORKSPACE;
    }
    double* inv = (double*)workspace;
    double* table = inv + N;
    const dim3 block(kPeThreads);
    hipLaunchKernelGGL(k_rw_inv, dim3((unsigned)((N + kPeThreads - 1) / kPeThreads)), block, 0, s, in_deg, N, inv);
    GN_LAUNCH_CHECK();
    const size_t lds = rw_lds_bytes(capacity);
    if (lds > 64 * 1024)
        GN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rw_return), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_rw_return, dim3((unsigned)N), dim3(capacity <= kRwOneWaveCapacity ? kWave : kPeThreads), lds, s, out_ptr, out_dst,
                       (const double*)inv, pe_dim, capacity, rw_pow2ceil(capacity), table, info, status);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pe_finish, dim3(pe_grid(N * pe_dim)), block, 0, s, (const double*)table, N * pe_dim, (const int32_t*)status,
                       out_is_f64 ? (float*)nullptr : (float*)out, out_is_f64 ? (double*)out : (double*)nullptr);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
