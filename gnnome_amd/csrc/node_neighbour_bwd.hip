// gnnome_node_neighbour_sum_bwd_f32: the gradient of gnnome_node_neighbour_sum_f32 (node_neighbour.hip) with respect to h, with the
// element-wise work that follows it in the training step of GCNModel / SAGEModel folded into the store - one pass over [N,H] per layer:
//
//   s_j   = rscale_j g_j + sum_{q in out(j)} rscale[dst_q] g[dst_q,:] + [both] sum_{p in in(j)} rscale[src_p] g[src_p,:]
//   v     = oscale_j * s_j           (oscale NULL: v = s_j)
//   v     = add[j,:] + v             (add NULL: skipped)           SAGE: the self path's gradient, the left half of dT
//   v     = v * mult[j,:]            (mult NULL: skipped)          SAGE: feat_drop's scaled keep-mask
//   out_j = y[j,:] > 0 ? v : 0       (y NULL: out_j = v)           the ReLU between two layers; a NaN in y gives 0, as gnnome_relu_bwd_f32 does
//
// rscale is the forward's dscale (a node's gradient reaches every row it summed), oscale the forward's sscale.  Reference lines
// replaced: what torch autograd runs for DGL's GraphConv(norm='both') (layers/processor.py:35-46) and SAGEConv('mean') (:73-84) on
// g' - the transposed gspmm - followed by the backward of feat_drop and of the ReLU of :44 / :82.
//
// LANE MAPPING AND ASSOCIATION: the forward kernel's, from the one copy in node_neighbour.h (stated in node_neighbour.hip's header) -
// one wave per node, lane group 0 starts at the self term, then the OUT-list, then (both) the IN-list; item k of a 64-item batch goes
// to lane group k mod G, ascending, fmaf(rscale, row, sum); lists above 4096 items in 128-item blocks; the __shfl_xor tree combines the
// groups.  No atomics, no scratch, no second launch.  Without an epilogue the result therefore has the bits of the forward kernel
// called on the reversed graph with sscale = rscale, dscale = oscale.
//
// THE EPILOGUE IS FOUR SEPARATE ROUNDINGS in the order above, written with __fmul_rn / __fadd_rn, which the compiler never contracts:
// oscale * s + add is NOT an fma here, so the result equals the four element-wise fp32 passes it replaces bit for bit.
//
// gnnome_node_neighbour_sum_bwd_part_f32: the same on one rank's shard (models/full_graph.py:56-75, :100-119; layers/processor.py:35-46,
// :73-84, per rank), as gnnome_node_neighbour_sum_part_f32: g and rscale have num_nodes_local rows - the halo rows of g FETCHED from their
// owners, a forward-direction exchange -, the epilogue's operands and out the owned rows; all owned rows, or the rows of a list
// (k_node_neighbour_sum_bwd_rows).  The owned nodes' out- and in-lists are complete on the default partition, so no partial sums exist.
//
// gnnome_relu_mul_rows_f32: x <- relu(x) * mult in place on row-strided rows (relu = 0: x <- x * mult), NaN kept - SAGE's feat_drop
// applied where the ReLU already touches the row.  The keep-mask is 0 or 1/(1-p) >= 1, so the stored x_d > 0 exactly where the ReLU
// passed AND the mask kept: the backward gates on the stored row itself (`y` above) and no pre-dropout copy is saved.
#include "node_neighbour.h"

namespace gnnome {

struct NbrBwdArgs {
    const float* g;
    int ldg;
    int64_t n;               // waves: the nodes [0, n), or the n listed rows
    const int32_t* rows;     // NULL, or the row list of gnnome_node_neighbour_sum_bwd_part_f32
    const int32_t *out_ptr, *out_dst, *in_ptr, *srt_src;
    const float *rscale, *oscale, *add;
    int ld_add;
    const float* mult;
    int ld_mult;
    const float* y;
    int ld_y;
    float* out;
    int ldo;
};

// one node's row: the sum of node_neighbour.h, then the epilogue on lane group 0 and its store (node: wave-uniform)
template <int H, bool SS>
__device__ __forceinline__ void neighbour_sum_bwd_row(const float* __restrict__ g, int ldg, int64_t node, const int32_t* __restrict__ out_ptr,
                                                      const int32_t* __restrict__ out_dst, const int32_t* __restrict__ in_ptr,
                                                      const int32_t* __restrict__ srt_src, const float* __restrict__ rscale,
                                                      const float* __restrict__ oscale, const float* add, int ld_add, const float* mult,
                                                      int ld_mult, const float* y, int ld_y, float* out, int ldo, int lane) {
    constexpr int LPR = H / 4;
    const int group = lane / LPR, c = (lane % LPR) * 4;

    f32x4 v = nbr_node_sum<H, SS>(g, ldg, rscale, node, out_ptr, out_dst, in_ptr, srt_src, lane, group, c);
    if (group != 0) return;   // every lane group holds the sum; group 0 runs the epilogue on the node's row and stores it
    if (oscale != nullptr) {
        const float o = oscale[node];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __fmul_rn(o, v[k]);
    }
    if (add != nullptr) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(add + node * ld_add + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __fadd_rn(a[k], v[k]);
    }
    if (mult != nullptr) {
        const f32x4 m = *reinterpret_cast<const f32x4*>(mult + node * ld_mult + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __fmul_rn(v[k], m[k]);
    }
    if (y != nullptr) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(y + node * ld_y + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = t[k] > 0.f ? v[k] : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + node * ldo + c) = v;
}

template <int H, bool SS>
__global__ __launch_bounds__(kNbrThreads) void k_node_neighbour_sum_bwd(const float* __restrict__ g, int ldg, int64_t num_nodes,
                                                                        const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                                                        const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ srt_src,
                                                                        const float* __restrict__ rscale, const float* __restrict__ oscale,
                                                                        const float* add, int ld_add, const float* mult, int ld_mult,
                                                                        const float* y, int ld_y, float* out, int ldo, int total_blocks) {
    // (the wave index as a scalar: see k_node_neighbour_sum)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kNbrThreads / 64) + wave;
    if (node >= num_nodes) return;
    neighbour_sum_bwd_row<H, SS>(g, ldg, node, out_ptr, out_dst, in_ptr, srt_src, rscale, oscale, add, ld_add, mult, ld_mult, y, ld_y, out, ldo, lane);
}

// The row-list form (gnnome_node_neighbour_sum_bwd_part_f32 with rows != NULL): wave w of the launch computes node rows[w], as
// k_node_neighbour_sum_rows does
template <int H, bool SS>
__global__ __launch_bounds__(kNbrThreads) void k_node_neighbour_sum_bwd_rows(const NbrBwdArgs a, int total_blocks) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kNbrThreads / 64) + wave;
    if (w >= a.n) return;
    neighbour_sum_bwd_row<H, SS>(a.g, a.ldg, (int64_t)a.rows[w], a.out_ptr, a.out_dst, a.in_ptr, a.srt_src, a.rscale, a.oscale, a.add, a.ld_add,
                                 a.mult, a.ld_mult, a.y, a.ld_y, a.out, a.ldo, lane);
}

template <int H>
static int launch_neighbour_sum_bwd(const NbrBwdArgs& a, hipStream_t s) {
    const int64_t blocks = (a.n + (kNbrThreads / 64) - 1) / (kNbrThreads / 64);
    GN_REQUIRE(blocks < (1ll << 31), "node_neighbour_sum_bwd: too many nodes");
    if (a.rows != nullptr) {
        if (a.rscale != nullptr)
            hipLaunchKernelGGL((k_node_neighbour_sum_bwd_rows<H, true>), dim3((unsigned)blocks), dim3(kNbrThreads), 0, s, a, (int)blocks);
        else
            hipLaunchKernelGGL((k_node_neighbour_sum_bwd_rows<H, false>), dim3((unsigned)blocks), dim3(kNbrThreads), 0, s, a, (int)blocks);
    } else if (a.rscale != nullptr)
        hipLaunchKernelGGL((k_node_neighbour_sum_bwd<H, true>), dim3((unsigned)blocks), dim3(kNbrThreads), 0, s, a.g, a.ldg, a.n, a.out_ptr, a.out_dst,
                           a.in_ptr, a.srt_src, a.rscale, a.oscale, a.add, a.ld_add, a.mult, a.ld_mult, a.y, a.ld_y, a.out, a.ldo, (int)blocks);
    else
        hipLaunchKernelGGL((k_node_neighbour_sum_bwd<H, false>), dim3((unsigned)blocks), dim3(kNbrThreads), 0, s, a.g, a.ldg, a.n, a.out_ptr, a.out_dst,
                           a.in_ptr, a.srt_src, a.rscale, a.oscale, a.add, a.ld_add, a.mult, a.ld_mult, a.y, a.ld_y, a.out, a.ldo, (int)blocks);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

constexpr int kReluMulThreads = 256;

// x <- relu(x) * mult (RELU) or x * mult on rows of `hidden` floats; NaN stays NaN (relu_keep_nan, and NaN * 0 = NaN)
template <bool RELU>
__global__ __launch_bounds__(kReluMulThreads) void k_relu_mul_rows(float* __restrict__ x, int ld, const float* __restrict__ mult, int ld_mult,
                                                                   int64_t rows, int hidden) {
    const int q = hidden / 4;
    const int64_t total = rows * q;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / q, c = (i % q) * 4;
        f32x4* p = reinterpret_cast<f32x4*>(x + r * ld + c);
        const f32x4 m = *reinterpret_cast<const f32x4*>(mult + r * ld_mult + c);
        f32x4 v = *p;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __fmul_rn(RELU ? relu_keep_nan(v[k]) : v[k], m[k]);
        *p = v;
    }
}

static bool table_ok(const void* p, int ld, int hidden) { return ld >= hidden && ld % 4 == 0 && (uintptr_t)p % 16 == 0; }

}  // namespace gnnome

// what both entries check and launch: `waves` nodes - [0, waves) or the listed rows - of tables with any number of rows
static int neighbour_sum_bwd_entry(const float* g, int ld_g, int hidden, int64_t waves, const int32_t* rows, const int32_t* out_ptr,
                                   const int32_t* out_dst, const int32_t* in_ptr, const int32_t* srt_src, int both, const float* rscale,
                                   const float* oscale, const float* add, int ld_add, const float* mult, int ld_mult, const float* y, int ld_y,
                                   float* out, int ld_out, void* stream) {
    using namespace gnnome;
    // out_dst / srt_src may be NULL for a graph without edges (never dereferenced then); in_ptr is read with `both` only
    GN_REQUIRE(g && out && out_ptr && (!both || in_ptr), "node_neighbour_sum_bwd: null pointer");
    GN_REQUIRE(table_ok(g, ld_g, hidden) && table_ok(out, ld_out, hidden) && (!add || table_ok(add, ld_add, hidden)) &&
                   (!mult || table_ok(mult, ld_mult, hidden)) && (!y || table_ok(y, ld_y, hidden)),
               "node_neighbour_sum_bwd: g, add, mult, y and out are 16-byte aligned tables with row strides >= hidden that are multiples of 4");
    GN_REQUIRE(out != g && out != add, "node_neighbour_sum_bwd: out must not alias g or add");
    const NbrBwdArgs a{g, ld_g, waves, rows, out_ptr, out_dst, both ? in_ptr : nullptr, both ? srt_src : nullptr, rscale, oscale, add, ld_add,
                       mult, ld_mult, y, ld_y, out, ld_out};
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 64: return launch_neighbour_sum_bwd<64>(a, s);
        case 128: return launch_neighbour_sum_bwd<128>(a, s);
        default: return launch_neighbour_sum_bwd<256>(a, s);
    }
}

extern "C" int gnnome_node_neighbour_sum_bwd_f32(const float* g, int ld_g, int hidden, int64_t num_nodes, const int32_t* out_ptr,
                                                 const int32_t* out_dst, const int32_t* in_ptr, const int32_t* srt_src, int both,
                                                 const float* rscale, const float* oscale, const float* add, int ld_add, const float* mult,
                                                 int ld_mult, const float* y, int ld_y, float* out, int ld_out, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes >= 0, "node_neighbour_sum_bwd: negative node count");
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "node_neighbour_sum_bwd: hidden=%d not in {64,128,256}", hidden);
    if (num_nodes == 0) return GNNOME_OK;
    return neighbour_sum_bwd_entry(g, ld_g, hidden, num_nodes, nullptr, out_ptr, out_dst, in_ptr, srt_src, both, rscale, oscale, add, ld_add, mult,
                                   ld_mult, y, ld_y, out, ld_out, stream);
}

// One rank's shard (see gnnome_node_neighbour_sum_part_f32): g and rscale have num_nodes_local rows - the halo rows of g fetched from
// their owners -, the lists num_nodes_local + 1 bounds; oscale, add, mult, y and out are touched at the computed rows (< num_nodes_out) only.
extern "C" int gnnome_node_neighbour_sum_bwd_part_f32(const float* g, int ld_g, int hidden, int64_t num_nodes_out, int64_t num_nodes_local,
                                                      const int32_t* rows, int64_t num_rows, const int32_t* out_ptr, const int32_t* out_dst,
                                                      const int32_t* in_ptr, const int32_t* srt_src, int both, const float* rscale,
                                                      const float* oscale, const float* add, int ld_add, const float* mult, int ld_mult,
                                                      const float* y, int ld_y, float* out, int ld_out, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0 && num_nodes_out <= num_nodes_local, "node_neighbour_sum_bwd_part: %lld destination rows of %lld local rows",
               (long long)num_nodes_out, (long long)num_nodes_local);
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "node_neighbour_sum_bwd_part: hidden=%d not in {64,128,256}", hidden);
    GN_REQUIRE(rows == nullptr || (num_rows >= 0 && num_rows <= num_nodes_out),
               "node_neighbour_sum_bwd_part: %lld listed rows of %lld destination rows", (long long)num_rows, (long long)num_nodes_out);
    const int64_t waves = rows != nullptr ? num_rows : num_nodes_out;
    if (waves == 0) return GNNOME_OK;
    return neighbour_sum_bwd_entry(g, ld_g, hidden, waves, rows, out_ptr, out_dst, in_ptr, srt_src, both, rscale, oscale, add, ld_add, mult,
                                   ld_mult, y, ld_y, out, ld_out, stream);
}

extern "C" int gnnome_relu_mul_rows_f32(float* x, int ld, const float* mult, int ld_mult, int64_t rows, int hidden, int relu, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(rows >= 0 && hidden > 0 && hidden % 4 == 0, "relu_mul_rows: bad shape rows=%lld hidden=%d", (long long)rows, hidden);
    GN_REQUIRE(mult != nullptr || rows == 0, "relu_mul_rows: mult is NULL (gnnome_relu_rows_f32 is the ReLU alone)");
    if (rows == 0) return GNNOME_OK;
    GN_REQUIRE(x && table_ok(x, ld, hidden) && table_ok(mult, ld_mult, hidden) && (const float*)x != mult,
               "relu_mul_rows: x and mult are distinct 16-byte aligned tables, row strides >= hidden and multiples of 4");
    const int64_t total = rows * (hidden / 4), want = (total + kReluMulThreads - 1) / kReluMulThreads;
    const unsigned grid = (unsigned)(want < 65536 ? want : 65536);
    if (relu)
        hipLaunchKernelGGL(k_relu_mul_rows<true>, dim3(grid), dim3(kReluMulThreads), 0, (hipStream_t)stream, x, ld, mult, ld_mult, rows, hidden);
    else
        hipLaunchKernelGGL(k_relu_mul_rows<false>, dim3(grid), dim3(kReluMulThreads), 0, (hipStream_t)stream, x, ld, mult, ld_mult, rows, hidden);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
