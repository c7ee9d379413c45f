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
// gnnome_relu_mul_rows_f32: x <- relu(x) * mult in place on row-strided rows (relu = 0: x <- x * mult), NaN kept - SAGE's feat_drop
// applied where the ReLU already touches the row.  The keep-mask is 0 or 1/(1-p) >= 1, so the stored x_d > 0 exactly where the ReLU
// passed AND the mask kept: the backward gates on the stored row itself (`y` above) and no pre-dropout copy is saved.
#include "node_neighbour.h"

namespace gnnome {

template <int H, bool SS>
__global__ __launch_bounds__(kNbrThreads) void k_node_neighbour_sum_bwd(const float* __restrict__ g, int ldg, int64_t num_nodes,
                                                                        const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                                                        const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ srt_src,
                                                                        const float* __restrict__ rscale, const float* __restrict__ oscale,
                                                                        const float* add, int ld_add, const float* mult, int ld_mult,
                                                                        const float* y, int ld_y, float* out, int ldo, int total_blocks) {
    constexpr int LPR = H / 4;
    // (the wave index as a scalar: see k_node_neighbour_sum)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kNbrThreads / 64) + wave;
    if (node >= num_nodes) return;
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

struct NbrBwdArgs {
    const float* g;
    int ldg;
    int64_t n;
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

template <int H>
static int launch_neighbour_sum_bwd(const NbrBwdArgs& a, hipStream_t s) {
    const int64_t blocks = (a.n + (kNbrThreads / 64) - 1) / (kNbrThreads / 64);
    GN_REQUIRE(blocks < (1ll << 31), "node_neighbour_sum_bwd: too many nodes");
    if (a.rscale != nullptr)
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

extern "C" int gnnome_node_neighbour_sum_bwd_f32(const float* g, int ld_g, int hidden, int64_t num_nodes, const int32_t* out_ptr,
                                                 const int32_t* out_dst, const int32_t* in_ptr, const int32_t* srt_src, int both,
                                                 const float* rscale, const float* oscale, const float* add, int ld_add, const float* mult,
                                                 int ld_mult, const float* y, int ld_y, float* out, int ld_out, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes >= 0, "node_neighbour_sum_bwd: negative node count");
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "node_neighbour_sum_bwd: hidden=%d not in {64,128,256}", hidden);
    if (num_nodes == 0) return GNNOME_OK;
    // out_dst / srt_src may be NULL for a graph without edges (never dereferenced then); in_ptr is read with `both` only
    GN_REQUIRE(g && out && out_ptr && (!both || in_ptr), "node_neighbour_sum_bwd: null pointer");
    GN_REQUIRE(table_ok(g, ld_g, hidden) && table_ok(out, ld_out, hidden) && (!add || table_ok(add, ld_add, hidden)) &&
                   (!mult || table_ok(mult, ld_mult, hidden)) && (!y || table_ok(y, ld_y, hidden)),
               "node_neighbour_sum_bwd: g, add, mult, y and out are 16-byte aligned tables with row strides >= hidden that are multiples of 4");
    GN_REQUIRE(out != g && out != add, "node_neighbour_sum_bwd: out must not alias g or add");
    const NbrBwdArgs a{g, ld_g, num_nodes, out_ptr, out_dst, both ? in_ptr : nullptr, both ? srt_src : nullptr, rscale, oscale, add, ld_add,
                       mult, ld_mult, y, ld_y, out, ld_out};
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 64: return launch_neighbour_sum_bwd<64>(a, s);
        case 128: return launch_neighbour_sum_bwd<128>(a, s);
        default: return launch_neighbour_sum_bwd<256>(a, s);
    }
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
