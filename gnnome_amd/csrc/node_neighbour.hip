// gnnome_node_neighbour_sum_f32: the unweighted, degree-normalised neighbour sum of the two sum / mean baselines, one wave per
// destination node, no atomics.
//
//   out_i = dscale_i * ( sscale_i * h_i + sum_{p in in(i)} sscale[src_p] * h[src_p,:] + [both] sum_{q in out(i)} sscale[dst_q] * h[dst_q,:] )
//
// Reference lines replaced: models/full_graph.py:65-75 and :109-119 build g' = add_self_loop(g) (directed=True) or
// add_self_loop(add_reverse_edges(g)) (directed=False) and run DGL's GraphConv(norm='both') (layers/processor.py:35-46) or
// SAGEConv('mean') (:73-84) on it; the message passing of both is this sum - GraphConv with sscale = dout'^-1/2 and
// dscale = din'^-1/2, SAGEConv with sscale absent and dscale = 1/din'.  g' is never built: the in-edges of a node are a contiguous
// run of srt_src (CSR by dst), its out-edges a contiguous run of out_dst (CSR by src), the loop edge is the node's own row.
// There is no e[E,H] stream here - the kernel is a pure gather of h rows.  Bound: the gather's traffic, (E' + N) H 4 bytes read
// (E' = E, or 2 E with both lists) and N H 4 written; where the rows come from (L2, Infinity Cache, HBM) depends on the numbering.
//
// Lane mapping: node_aggregate_in.hip's.  A row of H floats is covered by H/4 lanes holding a float4 each, a wave64 walks
// G = 64/(H/4) rows at once (U = 4 requests per lane group in flight), lane l of a 64-item batch loads the batch's l-th neighbour
// id (and its sscale), which the lane groups then fetch with ds_bpermute (one group, H = 256: v_readlane).
//
// ASSOCIATION - fixed, a function of the graph alone, so two runs leave equal bits:
//   * the accumulator of lane group 0 starts at the self term sscale_i * h_i, the other groups' at zero;
//   * then the in-list, then (both) the out-list.  Item k of a list (ascending sorted position) goes to lane group k mod G of its
//     64-item batch and is added there in ascending order, as fma(sscale, row, sum) (one rounding per item);
//   * a list of more than kNbrHubThreshold = 4096 items is summed in TWO LEVELS, as node_aggregate_in.hip does: every
//     kNbrHubBlock = 128 items (two batches) the per-group sums of the block are added, in block order, to the node's accumulators,
//     which keeps the rounding error of a 10^5-term sum at that of a ~10^3-term one.  A shorter list is one block;
//   * the G group accumulators are combined with the __shfl_xor tree of in_group_sum, and the result is multiplied by dscale_i.
// HUBS: a node's single wave walks its whole lists - no second launch, no scratch, no hub list.  The wave is alone with them:
// about a millisecond per 10^5 neighbours (an ESTIMATE from node_aggregate_in's per-wave row rate, not a measurement), during which
// the rest of the chip works on the other nodes.
//
// gnnome_node_neighbour_sum_part_f32: the same sum on one rank's shard of a destination-range partition (models/full_graph.py:56-75 and
// :100-119, layers/processor.py:35-46 and :73-84, per rank): tables of num_nodes_local rows, owned rows first; the rows < num_nodes_out
// are computed - all of them by the kernel above, or the rows of a LIST by k_node_neighbour_sum_rows, whose wave takes its node from the
// list instead of the block index (interior rows under the halo exchange, boundary rows after it).  Both run neighbour_sum_row, so a row's
// bits depend on its lists and the table rows they name alone: equal to the whole-graph entry's at any world size and under any split.
//
// gnnome_relu_rows_f32: the ReLU between two layers of those models (processor.py:44, :82), in place on row-strided rows, NaN kept.
#include "node_neighbour.h"   // the lane mapping and the association above, shared with node_neighbour_bwd.hip

namespace gnnome {

// one node's row: the sum of node_neighbour.h, dscale, the store by lane group 0 (node: wave-uniform)
template <int H, bool SS>
__device__ __forceinline__ void neighbour_sum_row(const float* __restrict__ h, int ldh, int64_t node, const int32_t* __restrict__ in_ptr,
                                                  const int32_t* __restrict__ srt_src, const int32_t* __restrict__ out_ptr,
                                                  const int32_t* __restrict__ out_dst, const float* __restrict__ sscale,
                                                  const float* __restrict__ dscale, float* __restrict__ out, int ldo, int lane) {
    constexpr int LPR = H / 4;
    const int group = lane / LPR, c = (lane % LPR) * 4;
    f32x4 v = nbr_node_sum<H, SS>(h, ldh, sscale, node, in_ptr, srt_src, out_ptr, out_dst, lane, group, c);
    if (dscale != nullptr) v *= dscale[node];
    if (group == 0) *reinterpret_cast<f32x4*>(out + node * ldo + c) = v;
}

template <int H, bool SS>
__global__ __launch_bounds__(kNbrThreads) void k_node_neighbour_sum(const float* __restrict__ h, int ldh, int64_t num_nodes,
                                                                    const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ srt_src,
                                                                    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                                                    const float* __restrict__ sscale, const float* __restrict__ dscale,
                                                                    float* __restrict__ out, int ldo, int total_blocks) {
    // the wave index read as a scalar: the node and everything loaded through it (the list bounds, its scales) live in scalar registers
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kNbrThreads / 64) + wave;
    if (node >= num_nodes) return;
    neighbour_sum_row<H, SS>(h, ldh, node, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ldo, lane);
}

// The row-list form (gnnome_node_neighbour_sum_part_f32 with rows != NULL): wave w of the launch computes node rows[w] - a scalar load
// through the wave index - and nothing else; the row's bits depend on its own lists alone, so they are the kernel's above.
template <int H, bool SS>
__global__ __launch_bounds__(kNbrThreads) void k_node_neighbour_sum_rows(const float* __restrict__ h, int ldh, const int32_t* __restrict__ rows,
                                                                         int64_t num_rows, const int32_t* __restrict__ in_ptr,
                                                                         const int32_t* __restrict__ srt_src, const int32_t* __restrict__ out_ptr,
                                                                         const int32_t* __restrict__ out_dst, const float* __restrict__ sscale,
                                                                         const float* __restrict__ dscale, float* __restrict__ out, int ldo,
                                                                         int total_blocks) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t w = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kNbrThreads / 64) + wave;
    if (w >= num_rows) return;
    neighbour_sum_row<H, SS>(h, ldh, (int64_t)rows[w], in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ldo, lane);
}

// n waves: the nodes [0, n) (rows == NULL) or the n listed ones
template <int H>
static int launch_neighbour_sum(const float* h, int ldh, int64_t n, const int32_t* rows, const int32_t* in_ptr, const int32_t* srt_src,
                                const int32_t* out_ptr, const int32_t* out_dst, const float* sscale, const float* dscale, float* out, int ldo,
                                hipStream_t s) {
    const int64_t blocks = (n + (kNbrThreads / 64) - 1) / (kNbrThreads / 64);
    GN_REQUIRE(blocks < (1ll << 31), "node_neighbour_sum: too many nodes");
    const dim3 grid((unsigned)blocks), block(kNbrThreads);
    if (rows != nullptr) {
        if (sscale != nullptr)
            hipLaunchKernelGGL((k_node_neighbour_sum_rows<H, true>), grid, block, 0, s, h, ldh, rows, n, in_ptr, srt_src, out_ptr, out_dst, sscale,
                               dscale, out, ldo, (int)blocks);
        else
            hipLaunchKernelGGL((k_node_neighbour_sum_rows<H, false>), grid, block, 0, s, h, ldh, rows, n, in_ptr, srt_src, out_ptr, out_dst, sscale,
                               dscale, out, ldo, (int)blocks);
    } else if (sscale != nullptr)
        hipLaunchKernelGGL((k_node_neighbour_sum<H, true>), grid, block, 0, s, h, ldh, n, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ldo,
                           (int)blocks);
    else
        hipLaunchKernelGGL((k_node_neighbour_sum<H, false>), grid, block, 0, s, h, ldh, n, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ldo,
                           (int)blocks);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

constexpr int kReluThreads = 256;

// x <- relu(x) on rows of `hidden` floats with row stride ld; NaN stays NaN (relu_keep_nan, see common.h)
__global__ __launch_bounds__(kReluThreads) void k_relu_rows(float* __restrict__ x, int ld, int64_t rows, int hidden) {
    const int q = hidden / 4;
    const int64_t total = rows * q;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4* p = reinterpret_cast<f32x4*>(x + (i / q) * ld + (i % q) * 4);
        f32x4 v = *p;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = relu_keep_nan(v[k]);
        *p = v;
    }
}

}  // namespace gnnome

// what both entries check and launch: `waves` nodes - [0, waves) or the listed rows - of tables with any number of rows
static int neighbour_sum_entry(const float* h, int ld_h, int hidden, int64_t waves, const int32_t* rows, const int32_t* in_ptr,
                               const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_dst, const float* sscale, const float* dscale,
                               float* out, int ld_out, void* stream) {
    using namespace gnnome;
    // srt_src / out_dst may be NULL for a graph without edges (never dereferenced then); out_ptr == NULL selects the directed form
    GN_REQUIRE(h && in_ptr && out, "node_neighbour_sum: null pointer");
    GN_REQUIRE(ld_h >= hidden && ld_h % 4 == 0 && ld_out >= hidden && ld_out % 4 == 0, "node_neighbour_sum: bad strides");
    GN_REQUIRE(((uintptr_t)h % 16 == 0) && ((uintptr_t)out % 16 == 0), "node_neighbour_sum: h and out must be 16-byte aligned");
    GN_REQUIRE(out != h, "node_neighbour_sum: out must not alias h");
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 64: return launch_neighbour_sum<64>(h, ld_h, waves, rows, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ld_out, s);
        case 128: return launch_neighbour_sum<128>(h, ld_h, waves, rows, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ld_out, s);
        default: return launch_neighbour_sum<256>(h, ld_h, waves, rows, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ld_out, s);
    }
}

extern "C" int gnnome_node_neighbour_sum_f32(const float* h, int ld_h, int hidden, int64_t num_nodes, const int32_t* in_ptr,
                                             const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_dst, const float* sscale,
                                             const float* dscale, float* out, int ld_out, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes >= 0, "node_neighbour_sum: negative node count");
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "node_neighbour_sum: hidden=%d not in {64,128,256}", hidden);
    if (num_nodes == 0) return GNNOME_OK;
    return neighbour_sum_entry(h, ld_h, hidden, num_nodes, nullptr, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ld_out, stream);
}

// One rank's shard of a destination-range partition that keeps every edge with an owned end (models/full_graph.py:56-75, :100-119;
// layers/processor.py:35-46, :73-84 per rank): the tables and lists have num_nodes_local rows, owned rows first; rows < num_nodes_out are
// computed - all of them, or the listed ones.  Same kernels' row code, so an owned row has the whole-graph entry's bits (header).
extern "C" int gnnome_node_neighbour_sum_part_f32(const float* h, int ld_h, int hidden, int64_t num_nodes_out, int64_t num_nodes_local,
                                                  const int32_t* rows, int64_t num_rows, const int32_t* in_ptr, const int32_t* srt_src,
                                                  const int32_t* out_ptr, const int32_t* out_dst, const float* sscale, const float* dscale,
                                                  float* out, int ld_out, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0 && num_nodes_out <= num_nodes_local, "node_neighbour_sum_part: %lld destination rows of %lld local rows",
               (long long)num_nodes_out, (long long)num_nodes_local);
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "node_neighbour_sum_part: hidden=%d not in {64,128,256}", hidden);
    GN_REQUIRE(rows == nullptr || (num_rows >= 0 && num_rows <= num_nodes_out), "node_neighbour_sum_part: %lld listed rows of %lld destination rows",
               (long long)num_rows, (long long)num_nodes_out);
    const int64_t waves = rows != nullptr ? num_rows : num_nodes_out;
    if (waves == 0) return GNNOME_OK;
    return neighbour_sum_entry(h, ld_h, hidden, waves, rows, in_ptr, srt_src, out_ptr, out_dst, sscale, dscale, out, ld_out, stream);
}

extern "C" int gnnome_relu_rows_f32(float* x, int ld, int64_t rows, int hidden, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(rows >= 0 && hidden > 0 && hidden % 4 == 0, "relu_rows: bad shape rows=%lld hidden=%d", (long long)rows, hidden);
    if (rows == 0) return GNNOME_OK;
    GN_REQUIRE(x && ld >= hidden && ld % 4 == 0 && (uintptr_t)x % 16 == 0, "relu_rows: x must be a 16-byte aligned table, row stride a multiple of 4");
    const int64_t total = rows * (hidden / 4);
    const unsigned grid = (unsigned)((total + kReluThreads - 1) / kReluThreads < 65536 ? (total + kReluThreads - 1) / kReluThreads : 65536);
    hipLaunchKernelGGL(k_relu_rows, dim3(grid), dim3(kReluThreads), 0, (hipStream_t)stream, x, ld, rows, hidden);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
