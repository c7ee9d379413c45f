// gnnome_node_aggregate_in_f32: the ONE gated aggregation of GatedGCN plus the node update, one wave per destination
// node, no atomics.
//
//   s_p   = sigmoid(e[p,:])
//   fwd_i = sum_{p in in(i)} s_p * A2h[src_p,:] / (sum_{p in in(i)} s_p + 1e-6)
//   h'_i  = relu(norm_h(A1h_i + fwd_i)) + h_i
//
// Reference lines replaced: gated_gcn_full.py:212 (sigmoid), :213-214 (DGL gspmm u_mul_e+sum and copy_e+sum on g), :215
// (divide), :217-225 (sum, bn_h, relu, residual) - the GatedGCN layer, which is the symmetric one without A_3 and without
// the pass over dgl.reverse(g).  In-edges of a node are a contiguous run of sorted positions (CSR by dst): the kernel is a
// pure stream over the e rows plus one gathered table, A2h[src].  There is no out-edge half: no out_ptr / out_pos /
// out_dst, no second (scattered) read of e.  Bound: HBM - 1 read of e[E,H] per layer (4*H bytes per edge).
//
// Lane mapping, association and arithmetic are those of node_aggregate.hip for the in-items, which come first in its work
// list: a row of H floats is covered by H/4 lanes holding a float4 each, a wave64 walks G = 64/(H/4) edges at once, item k
// of a node's in-list goes to lane group k mod G within each 64-item batch, is added in ascending order, and the groups are
// combined with the same __shfl_xor tree (group_sum); the same sigmoid4_, the same epilogue.  For every node that the
// symmetric kernel reduces with its single wave (in + out <= its kHubThreshold) the result therefore equals
// gnnome_node_aggregate_f32's with an all-zero A3h table BIT FOR BIT (its bwd term is 0 / (0 + 1e-6) = +0; the "+ 0.0f" of
// the epilogue below is that addend - it turns a -0 sum into the +0 the symmetric kernel leaves).
// tests/test_aggregate_in.py pins this.
//
// Long in-lists (hubs).  Design (b): the node's single wave walks the whole list - no second launch, no scratch, no hub
// list to find, and the result stays a function of the graph alone.  Above kInHubThreshold = 4096 in-edges the wave sums
// in TWO LEVELS: every kInHubBlock = 128 items (two 64-item batches) the per-lane-group sums are added, in block order,
// into a second set of accumulators, which keeps the rounding error of a 10^5-term sum at that of a ~10^3-term one
// (a fixed association, another than the symmetric kernel's chunk partials: hubs are outside the bit-equality above).
// At or below the threshold there is one block: the first-level sums are added to zero, which is exact.
// COST of (b): the wave is alone with its list - about a millisecond per 10^5 in-edges (an ESTIMATE from the per-wave
// row rate of the symmetric kernel, not a measurement), during which the rest of the chip works on the other nodes.
#include "common.h"

namespace gnnome {

constexpr int kAggInThreads = 256;
constexpr int kInHubThreshold = 4096;   // in-edges above which a node's list is summed in two levels
constexpr int kInHubBlock = 128;        // items per first-level block of such a list (a multiple of the 64-item batch)

template <int H>
__device__ __forceinline__ float in_group_sum(float v) {
    // all-reduce over the lane groups (lanes with equal lane % (H/4)): node_aggregate.hip's group_sum
    constexpr int LPR = H / 4;
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

template <int H>
__device__ __forceinline__ float in_row_sum(float v) {
    // all-reduce over the H/4 lanes of one row
    constexpr int LPR = H / 4;
#pragma unroll
    for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// The one exception to "no inline assembly" in this file: an EMPTY asm statement - it emits no instruction - that makes its operand
// opaque to the optimiser, node_aggregate.hip's opaque_.  Without it the compiler hoists the wait for the srt_src load above the e row
// requests of the step; with it the rows go out first.  It orders loads only and cannot change a value.
__device__ __forceinline__ int in_opaque_(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// The gated sums over in-items [lo, hi) of one node (ib: the sorted position of its first in-edge), lane group g taking every
// G-th item of every 64-item batch; per-lane-group partial sums (combine with in_group_sum).  node_aggregate.hip's
// accumulate_items_lean without its out-edge half: the bounds are wave-uniform (scalar loops), the e rows of a step are
// contiguous from a uniform address and are requested BEFORE the wave waits for its srt_src loads (everything that depends
// on them is derived from a copy the compiler cannot hoist), and the table rows are addressed with 32-bit byte offsets
// whenever the step's rows lie below a32_rows = 2^32 / (ldn * 4) (0: never).
template <int H, int U>
__device__ __forceinline__ void accumulate_in_items(const float* __restrict__ e, const float* __restrict__ A2h, int ldn,
                                                    const int32_t* __restrict__ srt_src, int ib, int lo, int hi, int lane, int group, int c,
                                                    f32x4& nf, f32x4& df, uint32_t a32_rows) {
    constexpr int LPR = H / 4, G = 64 / LPR;
    const uint32_t lc = (uint32_t)c * 4, lg = (uint32_t)group * (H * 4) + lc;
    // the value lane `it` holds: `it` is uniform inside a lane group, so with one group (H = 256) it is a scalar read
    auto pick = [&](uint32_t v, int it) -> uint32_t {
        if (G == 1) return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(it));
        return (uint32_t)__builtin_amdgcn_ds_bpermute(it << 2, (int)v);
    };
    auto row32 = [&](const float* tb, uint32_t off) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(tb) + (size_t)(uint32_t)(off + lc));
    };
    auto row64 = [&](const float* tb, uint32_t idx, int stride) -> f32x4 { return *reinterpret_cast<const f32x4*>(tb + (int64_t)(int)idx * stride + c); };
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;   // lane l owns item base + l
        int my_n = 0;
        if (j < hi) my_n = srt_src[ib + j];
        const int m = min(64, hi - base);
        for (int j0 = 0; j0 < m; j0 += G * U) {
            const char* xb = reinterpret_cast<const char*>(e + (int64_t)(ib + base + j0) * H);
            f32x4 x[U], a[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                live[u] = j0 + u * G + group < m;
                x[u] = *reinterpret_cast<const f32x4*>(xb + (size_t)(live[u] ? lg + (uint32_t)(u * G * H * 4) : lc));   // (a dead slot reads item j0)
            }
            const uint32_t nn = (uint32_t)in_opaque_(my_n);
            if (__ballot(nn >= a32_rows) == 0) {
                const uint32_t no = nn * (uint32_t)(ldn * 4);
#pragma unroll
                for (int u = 0; u < U; ++u) a[u] = row32(A2h, pick(no, live[u] ? j0 + u * G + group : j0));
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) a[u] = row64(A2h, pick(nn, live[u] ? j0 + u * G + group : j0), ldn);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (live[u]) {
                    const f32x4 s = sigmoid4_(x[u]);
                    nf += s * a[u];
                    df += s;
                }
            }
        }
    }
}

// One wave per node: the fused inference update.
template <int H, int NORM, int U = (H == 256 ? 2 : 4)>
__global__ __launch_bounds__(kAggInThreads) void k_node_aggregate_in(
    const float* __restrict__ e, int64_t n_end, const float* __restrict__ A1h, const float* __restrict__ A2h, int ldn,
    const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ srt_src, const float* __restrict__ h_in, int ldh,
    float* __restrict__ h_out, const float* __restrict__ scale, const float* __restrict__ shift, int total_blocks, int64_t node0,
    uint32_t a32_rows, int norm_width) {
    constexpr int LPR = H / 4;
    // the wave index read as a scalar: the node and everything loaded through it (the list bounds) live in scalar registers
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = node0 + (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kAggInThreads / 64) + wave;
    if (node >= n_end) return;
    const int group = lane / LPR, c = (lane % LPR) * 4;
    const int ib = in_ptr[node], din = in_ptr[node + 1] - ib;
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(A1h + node * ldn + c);

    f32x4 nf = {0.f, 0.f, 0.f, 0.f}, df = nf;
    const int blk = din > kInHubThreshold ? kInHubBlock : din;   // (one block unless the list is a hub's; wave-uniform)
    for (int blo = 0; blo < din; blo += blk) {
        f32x4 n1 = {0.f, 0.f, 0.f, 0.f}, d1 = n1;
        accumulate_in_items<H, U>(e, A2h, ldn, srt_src, ib, blo, min(din, blo + blk), lane, group, c, n1, d1, a32_rows);
        nf += n1;
        df += d1;
    }

    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float num_f = in_group_sum<H>(nf[k]), den_f = in_group_sum<H>(df[k]);
        v[k] = a1[k] + num_f / (den_f + kAggEps) + 0.0f;   // (+ 0.0f: the symmetric kernel's bwd term with a zero A3h table, see the header)
    }
    if (NORM == GNNOME_NORM_LAYER) {
        // norm_width = H, handed in as a run-time value: the statistics are written exactly as the symmetric kernel writes them for its
        // zero-padded widths (a masked square cannot fuse with the sum), which keeps the two kernels' LayerNorm rows equal bit for bit
        const float inv_w = 1.0f / (float)norm_width;
        const float mean = in_row_sum<H>(v[0] + v[1] + v[2] + v[3]) * inv_w;
        float s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) s2 += (c + k < norm_width) ? (v[k] - mean) * (v[k] - mean) : 0.f;
        const float rstd = rsqrtf(in_row_sum<H>(s2) * inv_w + kNormEps);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (v[k] - mean) * rstd;
    }
    if (group == 0) {
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(h_in + node * ldh + c);
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = relu_keep_nan(v[k] * sc[k] + sh[k]) + hi[k];
        *reinterpret_cast<f32x4*>(h_out + node * H + c) = y;
    }
}

template <int H>
static int launch_agg_in(const float* e, int64_t n_out, const float* A1h, const float* A2h, int ldn, const int32_t* in_ptr, const int32_t* ss,
                         const float* h_in, int ldh, float* h_out, int norm, const float* scale, const float* shift, hipStream_t s,
                         int64_t node_begin, int64_t node_end) {
    if (node_end < 0) node_end = n_out;
    GN_REQUIRE(node_begin >= 0 && node_begin < node_end && node_end <= n_out, "node_aggregate_in: bad node range [%lld, %lld) of %lld",
               (long long)node_begin, (long long)node_end, (long long)n_out);
    const int64_t blocks = (node_end - node_begin + (kAggInThreads / 64) - 1) / (kAggInThreads / 64);
    GN_REQUIRE(blocks < (1ll << 31), "node_aggregate_in: too many nodes");
    // table rows below this index are addressed with 32-bit byte offsets; gnnome_set_tuning(11, 1): none are
    const uint32_t a32_rows = tuning(kTuneAggAddr64) == 1 ? 0u : (uint32_t)((1ull << 32) / ((uint64_t)ldn * 4));
#define GN_AGG_IN_LAUNCH(NORM_)                                                                                                        \
    hipLaunchKernelGGL((k_node_aggregate_in<H, NORM_>), dim3((unsigned)blocks), dim3(kAggInThreads), 0, s, e, node_end, A1h, A2h, ldn, \
                       in_ptr, ss, h_in, ldh, h_out, scale, shift, (int)blocks, node_begin, a32_rows, H)
    if (norm == GNNOME_NORM_AFFINE)
        GN_AGG_IN_LAUNCH(GNNOME_NORM_AFFINE);
    else
        GN_AGG_IN_LAUNCH(GNNOME_NORM_LAYER);
#undef GN_AGG_IN_LAUNCH
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

static int agg_in_dispatch(const char* who, const float* e, int hidden, int64_t n_out, int64_t node_begin, int64_t node_end, const float* A1h,
                           const float* A2h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src, const float* h_in, int ld_h,
                           float* h_out, int norm_kind, const float* norm_scale, const float* norm_shift, void* stream) {
    // e / srt_src may be NULL for a graph without edges (never dereferenced then)
    GN_REQUIRE(A1h && A2h && in_ptr && h_in && h_out && norm_scale && norm_shift, "%s: null pointer", who);
    GN_REQUIRE(norm_kind == GNNOME_NORM_AFFINE || norm_kind == GNNOME_NORM_LAYER, "%s: bad norm_kind %d", who, norm_kind);
    GN_REQUIRE(ld_node >= hidden && ld_node % 4 == 0 && ld_h >= hidden && ld_h % 4 == 0, "%s: bad strides", who);
    GN_REQUIRE(((uintptr_t)A1h % 16 == 0) && ((uintptr_t)A2h % 16 == 0) && ((uintptr_t)h_in % 16 == 0) && ((uintptr_t)h_out % 16 == 0) &&
                   ((uintptr_t)e % 16 == 0) && ((uintptr_t)norm_scale % 16 == 0) && ((uintptr_t)norm_shift % 16 == 0),
               "%s: tensors must be 16-byte aligned", who);
    GN_REQUIRE(h_out != h_in, "%s: h_out must not alias h_in", who);
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 64: return launch_agg_in<64>(e, n_out, A1h, A2h, ld_node, in_ptr, srt_src, h_in, ld_h, h_out, norm_kind, norm_scale, norm_shift, s, node_begin, node_end);
        case 128: return launch_agg_in<128>(e, n_out, A1h, A2h, ld_node, in_ptr, srt_src, h_in, ld_h, h_out, norm_kind, norm_scale, norm_shift, s, node_begin, node_end);
        case 256: return launch_agg_in<256>(e, n_out, A1h, A2h, ld_node, in_ptr, srt_src, h_in, ld_h, h_out, norm_kind, norm_scale, norm_shift, s, node_begin, node_end);
        default: set_error("%s: hidden=%d not in {64,128,256}", who, hidden); return GNNOME_EINVAL;
    }
}

}  // namespace gnnome

extern "C" int gnnome_node_aggregate_in_f32(const float* e, int hidden, int64_t num_nodes_out, const float* A1h, const float* A2h, int ld_node,
                                            const int32_t* in_ptr, const int32_t* srt_src, const float* h_in, int ld_h, float* h_out,
                                            int norm_kind, const float* norm_scale, const float* norm_shift, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0, "node_aggregate_in: negative node count");
    if (num_nodes_out == 0) return GNNOME_OK;
    return agg_in_dispatch("node_aggregate_in", e, hidden, num_nodes_out, 0, -1, A1h, A2h, ld_node, in_ptr, srt_src, h_in, ld_h, h_out, norm_kind,
                           norm_scale, norm_shift, stream);
}

extern "C" int gnnome_node_aggregate_in_range_f32(const float* e, int hidden, int64_t num_nodes_out, int64_t node_begin, int64_t node_end,
                                                  const float* A1h, const float* A2h, int ld_node, const int32_t* in_ptr,
                                                  const int32_t* srt_src, const float* h_in, int ld_h, float* h_out, int norm_kind,
                                                  const float* norm_scale, const float* norm_shift, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out > 0, "node_aggregate_in_range: empty graph");
    GN_REQUIRE(node_end >= 0, "node_aggregate_in_range: bad node range [%lld, %lld) of %lld", (long long)node_begin, (long long)node_end,
               (long long)num_nodes_out);
    return agg_in_dispatch("node_aggregate_in_range", e, hidden, num_nodes_out, node_begin, node_end, A1h, A2h, ld_node, in_ptr, srt_src, h_in, ld_h,
                           h_out, norm_kind, norm_scale, norm_shift, stream);
}
