// gnnome_node_attention_sum_f32: the message passing of the attention baseline - a per-destination, per-head softmax over the neighbour
// list folded into the gather of the neighbours' rows; one wave per destination node, no atomics, no LDS.
//
//   out[i,k,:] = sum_{p in N'(i)} a_{p,k} * feat[nbr_p,k,:] + bias[k,:],   a_{.,k} = softmax_p( leaky_relu(el[nbr_p,k] + er[i,k], slope) )
//
// Reference lines replaced: models/full_graph.py:78-97 builds g' = add_self_loop(g) (directed=True) or
// add_self_loop(add_reverse_edges(g)) (directed=False) and runs DGL's GATConv(H, H, num_heads=3) (layers/processor.py:49-70) on it:
// feat = fc(h) viewed [N,3,H], el = (feat * attn_l).sum(-1), er = (feat * attn_r).sum(-1), an edge softmax of leaky_relu(el[src] + er[dst])
// over every destination's in-edges, the weighted sum of feat[src], plus bias.  This kernel is everything after el / er (which the host
// folds into the projection that makes feat - engine_gat.py).  g' is never built: N'(i) is the node's own row (the loop edge, once more
// where the graph already has one), the contiguous run [in_ptr[i], in_ptr[i+1]) of srt_src and, with out_ptr given, the run
// [out_ptr[i], out_ptr[i+1]) of out_dst - never empty, so every softmax has a term.
//
// TWO PASSES over a node's lists.  Pass one reads only the 16-byte score rows el[nbr,0..3] (three heads and a pad: one load per
// neighbour) and takes the per-head maximum m_k of the scores; pass two reads them again, forms w = exp(s - m_k) <= 1 per (item, head) -
// v_exp_f32 of (s - m) * log2(e) -, sums the weights (the denominator) and the weighted 3H-wide rows (the numerator), both in fp32, and
// divides once per (node, head) at the end.  Pass one is cheap next to the 768 - 3072-byte feature rows of pass two.
//
// Lane mapping: node_neighbour.hip's, three heads deep.  H/4 lanes cover ONE HEAD's H floats of a row as a float4 each and hold three
// of them - the same columns of the three heads, 16-byte loads at c, H + c, 2H + c - so a wave64 walks G = 64/(H/4) rows at once (4, 2, 1)
// with U = 4 rows (12 requests) per lane group in flight.  Lane l of a 64-item batch loads the batch's l-th neighbour id and score row and
// computes its three weights; the lane groups fetch id and weights with ds_bpermute (one group, H = 256: v_readlane).
//
// ASSOCIATION - fixed, a function of the graph alone, so two runs leave equal bits:
//   * the maximum does not depend on an order (NaN scores are skipped by it and caught in pass two, below);
//   * numerator: the accumulators of lane group 0 start at w_self * feat[i], the other groups' at zero; then the in-list, then the
//     out-list.  Item t of a list (ascending sorted position) goes to lane group t mod G of its 64-item batch and is added there in
//     ascending order as fma(w, row, sum);
//   * denominator: lane l sums the weights of the items it loaded (item l of every batch) in ascending order, lane 0 starting at w_self;
//   * a list of more than kAttHubThreshold = 4096 items is summed in TWO LEVELS, numerator and denominator alike: every kAttHubBlock =
//     128 items (two batches) the block's per-lane sums are added, in block order, to the node's.  A shorter list is one block;
//   * the lane groups' numerators and the 64 lanes' denominators are combined with __shfl_xor trees; out = round(num * (1 / den)) + bias, the bias
//     add a rounding of its own, so a call with a bias equals the call without plus the bias bit for bit.
// A node whose N'(i) is its loop alone has w_self = exp2(0) = 1 and den = 1: out = feat[i] + bias bit for bit.
// NaN POLICY: a NaN in el, er or feat of any member of N'(i) leaves a non-finite out[i] for that head (engine.forward_in_range reads a
// NaN row as "left fp16x3's range").  fmaxf drops a NaN score, so the maximum stays that of the others; the NaN then comes back as
// w = exp(NaN - m) = NaN in pass two, into numerator and denominator.  A weight that underflowed to 0 times a NaN row is NaN as well.
// HUBS: a node's single wave walks its whole lists twice - no second launch, no scratch, no hub list.  About three milliseconds per 10^5
// neighbours (an ESTIMATE: three times node_neighbour.hip's per-wave row estimate for the three-heads-wide rows, not a measurement),
// during which the rest of the chip works on the other nodes.
//
// gnnome_node_attention_sum_stats_f32 is the TRAINING FORM: the same kernel template with two more arguments (k_node_attention_sum<H,
// float*, int>) also leaves, per node, the row m0 m1 m2 0 | 1/den0 1/den1 1/den2 0 that the backward (node_attention_bwd.hip)
// recomputes every weight from.  The plain entry's kernels k_node_attention_sum<H> keep their arguments and their code.
//
// gnnome_node_attention_sum_part_f32 / _stats_part_f32 (end of this file): the two forms over the num_nodes_out OWNED rows of one rank's
// shard of a destination-range partition - feat and el tables of num_nodes_local rows, er / out / stats touched below num_nodes_out.  The
// kernel reads its own node's er and writes its own node's out and stats, and reads feat / el wherever a list points, so the part entries
// are these kernels launched over the owned rows: one copy of the row code, and an owned row's bits are the whole-graph entry's.
#include "node_attention.h"   // the constants and the score, shared with node_attention_bwd.hip

namespace gnnome {

// pass one: m <- max(m, scores of the list's items), lane l taking item l of every 64-item batch
__device__ __forceinline__ void att_list_max(const float* __restrict__ el, int ld_el, const int32_t* __restrict__ idx, int len, int lane,
                                             const AttScores& er, float slope, AttScores& m) {
    for (int j = lane; j < len; j += 64) {
        const AttScores s = att_scores(*reinterpret_cast<const f32x4*>(el + (int64_t)idx[j] * ld_el), er, slope);
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) m.v[k] = fmaxf(m.v[k], s.v[k]);
    }
}

// pass two over items [lo, hi) of one list: num[k] += w_k * feat[nbr, k, c..c+3] with lane group g taking every G-th item of every
// 64-item batch, den[k] += w_k on the lane that loaded the item.  The bounds are wave-uniform (scalar loops).
template <int H>
__device__ __forceinline__ void att_accumulate_rows(const float* __restrict__ feat, int ldf, const float* __restrict__ el, int ld_el,
                                                    const int32_t* __restrict__ idx, int lo, int hi, int lane, int group, int c,
                                                    const AttScores& er, const AttScores& m, float slope, f32x4 (&num)[kAttHeads],
                                                    AttScores& den) {
    constexpr int LPR = H / 4, G = 64 / LPR, U = kAttInFlight;
    // the value lane `it` holds: `it` is uniform inside a lane group, so with one group (H = 256) it is a scalar read
    auto pick = [&](int v, int it) -> int {
        if (G == 1) return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(it));
        return __builtin_amdgcn_ds_bpermute(it << 2, v);
    };
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;   // lane l owns item base + l
        int my_n = 0;
        AttScores my_w = {{0.f, 0.f, 0.f}};
        if (j < hi) {
            my_n = idx[j];
            const AttScores s = att_scores(*reinterpret_cast<const f32x4*>(el + (int64_t)my_n * ld_el), er, slope);
#pragma unroll
            for (int k = 0; k < kAttHeads; ++k) {
                my_w.v[k] = __builtin_amdgcn_exp2f((s.v[k] - m.v[k]) * kLog2e);
                den.v[k] += my_w.v[k];
            }
        }
        const int cnt = min(64, hi - base);
        for (int j0 = 0; j0 < cnt; j0 += G * U) {
            f32x4 a[U][kAttHeads];
            float w[U][kAttHeads];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int it = j0 + u * G + group;
                live[u] = it < cnt;
                const int sel = live[u] ? it : j0;   // (a dead slot reads item j0, which exists)
                const float* row = feat + (int64_t)pick(my_n, sel) * ldf + c;
#pragma unroll
                for (int k = 0; k < kAttHeads; ++k) {
                    a[u][k] = *reinterpret_cast<const f32x4*>(row + k * H);
                    w[u][k] = __int_as_float(pick(__float_as_int(my_w.v[k]), sel));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (live[u]) {
#pragma unroll
                    for (int k = 0; k < kAttHeads; ++k) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) num[k][q] = fmaf(w[u][k], a[u][k][q], num[k][q]);
                    }
                }
            }
        }
    }
}

// one list of `len` items into the node's sums: one block, or fixed 128-item blocks above the hub threshold
template <int H>
__device__ __forceinline__ void att_accumulate_list(const float* __restrict__ feat, int ldf, const float* __restrict__ el, int ld_el,
                                                    const int32_t* __restrict__ idx, int len, int lane, int group, int c,
                                                    const AttScores& er, const AttScores& m, float slope, f32x4 (&num)[kAttHeads],
                                                    AttScores& den) {
    const int blk = len > kAttHubThreshold ? kAttHubBlock : len;   // (wave-uniform)
    for (int blo = 0; blo < len; blo += blk) {
        f32x4 pnum[kAttHeads];
        AttScores pden = {{0.f, 0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) pnum[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        att_accumulate_rows<H>(feat, ldf, el, ld_el, idx, blo, min(len, blo + blk), lane, group, c, er, m, slope, pnum, pden);
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) {
            num[k] += pnum[k];
            den.v[k] += pden.v[k];
        }
    }
}

// the statistics row of a node, m0 m1 m2 0 | 1/den0 1/den1 1/den2 0: stored by the training form, which hands in (stats, ld_stats) ...
__device__ __forceinline__ void att_store_stats(int64_t node, const AttScores& m, const AttScores& inv, float* __restrict__ stats, int ld_stats) {
    *reinterpret_cast<f32x4*>(stats + node * ld_stats) = f32x4{m.v[0], m.v[1], m.v[2], 0.f};
    *reinterpret_cast<f32x4*>(stats + node * ld_stats + 4) = f32x4{inv.v[0], inv.v[1], inv.v[2], 0.f};
}
__device__ __forceinline__ void att_store_stats(int64_t, const AttScores&, const AttScores&) {}   // ... and not by the plain form, which has none

// One kernel template for both entries.  Stats... is EMPTY for gnnome_node_attention_sum_f32 - the kernel then has the arguments and the
// code it always had - and (float* stats, int ld_stats) for the training form gnnome_node_attention_sum_stats_f32, whose lane 0 also
// leaves the very maximum and reciprocal that made `out`: out has the bits of the plain form.
template <int H, typename... Stats>
__global__ __launch_bounds__(kAttThreads) void k_node_attention_sum(const float* __restrict__ feat, int ldf, const float* __restrict__ el,
                                                                    int ld_el, const float* __restrict__ er_rows, int ld_er, int64_t num_nodes,
                                                                    const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ srt_src,
                                                                    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst,
                                                                    float slope, const float* __restrict__ bias, float* __restrict__ out, int ldo,
                                                                    int total_blocks, Stats... stats) {
    constexpr bool STATS = sizeof...(Stats) != 0;
    constexpr int LPR = H / 4;
    // the wave index read as a scalar: the node and everything loaded through it (the list bounds, its own score rows) live in scalar registers
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kAttThreads / 64) + wave;
    if (node >= num_nodes) return;
    const int group = lane / LPR, c = (lane % LPR) * 4;

    const int ib = in_ptr[node], din = in_ptr[node + 1] - ib;
    int ob = 0, dout = 0;
    if (out_ptr != nullptr) {   // directed=False: the reverse copies of the node's out-edges
        ob = out_ptr[node];
        dout = out_ptr[node + 1] - ob;
    }
    AttScores er;
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) er.v[k] = er_rows[node * ld_er + k];
    // the loop edge of g': the node's own score
    const AttScores s_self = att_scores(*reinterpret_cast<const f32x4*>(el + node * ld_el), er, slope);

    // pass one: the per-head maximum over N'(i)
    AttScores m;
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) m.v[k] = fmaxf(-INFINITY, s_self.v[k]);
    att_list_max(el, ld_el, srt_src + ib, din, lane, er, slope, m);
    att_list_max(el, ld_el, out_dst + ob, dout, lane, er, slope, m);
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m.v[k] = fmaxf(m.v[k], __shfl_xor(m.v[k], o));
    }

    // pass two: weights, denominator, numerator
    f32x4 num[kAttHeads];
    AttScores den;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
        const float w_self = __builtin_amdgcn_exp2f((s_self.v[k] - m.v[k]) * kLog2e);
        den.v[k] = lane == 0 ? w_self : 0.f;
        num[k] = zero;
        if (group == 0) num[k] = *reinterpret_cast<const f32x4*>(feat + node * ldf + k * H + c) * w_self;
    }
    att_accumulate_list<H>(feat, ldf, el, ld_el, srt_src + ib, din, lane, group, c, er, m, slope, num, den);
    att_accumulate_list<H>(feat, ldf, el, ld_el, out_dst + ob, dout, lane, group, c, er, m, slope, num, den);

#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
        float d = den.v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
        const float inv = 1.0f / d;   // the one division per (node, head)
        if (STATS) den.v[k] = inv;
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float t = num[k][q];
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) t += __shfl_xor(t, o);
            v[q] = __fmul_rn(t, inv);
        }
        if (bias != nullptr) {   // a rounding of its own (never contracted into the product): out with a bias == out without + bias, bit for bit
            const f32x4 b = *reinterpret_cast<const f32x4*>(bias + k * H + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = __fadd_rn(v[q], b[q]);
        }
        if (group == 0) *reinterpret_cast<f32x4*>(out + node * ldo + k * H + c) = v;
    }
    if (STATS && lane == 0) att_store_stats(node, m, den, stats...);   // (den holds the reciprocals by now)
}

template <int H>
static int launch_attention_sum(const float* feat, int ldf, const float* el, int ld_el, const float* er, int ld_er, int64_t n,
                                const int32_t* in_ptr, const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_dst, float slope,
                                const float* bias, float* out, int ldo, float* stats, int ld_stats, hipStream_t s) {
    const int64_t blocks = (n + (kAttThreads / 64) - 1) / (kAttThreads / 64);
    GN_REQUIRE(blocks < (1ll << 31), "node_attention_sum: too many nodes");
    if (stats == nullptr)
        hipLaunchKernelGGL((k_node_attention_sum<H>), dim3((unsigned)blocks), dim3(kAttThreads), 0, s, feat, ldf, el, ld_el, er, ld_er, n, in_ptr,
                           srt_src, out_ptr, out_dst, slope, bias, out, ldo, (int)blocks);
    else
        hipLaunchKernelGGL((k_node_attention_sum<H, float*, int>), dim3((unsigned)blocks), dim3(kAttThreads), 0, s, feat, ldf, el, ld_el, er, ld_er, n,
                           in_ptr, srt_src, out_ptr, out_dst, slope, bias, out, ldo, (int)blocks, stats, ld_stats);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

}  // namespace gnnome

static int attention_sum_checked(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er, int hidden, int heads,
                                 int64_t num_nodes, const int32_t* in_ptr, const int32_t* srt_src, const int32_t* out_ptr,
                                 const int32_t* out_dst, float negative_slope, const float* bias, float* out, int ld_out, bool want_stats,
                                 float* stats, int ld_stats, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes >= 0, "node_attention_sum: negative node count");
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "node_attention_sum: hidden=%d not in {64,128,256}", hidden);
    GN_REQUIRE(heads == kAttHeads, "node_attention_sum: heads=%d, built for %d (layers/processor.py:50)", heads, kAttHeads);
    if (num_nodes == 0) return GNNOME_OK;
    // srt_src / out_dst may be NULL for a graph without edges (never dereferenced then); out_ptr == NULL selects the directed form
    GN_REQUIRE(feat && el && er && in_ptr && out, "node_attention_sum: null pointer");
    const int width = kAttHeads * hidden;
    GN_REQUIRE(ld_feat >= width && ld_feat % 4 == 0 && ld_out >= width && ld_out % 4 == 0, "node_attention_sum: bad strides of feat / out");
    GN_REQUIRE(ld_el >= 4 && ld_el % 4 == 0 && ld_er >= 4 && ld_er % 4 == 0, "node_attention_sum: el and er are rows of 4 floats, row strides multiples of 4");
    GN_REQUIRE(((uintptr_t)feat % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((uintptr_t)el % 16 == 0) && ((uintptr_t)er % 16 == 0) &&
                   ((uintptr_t)bias % 16 == 0),
               "node_attention_sum: feat, el, er, bias and out must be 16-byte aligned");
    GN_REQUIRE(out != feat, "node_attention_sum: out must not alias feat");
    if (want_stats) {
        GN_REQUIRE(stats != nullptr && ld_stats >= kAttStatsRow && ld_stats % 4 == 0 && (uintptr_t)stats % 16 == 0,
                   "node_attention_sum_stats: stats holds rows of 8 floats, 16-byte aligned, row stride a multiple of 4");
        GN_REQUIRE(stats != out && (const float*)stats != feat && (const float*)stats != el && (const float*)stats != er,
                   "node_attention_sum_stats: stats must not alias feat, el, er or out");
    }
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 64:
            return launch_attention_sum<64>(feat, ld_feat, el, ld_el, er, ld_er, num_nodes, in_ptr, srt_src, out_ptr, out_dst, negative_slope,
                                            bias, out, ld_out, stats, ld_stats, s);
        case 128:
            return launch_attention_sum<128>(feat, ld_feat, el, ld_el, er, ld_er, num_nodes, in_ptr, srt_src, out_ptr, out_dst, negative_slope,
                                             bias, out, ld_out, stats, ld_stats, s);
        default:
            return launch_attention_sum<256>(feat, ld_feat, el, ld_el, er, ld_er, num_nodes, in_ptr, srt_src, out_ptr, out_dst, negative_slope,
                                             bias, out, ld_out, stats, ld_stats, s);
    }
}

extern "C" int gnnome_node_attention_sum_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er, int hidden,
                                             int heads, int64_t num_nodes, const int32_t* in_ptr, const int32_t* srt_src,
                                             const int32_t* out_ptr, const int32_t* out_dst, float negative_slope, const float* bias, float* out,
                                             int ld_out, void* stream) {
    return attention_sum_checked(feat, ld_feat, el, ld_el, er, ld_er, hidden, heads, num_nodes, in_ptr, srt_src, out_ptr, out_dst,
                                 negative_slope, bias, out, ld_out, false, nullptr, 0, stream);
}

extern "C" int gnnome_node_attention_sum_stats_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er,
                                                   int hidden, int heads, int64_t num_nodes, const int32_t* in_ptr, const int32_t* srt_src,
                                                   const int32_t* out_ptr, const int32_t* out_dst, float negative_slope, const float* bias,
                                                   float* out, int ld_out, float* stats, int ld_stats, void* stream) {
    return attention_sum_checked(feat, ld_feat, el, ld_el, er, ld_er, hidden, heads, num_nodes, in_ptr, srt_src, out_ptr, out_dst,
                                 negative_slope, bias, out, ld_out, true, stats, ld_stats, stream);
}

// ---------------------------------------------------------------------------------------------------- one rank's shard
// The same two kernels over the num_nodes_out owned rows of a shard (include/gnnome_hip.h, "the attention sum on one rank's shard"): a
// wave reads er, and writes out and stats, at its own node's row - below num_nodes_out - and reads feat / el at whatever local id a list
// names, the halo rows included.  Nothing but the launch bound differs from the whole-graph entries, so the row code is theirs.

extern "C" int gnnome_node_attention_sum_part_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er,
                                                  int hidden, int heads, int64_t num_nodes_out, int64_t num_nodes_local, const int32_t* in_ptr,
                                                  const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_dst, float negative_slope,
                                                  const float* bias, float* out, int ld_out, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0 && num_nodes_out <= num_nodes_local, "node_attention_sum_part: %lld destination rows of %lld local rows",
               (long long)num_nodes_out, (long long)num_nodes_local);
    return attention_sum_checked(feat, ld_feat, el, ld_el, er, ld_er, hidden, heads, num_nodes_out, in_ptr, srt_src, out_ptr, out_dst,
                                 negative_slope, bias, out, ld_out, false, nullptr, 0, stream);
}

extern "C" int gnnome_node_attention_sum_stats_part_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er,
                                                        int hidden, int heads, int64_t num_nodes_out, int64_t num_nodes_local,
                                                        const int32_t* in_ptr, const int32_t* srt_src, const int32_t* out_ptr,
                                                        const int32_t* out_dst, float negative_slope, const float* bias, float* out, int ld_out,
                                                        float* stats, int ld_stats, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0 && num_nodes_out <= num_nodes_local, "node_attention_sum_stats_part: %lld destination rows of %lld local rows",
               (long long)num_nodes_out, (long long)num_nodes_local);
    return attention_sum_checked(feat, ld_feat, el, ld_el, er, ld_er, hidden, heads, num_nodes_out, in_ptr, srt_src, out_ptr, out_dst,
                                 negative_slope, bias, out, ld_out, true, stats, ld_stats, stream);
}
