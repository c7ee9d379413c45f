// gnnome_node_attention_sum_bwd_f32: the gradient of gnnome_node_attention_sum_f32 (node_attention.hip) with respect to feat, el and er -
// what torch autograd runs for DGL's GATConv (layers/processor.py:49-70: the backward of edge_softmax, of leaky_relu, of u_add_v and of
// u_mul_e_sum) on g', which is never built.  Per head k, with G = d out [N,3H], for every edge p = (j -> i) of g', loops included:
//
//   x_p = el[j,k] + er[i,k]     a_p = exp2((leaky_relu(x_p) - m[i,k]) * log2e) * inv_den[i,k]          (m, inv_den: the forward's, `stats`)
//   D[i,k]      = G[i,k,:] . (out[i,k,:] - bias[k,:])                                                   = sum_q a_q (G_i . feat_q)
//   dx_p        = a_p * (x_p > 0 ? 1 : slope) * (G[i,k,:] . feat[j,k,:] - D[i,k])
//   dfeat[j,k,:] = sum_{p: src(p) = j} a_p G[dst(p),k,:]      del[j,k] = sum_{p: src(p) = j} dx_p      der[i,k] = sum_{p: dst(p) = i} dx_p
//
// (d bias = the column sums of G: gnnome_colsum2_f32, not here.)
//
// DECOMPOSITION: TWO launches, one wave per node each, and NO per-edge table.
//   k_att_bwd_dst<H>, one wave per DESTINATION i: D[i] from the rows G_i and out_i - bias; then the forward's walk over N'(i) (the loop,
//     the in-list, with `both` the out-list) with G_i in registers: per item the neighbour's feat row, the three dots, dx; der[i] is their
//     sum.  It also packs what the second kernel needs of a destination into ONE 64-byte row of `work`: er | m | inv_den | D (4 floats each).
//   k_att_bwd_src<H>, one wave per SOURCE j: feat_j and el_j in registers, it walks the TRANSPOSED neighbourhood (the loop, the out-list,
//     with `both` the in-list); per item the destination's 64-byte row (one cache line) and its G row, the three dots again, a and dx;
//     dfeat[j] += a G_i, del[j] += dx.
// The alternative - dx stored once per edge by the source walk (16 bytes at the edge's sorted position, a second table for the reverse
// copies) and summed per destination by a third kernel - reads every feat row once less but needs 32 bytes per edge of scratch and the
// map from out-list to in-list positions, which views of a reversed graph do not carry in the direction that walk needs.  Here both walks
// read (list pointer, neighbour id) pairs only, so reversed views are the swapped lists and nothing else; the price is that the dots are
// formed twice, i.e. one more gather of the 3H-wide rows.  MEASURED (profiles/attention_sum_bwd_time.txt): the two launches together
// cost 2.1 - 2.6 forward calls (1M edges, H = 128: 0.456 ms directed, 0.741 ms both lists; 2.5M edges, H = 256: 1.521 / 2.457 ms),
// 10 - 18 times faster than torch autograd over the torch composition.  The three-kernel alternative was not built and is not measured;
// it could save at most the destination walk (about one forward call of the above).
//
// LANE MAPPING: node_attention.hip's - H/4 lanes hold one head's H floats of a row as a float4 each, three heads deep; G = 64/(H/4) rows
// at once, U = 4 rows per lane group in flight; lane l of a 64-item batch loads the batch's l-th id, its score (or 64-byte) row and forms
// its weights, the lane groups fetch them with ds_bpermute (one group: v_readlane).  The three dots are reduced inside the lane group with
// an __shfl_xor tree over its H/4 lanes.
// ASSOCIATION - fixed, a function of the graph alone; no atomics, no LDS, no scratch list, fp32 throughout:
//   * a dot: each lane's four products in column order (one product, three fma), then the tree over the group's lanes;
//   * a LIST's sum (the in-list or the out-list; above 4096 items: each 128-item block of it) starts at ZERO in every lane group.  Item t
//     of a 64-item batch goes to lane group t mod G and is added there in ascending order (dfeat: fma(a, row, sum); del, der: sum += dx);
//   * the node's running sums (der; dfeat and del) start, in lane group 0, at the loop's term and at zero in the other groups; to them
//     are ADDED, group by group, the completed sums of the first list and then of the second - a list above 4096 items block by block in
//     block order.  The loop's term is therefore added to finished list sums; it is not threaded through a list;
//   * the lane groups' sums are combined with __shfl_xor trees.
// A node without edges has a_loop = exp2(0) * (1 / 1) = 1: dfeat[j] = G[j] bit for bit.  Every output is linear in G through products
// and sums only, so scaling G by a power of two scales them exactly.  del and der are rows of 4 floats with pad column 0 WRITTEN; the
// kernels write nothing else: where dfeat | del | der are the column blocks of a [N, 3H + 64] table laid out like the projection, the
// remaining 56 score columns are ZEROED BY THE HOST (ops.node_attention_sum_bwd, engine_gat's step: once per table).
// HUBS: walked by their own wave in both kernels, as in the forward: about three milliseconds per 10^5 items per walk (the forward's
// ESTIMATE, not a measurement).
//
// gnnome_node_attention_sum_bwd_dst_part_f32 / _bwd_src_part_f32: the two launches as SEPARATE entries over the owned rows of one rank's
// shard of a destination-range partition (the default one: both lists of an owned node complete, in the whole graph's order).  The
// destination walk needs g, out, stats and er of its own node only and feat / el of the neighbours - local rows, halo included; the source
// walk needs g and the 64-byte work row of every DESTINATION its node points at, and a halo destination's are its owner's: the caller
// fetches the halo rows of g (under the destination phase, which does not read them) and of work between the two entries.  Both entries
// launch the kernels below with num_nodes = the owned rows - no second statement of the row code, so an owned row has the whole-graph
// entry's bits, and the two phases on a whole table are that entry, work included.  Every edge's term of dfeat[j] / del[j] is computed
// by j's owner and its term of der[i] by i's: nothing is summed across ranks.
#include "node_attention.h"

namespace gnnome {

constexpr int kAttWorkRow = 16;   // floats per destination of `work`: er(3) 0 | m(3) 0 | inv_den(3) 0 | D(3) 0

// a = softmax weight of the item from its pre-activation x and the destination's statistics (the forward's operations: att_scores'
// leaky_relu, exp2 of (s - m) * log2e; then the stored reciprocal), ag = a * d leaky_relu / dx
__device__ __forceinline__ void att_weight(float x, float m, float inv, float slope, float& a, float& ag) {
    const float s = x > 0.f ? x : slope * x;
    a = __builtin_amdgcn_exp2f((s - m) * kLog2e) * inv;
    ag = x > 0.f ? a : slope * a;
}

// the three per-head dots of two rows held like the forward's (a float4 per head and lane), summed over the lane group: every lane of
// the group gets them.  Executed by whole waves only (the tree is a cross-lane read).
template <int LPR>
__device__ __forceinline__ AttScores att_group_dots(const f32x4 (&r)[kAttHeads], const f32x4 (&x)[kAttHeads]) {
    AttScores d;
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
        float t = r[k][0] * x[k][0];
#pragma unroll
        for (int q = 1; q < 4; ++q) t = fmaf(r[k][q], x[k][q], t);
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) t += __shfl_xor(t, o);
        d.v[k] = t;
    }
    return d;
}

template <int H>
__device__ __forceinline__ int att_pick(int v, int it) {   // the value lane `it` holds; `it` is uniform inside a lane group
    if (H == 256) return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(it));
    return __builtin_amdgcn_ds_bpermute(it << 2, v);
}

// ---------------------------------------------------------------------------------------------------- per destination: D, der, work

// items [lo, hi) of one list of neighbour (source) ids: der[k] += dx of every item, lane group g taking every G-th item of a batch
template <int H>
__device__ __forceinline__ void attb_dst_rows(const float* __restrict__ feat, int ldf, const float* __restrict__ el, int ld_el,
                                              const int32_t* __restrict__ idx, int lo, int hi, int lane, int group, int c, const AttScores& er,
                                              const AttScores& m, const AttScores& inv, const AttScores& D, float slope,
                                              const f32x4 (&g)[kAttHeads], AttScores& der) {
    constexpr int LPR = H / 4, G = 64 / LPR, U = kAttInFlight;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;   // lane l owns item base + l
        int my_n = 0;
        AttScores my_ag = {{0.f, 0.f, 0.f}};
        if (j < hi) {
            my_n = idx[j];
            const f32x4 e = *reinterpret_cast<const f32x4*>(el + (int64_t)my_n * ld_el);
#pragma unroll
            for (int k = 0; k < kAttHeads; ++k) {
                float a;
                att_weight(e[k] + er.v[k], m.v[k], inv.v[k], slope, a, my_ag.v[k]);
            }
        }
        const int cnt = min(64, hi - base);
        for (int j0 = 0; j0 < cnt; j0 += G * U) {
            f32x4 x[U][kAttHeads];
            float ag[U][kAttHeads];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int it = j0 + u * G + group;
                live[u] = it < cnt;
                const int sel = live[u] ? it : j0;   // (a dead slot reads item j0, which exists)
                const float* row = feat + (int64_t)att_pick<H>(my_n, sel) * ldf + c;
#pragma unroll
                for (int k = 0; k < kAttHeads; ++k) {
                    x[u][k] = *reinterpret_cast<const f32x4*>(row + k * H);
                    ag[u][k] = __int_as_float(att_pick<H>(__float_as_int(my_ag.v[k]), sel));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const AttScores d = att_group_dots<LPR>(g, x[u]);
                if (live[u]) {
#pragma unroll
                    for (int k = 0; k < kAttHeads; ++k) der.v[k] += ag[u][k] * (d.v[k] - D.v[k]);
                }
            }
        }
    }
}

template <int H>
__device__ __forceinline__ void attb_dst_list(const float* __restrict__ feat, int ldf, const float* __restrict__ el, int ld_el,
                                              const int32_t* __restrict__ idx, int len, int lane, int group, int c, const AttScores& er,
                                              const AttScores& m, const AttScores& inv, const AttScores& D, float slope,
                                              const f32x4 (&g)[kAttHeads], AttScores& der) {
    const int blk = len > kAttHubThreshold ? kAttHubBlock : len;   // (wave-uniform)
    for (int blo = 0; blo < len; blo += blk) {
        AttScores pder = {{0.f, 0.f, 0.f}};
        attb_dst_rows<H>(feat, ldf, el, ld_el, idx, blo, min(len, blo + blk), lane, group, c, er, m, inv, D, slope, g, pder);
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) der.v[k] += pder.v[k];
    }
}

template <int H>
__global__ __launch_bounds__(kAttThreads) void k_att_bwd_dst(const float* __restrict__ gr, int ldg, const float* __restrict__ feat, int ldf,
                                                             const float* __restrict__ el, int ld_el, const float* __restrict__ er_rows, int ld_er,
                                                             const float* __restrict__ out, int ldo, const float* __restrict__ bias,
                                                             const float* __restrict__ stats, int ld_stats, int64_t num_nodes,
                                                             const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ srt_src,
                                                             const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst, float slope,
                                                             float* __restrict__ der_rows, int ld_der, float* __restrict__ work,
                                                             int total_blocks) {
    constexpr int LPR = H / 4;
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
    AttScores er, m, inv;
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
        er.v[k] = er_rows[node * ld_er + k];
        m.v[k] = stats[node * ld_stats + k];
        inv.v[k] = stats[node * ld_stats + 4 + k];
    }
    // G_i stays in registers; D = G_i . (out_i - bias), the subtraction a rounding of its own (the forward's bias add undone)
    f32x4 g[kAttHeads], t[kAttHeads];
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
        g[k] = *reinterpret_cast<const f32x4*>(gr + node * ldg + k * H + c);
        t[k] = *reinterpret_cast<const f32x4*>(out + node * ldo + k * H + c);
        if (bias != nullptr) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(bias + k * H + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) t[k][q] = __fsub_rn(t[k][q], b[q]);
        }
    }
    const AttScores D = att_group_dots<LPR>(g, t);

    // the loop edge of g'
    AttScores der;
    {
        const f32x4 e = *reinterpret_cast<const f32x4*>(el + node * ld_el);
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) t[k] = *reinterpret_cast<const f32x4*>(feat + node * ldf + k * H + c);
        const AttScores d = att_group_dots<LPR>(g, t);
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) {
            float a, ag;
            att_weight(e[k] + er.v[k], m.v[k], inv.v[k], slope, a, ag);
            const float dx = ag * (d.v[k] - D.v[k]);
            der.v[k] = group == 0 ? dx : 0.f;
        }
    }
    attb_dst_list<H>(feat, ldf, el, ld_el, srt_src + ib, din, lane, group, c, er, m, inv, D, slope, g, der);
    attb_dst_list<H>(feat, ldf, el, ld_el, out_dst + ob, dout, lane, group, c, er, m, inv, D, slope, g, der);

#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
#pragma unroll
        for (int o = LPR; o < 64; o <<= 1) der.v[k] += __shfl_xor(der.v[k], o);
    }
    if (lane == 0) {
        *reinterpret_cast<f32x4*>(der_rows + node * ld_der) = f32x4{der.v[0], der.v[1], der.v[2], 0.f};
        float* w = work + node * kAttWorkRow;
        *reinterpret_cast<f32x4*>(w) = f32x4{er.v[0], er.v[1], er.v[2], 0.f};
        *reinterpret_cast<f32x4*>(w + 4) = f32x4{m.v[0], m.v[1], m.v[2], 0.f};
        *reinterpret_cast<f32x4*>(w + 8) = f32x4{inv.v[0], inv.v[1], inv.v[2], 0.f};
        *reinterpret_cast<f32x4*>(w + 12) = f32x4{D.v[0], D.v[1], D.v[2], 0.f};
    }
}

// ---------------------------------------------------------------------------------------------------- per source: dfeat, del

// items [lo, hi) of one list of destination ids: num[k] += a * G[dst, k, c..c+3], del[k] += dx
template <int H>
__device__ __forceinline__ void attb_src_rows(const float* __restrict__ gr, int ldg, const float* __restrict__ work,
                                              const int32_t* __restrict__ idx, int lo, int hi, int lane, int group, int c, const AttScores& elj,
                                              float slope, const f32x4 (&f)[kAttHeads], f32x4 (&num)[kAttHeads], AttScores& del) {
    constexpr int LPR = H / 4, G = 64 / LPR, U = kAttInFlight;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;   // lane l owns item base + l
        int my_n = 0;
        AttScores my_a = {{0.f, 0.f, 0.f}}, my_ag = {{0.f, 0.f, 0.f}}, my_D = {{0.f, 0.f, 0.f}};
        if (j < hi) {
            my_n = idx[j];
            const float* w = work + (int64_t)my_n * kAttWorkRow;   // the destination's 64-byte row
            const f32x4 er4 = *reinterpret_cast<const f32x4*>(w), m4 = *reinterpret_cast<const f32x4*>(w + 4),
                        i4 = *reinterpret_cast<const f32x4*>(w + 8), D4 = *reinterpret_cast<const f32x4*>(w + 12);
#pragma unroll
            for (int k = 0; k < kAttHeads; ++k) {
                att_weight(elj.v[k] + er4[k], m4[k], i4[k], slope, my_a.v[k], my_ag.v[k]);
                my_D.v[k] = D4[k];
            }
        }
        const int cnt = min(64, hi - base);
        for (int j0 = 0; j0 < cnt; j0 += G * U) {
            f32x4 x[U][kAttHeads];
            float a[U][kAttHeads], ag[U][kAttHeads], Dd[U][kAttHeads];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int it = j0 + u * G + group;
                live[u] = it < cnt;
                const int sel = live[u] ? it : j0;   // (a dead slot reads item j0, which exists)
                const float* row = gr + (int64_t)att_pick<H>(my_n, sel) * ldg + c;
#pragma unroll
                for (int k = 0; k < kAttHeads; ++k) {
                    x[u][k] = *reinterpret_cast<const f32x4*>(row + k * H);
                    a[u][k] = __int_as_float(att_pick<H>(__float_as_int(my_a.v[k]), sel));
                    ag[u][k] = __int_as_float(att_pick<H>(__float_as_int(my_ag.v[k]), sel));
                    Dd[u][k] = __int_as_float(att_pick<H>(__float_as_int(my_D.v[k]), sel));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const AttScores d = att_group_dots<LPR>(f, x[u]);
                if (live[u]) {
#pragma unroll
                    for (int k = 0; k < kAttHeads; ++k) {
                        del.v[k] += ag[u][k] * (d.v[k] - Dd[u][k]);
#pragma unroll
                        for (int q = 0; q < 4; ++q) num[k][q] = fmaf(a[u][k], x[u][k][q], num[k][q]);
                    }
                }
            }
        }
    }
}

template <int H>
__device__ __forceinline__ void attb_src_list(const float* __restrict__ gr, int ldg, const float* __restrict__ work,
                                              const int32_t* __restrict__ idx, int len, int lane, int group, int c, const AttScores& elj,
                                              float slope, const f32x4 (&f)[kAttHeads], f32x4 (&num)[kAttHeads], AttScores& del) {
    const int blk = len > kAttHubThreshold ? kAttHubBlock : len;   // (wave-uniform)
    for (int blo = 0; blo < len; blo += blk) {
        f32x4 pnum[kAttHeads];
        AttScores pdel = {{0.f, 0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) pnum[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        attb_src_rows<H>(gr, ldg, work, idx, blo, min(len, blo + blk), lane, group, c, elj, slope, f, pnum, pdel);
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) {
            num[k] += pnum[k];
            del.v[k] += pdel.v[k];
        }
    }
}

template <int H>
__global__ __launch_bounds__(kAttThreads) void k_att_bwd_src(const float* __restrict__ gr, int ldg, const float* __restrict__ feat, int ldf,
                                                             const float* __restrict__ el, int ld_el, const float* __restrict__ work,
                                                             int64_t num_nodes, const int32_t* __restrict__ out_ptr,
                                                             const int32_t* __restrict__ out_dst, const int32_t* __restrict__ in_ptr,
                                                             const int32_t* __restrict__ srt_src, float slope, float* __restrict__ dfeat,
                                                             int ld_dfeat, float* __restrict__ del_rows, int ld_del, int total_blocks) {
    constexpr int LPR = H / 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kAttThreads / 64) + wave;
    if (node >= num_nodes) return;
    const int group = lane / LPR, c = (lane % LPR) * 4;

    const int ob = out_ptr[node], dout = out_ptr[node + 1] - ob;
    int ib = 0, din = 0;
    if (in_ptr != nullptr) {   // directed=False: the node is the source of the reverse copies of its in-edges
        ib = in_ptr[node];
        din = in_ptr[node + 1] - ib;
    }
    AttScores elj;
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) elj.v[k] = el[node * ld_el + k];
    f32x4 f[kAttHeads], num[kAttHeads];
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) f[k] = *reinterpret_cast<const f32x4*>(feat + node * ldf + k * H + c);

    // the loop edge of g': the node as its own destination
    AttScores del;
    {
        const float* w = work + node * kAttWorkRow;
        f32x4 x[kAttHeads];
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) x[k] = *reinterpret_cast<const f32x4*>(gr + node * ldg + k * H + c);
        const AttScores d = att_group_dots<LPR>(f, x);
#pragma unroll
        for (int k = 0; k < kAttHeads; ++k) {
            float a, ag;
            att_weight(elj.v[k] + w[k], w[4 + k], w[8 + k], slope, a, ag);
            const float dx = ag * (d.v[k] - w[12 + k]);
            del.v[k] = group == 0 ? dx : 0.f;
            num[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (group == 0) num[k] = x[k] * a;
        }
    }
    attb_src_list<H>(gr, ldg, work, out_dst + ob, dout, lane, group, c, elj, slope, f, num, del);
    attb_src_list<H>(gr, ldg, work, srt_src + ib, din, lane, group, c, elj, slope, f, num, del);

#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
#pragma unroll
        for (int o = LPR; o < 64; o <<= 1) del.v[k] += __shfl_xor(del.v[k], o);
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float t = num[k][q];
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) t += __shfl_xor(t, o);
            v[q] = t;
        }
        if (group == 0) *reinterpret_cast<f32x4*>(dfeat + node * ld_dfeat + k * H + c) = v;
    }
    if (lane == 0) *reinterpret_cast<f32x4*>(del_rows + node * ld_del) = f32x4{del.v[0], del.v[1], del.v[2], 0.f};
}

struct AttBwdArgs {
    const float* g;
    int ldg;
    const float* feat;
    int ldf;
    const float* el;
    int ld_el;
    const float* er;
    int ld_er;
    const float* out;
    int ldo;
    const float *bias, *stats;
    int ld_stats;
    int64_t n;
    const int32_t *in_ptr, *srt_src, *out_ptr, *out_dst;
    bool both;
    float slope;
    float* dfeat;
    int ld_dfeat;
    float* del;
    int ld_del;
    float* der;
    int ld_der;
    float* work;
};

constexpr int kAttPhaseDst = 1, kAttPhaseSrc = 2;   // the two launches; the whole-graph entry runs both, a part entry one

// a.n = the rows computed (one wave each): every node for the whole-graph entry, the owned rows of a shard for the part entries - the same
// two kernels either way, which index feat / el (and, the source walk, g / work) at whatever local row a list names
template <int H>
static int launch_attention_sum_bwd(const AttBwdArgs& a, int phases, hipStream_t s) {
    const int64_t blocks = (a.n + (kAttThreads / 64) - 1) / (kAttThreads / 64);
    GN_REQUIRE(blocks < (1ll << 31), "node_attention_sum_bwd: too many nodes");
    if (phases & kAttPhaseDst) {
        hipLaunchKernelGGL((k_att_bwd_dst<H>), dim3((unsigned)blocks), dim3(kAttThreads), 0, s, a.g, a.ldg, a.feat, a.ldf, a.el, a.ld_el, a.er,
                           a.ld_er, a.out, a.ldo, a.bias, a.stats, a.ld_stats, a.n, a.in_ptr, a.srt_src, a.both ? a.out_ptr : nullptr,
                           a.both ? a.out_dst : nullptr, a.slope, a.der, a.ld_der, a.work, (int)blocks);
        GN_LAUNCH_CHECK();
    }
    if (phases & kAttPhaseSrc) {
        hipLaunchKernelGGL((k_att_bwd_src<H>), dim3((unsigned)blocks), dim3(kAttThreads), 0, s, a.g, a.ldg, a.feat, a.ldf, a.el, a.ld_el, a.work,
                           a.n, a.out_ptr, a.out_dst, a.both ? a.in_ptr : nullptr, a.both ? a.srt_src : nullptr, a.slope, a.dfeat, a.ld_dfeat,
                           a.del, a.ld_del, (int)blocks);
        GN_LAUNCH_CHECK();
    }
    return GNNOME_OK;
}

}  // namespace gnnome

// The argument checks of the three entries, then the launch(es).  `what` names the entry in the error text; a phase that does not read or
// write a table is not asked for it (its pointer is NULL and its stride unused).
static int attention_sum_bwd_checked(const gnnome::AttBwdArgs& a, int hidden, int heads, int phases, const char* what, void* stream) {
    using namespace gnnome;
    const bool dst = phases & kAttPhaseDst, src = phases & kAttPhaseSrc;
    GN_REQUIRE(a.n >= 0, "%s: negative node count", what);
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "%s: hidden=%d not in {64,128,256}", what, hidden);
    GN_REQUIRE(heads == kAttHeads, "%s: heads=%d, built for %d (layers/processor.py:50)", what, heads, kAttHeads);
    if (a.n == 0) return GNNOME_OK;
    // both walks need both pointer arrays (the destination walk reads the in-list, the source walk the out-list), so `both` is a flag
    // here and not a NULL out_ptr; srt_src / out_dst may be NULL for a graph without edges (never dereferenced then)
    GN_REQUIRE(a.g && a.feat && a.el && a.work && (dst ? a.in_ptr != nullptr : a.out_ptr != nullptr), "%s: null pointer", what);
    GN_REQUIRE(!a.both || (a.in_ptr && a.out_ptr), "%s: null pointer", what);
    if (dst) GN_REQUIRE(a.er && a.out && a.stats && a.der, "%s: null pointer", what);
    if (src) GN_REQUIRE(a.out_ptr && a.dfeat && a.del, "%s: null pointer", what);
    const int width = kAttHeads * hidden;
    GN_REQUIRE(a.ldg >= width && a.ldg % 4 == 0 && a.ldf >= width && a.ldf % 4 == 0 && (!dst || (a.ldo >= width && a.ldo % 4 == 0)) &&
                   (!src || (a.ld_dfeat >= width && a.ld_dfeat % 4 == 0)),
               "%s: bad strides of g / feat / out / dfeat (>= 3 * hidden, multiples of 4)", what);
    GN_REQUIRE(a.ld_el >= 4 && a.ld_el % 4 == 0 && (!dst || (a.ld_er >= 4 && a.ld_er % 4 == 0 && a.ld_der >= 4 && a.ld_der % 4 == 0 &&
                                                              a.ld_stats >= kAttStatsRow && a.ld_stats % 4 == 0)) &&
                   (!src || (a.ld_del >= 4 && a.ld_del % 4 == 0)),
               "%s: el, er, del and der are rows of 4 floats, stats rows of 8, row strides multiples of 4", what);
    const void* all[] = {a.g, a.feat, a.el, a.er, a.out, a.bias, a.stats, a.dfeat, a.del, a.der, a.work};
    for (const void* p : all) GN_REQUIRE((uintptr_t)p % 16 == 0, "%s: every table must be 16-byte aligned", what);
    // (the source phase READS work: it is an output of the destination phase alone)
    const void* ins[] = {a.g, a.feat, a.el, a.er, a.out, a.stats, a.bias, dst ? nullptr : (const void*)a.work};
    const void* outs[] = {a.dfeat, a.del, a.der, dst ? (const void*)a.work : nullptr};
    for (int i = 0; i < 4; ++i) {
        if (outs[i] == nullptr) continue;
        for (const void* p : ins) GN_REQUIRE(outs[i] != p, "%s: an output must not alias an input", what);
        for (int k = i + 1; k < 4; ++k) GN_REQUIRE(outs[i] != outs[k], "%s: the outputs must not alias each other", what);
    }
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 64: return launch_attention_sum_bwd<64>(a, phases, s);
        case 128: return launch_attention_sum_bwd<128>(a, phases, s);
        default: return launch_attention_sum_bwd<256>(a, phases, s);
    }
}

extern "C" int gnnome_node_attention_sum_bwd_f32(const float* g, int ld_g, const float* feat, int ld_feat, const float* el, int ld_el,
                                                 const float* er, int ld_er, const float* out, int ld_out, const float* bias, const float* stats,
                                                 int ld_stats, int hidden, int heads, int64_t num_nodes, const int32_t* in_ptr,
                                                 const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_dst, int both,
                                                 float negative_slope, float* dfeat, int ld_dfeat, float* del, int ld_del, float* der, int ld_der,
                                                 float* work, void* stream) {
    using namespace gnnome;
    const AttBwdArgs a{g,       ld_g,    feat,    ld_feat, el,        ld_el,          er,    ld_er,    out, ld_out, bias, stats, ld_stats, num_nodes,
                       in_ptr,  srt_src, out_ptr, out_dst, both != 0, negative_slope, dfeat, ld_dfeat, del, ld_del, der,  ld_der, work};
    return attention_sum_bwd_checked(a, hidden, heads, kAttPhaseDst | kAttPhaseSrc, "node_attention_sum_bwd", stream);
}

// ---------------------------------------------------------------------------------------------------- one rank's shard: the two phases
// On a destination-range partition (include/gnnome_hip.h, "the attention sum on one rank's shard") a collective sits between the two
// launches - the halo rows of `work` are their owners' to compute - so each is an entry of its own.  Both are k_att_bwd_dst / k_att_bwd_src
// launched over the num_nodes_out owned rows: the kernels index their own node's rows below num_nodes_out and a neighbour's at whatever
// local id the list names, which is all a shard asks of them.

extern "C" int gnnome_node_attention_sum_bwd_dst_part_f32(const float* g, int ld_g, const float* feat, int ld_feat, const float* el, int ld_el,
                                                          const float* er, int ld_er, const float* out, int ld_out, const float* bias,
                                                          const float* stats, int ld_stats, int hidden, int heads, int64_t num_nodes_out,
                                                          int64_t num_nodes_local, const int32_t* in_ptr, const int32_t* srt_src,
                                                          const int32_t* out_ptr, const int32_t* out_dst, int both, float negative_slope,
                                                          float* der, int ld_der, float* work, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0 && num_nodes_out <= num_nodes_local, "node_attention_sum_bwd_dst_part: %lld destination rows of %lld local rows",
               (long long)num_nodes_out, (long long)num_nodes_local);
    const AttBwdArgs a{g,      ld_g,    feat,    ld_feat, el,        ld_el,          er,      ld_er, out,     ld_out, bias, stats, ld_stats, num_nodes_out,
                       in_ptr, srt_src, out_ptr, out_dst, both != 0, negative_slope, nullptr, 0,     nullptr, 0,      der,  ld_der, work};
    return attention_sum_bwd_checked(a, hidden, heads, kAttPhaseDst, "node_attention_sum_bwd_dst_part", stream);
}

extern "C" int gnnome_node_attention_sum_bwd_src_part_f32(const float* g, int ld_g, const float* feat, int ld_feat, const float* el, int ld_el,
                                                          const float* work, int hidden, int heads, int64_t num_nodes_out,
                                                          int64_t num_nodes_local, const int32_t* out_ptr, const int32_t* out_dst,
                                                          const int32_t* in_ptr, const int32_t* srt_src, int both, float negative_slope,
                                                          float* dfeat, int ld_dfeat, float* del, int ld_del, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0 && num_nodes_out <= num_nodes_local, "node_attention_sum_bwd_src_part: %lld source rows of %lld local rows",
               (long long)num_nodes_out, (long long)num_nodes_local);
    const AttBwdArgs a{g,      ld_g,    feat,    ld_feat, el,        ld_el,          nullptr, 0,        nullptr, 0,      nullptr, nullptr, 0, num_nodes_out,
                       in_ptr, srt_src, out_ptr, out_dst, both != 0, negative_slope, dfeat,   ld_dfeat, del,     ld_del, nullptr, 0, const_cast<float*>(work)};
    return attention_sum_bwd_checked(a, hidden, heads, kAttPhaseSrc, "node_attention_sum_bwd_src_part", stream);
}
