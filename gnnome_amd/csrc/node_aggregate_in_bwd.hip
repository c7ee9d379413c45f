// The training forms of GatedGCN's one gated aggregation (node_aggregate_in.hip is the inference form and is not touched):
//
//   gnnome_node_aggregate_in_raw_f32   the aggregation WITHOUT the node epilogue, with the two node tables its backward needs
//       s_p     = sigmoid(e[p,:])
//       aux0[i] = fwd_i = sum_{p in in(i)} s_p * A2h[src_p,:] / (sum_{p in in(i)} s_p + 1e-6)
//       aux1[i] = 1 / (sum_{p in in(i)} s_p + 1e-6)
//       v[i]    = A1h[i] + fwd_i
//     - mode 1 of gnnome_node_aggregate_raw_f32 without its backward direction: no A3h, no out-lists, no second read of e.
//
//   gnnome_node_aggregate_in_bwd_f32   the gradient of that aggregation, from the node tables Tf = dv * aux1, Uf = Tf * aux0
//       de[p,:]   += s_p (1 - s_p) * (Tf[dst_p,:] * A2h[src_p,:] - Uf[dst_p,:])          every edge p
//       dA2h[j,:]  = sum_{q in out(j)} s_{out_pos[q]} * Tf[out_dst[q],:]                  every node j
//     - the forward half of gnnome_agg_edge_bwd_f32 and aux2 of mode 2 of gnnome_node_aggregate_raw_f32 (tables Tb := 0, A3h := Tf).
//
//   gnnome_node_aggregate_in_raw_part_f32 / gnnome_node_aggregate_in_bwd_part_f32   the same two on one rank's shard of an in-edge-only
//     destination-range partition: the kernels below launched with TWO row counts - the n_own owned destinations (which come first) and the
//     n_local = owned + halo table rows.  See the entries at the end of the file.
//
// Reference lines replaced: gated_gcn_full.py:212-215 (sigmoid, DGL gspmm u_mul_e+sum and copy_e+sum, the divide) and :217 (A1h + ...)
// in train mode, and what torch autograd + DGL's backward kernels (gsddmm / gspmm on the reversed graph) run for those lines under
// loss.backward() (train.py:329).
//
// DECOMPOSITION of the backward: TWO launches, one wave per node each, no atomics, no per-edge scratch, fp32 throughout.
//   k_agg_in_bwd_dst<H>, one wave per DESTINATION i: the edges are destination-sorted, so the wave holds Tf[i], Uf[i] in registers and
//     streams its contiguous in-list exactly as the forward does - the e rows and the de rows from a uniform address, only A2h[src]
//     gathered.  Nothing is summed: every de row is read, updated and written by one lane group.
//   k_agg_in_bwd_src<H>, one wave per SOURCE j: walks out_ptr / out_pos / out_dst, gathers e[out_pos] and Tf[out_dst], sums.
//
// LANE MAPPING: node_aggregate_in.hip's.  A row of H floats is covered by H/4 lanes holding a float4 each, a wave64 walks G = 64/(H/4)
// items at once; lane l of a 64-item batch loads the batch's l-th index, the lane groups fetch it with ds_bpermute (one group, H = 256:
// v_readlane).
// ASSOCIATION of the sums (raw: num and den; bwd: dA2h) - fixed, a function of the graph alone: item t of a 64-item batch goes to lane
// group t mod G and is added there in ascending order; a list of more than 4096 items is summed in fixed 128-item blocks whose
// per-lane-group sums are added, in block order, to a second set of accumulators (at or below 4096 items there is one block, added to
// zero: exact); the lane groups are combined with the __shfl_xor tree.  For the in-lists this is node_aggregate_in.hip's association
// (the item loop below is a copy of its accumulate_in_items: that file stays byte for byte as it is, so the loop cannot move to a header).
// fp32 ROUNDINGS, per element.
//   raw: s = sigmoid4_(e) (v_exp_f32, v_rcp_f32: within 1 ulp each); num += s * a as one fma, den += s; after the tree
//        fwd = num / (den + 1e-6) (IEEE division), aux1 = 1 / (den + 1e-6), v = (A1h + fwd) + 0.0f - the trailing + 0.0f is mode 1's
//        backward term with a zero A3h table (0 / (0 + 1e-6) = +0): on nodes of at most 4096 in-edges the three outputs have mode 1's bits.
//   de:  w = s * (1 - s): one subtraction, one product; t = fma(Tf, A2h, -Uf): one rounding; de = fma(w, t, de): one rounding.
//        (gnnome_agg_edge_bwd_f32 forms the same expression plus its zero backward half; its contraction is the compiler's.)
//   dA2h: acc = fma(s, Tf row, acc) per item, then the blocks and the tree as above.  Mode 2 numbers a node's out-items after its
//        in-items, so its items land in other lane groups: the same terms in another order (equal bits are not promised).
// Every output of the backward is linear in (Tf, Uf) through products and sums only: scaling both by a power of two scales dA2h and the
// de increment exactly.
// HUBS: walked by their own wave in all three kernels, as in node_aggregate_in.hip (about a millisecond per 10^5 items - that file's
// ESTIMATE, not a measurement).
#include "common.h"

namespace gnnome {

constexpr int kAggInbThreads = 256;
constexpr int kInbHubThreshold = 4096;   // items above which a node's list is summed in two levels (node_aggregate_in.hip's kInHubThreshold)
constexpr int kInbHubBlock = 128;        // items per first-level block of such a list (its kInHubBlock)

template <int H>
__device__ __forceinline__ float inb_group_sum(float v) {
    // all-reduce over the lane groups (lanes with equal lane % (H/4)): node_aggregate_in.hip's in_group_sum
    constexpr int LPR = H / 4;
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// The one exception to "no inline assembly" in this file: an EMPTY asm statement - it emits no instruction - that makes its operand
// opaque to the optimiser, node_aggregate_in.hip's in_opaque_.  Without it the compiler hoists the wait for the index load above the
// contiguous row requests of the step; with it the rows go out first.  It orders loads only and cannot change a value.
__device__ __forceinline__ int inb_opaque_(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

template <int H>
__device__ __forceinline__ int inb_pick(int v, int it) {   // the value lane `it` holds; `it` is uniform inside a lane group
    if (H == 256) return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(it));
    return __builtin_amdgcn_ds_bpermute(it << 2, v);
}

// The gated sums over in-items [lo, hi) of one node (ib: the sorted position of its first in-edge): node_aggregate_in.hip's
// accumulate_in_items, statement for statement (same loop bounds, same operations in the same order: the same bits).
template <int H, int U>
__device__ __forceinline__ void inb_accumulate_in_items(const float* __restrict__ e, const float* __restrict__ A2h, int ldn,
                                                        const int32_t* __restrict__ srt_src, int ib, int lo, int hi, int lane, int group, int c,
                                                        f32x4& nf, f32x4& df, uint32_t a32_rows) {
    constexpr int LPR = H / 4, G = 64 / LPR;
    const uint32_t lc = (uint32_t)c * 4, lg = (uint32_t)group * (H * 4) + lc;
    auto pick = [&](uint32_t v, int it) -> uint32_t { return (uint32_t)inb_pick<H>((int)v, it); };
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
            const uint32_t nn = (uint32_t)inb_opaque_(my_n);
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

// One wave per node: v, fwd and the reciprocal denominator.
template <int H, int U = (H == 256 ? 2 : 4)>
__global__ __launch_bounds__(kAggInbThreads) void k_agg_in_raw(const float* __restrict__ e, int64_t n_end, const float* __restrict__ A1h,
                                                              const float* __restrict__ A2h, int ldn, const int32_t* __restrict__ in_ptr,
                                                              const int32_t* __restrict__ srt_src, float* __restrict__ v_out,
                                                              float* __restrict__ aux0, float* __restrict__ aux1, int total_blocks,
                                                              uint32_t a32_rows) {
    constexpr int LPR = H / 4;
    // the wave index read as a scalar: the node and everything loaded through it (the list bounds) live in scalar registers
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kAggInbThreads / 64) + wave;
    if (node >= n_end) return;
    const int group = lane / LPR, c = (lane % LPR) * 4;
    const int ib = in_ptr[node], din = in_ptr[node + 1] - ib;
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(A1h + node * ldn + c);

    f32x4 nf = {0.f, 0.f, 0.f, 0.f}, df = nf;
    const int blk = din > kInbHubThreshold ? kInbHubBlock : din;   // (one block unless the list is a hub's; wave-uniform)
    for (int blo = 0; blo < din; blo += blk) {
        f32x4 n1 = {0.f, 0.f, 0.f, 0.f}, d1 = n1;
        inb_accumulate_in_items<H, U>(e, A2h, ldn, srt_src, ib, blo, min(din, blo + blk), lane, group, c, n1, d1, a32_rows);
        nf += n1;
        df += d1;
    }

    f32x4 v, t0, t1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float num_f = inb_group_sum<H>(nf[k]), den_f = inb_group_sum<H>(df[k]);
        v[k] = a1[k] + num_f / (den_f + kAggEps) + 0.0f;   // (+ 0.0f: mode 1's bwd term with a zero A3h table, see the header)
        t0[k] = num_f / (den_f + kAggEps);
        t1[k] = 1.0f / (den_f + kAggEps);
    }
    if (group == 0) {
        *reinterpret_cast<f32x4*>(aux0 + node * H + c) = t0;
        *reinterpret_cast<f32x4*>(aux1 + node * H + c) = t1;
        *reinterpret_cast<f32x4*>(v_out + node * H + c) = v;
    }
}

// One wave per destination: de[p] += s (1 - s) (Tf[i] A2h[src_p] - Uf[i]) over its contiguous in-list.
template <int H, int U = (H == 256 ? 2 : 4)>
__global__ __launch_bounds__(kAggInbThreads) void k_agg_in_bwd_dst(const float* __restrict__ e, int64_t n_end, const float* __restrict__ Tf,
                                                                  const float* __restrict__ Uf, const float* __restrict__ A2h, int ldn,
                                                                  const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ srt_src,
                                                                  float* __restrict__ de, int total_blocks) {
    constexpr int LPR = H / 4, G = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kAggInbThreads / 64) + wave;
    if (node >= n_end) return;
    const int group = lane / LPR, c = (lane % LPR) * 4;
    const int ib = in_ptr[node], din = in_ptr[node + 1] - ib;
    if (din == 0) return;
    const f32x4 tf = *reinterpret_cast<const f32x4*>(Tf + node * H + c);
    const f32x4 uf = *reinterpret_cast<const f32x4*>(Uf + node * H + c);
    for (int base = 0; base < din; base += 64) {
        const int j = base + lane;   // lane l owns item base + l
        int my_n = 0;
        if (j < din) my_n = srt_src[ib + j];
        const int m = min(64, din - base);
        for (int j0 = 0; j0 < m; j0 += G * U) {
            const int64_t row0 = ((int64_t)ib + base + j0 + group) * H + c;   // this lane's slice of item j0 + group; slot u is u * G rows on
            f32x4 x[U], g[U], a[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                live[u] = j0 + u * G + group < m;
                if (live[u]) {
                    x[u] = *reinterpret_cast<const f32x4*>(e + row0 + (int64_t)u * G * H);
                    g[u] = *reinterpret_cast<const f32x4*>(de + row0 + (int64_t)u * G * H);
                }
            }
            const int nn = inb_opaque_(my_n);
#pragma unroll
            for (int u = 0; u < U; ++u)   // (a dead slot reads item j0's row, which exists)
                a[u] = *reinterpret_cast<const f32x4*>(A2h + (int64_t)inb_pick<H>(nn, live[u] ? j0 + u * G + group : j0) * ldn + c);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (live[u]) {
                    const f32x4 s = sigmoid4_(x[u]);
                    f32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = fmaf(s[k] * (1.0f - s[k]), fmaf(tf[k], a[u][k], -uf[k]), g[u][k]);
                    *reinterpret_cast<f32x4*>(de + row0 + (int64_t)u * G * H) = o;
                }
            }
        }
    }
}

// sum over out-items [lo, hi) of one node of s[pos] * Tf[dst], lane group g taking every G-th item of every 64-item batch
template <int H, int U>
__device__ __forceinline__ void inb_accumulate_out_items(const float* __restrict__ e, const float* __restrict__ Tf,
                                                         const int32_t* __restrict__ out_pos, const int32_t* __restrict__ out_dst, int ob, int lo,
                                                         int hi, int lane, int group, int c, f32x4& acc) {
    constexpr int LPR = H / 4, G = 64 / LPR;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;   // lane l owns item base + l
        int my_p = 0, my_n = 0;
        if (j < hi) {
            my_p = out_pos[ob + j];
            my_n = out_dst[ob + j];
        }
        const int m = min(64, hi - base);
        for (int j0 = 0; j0 < m; j0 += G * U) {
            f32x4 x[U], t[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int it = j0 + u * G + group;
                live[u] = it < m;
                const int sel = live[u] ? it : j0;   // (a dead slot reads item j0, which exists)
                x[u] = *reinterpret_cast<const f32x4*>(e + (int64_t)inb_pick<H>(my_p, sel) * H + c);
                t[u] = *reinterpret_cast<const f32x4*>(Tf + (int64_t)inb_pick<H>(my_n, sel) * H + c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (live[u]) {
                    const f32x4 s = sigmoid4_(x[u]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fmaf(s[k], t[u][k], acc[k]);
                }
            }
        }
    }
}

// One wave per source: dA2h[j] = sum over its out-list of s[out_pos] * Tf[out_dst].  A node without out-edges gets a zero row.
template <int H, int U = (H == 256 ? 2 : 4)>
__global__ __launch_bounds__(kAggInbThreads) void k_agg_in_bwd_src(const float* __restrict__ e, int64_t n_end, const float* __restrict__ Tf,
                                                                  const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_pos,
                                                                  const int32_t* __restrict__ out_dst, float* __restrict__ dA2h,
                                                                  int total_blocks) {
    constexpr int LPR = H / 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)xcd_remap(blockIdx.x, total_blocks) * (kAggInbThreads / 64) + wave;
    if (node >= n_end) return;
    const int group = lane / LPR, c = (lane % LPR) * 4;
    const int ob = out_ptr[node], dout = out_ptr[node + 1] - ob;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int blk = dout > kInbHubThreshold ? kInbHubBlock : dout;   // (wave-uniform)
    for (int blo = 0; blo < dout; blo += blk) {
        f32x4 part = {0.f, 0.f, 0.f, 0.f};
        inb_accumulate_out_items<H, U>(e, Tf, out_pos, out_dst, ob, blo, min(dout, blo + blk), lane, group, c, part);
        acc += part;
    }
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = inb_group_sum<H>(acc[k]);
    if (group == 0) *reinterpret_cast<f32x4*>(dA2h + node * H + c) = o;
}

static int inb_blocks(int64_t num_nodes, const char* who, int64_t* blocks) {
    *blocks = (num_nodes + (kAggInbThreads / 64) - 1) / (kAggInbThreads / 64);
    GN_REQUIRE(*blocks < (1ll << 31), "%s: too many nodes", who);
    return GNNOME_OK;
}

template <int H>
static int launch_agg_in_raw(const float* e, int64_t n, const float* A1h, const float* A2h, int ldn, const int32_t* in_ptr, const int32_t* ss,
                             float* v_out, float* aux0, float* aux1, hipStream_t s) {
    int64_t blocks;
    if (int rc = inb_blocks(n, "node_aggregate_in_raw", &blocks)) return rc;
    // table rows below this index are addressed with 32-bit byte offsets; gnnome_set_tuning(11, 1): none are
    const uint32_t a32_rows = tuning(kTuneAggAddr64) == 1 ? 0u : (uint32_t)((1ull << 32) / ((uint64_t)ldn * 4));
    hipLaunchKernelGGL((k_agg_in_raw<H>), dim3((unsigned)blocks), dim3(kAggInbThreads), 0, s, e, n, A1h, A2h, ldn, in_ptr, ss, v_out, aux0, aux1,
                       (int)blocks, a32_rows);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

// n_dst: the destinations whose in-lists are walked (Tf / Uf rows); n_src: the sources whose out-lists are walked (dA2h rows).  The whole
// graph: both its node count.  A shard of a destination-range partition: n_dst owned rows, n_src owned + halo rows.
template <int H>
static int launch_agg_in_bwd(const float* e, int64_t n_dst, int64_t n_src, const float* Tf, const float* Uf, const float* A2h, int ldn,
                             const int32_t* in_ptr, const int32_t* ss, const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                             float* de, float* dA2h, hipStream_t s) {
    int64_t blocks;
    if (int rc = inb_blocks(n_dst, "node_aggregate_in_bwd", &blocks)) return rc;
    hipLaunchKernelGGL((k_agg_in_bwd_dst<H>), dim3((unsigned)blocks), dim3(kAggInbThreads), 0, s, e, n_dst, Tf, Uf, A2h, ldn, in_ptr, ss, de,
                       (int)blocks);
    GN_LAUNCH_CHECK();
    if (int rc = inb_blocks(n_src, "node_aggregate_in_bwd", &blocks)) return rc;
    hipLaunchKernelGGL((k_agg_in_bwd_src<H>), dim3((unsigned)blocks), dim3(kAggInbThreads), 0, s, e, n_src, Tf, out_ptr, out_pos, out_dst, dA2h,
                       (int)blocks);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

// Argument checks and dispatch shared by the whole-graph entries and their partition forms (`who` names the entry in the error text).
static int agg_in_raw_entry(const char* who, const float* e, int hidden, int64_t num_nodes, const float* A1h, const float* A2h, int ld_node,
                            const int32_t* in_ptr, const int32_t* srt_src, float* v_out, float* aux0, float* aux1, void* stream) {
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "%s: hidden=%d not in {64,128,256}", who, hidden);
    if (num_nodes == 0) return GNNOME_OK;
    // e / srt_src may be NULL for a graph without edges (never dereferenced then)
    GN_REQUIRE(A1h && A2h && in_ptr && v_out && aux0 && aux1, "%s: null pointer", who);
    GN_REQUIRE(ld_node >= hidden && ld_node % 4 == 0, "%s: bad strides", who);
    GN_REQUIRE(((uintptr_t)A1h % 16 == 0) && ((uintptr_t)A2h % 16 == 0) && ((uintptr_t)e % 16 == 0) && ((uintptr_t)v_out % 16 == 0) &&
                   ((uintptr_t)aux0 % 16 == 0) && ((uintptr_t)aux1 % 16 == 0),
               "%s: tensors must be 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 64: return launch_agg_in_raw<64>(e, num_nodes, A1h, A2h, ld_node, in_ptr, srt_src, v_out, aux0, aux1, s);
        case 128: return launch_agg_in_raw<128>(e, num_nodes, A1h, A2h, ld_node, in_ptr, srt_src, v_out, aux0, aux1, s);
        default: return launch_agg_in_raw<256>(e, num_nodes, A1h, A2h, ld_node, in_ptr, srt_src, v_out, aux0, aux1, s);
    }
}

static int agg_in_bwd_entry(const char* who, const float* e, int64_t num_edges, int hidden, int64_t n_dst, int64_t n_src, const float* Tf,
                            const float* Uf, const float* A2h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src,
                            const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, float* de, float* dA2h, void* stream) {
    GN_REQUIRE(hidden == 64 || hidden == 128 || hidden == 256, "%s: hidden=%d not in {64,128,256}", who, hidden);
    if (n_src == 0) return GNNOME_OK;
    GN_REQUIRE(dA2h && (uintptr_t)dA2h % 16 == 0, "%s: dA2h is null or not 16-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if (num_edges == 0) {   // no edge: every out-list is empty and de has no rows
        GN_HIP(hipMemsetAsync(dA2h, 0, (size_t)n_src * hidden * sizeof(float), s));
        return GNNOME_OK;
    }
    GN_REQUIRE(n_dst > 0, "%s: %lld edges but no destination row", who, (long long)num_edges);
    GN_REQUIRE(e && Tf && Uf && A2h && in_ptr && srt_src && out_ptr && out_pos && out_dst && de, "%s: null pointer", who);
    GN_REQUIRE(ld_node >= hidden && ld_node % 4 == 0, "%s: bad strides", who);
    GN_REQUIRE(((uintptr_t)e % 16 == 0) && ((uintptr_t)Tf % 16 == 0) && ((uintptr_t)Uf % 16 == 0) && ((uintptr_t)A2h % 16 == 0) &&
                   ((uintptr_t)de % 16 == 0),
               "%s: tensors must be 16-byte aligned", who);
    GN_REQUIRE(de != e && dA2h != Tf && dA2h != Uf, "%s: outputs must not alias inputs", who);
    switch (hidden) {
        case 64: return launch_agg_in_bwd<64>(e, n_dst, n_src, Tf, Uf, A2h, ld_node, in_ptr, srt_src, out_ptr, out_pos, out_dst, de, dA2h, s);
        case 128: return launch_agg_in_bwd<128>(e, n_dst, n_src, Tf, Uf, A2h, ld_node, in_ptr, srt_src, out_ptr, out_pos, out_dst, de, dA2h, s);
        default: return launch_agg_in_bwd<256>(e, n_dst, n_src, Tf, Uf, A2h, ld_node, in_ptr, srt_src, out_ptr, out_pos, out_dst, de, dA2h, s);
    }
}

}  // namespace gnnome

extern "C" int gnnome_node_aggregate_in_raw_f32(const float* e, int hidden, int64_t num_nodes, const float* A1h, const float* A2h, int ld_node,
                                                const int32_t* in_ptr, const int32_t* srt_src, float* v_out, float* aux0, float* aux1,
                                                void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes >= 0, "node_aggregate_in_raw: negative node count");
    return agg_in_raw_entry("node_aggregate_in_raw", e, hidden, num_nodes, A1h, A2h, ld_node, in_ptr, srt_src, v_out, aux0, aux1, stream);
}

extern "C" int gnnome_node_aggregate_in_bwd_f32(const float* e, int64_t num_edges, int hidden, int64_t num_nodes, const float* Tf,
                                                const float* Uf, const float* A2h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src,
                                                const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, float* de, float* dA2h,
                                                void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes >= 0 && num_edges >= 0, "node_aggregate_in_bwd: negative node or edge count");
    return agg_in_bwd_entry("node_aggregate_in_bwd", e, num_edges, hidden, num_nodes, num_nodes, Tf, Uf, A2h, ld_node, in_ptr, srt_src, out_ptr,
                            out_pos, out_dst, de, dA2h, stream);
}

// ---- the partition forms: num_nodes_out destination rows (a rank's owned nodes, which come first), num_nodes_local table rows (owned + halo).
// The kernels are the ones above - same lane mapping, same association - launched over the rows that have work: the raw form and the
// backward's destination launch over the num_nodes_out owned rows (no wave per halo row, no [num_nodes_local, H] output nobody reads), the
// backward's source launch over all num_nodes_local rows.

extern "C" int gnnome_node_aggregate_in_raw_part_f32(const float* e, int hidden, int64_t num_nodes_out, int64_t num_nodes_local, const float* A1h,
                                                     const float* A2h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src, float* v_out,
                                                     float* aux0, float* aux1, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_nodes_out >= 0 && num_nodes_out <= num_nodes_local, "node_aggregate_in_raw_part: %lld destination rows of %lld local rows",
               (long long)num_nodes_out, (long long)num_nodes_local);
    return agg_in_raw_entry("node_aggregate_in_raw_part", e, hidden, num_nodes_out, A1h, A2h, ld_node, in_ptr, srt_src, v_out, aux0, aux1, stream);
}

extern "C" int gnnome_node_aggregate_in_bwd_part_f32(const float* e, int64_t num_edges, int hidden, int64_t num_nodes_out, int64_t num_nodes_local,
                                                     const float* Tf, const float* Uf, const float* A2h, int ld_node, const int32_t* in_ptr,
                                                     const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos,
                                                     const int32_t* out_dst, float* de, float* dA2h, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_edges >= 0 && num_nodes_out >= 0 && num_nodes_out <= num_nodes_local,
               "node_aggregate_in_bwd_part: %lld edges, %lld destination rows of %lld local rows", (long long)num_edges, (long long)num_nodes_out,
               (long long)num_nodes_local);
    return agg_in_bwd_entry("node_aggregate_in_bwd_part", e, num_edges, hidden, num_nodes_out, num_nodes_local, Tf, Uf, A2h, ld_node, in_ptr,
                            srt_src, out_ptr, out_pos, out_dst, de, dA2h, stream);
}
