/*
 * gnnome_hip.h - C ABI of libgnnome_hip.so, the MI355X (gfx950) implementation of GNNome's
 * SymGatedGCN edge-scoring path.
 *
 * The reference (lbcb-sci/GNNome) has no FFI seam for this path: the seam is the Python module
 * `models.SymGatedGCNModel.forward(graph, x, e)` (models/full_graph.py:22-30), whose native work
 * is done by two third-party wheels (DGL 0.8.1 graph kernels, PyTorch 1.9 dense/elementwise ops).
 * Each entry point below names the reference call sites it replaces.  The Python host module
 * `gnnome_amd.models.SymGatedGCNModel` binds them through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is stream-ordered,
 *     nothing synchronises the host
 *   - matrices are row-major fp32; `ld*` arguments are row strides in ELEMENTS
 *   - graph indices are int32 (the reference casts graphs with g.int(), utils/data_utils.py:32)
 *   - return value: 0 on success, a negative GNNOME_E* code otherwise; gnnome_last_error() returns a
 *     thread-local message for the last failure
 *   - "sorted position" p in [0,E) is an edge's slot in destination-sorted (CSR-by-dst) order; all
 *     [E,H] edge tensors handed to the kernels live in that order
 */
#ifndef GNNOME_HIP_H
#define GNNOME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Raised when an existing entry changes its signature or meaning.  32 also covers gnnome_node_neighbour_sum_part_f32,
 * gnnome_node_neighbour_sum_bwd_part_f32 and the four part entries of the attention sum (gnnome_node_attention_sum_part_f32, _stats_part_f32,
 * _bwd_dst_part_f32, _bwd_src_part_f32), which were ADDED without touching any other entry: a caller built against 32 keeps working, and
 * the Python binding resolves every entry by name when it loads the library, so a library that predates them is refused there, by name.
 * The three interval-union entries and the five positional-encoding entries were added in the same way. */
#define GNNOME_ABI_VERSION 32

#define GNNOME_OK 0
#define GNNOME_EINVAL (-1)    /* bad argument (null pointer, unsupported width, bad stride)      */
#define GNNOME_EHIP (-2)      /* a HIP runtime call or a kernel launch failed                     */
#define GNNOME_EWORKSPACE (-3) /* workspace too small                                             */

/* normalisation applied inside the fused kernels (gated_gcn_full.py:37-42) */
#define GNNOME_NORM_AFFINE 0  /* y = x*scale[c] + shift[c]: eval-mode BatchNorm1d folded to an affine,
                                 or train-mode BatchNorm1d once the batch statistics are known     */
#define GNNOME_NORM_LAYER 1   /* y = (x-mean_row)/sqrt(var_row+1e-5)*scale[c] + shift[c]: LayerNorm */
/* LayerNorm whose row statistics run over the first w channels only: a model narrower than the built width (64 / 128 / 256) runs
 * zero-padded - its padded channels hold exact zeros and zero scale / shift - and normalises over its OWN width
 * (configs/hyperparameters.py:22 takes any hidden_features).  Accepted wherever norm_kind is; w = hidden is GNNOME_NORM_LAYER. */
#define GNNOME_NORM_LAYER_OVER(w) (GNNOME_NORM_LAYER | ((w) << 8))

int gnnome_abi_version(void);
const char* gnnome_last_error(void);

/* Measurement knobs, not part of the reference-facing contract: select kernel variants for A/B runs
 * (tools/kernel_ab.py).  0 is always the shipped default.
 *   key 0 edge gate variant : 0 shipped default (H = 128: plane-form bf16x6 edge-tile kernel k_edge_gate_pl, layer 0
 *                             k_edge_gate_enc16; H = 64: k_edge_gate_bf; H = 256: the wave-specialised / streaming kernel),
 *                             1 tile-per-workgroup kernel, 5 exact-fp32 MFMA wave-specialised kernel (LDS-counter
 *                             hand-over), 6 the same with workgroup barriers, 7 = 0 spelled out (plane form),
 *                             8 second-generation bf16x6 kernel k_edge_gate_bf at H = 128 (split in the compute waves)
 *   key 1 edge gate ablation: bit mask, timing only (results are wrong): 1 no node gathers, 2 no stores,
 *                             4 no e loads, 8 no MFMA, 16 nontemporal e loads / e' stores
 *   key 2 linear variant    : 0 shipped default (bf16x6 streaming kernel, A-stationary from 400k rows), 1 tile kernel,
 *                             2 exact-fp32 weight-stationary, 3 bf16x6 with A staged through LDS, 4 8-wave workgroups,
 *                             5 2-wave workgroups, 6 A-stationary at every size, 7 streaming kernel with row-major 16-byte
 *                             stores (the default at K = 64)
 *   key 3 gate tile order   : 1 contiguous run per workgroup (default: interleaved, XCD-contiguous)
 *   key 4 gate experiment   : kernel-specific measurement switch (H = 256 streaming gate: tiles per workgroup piece)
 *   key 5 aggregation LDS   : KiB of unused dynamic LDS per workgroup (caps the resident workgroups per CU)
 *   key 6 aggregation hubs  : 1 = hub split path off
 *   key 7 aggregation variant: 1-5 items in flight / occupancy A/B, 6 unsplit item loop
 *   key 8 reference-order kernels: 0 the fp32 matrix cores (v_mfma_f32_32x32x2_f32 as a k-ascending fma chain), 1 the
 *                             scalar-fed VALU chains of round 2 (same bits)
 *   key 9 overlap edit distance: 0 banded (Ukkonen) pass first, the full matrix for what exceeds the band; 1 full matrix only
 *   key 10 forward arithmetic : 0 fp16x3 on the f16 matrix cores for the forward's dense products at H = 128 / 256 (round 4; see
 *                             gnnome_linear_f32), 1 bf16x6 everywhere (round 3's arithmetic; the plane-form kernels at H = 256)
 *   key 7 also: 9 / 10 two nodes per wave (U = 4 / 2), 11-13 persistent contiguous chunks (measured negatives),
 *                             16 the item loop before the lean one (accumulate_items_split; the same bits, every mode),
 *                             17 the lean loop with fixed-width rounds (G * U row-load slots in every round, as before the exact-width
 *                             rounds; the same bits, every mode) - the A/B partner and bit oracle of tests/test_aggregate_exact_rounds.py
 *   key 11 aggregation addressing: 1 = row addresses in 64 bits per item at every size (default: 32-bit byte offsets wherever a step's
 *                             rows lie below 4 GiB; the same bits)
 *   key 12 node projection schedule (gnnome_linear_planes_f32 at K = 128): 0 the shipped default, 1 the schedule before it (plain stores for P, where the
 *                             default stores nontemporally) - the same bits, the A/B partner and the bit oracle of
 *                             tests/test_node_project_schedule.py */
int gnnome_set_tuning(int key, int value);

/* Measurement only: when set to a device buffer of 256 x 8 int64, every launch of the edge-tile kernel leaves, per
 * workgroup, the shader-clock cycles its first compute wave spent [0] waiting for a slot, [1] in the tile prologue,
 * [2] in the MFMA loop, [3] writing x back, and [4] its tile count.  NULL (the default) turns it off. */
int gnnome_debug_gate_profile(void* counters);

/* ---- graph views -------------------------------------------------------------------------------
 * Replaces what DGL builds lazily inside g.update_all / dgl.reverse (gated_gcn_full.py:99,112-113,
 * 125-126): the in-edge (by dst) and out-edge (by src) orderings of one edge list.
 *   src,dst      int32[E]   edge endpoints in edge-id order (graph.edges())
 *   in_ptr       int32[N+1] CSR offsets by destination over sorted positions
 *   srt_src/dst  int32[E]   endpoints of the edge at sorted position p
 *   srt_eid      int32[E]   original edge id of sorted position p (stable: ties keep edge-id order)
 *   out_ptr      int32[N+1] CSR offsets by source
 *   out_pos      int32[E]   for each node, the sorted positions of its out-edges (ascending)
 *   out_dst      int32[E]   out_dst[q] = srt_dst[out_pos[q]], the far endpoint of that out-edge
 */
/* Building views also resets the aggregation's per-device hub cache: the list of nodes with more than 4096 incident edges is
 * keyed by the addresses of in_ptr / out_ptr; a caller that rewrites such arrays in place must call this entry (or use new arrays). */
int gnnome_graph_views_workspace_bytes(int64_t num_nodes, int64_t num_edges, size_t* bytes_host);
int gnnome_build_graph_views(const int32_t* src, const int32_t* dst, int64_t num_nodes, int64_t num_edges,
                             int32_t* in_ptr, int32_t* srt_src, int32_t* srt_dst, int32_t* srt_eid,
                             int32_t* out_ptr, int32_t* out_pos, int32_t* out_dst, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- encoders ----------------------------------------------------------------------------------
 * out[r,:] = W2 * relu(W1 * in[row(r),:] + b1) + b2, row(r) = gather ? gather[r] : r.
 * Replaces linear2_*(relu(linear1_*(.))) at models/full_graph.py:26-27.  `gather` = srt_eid turns
 * the edge-id-ordered e[E,F] into the sorted-order e0[E,H] without a separate permute pass.
 *   in [rows_in,F]  W1 [M,F]  b1 [M]  W2 [H,M]  b2 [H]  out [rows,H];  F <= 8, M <= 64
 */
int gnnome_encode_f32(const float* in, int64_t rows, int in_features, const int32_t* gather,
                      const float* W1, const float* b1, int hidden_ne, const float* W2, const float* b2,
                      int hidden, float* out, void* stream);

/* ---- dense linear on the matrix cores -----------------------------------------------------------
 * C[M,Nout] = A[M,K] * W[Nout,K]^T + bias (torch nn.Linear layout).
 * Replaces the five node projections A_1,A_2,A_3,B_1,B_2 (gated_gcn_full.py:91-96, one call with the
 * weights concatenated) and the node halves of predictor.W1 (score_predictor.py:13-14).
 * Arithmetic: the fp32-faithful "bf16x6" product on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16): every fp32
 * operand is split EXACTLY into three bf16 and six of the nine partial products are accumulated in fp32; the dropped
 * terms are <= 3 * 2^-24 |a b| per product, i.e. one fp32 rounding, so |C - exact| <= ~(K + 3) * 2^-24 * sum|a b| like
 * any fp32 dot product - but the fp32 number produced is not the one a k-ordered fma chain produces (see
 * gnnome_linear_ref_f32 for that).  The exact-fp32 MFMA kernels (v_mfma_f32_32x32x2_f32) stay selectable with
 * gnnome_set_tuning(2, 2).
 * Round 4: where the output is whole 128-column blocks (K = 128 with Nout >= 256, K = 256) - the node projections - and in the forward modes of
 * the edge gate at H = 128 / 256 the product runs as "fp16x3" on the f16 matrix cores (v_mfma_f32_32x32x16_f16): every fp32 operand as TWO fp16
 * planes x1 = RN16(x), x2 = RN16((x - x1) * 2048) and three of the four plane products, the two small ones in a second fp32 accumulator that is
 * folded in with 2^-11; dropped terms <= 3 * 2^-22 |a b| per product, measured no further from an fp64 product than an fp32 GEMM
 * (tests/test_f16x3_model.py: 8e-8 of sum |a b| against 3.3e-7 at K = 256).  Operands must lie inside fp16's range, |x| < 65504: an element beyond it
 * makes its output row NaN (never a wrong finite value).  gnnome_set_tuning(10, 1) keeps bf16x6 there too.
 *   K % 32 == 0; bias may be NULL; A and W 16-byte aligned with lda, ldw % 4 == 0
 */
int gnnome_linear_f32(const float* A, int64_t M, int K, int lda, const float* W, int ldw, const float* bias,
                      int Nout, float* C, int ldc, void* stream);
/* C += A*W^T + bias: the residual form the backward uses (d e_in = d e' + dxe*W3; dh = dh_in + dP*Wcat). */
int gnnome_linear_acc_f32(const float* A, int64_t M, int K, int lda, const float* W, int ldw, const float* bias,
                          int Nout, float* C, int ldc, void* stream);

/* Round 6 - the node projection with PREPARED weights (gated_gcn_full.py:91-96 as one GEMM over the row-concatenated A_1 | A_2 | A_3 | B_1 | B_2;
 * score_predictor.py:13-14's node halves): gnnome_weight_planes_f16 splits W[Nout, K] ONCE into the two fp16 planes of the fp16x3 arithmetic
 * (see gnnome_linear_f32), laid out in MFMA fragment order as 16 KB chunks [Nout / 32][K / 128][8 k steps][2 planes][64 lanes][8 halves] =
 * Nout * K * 4 bytes at `planes` (256-byte aligned); gnnome_linear_planes_f32 computes C[M, Nout] = A W^T + bias from them
 * (csrc/node_project.hip): a wave keeps its 32 rows of A as planes in registers for every output column, the chunks of W arrive from L2 in an
 * LDS ring by LDS-DMA, 16-byte row pieces leave straight from the accumulators.  K in {64, 128, 256}, Nout % 32 == 0 (K <= 128: % 64), Nout <= 1536;
 * lda, ldc % 4 == 0, A, C 16-byte aligned, C must not alias A; bias may be NULL.  A row's bits depend on that row and W alone (not on M).  Same
 * operand range as every fp16x3 product: an |element| >= 65504 makes its output row NaN.
 * gnnome_linear_planes_route: 1 when a product of this shape is to run on gnnome_linear_planes_f32 under the current tuning, 0 when it keeps
 * gnnome_linear_f32's routes - ONE rule for every host above the ABI (gnnome_amd.ops.linear, gnnome_model_forward_f32, the dispatcher operator
 * gnnome_hip::linear): the kernel's shapes; without planes from the caller (`given_planes` = 0) only the node projections' shapes at K >= 128, whole 128-column
 * blocks with K = 256 or Nout >= 256; not under gnnome_set_tuning(10, 1) (bf16x6) or a gnnome_set_tuning(2, .) variant of the older kernels; not
 * when the environment holds GNNOME_PLANES_LINEAR=0 (A/B against round 5's routes).  Alignment and aliasing stay the caller's to check. */
int gnnome_weight_planes_f16(const float* W, int ldw, int Nout, int K, void* planes, void* stream);
int gnnome_linear_planes_f32(const float* A, int64_t M, int K, int lda, const void* planes, const float* bias, int Nout, float* C,
                             int ldc, void* stream);
int gnnome_linear_planes_route(int64_t M, int K, int Nout, int given_planes);

/* ---- fused edge gate ----------------------------------------------------------------------------
 * For every sorted position p:
 *   e_out[p,:] = relu(norm_e(B1h[srt_src[p],:] + B2h[srt_dst[p],:] + e_in[p,:] * W3^T)) + e_in[p,:]
 * i.e. B_3(e), u_add_v, bn_e, relu and the residual of gated_gcn_full.py:97,104-110 (and the
 * bit-identical second evaluation at :117-122) in one pass.  B_3's bias must already be folded into
 * B2h.  e_out may alias e_in.  H in {64,128,256}.
 */
int gnnome_edge_gate_f32(const float* e_in, float* e_out, int64_t num_edges, int hidden,
                         const float* B1h, const float* B2h, int ld_node, const int32_t* srt_src,
                         const int32_t* srt_dst, const float* W3, int ldw, int norm_kind,
                         const float* norm_scale, const float* norm_shift, void* stream);

/* Layer-0 form of the gate with the edge encoder folded in (models/full_graph.py:27 + gated_gcn_full.py:97-110):
 *   e0[p,:]    = encW2 * relu(encW1 * e_raw[srt_eid[p],:] + encb1) + encb2          (in_features 2, hidden_ne 16)
 *   e_out[p,:] = relu(norm_e(B1h[srt_src[p],:] + B2h[srt_dst[p],:] + e0[p,:]*W3^T)) + e0[p,:]
 * e0 is produced tile by tile in LDS and never touches HBM.  hidden in {64,128}, affine norm only; 256 since round 4 (the encoder folded
 * algebraically into a K = 16 product on the fp16x3 edge-tile kernel; default kernels only).
 * At hidden = 128 the encoder is folded algebraically: with t = relu(encW1 * e_raw + encb1) (16 wide), e0*W3^T = t*(W3*encW2)^T +
 * W3*encb2, so the gate's product and the residual e0 are two K = 16 products of one tile; W3*encW2 and W3*encb2 are recomputed at
 * every call (fp32, fixed summation tree) into a small per-device buffer - calls on DIFFERENT streams of one device must not
 * overlap.  The result differs from the unfolded form by fp32 reassociation only (a few 1e-7 relative). */
int gnnome_edge_gate_encode_f32(const float* e_raw, const int32_t* srt_eid, const float* encW1, const float* encb1,
                                const float* encW2, const float* encb2, float* e_out, int64_t num_edges, int hidden,
                                const float* B1h, const float* B2h, int ld_node, const int32_t* srt_src,
                                const int32_t* srt_dst, const float* W3, int ldw, const float* norm_scale,
                                const float* norm_shift, void* stream);

/* ---- the same two operations in the REFERENCE'S ORDER of evaluation --------------------------------
 * torch's CPU nn.Linear evaluates every output element as one k-ascending chain of fused multiply-adds that starts
 * from zero and adds the bias afterwards; its eval-mode BatchNorm1d is fma(x, alpha, beta).  These two entry points
 * reproduce that sequence operation for operation, so their results equal the reference's CPU results BIT FOR BIT on
 * equal inputs (tests/test_reference_order.py) - which matters for layers whose normalisation magnifies reorder noise
 * (weights/weights.pt layer 0: bn_e gain up to 135).  One row per lane, weights through scalar
 * loads, fp32 VALU; by default the same chain on the fp32 matrix cores (v_mfma_f32_32x32x2_f32 evaluates its two k in order).
 * K / hidden in {64,128}; 256 on the matrix-core form only (round 4; Nout % 32 == 0 there).
 *
 * gnnome_linear_ref_f32: C[M,Nout] = chain(A W^T) + bias;  Nout % 8 == 0  (gated_gcn_full.py:91-96)
 * gnnome_edge_gate_ref_f32 (gated_gcn_full.py:97,104-110; B_3's bias is NOT folded into B2h here):
 *   B3e  = chain(e W3^T) + b3
 *   x    = (B1h[srt_src[p]] + B2h[srt_dst[p]]) + B3e
 *   e'   = max(fma(x, norm_scale, norm_shift), 0) + e
 *   with e = e_in[p,:], or - when e_raw != NULL - the edge encoder's output for edge srt_eid[p], computed in registers
 *   in the same order (models/full_graph.py:27; in_features 2, hidden_ne 16).  e_out may alias e_in.
 */
int gnnome_linear_ref_f32(const float* A, int64_t M, int K, int lda, const float* W, int ldw, const float* bias, int Nout,
                          float* C, int ldc, void* stream);
int gnnome_edge_gate_ref_f32(const float* e_in, float* e_out, int64_t num_edges, int hidden, const float* B1h,
                             const float* B2h, int ld_node, const int32_t* srt_src, const int32_t* srt_dst, const float* W3,
                             int ldw, const float* b3, const float* norm_scale, const float* norm_shift, const float* e_raw,
                             const int32_t* srt_eid, const float* encW1, const float* encb1, const float* encW2,
                             const float* encb2, void* stream);

/* ---- fused gated aggregation + node update -------------------------------------------------------
 * For every node i < num_nodes_out, with s_p = sigmoid(e[p,:]):
 *   fwd = sum_{p in in(i)}  s_p * A2h[srt_src[p],:] / (sum_{p in in(i)}  s_p + 1e-6)
 *   bwd = sum_{q in out(i)} s_p * A3h[out_dst[q],:] / (sum_{q in out(i)} s_p + 1e-6),  p = out_pos[q]
 *   h_out[i,:] = relu(norm_h(A1h[i,:] + fwd + bwd)) + h_in[i,:]
 * Replaces sigmoid + both update_all pairs + the node epilogue, gated_gcn_full.py:111-114,124-137.
 * The summation order depends on the graph only (never on scheduling): bit-reproducible.
 * h_out is dense [num_nodes_out, H]; it must not alias h_in.
 */
int gnnome_node_aggregate_f32(const float* e, int hidden, int64_t num_nodes_out, const float* A1h,
                              const float* A2h, const float* A3h, int ld_node, const int32_t* in_ptr,
                              const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos,
                              const int32_t* out_dst, const float* h_in, int ld_h, float* h_out, int norm_kind,
                              const float* norm_scale, const float* norm_shift, void* stream);

/* The aggregation's record form (round 6; same bits as the default kernel): per-node 256-byte records [ib, in-degree, ob, out-degree, 20 x srt_src,
 * 20 x out_pos, 20 x out_dst] (records[num_nodes][64], 256-byte aligned) and the switch that makes the calling thread's following gnnome_node_aggregate_f32
 * calls (BatchNorm, whole node range) take a node's pointers AND neighbour ids from ONE load; NULL: off.  -11 % per launch at hidden = 64, level from 128 on. */
int gnnome_build_node_records(const int32_t* in_ptr, const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos,
                              const int32_t* out_dst, int64_t num_nodes, int32_t* records, void* stream);
int gnnome_debug_node_records(const int32_t* records);

/* The same update for the nodes [node_begin, node_end) only - all pointers and num_nodes_out describe the WHOLE graph
 * exactly as for gnnome_node_aggregate_f32, rows outside the range are not touched.  Lets a caller cut one aggregation
 * (gated_gcn_full.py:111-137) into consecutive launches and start the NEXT layer's node projection (:91-96) on the rows
 * that are complete, on a second stream, while the remaining ranges are still being reduced (engine.aggregate_then_project).
 * Results are bit-identical to the single launch.  The ranges of one aggregation must be issued in ascending order
 * starting at node 0: the range that begins at 0 also runs the long-list (hub) path for the whole graph. */
int gnnome_node_aggregate_range_f32(const float* e, int hidden, int64_t num_nodes_out, int64_t node_begin, int64_t node_end,
                                    const float* A1h, const float* A2h, const float* A3h, int ld_node, const int32_t* in_ptr,
                                    const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos,
                                    const int32_t* out_dst, const float* h_in, int ld_h, float* h_out, int norm_kind,
                                    const float* norm_scale, const float* norm_shift, void* stream);

/* ---- in-edge gated aggregation + node update: the GatedGCN layer (one direction) ---------------------
 * For every node i < num_nodes_out, with s_p = sigmoid(e[p,:]):
 *   fwd = sum_{p in in(i)} s_p * A2h[srt_src[p],:] / (sum_{p in in(i)} s_p + 1e-6)
 *   h_out[i,:] = relu(norm_h(A1h[i,:] + fwd)) + h_in[i,:]
 * Replaces sigmoid + the one update_all pair + the node epilogue of the reference's GatedGCN layer, gated_gcn_full.py:212-225
 * (the symmetric layer without A_3 and without the pass over dgl.reverse(g)).  A pure stream over the destination-sorted e rows
 * plus one gathered table: no out_ptr / out_pos / out_dst.  hidden in {64,128,256}; norm_kind GNNOME_NORM_AFFINE or
 * GNNOME_NORM_LAYER; ld_node is free (a [N,4H] projection here, any row stride >= hidden that is a multiple of 4); the table rows
 * A2h[srt_src[p]] may lie beyond num_nodes_out (halo rows of a partition).  All row pointers, norm_scale and norm_shift 16-byte aligned.
 * The summation order depends on the graph only: bit-reproducible, and for every node whose in + out list gnnome_node_aggregate_f32
 * reduces with one wave (<= 4096 items) EQUAL BIT FOR BIT to that entry's result with an all-zero A3h table.  A node with more than
 * 4096 in-edges is still reduced by its one wave (about a millisecond per 10^5 edges - an estimate), in two levels of fixed
 * 128-item blocks.  h_out is dense [num_nodes_out, H]; it must not alias h_in. */
int gnnome_node_aggregate_in_f32(const float* e, int hidden, int64_t num_nodes_out, const float* A1h, const float* A2h, int ld_node,
                                 const int32_t* in_ptr, const int32_t* srt_src, const float* h_in, int ld_h, float* h_out,
                                 int norm_kind, const float* norm_scale, const float* norm_shift, void* stream);

/* The same update for the nodes [node_begin, node_end) only - all pointers and num_nodes_out describe the WHOLE graph exactly as for
 * gnnome_node_aggregate_in_f32, rows outside the range are not touched (the contract of gnnome_node_aggregate_range_f32).  Results are
 * bit-identical to the single launch; there is no hub pass here, so the ranges of one aggregation may be issued in any order. */
int gnnome_node_aggregate_in_range_f32(const float* e, int hidden, int64_t num_nodes_out, int64_t node_begin, int64_t node_end,
                                       const float* A1h, const float* A2h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src,
                                       const float* h_in, int ld_h, float* h_out, int norm_kind, const float* norm_scale,
                                       const float* norm_shift, void* stream);

/* The same aggregation WITHOUT the node epilogue, with the two node tables its backward needs - the train-mode forward of the GatedGCN
 * layer, gated_gcn_full.py:212-215 (sigmoid, the update_all pair, the divide) and :217 (the sum with A1h); the one-direction form of mode 1
 * of gnnome_node_aggregate_raw_f32.  For every node i < num_nodes:
 *   aux0[i,:]  = fwd = sum_{p in in(i)} s_p * A2h[srt_src[p],:] / (sum_{p in in(i)} s_p + 1e-6)
 *   aux1[i,:]  = 1 / (sum_{p in in(i)} s_p + 1e-6)
 *   v_out[i,:] = A1h[i,:] + fwd
 * v_out, aux0, aux1 dense [num_nodes, H]; everything else as for gnnome_node_aggregate_in_f32 (same lane mapping and association:
 * lists above 4096 items in fixed 128-item blocks).  On nodes of at most 4096 in-edges the three outputs equal mode 1's with an all-zero
 * A3h table bit for bit. */
int gnnome_node_aggregate_in_raw_f32(const float* e, int hidden, int64_t num_nodes, const float* A1h, const float* A2h, int ld_node,
                                     const int32_t* in_ptr, const int32_t* srt_src, float* v_out, float* aux0, float* aux1,
                                     void* stream);

/* The gradient of that aggregation - what torch autograd and DGL's backward kernels run for gated_gcn_full.py:212-215 under
 * loss.backward() (train.py:329).  Tf = dv * aux1 and Uf = Tf * aux0 are dense [num_nodes, H] (gnnome_mul23_f32), s_p = sigmoid(e[p,:]):
 *   de[p,:]   += s_p (1 - s_p) * (Tf[dst_p,:] * A2h[srt_src[p],:] - Uf[dst_p,:])       every edge p   (dst_p: the node whose in-list holds p)
 *   dA2h[j,:]  = sum_{q in out(j)} s_{out_pos[q]} * Tf[out_dst[q],:]                    every node j   (dense [num_nodes, H], overwritten)
 * - the first half of gnnome_agg_edge_bwd_f32 and aux2 of mode 2 of gnnome_node_aggregate_raw_f32.  Two launches (one wave per
 * destination, one wave per source), no atomics, no scratch, fp32; the association depends on the graph alone (lists above 4096 items in
 * fixed 128-item blocks).  hidden in {64,128,256}; ld_node: the row stride of A2h.  num_nodes == 0: a no-op; num_edges == 0: dA2h is
 * zeroed and de is not touched.  de must not alias e. */
int gnnome_node_aggregate_in_bwd_f32(const float* e, int64_t num_edges, int hidden, int64_t num_nodes, const float* Tf, const float* Uf,
                                     const float* A2h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src,
                                     const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, float* de, float* dA2h,
                                     void* stream);

/* The PARTITION FORMS of the two entries above: one rank's rows of the train-mode GatedGCN layer (layers/gated_gcn_full.py:182-230:
 * its aggregation lines :212-217 and what autograd runs for them) on a destination-range partition that keeps, per rank, the in-edges
 * of its owned nodes only.  Local node ids put the num_nodes_out OWNED nodes first, then the halo (the distinct non-owned sources) up to
 * num_nodes_local; every local edge ends in an owned node, so in_ptr[num_nodes_out] = num_edges and a halo node has no in-list.
 *
 * raw:  v_out / aux0 / aux1 dense [num_nodes_out, H] for the owned rows only; A1h rows < num_nodes_out are read, A2h[srt_src[p]] is
 *       gathered from the num_nodes_local-row table.  The in-lists and their order are the whole graph's (the partition keeps the global
 *       edge-id order within a destination run), so an owned row equals gnnome_node_aggregate_in_raw_f32's row on the whole graph bit for bit.
 * bwd:  Tf, Uf dense [num_nodes_out, H].  The destination launch (de += ..., the Tf / Uf consumer) runs over the num_nodes_out owned rows;
 *       the source launch runs over ALL num_nodes_local rows and walks out_ptr / out_pos / out_dst of the LOCAL edges (out_ptr has
 *       num_nodes_local + 1 entries, out_dst[q] < num_nodes_out), so dA2h is dense [num_nodes_local, H] and a halo source's row is this
 *       rank's PARTIAL sum: the owner adds its own row and the partials it receives in ascending rank order (the halo transpose), which
 *       makes the final row a function of the graph and the world size alone.
 * Same kernels, lane mapping and association as the whole-graph entries (lists above 4096 items in fixed 128-item blocks, no atomics, no
 * per-edge table); no wave is spent on a halo destination and no [num_nodes_local, H] output is written that nobody reads.
 * num_nodes_out <= num_nodes_local is required; with num_nodes_out == num_nodes_local both are the whole-graph entries. */
int gnnome_node_aggregate_in_raw_part_f32(const float* e, int hidden, int64_t num_nodes_out, int64_t num_nodes_local, const float* A1h,
                                          const float* A2h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src, float* v_out,
                                          float* aux0, float* aux1, void* stream);
int gnnome_node_aggregate_in_bwd_part_f32(const float* e, int64_t num_edges, int hidden, int64_t num_nodes_out, int64_t num_nodes_local,
                                          const float* Tf, const float* Uf, const float* A2h, int ld_node, const int32_t* in_ptr,
                                          const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                                          float* de, float* dA2h, void* stream);

/* ---- unweighted, degree-normalised neighbour sum: the message passing of GCNModel and SAGEModel -------
 * For every node i < num_nodes:
 *   out[i,:] = dscale[i] * ( sscale[i] * h[i,:] + sum_{p in in(i)} sscale[srt_src[p]] * h[srt_src[p],:]
 *                                               + sum_{q in out(i)} sscale[out_dst[q]] * h[out_dst[q],:] )     (last sum: out_ptr != NULL only)
 * Replaces the convolutions' message passing on g' = dgl.add_self_loop(g) (directed=True) or add_self_loop(add_reverse_edges(g))
 * (directed=False), models/full_graph.py:65-75 (GCNModel) and :109-119 (SAGEModel): DGL's GraphConv(norm='both') of
 * layers/processor.py:35-46 with sscale = dout'^-1/2, dscale = din'^-1/2, and SAGEConv('mean') of :73-84 with sscale = NULL,
 * dscale = 1/din'.  g' is never built: in(i) = [in_ptr[i], in_ptr[i+1]) of srt_src, out(i) = [out_ptr[i], out_ptr[i+1]) of out_dst
 * (the arrays of gnnome_build_graph_views), the loop edge is the node's own row and counts once more where the graph already has one.
 * sscale, dscale: per-node floats, each may be NULL (= 1).  out_ptr == NULL selects the directed form (in-list only); srt_src and
 * out_dst may be NULL for a graph without edges.  h and out are row-strided (ld_h, ld_out >= hidden, multiples of 4; 16-byte aligned):
 * column blocks of a wider table - of the same one, too, as long as they do not overlap.  hidden in {64,128,256}.
 * One wave per node, no atomics; the association is fixed and a function of the graph alone (self term, in-list ascending, out-list
 * ascending; lists above 4096 items in fixed 128-item blocks - csrc/node_neighbour.hip), so two runs leave equal bits.  A hub is walked
 * by its own wave: about a millisecond per 10^5 neighbours (an estimate). */
int gnnome_node_neighbour_sum_f32(const float* h, int ld_h, int hidden, int64_t num_nodes, const int32_t* in_ptr, const int32_t* srt_src,
                                  const int32_t* out_ptr, const int32_t* out_dst, const float* sscale, const float* dscale, float* out,
                                  int ld_out, void* stream);

/* x[r, 0..hidden) <- relu(x[r, 0..hidden)) in place for r < rows, row stride ld (a multiple of 4; x 16-byte aligned, hidden % 4 == 0):
 * the ReLU between two layers of GCN_processor / SAGE_processor (processor.py:44, :82).  NaN stays NaN. */
int gnnome_relu_rows_f32(float* x, int ld, int64_t rows, int hidden, void* stream);

/* ---- the neighbour sum's gradient with respect to h, with the training step's element-wise epilogue ------
 * For every node j < num_nodes:
 *   s     = rscale[j] * g[j,:] + sum_{q in out(j)} rscale[out_dst[q]] * g[out_dst[q],:]
 *                              + sum_{p in in(j)} rscale[srt_src[p]] * g[srt_src[p],:]                       (last sum: both != 0 only)
 *   v     = oscale[j] * s ;  v = add[j,:] + v ;  v = v * mult[j,:] ;  out[j,:] = y[j,:] > 0 ? v : 0
 * each of the four steps skipped where its operand is NULL, each one fp32 rounding of its own (never contracted into an fma), so the
 * result equals the four element-wise passes bit for bit.  Replaces what torch autograd runs in the reference's training loop
 * (train.py:328-330) for DGL's GraphConv(norm='both') and SAGEConv('mean') on g' under layers/processor.py:35-46 and :73-84 - the
 * transposed message passing, then the backward of SAGEConv's feat_drop and of the ReLU of :44 / :82:
 *   GCN   g = dA, rscale = din'^-1/2, oscale = dout'^-1/2, y = the layer's post-ReLU input (NULL at layer 0)
 *   SAGE  g = dT[:, H:], rscale = 1/din', add = dT[:, :H], mult = the layer's scaled keep-mask, y = its stored input h_d (NULL at layer 0)
 * rscale is gnnome_node_neighbour_sum_f32's dscale, oscale its sscale; out(j) = [out_ptr[j], out_ptr[j+1]) of out_dst, in(j) =
 * [in_ptr[j], in_ptr[j+1]) of srt_src; in_ptr is read with `both` only, out_dst and srt_src may be NULL for a graph without edges.
 * g, add, mult, y and out are row-strided [N,hidden] tables, each with its own row stride (>= hidden, a multiple of 4) and 16-byte
 * aligned - column blocks of wider tables; out must not alias g or add.  hidden in {64,128,256}; num_nodes == 0 returns at once.
 * One wave per node, no atomics, the forward kernel's lane mapping and association (self term, out-list ascending, in-list ascending;
 * lists above 4096 items in fixed 128-item blocks - csrc/node_neighbour.h): with oscale alone the bits are those of
 * gnnome_node_neighbour_sum_f32 on the reversed graph with sscale = rscale, dscale = oscale, and two runs leave equal bits. */
int gnnome_node_neighbour_sum_bwd_f32(const float* g, int ld_g, int hidden, int64_t num_nodes, const int32_t* out_ptr, const int32_t* out_dst,
                                      const int32_t* in_ptr, const int32_t* srt_src, int both, const float* rscale, const float* oscale,
                                      const float* add, int ld_add, const float* mult, int ld_mult, const float* y, int ld_y, float* out,
                                      int ld_out, void* stream);

/* ---- the two neighbour sums on one rank's shard of a destination-range partition --------------------------
 * GCNModel (models/full_graph.py:56-75, layers/processor.py:35-46) and SAGEModel (full_graph.py:100-119, processor.py:73-84) per rank.
 * The shard is the DEFAULT partition: num_nodes_out owned nodes first, then the halo, every edge with an owned end kept - so an owned
 * node's in-list AND out-list are complete, in the whole graph's order.  h / g, sscale / rscale are [num_nodes_local] tables (the halo
 * rows fetched from their owners), in_ptr and out_ptr have num_nodes_local + 1 entries, neighbour ids are < num_nodes_local.  out,
 * dscale / oscale, add, mult and y are read and written at the computed rows (< num_nodes_out) only: no wave is spent on a halo row
 * and no [num_nodes_local, H] output exists.  num_nodes_out <= num_nodes_local is required (GNNOME_EINVAL otherwise, as for a NULL
 * required pointer or a hidden outside {64,128,256}).
 * rows: NULL - the rows 0 .. num_nodes_out, num_rows ignored - or int32[num_rows] DISTINCT owned row ids (the caller's contract, as
 * in_ptr is): the launch computes exactly those rows, one wave per listed row, and leaves every other output row untouched;
 * num_rows == 0 launches nothing and returns GNNOME_OK.  A rank launches its INTERIOR rows (no list entry is a halo id) while the
 * halo exchange is in flight and its BOUNDARY rows after it.
 * BIT EQUALITY: the device code, lane mapping and association are the whole-graph entries' (csrc/node_neighbour.h is the single copy);
 * the bits of a row depend on that row's lists and the table rows they name alone.  So with num_nodes_out == num_nodes_local and
 * rows == NULL the result is the whole-graph entry's bit for bit, any split into row lists gives the unsplit result bit for bit, and
 * an owned row of a shard whose tables hold the whole graph's rows equals the whole-graph entry's row at any world size - forward,
 * and backward once the halo rows of g have been fetched.  Per layer a rank therefore needs ONE forward exchange (h) and ONE
 * forward-direction exchange of g in the backward, each of the size of the symmetric model's halo exchange; no halo transpose, no
 * partial sums.  No atomics; lists above 4096 items in the fixed 128-item blocks. */
int gnnome_node_neighbour_sum_part_f32(const float* h, int ld_h, int hidden, int64_t num_nodes_out, int64_t num_nodes_local,
                                       const int32_t* rows, int64_t num_rows, const int32_t* in_ptr, const int32_t* srt_src,
                                       const int32_t* out_ptr, const int32_t* out_dst, const float* sscale, const float* dscale, float* out,
                                       int ld_out, void* stream);
int gnnome_node_neighbour_sum_bwd_part_f32(const float* g, int ld_g, int hidden, int64_t num_nodes_out, int64_t num_nodes_local,
                                           const int32_t* rows, int64_t num_rows, const int32_t* out_ptr, const int32_t* out_dst,
                                           const int32_t* in_ptr, const int32_t* srt_src, int both, const float* rscale, const float* oscale,
                                           const float* add, int ld_add, const float* mult, int ld_mult, const float* y, int ld_y,
                                           float* out, int ld_out, void* stream);

/* x[r, 0..hidden) <- relu(x[r, 0..hidden)) * mult[r, 0..hidden) in place for r < rows (relu == 0: x <- x * mult, the encoder's output
 * has no ReLU): SAGEConv's feat_drop (processor.py:77) on a layer's input, applied where the ReLU of :82 touches the row.  mult is the
 * scaled keep-mask, 0 or 1/(1-p); NULL is GNNOME_EINVAL (gnnome_relu_rows_f32 is the ReLU alone).  Row strides ld, ld_mult multiples of
 * 4, both tables 16-byte aligned and distinct, hidden % 4 == 0.  NaN stays NaN. */
int gnnome_relu_mul_rows_f32(float* x, int ld, const float* mult, int ld_mult, int64_t rows, int hidden, int relu, void* stream);

/* ---- edge-softmax attention sum: the message passing of GATModel ---------------------------------------
 * For every node i < num_nodes and head k < heads, over N'(i) = {i} + in(i) (+ out(i) when out_ptr != NULL), parallel edges and loops
 * as separate items:
 *   a_{p,k}     = softmax over p in N'(i) of leaky_relu(el[nbr_p,k] + er[i,k], negative_slope)
 *   out[i,k,:]  = sum_{p in N'(i)} a_{p,k} * feat[nbr_p,k,:] + bias[k,:]
 * Replaces everything after el / er in DGL's GATConv(hidden, hidden, num_heads=3) of layers/processor.py:49-70 on
 * g' = dgl.add_self_loop(g) (directed=True) or add_self_loop(add_reverse_edges(g)) (directed=False), models/full_graph.py:78-97.
 * g' is never built: in(i) = [in_ptr[i], in_ptr[i+1]) of srt_src, out(i) = [out_ptr[i], out_ptr[i+1]) of out_dst (the arrays of
 * gnnome_build_graph_views), the loop edge is the node's own row and counts once more where the graph already has one.
 * feat and out are [N, heads*hidden] (head k in columns [k*hidden, (k+1)*hidden)), row-strided (ld_feat, ld_out multiples of 4, 16-byte
 * aligned), out must not alias feat; el and er are per-node rows of 4 floats - the three heads and a pad - with row strides ld_el,
 * ld_er (multiples of 4, 16-byte aligned): all of them may be column blocks of one projection table.  bias[heads*hidden] may be NULL.
 * out_ptr == NULL selects the directed form; srt_src and out_dst may be NULL for a graph without edges.  hidden in {64,128,256},
 * heads == 3; anything else is GNNOME_EINVAL.
 * One wave per node, two passes (the per-head maximum over the 16-byte score rows, then exp(s - max), an fp32 numerator and
 * denominator, one division per (node, head)), no atomics.  The association is fixed and a function of the graph alone (self term,
 * in-list ascending, out-list ascending; lists above 4096 items in fixed 128-item blocks, numerator and denominator alike -
 * csrc/node_attention.hip), so two runs leave equal bits.  A NaN in el, er or feat of any member of N'(i) leaves a non-finite out[i,k,:].
 * A node that sees its loop alone gets out = feat + bias bit for bit.  A hub is walked by its own wave: about three milliseconds per 10^5
 * neighbours (an estimate). */
int gnnome_node_attention_sum_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er, int hidden,
                                  int heads, int64_t num_nodes, const int32_t* in_ptr, const int32_t* srt_src, const int32_t* out_ptr,
                                  const int32_t* out_dst, float negative_slope, const float* bias, float* out, int ld_out, void* stream);

/* The TRAINING FORM of gnnome_node_attention_sum_f32: the same arguments and, bit for bit, the same `out` (one kernel template, the
 * statistics behind a compile-time flag), plus per node a row of 8 floats in `stats` (row stride ld_stats >= 8, a multiple of 4; 16-byte
 * aligned; distinct from feat, el, er and out):  m0 m1 m2 0 | 1/den0 1/den1 1/den2 0  - per head the maximum of the leaky-relu scores over
 * N'(i) and the reciprocal of the sum of exp(s - m) that divided the numerator.  A weight of the forward is then
 * exp2((s - m) * log2(e)) * (1/den) again, which is how gnnome_node_attention_sum_bwd_f32 recomputes it. */
int gnnome_node_attention_sum_stats_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er, int hidden,
                                        int heads, int64_t num_nodes, const int32_t* in_ptr, const int32_t* srt_src, const int32_t* out_ptr,
                                        const int32_t* out_dst, float negative_slope, const float* bias, float* out, int ld_out, float* stats,
                                        int ld_stats, void* stream);

/* ---- the attention sum's gradient with respect to feat, el and er ----------------------------------------
 * Given g = d out [N, heads*hidden] and the forward's feat, el, er, out (= A, with its bias), bias (NULL as in the forward) and stats,
 * for every head k and every edge p = (j -> i) of g', loops included:
 *   x_p = el[j,k] + er[i,k]     a_p = exp2((leaky_relu(x_p) - m[i,k]) * log2(e)) * inv_den[i,k]
 *   D[i,k]       = g[i,k,:] . (out[i,k,:] - bias[k,:])
 *   dx_p         = a_p * (x_p > 0 ? 1 : negative_slope) * (g[i,k,:] . feat[j,k,:] - D[i,k])
 *   dfeat[j,k,:] = sum_{p: src(p) = j} a_p g[dst(p),k,:]     del[j,k] = sum_{p: src(p) = j} dx_p     der[i,k] = sum_{p: dst(p) = i} dx_p
 * Replaces what torch autograd runs in the reference's training loop (train.py:328-330) for DGL's GATConv(hidden, hidden, num_heads=3)
 * of layers/processor.py:49-70 on g' (models/full_graph.py:78-97): the backward of u_mul_e_sum, edge_softmax, leaky_relu and u_add_v.
 * d bias is the column sums of g (gnnome_colsum2_f32), not written here.
 * dfeat is [N, heads*hidden], del and der rows of 4 floats (pad column written 0), each row-strided (multiples of 4, 16-byte aligned):
 * they may be the column blocks of one [N, 3*hidden + 64] table laid out like the projection; the kernels write nothing but these three
 * blocks, the table's remaining score columns are the caller's to zero.  work: num_nodes * 16 floats of scratch, 16-byte aligned (per
 * destination er | m | 1/den | D, written by the first launch, read by the second).  No output may alias an input or another output.
 * in_ptr and out_ptr are BOTH required (the per-destination walk reads the in-list, the per-source walk the out-list): `both` != 0
 * selects the doubled graph of directed=False, not a NULL out_ptr; srt_src and out_dst may be NULL for a graph without edges.
 * hidden in {64,128,256}, heads == 3, anything else GNNOME_EINVAL; num_nodes == 0 returns at once.
 * Two launches, one wave per node each (per destination: D, der and the work row; per source: dfeat and del), the forward's lane mapping,
 * no atomics, fp32; the association is fixed and a function of the graph alone (the loop's term, then the lists ascending; lists above
 * 4096 items in fixed 128-item blocks - csrc/node_attention_bwd.hip), so two runs leave equal bits; a node without edges gets
 * dfeat = g bit for bit.  A hub is walked by its own wave: about three milliseconds per 10^5 items per launch (an estimate). */
int gnnome_node_attention_sum_bwd_f32(const float* g, int ld_g, const float* feat, int ld_feat, const float* el, int ld_el, const float* er,
                                      int ld_er, const float* out, int ld_out, const float* bias, const float* stats, int ld_stats, int hidden,
                                      int heads, int64_t num_nodes, const int32_t* in_ptr, const int32_t* srt_src, const int32_t* out_ptr,
                                      const int32_t* out_dst, int both, float negative_slope, float* dfeat, int ld_dfeat, float* del, int ld_del,
                                      float* der, int ld_der, float* work, void* stream);

/* ---- the attention sum on one rank's shard of a destination-range partition -----------------------------
 * GATModel (models/full_graph.py:78-97, layers/processor.py:49-70) per rank.  The shard is the DEFAULT partition, as for the two
 * neighbour sums above: num_nodes_out owned nodes first, then the halo, every edge with an owned end kept - so an owned node's in-list
 * AND out-list are complete, in the whole graph's order, and every softmax of an owned destination sees all of its terms.  in_ptr and
 * out_ptr have num_nodes_local + 1 entries (the first num_nodes_out + 1 are read), neighbour ids are < num_nodes_local.
 * num_nodes_out <= num_nodes_local is required: GNNOME_EINVAL otherwise, as for heads != 3, a hidden outside {64,128,256}, a NULL
 * required pointer or a bad stride - the whole-graph entries' argument errors, checked before anything is launched.  num_nodes_out == 0
 * returns at once.  Strides, alignment and aliasing rules are the whole-graph entries'.
 *
 * FORWARD, the two forms: feat and el are tables of num_nodes_local rows (the halo rows projected locally or fetched); er, out and
 * stats are read and written at rows < num_nodes_out only.  No wave is spent on a halo row and no [num_nodes_local, 3*hidden] output
 * exists.
 *
 * BACKWARD, the two launches of gnnome_node_attention_sum_bwd_f32 as separate entries, because on a partition a collective sits between
 * them:
 *   the DESTINATION phase computes D, der and the 16-float work row  er | m | 1/den | D  of the owned rows.  It reads g, out, stats and
 *     er at owned rows, feat / el at any local row through the in-list and, with `both`, the out-list, and writes der rows and work rows
 *     < num_nodes_out of a [num_nodes_local, 16] table - the rows at and above num_nodes_out are not touched;
 *   the SOURCE phase computes dfeat and del of the owned rows.  It reads feat / el at owned rows and g and work at ANY local row through
 *     the out-list and, with `both`, the in-list: the caller fills the halo rows of g and of work - from their owners, two
 *     forward-direction exchanges of 3*hidden and of 16 floats per halo row - between the two phases.
 * Every edge's term of dfeat[j] / del[j] is computed by j's owner and its term of der[i] by i's owner: no halo transpose, no partial sums.
 *
 * BIT EQUALITY: the part entries launch the whole-graph entries' kernels over the owned rows - the row code, lane mapping and
 * association (the loop's term first, lists ascending, 128-item blocks above 4096 items) exist once, in csrc/node_attention.hip and
 * csrc/node_attention_bwd.hip.  The bits of an owned row depend only on that row's lists and the table rows they name.  So with
 * num_nodes_out == num_nodes_local the part entries equal the whole-graph entries bit for bit; the destination phase followed by the
 * source phase on a whole table equals gnnome_node_attention_sum_bwd_f32, work included; and an owned row of a shard whose tables hold
 * the whole graph's rows equals the whole-graph entry's row at any world size. */
int gnnome_node_attention_sum_part_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er, int hidden,
                                       int heads, int64_t num_nodes_out, int64_t num_nodes_local, const int32_t* in_ptr,
                                       const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_dst, float negative_slope,
                                       const float* bias, float* out, int ld_out, void* stream);
int gnnome_node_attention_sum_stats_part_f32(const float* feat, int ld_feat, const float* el, int ld_el, const float* er, int ld_er,
                                             int hidden, int heads, int64_t num_nodes_out, int64_t num_nodes_local, const int32_t* in_ptr,
                                             const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_dst, float negative_slope,
                                             const float* bias, float* out, int ld_out, float* stats, int ld_stats, void* stream);
int gnnome_node_attention_sum_bwd_dst_part_f32(const float* g, int ld_g, const float* feat, int ld_feat, const float* el, int ld_el,
                                               const float* er, int ld_er, const float* out, int ld_out, const float* bias,
                                               const float* stats, int ld_stats, int hidden, int heads, int64_t num_nodes_out,
                                               int64_t num_nodes_local, const int32_t* in_ptr, const int32_t* srt_src,
                                               const int32_t* out_ptr, const int32_t* out_dst, int both, float negative_slope, float* der,
                                               int ld_der, float* work, void* stream);
int gnnome_node_attention_sum_bwd_src_part_f32(const float* g, int ld_g, const float* feat, int ld_feat, const float* el, int ld_el,
                                               const float* work, int hidden, int heads, int64_t num_nodes_out, int64_t num_nodes_local,
                                               const int32_t* out_ptr, const int32_t* out_dst, const int32_t* in_ptr,
                                               const int32_t* srt_src, int both, float negative_slope, float* dfeat, int ld_dfeat,
                                               float* del, int ld_del, void* stream);

/* ---- streaming aggregation (round 5) -----------------------------------------------------------------
 * The same node update as gnnome_node_aggregate_f32 with norm_kind = GNNOME_NORM_AFFINE (gated_gcn_full.py:111-114, :124-127,
 * :129-137), with every e row read ONCE: the rows are streamed in destination order, the in-edge sums are reduced per run, and a
 * row's contribution to its SOURCE node (the out-edge sums of dgl.reverse(g), :125-126) is accumulated in a window of slots in LDS.
 * What a row does to which slot is a SCHEDULE, a function of the graph alone, built once per graph:
 *   - the nodes are cut into num_chunks ranges of consecutive destination nodes with about equal numbers of in-edge rows
 *     (chunk_node[num_chunks + 1]); one workgroup walks one chunk, a wave of it one 32-channel slice of the rows;
 *   - a chunk's rows are walked in STEPS of <= rows_per_step (16) rows of ONE destination node: steps[][4] =
 *     {first row, node, count | flags | slot << 16, pending index}; chunk c's steps start at in_ptr[chunk_node[c]] / 16 +
 *     chunk_node[c], chunk_steps[c] of them (capacity from gnnome_stream_schedule_sizes);
 *   - edge_meta[p]: 0xFF = FAR (source in another chunk, a repeated (src, dst) pair, or no free slot: the stream skips the row's
 *     out-edge half), else state << 6 | slot, state 0 / 1 = accumulate, 2 / 3 = the LAST event of the row's source - that row
 *     also runs the source's node update (3: the source is pending);
 *   - a node with far rows is PENDING (node_pend[node] = its index, pend_nodes[index] = node, counters[0] = their number): its
 *     last event parks (A1h + fwd, num_b, den_b) in pend_rows[index][3][H], and a second launch adds the far rows in out-list
 *     order and finishes the update.
 * counters[8] (device): [0] pending nodes, [1] far rows, [2] nodes that found no free slot, [3] most slots in use, [4] most
 * steps in a chunk.  A caller reads [0] back once to size pend_rows and decides from [1] / E whether the graph's numbering has
 * the locality this form needs (a uniform random graph is all far rows: use gnnome_node_aggregate_f32).  num_slots <= 62.
 * Results are bit-reproducible and equal gnnome_node_aggregate_f32's up to fp32 reassociation (and 1-ulp reciprocals).
 * h_out must not alias h_in; hidden in {64,128,256}. */
int gnnome_stream_schedule_sizes(int64_t num_nodes, int64_t num_edges, int rows_per_step, int64_t* steps_capacity_host,
                                 size_t* scratch_bytes_host);
int gnnome_build_stream_schedule(int64_t num_nodes, int64_t num_edges, const int32_t* in_ptr, const int32_t* srt_src,
                                 const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, int num_chunks,
                                 int rows_per_step, int num_slots, int32_t* chunk_node, int32_t* chunk_steps, int32_t* steps,
                                 uint8_t* edge_meta, int32_t* node_pend, int32_t* pend_nodes, int32_t* counters, void* scratch,
                                 size_t scratch_bytes, void* stream);
int gnnome_node_aggregate_stream_f32(const float* e, int hidden, int64_t num_nodes, int64_t num_edges, const float* A1h, const float* A2h,
                                     const float* A3h, int ld_node, const int32_t* in_ptr, const int32_t* srt_src,
                                     const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const float* h_in,
                                     int ld_h, float* h_out, const float* norm_scale, const float* norm_shift, int num_chunks,
                                     int rows_per_step, int num_slots, const int32_t* chunk_node, const int32_t* chunk_steps,
                                     const int32_t* steps, const uint8_t* edge_meta, const int32_t* node_pend,
                                     const int32_t* pend_nodes, const int32_t* counters, int64_t num_pending, float* pend_rows,
                                     void* stream);

/* ---- fused edge scorer --------------------------------------------------------------------------
 * For every sorted position p < num_edges:
 *   z1 = relu(Ps[srt_src[p],:] + Qd[srt_dst[p],:] + e[p,:] * W1e^T)        (b1 folded into Qd)
 *   logits[eid(p)] = W3 . relu(W2 * z1 + b2) + b3,   eid(p) = srt_eid ? srt_eid[p] : p
 * Replaces ScorePredictor.apply_edges (score_predictor.py:12-17) without materialising the
 * [E,3H] concatenation; W1e is the third column block of predictor.W1 (row stride ldw1 = 3H).
 *   hidden in {64,128,256}; hidden_edge_scores in {32,64,128}; W2 is [32,hs], W3 is [32]
 */
int gnnome_edge_score_f32(const float* e, int64_t num_edges, int hidden, int hidden_edge_scores,
                          const float* Ps, const float* Qd, int ld_node, const int32_t* srt_src,
                          const int32_t* srt_dst, const int32_t* srt_eid, const float* W1e, int ldw1,
                          const float* W2, const float* b2, const float* W3, const float* b3, float* logits,
                          float* z1_out /* NULL, or [E,hs]: relu(z1) kept for the backward */, void* stream);

/* ---- the whole eval forward as ONE call (round 6) ---------------------------------------------------
 * models/full_graph.py:22-30 - `x = linear2_node(relu(linear1_node(x))); e = linear2_edge(relu(linear1_edge(e)));
 * x, e = gnn(graph, x, e); scores = predictor(graph, x, e)` - i.e. what inference.py:440 calls once per graph, enqueued from C on one
 * stream: encoders -> num_layers x (node projection, edge gate, gated aggregation + node update: layers/processor.py:16-19 over
 * gated_gcn_full.py:84-142) -> score_predictor.py:12-24.  It calls the per-kernel entries above in exactly the order
 * gnnome_amd/engine.py::run_stack calls them (same kernels, same bits; tests/test_model_forward_entry.py), so a caller that scores each graph
 * once (where a hipGraph replay does not help) pays one host call instead of ~30.  No allocation, no host synchronisation, capturable.
 *   gnnome_layer_params: one SymGatedGCN layer with eval semantics - Wcat = rows A_1 | A_2 | A_3 | B_1 | B_2 (gated_gcn_full.py:29-33,91-96),
 *     bcat their biases (not reference_order: B_3's bias added to the B_2 block, it rides on the B2h rows), Wcat_planes =
 *     gnnome_weight_planes_f16(Wcat) or NULL, W3 / b3 = B_3 (:34,97), norm_kind + scale / shift = bn_e and bn_h folded as the fused
 *     kernels take them (:37-42,106,132); reference_order != 0: the layer's dense products in the reference's order of evaluation
 *     (gnnome_linear_ref_f32 / gnnome_edge_gate_ref_f32)
 *   gnnome_model_params: encoders (models/full_graph.py:13-16), layers (a HOST array), predictor with W1 split as the scorer takes it:
 *     W_nodes [2 hs, H] = W1's x[src] block over its x[dst] block, b_nodes = [0 | b1], W1e [hs, H] = W1's e block (score_predictor.py:13)
 *   gnnome_views: the arrays of gnnome_build_graph_views; node_gather: NULL, or the row of x each node of the views' numbering reads
 *     (views over renumbered nodes); transposed != 0: the views describe dgl.reverse(g) (train.py:165) - src / dst roles swapped
 *   workspace: gnnome_model_forward_workspace_bytes(...) bytes, 256-byte aligned; logits [E] in EDGE-ID order (what the model returns,
 *     squeezed).  hidden in {64, 128, 256}, score_hidden in {32, 64, 128}: narrower models are zero-padded by the caller (engine.Prepared). */
typedef struct gnnome_layer_params {
    const float* Wcat;
    const void* Wcat_planes;
    const float* bcat;
    const float* W3;
    const float* b3;
    const float* scale_e;
    const float* shift_e;
    const float* scale_h;
    const float* shift_h;
    int32_t norm_kind;
    int32_t reference_order;
} gnnome_layer_params;

typedef struct gnnome_model_params {
    int32_t hidden, hidden_ne, num_layers, score_hidden, node_features, edge_features;
    const float *node_W1, *node_b1, *node_W2, *node_b2;   /* linear1_node [hidden_ne, node_features], linear2_node [hidden, hidden_ne] */
    const float *edge_W1, *edge_b1, *edge_W2, *edge_b2;   /* linear1_edge, linear2_edge */
    const gnnome_layer_params* layers_host;                /* [num_layers], host memory */
    const float* W_nodes;
    const void* W_nodes_planes;                            /* gnnome_weight_planes_f16(W_nodes) or NULL */
    const float* b_nodes;
    const float* W1e;
    int32_t ld_w1e, reserved;
    const float *W2, *b2, *W3, *b3;                        /* predictor.W2 [32, hs], W3 [32], biases */
} gnnome_model_params;

typedef struct gnnome_views {
    int64_t num_nodes, num_edges;
    const int32_t *in_ptr, *srt_src, *srt_dst, *srt_eid, *out_ptr, *out_pos, *out_dst;
    const int32_t* node_gather;
    int32_t transposed, reserved;
} gnnome_views;

/* Measurement only (bench.py's live `roofline`): four hipEvent_t (as void*) that every following gnnome_model_forward_f32 of the calling thread
 * records on its stream around layer `layer`'s edge-gate launch (start, stop) and its aggregation launch (start, stop); NULLs / layer < 0: off. */
int gnnome_debug_forward_events(void* gate_start, void* gate_stop, void* aggregate_start, void* aggregate_stop, int layer);
int gnnome_model_forward_workspace_bytes(int64_t num_nodes, int64_t num_edges, int hidden, int score_hidden, size_t* bytes_host);
int gnnome_model_forward_f32(const gnnome_model_params* params_host, const gnnome_views* views_host, const float* x, const float* e_raw,
                             float* logits, void* workspace, size_t workspace_bytes, void* stream);
/* The same forward on buffers the caller allocated one by one instead of one workspace block (round 6): where the driver places a buffer in HBM is
 * worth ~3 % of the forward at configs[1], and separate allocations come out on the fast side more often than one block holding everything
 * (NOTES.md round 6).  h[0], h[1] [N, hidden]; P [N, 5 hidden]; e[0] [E, hidden], and e[1] (another [E, hidden], used at hidden = 256 only, may be NULL
 * otherwise); PQ [N, 2 score_hidden]; all 16-byte aligned, distinct, contents undefined on entry and on return. */
typedef struct gnnome_forward_buffers {
    float* h[2];
    float* P;
    float* e[2];
    float* PQ;
} gnnome_forward_buffers;
int gnnome_model_forward_buffers_f32(const gnnome_model_params* params_host, const gnnome_views* views_host, const float* x, const float* e_raw,
                                     float* logits, const gnnome_forward_buffers* buffers_host, void* stream);

/* ================================================================================================
 * Training step (train.py:138-145 + :328-330: forward in train mode, BCE-with-logits, loss.backward()).
 * The reference gets its backward from torch autograd over DGL's gspmm/gsddmm; here the layer backward is
 * written out in gnnome_amd/train.py and built from the entries below.  All are stream-ordered.
 * ================================================================================================ */

/* x_out[p,:] = B1h[srt_src[p],:] + B2h[srt_dst[p],:] + e_in[p,:] * W3^T  - the input of bn_e
 * (gated_gcn_full.py:104-106) materialised so that train-mode BatchNorm can take batch statistics. */
int gnnome_edge_gate_raw_f32(const float* e_in, float* x_out, int64_t num_edges, int hidden, const float* B1h,
                             const float* B2h, int ld_node, const int32_t* srt_src, const int32_t* srt_dst,
                             const float* W3, int ldw, void* stream);

/* The same, with the BatchNorm batch statistics gathered on the way (hidden in {64,128,256}): every workgroup writes
 * its shifted column sums  stats_partial[w][c] = sum (x - center[c]),  stats_partial[w][hidden + c] = sum (x - center[c])^2
 * over the rows it produced; w < R = gnnome_edge_gate_raw_stats_rows(hidden).  (hidden = 256: two stacked matrices instead,
 * stats_partial[0][w][c] the sums and stats_partial[1][w][c] the sums of squares, 2 * R * 256 floats in all, and x_out
 * must not alias e_in.)  Summing the rows of stats_partial (in any
 * FIXED order, e.g. gnnome_colsum2_f32) gives the sums the statistics need without a second pass over x_out.
 * center: any per-column value near the column mean (row 0 of x_out is one) - the shift keeps the second moment
 * free of cancellation.
 * R depends on the kernel that gnnome_set_tuning key 0 selects at the time of the call: at hidden = 64 / 128, 8 rows per CU (2048) for
 * the bf16x6 edge-tile kernels (key 0 = 0 or 8) and 2 / 1 rows per CU for the exact-fp32 kernel (every other value); at hidden = 256,
 * 4 rows per workgroup of the plane form whatever key 0 says.  Ask for R under the key 0 the launch will run with.  The bf16-storage
 * form (gnnome_edge_gate_raw_stats_x16) exists on the bf16x6 kernels only: at hidden = 64 / 128 under another key 0 it is refused
 * (GNNOME_EINVAL) - R would be sized for a kernel that does not run. */
/* x_out == NULL (hidden = 128): the statistics alone - the first pass of the two-pass training forward (round 4): the product is cheap on the
 * matrix cores (fp16x3), a written and re-read [E,H] tensor is not.  The second pass is gnnome_edge_gate_bn_f32 below. */
int gnnome_edge_gate_raw_stats_rows(int hidden, int* rows_host);
int gnnome_edge_gate_raw_stats_f32(const float* e_in, float* x_out, int64_t num_edges, int hidden, const float* B1h,
                                   const float* B2h, int ld_node, const int32_t* srt_src, const int32_t* srt_dst,
                                   const float* W3, int ldw, const float* center, float* stats_partial, void* stream);
/* e_out = relu(xe * scale + shift) + e_in  AND  x_out = xe = e_in W3^T + B1h[src] + B2h[dst]: the train-mode gate once the batch statistics are
 * known (scale = gamma * rstd, shift = beta - mean * scale): what gnnome_edge_gate_raw_f32 + gnnome_bn_relu_res_f32 did in two passes over
 * [E,H] (gated_gcn_full.py:97,104-110 under train()).  hidden = 128; e_out, x_out and e_in distinct. */
int gnnome_edge_gate_bn_f32(const float* e_in, float* e_out, float* x_out, int64_t num_edges, int hidden, const float* B1h,
                            const float* B2h, int ld_node, const int32_t* srt_src, const int32_t* srt_dst, const float* W3, int ldw,
                            const float* scale, const float* shift, void* stream);

/* Gated aggregation without the node epilogue.
 *   mode 1: v_out = A1h + fwd + bwd (input of bn_h, gated_gcn_full.py:129); aux0 = fwd, aux1 = 1/(den_f+1e-6),
 *           aux2 = bwd, aux3 = 1/(den_b+1e-6)   (kept for the backward)
 *   mode 2: aux0[i] = sum_{in(i)} s_p * A2h[srt_src[p]], aux2[i] = sum_{out(i)} s_p * A3h[out_dst[q]] (raw sums:
 *           with A2h := dv/(den_b+eps), A3h := dv/(den_f+eps) these are dA3h and dA2h) */
int gnnome_node_aggregate_raw_f32(const float* e, int hidden, int64_t num_nodes, int mode, const float* A1h,
                                  const float* A2h, const float* A3h, int ld_node, const int32_t* in_ptr,
                                  const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos,
                                  const int32_t* out_dst, float* v_out, float* aux0, float* aux1, float* aux2,
                                  float* aux3, void* stream);

/* s1[c] = sum_r x'[r,c];  s2[c] = sum_r x'[r,c]*y'[r,c]  with x' = x - center[c] (center NULL: 0) and y NULL -> x'
 * (sum of squares).  s1/s2 are overwritten (rows = 0: left untouched).  hidden in {16,32,64,128,256}.  Two calls give train-mode
 * BatchNorm its batch statistics (gated_gcn_full.py:106,119,132): the mean, then the centred second moment - the
 * one-pass E[x^2]-E[x]^2 form cancels badly on this path (|e| ~ 500, spread of a few units).  Also bias gradients.
 * The sum over workgroups is deterministic (partials parked in `workspace`, added up in workgroup order by a second
 * small kernel), so BatchNorm statistics and bias gradients are bit-identical from run to run.  workspace:
 * gnnome_colsum_workspace_bytes() bytes, 16-byte aligned, not shared by launches that may run concurrently. */
int gnnome_colsum_workspace_bytes(size_t* bytes_host);
int gnnome_colsum2_f32(const float* x, const float* y, int64_t rows, int hidden, const float* center, float* s1,
                       float* s2, void* workspace, size_t workspace_bytes, void* stream);

/* out = relu(x*scale[c] + shift[c]) + res : train-mode bn + relu + residual (gated_gcn_full.py:106-110, 132-137) */
int gnnome_bn_relu_res_f32(const float* x, const float* scale, const float* shift, const float* res, int64_t rows,
                           int hidden, float* out, void* stream);

/* BatchNorm backward through the relu of out = relu(x*scale + shift) + res, m = (x*scale + shift > 0):
 *   stats: s1[c] = sum_r dy*m,  s2[c] = sum_r dy*m*(x - mean[c])   (overwritten)
 *   apply: dx = a[c] * (dy*m - c1[c] - (x - mean[c])*rstd[c]*c2[c]) */
int gnnome_bn_bwd_stats_f32(const float* dy, const float* x, const float* scale, const float* shift,
                            const float* mean, int64_t rows, int hidden, float* s1, float* s2, void* workspace,
                            size_t workspace_bytes, void* stream);
int gnnome_bn_bwd_apply_f32(const float* dy, const float* x, const float* scale, const float* shift, int64_t rows,
                            int hidden, const float* a, const float* c1, const float* c2, const float* mean,
                            const float* rstd, float* dx, void* stream);

/* gnnome_bn_bwd_apply_f32 for bn_h of a layer WITH the four node tables of the aggregation's backward in the same pass (round 5; what two
 * gnnome_mul23_f32 launches made of dx, each reading it again):  Tf = dx rdf,  Uf = Tf hf,  Tb = dx rdb,  Ub = Tb hb, all [rows, hidden]
 * contiguous; rdf / hf / rdb / hb are the forward's gnnome_node_aggregate_raw_f32 mode-1 outputs aux1 / aux0 / aux3 / aux2. */
int gnnome_bn_bwd_apply_tables_f32(const float* dy, const float* x, const float* scale, const float* shift, int64_t rows, int hidden,
                                   const float* a, const float* c1, const float* c2, const float* mean, const float* rstd,
                                   const float* rdf, const float* hf, const float* rdb, const float* hb, float* dx, float* Tf, float* Uf,
                                   float* Tb, float* Ub, unsigned* amax_bits, void* stream);   /* amax_bits (NULL: skip): raised to max |dx| */

/* LayerNorm variant (normalization='layer', gated_gcn_full.py:40-42,106,119,132) of the two groups above:
 *   out = relu(LN(x) * gamma + beta) + res, LN over the `hidden` entries of each row (biased variance, eps 1e-5);
 *   backward: dx = rstd_row (g - mean_row(g) - xhat mean_row(g xhat)) with g = dy m gamma, m the relu mask;
 *   dbeta[c] = sum_r dy m, dgamma[c] = sum_r dy m xhat (deterministic; overwritten; workspace as colsum2). */
/* norm_width (round 5): the statistics run over the first norm_width <= hidden channels (0 = hidden) - see GNNOME_NORM_LAYER_OVER;
 * dx of a channel beyond norm_width is 0. */
int gnnome_ln_relu_res_f32(const float* x, const float* gamma, const float* beta, const float* res, int64_t rows, int hidden,
                           int norm_width, float* out, void* stream);
int gnnome_ln_bwd_f32(const float* dy, const float* x, const float* gamma, const float* beta, int64_t rows, int hidden, int norm_width,
                      float* dx, float* dbeta, float* dgamma, void* workspace, size_t workspace_bytes, void* stream);

/* o1 = a*b, o2 = a*b*c (count floats, count % 4 == 0);  out = a + b;  dx = dy*(y > 0) */
int gnnome_mul23_f32(const float* a, const float* b, const float* c, int64_t count, float* o1, float* o2, void* stream);
int gnnome_add_f32(const float* a, const float* b, int64_t count, float* out, void* stream);
int gnnome_relu_bwd_f32(const float* dy, const float* y, int64_t count, float* dx, void* stream);

/* out[i,:] = sum_{q in [ptr[i], ptr[i+1])} X[pos ? pos[q] : q, :]  width in {32,64,128,256}: the transposes of the
 * per-edge gathers (dB2h, dQd with ptr = in_ptr; dB1h, dPs with ptr = out_ptr, pos = out_pos). */
int gnnome_segment_sum_f32(const float* X, int width, const int32_t* ptr, const int32_t* pos, int64_t num_nodes,
                           float* out, int ld_out, void* stream);

/* Both segment sums of one tensor in one launch: out_in[i,:] = sum over node i's in-edge rows (ptr = in_ptr, contiguous),
 * out_out[i,:] = sum over its out-edge rows (out_ptr / out_pos).  Same values as two gnnome_segment_sum_f32 calls. */
int gnnome_segment_sum2_f32(const float* X, int width, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_pos,
                            int64_t num_nodes, float* out_in, int ld_in, float* out_out, int ld_out, void* stream);

/* C[Ka,Kb] = A[rows,Ka]^T * B[rows,Kb]: nn.Linear weight gradients on the bf16 matrix cores as the fp32-faithful
 * bf16x6 product (see gnnome_linear_f32; error of the size of an fp32 dot product's), chunked over rows with a
 * deterministic second-stage sum.  Ka, Kb % 4 == 0; A, B 16-byte aligned. */
int gnnome_wgrad_workspace_bytes(int64_t rows, int Ka, int Kb, size_t* bytes_host);
int gnnome_wgrad_f32(const float* A, int lda, int Ka, const float* B, int ldb, int Kb, int64_t rows, float* C, int ldc,
                     void* workspace, size_t workspace_bytes, void* stream);
/* gnnome_wgrad_f32 for a GRADIENT operand A whose largest magnitude is known on the device (round 5; VERDICT r4: "fp16x3 for the backward's
 * products: gradients need a per-tensor scale"): amax_bits[0] = the bits of max |A| as a non-negative float.  Where the 128 x 128 tile
 * kernel runs, the product is formed as fp16x3 - A multiplied by 2^(13 - floor(log2 max|A|)) while it is split into two fp16 planes (exact),
 * the result by the inverse - three MFMAs per k step instead of bf16x6's six; error per term <= max(2^-22 |a|, 2^-49 max|A|) |b|
 * (measured 2.6e-9 of max sum |a||b| at 1M rows against bf16x6's 8.1e-9).  B must lie in fp16's range like every operand of the forward
 * (NaN otherwise, never a wrong finite value).  Operands that take the 256 x 256 kernel ignore amax_bits (bf16x6). */
int gnnome_wgrad_scaled_f32(const float* A, int lda, int Ka, const float* B, int ldb, int Kb, int64_t rows, const unsigned* amax_bits,
                            float* C, int ldc, void* workspace, size_t workspace_bytes, void* stream);
/* The same for the column-block form (gnnome_wgrad_blocks_f32) with ONE maximum over all blocks - the slot the blocks' producers raised
 * (gnnome_bn_bwd_apply_tables_f32, gnnome_agg_bwd_fused_f32, gnnome_segment_sum2_amax_f32; the caller zeroes it once before them): fp16x3 with
 * that common scale (block_width a multiple of 128); a block much smaller than the largest keeps an absolute error of 2^-49 max|A| |b| per term. */
int gnnome_wgrad_blocks_scaled_f32(const float* const* A_blocks, int num_blocks, int block_width, int lda, const float* B, int ldb, int Kb,
                                   int64_t rows, const unsigned* amax_bits, float* C, int ldc, float* colsum, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* gnnome_linear_blocks_f32 as ONE fp16x3 launch with the blocks scaled by their common maximum (the same slot): a workgroup keeps a 128 x 128
 * tile of C in its accumulators over all of K = num_blocks x block_width (block_width a multiple of 32), so C is read and written once - the
 * data gradient dh += [dv | dA2 | dA3 | dB1 | dB2] Wcat of the node projection (gated_gcn_full.py:91-96 under autograd). */
int gnnome_linear_blocks_scaled_f32(const float* const* A_blocks, int num_blocks, int block_width, int64_t M, int lda, const float* W, int ldw,
                                    int Nout, const unsigned* amax_bits, float* C, int ldc, int accumulate, void* stream);
/* gnnome_segment_sum2_f32 that also raises amax_bits[0] to max |out_in|, |out_out| (not zeroed here) */
int gnnome_segment_sum2_amax_f32(const float* X, int width, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_pos,
                                 int64_t num_nodes, float* out_in, int ld_in, float* out_out, int ld_out, unsigned* amax_bits, void* stream);

/* The same with A given as num_blocks (1..8) column blocks of equal width in separate buffers - A_blocks is a HOST array of
 * device pointers, each [rows, block_width] with row stride lda - so that the five gradients of a layer's node projections
 * (dA1h | dA2h | dA3h | dB1h | dB2h, gated_gcn_full.py:89-95) need not be concatenated: C[num_blocks*block_width, Kb].
 * colsum (may be NULL): [num_blocks*block_width] column sums of A over the rows = the bias gradients, from the same pass.
 * Workspace: gnnome_wgrad_workspace_bytes(rows, num_blocks*block_width, Kb). */
int gnnome_wgrad_blocks_f32(const float* const* A_blocks, int num_blocks, int block_width, int lda, const float* B, int ldb,
                            int Kb, int64_t rows, float* C, int ldc, float* colsum, void* workspace, size_t workspace_bytes,
                            void* stream);

/* C[M,Nout] (accumulate != 0: +=) [A_0 | A_1 | ...] * W[Nout, num_blocks*block_width]^T with the column blocks of A in separate
 * buffers as above (block_width % 32 == 0): the backward's dh += dP * Wcat (gnnome_linear_acc_f32 on the concatenation). */
int gnnome_linear_blocks_f32(const float* const* A_blocks, int num_blocks, int block_width, int64_t M, int lda, const float* W,
                             int ldw, int Nout, float* C, int ldc, int accumulate, void* stream);

/* Backward of the scorer tail (score_predictor.py:15-16) from the saved relu(z1) and d(score) (edge-id order,
 * read through srt_eid): dz1[E,hs], dz2[E,32], u[E,32] = dscore*z2.  hs in {32,64}. */
int gnnome_score_tail_bwd_f32(const float* z1, const float* dscore, const int32_t* srt_eid, int64_t num_edges,
                              int hidden_edge_scores, const float* W2, const float* b2, const float* W3, float* dz1,
                              float* dz2, float* u, void* stream);

/* de[p,:] += s(1-s) * (Tf[dst]*A2h[src] - Uf[dst] + Tb[src]*A3h[dst] - Ub[src]),  s = sigmoid(e[p,:]):
 * the gradient the two gated aggregations send back to the edge state (gated_gcn_full.py:111-114,124-127). */
int gnnome_agg_edge_bwd_f32(const float* e, int64_t num_edges, int hidden, const float* Tf, const float* Uf,
                            const float* Tb, const float* Ub, const float* A2h, const float* A3h, int ld_node,
                            const int32_t* srt_src, const int32_t* srt_dst, float* de, void* stream);

/* t[r,:] = relu(W1*in[row(r),:] + b1): an encoder's hidden layer, recomputed for its backward */
int gnnome_encode_hidden_f32(const float* in, int64_t rows, int in_features, const int32_t* gather, const float* W1,
                             const float* b1, int hidden_ne, float* t, void* stream);

/* ---- row gather (halo packing for the destination-range partition) ------------------------------
 * out[r,:] = in[idx[r],:]   rows of `width` floats, width % 4 == 0
 */
int gnnome_gather_rows_f32(const float* in, int ld_in, const int32_t* idx, int64_t rows, int width, float* out,
                           int ld_out, void* stream);

/* out[idx[r],:] += in[r,:]  - the transpose of the halo gather: in the partitioned training step the gradient of
 * a halo row travels back to the row's owner and is added there (no reference counterpart).  The
 * rows in idx must be DISTINCT within one call (one peer's block of the exchange plan), which makes the sum
 * order, and therefore the result, deterministic. */
int gnnome_scatter_add_rows_f32(const float* in, int ld_in, const int32_t* idx, int64_t rows, int width, float* out,
                                int ld_out, void* stream);

/* ================================================================================================
 * The callers' arithmetic either side of the model call: feature preparation
 * before it, loss and confusion counts after it.  Deterministic reductions; `workspace` for all three is
 * gnnome_closure_workspace_bytes() bytes, 8-byte aligned.
 * ================================================================================================ */
int gnnome_closure_workspace_bytes(size_t* bytes_host);

/* x[N,2] = [zscore(in_degree) | zscore(out_degree)] (columns swapped when `reverse`), degrees read off the CSR
 * pointers of the graph views, mean and UNBIASED std as torch.mean / torch.std.
 * Replaces inference.py:416-420 and train.py:112-122 (get_full_ne_features). */
int gnnome_degree_features_f32(const int32_t* in_ptr, const int32_t* out_ptr, int64_t num_nodes, int reverse, float* x,
                               void* workspace, size_t workspace_bytes, void* stream);

/* e[E,2] = [zscore(overlap_length) | overlap_similarity], unbiased std.
 * Replaces utils/data_utils.py:31-41 (preprocess_graph with use_similarities, configs/hyperparameters.py:17). */
int gnnome_edge_features_f32(const float* overlap_length, const float* overlap_similarity, int64_t num_edges, float* e,
                             void* workspace, size_t workspace_bytes, void* stream);

/* loss[0] = mean_i ( bce(logits_i) [+ bce(logits_rev_i) + alpha |logits_i - logits_rev_i|] ),
 * bce = F.binary_cross_entropy_with_logits(., labels, pos_weight) - train.py:144 (logits_rev NULL) and
 * train.py:103-109 symmetry_loss (logits_rev given).  pos_weight: DEVICE scalar.  dlogits / dlogits_rev (NULL: skip) =
 * grad_scale * d(sum of per-edge terms)/d logits, so grad_scale = 1/E gives the gradient of the mean.
 * tfpn (NULL: skip) = int64[4] TP, TN, FP, FN of round(sigmoid(logits)) against labels - utils/metrics.py:6-12. */
int gnnome_edge_loss_f32(const float* logits, const float* logits_rev, const float* labels, int64_t num_edges,
                         const float* pos_weight, float alpha, float grad_scale, float* loss, float* dlogits,
                         float* dlogits_rev, int64_t* tfpn, void* workspace, size_t workspace_bytes, void* stream);

/* gnnome_bn_bwd_apply_f32 followed by gnnome_linear_acc_f32 in one pass over the [rows,hidden] tensors (hidden in {64,128}):
 *   dxe[r,:] = a (C[r,:] m - c1 - (X[r,:] - mean) rstd c2),  m = (X scale + shift > 0)        (written out)
 *   C[r,:]  += dxe[r,:] * W^T                                                                  (in place)
 * i.e. train.py's  dxe = bn_e backward(de, xe);  d e_in = d e' + dxe W3  with C = de, X = xe, W = W3^T.
 * rows_once (0 <= rows_once <= rows): the mean-subtraction terms c1, c2 enter the first rows_once rows only - on a
 * destination-range partition the rows past the owned in-edges are replicas of edges another rank owns, and those terms
 * must enter once per edge of the whole graph; rows_once = rows on a single rank. */
int gnnome_bn_bwd_dgrad_f32(float* C, const float* X, int64_t rows, int64_t rows_once, int hidden, const float* scale, const float* shift,
                            const float* a, const float* c1, const float* c2, const float* mean, const float* rstd,
                            const float* W, int ldw, float* dxe, void* stream);
/* gnnome_bn_bwd_dgrad_f32 (hidden = 128) that also leaves max |dxe| at amax_bits[0] - the bits of a non-negative float, zeroed by the call
 * and raised with atomicMax on the unsigned value (a maximum does not depend on the order it is formed in) - for gnnome_wgrad_scaled_f32. */
int gnnome_bn_bwd_dgrad_amax_f32(float* C, const float* X, int64_t rows, int64_t rows_once, int hidden, const float* scale, const float* shift,
                                 const float* a, const float* c1, const float* c2, const float* mean, const float* rstd,
                                 const float* W, int ldw, float* dxe, unsigned* amax_bits, void* stream);
/* the same at hidden = 256, OUT OF PLACE (C_out != C_in): there two workgroups - one per column half - read whole rows of C,
 * so the updated rows cannot overwrite them: C_out = C_in + dxe W^T. */
int gnnome_bn_bwd_dgrad_out_f32(const float* C_in, float* C_out, const float* X, int64_t rows, int64_t rows_once, int hidden,
                                const float* scale, const float* shift, const float* a, const float* c1, const float* c2,
                                const float* mean, const float* rstd, const float* W, int ldw, float* dxe, void* stream);
/* ... and max |dxe| left at amax_bits[0] as the bits of a non-negative float (zeroed first), as gnnome_bn_bwd_dgrad_amax_f32 does at hidden = 128:
 * gnnome_wgrad_scaled_f32(dxe, e, amax_bits) then runs B_3's weight gradient as fp16x3 (round 6). */
int gnnome_bn_bwd_dgrad_out_amax_f32(const float* C_in, float* C_out, const float* X, int64_t rows, int64_t rows_once, int hidden,
                                     const float* scale, const float* shift, const float* a, const float* c1, const float* c2,
                                     const float* mean, const float* rstd, const float* W, int ldw, float* dxe, unsigned* amax_bits, void* stream);

/* gnnome_agg_edge_bwd_f32 with the BatchNorm-backward statistics of its result gathered in the same pass:
 *   de[p,:] += s(1-s)(...)   as above, then   s1[c] = sum_p de[p,c] m,  s2[c] = sum_p de[p,c] m (xe[p,c] - mean[c]),
 *   m = (xe*scale + shift > 0): what gnnome_bn_bwd_stats_f32(de, xe, ...) would return, without its pass over de and xe. */
int gnnome_agg_edge_bwd_stats_f32(const float* e, int64_t num_edges, int hidden, const float* Tf, const float* Uf,
                                  const float* Tb, const float* Ub, const float* A2h, const float* A3h, int ld_node,
                                  const int32_t* srt_src, const int32_t* srt_dst, float* de, const float* xe, const float* scale,
                                  const float* shift, const float* mean, float* s1, float* s2, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* The aggregation's whole backward over the edges in ONE launch (round 5; the backward of gated_gcn_full.py:118-126's two gated
 * sums as autograd derives it): gnnome_node_aggregate_raw_f32 mode 2 with the tables (Tb at src, Tf at dst)
 *   sum_in[i,:]  = sum_{p: dst_p = i} sigmoid(e[p,:]) Tb[src_p,:]      sum_out[i,:] = sum_{p: src_p = i} sigmoid(e[p,:]) Tf[dst_p,:]
 * AND gnnome_agg_edge_bwd_stats_f32 (de updated in place, s1 / s2 of the result) - as two launches they stream e from HBM twice.
 * One wave per node over the destination-sorted views; num_nodes rows of Tf/Uf/Tb/Ub [., hidden] and A2h/A3h (row stride ld_node),
 * sum_in / sum_out [num_nodes, hidden] overwritten.  Equal to the two launches up to fp32 reassociation of the sums; every sum is
 * formed in an order that depends on the graph and the launch geometry only (same bits on every run).  workspace as gnnome_colsum2_f32.
 * amax_bits (NULL: skip): a slot holding the bits of a non-negative float, RAISED (atomicMax on the unsigned value, never zeroed here) to
 * max |sum_in|, |sum_out| - see gnnome_wgrad_blocks_scaled_f32. */
int gnnome_agg_bwd_fused_f32(const float* e, int64_t num_nodes, int64_t num_edges, int hidden, const float* Tf, const float* Uf,
                             const float* Tb, const float* Ub, const float* A2h, const float* A3h, int ld_node, const int32_t* in_ptr,
                             const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, float* de,
                             const float* xe, const float* scale, const float* shift, const float* mean, float* sum_in, float* sum_out,
                             float* s1, float* s2, unsigned* amax_bits, void* workspace, size_t workspace_bytes, void* stream);

/* The per-channel arithmetic of a train-mode BatchNorm1d call in one launch (gated_gcn_full.py:106,119,132 with
 * nn.BatchNorm1d's buffer semantics): from shifted column sums d1 = sum(x - center), d2 = sum((x - center)^2) over `rows`
 * rows -> mean, rstd = 1/sqrt(biased var + eps), scale = gamma*rstd, shift = beta - mean*scale, and `updates` momentum
 * updates of running_mean / running_var (unbiased variance) + num_batches_tracked += updates.  center, running_* and
 * num_batches_tracked may be NULL. */
int gnnome_bn_train_finish_f32(const float* d1, const float* d2, const float* center, int64_t rows, int hidden, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                               float momentum, float eps, int updates, float* mean, float* rstd, float* scale, float* shift,
                               void* stream);
/* BatchNorm backward, one rank: the per-channel vectors between the statistics pass and the apply pass in one launch -
 * s2h = rstd * s2, c1 = s1 / rows, c2 = s2h / rows (what torch autograd derives for nn.BatchNorm1d in train mode,
 * gated_gcn_full.py:106,119,132; the reference spends three elementwise operators on them). */
int gnnome_bn_bwd_terms_f32(const float* s1, const float* s2, const float* rstd, int64_t rows, int hidden, float* s2h, float* c1,
                            float* c2, void* stream);
/* One layer's weights as the kernels read them, in one launch (gated_gcn_full.py:91-97: the five node projections run as ONE
 * product with the stacked weight): Wcat[5H,H] = A_1|A_2|A_3|B_1|B_2 weights stacked, bcat[5H] = their biases with B_3's added
 * to B_2's, WcatT[H,5H] and W3T[H,H] = the transposes the backward's data-gradient products read.  weights5 / biases5 are HOST
 * arrays of five device pointers; hidden a multiple of 32. */
int gnnome_pack_layer_f32(const float* const* weights5, const float* const* biases5, const float* B3_weight, const float* B3_bias,
                          int hidden, float* Wcat, float* bcat, float* WcatT, float* W3T, void* stream);
/* center[:] = B1h[srt_src[0],:] + B2h[srt_dst[0],:] + e[0,:] W3^T: row 0 of the raw gate, the shift of its batch statistics. */
int gnnome_gate_center_f32(const float* e, int64_t num_edges, int hidden, const float* B1h, const float* B2h, int ld_node,
                           const int32_t* srt_src, const int32_t* srt_dst, const float* W3, int ldw, float* center, void* stream);

/* ---- greedy decode of the edge scores into contig walks -----------------------------
 * What inference.py:70-165 (greedy_forwards, greedy_backwards_rc, run_greedy_both_ways) and :29-36 (get_contig_length)
 * do with Python dicts and sets, for all sampled start edges of one iteration of get_contigs_greedy (:193-300) in one
 * launch, one wavefront per candidate.
 *   succ_ptr/succ_nbr/succ_eid  successor lists in EDGE-ID order (graph_parser.py:31-37) and the edge id of every slot
 *   logp        float[E]  log(sigmoid(score)) by edge id (inference.py:184); prefix_len int32[E]; read_len int32[N]
 *   visited     uint8[N]  nodes consumed by earlier contigs; cand_* the sampled edges (endpoints and edge id)
 *   walks_f[c,:len_f[c]]  forward walk from dst; walks_b[c,:len_b[c]] the walk from src^1 on the reverse-complement
 *   strand in walk order (the contig is reversed(walks_b ^ 1) followed by walks_f, inference.py:157, :254)
 *   sum_f/sum_b  fp32 sums of the chosen log-probabilities in walk order; contig_len[c] int64 as get_contig_length
 *   status[c]    0, or bit 0: a walk reached `capacity` and was cut, bit 1: an edge of the backward half has no mate
 *   exact ties for the best successor are resolved as torch.topk(k=1) resolves them on the CPU (decode.hip)
 * Node 2r+1 is the reverse complement of node 2r (x ^ 1, as in the reference); N even.
 */
int gnnome_greedy_walks_workspace_bytes(int64_t num_nodes, int num_candidates, size_t* bytes_host);
int gnnome_greedy_walks(const int32_t* succ_ptr, const int32_t* succ_nbr, const int32_t* succ_eid, const float* logp,
                        const int32_t* prefix_len, const int32_t* read_len, const uint8_t* visited, int64_t num_nodes,
                        const int32_t* cand_src, const int32_t* cand_dst, const int32_t* cand_eid, int num_candidates,
                        int32_t* walks_f, int32_t* walks_b, int64_t capacity, int32_t* len_f, int32_t* len_b, float* sum_f,
                        float* sum_b, int64_t* contig_len, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* The same launch with the reference's two decoder switches (inference.py:26-28); gnnome_greedy_walks is this entry with
 * stop_logp = -infinity, choice_mode = 0, and with those values the outputs are bit-identical to it.
 *   stop_logp    early_stopping / p_threshold (inference.py:98-100, :142-145): fp32(log(p_threshold)), or -infinity for off.  In
 *                the ranked branch only - a successor list of 2 or more with an admissible successor - a walk (either half) ends
 *                at its current node when EVERY admissible successor has logp < stop_logp.  The reference compares an fp32 tensor
 *                with a Python double, which torch rounds to fp32 first: the compare here is that fp32 compare, and a logp equal
 *                to stop_logp does not stop.  A single successor (:84-91) is taken however improbable.  Nothing is added to the
 *                sum at a stop; contig_len is computed as for any other end of walk; status is unchanged.
 *   choice_mode  0 = rank (torch.topk, as above); 1 = RANDOM (inference.py:102-104, :147-149): after the early-stopping test, the
 *                j-th of the n admissible successors in list order is taken and its own logp added.
 *   seed         DELIBERATE DIVERGENCE from the reference, which draws torch.randint from the CPU generator once per step and
 *                candidate after candidate - no wave can replay that stream.  Here j is a pure function of (seed, candidate index c,
 *                half, step): key = c << 32 | half << 31 | step (half 0 forward / 1 backward; step = the iteration of that half's
 *                walk loop, every iteration counted), u = mix64(seed + (key + 1) * 0x9E3779B97F4A7C15) with mix64 the finaliser of
 *                splitmix64 - the (key + 1)-th output of splitmix64 seeded with `seed`, the int64 taken as its 64 bits - and
 *                j = ((u >> 32) * n) >> 32.  The same seed gives the same walks whatever the scheduling.  Ignored in mode 0. */
int gnnome_greedy_walks_opts(const int32_t* succ_ptr, const int32_t* succ_nbr, const int32_t* succ_eid, const float* logp,
                             const int32_t* prefix_len, const int32_t* read_len, const uint8_t* visited, int64_t num_nodes,
                             const int32_t* cand_src, const int32_t* cand_dst, const int32_t* cand_eid, int num_candidates,
                             int32_t* walks_f, int32_t* walks_b, int64_t capacity, int32_t* len_f, int32_t* len_b, float* sum_f,
                             float* sum_b, int64_t* contig_len, int32_t* status, void* workspace, size_t workspace_bytes,
                             float stop_logp, int choice_mode, int64_t seed, void* stream);
/* The figures the reference prints for every candidate (inference.py:267-296) from one launch's outputs, in the doubles Python
 * computes them in.  table: double[7, P], rows src, dst, len_walk, len_contig, sumLogProb, meanLogProb, meanLogProb_scaled:
 * len_walk = len_f + len_b, 1 for a self-loop start edge (then every figure is 0); sumLogProb = (double)sum_f + (double)sum_b;
 * meanLogProb = sumLogProb / (len_walk - 2), 0 at len_walk 2; scaled = meanLogProb / sqrt(len_contig), 0 where len_contig <= 0. */
int gnnome_candidate_table(const int32_t* cand_src, const int32_t* cand_dst, const int32_t* len_f, const int32_t* len_b,
                           const float* sum_f, const float* sum_b, const int64_t* contig_len, int num_candidates, double* table,
                           void* stream);
/* visited[n] = visited[n^1] = 1 for every node of `walk` and for every node it jumped over: for consecutive (ss, dd),
 * succs[ss] & preds[dd] and their mates (inference.py:313-318, :334). */
int gnnome_mark_walk_visited(const int32_t* succ_ptr, const int32_t* succ_nbr, const int32_t* walk, int64_t walk_len,
                             uint8_t* visited, void* stream);

/* ---- overlap similarity -------------------------------------------------------------------------------
 * Replaces graph_parser.py:101-117 (calculate_similarities): for every edge
 *     edit_distance = edlib.align(read_seqs[src][-ol:], read_seqs[dst][:ol])['editDistance']     (edlib defaults: global / NW)
 *     overlap_similarity = 1 - edit_distance / ol        (0.5 where ol == 0)
 * with read_seqs[2r] = read r, read_seqs[2r+1] = its reverse complement (:365).  The distance is the exact Levenshtein
 * distance (Myers' bit-vector programme, one wavefront per overlap: csrc/overlap_similarity.hip).
 *   reads       uint8[total]   the reads as the S lines give them, concatenated (forward strand only)
 *   read_off    int64[R+1]     offsets of read r in `reads`
 *   symtab      uint8[512]     [b] = index of byte b in the caller's alphabet, [256+b] = index of complement(b)
 *                              (the table Bio.Seq.reverse_complement applies); num_symbols <= 32
 *   src, dst    int32[E]       node ids (graph.edges()); overlap_length int32[E].  An edge with an endpoint outside [0, 2 num_reads)
 *                              is reported as -1 and not aligned; symtab entries >= num_symbols are read as num_symbols - 1
 *   dist_out    int32[E]       edit distances; entries the kernels cannot serve keep the caller's fill value (fill with -1):
 *                              a query longer than 65 536 bases, or an alphabet whose match masks exceed LDS at that length
 *   similarity_out float32[E]  (NULL: skip) 1 - dist / ol evaluated in double precision like the reference's Python floats */
int gnnome_overlap_workspace_bytes(size_t* bytes_host);
int gnnome_overlap_edit_distance(const uint8_t* reads, const int64_t* read_off, int64_t num_reads, const uint8_t* symtab,
                                 int num_symbols, const int32_t* src, const int32_t* dst, const int32_t* overlap_length,
                                 int64_t num_edges, int32_t* dist_out, float* similarity_out, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* The same, for overlaps of any length (graph_parser.py:101-117 has no limit: edlib aligns what it is given).  gnnome_overlap_edit_distance_long
 * runs the passes of gnnome_overlap_edit_distance and then, before anything is reported as -1, a STRIP pass over what is left: a query
 * longer than 65 536 bases, or one whose match masks exceed LDS at its length, is cut into strips of B * 2048 rows (B = 32 up to 19
 * symbols, 16 up to 32), one wavefront runs the strips of an overlap one after another and hands the last row's horizontal deltas, one byte
 * per target column, from strip to strip through its slot of the workspace (csrc/overlap_similarity.hip, k_overlap_strips).  Cost per
 * overlap: ceil(m / (B * 2048)) strips of (n + 63) * B block steps each; exact like every other pass.
 *   max_columns  the largest target length min(overlap_length, len(read dst)) over the edges, >= 0: it sizes the carry slots.  An overlap
 *                whose target is longer than max_columns is not aligned by the strip pass (-1 unless an earlier pass settled it)
 *   workspace    gnnome_overlap_long_workspace_bytes(max_columns) bytes: the 16 ints of the short entry, padded to 128 bytes, then one slot
 *                of max_columns bytes (rounded up to 128) per strip wave, four per CU of the largest device.  A smaller workspace is accepted
 *                down to one slot; the strip pass then launches as many waves as there are whole slots
 *   workspace ints 0-11 as in the short entry (11: overlaps the banded pass settled), 12 the strip pass's ticket counter,
 *                13 the overlaps the strip pass settled (statistics only)
 * Everything else - arguments, the -1 report for endpoints out of range, similarity_out - as gnnome_overlap_edit_distance, whose own
 * behaviour and 16-int workspace are unchanged. */
int gnnome_overlap_long_workspace_bytes(int64_t max_columns, size_t* bytes_host);
int gnnome_overlap_edit_distance_long(const uint8_t* reads, const int64_t* read_off, int64_t num_reads, const uint8_t* symtab,
                                      int num_symbols, const int32_t* src, const int32_t* dst, const int32_t* overlap_length,
                                      int64_t num_edges, int64_t max_columns, int32_t* dist_out, float* similarity_out, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* ---- contig spelling: walks -> sequences and FASTA bodies ------------------------------------------------------------------------
 * Replaces utils/evaluate.py:38-48 (walk_to_sequence) and the byte layout of :51-53 (save_assembly: Biopython's FASTA writer,
 * 60 columns).  For step j of walk w, node u = walk_nodes[j], read r = u >> 1, len_u = read_off[r+1] - read_off[r]:
 *   not the walk's last node: p = prefix_length[edges[(u, walk_nodes[j+1])]] with the id as decode's succ_eid gives it (the last
 *       inserted id of a parallel pair), and the piece is reads[u][:p] under Python's slice rule: min(p, len_u) for p >= 0,
 *       max(len_u + p, 0) for p < 0 (pipeline.assemble masks p < 0 to 0 first, inference.py:463; the drop-in entry does not)
 *   the walk's last node: its whole read
 *   node 2r copies read r; node 2r+1 the first `piece` bytes of its reverse complement, i.e. read r read backwards from its end
 *   through Bio.Seq's IUPAC complement table in both letter cases, every other byte unchanged (graph_parser.py:183-184, :365)
 *   reads uint8[T], read_off int64[R+1]: the forward strand only (gnnome_amd/overlap.py pack_reads); num_nodes == 2 R
 *   walk_nodes int32[S], walk_off int64[W+1]: the walks concatenated
 * gnnome_contig_pieces: piece_len int64[S].  It first checks every walk and pair and SYNCHRONISES `stream` to report the first
 *   failure (an empty walk, offsets that do not rise from 0 to S, a node outside [0, num_nodes), a pair that is not an edge - the
 *   reference raises KeyError) as GNNOME_EINVAL naming the walk and the pair; nothing is written then.  Not capturable.
 *   "First" is the smallest item in this order: the W walks' offsets (item w: walk_off[w] < walk_off[w+1], walk_off[0] == 0,
 *   walk_off[W] == S), then the S steps in walk order (item W + j: the nodes in range, the pair an edge) - so any bad offset is
 *   reported before any bad step.  Offsets are only compared and nodes range-checked before use: nothing is read out of bounds.
 *   succ_nbr / succ_eid / prefix_length must be pointers even for a graph without edges (they are not read then).
 *   workspace: gnnome_contig_pieces_workspace_bytes.  num_walks == 0 is a no-op.
 * gnnome_contig_spell: piece_off int64[S+1] = the exclusive scan of piece_len (contig w holds unwrapped bytes
 *   [piece_off[walk_off[w]], piece_off[walk_off[w+1]]) ).  line_width == 0: out = the contigs concatenated in that layout.
 *   line_width > 0: contig w's FASTA body goes to out + body_off[w] (body_off int64[W], rising, bodies disjoint): '\n' after every
 *   line_width bytes and after a final partial line; bytes between bodies (where the caller puts header lines) are not written.
 *   An empty contig has a body of zero bytes in either layout (its FASTA record is the header line alone, as Biopython writes it),
 *   so body_off may repeat where bodies are empty.  Only bytes below out_bytes are written: a smaller out_bytes cuts the image there,
 *   mid-line or mid-body, and every byte from out + out_bytes on is left alone.  The copy is split into fixed tiles of the output, stores 16-byte vectors where out is
 *   16-byte aligned, and uses no atomics: equal inputs give equal bytes.  walk_off / piece_off as gnnome_contig_pieces checked and
 *   produced them. */
int gnnome_contig_pieces_workspace_bytes(int64_t num_walks, int64_t num_steps, size_t* bytes_host);
int gnnome_contig_pieces(const int32_t* walk_nodes, int64_t num_steps, const int64_t* walk_off, int64_t num_walks, const int32_t* succ_ptr,
                         const int32_t* succ_nbr, const int32_t* succ_eid, const int32_t* prefix_length, int64_t num_nodes,
                         const int64_t* read_off, int64_t num_reads, int64_t* piece_len, void* workspace, size_t workspace_bytes,
                         void* stream);
int gnnome_contig_spell(const int32_t* walk_nodes, int64_t num_steps, const int64_t* walk_off, int64_t num_walks, const int64_t* piece_off,
                        const uint8_t* reads, const int64_t* read_off, int64_t num_reads, const int64_t* body_off, int line_width,
                        uint8_t* out, int64_t out_bytes, void* stream);

/* ---- ground-truth edge labels from read positions --------------------------------------------------------------------------------
 * Replaces utils/labels.py (process_graph / process_graph_combo: create_correct_graphs[_combo] + get_gt_for_single_strand), which
 * graph_parser.py:387-400 runs on the networkx graph when training=True.  Per node: read_strand int32[N] in {-1, +1}, read_start /
 * read_end int64[N], read_chr int32[N] the raw chromosome code (X = -1, Y = -2, M = -3); the entry groups by chromosome itself.
 *   An edge (u, v) is a class edge of problem (c, s) when chr[u] == chr[v] == c, strand[u] == strand[v] == s and start[u] < start[v]
 *   < end[u] (s = +1) or start[v] < start[u] < end[v] (s = -1).  Per problem, over its class edges and their endpoints V:
 *     s = +1: final = argmax_V end, reached = argmin_V end; while nodes are alive: a = argmin_alive start, F = reachable from a in
 *       G[alive], h = argmax_F end, C = the nodes that reach h in G[F]; if |C| >= 2 and not end[h] < end[reached]: reached = h, the
 *       class edges inside C are labelled 1, stop if h == final; alive -= F.
 *     s = -1: final = argmin_V start, reached = argmax_V start, a = argmax_alive end, h = argmin_F start, reject when start[h] >
 *       start[reached].
 *   Every argmin / argmax takes the SMALLEST NODE ID among equal keys (the reference takes a networkx view's or a Python set's order).
 *   y float32[E] in edge-id order: 1.0 for the labelled edges, 0.0 for every other; all of y is written.  A problem with no class edges
 *   contributes nothing (the reference raises ValueError there).
 *   stats: NULL, or int64[1 + 8 * stats_rows]: stats[0] = P, the number of problems; row p < stats_rows (problems by chromosome code
 *   ascending, strand -1 before +1) at stats + 1 + 8 p = {chr, strand, nodes |V|, class edges, passes, accepted components, forward
 *   queue pops, backward queue pops}.
 *   N and E below 2^31.  The entry checks node ids in [0, N) and strands in {-1, +1} in a first pass and SYNCHRONISES `stream` to
 *   report the first failure as GNNOME_EINVAL (y is not written then); not capturable.  The loop is one wavefront per problem (one
 *   launch; problems share nothing); y is a function of the inputs alone.  workspace: gnnome_edge_labels_workspace_bytes. */
int gnnome_edge_labels_workspace_bytes(int64_t num_nodes, int64_t num_edges, size_t* bytes_host);
int gnnome_edge_labels(const int32_t* src, const int32_t* dst, int64_t num_edges, int64_t num_nodes, const int32_t* read_strand,
                       const int64_t* read_start, const int64_t* read_end, const int32_t* read_chr, float* y, int64_t* stats,
                       int64_t stats_rows, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Every cluster's model inputs at once (mini-batch training) -------------------------------------------------------------
 * train.py:125-135 (get_partition_ne_features, both orientations) and the gathers of train.py:148-186 (get_bce_loss_partition,
 * get_symmetry_loss_partition: e[sub_g.edata['_ID']], y[sub_g.edata['_ID']]) for all k clusters of a graph in one call.
 * Packed layout: cluster c owns node positions [node_ptr[c], node_ptr[c+1]) of nid and edge positions [edge_ptr[c], edge_ptr[c+1])
 * of eid (int64 each; node_ptr[0] = edge_ptr[0] = 0, node_ptr[k] = total_nodes, edge_ptr[k] = total_edges).  outer_nid / outer_eid
 * (NULL: none) compose one more id map - cluster -> masked graph -> full graph: position p stands for node outer_nid[nid[p]] of the
 * full graph (outer_nodes entries; nid indexes it) - so a masked graph's clusters need no intermediate gather.
 * in_deg / out_deg float32[num_nodes]: the FULL graph's stored degrees; e float32[num_edges,2]; y float32[num_edges] (NULL with y_sub).
 * Outputs, packed the same way: x_org float32[total_nodes,2] = [z(in) | z(out)], x_rev (NULL: skip) = [z(out) | z(in)],
 * e_sub float32[total_edges,2], y_sub float32[total_edges]; z = (d - mean) / std over the cluster's own nodes in fp32, mean and
 * UNBIASED std from fixed-order fp64 sums (no float atomics; the bits do not depend on the launch), rounded to fp32 as torch's CPU
 * statistics are.  A one-node cluster (std NaN) and a cluster of equal degrees (std 0) give torch's NaN / inf: nothing is clamped.
 * Any mix of cluster sizes, from one cluster of the whole graph to many of a few nodes.  The entry checks both ptrs and every id in a
 * first pass and SYNCHRONISES `stream` once: the first failure is GNNOME_EINVAL naming the cluster, and no output is written then;
 * not capturable.  workspace: gnnome_cluster_inputs_workspace_bytes(k, total_nodes). */
int gnnome_cluster_inputs_workspace_bytes(int64_t num_clusters, int64_t total_nodes, size_t* bytes_host);
int gnnome_cluster_inputs_f32(const int64_t* node_ptr, const int64_t* nid, int64_t num_clusters, int64_t total_nodes,
                              const int64_t* edge_ptr, const int64_t* eid, int64_t total_edges, const int64_t* outer_nid,
                              int64_t outer_nodes, const int64_t* outer_eid, int64_t outer_edges, const float* in_deg,
                              const float* out_deg, int64_t num_nodes, const float* e, const float* y, int64_t num_edges,
                              float* x_org, float* x_rev, float* e_sub, float* y_sub, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---- Node order (round 4): locality for inputs whose node ids do not follow the layout ---------------------------------------
 * The reference numbers nodes in S-line order of the GFA (graph_parser.py:174-181: read r -> nodes 2r, 2r+1), which need not be
 * the order of the reads along the genome; gnnome_amd/node_order.py renumbers the READS once per graph so that the
 * destination-range partition (gnnome_amd/dist.py) cuts few edges and gathers hit L2.  Logits stay in edge-id order: nothing
 * the reference's callers see changes.  Two kernels; sorting, compaction and the final numbering are torch operators.
 *
 * gnnome_adjacency_support: for every entry p of a CSR adjacency with SORTED rows (row_of[p] = its row), supported[p] = 1 iff
 *   the two endpoints have a common neighbour (an overlap graph is locally transitive; repeat-induced edges are not).
 * gnnome_bfs_levels: breadth-first levels of every component, one workgroup for the whole graph (the frontier of an overlap graph
 *   is dozens of reads wide and tens of thousands of levels deep).  level_key[v] int32[num_nodes] = a counter that grows by one
 *   per level and does not restart between components (-1: never reached - no neighbours); seeds / num_seeds (device, NULL: the
 *   smallest unvisited id that has a neighbour starts the next component); far_node[c] = the smallest id in the last level of
 *   component c; *num_components (device).  frontier_workspace: int32[2 * num_nodes].  Levels and far nodes are functions of the
 *   graph alone. */
int gnnome_adjacency_support(const int32_t* ptr, const int32_t* adj, const int32_t* row_of, int64_t num_rows, int64_t nnz,
                             uint8_t* supported, void* stream);
int gnnome_bfs_levels(const int32_t* ptr, const int32_t* adj, int64_t num_nodes, const int32_t* seeds, const int32_t* num_seeds,
                      int32_t* level_key, int32_t* frontier_workspace, int32_t* far_node, int32_t* num_components, void* stream);

/* ---- bf16 STORAGE of two training activations (activation_storage = "bf16", BASELINE configs[2]) ------------------------------
 * The reference trains in fp32 throughout; as an OPTION the pre-normalisation gate output xe[E,H] (written once, read three
 * times per layer) and its gradient dxe[E,H] (written once, read twice) can live in HBM as bfloat16 - rounded to nearest even
 * when written, widened exactly when read; every sum, product and statistic is still fp32, and the residual streams e, e', de,
 * h stay fp32 (|e| reaches several hundred with per-layer updates of order one: bf16 there would drop the updates).  Each entry
 * is its _f32 namesake with the marked tensor as uint16_t (bf16 bits), contiguous, 8-byte aligned:
 *   raw_stats: x_out (the statistics are those of the ROUNDED values; hidden = 64 / 128: gnnome_set_tuning key 0 = 0 or 8 only, see
 *   gnnome_edge_gate_raw_stats_rows);  bn_relu_res: x;  agg_edge_bwd_stats, agg_bwd_fused: xe;
 *   bn_bwd_dgrad: X and dxe (C += dxe W^T uses the unrounded dxe);  segment_sum2: X;  wgrad: A (lda in elements). */
int gnnome_edge_gate_raw_stats_x16(const float* e_in, uint16_t* x_out, int64_t num_edges, int hidden, const float* B1h, const float* B2h,
                                   int ld_node, const int32_t* srt_src, const int32_t* srt_dst, const float* W3, int ldw,
                                   const float* center, float* stats_partial, void* stream);
/* gnnome_edge_gate_bn_f32 with x_out stored as bf16; e_out is computed from the ROUNDED rows (what gnnome_bn_relu_res_x16 reads back). */
int gnnome_edge_gate_bn_x16(const float* e_in, float* e_out, uint16_t* x_out, int64_t num_edges, int hidden, const float* B1h,
                            const float* B2h, int ld_node, const int32_t* srt_src, const int32_t* srt_dst, const float* W3, int ldw,
                            const float* scale, const float* shift, void* stream);
int gnnome_bn_relu_res_x16(const uint16_t* x, const float* scale, const float* shift, const float* res, int64_t rows, int hidden,
                           float* out, void* stream);
int gnnome_agg_edge_bwd_stats_x16(const float* e, int64_t num_edges, int hidden, const float* Tf, const float* Uf, const float* Tb,
                                  const float* Ub, const float* A2h, const float* A3h, int ld_node, const int32_t* srt_src,
                                  const int32_t* srt_dst, float* de, const uint16_t* xe, const float* scale, const float* shift,
                                  const float* mean, float* s1, float* s2, void* workspace, size_t workspace_bytes, void* stream);
int gnnome_agg_bwd_fused_x16(const float* e, int64_t num_nodes, int64_t num_edges, int hidden, const float* Tf, const float* Uf,
                             const float* Tb, const float* Ub, const float* A2h, const float* A3h, int ld_node, const int32_t* in_ptr,
                             const int32_t* srt_src, const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, float* de,
                             const uint16_t* xe, const float* scale, const float* shift, const float* mean, float* sum_in, float* sum_out,
                             float* s1, float* s2, unsigned* amax_bits, void* workspace, size_t workspace_bytes, void* stream);
int gnnome_bn_bwd_dgrad_x16(float* C, const uint16_t* X, int64_t rows, int64_t rows_once, int hidden, const float* scale, const float* shift, const float* a,
                            const float* c1, const float* c2, const float* mean, const float* rstd, const float* W, int ldw,
                            uint16_t* dxe, void* stream);
/* hidden = 256 (round 4): the out-of-place form, gnnome_bn_bwd_dgrad_out_f32 with X and dxe as bf16; gnnome_edge_gate_raw_stats_x16 and
 * gnnome_wgrad_x16 take hidden / Ka = 256 as well (the raw gate on the fp16x3 kernel: not under gnnome_set_tuning(10, 1)). */
int gnnome_bn_bwd_dgrad_out_x16(const float* C_in, float* C_out, const uint16_t* X, int64_t rows, int64_t rows_once, int hidden,
                                const float* scale, const float* shift, const float* a, const float* c1, const float* c2,
                                const float* mean, const float* rstd, const float* W, int ldw, uint16_t* dxe, void* stream);
int gnnome_segment_sum2_x16(const uint16_t* X, int width, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_pos,
                            int64_t num_nodes, float* out_in, int ld_in, float* out_out, int ld_out, void* stream);
int gnnome_wgrad_x16(const uint16_t* A, int lda, int Ka, const float* B, int ldb, int Kb, int64_t rows, float* C, int ldc,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- clusters for mini-batch training (round 5) ----------------------------------------------
 * train.py:333-346 calls dgl.metis_partition(g.long(), num_clusters, extra_cached_hops=1): METIS 5.1.0's multilevel k-way partitioner
 * behind DGL 0.8.1 (requirements.txt:23; neither is in the reference checkout).  gnnome_amd/partition.py runs the published scheme
 * (Karypis & Kumar 1998: heavy-edge matching, a greedy-growing initial partition of the coarsest graph, greedy k-way boundary refinement
 * while uncoarsening) on the device; these are its two inner loops over an undirected weighted CSR (ptr int32[n+1], adj / wgt int32[nnz],
 * both directions stored, no self loops needed), deterministic and atomic-free:
 *   gnnome_hem_propose: proposal[v] = the heaviest unmatched neighbour u of an unmatched v (match[.] < 0) with vwgt[v] + vwgt[u] <=
 *     max_vwgt, ties to the lighter vertex, then the smaller id; -1 if none.  The caller pairs mutual proposals (handshake).
 *   gnnome_kway_gains: best_part[v] = the part, other than label[v], that v's neighbours connect it to most heavily (ties: smaller id;
 *     -1 for an interior vertex) and gain[v] = that connectivity - the connectivity to its own part. */
int gnnome_hem_propose(const int32_t* ptr, const int32_t* adj, const int32_t* wgt, const int32_t* vwgt, const int32_t* match,
                       int64_t num_vertices, int max_vwgt, int32_t* proposal, void* stream);
int gnnome_kway_gains(const int32_t* ptr, const int32_t* adj, const int32_t* wgt, const int32_t* label, int64_t num_vertices,
                      int32_t* best_part, int32_t* gain, void* stream);
/* The coarsest level's initial partition (METIS's greedy graph growing), on the HOST: all pointers are host memory, nothing is launched.
 * k - 1 regions grown one after the other from the free vertex with the smallest id, always taking the free vertex most heavily connected to the
 * region (ties: the one that became its neighbour first), until the region holds (remaining weight) / (remaining parts); the rest is the last
 * part.  label_host[v] in [0, num_parts).  (train.py:333: dgl.metis_partition -> METIS 5.1.0 InitKWayPartitioning; see csrc/partition.hip.) */
int gnnome_greedy_growing_host(const int32_t* ptr_host, const int32_t* adj_host, const int32_t* wgt_host, const int32_t* vwgt_host,
                               int64_t num_vertices, int num_parts, int32_t* label_host);

/* ---- GFA ingestion: parse, resolve names, pack the reads ----------------------------------------------------------------------------
 * Replaces the line loop of graph_parser.py:159-340 (only_from_gfa) as gnnome_amd/gfa.py read_gfa states it; the file's bytes are on the
 * device (buf uint8[num_bytes]).  Whitespace is str.split()'s in ASCII (0x09-0x0d, 0x1c-0x20); a line ends at '\n'.  Compaction of the
 * marks, the scans and the sorts between these entries are torch operators (gnnome_amd/gfa.py read_gfa_device).  Nothing here produces a
 * float; no float atomics.
 * gnnome_gfa_tile_sizes: bytes per workgroup of gnnome_gfa_mark and output bytes per workgroup of gnnome_gfa_pack (host, no launch).
 * gnnome_gfa_mark (graph_parser.py:160, :167: strip().split() of every line, elementwise): marks uint8[num_bytes], bit 0 = first byte of a
 *   field, bit 1 = last byte of a field, bit 2 = first byte of a line (also of an empty one).  bad_pos int64[2], preset to INT64_MAX by the
 *   caller: lowered (atomicMin) to the first byte >= 0x80 and to the first '\r' that no '\n' follows.
 * gnnome_gfa_classify (:167-208 S and A lines, :276-300 L lines): one thread per line.  field_start / field_end int64[num_fields] = the
 *   positions of bits 0 / 1 in rising order; line_field int64[num_lines+1] = the index of the first field at or after every line start,
 *   line_field[num_lines] = num_fields.  kind int32[L]: 0 other or blank, 1 S, 2 L, 3 A.  rec int64[L,8], byte ranges as [begin, end):
 *     S: name, sequence (field 3), LN = int(field4[5:]), bit 0 the sequence is "*" | bit 1 the name starts with "utg", -, -
 *     L: name 1, name 2 (after every SI:f: field is dropped when one stands at index >= 6, and, with 7 fields left, without the hifiasm
 *        suffix: everything from the LAST ":<digit>-" on), overlap = int(cigar[:-1]), orientation case 0 "++" 1 "+-" 2 "-+" 3 anything
 *        else, begin and length of the first SI:f: value (-1, -1 without one)
 *     A: field 5 (the read), field 4 (its orientation); -1 with fewer than 5 fields
 *   err int32[L]: 0, or why the line cannot be served: 1 S line with < 4 fields, 2 LN not 1-18 plain digits, 3 L line without 6, 7 or 8
 *   fields, 4 a 7-field name without a suffix, 5 overlap not 1-18 plain digits, 6 a tag value above 31 bytes, 7 a tag value that is not
 *   plain decimal text (6 and 7 only where the overlap is not zero), 14 descriptors that gnnome_gfa_mark did not produce.
 *   first_bad int32[1], preset to INT32_MAX: lowered to the smallest line with a code, by this entry and the next two.
 * gnnome_gfa_names_insert (:174-175 read_to_node): seg_rec int64[R,8] / seg_line int64[R] = rec and line number of the S lines in file
 *   order; table int32[capacity] preset to -1, capacity a power of two above R.  Linear probing; a slot is claimed with a 32-bit
 *   compare-and-swap and every probe compares length and bytes, so hash collisions cost probes and change no answer.  A slot ends up with
 *   the SMALLEST S index of its name; every later S line of that name gets code 9 (15: no free slot).  Independent of arrival order.
 * gnnome_gfa_links (:302-321): link_rec / link_line of the L lines; for link m without a code and with overlap != 0, both names are looked
 *   up (code 10: unknown, 11: defined on a later line) and event_u / event_v int64[2M] receive (sr, dr) at 2m and (sv, dv) at 2m+1;
 *   -1 where the link contributes nothing.
 * gnnome_gfa_pack (:183-184, and overlap.pack_reads): out[out_off[r] : out_off[r+1]] = src[src_beg[r] : ...] for r < num_items, out_off
 *   int64[num_items+1] rising from 0 to out_bytes (a scan of the lengths; a keep mask enters as zero lengths).  Fixed tiles of the
 *   OUTPUT, a binary search for the tile's first item, 16-byte stores where aligned; reads outside src are skipped, not made. */
int gnnome_gfa_tile_sizes(int* tokenise_tile_host, int* pack_tile_host);
int gnnome_gfa_mark(const uint8_t* buf, int64_t num_bytes, uint8_t* marks, int64_t* bad_pos, void* stream);
int gnnome_gfa_classify(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end, int64_t num_fields,
                        const int64_t* line_field, int64_t num_lines, int32_t* kind, int64_t* rec, int32_t* err, int32_t* first_bad,
                        void* stream);
int gnnome_gfa_names_insert(const uint8_t* buf, int64_t num_bytes, const int64_t* seg_rec, const int64_t* seg_line, int64_t num_segments,
                            int32_t* table, int64_t capacity, int32_t* err, int64_t num_lines, int32_t* first_bad, void* stream);
int gnnome_gfa_links(const uint8_t* buf, int64_t num_bytes, const int64_t* link_rec, const int64_t* link_line, int64_t num_links,
                     const int64_t* seg_rec, const int64_t* seg_line, int64_t num_segments, const int32_t* table, int64_t capacity,
                     int32_t* err, int64_t num_lines, int32_t* first_bad, int64_t* event_u, int64_t* event_v, void* stream);
int gnnome_gfa_pack(const uint8_t* src, int64_t src_bytes, const int64_t* src_beg, const int64_t* out_off, int64_t num_items, uint8_t* out,
                    int64_t out_bytes, void* stream);

/* ---- FASTA / FASTQ reads files: records, wanted ids, sequences, positions ------------------------------------------------------------
 * Replaces the per-record loops of graph_parser.py:121-136 (the titles of the reads file), :213-272 (strand, start, end and chromosome
 * from those titles, per node) and :341-366 (the sequences of a GFA whose S lines say '*'), as gnnome_amd/contigs.py _records /
 * read_sequences / read_titles and gnnome_amd/gfa.py _annotation state them.  The file's bytes are on the device (buf uint8[num_bytes],
 * .gz decompressed on the host) and are tokenised by gnnome_gfa_mark unchanged; field_start / field_end / line_field are what
 * gnnome_gfa_classify takes, line_start int64[num_lines] the positions of mark bit 2.  Compactions, scans, sorts and the unitig
 * combination are torch operators (gnnome_amd/reads.py); the bases are copied by gnnome_gfa_pack, one item per sequence line.  Nothing
 * here produces a float; no float atomics.  err int32[num_lines] preset to 0 and first_bad int32[1] preset to INT32_MAX are shared by
 * the entries: a line this path does not serve gets a code (1 a sequence or quality line with more than one field, 2 a FASTQ record
 * that is not in the four-line form, 3 a number of more than 18 digits in a title, 4 a chr= value that mixes digits and letters) and
 * first_bad is lowered (atomicMin) to the smallest such line.
 * gnnome_reads_records_fasta: one thread per line.  kind int32[L]: 0 blank, 1 header (the line's first BYTE is '>'), 2 any other
 *   line with a field.  rec int64[L,4], byte ranges as [begin, end): header: id (the first whitespace-separated token of line[1:], empty
 *   when nothing follows the marker), title (line[1:].rstrip()); other: its first field, -, -.  first_header int64[1] on the device: the
 *   line of the first header (num_lines without one); a line of kind 2 with more than one field gets code 1 only below it.
 * gnnome_reads_records_fastq: one thread per record over nonblank int64[num_nonblank], the lines with a field, in file order; record k
 *   is lines 4k..4k+3 of them and must be: first byte '@'; first byte not '+', one field; first byte '+'; one field as long as the
 *   sequence.  rec int64[ceil(num_nonblank / 4), 6]: id, title, sequence; all 0 for a record that breaks the form, whose first
 *   offending line gets code 2 (1 for the field count); a trailing group of fewer than 4 lines gets code 2 at its first line.
 * gnnome_reads_names_insert: names uint8[names_bytes] = the wanted names one after the other, name r = names[name_off[r] : name_off[r+1]],
 *   name_off int64[R+1]; table int32[capacity] preset to -1, capacity a power of two (>= 2).  Linear probing, 32-bit compare-and-swap,
 *   every probe compares length and bytes.  Names with equal bytes share a slot (two nodes may name one read).  slot_of int32[R]: the
 *   slot of every name, -1 when the table had no room, in which case full int32[1] (preset to 0) becomes 1.
 * gnnome_reads_match: record k's id = buf[rec[k*rec_stride] : rec[k*rec_stride+1]) is looked up; where a wanted name has its bytes,
 *   match[slot] (int32[capacity], preset to -1) is raised to k with an integer atomicMax: a repeated id keeps its last record.
 * gnnome_reads_annotations: one thread per entry of which int64[num_which] (a record index, or -1: no record).  The title
 *   buf[rec[k*rec_stride+2] : rec[k*rec_stride+3]) is searched for the first match of strand=(\+|\-), start=(\d+), end=(\d+) and
 *   chr=([0-9XYM]+) as re.search finds them (substring matches; an occurrence the pattern does not match is passed over).  ann
 *   int64[num_which,4] = +1 / -1, start, end, chromosome (X, Y, M: -1, -2, -3); missing int32[num_which]: bit 0 strand, 1 start, 2 end,
 *   3 chr has no match (15 for which = -1).  Codes 3 and 4 go to line rec_line[k] (int64[num_records], the record's header line). */
int gnnome_reads_records_fasta(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end,
                               int64_t num_fields, const int64_t* line_field, const int64_t* line_start, int64_t num_lines,
                               const int64_t* first_header, int32_t* kind, int64_t* rec, int32_t* err, int32_t* first_bad, void* stream);
int gnnome_reads_records_fastq(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end,
                               int64_t num_fields, const int64_t* line_field, const int64_t* line_start, int64_t num_lines,
                               const int64_t* nonblank, int64_t num_nonblank, int64_t* rec, int32_t* err, int32_t* first_bad, void* stream);
int gnnome_reads_names_insert(const uint8_t* names, int64_t names_bytes, const int64_t* name_off, int64_t num_names, int32_t* table,
                              int64_t capacity, int32_t* slot_of, int32_t* full, void* stream);
int gnnome_reads_match(const uint8_t* buf, int64_t num_bytes, const int64_t* rec, int rec_stride, int64_t num_records,
                       const uint8_t* names, int64_t names_bytes, const int64_t* name_off, int64_t num_names, const int32_t* table,
                       int64_t capacity, int32_t* match, void* stream);
int gnnome_reads_annotations(const uint8_t* buf, int64_t num_bytes, const int64_t* rec, int rec_stride, int64_t num_records,
                             const int64_t* rec_line, const int64_t* which, int64_t num_which, int64_t* ann, int32_t* missing, int32_t* err,
                             int64_t num_lines, int32_t* first_bad, void* stream);

/* ---- pbsim3 MAF files: the read positions of the training labels -----------------------------------------------------------------------
 * Replaces the Biopython AlignIO loop of generate_data.py:43-60 (change_description_pbsim: start and size of the reference line of every
 * alignment block, the strand of its read line), as gnnome_amd/maf.py states it.  The file's bytes are on the device and are tokenised by
 * gnnome_gfa_mark unchanged; field_start / field_end / line_field are what gnnome_gfa_classify takes.  Grouping the s lines under the
 * nearest a line, "exactly two" and "equal text lengths" are torch scans (gnnome_amd/maf.py); the wanted names go through
 * gnnome_reads_names_insert / gnnome_reads_match with the block records (rec_stride 8).  err int32[num_lines] preset to 0 and first_bad
 * int32[1] preset to INT32_MAX as for the reads entries; the codes: 1 an s line without exactly 7 fields, 2 a start, size or srcSize that
 * is not plain digits, 3 one of more than 18 digits, 4 a strand other than + or -, 5 a line that is neither blank, a comment, a track
 * line, an a line nor an s line, 9 a text whose bytes other than '-' are not `size` many (6-8 are set by the torch scans).
 * gnnome_maf_lines (generate_data.py:43-60, the fields AlignIO reads from an s line): one thread per line.  kind int32[L]: 0 blank,
 *   1 comment (first field begins with '#', or is "track"), 2 a (first field "a"), 3 s (first field "s"), 4 other.  rec int64[L,8], for
 *   an s line without a code: name begin, name end, start, size, strand (+1 / -1), text begin, text end, 1; all 0 otherwise.
 * gnnome_maf_text_check (generate_data.py:43-60, the size the reference trusts instead of len(seq)): one wavefront per record of rec
 *   int64[num_records,8] (the s lines' records, compacted; rec_line int64[num_records] their lines).  A record whose last word is 1 and
 *   whose text range lies inside [0, num_bytes) has the bytes of its text that are not '-' counted (16-byte loads where aligned, byte
 *   loads at the ragged ends, a wave reduction); a count other than `size` gives its line code 9. */
int gnnome_maf_lines(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end, int64_t num_fields,
                     const int64_t* line_field, int64_t num_lines, int32_t* kind, int64_t* rec, int32_t* err, int32_t* first_bad,
                     void* stream);
int gnnome_maf_text_check(const uint8_t* buf, int64_t num_bytes, const int64_t* rec, const int64_t* rec_line, int64_t num_records,
                          int32_t* err, int64_t num_lines, int32_t* first_bad, void* stream);

/* ---- Precision-recall curve and average precision of the edge scores -----------------------------------------------------------------
 * Replaces the scikit-learn calls of utils/metrics.py:51-80 (precision_recall_curve, average_precision_score) for either class, as
 * gnnome_amd/metrics.py states them.  With v the score of an edge and `positive` its class bit: sort by v descending; idx = the last
 * position of every run of equal v; tp[j] = positives at positions <= idx[j], fp[j] = 1 + idx[j] - tp[j], thresholds[j] = v at idx[j].
 * The sort between the first two entries is the caller's (torch.sort, descending, of the keys as int32).  Every count is an exact
 * integer scan in three launches (per-tile sums, ONE workgroup over the tile sums, per-tile downsweep): no kernel waits on another
 * workgroup, the tiles are fixed, and the only atomics are integer minima of the check words.  1 <= num_edges < 2^31.
 * The workspace is shared by the four entries of one curve and must not be touched between them.
 * gnnome_pr_curve_tile_size: sorted positions per tile of the scan and terms per tile of the AP sum (host, no launch).
 * gnnome_pr_curve_keys (utils/metrics.py:52, :59-60, :68, :76-77): p = preds (apply_sigmoid = 0) or 1 / (1 + expf(-preds)) in float32
 *   (apply_sigmoid = 1), also written to probs_out when that is not NULL; v = p, positive = (label == 1), or with inverse != 0
 *   v = 1.0f - p in float32, positive = (label == 0); keys uint32[E] = (bits(v) << 1) | positive (v in [0, 1]: 30 bits, monotone in
 *   v).  The check words are preset here: the smallest edge id with p NaN or outside [0, 1], and with a label other than 0 or 1.
 * gnnome_pr_curve_scan (utils/metrics.py:54, :62, :70, :79): sorted_keys uint32[E] descending.  SYNCHRONISES `stream` once and fills
 *   result_host int64[4] (HOST memory): the number of thresholds M, the number of positives P, the two check words (-1: none).
 * gnnome_pr_curve_emit (utils/metrics.py:54-55, :62-63): any output may be NULL.  thresholds float32[M], tp, fp int64[M] at j (descending
 *   threshold); precision, recall float64[M+1] in scikit-learn's order: (double)tp / (double)(tp + fp) and (double)tp / (double)P at
 *   M-1-j, and (1, 0) at M; last int64[1] = the first j with tp[j] = P, where scikit-learn 0.24.2 cuts the curve (it keeps j = last..0).
 *   num_thresholds and num_positives are what gnnome_pr_curve_scan returned (P >= 1).
 * gnnome_pr_curve_ap (utils/metrics.py:70, :79): ap float64[1] = max(0, -sum over r < M of (recall[r+1] - recall[r]) * precision[r]),
 *   each term one IEEE subtraction and one IEEE multiplication (no fma), summed per tile and then over the tiles in fixed trees. */
int gnnome_pr_curve_tile_size(int* tile_host);
int gnnome_pr_curve_workspace_bytes(int64_t num_edges, size_t* bytes_host);
int gnnome_pr_curve_keys(const float* preds, const float* labels, int64_t num_edges, int apply_sigmoid, int inverse, uint32_t* keys,
                         float* probs_out, void* workspace, size_t workspace_bytes, void* stream);
int gnnome_pr_curve_scan(const uint32_t* sorted_keys, int64_t num_edges, void* workspace, size_t workspace_bytes, int64_t* result_host,
                         void* stream);
int gnnome_pr_curve_emit(const uint32_t* sorted_keys, int64_t num_edges, int64_t num_thresholds, int64_t num_positives, float* thresholds,
                         int64_t* tp, int64_t* fp, double* precision, double* recall, int64_t* last, void* workspace,
                         size_t workspace_bytes, void* stream);
int gnnome_pr_curve_ap(const double* precision, const double* recall, int64_t num_thresholds, double* ap, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- Walk audit: the strand, chromosome and overlap checks of decoded walks ---------------------------------------------------------
 * Replaces utils/analyze.py:1-38 (assert_strand, assert_chromosome, assert_overlap, each a Python loop with .item() round trips per
 * step) for a whole batch of walks, as tests/walk_audit_statement.py states them.  Walks are flattened: walk w is
 * walk_nodes[walk_ptr[w] .. walk_ptr[w+1]) (int32, walk_ptr[W+1] ascending from 0 to T), and walk_id int32[T] names the walk of every
 * position (the caller's repeat_interleave of the walk lengths).  read_strand, read_start, read_end, read_chr: int64[num_nodes].
 * One thread per position t of walk w, with first = walk_nodes[walk_ptr[w]]; flags uint8[T]:
 *   bit 0  (:1-8)    t is not the walk's first position and read_strand[node] != read_strand[first]
 *   bit 1  (:11-18)  t is not the walk's first position and read_chr[node] != read_chr[first]
 *   bit 2  (:21-38)  t is not the walk's last position and, with d = walk_nodes[t+1], both strands are 1 and read_start[d] >
 *                    read_end[node], or both are -1 and read_end[d] < read_start[node]  (equality, unequal strands and strand values
 *                    other than 1 / -1 are silent; the chromosome is not looked at)
 *   bit 6  walk_id[t] outside [0, W) or t outside [walk_ptr[w], walk_ptr[w+1]) within [0, T): the position is not examined
 *   bit 7  the node id is outside [0, num_nodes): it is never used as an index, and no other bit of the position is set
 * The reference's printed `walk index` is t - walk_ptr[w] - 1 for bits 0 and 1 (it enumerates walk[1:]) and t - walk_ptr[w] for bit 2.
 * counts int32[W,3]: zeroed here, then the number of positions of walk w with bit 0, bit 1, bit 2 - summed per wavefront run of equal
 * walk_id and added with integer atomics (exact, order-free).  num_walks, num_positions < 2^31; either being 0 returns 0 without a
 * launch and without writing anything. */
int gnnome_walk_audit(const int32_t* walk_ptr, const int32_t* walk_nodes, const int32_t* walk_id, int64_t num_walks, int64_t num_positions,
                      const int64_t* read_strand, const int64_t* read_start, const int64_t* read_end, const int64_t* read_chr,
                      int64_t num_nodes, uint8_t* flags, int32_t* counts, void* stream);

/* ---- Interval union: the islands of reference that the reads cover, per group -------------------------------------------------------
 * Replaces utils/labels.py:5-20 (interval_union: a sort and a Python loop over every strand +1 read), as tests/interval_statement.py
 * states it, with groups added: start, end int64[M] and group int32[M] are ordered by (group, start) - the caller's stable torch sorts;
 * equal group values must be adjacent, their order is the caller's.  Walking a group in that order with R = the largest end seen so
 * far in the group, interval i heads a new island iff it is the group's first or start[i] > R (start[i] == R touches and merges); the
 * island is [start of its head, R at its last member].  For intervals with end >= start - which the caller checks - that R is the
 * largest end of the island's own members, the reference's result; one group of all intervals is the reference's single line.
 * Two exact segmented scans over tiles of a fixed number of intervals (running maximum; island, group and length counts), each as a
 * per-tile reduce, ONE workgroup over the tile summaries and a per-tile apply, five launches: no kernel waits on another workgroup, no
 * atomics, no floating point, one writer per output slot.
 * gnnome_interval_union_tile_size: intervals per tile (host, no launch); results do not depend on it.
 * gnnome_interval_union_workspace_bytes: 0 <= num_intervals < 2^31.
 * gnnome_interval_union: head uint8[M] (may be NULL): 1 where an island starts.  isl_group int32, isl_start, isl_end int64, each with
 *   room for M entries: island k in input order, the first K are written.  grp_code int32, grp_covered, grp_count int64, each
 *   [max_groups]: per group in input order its value of `group`, the sum of (end - start) over its islands (64-bit wrap-around sums:
 *   exact when the figure fits) and the number of its islands.  SYNCHRONISES `stream` once and fills result_host int64[2] (HOST
 *   memory): K and the number of groups G.  G > max_groups is an error reported after the fact; only the first max_groups groups
 *   were written.  M = 0 gives K = G = 0 without a launch. */
int gnnome_interval_union_tile_size(int* tile_host);
int gnnome_interval_union_workspace_bytes(int64_t num_intervals, size_t* bytes_host);
int gnnome_interval_union(const int64_t* start, const int64_t* end, const int32_t* group, int64_t num_intervals, uint8_t* head,
                          int32_t* isl_group, int64_t* isl_start, int64_t* isl_end, int64_t max_groups, int32_t* grp_code,
                          int64_t* grp_covered, int64_t* grp_count, int64_t* result_host, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- Positional encodings: k-step PageRank and random-walk return probabilities ------------------------------------------------------
 * Replaces the nb_pos_enc > 0 half of utils/data_utils.py:44-92 (add_positional_encoding; the in_deg / out_deg half is read off the
 * views' CSR pointers), as tests/positional_statement.py states it.  Both are fp64 until one final cast, use no atomics and sum in a
 * fixed association: the same input gives the same bits on every launch.  num_nodes < 2^31, 1 <= pe_dim <= 1024; num_nodes == 0
 * returns 0 without a launch.
 *
 * gnnome_pagerank_steps_f64 (data_utils.py:74-90): x_0 = 1/n, x_{t+1}[v] = 0.95 * sum_{u -> v} x_t[u] * dinv[u] + (1 - 0.95)/n with
 *   dinv[u] = 1/(out_deg[u] + 1e-9), 0 where out_deg[u] < 1e-9; table[v, t] = x_{t+1}[v], t = 0 .. pe_dim-1 (double[num_nodes, pe_dim],
 *   row-major, stays on the device).  in_ptr int32[N+1] / in_src int32[E]: the destination-sorted in-lists of the graph views
 *   (in_ptr, srt_src); out_deg int32[N].  A parallel edge is one term per copy, a self-loop an ordinary edge.  One launch per step;
 *   a destination's terms are added in list order, a list longer than 64 by the wavefront (lane l takes entries l, l + 64, ..., the
 *   64 partial sums meet in the xor butterfly 32 .. 1).  out_f32 float[num_nodes, pe_dim], or NULL to keep the fp64 table only: the
 *   reference's .float() (:88), one cast of the finished table.  Workspace: gnnome_pagerank_workspace_bytes (two fp64 vectors).
 *
 * gnnome_rw_return_f64 (data_utils.py:59-72): PE[i, t-1] = (M^t)[i, i], t = 1 .. pe_dim, M[u, v] = mult(u -> v) / max(in_deg[v], 1).
 *   Which axis DGL's adjacency_matrix puts the sources on does not matter: the diagonal entry is the sum over the closed walks of
 *   length t through i of the product of 1/max(in_deg, 1) over the walk's nodes, and the transposed convention sums the same walks
 *   read backwards.  out_ptr int32[N+1] / out_dst int32[E]: the out-lists of the graph views; in_deg int32[N].  No matrix power is
 *   formed: the workgroup of node i keeps the sparse row e_i^T M^t as (node id, fp64 value) pairs in LDS and advances it pe_dim
 *   times through the out-lists - expand, sort the pairs by (node id, row order, edge order), add every run of equal ids left to
 *   right - reading off the entry of i after each step; an empty row ends the node, its remaining columns are 0.
 *   capacity: the (node, value) pairs ONE expansion may hold = the sum of the out-degrees over the row's nodes; it costs
 *   gnnome_rw_return_lds_bytes = 8 * pow2ceil(capacity) + 24 * capacity + 4 bytes of LDS per workgroup, which must fit a CU's
 *   160 KiB (capacity <= 4096; GNNOME_EINVAL beyond).  A node whose expansion would exceed it stops before writing anything past a
 *   buffer, stores the size it needed in info and sets status[0] = 1 (zeroed here first).
 *   info int32[num_nodes, 2]: per node the largest expansion it needed (at least that: a node stops at its first overflow) and the
 *   number of steps it ran before its row was empty (pe_dim if it never was).
 *   out: float[num_nodes, pe_dim], or double[...] with out_is_f64 != 0 - written by the last launch from the fp64 table in the
 *   workspace (one cast, :70) and ONLY if no node overflowed: with status[0] = 1 `out` is untouched.  Nothing synchronises; the
 *   caller reads status[0] after the stream.  Workspace: gnnome_rw_return_workspace_bytes (1/in_deg and the fp64 table). */
int gnnome_pagerank_workspace_bytes(int64_t num_nodes, size_t* bytes_host);
int gnnome_pagerank_steps_f64(const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_deg, int64_t num_nodes, int pe_dim,
                              double* table, float* out_f32, void* workspace, size_t workspace_bytes, void* stream);
int gnnome_rw_return_lds_bytes(int capacity, size_t* bytes_host);
int gnnome_rw_return_workspace_bytes(int64_t num_nodes, int pe_dim, size_t* bytes_host);
int gnnome_rw_return_f64(const int32_t* out_ptr, const int32_t* out_dst, const int32_t* in_deg, int64_t num_nodes, int pe_dim,
                         int capacity, void* out, int out_is_f64, int32_t* info, int32_t* status, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- Overlap graph from reads: minimizer sketch, seed pairs, banded chains -----------------------------------------------------------
 * The step graph_dataset.py:76-186 leaves to hifiasm / raven, as tests/overlap_graph_statement.py states it: integers only, every output
 * order fixed by a count and an exclusive scan before anything is written, no result depends on the grid or on the order atomics land in
 * (there are none).  data uint8[total] / off int64[R+1]: the reads as overlap.pack_reads lays them out, data 4-byte aligned, R < 2^30,
 * every read shorter than 2^30 bases.  1 <= k <= 31.
 *
 * The hash: bases A, C, G, T in either case are 0 .. 3, a k-mer's code is the smaller of its forward (first base most significant) and
 * reverse-complement 2k-bit codes, strand = 1 where that is the reverse complement; a k-mer over any other byte, or equal to its reverse
 * complement, is invalid.  With m = 2^(2k) - 1 the hash is Thomas Wang's 64-bit mix, every step masked to m (a bijection of [0, m]):
 *   x = (~x + (x << 21)) & m; x ^= x >> 24; x = (x + (x << 3) + (x << 8)) & m; x ^= x >> 14; x = (x + (x << 2) + (x << 4)) & m;
 *   x ^= x >> 28; x = (x + (x << 31)) & m.
 *
 * gnnome_sketch_reads: position p of a read is a minimizer when some window of w consecutive k-mer starts inside the read has its
 *   smallest valid hash at p, ties to the leftmost; reads shorter than k + w - 1 give none.  One workgroup per tile of
 *   gnnome_sketch_tile_size windows of one read; tile_first int64[R+1] (device): the exclusive scan of ceil(windows / tile) over the
 *   reads, num_tiles = tile_first[R]; k + w - 1 <= 256.  Called twice on one workspace (gnnome_sketch_workspace_bytes(num_tiles)):
 *   with hash == NULL it counts, scans and SYNCHRONISES `stream` once to fill result_host[0] (HOST memory) with the number of
 *   minimizers M; with the four outputs (hash uint64, read int32, pos int32, strand uint8, each [capacity], capacity = M) it writes
 *   them in (read, pos) order and does not synchronise.  The workspace starts with int64[num_tiles + 1]: the first output slot of every
 *   tile, M last - a read's slice of the output starts at the slot of its first tile.
 * gnnome_seed_pairs: hash / read / pos / strand [num_seeds]: the sketch sorted STABLY by hash.  A hash with more than max_occ seeds is
 *   dropped whole; every other gives each pair of its seeds that lie in different reads, a < b their reads: rel = strand_a ^ strand_b,
 *   pb' = pb if rel == 0 else len_b - k - pb, d = pa - pb'.  Record t is the two sort keys key_ab[t] = a << 32 | b << 1 | rel and
 *   key_dp[t] = (d + 2^30) << 32 | pa; the order the records are written in is fixed (by the later seed, then by the earlier) and is
 *   not the sorted order - the caller sorts by (key_ab, key_dp).  Called twice on one workspace (gnnome_seed_pairs_workspace_bytes):
 *   key_ab == NULL counts, scans and SYNCHRONISES once to fill result_host[0] with the exact number of records P - nothing is
 *   written anywhere but the workspace; with key_ab / key_dp int64[capacity], capacity = P, it writes them.  1 <= max_occ <= 2^20.
 * gnnome_chain_overlaps: key_ab / key_dp [num_records] sorted by (key_ab, key_dp); group_start int64[num_groups + 1]: where each run
 *   of equal key_ab starts, num_records last.  One wavefront per group walks it in order: a band starts at a record and takes every
 *   following record whose d is at most `band` above the band's first d, the next band starts at the first record left out; per band
 *   n_seeds, span_beg = min pa, span_end = max pa + k, d_beg = the d at the smallest pa (ties: smallest d), d_end = the d at the largest
 *   pa (ties: largest d); the group's overlap is the band with the most seeds, ties to the first.  In the frame where a is forward and
 *   b' is b (rel = 0) or its reverse complement, As = max(0, d_beg), Ae = min(len_a, len_b + d_end), and kind is, first match wins:
 *   5 n_seeds < min_seeds; 0 (internal match) span_beg - As > max_hang or Ae - span_end > max_hang; 1 (b contained) d_beg >= 0 and
 *   len_b + d_end <= len_a; 2 (a contained) d_beg <= 0 and len_a <= len_b + d_end; 3 (a -> b', edge (2a, 2b + rel)) d_beg > 0,
 *   overlap_length = min(len_a - d_beg, len_b); 4 (b' -> a, edge (2b + rel, 2a)) the rest, overlap_length = min(len_b + d_beg, len_a);
 *   a kind 3 or 4 with overlap_length < min_overlap becomes 6.  out int32[10, num_groups], one plane per field: a, b, rel, kind, d_beg,
 *   d_end, n_seeds, span_beg, span_end, overlap_length (0 unless kind is 3, 4 or 6).  No workspace, no synchronisation. */
int gnnome_sketch_tile_size(int* tile_host);
int gnnome_sketch_workspace_bytes(int64_t num_tiles, size_t* bytes_host);
int gnnome_sketch_reads(const uint8_t* data, const int64_t* off, int64_t num_reads, int k, int w, const int64_t* tile_first,
                        int64_t num_tiles, uint64_t* hash, int32_t* read, int32_t* pos, uint8_t* strand, int64_t capacity,
                        int64_t* result_host, void* workspace, size_t workspace_bytes, void* stream);
int gnnome_seed_pairs_workspace_bytes(int64_t num_seeds, size_t* bytes_host);
int gnnome_seed_pairs(const uint64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand, int64_t num_seeds,
                      const int64_t* off, int64_t num_reads, int k, int max_occ, int64_t* key_ab, int64_t* key_dp, int64_t capacity,
                      int64_t* result_host, void* workspace, size_t workspace_bytes, void* stream);
int gnnome_chain_overlaps(const int64_t* key_ab, const int64_t* key_dp, int64_t num_records, const int64_t* group_start,
                          int64_t num_groups, const int64_t* off, int64_t num_reads, int k, int band, int min_seeds, int min_overlap,
                          int max_hang, int32_t* out, void* stream);

/* ---- Overlap-graph simplification: transitive edges and tips ------------------------------------------------------------------------
 * As tests/graph_simplify_statement.py states them, on a graph that follows the complement convention (node v ^ 1 is the reverse
 * complement of v, edge (u, v) has the mate (v ^ 1, u ^ 1)); p(e) is the edge's prefix length.  Integers only, no atomics; every decision
 * reads only the inputs and every flag stored is 1, so no result depends on the grid or on timing.  num_nodes, num_edges < 2^31.
 *
 * gnnome_transitive_edges: the edges sorted by (src, dst) - row_ptr int64[N + 1]: node v's out-edges are the positions
 *   row_ptr[v] .. row_ptr[v + 1]; dst, prefix, edge_id int32[E] per position (edge_id: where the edge's flag goes) - and mark uint8[E],
 *   zeroed here.  A simultaneous rule on the input graph (raven's; not Myers' sequential marking): mark[e] = 1 for e = (v, x) iff there
 *   are a node w, w != v and w != x, and edges e1 = (v, w), e2 = (w, x) with |p(e1) + p(e2) - p(e)| <= fuzz (fuzz >= 0, an absolute
 *   number of bases; parallel edges are separate edges).  p(e1) + p(e2) - p(e) = len(w) - ol(e1) - ol(e2) + ol(e) is the same for the
 *   mates, so an edge is marked iff its mate is.  One wavefront per v; out(v) is staged in LDS gnnome_transitive_tile_size entries at a
 *   time, and a longer row is done tile by tile.  No workspace, no synchronisation.
 * gnnome_tip_nodes: in_deg, out_deg int32[N]; succ, succ_prefix int32[N]: the target and the p of a node's out-edge where out_deg
 *   is 1 (not read elsewhere); in_ptr int64[N + 1] / in_src int32[E]: the sources of every node's in-edges; tip uint8[N], zeroed
 *   here; N even.  A tip start is a node of in-degree 0 and out-degree 1.  From c0 = s the unique out-edges are followed; the node
 *   reached next is, in this order: the junction j if its in-degree is >= 2 (the chain ends); the end of a chain that is no tip if
 *   its out-degree is not 1; else the next chain node.  The chain c0 .. c(m-1) is a candidate iff it reached a junction with
 *   m <= max_tip (>= 1); its weight is the sum of p over its m edges.  At a junction with an in-edge that does not come from the
 *   last node of one of its candidates every candidate is a tip; where all in-edges do, all but one are: the heaviest, ties to the
 *   smallest c(m-1), survives.  tip[c] = tip[c ^ 1] = 1 for every node c of a tip.  Two launches, one lane per node; the
 *   workspace (gnnome_tip_nodes_workspace_bytes) holds the candidates.  No synchronisation. */
int gnnome_transitive_tile_size(int* tile_host);
int gnnome_transitive_edges(const int64_t* row_ptr, const int32_t* dst, const int32_t* prefix, const int32_t* edge_id, int64_t num_nodes,
                            int64_t num_edges, int fuzz, uint8_t* mark, void* stream);
int gnnome_tip_nodes_workspace_bytes(int64_t num_nodes, size_t* bytes_host);
int gnnome_tip_nodes(const int32_t* in_deg, const int32_t* out_deg, const int32_t* succ, const int32_t* succ_prefix,
                     const int64_t* in_ptr, const int32_t* in_src, int64_t num_nodes, int max_tip, uint8_t* tip, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- Unitig compaction: links, chains and their ranking -----------------------------------------------------------------------------
 * As tests/unitig_statement.py states it, on a graph that follows the complement convention, whose edge multiset is closed under
 * mates and whose prefixes are p(e) = read_length[src] - overlap_length (the caller checks all three before any launch).
 *
 * The rule.  Degrees count parallel edges.  Edge (u, v) is a link iff out_deg(u) == 1, in_deg(v) == 1 and u >> 1 != v >> 1; the last
 * clause keeps self-loops and hairpins u -> u ^ 1 out, and an edge is a link iff its mate is.  A chain is a maximal path over links;
 * every node is in exactly one chain, a node without links is a chain of one, and under mate closure no chain holds both v and v ^ 1,
 * so the complement of a chain (reversed, every node ^ 1) is another chain.  A component all of whose edges are links has no head:
 * with r its smallest read, the cycle that holds node 2r starts at 2r and the cycle that holds 2r + 1 ends at 2r + 1; the link that
 * enters the start is the cut link and is not internal.  Of a chain and its complement the forward one has the smaller head; the
 * pairs are numbered q = 0, 1, .. by ascending forward head, unitig node 2q is the forward chain and 2q + 1 its complement.  A node's
 * rank is its 0-based place in its chain, its offset the summed p of the links before it, a chain's length offset[tail] +
 * read_length[tail] (equal for 2q and 2q + 1 by the prefix identity).  Every edge that is not internal runs from a chain's tail to a
 * chain's head and becomes the edge (unitig[u], unitig[v]) of the unitig graph, a cut link thereby a self-edge; compaction of that
 * graph changes nothing.
 *
 * gnnome_unitig_links: src, dst, prefix int64[E]; out_deg, in_deg int32[N].  link uint8[E] = the link flag of every edge; succ, pred
 *   int32[N] (-1: none), weight int32[N] (the p of the node's out-link) and succ_edge int32[N] (its edge id) are initialised here
 *   and written by the links - one writer per slot.  Node ids outside [0, N) make no link.  No synchronisation.
 * gnnome_unitig_rank: list ranking by pointer jumping over those tables, N even.  head int32[N], rank int32[N], offset int64[N] per
 *   node; cyc uint8[N] = 1 for the nodes of cycles; succ, pred and link are UPDATED where a cycle is cut.  No atomics, integers
 *   only, double-buffered 16-byte records (ancestor, hops, bases): every byte is the same on every call and for every `grid` (the
 *   workgroups per launch; 0: by size).  One jump per node and launch, so a chain of n nodes takes ceil(log2 n) launches; after each
 *   the number of unfinished nodes is read back (the entry SYNCHRONISES `stream`; not capturable).  When that number stops falling
 *   the rest are cycles: their smallest reads are found by the same doubling until the jump distance reaches the number of leftover
 *   nodes, the cycles are cut and the leftover ranked.  rounds_host int64[4] (or NULL): jump launches on the paths, minimum launches,
 *   jump launches after the cut, nodes on cycles - a graph without cycles reports 0 for the last three and launches nothing for them.
 *   Every index read from a table is range-checked before use.  workspace: gnnome_unitig_rank_workspace_bytes.
 * gnnome_unitig_scatter: chain_nodes[chain_off[unitig[v]] + rank[v]] = v for every node v (unitig, rank int32[N], chain_off
 *   int64[U + 1], chain_nodes int32[N], preset to -1); an index outside its table is skipped.  No synchronisation. */
int gnnome_unitig_links(const int64_t* src, const int64_t* dst, const int64_t* prefix, const int32_t* out_deg, const int32_t* in_deg,
                        int64_t num_nodes, int64_t num_edges, int32_t* succ, int32_t* pred, int32_t* weight, int32_t* succ_edge,
                        uint8_t* link, void* stream);
int gnnome_unitig_rank_workspace_bytes(int64_t num_nodes, size_t* bytes_host);
int gnnome_unitig_rank(int32_t* succ, int32_t* pred, const int32_t* weight, const int32_t* succ_edge, int64_t num_nodes,
                       int64_t num_edges, uint8_t* link, uint8_t* cyc, int32_t* head, int32_t* rank, int64_t* offset, int grid,
                       int64_t* rounds_host, void* workspace, size_t workspace_bytes, void* stream);
int gnnome_unitig_scatter(const int32_t* unitig, const int32_t* rank, const int64_t* chain_off, int64_t num_nodes, int64_t num_unitigs,
                          int32_t* chain_nodes, void* stream);

/* ---- Simple bubbles: arms, their judgement and the node mark ------------------------------------------------------------------------
 * As tests/bubble_statement.py states it, on the kept edges of a graph that follows the complement convention, closed under mates and
 * with p(e) = read_length[src] - overlap_length (the caller checks all three before any launch); degrees count parallel edges.
 *
 * The rule.  An arm is a chain a_1 .. a_k (k >= 1) of the unitig ranking on the kept edges that is not circular, whose head has
 * in-degree 1 and whose tail has out-degree 1 (every node of it then has both), whose one in-edge comes from a node s of out-degree
 * >= 2 and whose one out-edge goes to a node t of in-degree >= 2, with t != s and t != s ^ 1.  s -> a_1 and a_k -> t are no links,
 * so an arm is one whole chain; a direct edge s -> t is no arm (the transitive rule's case), and parallel edges s -> a_1 make a_1 a
 * join.  Three integers, equal for an arm and for its mate arm a_k ^ 1 .. a_1 ^ 1 from t ^ 1 to s ^ 1: weight = the sum of a
 * caller's weight[a_i] (weight[v] == weight[v ^ 1]); overlap = the sum of overlap_length over the arm's k + 1 edges; dist = the sum
 * of read_length[a_i] - overlap, the bases between the end of s and the start of t (it may be negative; the summed p would differ
 * between an arm and its mate by len(s) - len(t)).  A bubble is the arms that share (s, t), when there are at least two; its winner
 * has the largest (weight, overlap, -min(a_1, a_k ^ 1)), a triple that is equal for an arm and its mate and differs between two
 * arms of one bubble.  Another arm of the bubble is a loser iff dist(winner) <= max_dist, dist(arm) <= max_dist and
 * |dist(arm) - dist(winner)| <= max_diff (absolute numbers of bases).  The nodes of every loser and their complements are marked;
 * all bubbles are judged on the input at once: s and t are no arm nodes, arms are disjoint, and an arm whose complement lay in an arm
 * of the same bubble would need t == s ^ 1, so the mark is the same on both strands, the kept edges stay closed under mates and s
 * still reaches t.  Bubbles with a direct-edge arm, bubbles whose arms branch and t == s ^ 1 are left alone.
 *
 * gnnome_bubble_arms: src, dst, overlap int64[E] (the kept edges); in_deg, out_deg int32[N]; chain_off int64[U + 1], chain_nodes
 *   int32[N], circular uint8[U], length int64[U] as the unitig entries and their caller give them; cum_weight, cum_length int64[N + 1]:
 *   the exclusive prefix sums of weight and read_length in chain_nodes' order.  in_edge, out_edge int32[N] are set here: the id of a
 *   node's one in-edge / out-edge where that degree is 1, else -1.  arms: U records of 40 bytes {int32 s, t, key, nodes; int64 weight,
 *   overlap, dist}, s = -1 where the chain is no arm.  Two launches, one lane per edge, then one per chain; no lane walks a chain.
 * gnnome_bubble_judge: row_ptr int64[N + 1] / dst int32[E]: the kept edges sorted by (src, dst), as for gnnome_transitive_edges;
 *   unitig, rank int32[N]; loser uint8[U], zeroed here, = 1 for every losing arm's chain.  One wavefront per source of out-degree >= 2;
 *   its row is staged in LDS gnnome_bubble_tile_size entries at a time, a longer row is done tile by tile and in passes of 64 arms.
 * gnnome_bubble_mark: mark uint8[N], every entry written: loser[unitig[v]] | loser[unitig[v ^ 1]]; N even.
 * Integers only, no atomics, one writer per slot or every writer storing the same 1: the bytes are the same on every call and for every
 * `grid` (the workgroups per launch; 0: by size).  Every index read from a table is range-checked before use.  No workspace, no
 * synchronisation. */
int gnnome_bubble_tile_size(int* tile_host);
int gnnome_bubble_arms(const int64_t* src, const int64_t* dst, const int64_t* overlap, const int32_t* in_deg, const int32_t* out_deg,
                       int64_t num_nodes, int64_t num_edges, const int64_t* chain_off, const int32_t* chain_nodes, const uint8_t* circular,
                       const int64_t* length, const int64_t* cum_weight, const int64_t* cum_length, int64_t num_unitigs, int32_t* in_edge,
                       int32_t* out_edge, void* arms, int grid, void* stream);
int gnnome_bubble_judge(const int64_t* row_ptr, const int32_t* dst, const int32_t* unitig, const int32_t* rank, const void* arms,
                        int64_t num_nodes, int64_t num_edges, int64_t num_unitigs, int64_t max_dist, int64_t max_diff, uint8_t* loser,
                        int grid, void* stream);
int gnnome_bubble_mark(const int32_t* unitig, const uint8_t* loser, int64_t num_nodes, int64_t num_unitigs, uint8_t* mark, int grid,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNOME_HIP_H */
