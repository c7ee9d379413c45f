// Contig spelling: decoded walks -> contig sequences, optionally as FASTA bodies (utils/evaluate.py:38-48 walk_to_sequence,
// :51-53 save_assembly; inference.py:463 masks the prefixes first).
//
//   gnnome_contig_pieces   one thread per step: the piece a step contributes, after checking every walk and every pair
//   (exclusive scan of the pieces: a torch operator in gnnome_amd/contigs.py)
//   gnnome_contig_spell    the copy, split by OUTPUT bytes
//
// The contract, step by step (evaluate.py:40-43): for a step u -> v that is not the walk's last node the piece is
// reads[u][:prefix_length[edges[u, v]]] under Python's slice rule, and the last node contributes its whole read.  Node 2r is
// read r and node 2r+1 its reverse complement (graph_parser.py:183-184, :365); the store holds the forward strand only, so
// an odd node reads read r backwards from its end through the complement table (Bio.Seq's IUPAC table in both cases; every
// other byte unchanged) - no reverse-complemented copy of the reads exists anywhere.
//
// Contig lengths span five orders of magnitude, so the copy does not give a workgroup a walk: every workgroup owns a fixed
// tile of the output, finds the first contig and the first piece that reach into it by binary search, and every lane builds
// 16 consecutive output bytes and writes them with one 16-byte store where the tile is a whole vector of body bytes.  No
// atomics: the output is a function of the inputs alone.  All offsets are int64 (a human assembly's FASTA image exceeds 2^31).
#include "common.h"

namespace gnnome {

constexpr int kSpellThreads = 256;
constexpr int kSpellChunks = 4;                                   // 16-byte chunks per lane per tile
constexpr int64_t kSpellTile = (int64_t)kSpellThreads * 16 * kSpellChunks;
constexpr int kCheckThreads = 256;
constexpr int kCheckBlocksMax = 1024;
constexpr int kInfoWords = 8;

enum { kSpellOk = 0, kSpellEmptyWalk = 1, kSpellBadOffsets = 2, kSpellNodeRange = 3, kSpellNotEdge = 4 };

// Bio.Data.IUPACData.ambiguous_dna_complement in both letter cases (gnnome_amd/overlap.py COMPLEMENT); identity elsewhere
__constant__ uint8_t kComplementPairs[2][17] = {
    {'A', 'C', 'G', 'T', 'M', 'R', 'W', 'S', 'Y', 'K', 'V', 'H', 'D', 'B', 'X', 'N', 'U'},
    {'T', 'G', 'C', 'A', 'K', 'Y', 'W', 'S', 'R', 'M', 'B', 'D', 'H', 'V', 'X', 'N', 'A'}};

// last index i in [lo, hi) with key(i) <= x; lo when there is none
template <class Key>
__device__ __forceinline__ int64_t last_le(int64_t lo, int64_t hi, int64_t x, Key key) {
    int64_t a = lo, b = hi;   // invariant: the answer is in [a, b)
    while (b - a > 1) {
        const int64_t m = a + (b - a) / 2;
        if (key(m) <= x) a = m;
        else b = m;
    }
    return a;
}

// the same answer found by the 64 lanes of one wave together: 64 probes per round, so a million keys take four dependent
// rounds instead of twenty.  Every lane must call it with the same arguments.
template <class Key>
__device__ __forceinline__ int64_t wave_last_le(int64_t lo, int64_t hi, int64_t x, Key key) {
    const int lane = threadIdx.x & 63;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64, idx = lo + lane * step;
        const int n = __popcll(__ballot(idx < hi && key(idx) <= x));   // keys are sorted: the lanes that pass are a prefix
        if (n == 0) return lo;
        const int64_t nlo = lo + (int64_t)(n - 1) * step;
        hi = nlo + step < hi ? nlo + step : hi;
        lo = nlo;
    }
    return lo;
}

struct StepCheck {
    int code;
    int64_t walk, u, v;   // v: the next node, unless `last`
    bool last;
    int64_t piece;        // bytes the step contributes (code == kSpellOk)
};

// What step s contributes, or why it cannot (evaluate.py:40-43).  Walk offsets are checked by the caller's walk items.
__device__ StepCheck check_step(int64_t s, const int32_t* walk_nodes, int64_t S, const int64_t* walk_off, int64_t W,
                                const int32_t* succ_ptr, const int32_t* succ_nbr, const int32_t* succ_eid, const int32_t* prefix_len,
                                int64_t N, const int64_t* read_off) {
    StepCheck c{kSpellOk, 0, 0, -1, false, 0};
    c.walk = last_le(0, W, s, [&](int64_t i) { return walk_off[i]; });
    const int64_t end = walk_off[c.walk + 1];
    const bool last = s + 1 >= end || s + 1 >= S;
    c.last = last;
    c.u = walk_nodes[s];
    if (!last) c.v = walk_nodes[s + 1];
    if (c.u < 0 || c.u >= N || (!last && (c.v < 0 || c.v >= N))) {
        c.code = kSpellNodeRange;
        return c;
    }
    const int64_t r = c.u >> 1;
    const int64_t len_u = read_off[r + 1] - read_off[r];
    if (last) {
        c.piece = len_u;
        return c;
    }
    const int row = succ_ptr[c.u], deg = succ_ptr[c.u + 1] - row;
    int eid = -1;
    for (int j = 0; j < deg; ++j)
        if (succ_nbr[row + j] == (int)c.v) {   // every slot of a parallel pair carries the pair's id (decode.DecodeGraph)
            eid = succ_eid[row + j];
            break;
        }
    if (eid < 0) {
        c.code = kSpellNotEdge;
        return c;
    }
    const int64_t p = prefix_len[eid];
    c.piece = p >= 0 ? (p < len_u ? p : len_u) : (len_u + p > 0 ? len_u + p : 0);   // reads[u][:p]
    return c;
}

// items [0, W) check the walk offsets, items [W, W + S) the steps; block b writes the smallest failing item it saw (or
// INT64_MAX) to partial[b] - a grid-stride loop over a fixed grid, so the answer does not depend on scheduling
__global__ __launch_bounds__(kCheckThreads) void k_contig_check(const int32_t* __restrict__ walk_nodes, int64_t S,
                                                                const int64_t* __restrict__ walk_off, int64_t W,
                                                                const int32_t* __restrict__ succ_ptr, const int32_t* __restrict__ succ_nbr,
                                                                const int32_t* __restrict__ succ_eid, const int32_t* __restrict__ prefix_len,
                                                                int64_t N, const int64_t* __restrict__ read_off, int64_t* partial) {
    __shared__ int64_t red[kCheckThreads / 64];
    int64_t bad = INT64_MAX;
    const int64_t items = W + S;
    for (int64_t i = (int64_t)blockIdx.x * kCheckThreads + threadIdx.x; i < items && bad == INT64_MAX;
         i += (int64_t)gridDim.x * kCheckThreads) {
        if (i < W) {
            const int64_t a = walk_off[i], b = walk_off[i + 1];
            if (a >= b || a < 0 || b > S || (i == 0 && a != 0) || (i == W - 1 && b != S)) bad = i;
        } else if (check_step(i - W, walk_nodes, S, walk_off, W, succ_ptr, succ_nbr, succ_eid, prefix_len, N, read_off).code != kSpellOk) {
            bad = i;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = __shfl_xor(bad, o);
        bad = t < bad ? t : bad;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kCheckThreads / 64; ++k) bad = red[k] < bad ? red[k] : bad;
        partial[blockIdx.x] = bad;
    }
}

// one block: the first failing item over all blocks, and what is wrong with it -> info[0..5] = {item, code, walk, u, v, last}
__global__ __launch_bounds__(kCheckThreads) void k_contig_first_error(const int64_t* __restrict__ partial, int nparts,
                                                                      const int32_t* __restrict__ walk_nodes, int64_t S,
                                                                      const int64_t* __restrict__ walk_off, int64_t W,
                                                                      const int32_t* __restrict__ succ_ptr, const int32_t* __restrict__ succ_nbr,
                                                                      const int32_t* __restrict__ succ_eid, const int32_t* __restrict__ prefix_len,
                                                                      int64_t N, const int64_t* __restrict__ read_off, int64_t* info) {
    __shared__ int64_t red[kCheckThreads / 64];
    int64_t bad = INT64_MAX;
    for (int k = threadIdx.x; k < nparts; k += kCheckThreads) bad = partial[k] < bad ? partial[k] : bad;
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = __shfl_xor(bad, o);
        bad = t < bad ? t : bad;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < kCheckThreads / 64; ++k) bad = red[k] < bad ? red[k] : bad;
    int64_t out[kInfoWords] = {bad, kSpellOk, -1, -1, -1, 0, 0, 0};
    if (bad < W) {
        const int64_t a = walk_off[bad], b = walk_off[bad + 1];
        out[1] = (a == b) ? kSpellEmptyWalk : kSpellBadOffsets;
        out[2] = bad;
    } else if (bad != INT64_MAX) {
        const StepCheck c = check_step(bad - W, walk_nodes, S, walk_off, W, succ_ptr, succ_nbr, succ_eid, prefix_len, N, read_off);
        out[1] = c.code;
        out[2] = c.walk;
        out[3] = c.u;
        out[4] = c.v;
        out[5] = c.last;
    }
    for (int k = 0; k < kInfoWords; ++k) info[k] = out[k];
}

__global__ __launch_bounds__(kCheckThreads) void k_contig_pieces(const int32_t* __restrict__ walk_nodes, int64_t S,
                                                                 const int64_t* __restrict__ walk_off, int64_t W,
                                                                 const int32_t* __restrict__ succ_ptr, const int32_t* __restrict__ succ_nbr,
                                                                 const int32_t* __restrict__ succ_eid, const int32_t* __restrict__ prefix_len,
                                                                 int64_t N, const int64_t* __restrict__ read_off, int64_t* __restrict__ piece_len) {
    for (int64_t s = (int64_t)blockIdx.x * kCheckThreads + threadIdx.x; s < S; s += (int64_t)gridDim.x * kCheckThreads)
        piece_len[s] = check_step(s, walk_nodes, S, walk_off, W, succ_ptr, succ_nbr, succ_eid, prefix_len, N, read_off).piece;
}

// The layout of one contig in the output: its body starts at bo and is blen bytes long; it holds the n bytes that start at
// cst in the unwrapped stream (piece_off's coordinates), with '\n' after every lw bytes and after a final partial line.
struct Body {
    int64_t bo, blen, cst, n;
};

struct SpellArgs {
    const int32_t* walk_nodes;
    const int64_t* walk_off;
    const int64_t* piece_off;
    const uint8_t* reads;
    const int64_t* read_off;
    const int64_t* body_off;   // NULL: bo = cst
    uint8_t* out;
    int64_t S, W, R, out_bytes;
    int lw;
    int aligned;               // out is 16-byte aligned: whole chunks go out as one vector store
};

__device__ __forceinline__ int64_t body_start(const SpellArgs& a, int64_t w) {
    return a.body_off ? a.body_off[w] : a.piece_off[a.walk_off[w]];
}

__device__ __forceinline__ Body body_of(const SpellArgs& a, int64_t w) {
    Body b;
    b.cst = a.piece_off[a.walk_off[w]];
    b.n = a.piece_off[a.walk_off[w + 1]] - b.cst;
    b.bo = a.body_off ? a.body_off[w] : b.cst;
    b.blen = a.lw > 0 ? b.n + (b.n + a.lw - 1) / a.lw : b.n;
    return b;
}

// the data byte of body b nearest to output position o, as an unwrapped position (clamped into the contig)
__device__ __forceinline__ int64_t unwrapped_near(const Body& b, int64_t o, int lw) {
    if (b.n <= 0) return b.cst;
    int64_t qo = o - b.bo;
    qo = qo < 0 ? 0 : (qo >= b.blen ? b.blen - 1 : qo);
    int64_t q = qo;
    if (lw > 0) {
        const int64_t line = qo / (lw + 1), col = qo - line * (lw + 1);
        q = line * lw + (col < lw ? col : lw);
    }
    return b.cst + (q < b.n ? q : b.n - 1);
}

__global__ __launch_bounds__(kSpellThreads) void k_contig_spell(const SpellArgs a) {
    __shared__ uint8_t comp[256];
    __shared__ int64_t range[4];   // contigs [w_lo, w_hi] and pieces [s_lo, s_hi] that reach into this tile
    for (int k = threadIdx.x; k < 256; k += kSpellThreads) comp[k] = (uint8_t)k;
    __syncthreads();
    if (threadIdx.x < 17) {
        const uint8_t f = kComplementPairs[0][threadIdx.x], t = kComplementPairs[1][threadIdx.x];
        comp[f] = t;
        comp[f + 32] = t + 32;   // lower case
    }
    const int64_t t0 = (int64_t)blockIdx.x * kSpellTile;
    const int64_t t1 = (t0 + kSpellTile < a.out_bytes ? t0 + kSpellTile : a.out_bytes) - 1;
    if (threadIdx.x < 64) {   // wave 0 narrows the search for the whole workgroup
        const auto bo = [&](int64_t w) { return body_start(a, w); };
        const int64_t w_lo = wave_last_le(0, a.W, t0, bo), w_hi = wave_last_le(w_lo, a.W, t1, bo);
        const int64_t g_lo = unwrapped_near(body_of(a, w_lo), t0, a.lw), g_hi = unwrapped_near(body_of(a, w_hi), t1, a.lw);
        const int64_t p0 = a.walk_off[w_lo], p1 = a.walk_off[w_hi + 1];
        const auto po = [&](int64_t s) { return a.piece_off[s]; };
        const int64_t s_lo = wave_last_le(p0, p1, g_lo, po), s_hi = wave_last_le(s_lo, p1, g_hi, po);
        if (threadIdx.x == 0) {
            range[0] = w_lo;
            range[1] = w_hi;
            range[2] = s_lo;
            range[3] = s_hi;
        }
    }
    __syncthreads();
    const int64_t w_lo = range[0], w_hi = range[1], s_lo = range[2], s_hi = range[3];
    const int lw = a.lw;
    for (int ch = 0; ch < kSpellChunks; ++ch) {
        const int64_t o0 = t0 + ((int64_t)ch * kSpellThreads + threadIdx.x) * 16;
        if (o0 >= a.out_bytes) break;
        int64_t w = last_le(w_lo, w_hi + 1, o0, [&](int64_t i) { return body_start(a, i); });
        Body b = body_of(a, w);
        int64_t q = 0, col = 0;          // data bytes of the contig before the current position; column in its line
        bool fresh = true;               // q / col not yet derived for this contig
        int64_t s = -1, ps = 0, pe = 0;  // current piece and its [start, end) in the unwrapped stream
        int64_t rbeg = 0, rlen = 0;
        bool odd = false;
        uint32_t word[4] = {0, 0, 0, 0};
        uint32_t valid = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t o = o0 + j;
            if (o >= a.out_bytes) break;
            if (o >= b.bo + b.blen) {    // past this body: a later contig, or a gap the caller keeps for a header
                bool moved = false;
                while (w < w_hi && body_start(a, w + 1) <= o) {
                    ++w;
                    moved = true;
                }
                if (moved) {
                    b = body_of(a, w);
                    fresh = true;
                }
            }
            if (o < b.bo || o >= b.bo + b.blen) continue;
            if (fresh) {
                const int64_t qo = o - b.bo;
                if (lw > 0) {
                    const int64_t line = qo / (lw + 1);
                    col = qo - line * (lw + 1);
                    q = line * lw + col;
                } else {
                    q = qo;
                }
                fresh = false;
            }
            uint32_t byte;
            bool ok = true;
            if (lw > 0 && (col == lw || q >= b.n)) {
                byte = '\n';
            } else {
                const int64_t g = b.cst + q;
                if (s < 0 || g >= pe || g < ps) {
                    if (s < 0 || g < ps) s = last_le(s_lo, s_hi + 1, g, [&](int64_t i) { return a.piece_off[i]; });
                    while (s + 1 < a.S && a.piece_off[s + 1] <= g) ++s;
                    ps = a.piece_off[s];
                    pe = a.piece_off[s + 1];
                    const int64_t u = a.walk_nodes[s];
                    if (u < 0 || u >= 2 * a.R) {
                        rlen = -1;
                    } else {
                        rbeg = a.read_off[u >> 1];
                        rlen = a.read_off[(u >> 1) + 1] - rbeg;
                    }
                    odd = u & 1;
                }
                const int64_t k = g - ps;
                if (k < 0 || k >= rlen) {   // only a piece_off that gnnome_contig_pieces did not produce gets here
                    ok = false;
                    byte = 0;
                } else {
                    byte = odd ? comp[a.reads[rbeg + rlen - 1 - k]] : a.reads[rbeg + k];
                }
                ++q;
            }
            if (lw > 0 && ++col == lw + 1) col = 0;
            if (ok) {
                word[j >> 2] |= byte << (8 * (j & 3));
                valid |= 1u << j;
            }
        }
        if (valid == 0xFFFFu && a.aligned) {
            *reinterpret_cast<uint4*>(a.out + o0) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (valid & (1u << j)) a.out[o0 + j] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
        }
    }
}

}  // namespace gnnome

extern "C" int gnnome_contig_pieces_workspace_bytes(int64_t num_walks, int64_t num_steps, size_t* bytes_host) {
    using namespace gnnome;
    GN_REQUIRE(num_walks >= 0 && num_steps >= 0 && bytes_host, "contig_pieces_workspace_bytes: bad arguments");
    *bytes_host = (size_t)(kCheckBlocksMax + kInfoWords) * sizeof(int64_t);
    return GNNOME_OK;
}

extern "C" int gnnome_contig_pieces(const int32_t* walk_nodes, int64_t num_steps, const int64_t* walk_off, int64_t num_walks,
                                    const int32_t* succ_ptr, const int32_t* succ_nbr, const int32_t* succ_eid, const int32_t* prefix_length,
                                    int64_t num_nodes, const int64_t* read_off, int64_t num_reads, int64_t* piece_len, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    if (num_walks == 0) return GNNOME_OK;
    GN_REQUIRE(num_walks > 0 && num_steps >= 0 && num_nodes >= 0 && num_reads >= 0, "contig_pieces: negative size");
    GN_REQUIRE(walk_off && succ_ptr && read_off && workspace && (num_steps == 0 || (walk_nodes && piece_len)) &&
                   (num_nodes == 0 || (succ_nbr && succ_eid && prefix_length) || num_steps == 0),
               "contig_pieces: null pointer");
    GN_REQUIRE(num_nodes == 2 * num_reads, "contig_pieces: the graph has %lld nodes, the read store %lld reads (node 2r is read r, 2r+1 its "
               "reverse complement)", (long long)num_nodes, (long long)num_reads);
    GN_REQUIRE(num_nodes < ((int64_t)1 << 31), "contig_pieces: node ids are int32");
    GN_REQUIRE(workspace_bytes >= (size_t)(kCheckBlocksMax + kInfoWords) * sizeof(int64_t), "contig_pieces: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    int64_t* partial = (int64_t*)workspace;
    int64_t* info = partial + kCheckBlocksMax;
    const int64_t items = num_walks + num_steps;
    const int grid = (int)((items + kCheckThreads - 1) / kCheckThreads < kCheckBlocksMax ? (items + kCheckThreads - 1) / kCheckThreads
                                                                                        : kCheckBlocksMax);
    hipLaunchKernelGGL(k_contig_check, dim3(grid), dim3(kCheckThreads), 0, s, walk_nodes, num_steps, walk_off, num_walks, succ_ptr,
                       succ_nbr, succ_eid, prefix_length, num_nodes, read_off, partial);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_contig_first_error, dim3(1), dim3(kCheckThreads), 0, s, partial, grid, walk_nodes, num_steps, walk_off,
                       num_walks, succ_ptr, succ_nbr, succ_eid, prefix_length, num_nodes, read_off, info);
    GN_LAUNCH_CHECK();
    int64_t h[kInfoWords];
    GN_HIP(hipMemcpyAsync(h, info, sizeof(h), hipMemcpyDeviceToHost, s));
    GN_HIP(hipStreamSynchronize(s));
    const long long walk = (long long)h[2], u = (long long)h[3], v = (long long)h[4];
    switch ((int)h[1]) {
        case kSpellOk: break;
        case kSpellEmptyWalk: GN_REQUIRE(false, "contig_pieces: walk %lld is empty", walk);
        case kSpellBadOffsets:
            GN_REQUIRE(false, "contig_pieces: walk offsets must rise strictly from 0 to num_steps = %lld (walk %lld)", (long long)num_steps, walk);
        case kSpellNodeRange:
            if (!h[5])
                GN_REQUIRE(false, "contig_pieces: walk %lld: pair (%lld, %lld) has a node outside [0, %lld)", walk, u, v, (long long)num_nodes);
            GN_REQUIRE(false, "contig_pieces: walk %lld: node %lld outside [0, %lld)", walk, u, (long long)num_nodes);
        case kSpellNotEdge: GN_REQUIRE(false, "contig_pieces: walk %lld: (%lld, %lld) is not an edge", walk, u, v);
        default: GN_REQUIRE(false, "contig_pieces: unknown check result %lld", (long long)h[1]);
    }
    if (num_steps == 0) return GNNOME_OK;
    const int64_t pblocks = (num_steps + kCheckThreads - 1) / kCheckThreads;
    hipLaunchKernelGGL(k_contig_pieces, dim3((unsigned)(pblocks < 65536 ? pblocks : 65536)), dim3(kCheckThreads), 0, s, walk_nodes,
                       num_steps, walk_off, num_walks, succ_ptr, succ_nbr, succ_eid, prefix_length, num_nodes, read_off, piece_len);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_contig_spell(const int32_t* walk_nodes, int64_t num_steps, const int64_t* walk_off, int64_t num_walks,
                                   const int64_t* piece_off, const uint8_t* reads, const int64_t* read_off, int64_t num_reads,
                                   const int64_t* body_off, int line_width, uint8_t* out, int64_t out_bytes, void* stream) {
    using namespace gnnome;
    if (num_walks == 0 || out_bytes == 0) return GNNOME_OK;
    GN_REQUIRE(num_walks > 0 && num_steps >= num_walks && num_reads >= 0 && out_bytes > 0, "contig_spell: bad sizes");
    GN_REQUIRE(line_width >= 0, "contig_spell: line_width %d < 0", line_width);
    GN_REQUIRE(walk_nodes && walk_off && piece_off && reads && read_off && out && (line_width == 0 || body_off),
               "contig_spell: null pointer");
    const int64_t tiles = (out_bytes + kSpellTile - 1) / kSpellTile;
    GN_REQUIRE(tiles < ((int64_t)1 << 31), "contig_spell: output of %lld bytes too large", (long long)out_bytes);
    SpellArgs a{walk_nodes, walk_off, piece_off, reads, read_off, line_width > 0 ? body_off : nullptr, out, num_steps, num_walks,
                num_reads, out_bytes, line_width, (int)(((uintptr_t)out & 15) == 0)};
    hipLaunchKernelGGL(k_contig_spell, dim3((unsigned)tiles), dim3(kSpellThreads), 0, (hipStream_t)stream, a);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
