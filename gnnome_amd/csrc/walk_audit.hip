// The walk checks of utils/analyze.py:1-38 (assert_strand, assert_chromosome, assert_overlap) over a batch of decoded walks: one gather
// pass in place of four .item() round trips per step of a walk.
//
// The statement (tests/walk_audit_statement.py), per walk w = nodes[ptr[w] .. ptr[w+1]) with first node f = nodes[ptr[w]]:
//   strand      every later node v with strand[v] != strand[f]           -> (idx = position - 1, v)       analyze.py:1-8
//   chromosome  every later node v with chr[v] != chr[f]                 -> (idx = position - 1, v)       analyze.py:11-18
//   overlap     every pair (s, d) of consecutive nodes, idx = position of s, with                         analyze.py:21-38
//               strand[s] == strand[d] == 1 and start[d] > end[s], or strand[s] == strand[d] == -1 and end[d] < start[s]
// Both comparisons are against the walk's FIRST node, not the predecessor; equality of positions is no finding; pairs of unequal
// strands and strand values other than +-1 are silent in the overlap check; the chromosome plays no part in it.
//
// k_walk_audit: one thread per walk position t.  The walk of t comes from the caller as walk_id[t] (one repeat_interleave on the
// host side).  The thread reads its node's four values, the first node's strand and chromosome and - unless it is the walk's last
// position - its successor's strand, start and end (8-byte loads of the int64 arrays as read_gfa stores them), and writes one flag
// byte.  A node id outside [0, N) is flagged and never used as an index, and neither is a position whose walk_id / walk_ptr do not
// enclose it.  Per-walk counts: the lanes of a wavefront that share a walk form a run (walk_id ascends with t); the first lane of a
// run counts the run's flags from three ballots and adds the non-zero counts to counts[w] with integer atomics - exact integers, so
// no bit depends on the schedule.
#include "common.h"

namespace gnnome {

constexpr int kAuditThreads = 256;
enum { kAuditStrand = 1, kAuditChr = 2, kAuditOverlap = 4, kAuditBadMap = 64, kAuditBadNode = 128 };

__global__ void __launch_bounds__(kAuditThreads) k_walk_audit(const int32_t* __restrict__ walk_ptr, const int32_t* __restrict__ walk_nodes,
                                                              const int32_t* __restrict__ walk_id, int64_t W, int64_t T,
                                                              const int64_t* __restrict__ strand, const int64_t* __restrict__ start,
                                                              const int64_t* __restrict__ end, const int64_t* __restrict__ chr, int64_t N,
                                                              uint8_t* __restrict__ flags, int32_t* __restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * kAuditThreads + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int w = -1;   // < 2^31
    unsigned f = 0;
    if (t < T) {
        w = walk_id[t];
        int64_t b = 0, e = 0;
        const bool in_map = w >= 0 && w < W;
        if (in_map) {
            b = walk_ptr[w];
            e = walk_ptr[w + 1];
        }
        if (!in_map || b < 0 || e > T || t < b || t >= e) {
            f = kAuditBadMap;
            w = -1;
        } else {
            const int64_t v = walk_nodes[t];
            if (v < 0 || v >= N) {
                f = kAuditBadNode;
            } else {
                const int64_t sv = strand[v];
                const int64_t first = walk_nodes[b];
                if (t > b && first >= 0 && first < N) {   // an unusable first node is flagged at its own position
                    if (sv != strand[first]) f |= kAuditStrand;
                    if (chr[v] != chr[first]) f |= kAuditChr;
                }
                if (t + 1 < e) {
                    const int64_t d = walk_nodes[t + 1];
                    if (d >= 0 && d < N && strand[d] == sv) {
                        if (sv == 1 && start[d] > end[v]) f |= kAuditOverlap;
                        if (sv == -1 && end[d] < start[v]) f |= kAuditOverlap;
                    }
                }
            }
        }
        flags[t] = (uint8_t)f;
    }
    // runs of equal w inside the wavefront; lanes past T and unmapped positions carry w = -1 and no finding
    const int w_prev = __shfl_up(w, 1);
    const unsigned long long heads = __ballot(lane == 0 || w != w_prev);
    const unsigned long long b_strand = __ballot(f & kAuditStrand), b_chr = __ballot(f & kAuditChr), b_overlap = __ballot(f & kAuditOverlap);
    if (w >= 0 && ((heads >> lane) & 1ull)) {
        const unsigned long long later = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
        const int len = later ? __ffsll((long long)later) : kWave - lane;   // lanes of this run
        const unsigned long long run = (len == kWave ? ~0ull : ((1ull << len) - 1ull)) << lane;
        const int n_strand = __popcll(b_strand & run), n_chr = __popcll(b_chr & run), n_overlap = __popcll(b_overlap & run);
        if (n_strand) atomicAdd(counts + 3 * (int64_t)w + 0, n_strand);
        if (n_chr) atomicAdd(counts + 3 * (int64_t)w + 1, n_chr);
        if (n_overlap) atomicAdd(counts + 3 * (int64_t)w + 2, n_overlap);
    }
}

}  // namespace gnnome

extern "C" int gnnome_walk_audit(const int32_t* walk_ptr, const int32_t* walk_nodes, const int32_t* walk_id, int64_t num_walks,
                                 int64_t num_positions, const int64_t* read_strand, const int64_t* read_start, const int64_t* read_end,
                                 const int64_t* read_chr, int64_t num_nodes, uint8_t* flags, int32_t* counts, void* stream) {
    using namespace gnnome;
    const int64_t W = num_walks, T = num_positions, N = num_nodes;
    GN_REQUIRE(W >= 0 && W < ((int64_t)1 << 31) && T >= 0 && T < ((int64_t)1 << 31) && N >= 0,
               "walk_audit: num_walks=%lld or num_positions=%lld outside [0, 2^31), or num_nodes=%lld < 0", (long long)W, (long long)T,
               (long long)N);
    if (W == 0 || T == 0) return GNNOME_OK;   // nothing to look at, nothing launched: without a position no count is written either
    GN_REQUIRE(walk_ptr && walk_nodes && walk_id && flags && counts, "walk_audit: null pointer");
    GN_REQUIRE(N == 0 || (read_strand && read_start && read_end && read_chr), "walk_audit: null node array");
    hipStream_t s = (hipStream_t)stream;
    GN_HIP(hipMemsetAsync(counts, 0, (size_t)W * 3 * sizeof(int32_t), s));
    const int64_t blocks = (T + kAuditThreads - 1) / kAuditThreads;
    hipLaunchKernelGGL(k_walk_audit, dim3((unsigned)blocks), dim3(kAuditThreads), 0, s, walk_ptr, walk_nodes, walk_id, W, T, read_strand,
                       read_start, read_end, read_chr, N, flags, counts);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
