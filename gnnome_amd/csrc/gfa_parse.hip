// GFA ingestion on the device (graph_parser.py:159-340, only_from_gfa's line loop; gnnome_amd/gfa.py read_gfa is its statement here).
//
//   gnnome_gfa_mark          elementwise over the file's bytes: field starts, field ends, line starts; the first byte >= 0x80 and
//                            the first '\r' that no '\n' follows
//   (compaction of the marks and the field index of every line: torch nonzero / searchsorted in gnnome_amd/textscan.py tokenise)
//   gnnome_gfa_classify      one thread per line: kind, byte ranges of the names, LN, overlap, orientation case, SI:f: tag
//   gnnome_gfa_names_insert  the S names into an open-addressing table (32-bit compare-and-swap per slot)
//   gnnome_gfa_links         both names of every L line looked up; the line's two events (sr, dr), (sv, dv)
//   (events -> edges: sorts and segment firsts / lasts in gfa.assemble_edges, torch)
//   gnnome_gfa_pack          byte ranges of a buffer -> one packed store, split by OUTPUT bytes like gnnome_contig_spell
//
// No thread walks a line: a 50 kb sequence is two marks (its first and last byte) like every other field, so the per-line
// threads read descriptors and the short fields only.  Whitespace is what str.split() takes for it in ASCII (0x09-0x0d,
// 0x1c-0x20); a line ends at '\n' (a '\r' before it is whitespace).  Everything the host parser would turn into an exception
// or that this parser does not reproduce (see include/gnnome_hip.h) sets a per-line code, and the smallest such line is kept
// with an integer atomicMin: the caller reads it after one synchronisation.  No float is produced here: a tag's value stays
// text (the host converts all of them in one vectorised cast).  All byte offsets are int64.
#include "text_fields.h"   // the line descriptors, fields, digits, the line flag and the name hash: shared with the other text readers

namespace gnnome {

constexpr int kTokThreads = 256;
constexpr int kTokBytes = 16;                                        // bytes per lane: one 16-byte load, one 16-byte store
constexpr int64_t kTokTile = (int64_t)kTokThreads * kTokBytes;
constexpr int kPackThreads = 256;
constexpr int kPackChunks = 4;                                       // 16-byte chunks per lane per tile
constexpr int64_t kPackTile = (int64_t)kPackThreads * 16 * kPackChunks;
constexpr int kLineThreads = 256;
constexpr int kRec = 8;                                              // int64 words per line record
constexpr int kTagMax = 31;

enum { kMarkStart = 1, kMarkEnd = 2, kMarkLine = 4 };
enum { kKindOther = 0, kKindS = 1, kKindL = 2, kKindA = 3 };
// per-line codes (gnnome_amd/gfa.py _DECLINED names them)
enum {
    kGfaOk = 0, kGfaSFields = 1, kGfaLength = 2, kGfaLFields = 3, kGfaSuffix = 4, kGfaOverlap = 5, kGfaTagLong = 6, kGfaTagText = 7,
    kGfaAFields = 8, kGfaDuplicate = 9, kGfaUnknown = 10, kGfaLater = 11, kGfaHighByte = 12, kGfaBareCr = 13, kGfaDescriptor = 14,
    kGfaTableFull = 15
};

__device__ __forceinline__ bool is_ws(unsigned c) { return (c >= 0x09u && c <= 0x0du) || (c >= 0x1cu && c <= 0x20u); }

__global__ __launch_bounds__(kTokThreads) void k_gfa_mark(const uint8_t* __restrict__ buf, int64_t n, uint8_t* __restrict__ marks,
                                                          unsigned long long* bad_pos, int aligned) {
    const int64_t i0 = ((int64_t)blockIdx.x * kTokThreads + threadIdx.x) * kTokBytes;
    if (i0 >= n) return;
    const int cnt = n - i0 < kTokBytes ? (int)(n - i0) : kTokBytes;
    uint32_t w[4] = {0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au};   // past the end of the file: '\n'
    if (cnt == kTokBytes && aligned) {
        const uint4 v = *reinterpret_cast<const uint4*>(buf + i0);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < kTokBytes; ++j)
            if (j < cnt) w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((uint32_t)buf[i0 + j] << (8 * (j & 3)));
    }
    unsigned prev = i0 > 0 ? buf[i0 - 1] : '\n';
    const unsigned after = i0 + kTokBytes < n ? buf[i0 + kTokBytes] : '\n';
    uint32_t m[4] = {0, 0, 0, 0};
    long long hi = -1, cr = -1;
#pragma unroll
    for (int j = 0; j < kTokBytes; ++j) {
        const unsigned cur = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        const unsigned next = j + 1 < kTokBytes ? (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xffu : after;
        unsigned f = 0;
        if (!is_ws(cur)) f = (is_ws(prev) ? kMarkStart : 0) | (is_ws(next) ? kMarkEnd : 0);
        if (prev == '\n') f |= kMarkLine;
        if (j < cnt) {
            m[j >> 2] |= f << (8 * (j & 3));
            if (cur >= 0x80u && hi < 0) hi = i0 + j;
            if (cur == '\r' && next != '\n' && cr < 0) cr = i0 + j;
        }
        prev = cur;
    }
    if (cnt == kTokBytes && aligned) {
        *reinterpret_cast<uint4*>(marks + i0) = make_uint4(m[0], m[1], m[2], m[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kTokBytes; ++j)
            if (j < cnt) marks[i0 + j] = (uint8_t)(m[j >> 2] >> (8 * (j & 3)));
    }
    if (hi >= 0) atomicMin(&bad_pos[0], (unsigned long long)hi);
    if (cr >= 0) atomicMin(&bad_pos[1], (unsigned long long)cr);
}

// [+-]? (digits [. digits*] | . digits) ([eE] [+-]? digits)? : text that float() and numpy's cast read alike
__device__ __forceinline__ bool is_decimal(const uint8_t* buf, int64_t b, int64_t e) {
    int64_t p = b;
    if (p < e && (buf[p] == '+' || buf[p] == '-')) ++p;
    int64_t d = 0;
    while (p < e && text_is_digit(buf[p])) ++p, ++d;
    if (p < e && buf[p] == '.') {
        ++p;
        while (p < e && text_is_digit(buf[p])) ++p, ++d;
    }
    if (d == 0) return false;
    if (p < e && (buf[p] == 'e' || buf[p] == 'E')) {
        ++p;
        if (p < e && (buf[p] == '+' || buf[p] == '-')) ++p;
        int64_t x = 0;
        while (p < e && text_is_digit(buf[p])) ++p, ++x;
        if (x == 0) return false;
    }
    return p == e;
}

// the hifiasm id of a 7-field link: everything before the LAST ":<digit>-" (gfa.py _HIFIASM_ID, greedy); false without one
__device__ __forceinline__ bool trim_suffix(const uint8_t* buf, int64_t b, int64_t& e) {
    for (int64_t p = e - 3; p >= b; --p)
        if (buf[p] == ':' && text_is_digit(buf[p + 1]) && buf[p + 2] == '-') {
            e = p;
            return true;
        }
    return false;
}

__global__ __launch_bounds__(kLineThreads) void k_gfa_classify(const TextLineArgs a, int32_t* __restrict__ kinds, int64_t* __restrict__ rec) {
    const int64_t l = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    if (l >= a.L) return;
    int64_t r[kRec] = {-1, -1, -1, -1, 0, 0, -1, -1};
    int kind = kKindOther, code = kGfaOk;
    const int64_t f0 = a.ff[l], f1 = a.ff[l + 1], nf = f1 - f0;
    int64_t b = 0, e = 0;
    if (nf < 0 || f0 < 0 || f1 > a.F) {
        code = kGfaDescriptor;
    } else if (nf > 0) {
        if (!text_field(a, f0, b, e)) {
            code = kGfaDescriptor;
        } else if (e - b == 1 && a.buf[b] == 'S') {
            kind = kKindS;
            int64_t lb = 0, le = 0;
            if (nf < 4) {
                code = kGfaSFields;
            } else if (!text_field(a, f0 + 1, r[0], r[1]) || !text_field(a, f0 + 2, r[2], r[3]) || !text_field(a, f0 + 3, lb, le)) {
                code = kGfaDescriptor;
            } else {
                if (text_uint(a.buf, lb + 5 < le ? lb + 5 : le, le, r[4]) != kTextUintRead) code = kGfaLength;   // int(length[5:])
                r[5] = (r[3] - r[2] == 1 && a.buf[r[2]] == '*' ? 1 : 0) | (text_has_prefix(a.buf, r[0], r[1], "utg", 3) ? 2 : 0);
            }
        } else if (e - b == 1 && a.buf[b] == 'A') {
            kind = kKindA;   // whether it belongs to a segment is decided over the kinds of its neighbours (gfa.py)
            if (nf >= 5 && (!text_field(a, f0 + 4, r[0], r[1]) || !text_field(a, f0 + 3, r[2], r[3]))) code = kGfaDescriptor;
        } else if (e - b == 1 && a.buf[b] == 'L') {
            kind = kKindL;
            bool tagged = false;
            int64_t tb = -1, te = -1;
            for (int64_t k = f0 + 6; k < f1; ++k) {
                if (!text_field(a, k, b, e)) {
                    code = kGfaDescriptor;
                    break;
                }
                if (text_has_prefix(a.buf, b, e, "SI:f:", 5)) {
                    tagged = true;
                    tb = b + 5, te = e;   // the first one is the tag
                    break;
                }
            }
            int64_t kept[6] = {-1, -1, -1, -1, -1, -1}, count = 0;
            if (!tagged) {
                count = nf;
                for (int j = 0; j < 6 && j < nf; ++j) kept[j] = f0 + j;
            } else {
                for (int64_t k = f0; k < f1 && code == kGfaOk; ++k) {   // every SI:f: field is dropped, wherever it stands
                    if (!text_field(a, k, b, e)) code = kGfaDescriptor;
                    else if (!text_has_prefix(a.buf, b, e, "SI:f:", 5)) {
                        if (count < 6) kept[count] = k;
                        ++count;
                    }
                }
            }
            int64_t ob[2] = {0, 0}, oe[2] = {0, 0}, cb = 0, ce = 0;
            if (code == kGfaOk && (count < 6 || count > 8)) code = kGfaLFields;
            if (code == kGfaOk && !(text_field(a, kept[1], r[0], r[1]) && text_field(a, kept[3], r[2], r[3]) && text_field(a, kept[2], ob[0], oe[0]) &&
                                    text_field(a, kept[4], ob[1], oe[1]) && text_field(a, kept[5], cb, ce)))
                code = kGfaDescriptor;
            if (code == kGfaOk && count == 7 && !(trim_suffix(a.buf, r[0], r[1]) && trim_suffix(a.buf, r[2], r[3]))) code = kGfaSuffix;
            if (code == kGfaOk && text_uint(a.buf, cb, ce - 1, r[4]) != kTextUintRead) code = kGfaOverlap;   // int(cigar[:-1])
            if (code == kGfaOk) {
                const bool p1 = oe[0] - ob[0] == 1 && a.buf[ob[0]] == '+', m1 = oe[0] - ob[0] == 1 && a.buf[ob[0]] == '-';
                const bool p2 = oe[1] - ob[1] == 1 && a.buf[ob[1]] == '+', m2 = oe[1] - ob[1] == 1 && a.buf[ob[1]] == '-';
                r[5] = (p1 && p2) ? 0 : (p1 && m2) ? 1 : (m1 && p2) ? 2 : 3;
                if (tagged && r[4] != 0) {   // the host reads the tag of a link it keeps
                    if (te - tb > kTagMax) code = kGfaTagLong;
                    else if (!is_decimal(a.buf, tb, te)) code = kGfaTagText;
                }
                if (tagged) r[6] = tb, r[7] = te - tb;
            }
        }
    }
    kinds[l] = kind;
    a.err[l] = code;
#pragma unroll
    for (int j = 0; j < kRec; ++j) rec[l * kRec + j] = r[j];
    if (code != kGfaOk) atomicMin(a.first_bad, (int32_t)l);
}

struct TableArgs {
    const uint8_t* buf;
    int64_t n;
    const int64_t* seg_rec;    // [R, kRec] the S lines' records
    const int64_t* seg_line;   // [R] their line numbers
    int64_t R;
    int32_t* table;
    int64_t cap;               // a power of two > R
    int32_t* err;
    int64_t L;
    int32_t* first_bad;
};

__device__ __forceinline__ bool seg_name(const TableArgs& t, int64_t k, int64_t& b, int64_t& e) {
    if (k < 0 || k >= t.R) return false;
    b = t.seg_rec[k * kRec];
    e = t.seg_rec[k * kRec + 1];
    return b >= 0 && b <= e && e <= t.n;
}

__device__ __forceinline__ bool same_name(const TableArgs& t, int64_t k, int64_t b, int64_t e) {
    int64_t sb, se;
    if (!seg_name(t, k, sb, se) || se - sb != e - b) return false;
    for (int64_t j = 0; j < e - b; ++j)
        if (t.buf[sb + j] != t.buf[b + j]) return false;
    return true;
}

// A slot holds the SMALLEST S index of its name, whatever order the lanes arrive in: a lane that meets its own name lowers the
// slot with atomicMin and flags the larger of the two indices, so every S line of a repeated name but the first is flagged.
__global__ __launch_bounds__(kLineThreads) void k_gfa_names_insert(const TableArgs t) {
    const int64_t k = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    if (k >= t.R) return;
    int64_t b, e;
    if (!seg_name(t, k, b, e)) return;   // an S line without a name field: flagged by the classifier
    const uint32_t h = text_hash(t.buf, b, e);
    for (int64_t probe = 0; probe < t.cap; ++probe) {
        const int64_t slot = (h + probe) & (t.cap - 1);
        const int32_t prev = atomicCAS(&t.table[slot], -1, (int32_t)k);
        if (prev == -1) return;
        if (same_name(t, prev, b, e)) {
            const int32_t old = atomicMin(&t.table[slot], (int32_t)k);
            const int64_t loser = old > k ? old : k;
            const int64_t line = loser < t.R ? t.seg_line[loser] : -1;
            text_flag(t.err, t.first_bad, line, t.L, kGfaDuplicate);
            return;
        }
    }
    text_flag(t.err, t.first_bad, t.seg_line[k], t.L, kGfaTableFull);
}

// S index of the name in [b, e), or -1
__device__ __forceinline__ int64_t lookup(const TableArgs& t, int64_t b, int64_t e) {
    const uint32_t h = text_hash(t.buf, b, e);
    for (int64_t probe = 0; probe < t.cap; ++probe) {
        const int32_t k = t.table[(h + probe) & (t.cap - 1)];
        if (k == -1) return -1;
        if (same_name(t, k, b, e)) return k;
    }
    return -1;
}

__global__ __launch_bounds__(kLineThreads) void k_gfa_links(const TableArgs t, const int64_t* __restrict__ link_rec,
                                                            const int64_t* __restrict__ link_line, int64_t M, int64_t* __restrict__ ev_u,
                                                            int64_t* __restrict__ ev_v) {
    const int64_t m = (int64_t)blockIdx.x * kLineThreads + threadIdx.x;
    if (m >= M) return;
    int64_t u[2] = {-1, -1}, v[2] = {-1, -1};
    const int64_t line = link_line[m];
    const int64_t* r = link_rec + m * kRec;
    if (line >= 0 && line < t.L && t.err[line] == kGfaOk && r[4] != 0 && r[0] >= 0 && r[0] <= r[1] && r[1] <= t.n && r[2] >= 0 &&
        r[2] <= r[3] && r[3] <= t.n) {   // a zero overlap is dropped before its names are looked at (gfa.py:161-163)
        const int64_t a = lookup(t, r[0], r[1]), b = lookup(t, r[2], r[3]);
        if (a < 0 || b < 0) {
            text_flag(t.err, t.first_bad, line, t.L, kGfaUnknown);
        } else if (t.seg_line[a] > line || t.seg_line[b] > line) {
            text_flag(t.err, t.first_bad, line, t.L, kGfaLater);
        } else {
            const int64_t a0 = 2 * a, a1 = 2 * a + 1, b0 = 2 * b, b1 = 2 * b + 1;
            switch ((int)r[5]) {   // graph_parser.py:302-321
                case 0: u[0] = a0, v[0] = b0, u[1] = b1, v[1] = a1; break;
                case 1: u[0] = a0, v[0] = b1, u[1] = b0, v[1] = a1; break;
                case 2: u[0] = a1, v[0] = b0, u[1] = b1, v[1] = a0; break;
                default: u[0] = a1, v[0] = b1, u[1] = b0, v[1] = a0; break;
            }
        }
    }
    ev_u[2 * m] = u[0], ev_v[2 * m] = v[0];
    ev_u[2 * m + 1] = u[1], ev_v[2 * m + 1] = v[1];
}

struct PackArgs {
    const uint8_t* src;
    int64_t n;
    const int64_t* src_beg;   // [R] where item r starts in src
    const int64_t* out_off;   // [R+1] where it goes; its length is out_off[r+1] - out_off[r]
    int64_t R;
    uint8_t* out;
    int64_t total;
    int aligned;
};

// last index i in [lo, hi) with off[i] <= x; lo when there is none
__device__ __forceinline__ int64_t pack_last_le(const int64_t* off, int64_t lo, int64_t hi, int64_t x) {
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kPackThreads) void k_gfa_pack(const PackArgs a) {
    __shared__ int64_t range[2];   // items [r_lo, r_hi] reach into this tile
    const int64_t t0 = (int64_t)blockIdx.x * kPackTile;
    const int64_t t1 = (t0 + kPackTile < a.total ? t0 + kPackTile : a.total) - 1;
    if (threadIdx.x == 0) {
        range[0] = pack_last_le(a.out_off, 0, a.R, t0);
        range[1] = pack_last_le(a.out_off, range[0], a.R, t1);
    }
    __syncthreads();
    const int64_t r_lo = range[0], r_hi = range[1];
    for (int ch = 0; ch < kPackChunks; ++ch) {
        const int64_t o0 = t0 + ((int64_t)ch * kPackThreads + threadIdx.x) * 16;
        if (o0 >= a.total) break;
        int64_t r = pack_last_le(a.out_off, r_lo, r_hi + 1, o0);
        int64_t ob = a.out_off[r], oe = a.out_off[r + 1], sb = a.src_beg[r];
        uint32_t word[4] = {0, 0, 0, 0};
        uint32_t valid = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t o = o0 + j;
            if (o >= a.total) break;
            bool moved = false;
            while (o >= oe && r + 1 < a.R) {   // past this item: zero-length items are stepped over
                ++r;
                oe = a.out_off[r + 1];
                moved = true;
            }
            if (moved) ob = a.out_off[r], sb = a.src_beg[r];
            const int64_t p = sb + (o - ob);
            if (o < ob || o >= oe || p < 0 || p >= a.n) continue;   // only offsets that no scan produced get here
            word[j >> 2] |= (uint32_t)a.src[p] << (8 * (j & 3));
            valid |= 1u << j;
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

static inline int64_t blocks_for(int64_t items, int64_t per_block) { return (items + per_block - 1) / per_block; }

}  // namespace gnnome

extern "C" int gnnome_gfa_tile_sizes(int* tokenise_tile_host, int* pack_tile_host) {
    using namespace gnnome;
    GN_REQUIRE(tokenise_tile_host && pack_tile_host, "gfa_tile_sizes: null pointer");
    *tokenise_tile_host = (int)kTokTile;
    *pack_tile_host = (int)kPackTile;
    return GNNOME_OK;
}

extern "C" int gnnome_gfa_mark(const uint8_t* buf, int64_t num_bytes, uint8_t* marks, int64_t* bad_pos, void* stream) {
    using namespace gnnome;
    if (num_bytes == 0) return GNNOME_OK;
    GN_REQUIRE(num_bytes > 0, "gfa_mark: negative size");
    GN_REQUIRE(buf && marks && bad_pos, "gfa_mark: null pointer");
    const int64_t blocks = blocks_for(num_bytes, kTokTile);
    GN_REQUIRE(blocks < ((int64_t)1 << 31), "gfa_mark: %lld bytes are too many for one launch", (long long)num_bytes);
    const int aligned = (((uintptr_t)buf | (uintptr_t)marks) & 15) == 0;
    hipLaunchKernelGGL(k_gfa_mark, dim3((unsigned)blocks), dim3(kTokThreads), 0, (hipStream_t)stream, buf, num_bytes, marks,
                       (unsigned long long*)bad_pos, aligned);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_gfa_classify(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end,
                                   int64_t num_fields, const int64_t* line_field, int64_t num_lines, int32_t* kind, int64_t* rec,
                                   int32_t* err, int32_t* first_bad, void* stream) {
    using namespace gnnome;
    if (num_lines == 0) return GNNOME_OK;
    const TextLineArgs a{buf, num_bytes, field_start, field_end, num_fields, line_field, nullptr, num_lines, err, first_bad};
    const int rc = text_line_args_ok(a, "gfa_classify");
    if (rc != GNNOME_OK) return rc;
    GN_REQUIRE(kind && rec, "gfa_classify: null pointer");
    hipLaunchKernelGGL(k_gfa_classify, dim3((unsigned)blocks_for(num_lines, kLineThreads)), dim3(kLineThreads), 0, (hipStream_t)stream, a,
                       kind, rec);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

static int table_args_ok(const uint8_t* buf, int64_t num_bytes, const int64_t* seg_rec, const int64_t* seg_line, int64_t num_segments,
                         const int32_t* table, int64_t capacity, const int32_t* err, int64_t num_lines, const int32_t* first_bad,
                         const char* who) {
    using namespace gnnome;
    GN_REQUIRE(num_segments >= 0 && num_bytes >= 0 && num_lines >= 0, "%s: negative size", who);
    GN_REQUIRE(table && err && first_bad && (num_segments == 0 || (buf && seg_rec && seg_line)), "%s: null pointer", who);
    GN_REQUIRE(capacity > num_segments && capacity < ((int64_t)1 << 31) && (capacity & (capacity - 1)) == 0,
               "%s: capacity %lld must be a power of two above the %lld segments", who, (long long)capacity, (long long)num_segments);
    return GNNOME_OK;
}

extern "C" int gnnome_gfa_names_insert(const uint8_t* buf, int64_t num_bytes, const int64_t* seg_rec, const int64_t* seg_line,
                                       int64_t num_segments, int32_t* table, int64_t capacity, int32_t* err, int64_t num_lines,
                                       int32_t* first_bad, void* stream) {
    using namespace gnnome;
    const int rc = table_args_ok(buf, num_bytes, seg_rec, seg_line, num_segments, table, capacity, err, num_lines, first_bad,
                                 "gfa_names_insert");
    if (rc != GNNOME_OK) return rc;
    if (num_segments == 0) return GNNOME_OK;
    TableArgs t{buf, num_bytes, seg_rec, seg_line, num_segments, table, capacity, err, num_lines, first_bad};
    hipLaunchKernelGGL(k_gfa_names_insert, dim3((unsigned)blocks_for(num_segments, kLineThreads)), dim3(kLineThreads), 0,
                       (hipStream_t)stream, t);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_gfa_links(const uint8_t* buf, int64_t num_bytes, const int64_t* link_rec, const int64_t* link_line,
                                int64_t num_links, const int64_t* seg_rec, const int64_t* seg_line, int64_t num_segments,
                                const int32_t* table, int64_t capacity, int32_t* err, int64_t num_lines, int32_t* first_bad,
                                int64_t* event_u, int64_t* event_v, void* stream) {
    using namespace gnnome;
    const int rc = table_args_ok(buf, num_bytes, seg_rec, seg_line, num_segments, table, capacity, err, num_lines, first_bad, "gfa_links");
    if (rc != GNNOME_OK) return rc;
    if (num_links == 0) return GNNOME_OK;
    GN_REQUIRE(num_links > 0 && num_links < ((int64_t)1 << 30), "gfa_links: bad link count %lld", (long long)num_links);
    GN_REQUIRE(buf && link_rec && link_line && event_u && event_v, "gfa_links: null pointer");
    TableArgs t{buf, num_bytes, seg_rec, seg_line, num_segments, const_cast<int32_t*>(table), capacity, err, num_lines, first_bad};
    hipLaunchKernelGGL(k_gfa_links, dim3((unsigned)blocks_for(num_links, kLineThreads)), dim3(kLineThreads), 0, (hipStream_t)stream, t,
                       link_rec, link_line, num_links, event_u, event_v);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_gfa_pack(const uint8_t* src, int64_t src_bytes, const int64_t* src_beg, const int64_t* out_off, int64_t num_items,
                               uint8_t* out, int64_t out_bytes, void* stream) {
    using namespace gnnome;
    if (num_items == 0 || out_bytes == 0) return GNNOME_OK;
    GN_REQUIRE(num_items > 0 && out_bytes > 0 && src_bytes >= 0, "gfa_pack: negative size");
    GN_REQUIRE(src && src_beg && out_off && out, "gfa_pack: null pointer");
    const int64_t tiles = blocks_for(out_bytes, kPackTile);
    GN_REQUIRE(tiles < ((int64_t)1 << 31), "gfa_pack: output of %lld bytes too large", (long long)out_bytes);
    PackArgs a{src, src_bytes, src_beg, out_off, num_items, out, out_bytes, (int)(((uintptr_t)out & 15) == 0)};
    hipLaunchKernelGGL(k_gfa_pack, dim3((unsigned)tiles), dim3(kPackThreads), 0, (hipStream_t)stream, a);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
