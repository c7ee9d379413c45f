// What the device text readers (gfa_parse.hip, reads_parse.hip, maf_parse.hip) share: the descriptors gnnome_gfa_mark's marks are
// compacted into (gnnome_amd/textscan.py tokenise), the bounds-checked access to a field and a line, the line-flag protocol, plain
// digits with their cap, and the hash of the name tables.  Together they are all that stands between a malformed file and a read out
// of bounds, so each is stated here once; a reader adds its line kernel and its codes.
#pragma once
#include "common.h"

namespace gnnome {

constexpr int kTextMaxDigits = 18;   // what an int64 holds whatever the digits are

struct TextLineArgs {
    const uint8_t* buf;
    int64_t n;
    const int64_t* fs;   // first byte of every field
    const int64_t* fe;   // last byte of every field
    int64_t F;
    const int64_t* ff;   // [L+1] index of the first field at or after every line start; ff[L] = F
    const int64_t* ls;   // [L] first byte of every line; null for a reader that never calls text_line
    int64_t L;
    int32_t* err;        // [L] per-line code, 0 = nothing to report
    int32_t* first_bad;  // the smallest line that carries a code
};

// Code `code` on `line` unless an earlier stage left one (stages are separate launches: the first that objects names the reason), and
// the smallest flagged line kept with an integer atomicMin: the caller reads both after one synchronisation.
__device__ __forceinline__ void text_flag(int32_t* err, int32_t* first_bad, int64_t line, int64_t L, int code) {
    if (line < 0 || line >= L) return;
    atomicCAS(&err[line], 0, code);
    atomicMin(first_bad, (int32_t)line);
}

// field k as [b, e); false when the descriptors are not what gnnome_gfa_mark produces
__device__ __forceinline__ bool text_field(const TextLineArgs& a, int64_t k, int64_t& b, int64_t& e) {
    if (k < 0 || k >= a.F) return false;
    b = a.fs[k];
    e = a.fe[k] + 1;
    return b >= 0 && b < e && e <= a.n;
}

// fields [f0, f1) of line l, which starts at byte `start`; false when the line is outside the arrays
__device__ __forceinline__ bool text_line(const TextLineArgs& a, int64_t l, int64_t& start, int64_t& f0, int64_t& f1) {
    if (l < 0 || l >= a.L) return false;
    start = a.ls[l], f0 = a.ff[l], f1 = a.ff[l + 1];
    return start >= 0 && start < a.n && f0 >= 0 && f0 <= f1 && f1 <= a.F;
}

__device__ __forceinline__ bool text_is_digit(unsigned c) { return c >= '0' && c <= '9'; }

// [b, e) begins with the `len` bytes of p
__device__ __forceinline__ bool text_has_prefix(const uint8_t* buf, int64_t b, int64_t e, const char* p, int len) {
    if (e - b < len) return false;
    for (int j = 0; j < len; ++j)
        if (buf[b + j] != (uint8_t)p[j]) return false;
    return true;
}

// [b, e) is the `len` bytes of p
__device__ __forceinline__ bool text_equals(const uint8_t* buf, int64_t b, int64_t e, const char* p, int len) {
    return e - b == len && text_has_prefix(buf, b, e, p, len);
}

// Plain digits in [b, e) -> value.  Every byte is examined before the length is judged: "12x" followed by twenty digits is no number,
// not a long one (k_maf_lines reports the two apart and prefers the first).
enum { kTextUintRead = 0, kTextUintNoNumber = 1 /* empty, or a byte that is no digit */, kTextUintTooLong = 2 /* > kTextMaxDigits */ };
__device__ __forceinline__ int text_uint(const uint8_t* buf, int64_t b, int64_t e, int64_t& value) {
    if (e <= b) return kTextUintNoNumber;
    int64_t v = 0;
    for (int64_t p = b; p < e; ++p) {
        const unsigned c = buf[p];
        if (!text_is_digit(c)) return kTextUintNoNumber;
        if (p - b < kTextMaxDigits) v = v * 10 + (c - '0');
    }
    if (e - b > kTextMaxDigits) return kTextUintTooLong;
    value = v;
    return kTextUintRead;
}

// FNV-1a over p[b : e), the high bits folded down: the tables take the low bits
__device__ __forceinline__ uint32_t text_hash(const uint8_t* p, int64_t b, int64_t e) {
    uint32_t h = 2166136261u;
    for (int64_t q = b; q < e; ++q) h = (h ^ p[q]) * 16777619u;
    return h ^ (h >> 15);
}

// The host-side checks of a line kernel's descriptors (an entry point returns early on num_lines == 0 before it asks).  A null buf
// with no field is served: no line kernel reads a byte that no field or line start points at.
static inline int text_line_args_ok(const TextLineArgs& a, const char* who) {
    GN_REQUIRE(a.L > 0 && a.F >= 0 && a.n >= 0, "%s: negative size", who);
    GN_REQUIRE(a.L < ((int64_t)1 << 31) && a.F < ((int64_t)1 << 31), "%s: line and field counts are int32", who);
    GN_REQUIRE(a.ff && a.err && a.first_bad && (a.F == 0 || (a.buf && a.fs && a.fe)), "%s: null pointer", who);
    return GNNOME_OK;
}

}  // namespace gnnome
