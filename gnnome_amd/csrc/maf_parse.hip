// pbsim3 MAF files on the device (generate_data.py:43-60, change_description_pbsim: start and size from the reference line of every
// alignment block, the strand from the read line; gnnome_amd/maf.py is the statement here).
//
//   (gnnome_amd/textscan.py tokenise: gnnome_gfa_mark marks the bytes - a 50 kb alignment text is two marks - and torch operators compact
//    the marks into text_fields.h's descriptors; the scans that group the s lines under the nearest a line are torch operators in
//    gnnome_amd/maf.py; the wanted names go through gnnome_reads_names_insert / gnnome_reads_match as they are: textscan.lookup_names)
//   gnnome_maf_lines        one thread per line: blank / comment / a / s / other; an s line's name, start, size, strand and text range
//   gnnome_maf_text_check   one wavefront per s line: the bytes of its text that are not '-' counted and compared with its size - the
//                           only pass over the alignment texts
//
// Every byte range is checked against the buffer before it is read; a line this path does not serve gets a per-line code and the
// smallest such line is kept with an integer atomicMin (gnnome_amd/maf.py _DECLINED names the codes).  No float is produced here.
#include "text_fields.h"   // the line descriptors, fields, digits and the line flag: shared with the other text readers

namespace gnnome {

constexpr int kMafThreads = 256;
constexpr int kMafRec = 8;   // int64 words per s-line record

// per-line codes (gnnome_amd/maf.py _DECLINED)
enum { kMafOk = 0, kMafFields = 1, kMafNumber = 2, kMafDigits = 3, kMafStrand = 4, kMafOtherLine = 5, kMafSize = 9 };
enum { kMafBlank = 0, kMafComment = 1, kMafA = 2, kMafS = 3, kMafOther = 4 };

__global__ __launch_bounds__(kMafThreads) void k_maf_lines(const TextLineArgs a, int32_t* __restrict__ kind, int64_t* __restrict__ rec) {
    const int64_t l = (int64_t)blockIdx.x * kMafThreads + threadIdx.x;
    if (l >= a.L) return;
    int64_t r[kMafRec] = {0, 0, 0, 0, 0, 0, 0, 0};
    int k = kMafBlank, code = kMafOk;
    const int64_t f0 = a.ff[l], f1 = a.ff[l + 1];
    int64_t b = 0, e = 0;
    if (f0 >= 0 && f0 < f1 && f1 <= a.F) {
        if (!text_field(a, f0, b, e)) {
            k = kMafOther, code = kMafOtherLine;
        } else if (a.buf[b] == '#' || text_equals(a.buf, b, e, "track", 5)) {
            k = kMafComment;
        } else if (text_equals(a.buf, b, e, "a", 1)) {
            k = kMafA;
        } else if (text_equals(a.buf, b, e, "s", 1)) {
            k = kMafS;
            int64_t nb[7], ne[7];
            bool ok = f1 - f0 == 7;
            for (int j = 0; ok && j < 7; ++j) ok = text_field(a, f0 + j, nb[j], ne[j]);
            if (!ok) {
                code = kMafFields;
            } else {
                int64_t start = 0, size = 0, src_size = 0;
                const int rc[3] = {text_uint(a.buf, nb[2], ne[2], start), text_uint(a.buf, nb[3], ne[3], size),
                                   text_uint(a.buf, nb[5], ne[5], src_size)};
                const unsigned sign = a.buf[nb[4]];
                if (rc[0] == kTextUintNoNumber || rc[1] == kTextUintNoNumber || rc[2] == kTextUintNoNumber) code = kMafNumber;
                else if (ne[4] - nb[4] != 1 || (sign != '+' && sign != '-')) code = kMafStrand;
                else if (rc[0] != kTextUintRead || rc[1] != kTextUintRead || rc[2] != kTextUintRead) code = kMafDigits;
                if (code == kMafOk) {
                    r[0] = nb[1], r[1] = ne[1], r[2] = start, r[3] = size, r[4] = sign == '+' ? 1 : -1, r[5] = nb[6], r[6] = ne[6], r[7] = 1;
                }
            }
        } else {
            k = kMafOther, code = kMafOtherLine;
        }
    }
    if (code != kMafOk) text_flag(a.err, a.first_bad, l, a.L, code);
    kind[l] = k;
#pragma unroll
    for (int j = 0; j < kMafRec; ++j) rec[l * kMafRec + j] = r[j];
}

// the bytes of a 32-bit word that are '-': exact (no carry crosses a byte), one popcount
__device__ __forceinline__ int maf_dashes(uint32_t w) {
    const uint32_t x = w ^ 0x2d2d2d2du;
    const uint32_t t = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
    return __popc(t);
}

// One wavefront per s-line record: the text [r[5], r[6]) minus its '-' bytes must have r[3] bytes.  Byte loads up to the first 16-byte
// aligned address and behind the last, 16-byte loads between, every load inside [text_begin, text_end), which is inside [0, n).
__global__ __launch_bounds__(kMafThreads) void k_maf_text_check(const uint8_t* __restrict__ buf, int64_t n, const int64_t* __restrict__ rec,
                                                                const int64_t* __restrict__ rec_line, int64_t S, int32_t* err, int64_t L,
                                                                int32_t* first_bad) {
    const int64_t s = (int64_t)blockIdx.x * (kMafThreads / kWave) + threadIdx.x / kWave;   // uniform over the wavefront
    const int lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    const int64_t* r = rec + s * kMafRec;
    const int64_t tb = r[5], te = r[6];
    if (r[7] != 1 || tb < 0 || tb > te || te > n) return;
    const uint64_t addr = (uint64_t)(uintptr_t)(buf + tb);
    int64_t head = (int64_t)((16 - (addr & 15)) & 15);
    if (head > te - tb) head = te - tb;
    const int64_t body = tb + head;                     // 16-byte aligned, or te
    const int64_t chunks = (te - body) >> 4;
    const int64_t tail = body + (chunks << 4);
    int64_t dashes = 0;
    if (lane < head) dashes += buf[tb + lane] == '-';                                    // head < 16
    if (lane >= 16 && tail + (lane - 16) < te) dashes += buf[tail + (lane - 16)] == '-';   // te - tail < 16
    for (int64_t c = lane; c < chunks; c += kWave) {
        const uint4 v = *reinterpret_cast<const uint4*>(buf + body + (c << 4));
        dashes += maf_dashes(v.x) + maf_dashes(v.y) + maf_dashes(v.z) + maf_dashes(v.w);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) dashes += __shfl_xor(dashes, o);
    if (lane == 0 && (te - tb) - dashes != r[3]) text_flag(err, first_bad, rec_line[s], L, kMafSize);
}

}  // namespace gnnome

extern "C" int gnnome_maf_lines(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end, int64_t num_fields,
                                const int64_t* line_field, int64_t num_lines, int32_t* kind, int64_t* rec, int32_t* err, int32_t* first_bad,
                                void* stream) {
    using namespace gnnome;
    if (num_lines == 0) return GNNOME_OK;
    const TextLineArgs a{buf, num_bytes, field_start, field_end, num_fields, line_field, nullptr, num_lines, err, first_bad};
    const int rc = text_line_args_ok(a, "maf_lines");
    if (rc != GNNOME_OK) return rc;
    GN_REQUIRE(kind && rec, "maf_lines: null pointer");
    hipLaunchKernelGGL(k_maf_lines, dim3((unsigned)((num_lines + kMafThreads - 1) / kMafThreads)), dim3(kMafThreads), 0, (hipStream_t)stream, a,
                       kind, rec);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_maf_text_check(const uint8_t* buf, int64_t num_bytes, const int64_t* rec, const int64_t* rec_line, int64_t num_records,
                                     int32_t* err, int64_t num_lines, int32_t* first_bad, void* stream) {
    using namespace gnnome;
    if (num_records == 0) return GNNOME_OK;
    GN_REQUIRE(num_records > 0 && num_records <= num_lines && num_lines < ((int64_t)1 << 31) && num_bytes > 0, "maf_text_check: bad sizes");
    GN_REQUIRE(buf && rec && rec_line && err && first_bad, "maf_text_check: null pointer");
    constexpr int per_block = kMafThreads / kWave;
    hipLaunchKernelGGL(k_maf_text_check, dim3((unsigned)((num_records + per_block - 1) / per_block)), dim3(kMafThreads), 0, (hipStream_t)stream,
                       buf, num_bytes, rec, rec_line, num_records, err, num_lines, first_bad);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
