// FASTA / FASTQ reads files on the device (graph_parser.py:121-136 the titles, :213-272 the positions in them, :341-366 the sequences;
// gnnome_amd/contigs.py _records / read_sequences / read_titles and gfa.py _annotation are their statement here).
//
//   (gnnome_amd/textscan.py tokenise: gnnome_gfa_mark marks the bytes, torch operators compact the marks into text_fields.h's descriptors)
//   gnnome_reads_records_fasta   one thread per line: header ('>' as the line's first byte) or sequence line; id, title, sequence ranges
//   gnnome_reads_records_fastq   one thread per record over the non-blank lines: the four-line form checked, id, title, sequence ranges
//   gnnome_reads_names_insert    the wanted names into an open-addressing table; equal names share a slot
//   gnnome_reads_match           every record looks its id up and raises match[slot] to its index: the last record of an id wins
//   gnnome_reads_annotations     one thread per matched record: the first strand= / start= / end= / chr= of its title, as re.search
//   (the unitig combination, the pack items and the scans are torch operators in gnnome_amd/reads.py; gnnome_gfa_pack copies the bases)
//
// Why the four-line form is enough for FASTQ.  The host (contigs._records, a restatement of Biopython's FastqGeneralIterator) reads a
// header, then sequence lines until one starts with '+', then quality lines until it has as many characters as bases, skipping blank
// lines throughout.  Let the non-blank lines be n_0, n_1, ... and assume for every k: n_4k starts with '@'; n_4k+1 does not start with
// '+' and is one field of b > 0 bytes; n_4k+2 starts with '+'; n_4k+3 is one field of b bytes; and the count is a multiple of 4.  By
// induction the host stands at n_4k when it looks for a header: it takes n_4k+1 as sequence (blank lines add nothing), stops at n_4k+2
// because that is the first later line starting with '+', and then needs b > 0 quality characters, so it must take the next non-blank
// line n_4k+3 WHATEVER its first byte is - a quality line beginning with '@' or '+' is consumed as quality and never seen as a header
// or separator - and that line has exactly b, so the host stops there and stands at n_4k+4.  Both sides therefore yield the same
// (title, sequence) per record.  Where one condition fails the host either raises or regroups the lines (multi-line records, an empty
// sequence whose quality line becomes the next header): those files are declined, naming the first line that breaks the form.
//
// Every byte range is checked against the buffer before it is read; a line this path does not serve gets a per-line code and the
// smallest such line is kept with an integer atomicMin (gnnome_amd/reads.py _DECLINED names the codes).  No float is produced here.
#include "text_fields.h"   // the line descriptors, fields, lines, digits, the line flag and the name hash: shared with the other text readers

namespace gnnome {

constexpr int kReadsThreads = 256;

// per-line codes (gnnome_amd/reads.py _DECLINED)
enum { kReadsOk = 0, kReadsFields = 1, kReadsFourLine = 2, kReadsDigits = 3, kReadsChrMixed = 4 };
enum { kLineBlank = 0, kLineHeader = 1, kLineSequence = 2 };

// A header line that starts at `start` with its marker byte: id = the first whitespace-separated token of line[1:], title =
// line[1:].rstrip(), both as [b, e).  out[0..3] = id_b, id_e, title_b, title_e.
__device__ __forceinline__ bool rd_header(const TextLineArgs& a, int64_t start, int64_t f0, int64_t f1, int64_t* out) {
    int64_t b = 0, e = 0, lb = 0, le = 0;
    if (f1 <= f0 || !text_field(a, f0, b, e) || b != start || !text_field(a, f1 - 1, lb, le)) return false;
    out[2] = start + 1;
    out[3] = le > start + 1 ? le : start + 1;
    if (e - b > 1) {                                   // ">id ..."
        out[0] = start + 1, out[1] = e;
    } else if (f1 - f0 >= 2) {                         // "> id ...": the marker alone is the first field
        if (!text_field(a, f0 + 1, out[0], out[1])) return false;
    } else {
        out[0] = out[1] = start + 1;                   // nothing behind the marker: the empty id
    }
    return true;
}

__global__ __launch_bounds__(kReadsThreads) void k_reads_records_fasta(const TextLineArgs a, const int64_t* __restrict__ first_header,
                                                                       int32_t* __restrict__ kind, int64_t* __restrict__ rec) {
    const int64_t l = (int64_t)blockIdx.x * kReadsThreads + threadIdx.x;
    if (l >= a.L) return;
    int64_t r[4] = {0, 0, 0, 0};
    int k = kLineBlank;
    int64_t start = 0, f0 = 0, f1 = 0;
    if (text_line(a, l, start, f0, f1) && f1 > f0) {
        if (a.buf[start] == '>') {
            if (rd_header(a, start, f0, f1, r)) k = kLineHeader;
        } else if (text_field(a, f0, r[0], r[1])) {
            k = kLineSequence;
            if (f1 - f0 > 1 && l > *first_header) text_flag(a.err, a.first_bad, l, a.L, kReadsFields);   // above the first header: no record's
        }
    }
    kind[l] = k;
#pragma unroll
    for (int j = 0; j < 4; ++j) rec[l * 4 + j] = r[j];
}

__global__ __launch_bounds__(kReadsThreads) void k_reads_records_fastq(const TextLineArgs a, const int64_t* __restrict__ nonblank, int64_t Q,
                                                                       int64_t K, int64_t* __restrict__ rec) {
    const int64_t k = (int64_t)blockIdx.x * kReadsThreads + threadIdx.x;
    if (k >= K) return;
    int64_t r[6] = {0, 0, 0, 0, 0, 0};
    int64_t bad = -1;   // the first line of this record that breaks the form
    const int64_t l0 = nonblank[4 * k];
    if (4 * k + 3 >= Q) {
        bad = l0;       // the file ends inside this record
    } else {
        int64_t line[4], start[4], f0[4], f1[4];
        bool ok = true;
        for (int j = 0; j < 4; ++j) {
            line[j] = nonblank[4 * k + j];
            ok = ok && text_line(a, line[j], start[j], f0[j], f1[j]) && f1[j] > f0[j];
        }
        int64_t qb = 0, qe = 0;
        if (!ok) bad = l0;
        else if (a.buf[start[0]] != '@' || !rd_header(a, start[0], f0[0], f1[0], r)) bad = line[0];
        else if (a.buf[start[1]] == '+' || !text_field(a, f0[1], r[4], r[5])) bad = line[1];
        else if (f1[1] - f0[1] != 1) bad = -2 - line[1];
        else if (a.buf[start[2]] != '+') bad = line[2];
        else if (!text_field(a, f0[3], qb, qe)) bad = line[3];
        else if (f1[3] - f0[3] != 1) bad = -2 - line[3];
        else if (qe - qb != r[5] - r[4]) bad = line[3];
    }
    if (bad <= -2) text_flag(a.err, a.first_bad, -2 - bad, a.L, kReadsFields);
    else if (bad >= 0) text_flag(a.err, a.first_bad, bad, a.L, kReadsFourLine);
    if (bad != -1) r[0] = r[1] = r[2] = r[3] = r[4] = r[5] = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) rec[k * 6 + j] = r[j];
}

struct NamesArgs {
    const uint8_t* names;      // the wanted names, one after the other
    int64_t names_bytes;
    const int64_t* name_off;   // [R+1] name r = names[name_off[r] : name_off[r+1]]
    int64_t R;
    int32_t* table;
    int64_t cap;               // a power of two; fewer slots than distinct names: the insert reports it
};

__device__ __forceinline__ bool rd_name(const NamesArgs& t, int64_t r, int64_t& b, int64_t& e) {
    if (r < 0 || r >= t.R) return false;
    b = t.name_off[r], e = t.name_off[r + 1];
    return b >= 0 && b <= e && e <= t.names_bytes;
}

// name r against src[b : e) - length and bytes, across two buffers
__device__ __forceinline__ bool rd_same(const NamesArgs& t, int64_t r, const uint8_t* src, int64_t b, int64_t e) {
    int64_t nb, ne;
    if (!rd_name(t, r, nb, ne) || ne - nb != e - b) return false;
    for (int64_t j = 0; j < e - b; ++j)
        if (t.names[nb + j] != src[b + j]) return false;
    return true;
}

// The slot of the name in names[b : e): an empty slot claimed for index r, or the slot that already holds a name with these bytes
// (a repeated wanted name is legal - two nodes may name one read - and shares its slot); -1 when the table has no room.  Which of the
// equal names' indices a slot holds depends on arrival order and changes nothing: only the bytes behind it are ever compared.
// Kept out of line on purpose: with this loop inlined into the kernel (a break under `claimed || same bytes`), the code hipcc generated
// for gfx950 lost the slot on the same-bytes path - every repeated name came back as -1 on the MI355X - while this form returns it.
__device__ __noinline__ int32_t rd_claim(const NamesArgs& t, int64_t r, int64_t b, int64_t e) {
    const uint32_t h = text_hash(t.names, b, e);
    for (int64_t probe = 0; probe < t.cap; ++probe) {
        const int64_t slot = (h + probe) & (t.cap - 1);
        const int32_t prev = atomicCAS(&t.table[slot], -1, (int32_t)r);
        if (prev == -1) return (int32_t)slot;
        if (rd_same(t, prev, t.names, b, e)) return (int32_t)slot;
    }
    return -1;
}

__global__ __launch_bounds__(kReadsThreads) void k_reads_names_insert(const NamesArgs t, int32_t* __restrict__ slot_of, int32_t* full) {
    const int64_t r = (int64_t)blockIdx.x * kReadsThreads + threadIdx.x;
    if (r >= t.R) return;
    int64_t b = 0, e = 0;
    const int32_t found = rd_name(t, r, b, e) ? rd_claim(t, r, b, e) : -1;
    slot_of[r] = found;
    if (found < 0) atomicMax(full, 1);
}

__global__ __launch_bounds__(kReadsThreads) void k_reads_match(const NamesArgs t, const uint8_t* __restrict__ buf, int64_t n,
                                                               const int64_t* __restrict__ rec, int stride, int64_t K,
                                                               int32_t* __restrict__ match) {
    const int64_t k = (int64_t)blockIdx.x * kReadsThreads + threadIdx.x;
    if (k >= K) return;
    const int64_t b = rec[k * stride], e = rec[k * stride + 1];
    if (b < 0 || b > e || e > n) return;
    const uint32_t h = text_hash(buf, b, e);
    for (int64_t probe = 0; probe < t.cap; ++probe) {
        const int64_t slot = (h + probe) & (t.cap - 1);
        const int32_t r = t.table[slot];
        if (r == -1) return;
        if (rd_same(t, r, buf, b, e)) {
            atomicMax(&match[slot], (int32_t)k);   // a repeated id keeps its LAST record, whatever order the lanes arrive in
            return;
        }
    }
}

// first p >= from with buf[p : p+len) == key and p + len < e (one more byte must follow: every pattern captures at least one); -1
__device__ __forceinline__ int64_t rd_find(const uint8_t* buf, int64_t from, int64_t e, const char* key, int len) {
    for (int64_t p = from; p + len < e; ++p) {
        int j = 0;
        while (j < len && buf[p + j] == (uint8_t)key[j]) ++j;
        if (j == len) return p;
    }
    return -1;
}

__device__ __forceinline__ bool rd_is_chr(unsigned c) { return text_is_digit(c) || c == 'X' || c == 'Y' || c == 'M'; }

// key followed by a run of digits: the first such place in [b, e), as re.search(key + r"(\d+)") finds it.  0 found, 1 missing, 2 the
// run has more than 18 digits
__device__ __forceinline__ int rd_number(const uint8_t* buf, int64_t b, int64_t e, const char* key, int len, int64_t& value) {
    for (int64_t from = b;;) {
        const int64_t p = rd_find(buf, from, e, key, len);
        if (p < 0) return 1;
        int64_t q = p + len;
        if (!text_is_digit(buf[q])) {
            from = p + 1;
            continue;
        }
        int64_t v = 0;
        int digits = 0;
        for (; q < e && text_is_digit(buf[q]); ++q) {
            if (++digits > kTextMaxDigits) return 2;
            v = v * 10 + (buf[q] - '0');
        }
        value = v;
        return 0;
    }
}

__global__ __launch_bounds__(kReadsThreads) void k_reads_annotations(const uint8_t* __restrict__ buf, int64_t n, const int64_t* __restrict__ rec,
                                                                     int stride, int64_t K, const int64_t* __restrict__ rec_line,
                                                                     const int64_t* __restrict__ which, int64_t M, int64_t* __restrict__ ann,
                                                                     int32_t* __restrict__ missing, int32_t* err, int64_t L, int32_t* first_bad) {
    const int64_t m = (int64_t)blockIdx.x * kReadsThreads + threadIdx.x;
    if (m >= M) return;
    int64_t v[4] = {0, 0, 0, 0};
    int miss = 15, code = kReadsOk;
    const int64_t k = which[m];
    if (k >= 0 && k < K) {
        const int64_t b = rec[k * stride + 2], e = rec[k * stride + 3];
        if (b >= 0 && b <= e && e <= n) {
            miss = 0;
            int64_t p = -1;                                                     // strand=(\+|\-)
            for (int64_t from = b; (p = rd_find(buf, from, e, "strand=", 7)) >= 0; from = p + 1)
                if (buf[p + 7] == '+' || buf[p + 7] == '-') break;
            if (p < 0) miss |= 1;
            else v[0] = buf[p + 7] == '+' ? 1 : -1;
            int rc = rd_number(buf, b, e, "start=", 6, v[1]);                   // start=(\d+)
            if (rc == 1) miss |= 2;
            if (rc == 2) code = kReadsDigits;
            rc = rd_number(buf, b, e, "end=", 4, v[2]);                         // end=(\d+)
            if (rc == 1) miss |= 4;
            if (rc == 2) code = kReadsDigits;
            for (int64_t from = b; (p = rd_find(buf, from, e, "chr=", 4)) >= 0; from = p + 1)   // chr=([0-9XYM]+), greedy
                if (rd_is_chr(buf[p + 4])) break;
            if (p < 0) {
                miss |= 8;
            } else {
                int64_t q = p + 4, value = 0;
                int digits = 0, letters = 0;
                for (; q < e && rd_is_chr(buf[q]); ++q) {
                    if (text_is_digit(buf[q])) {
                        if (++digits <= kTextMaxDigits) value = value * 10 + (buf[q] - '0');
                    } else {
                        ++letters;
                    }
                }
                const unsigned c = buf[p + 4];
                if (letters == 1 && digits == 0) v[3] = c == 'X' ? -1 : c == 'Y' ? -2 : -3;
                else if (letters != 0) code = kReadsChrMixed;      // the host's int() raises on it
                else if (digits > kTextMaxDigits) code = kReadsDigits;
                else v[3] = value;
            }
            if (code != kReadsOk) text_flag(err, first_bad, rec_line[k], L, code);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) ann[m * 4 + j] = v[j];
    missing[m] = miss;
}

static inline int64_t reads_blocks(int64_t items) { return (items + kReadsThreads - 1) / kReadsThreads; }

static int reads_names_ok(const uint8_t* names, int64_t names_bytes, const int64_t* name_off, int64_t num_names, const int32_t* table,
                          int64_t capacity, const char* who) {
    GN_REQUIRE(num_names >= 0 && names_bytes >= 0, "%s: negative size", who);
    GN_REQUIRE(table && name_off && (names_bytes == 0 || names), "%s: null pointer", who);
    GN_REQUIRE(capacity >= 2 && capacity < ((int64_t)1 << 31) && (capacity & (capacity - 1)) == 0 && num_names < ((int64_t)1 << 31),
               "%s: capacity %lld must be a power of two (%lld names)", who, (long long)capacity, (long long)num_names);
    return GNNOME_OK;
}

}  // namespace gnnome

extern "C" int gnnome_reads_records_fasta(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end,
                                          int64_t num_fields, const int64_t* line_field, const int64_t* line_start, int64_t num_lines,
                                          const int64_t* first_header, int32_t* kind, int64_t* rec, int32_t* err, int32_t* first_bad,
                                          void* stream) {
    using namespace gnnome;
    if (num_lines == 0) return GNNOME_OK;
    const TextLineArgs a{buf, num_bytes, field_start, field_end, num_fields, line_field, line_start, num_lines, err, first_bad};
    const int rc = text_line_args_ok(a, "reads_records_fasta");
    if (rc != GNNOME_OK) return rc;
    GN_REQUIRE(line_start && first_header && kind && rec, "reads_records_fasta: null pointer");
    hipLaunchKernelGGL(k_reads_records_fasta, dim3((unsigned)reads_blocks(num_lines)), dim3(kReadsThreads), 0, (hipStream_t)stream, a,
                       first_header, kind, rec);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_reads_records_fastq(const uint8_t* buf, int64_t num_bytes, const int64_t* field_start, const int64_t* field_end,
                                          int64_t num_fields, const int64_t* line_field, const int64_t* line_start, int64_t num_lines,
                                          const int64_t* nonblank, int64_t num_nonblank, int64_t* rec, int32_t* err, int32_t* first_bad,
                                          void* stream) {
    using namespace gnnome;
    if (num_nonblank == 0) return GNNOME_OK;
    const TextLineArgs a{buf, num_bytes, field_start, field_end, num_fields, line_field, line_start, num_lines, err, first_bad};
    const int rc = text_line_args_ok(a, "reads_records_fastq");
    if (rc != GNNOME_OK) return rc;
    GN_REQUIRE(num_nonblank > 0 && num_nonblank <= num_lines, "reads_records_fastq: %lld non-blank lines of %lld", (long long)num_nonblank,
               (long long)num_lines);
    GN_REQUIRE(line_start && nonblank && rec, "reads_records_fastq: null pointer");
    const int64_t K = (num_nonblank + 3) / 4;
    hipLaunchKernelGGL(k_reads_records_fastq, dim3((unsigned)reads_blocks(K)), dim3(kReadsThreads), 0, (hipStream_t)stream, a, nonblank,
                       num_nonblank, K, rec);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_reads_names_insert(const uint8_t* names, int64_t names_bytes, const int64_t* name_off, int64_t num_names, int32_t* table,
                                         int64_t capacity, int32_t* slot_of, int32_t* full, void* stream) {
    using namespace gnnome;
    const int rc = reads_names_ok(names, names_bytes, name_off, num_names, table, capacity, "reads_names_insert");
    if (rc != GNNOME_OK) return rc;
    if (num_names == 0) return GNNOME_OK;
    GN_REQUIRE(slot_of && full, "reads_names_insert: null pointer");
    NamesArgs t{names, names_bytes, name_off, num_names, table, capacity};
    hipLaunchKernelGGL(k_reads_names_insert, dim3((unsigned)reads_blocks(num_names)), dim3(kReadsThreads), 0, (hipStream_t)stream, t, slot_of,
                       full);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_reads_match(const uint8_t* buf, int64_t num_bytes, const int64_t* rec, int rec_stride, int64_t num_records,
                                  const uint8_t* names, int64_t names_bytes, const int64_t* name_off, int64_t num_names, const int32_t* table,
                                  int64_t capacity, int32_t* match, void* stream) {
    using namespace gnnome;
    const int rc = reads_names_ok(names, names_bytes, name_off, num_names, table, capacity, "reads_match");
    if (rc != GNNOME_OK) return rc;
    if (num_records == 0 || num_names == 0) return GNNOME_OK;
    GN_REQUIRE(num_records > 0 && num_records < ((int64_t)1 << 31) && num_bytes >= 0, "reads_match: bad record count %lld",
               (long long)num_records);
    GN_REQUIRE(rec_stride >= 2 && rec_stride <= 8, "reads_match: rec_stride=%d", rec_stride);
    GN_REQUIRE(rec && match && (num_bytes == 0 || buf), "reads_match: null pointer");
    NamesArgs t{names, names_bytes, name_off, num_names, const_cast<int32_t*>(table), capacity};
    hipLaunchKernelGGL(k_reads_match, dim3((unsigned)reads_blocks(num_records)), dim3(kReadsThreads), 0, (hipStream_t)stream, t, buf, num_bytes,
                       rec, rec_stride, num_records, match);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_reads_annotations(const uint8_t* buf, int64_t num_bytes, const int64_t* rec, int rec_stride, int64_t num_records,
                                        const int64_t* rec_line, const int64_t* which, int64_t num_which, int64_t* ann, int32_t* missing,
                                        int32_t* err, int64_t num_lines, int32_t* first_bad, void* stream) {
    using namespace gnnome;
    if (num_which == 0) return GNNOME_OK;
    GN_REQUIRE(num_which > 0 && num_which < ((int64_t)1 << 31) && num_records >= 0 && num_bytes >= 0 && num_lines >= 0,
               "reads_annotations: bad sizes");
    GN_REQUIRE(rec_stride >= 4 && rec_stride <= 8, "reads_annotations: rec_stride=%d", rec_stride);
    GN_REQUIRE(which && ann && missing && err && first_bad && (num_records == 0 || (buf && rec && rec_line)), "reads_annotations: null pointer");
    hipLaunchKernelGGL(k_reads_annotations, dim3((unsigned)reads_blocks(num_which)), dim3(kReadsThreads), 0, (hipStream_t)stream, buf, num_bytes,
                       rec, rec_stride, num_records, rec_line, which, num_which, ann, missing, err, num_lines, first_bad);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
