// Reads -> overlaps: minimizer sketch, seed pairs, banded chains and their classification (the step graph_dataset.py:76-186 leaves to
// hifiasm / raven).  tests/overlap_graph_statement.py states every stage; everything here is integer arithmetic, every output slot has one
// writer at a position that a count and an exclusive scan fixed before it was written, so the bytes do not depend on the grid or on timing.
//
// The hash of a k-mer (k <= 31): its code is the smaller of the forward and the reverse-complement 2k-bit codes (A, C, G, T = 0 .. 3 in either
// case, first base most significant; equal codes - palindromes - and k-mers over any other byte are invalid), mixed by Thomas Wang's 64-bit
// integer hash with every step masked to m = 2^(2k) - 1, which keeps it a bijection of [0, m]:
//     x = (~x + (x << 21)) & m;  x ^= x >> 24;  x = (x + (x << 3) + (x << 8)) & m;  x ^= x >> 14;
//     x = (x + (x << 2) + (x << 4)) & m;  x ^= x >> 28;  x = (x + (x << 31)) & m
//
// gnnome_sketch_reads   one workgroup per tile of kSkTile windows of one read (window s = the k-mer starts s .. s + w - 1, all inside the read).
//   The tile's bases, the one base before them and the k + w - 2 after, are loaded once as aligned dwords into LDS; a thread packs 16
//   bases into 2-bit codes and a bad-byte mask; a thread rolls the forward and reverse codes over 16 consecutive k-mer starts after a
//   (k - 1)-base warm-up and leaves the hashes (all ones = invalid) in LDS, padded by one slot per 16 so that the 16-apart stores spread
//   over the banks; a thread per window takes the leftmost minimum of its w hashes.  The leftmost minimum never moves left from one
//   window to the next, so a window emits its minimum iff it differs from the previous window's: every position once, in rising order.
//   A count launch leaves the tile totals, a scan makes them bases, the write launch repeats the work and stores at base + rank.
// gnnome_seed_pairs     on the seeds sorted stably by hash (ties stay in (read, pos) order).  Seed i pairs with every EARLIER seed of its
//   bucket that lies in another read: as a bucket is ordered by read these are the bucket's seeds before the run of i's own read, so the
//   count is (start of that run) - (start of the bucket), found by three binary searches of at most log2(max_occ + 1) steps around i; a
//   bucket of more than max_occ seeds counts 0.  After the scan one thread per record finds its seed by binary search over the bases and
//   its partner by offset.  A record is two sort keys: (a << 32 | b << 1 | rel) and ((d + 2^30) << 32 | pa).
// gnnome_chain_overlaps one wavefront per run of equal (a, b, rel), 64 records per pass in (d, pa) order.  A band takes the records whose
//   d is at most `band` above its first; they are a prefix of what is left of the pass, found with one ballot, counted with a popcount and
//   reduced with two butterflies - min and max of (pa << 32 | d + 2^30).  The open band (first d, count, min, max) and the best closed one
//   are carried from pass to pass in wave-uniform registers.  The classification of the best band is done by the same wavefront.
#include "common.h"

namespace gnnome {

typedef unsigned long long u64;

constexpr int kSkThreads = 256;
constexpr int kSkWaves = kSkThreads / kWave;
constexpr int kSkRun = 16;                                  // k-mer starts per thread and pass: one dword of 2-bit codes
constexpr int kSkTile = kSkThreads * kSkRun;                // windows per tile
constexpr int kSkMaxHalo = 256;                             // k + w - 1 <= kSkMaxHalo
constexpr int kSkRuns = (kSkTile + kSkMaxHalo) / kSkRun;    // 16-position runs that can hold a k-mer start the tile looks at
constexpr int kSkGroups = kSkRuns + 2;                      // 16-base groups: a run reads its own group and the two after it
constexpr int kSkRawWords = 4 * kSkGroups + 4;
constexpr int kSkHashSlots = kSkRuns * (kSkRun + 1);
constexpr int kSkChunks = kSkTile / kSkThreads;
constexpr u64 kSkInvalid = ~0ull;
constexpr int kSkNone = 0xFFFF;
constexpr int64_t kDiagBias = (int64_t)1 << 30;             // read lengths are below 2^30: d + kDiagBias lies in (0, 2^31)

__device__ __forceinline__ u64 kmer_mix(u64 x, const u64 m) {
    x = (~x + (x << 21)) & m;
    x ^= x >> 24;
    x = (x + (x << 3) + (x << 8)) & m;
    x ^= x >> 14;
    x = (x + (x << 2) + (x << 4)) & m;
    x ^= x >> 28;
    x = (x + (x << 31)) & m;
    return x;
}

__device__ __forceinline__ int sk_slot(int j) { return j + (j >> 4); }

// the read of tile t: the largest r with tile_first[r] <= t (reads without a window own no tile)
__device__ __forceinline__ int64_t sk_read_of(const int64_t* __restrict__ tile_first, int64_t R, int64_t t) {
    int64_t lo = 0, hi = R;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

template <bool WRITE>
__global__ void __launch_bounds__(kSkThreads) k_sketch(const uint8_t* __restrict__ data, const int64_t* __restrict__ off, int64_t R, int k, int w,
                                                       const int64_t* __restrict__ tile_first, int64_t num_tiles, int64_t* __restrict__ tile_cnt,
                                                       u64* __restrict__ o_hash, int32_t* __restrict__ o_read, int32_t* __restrict__ o_pos,
                                                       uint8_t* __restrict__ o_strand, int64_t capacity) {
    __shared__ __attribute__((aligned(16))) uint32_t raw_s[kSkRawWords];
    __shared__ uint32_t code_s[kSkGroups], bad_s[kSkGroups], strand_s[kSkRuns];
    __shared__ u64 hash_s[kSkHashSlots];
    __shared__ uint16_t min_s[kSkTile + 1];
    __shared__ int chunk_s[kSkChunks * kSkWaves + 1];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t total = off[R];
    const u64 mask = (1ull << (2 * k)) - 1, kbits = (1ull << k) - 1;
    const int top = 2 * (k - 1);
    for (int64_t t = blockIdx.x; t < num_tiles; t += gridDim.x) {
        const int64_t r = sk_read_of(tile_first, R, t), rb = off[r];
        const int L = (int)(off[r + 1] - rb);
        const int t0 = (int)(t - tile_first[r]) * kSkTile;   // the tile's first window
        const int lb = t0 > 0;                               // it also looks at the window before, to know what that one emitted
        const int b0 = t0 - lb;                              // local index 0 = base, k-mer start and window b0 of the read
        const int nwin = L - k - w + 2;
        const int nv = (nwin - t0 < kSkTile ? nwin - t0 : kSkTile) + lb;   // local windows
        const int np = nv + w - 1;                                          // local k-mer starts
        const int nb = np + k - 1;                                          // local bases: b0 + nb <= L
        const int64_t g0 = rb + b0;
        const int sh = (int)(g0 & 3);
        const uint32_t* __restrict__ p32 = reinterpret_cast<const uint32_t*>(data + (g0 - sh));
        const int nwords = (sh + nb + 3) >> 2;
        for (int i = tid; i < kSkRawWords; i += kSkThreads) {
            uint32_t v = 0;
            if (i < nwords) {
                const int64_t byte0 = g0 - sh + 4 * (int64_t)i;
                if (byte0 + 4 <= total) {
                    v = p32[i];
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (byte0 + j < total) v |= (uint32_t)data[byte0 + j] << (8 * j);
                }
            }
            raw_s[i] = v;
        }
        __syncthreads();
        for (int g = tid; g < kSkGroups; g += kSkThreads) {
            const uint4 q = *reinterpret_cast<const uint4*>(&raw_s[4 * g]);
            const uint32_t wv[5] = {q.x, q.y, q.z, q.w, raw_s[4 * g + 4]};
            uint32_t codes = 0, bad = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t word = (uint32_t)((((u64)wv[j + 1] << 32) | wv[j]) >> (8 * sh));
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t c = (word >> (8 * b)) & 0xFFu, uc = c & 0xDFu, x = (c >> 1) & 3u, n = 4 * j + b;
                    const bool ok = (uc == 'A' || uc == 'C' || uc == 'G' || uc == 'T') && 16 * g + (int)n < nb;
                    codes |= ok ? (x ^ (x >> 1)) << (2 * n) : 0u;
                    bad |= ok ? 0u : 1u << n;
                }
            }
            code_s[g] = codes;
            bad_s[g] = bad;
        }
        __syncthreads();
        for (int g = tid; g < kSkRuns; g += kSkThreads) {
            if (16 * g >= np) continue;
            unsigned __int128 S = ((unsigned __int128)code_s[g + 2] << 64) | ((u64)code_s[g + 1] << 32) | code_s[g];
            const u64 B = ((u64)bad_s[g + 2] << 32) | ((u64)bad_s[g + 1] << 16) | bad_s[g];
            u64 fwd = 0, rev = 0;
            for (int i = 0; i < k - 1; ++i) {
                const u64 c = (u64)S & 3;
                S >>= 2;
                fwd = ((fwd << 2) | c) & mask;
                rev = (rev >> 2) | ((3 - c) << top);
            }
            uint32_t sbits = 0;
#pragma unroll
            for (int i = 0; i < kSkRun; ++i) {
                const u64 c = (u64)S & 3;
                S >>= 2;
                fwd = ((fwd << 2) | c) & mask;
                rev = (rev >> 2) | ((3 - c) << top);
                const bool ok = ((B >> i) & kbits) == 0 && fwd != rev && 16 * g + i < np;
                sbits |= (uint32_t)(rev < fwd) << i;
                hash_s[sk_slot(16 * g + i)] = ok ? kmer_mix(rev < fwd ? rev : fwd, mask) : kSkInvalid;
            }
            strand_s[g] = sbits;
        }
        __syncthreads();
        for (int v = tid; v < nv; v += kSkThreads) {
            u64 best = kSkInvalid;
            int arg = kSkNone;
            for (int j = 0; j < w; ++j) {
                const u64 h = hash_s[sk_slot(v + j)];
                if (h < best) {
                    best = h;
                    arg = v + j;
                }
            }
            min_s[v] = (uint16_t)arg;
        }
        __syncthreads();
        uint32_t ebits = 0;
#pragma unroll
        for (int i = 0; i < kSkChunks; ++i) {
            const int v = lb + i * kSkThreads + tid;
            const bool e = v < nv && min_s[v] != kSkNone && (v == 0 || min_s[v - 1] != min_s[v]);
            const u64 bal = __ballot(e);
            if (lane == 0) chunk_s[i * kSkWaves + wave] = __popcll(bal);
            ebits |= (uint32_t)e << i;
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int c = 0; c < kSkChunks * kSkWaves; ++c) {
                const int x = chunk_s[c];
                chunk_s[c] = run;
                run += x;
            }
            chunk_s[kSkChunks * kSkWaves] = run;
        }
        __syncthreads();
        if (!WRITE) {
            if (tid == 0) tile_cnt[t] = chunk_s[kSkChunks * kSkWaves];
        } else {
            const int64_t base = tile_cnt[t];
#pragma unroll
            for (int i = 0; i < kSkChunks; ++i) {
                const bool e = (ebits >> i) & 1u;
                const u64 bal = __ballot(e);
                const int64_t slot = base + chunk_s[i * kSkWaves + wave] + __popcll(bal & ((1ull << lane) - 1));
                if (e && slot < capacity) {
                    const int m = min_s[lb + i * kSkThreads + tid];
                    o_hash[slot] = hash_s[sk_slot(m)];
                    o_read[slot] = (int32_t)r;
                    o_pos[slot] = b0 + m;
                    o_strand[slot] = (uint8_t)((strand_s[m >> 4] >> (m & 15)) & 1u);
                }
            }
        }
        __syncthreads();   // the next tile overwrites the LDS images
    }
}

// ---- exclusive scan of int64[n] in place, the total to a[n]: per-tile sums, ONE workgroup over them, per-tile apply ---------------------
constexpr int kScThreads = 256;
constexpr int kScItems = 4;
constexpr int kScTile = kScThreads * kScItems;
constexpr int kScWaves = kScThreads / kWave;

static inline int64_t sc_tiles(int64_t n) { return (n + kScTile - 1) / kScTile; }
static inline size_t og_align(size_t x) { return (x + 255) & ~(size_t)255; }
static unsigned og_grid(int64_t blocks) { return (unsigned)(blocks < 1 ? 1 : blocks < kNumCUs * 8 ? blocks : kNumCUs * 8); }

// the sum over the workgroup's earlier threads, and over all of them
__device__ __forceinline__ int64_t sc_block_scan(const int64_t agg, int64_t* __restrict__ wave_s, int64_t& total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int64_t inc = agg;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int64_t up = (int64_t)__shfl_up((u64)inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();   // wave_s may still be read by the previous call
    if (lane == kWave - 1) wave_s[wave] = inc;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int x = 0; x < kScWaves; ++x) {
        const int64_t s = wave_s[x];
        if (x < wave) before += s;
        all += s;
    }
    total = all;
    return before + inc - agg;
}

__global__ void __launch_bounds__(kScThreads) k_scan_reduce(const int64_t* __restrict__ a, int64_t n, int64_t* __restrict__ part) {
    __shared__ int64_t wave_s[kScWaves];
    const int64_t tiles = (n + kScTile - 1) / kScTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i0 = t * kScTile + (int64_t)threadIdx.x * kScItems;
        int64_t agg = 0, total;
#pragma unroll
        for (int x = 0; x < kScItems; ++x) agg += i0 + x < n ? a[i0 + x] : 0;
        sc_block_scan(agg, wave_s, total);
        if (threadIdx.x == 0) part[t] = total;
    }
}

// launched with ONE workgroup: v[0 .. n) becomes its exclusive scan on top of `seed`, the total goes to total_out[0]
__global__ void __launch_bounds__(kScThreads) k_scan_one(int64_t* __restrict__ v, int64_t n, int64_t* __restrict__ total_out) {
    __shared__ int64_t wave_s[kScWaves];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < n; c0 += kScTile) {
        const int64_t i0 = c0 + (int64_t)threadIdx.x * kScItems;
        int64_t x[kScItems], agg = 0, total;
#pragma unroll
        for (int j = 0; j < kScItems; ++j) {
            x[j] = i0 + j < n ? v[i0 + j] : 0;
            agg += x[j];
        }
        int64_t run = carry + sc_block_scan(agg, wave_s, total);
#pragma unroll
        for (int j = 0; j < kScItems; ++j) {
            if (i0 + j < n) v[i0 + j] = run;
            run += x[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0 && total_out) total_out[0] = carry;
}

__global__ void __launch_bounds__(kScThreads) k_scan_apply(int64_t* __restrict__ a, int64_t n, const int64_t* __restrict__ part) {
    __shared__ int64_t wave_s[kScWaves];
    const int64_t tiles = (n + kScTile - 1) / kScTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i0 = t * kScTile + (int64_t)threadIdx.x * kScItems;
        int64_t x[kScItems], agg = 0, total;
#pragma unroll
        for (int j = 0; j < kScItems; ++j) {
            x[j] = i0 + j < n ? a[i0 + j] : 0;
            agg += x[j];
        }
        int64_t run = part[t] + sc_block_scan(agg, wave_s, total);
#pragma unroll
        for (int j = 0; j < kScItems; ++j) {
            if (i0 + j < n) a[i0 + j] = run;
            run += x[j];
        }
    }
}

// a[0 .. n) -> its exclusive scan, a[n] = the total; part: int64[sc_tiles(n)]
static int og_exclusive_scan(int64_t* a, int64_t n, int64_t* part, hipStream_t s) {
    const int64_t tiles = sc_tiles(n);
    const dim3 grid(og_grid(tiles)), block(kScThreads);
    hipLaunchKernelGGL(k_scan_reduce, grid, block, 0, s, (const int64_t*)a, n, part);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scan_one, dim3(1), block, 0, s, part, tiles, a + n);
    GN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scan_apply, grid, block, 0, s, a, n, (const int64_t*)part);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

// ---- seed pairs --------------------------------------------------------------------------------------------------------------------------
constexpr int kSpThreads = 256;

// cnt[i]: the seeds of i's bucket in earlier reads (0 for a bucket of more than max_occ seeds); back[i] = i - (start of the bucket)
__global__ void __launch_bounds__(kSpThreads) k_sp_count(const u64* __restrict__ hash, const int32_t* __restrict__ read, int64_t M, int max_occ,
                                                         int64_t* __restrict__ cnt, int32_t* __restrict__ back) {
    for (int64_t i = (int64_t)blockIdx.x * kSpThreads + threadIdx.x; i < M; i += (int64_t)gridDim.x * kSpThreads) {
        const u64 h = hash[i];
        int64_t l = i - max_occ < 0 ? 0 : i - max_occ, r = i;
        while (l < r) {   // the first seed of the bucket, or of what of it lies within max_occ of i
            const int64_t m = (l + r) >> 1;
            if (hash[m] == h) r = m; else l = m + 1;
        }
        const int64_t lo = l;
        l = i + 1;
        r = i + (int64_t)max_occ + 1 < M ? i + (int64_t)max_occ + 1 : M;
        while (l < r) {
            const int64_t m = (l + r) >> 1;
            if (hash[m] == h) l = m + 1; else r = m;
        }
        int64_t c = 0;
        if (l - lo <= max_occ) {   // the clipped size exceeds max_occ whenever the true size does
            const int32_t mine = read[i];
            int64_t a = lo, b = i;
            while (a < b) {
                const int64_t m = (a + b) >> 1;
                if (read[m] < mine) a = m + 1; else b = m;
            }
            c = a - lo;
        }
        cnt[i] = c;
        back[i] = (int32_t)(i - lo);
    }
}

__global__ void __launch_bounds__(kSpThreads) k_sp_write(const int64_t* __restrict__ base, const int32_t* __restrict__ back,
                                                         const int32_t* __restrict__ read, const int32_t* __restrict__ pos,
                                                         const uint8_t* __restrict__ strand, int64_t M, const int64_t* __restrict__ off, int k,
                                                         int64_t P, int64_t* __restrict__ key_ab, int64_t* __restrict__ key_dp) {
    for (int64_t t = (int64_t)blockIdx.x * kSpThreads + threadIdx.x; t < P; t += (int64_t)gridDim.x * kSpThreads) {
        int64_t l = 0, r = M;   // the seed i with base[i] <= t < base[i + 1]: base[M] = P > t
        while (r - l > 1) {
            const int64_t m = (l + r) >> 1;
            if (base[m] <= t) l = m; else r = m;
        }
        const int64_t i = l, p = i - back[i] + (t - base[i]);
        const int64_t a = read[p], b = read[i];
        const int rel = strand[p] ^ strand[i];
        const int64_t pa = pos[p], pb = pos[i];
        const int64_t d = pa - (rel ? (off[b + 1] - off[b]) - k - pb : pb);
        key_ab[t] = (a << 32) | (b << 1) | rel;
        key_dp[t] = ((d + kDiagBias) << 32) | pa;
    }
}

// ---- chains ------------------------------------------------------------------------------------------------------------------------------
constexpr int kChThreads = 256;
constexpr int kChWaves = kChThreads / kWave;
constexpr int kChFields = 10;   // a, b, rel, kind, d_beg, d_end, n_seeds, span_beg, span_end, overlap_length

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 x = __shfl_xor(v, o);
        v = x < v ? x : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 x = __shfl_xor(v, o);
        v = x > v ? x : v;
    }
    return v;
}

__global__ void __launch_bounds__(kChThreads) k_chain(const int64_t* __restrict__ key_ab, const int64_t* __restrict__ key_dp,
                                                      const int64_t* __restrict__ group_start, int64_t G, const int64_t* __restrict__ off, int k,
                                                      int band, int min_seeds, int min_overlap, int max_hang, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t first = (int64_t)blockIdx.x * kChWaves + threadIdx.x / kWave, step = (int64_t)gridDim.x * kChWaves;
    for (int64_t g = first; g < G; g += step) {
        const int64_t s = group_start[g], e = group_start[g + 1];
        bool open = false;
        int64_t d0 = 0;
        int cur_n = 0, best_n = 0;
        u64 cur_min = ~0ull, cur_max = 0, best_min = 0, best_max = 0;
        for (int64_t c = s; c < e; c += kWave) {
            const int cnt = e - c < kWave ? (int)(e - c) : kWave;
            const u64 kd = lane < cnt ? (u64)key_dp[c + lane] : 0;
            const int64_t d = (int64_t)(kd >> 32) - kDiagBias;
            const u64 pk = (kd << 32) | (kd >> 32);   // (pa, d + bias): smallest pa then smallest d, largest pa then largest d
            int at = 0;
            while (at < cnt) {
                if (!open) {
                    d0 = (int64_t)__shfl((u64)d, at);
                    open = true;
                    cur_n = 0;
                    cur_min = ~0ull;
                    cur_max = 0;
                }
                const bool in = lane >= at && lane < cnt && d <= d0 + band;   // sorted by d: a prefix of what is left
                const int n = __popcll(__ballot(in));
                cur_min = min(cur_min, wave_min_u64(in ? pk : ~0ull));
                cur_max = max(cur_max, wave_max_u64(in ? pk : 0ull));
                cur_n += n;
                at += n;
                if (at < cnt) {   // the record at `at` lies above the band: the band is closed
                    if (cur_n > best_n) best_n = cur_n, best_min = cur_min, best_max = cur_max;
                    open = false;
                }
            }
        }
        if (open && cur_n > best_n) best_n = cur_n, best_min = cur_min, best_max = cur_max;
        if (lane == 0) {
            const u64 ab = (u64)key_ab[s];
            const int64_t a = (int64_t)(ab >> 32), b = (int64_t)((ab & 0xFFFFFFFFull) >> 1);
            const int rel = (int)(ab & 1);
            const int64_t la = off[a + 1] - off[a], lb = off[b + 1] - off[b];
            const int64_t span_beg = (int64_t)(best_min >> 32), span_end = (int64_t)(best_max >> 32) + k;
            const int64_t d_beg = (int64_t)(best_min & 0xFFFFFFFFull) - kDiagBias, d_end = (int64_t)(best_max & 0xFFFFFFFFull) - kDiagBias;
            const int64_t As = d_beg > 0 ? d_beg : 0, Ae = la < lb + d_end ? la : lb + d_end;
            int kind;
            int64_t ol = 0;
            if (best_n < min_seeds) kind = 5;
            else if (span_beg - As > max_hang || Ae - span_end > max_hang) kind = 0;
            else if (d_beg >= 0 && lb + d_end <= la) kind = 1;
            else if (d_beg <= 0 && la <= lb + d_end) kind = 2;
            else if (d_beg > 0) kind = 3, ol = la - d_beg < lb ? la - d_beg : lb;
            else kind = 4, ol = lb + d_beg < la ? lb + d_beg : la;
            if (kind >= 3 && ol < min_overlap) kind = 6;
            const int32_t row[kChFields] = {(int32_t)a, (int32_t)b, rel, kind, (int32_t)d_beg, (int32_t)d_end, best_n, (int32_t)span_beg,
                                            (int32_t)span_end, (int32_t)ol};
#pragma unroll
            for (int f = 0; f < kChFields; ++f) out[(int64_t)f * G + g] = row[f];
        }
    }
}

struct SkLayout {
    size_t tiles, part, total;
};
static SkLayout sk_layout(int64_t num_tiles) {
    SkLayout L;
    size_t o = 0;
    L.tiles = o; o = og_align(o + (size_t)(num_tiles + 1) * sizeof(int64_t));
    L.part = o;  o = og_align(o + (size_t)sc_tiles(num_tiles) * sizeof(int64_t));
    L.total = o;
    return L;
}

struct SpLayout {
    size_t base, back, part, total;
};
static SpLayout sp_layout(int64_t M) {
    SpLayout L;
    size_t o = 0;
    L.base = o; o = og_align(o + (size_t)(M + 1) * sizeof(int64_t));
    L.back = o; o = og_align(o + (size_t)M * sizeof(int32_t));
    L.part = o; o = og_align(o + (size_t)sc_tiles(M) * sizeof(int64_t));
    L.total = o;
    return L;
}

}  // namespace gnnome

extern "C" int gnnome_sketch_tile_size(int* tile_host) {
    GN_REQUIRE(tile_host, "sketch_tile_size: null pointer");
    *tile_host = gnnome::kSkTile;
    return GNNOME_OK;
}

extern "C" int gnnome_sketch_workspace_bytes(int64_t num_tiles, size_t* bytes_host) {
    GN_REQUIRE(num_tiles >= 0 && num_tiles < ((int64_t)1 << 31) && bytes_host, "sketch_workspace_bytes: bad argument (num_tiles=%lld)",
               (long long)num_tiles);
    *bytes_host = gnnome::sk_layout(num_tiles).total;
    return GNNOME_OK;
}

extern "C" int gnnome_sketch_reads(const uint8_t* data, const int64_t* off, int64_t num_reads, int k, int w, const int64_t* tile_first,
                                   int64_t num_tiles, uint64_t* hash, int32_t* read, int32_t* pos, uint8_t* strand, int64_t capacity,
                                   int64_t* result_host, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(result_host, "sketch_reads: null result_host");
    GN_REQUIRE(k >= 1 && k <= 31 && w >= 1 && k + w - 1 <= kSkMaxHalo, "sketch_reads: k=%d w=%d: need 1 <= k <= 31, w >= 1, k + w - 1 <= %d", k, w,
               kSkMaxHalo);
    GN_REQUIRE(num_reads >= 0 && num_reads < ((int64_t)1 << 30) && num_tiles >= 0 && num_tiles < ((int64_t)1 << 31),
               "sketch_reads: num_reads=%lld num_tiles=%lld out of range", (long long)num_reads, (long long)num_tiles);
    const bool write = hash != nullptr;
    if (!write) result_host[0] = 0;
    if (num_tiles == 0) return GNNOME_OK;   // no read holds a window: no minimizer, nothing launched
    GN_REQUIRE(data && off && tile_first && workspace, "sketch_reads: null pointer");
    GN_REQUIRE(((uintptr_t)data & 3) == 0, "sketch_reads: data must be 4-byte aligned");
    const SkLayout L = sk_layout(num_tiles);
    if (workspace_bytes < L.total) {
        set_error("sketch_reads: workspace %zu < %zu bytes", workspace_bytes, L.total);
        return GNNOME_EWORKSPACE;
    }
    int64_t* tiles = (int64_t*)((char*)workspace + L.tiles);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)num_tiles), block(kSkThreads);
    if (!write) {
        hipLaunchKernelGGL(k_sketch<false>, grid, block, 0, s, data, off, num_reads, k, w, tile_first, num_tiles, tiles, (u64*)nullptr,
                           (int32_t*)nullptr, (int32_t*)nullptr, (uint8_t*)nullptr, (int64_t)0);
        GN_LAUNCH_CHECK();
        const int rc = og_exclusive_scan(tiles, num_tiles, (int64_t*)((char*)workspace + L.part), s);
        if (rc != GNNOME_OK) return rc;
        GN_HIP(hipMemcpyAsync(result_host, tiles + num_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        return GNNOME_OK;
    }
    GN_REQUIRE(read && pos && strand && capacity >= 0, "sketch_reads: null output or capacity=%lld", (long long)capacity);
    hipLaunchKernelGGL(k_sketch<true>, grid, block, 0, s, data, off, num_reads, k, w, tile_first, num_tiles, tiles, (u64*)hash, read, pos,
                       strand, capacity);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_seed_pairs_workspace_bytes(int64_t num_seeds, size_t* bytes_host) {
    GN_REQUIRE(num_seeds >= 0 && num_seeds < ((int64_t)1 << 40) && bytes_host, "seed_pairs_workspace_bytes: bad argument (num_seeds=%lld)",
               (long long)num_seeds);
    *bytes_host = gnnome::sp_layout(num_seeds).total;
    return GNNOME_OK;
}

extern "C" int gnnome_seed_pairs(const uint64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand, int64_t num_seeds,
                                 const int64_t* off, int64_t num_reads, int k, int max_occ, int64_t* key_ab, int64_t* key_dp,
                                 int64_t capacity, int64_t* result_host, void* workspace, size_t workspace_bytes, void* stream) {
    using namespace gnnome;
    const int64_t M = num_seeds;
    GN_REQUIRE(result_host, "seed_pairs: null result_host");
    GN_REQUIRE(M >= 0 && M < ((int64_t)1 << 40) && num_reads >= 0 && num_reads < ((int64_t)1 << 30), "seed_pairs: num_seeds=%lld num_reads=%lld",
               (long long)M, (long long)num_reads);
    GN_REQUIRE(k >= 1 && k <= 31 && max_occ >= 1 && max_occ <= (1 << 20), "seed_pairs: k=%d max_occ=%d out of range", k, max_occ);
    const bool write = key_ab != nullptr;
    if (!write) result_host[0] = 0;
    if (M == 0) return GNNOME_OK;
    GN_REQUIRE(hash && read && pos && strand && off && workspace, "seed_pairs: null pointer");
    const SpLayout L = sp_layout(M);
    if (workspace_bytes < L.total) {
        set_error("seed_pairs: workspace %zu < %zu bytes", workspace_bytes, L.total);
        return GNNOME_EWORKSPACE;
    }
    int64_t* base = (int64_t*)((char*)workspace + L.base);
    int32_t* back = (int32_t*)((char*)workspace + L.back);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(kSpThreads);
    if (!write) {
        hipLaunchKernelGGL(k_sp_count, dim3(og_grid((M + kSpThreads - 1) / kSpThreads)), block, 0, s, (const u64*)hash, read, M, max_occ, base, back);
        GN_LAUNCH_CHECK();
        const int rc = og_exclusive_scan(base, M, (int64_t*)((char*)workspace + L.part), s);
        if (rc != GNNOME_OK) return rc;
        GN_HIP(hipMemcpyAsync(result_host, base + M, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        GN_HIP(hipStreamSynchronize(s));
        return GNNOME_OK;
    }
    GN_REQUIRE(key_dp && capacity >= 0, "seed_pairs: null key_dp or capacity=%lld", (long long)capacity);
    if (capacity == 0) return GNNOME_OK;
    // capacity is the count pass's total: base[M] = capacity, so every record t < capacity has its seed
    hipLaunchKernelGGL(k_sp_write, dim3(og_grid((capacity + kSpThreads - 1) / kSpThreads)), block, 0, s, (const int64_t*)base, (const int32_t*)back,
                       read, pos, strand, M, off, k, capacity, key_ab, key_dp);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}

extern "C" int gnnome_chain_overlaps(const int64_t* key_ab, const int64_t* key_dp, int64_t num_records, const int64_t* group_start,
                                     int64_t num_groups, const int64_t* off, int64_t num_reads, int k, int band, int min_seeds, int min_overlap,
                                     int max_hang, int32_t* out, void* stream) {
    using namespace gnnome;
    GN_REQUIRE(num_records >= 0 && num_groups >= 0 && num_groups <= num_records && num_reads >= 0, "chain_overlaps: %lld records, %lld groups",
               (long long)num_records, (long long)num_groups);
    GN_REQUIRE(k >= 1 && k <= 31 && band >= 0 && min_seeds >= 1 && min_overlap >= 0 && max_hang >= 0,
               "chain_overlaps: k=%d band=%d min_seeds=%d min_overlap=%d max_hang=%d out of range", k, band, min_seeds, min_overlap, max_hang);
    if (num_groups == 0) return GNNOME_OK;
    GN_REQUIRE(key_ab && key_dp && group_start && off && out, "chain_overlaps: null pointer");
    hipLaunchKernelGGL(k_chain, dim3(og_grid((num_groups + kChWaves - 1) / kChWaves)), dim3(kChThreads), 0, (hipStream_t)stream, key_ab, key_dp,
                       group_start, num_groups, off, k, band, min_seeds, min_overlap, max_hang, out);
    GN_LAUNCH_CHECK();
    return GNNOME_OK;
}
