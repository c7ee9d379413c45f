// The two exact operand splits behind every dense product of the library, defined ONCE: an fp32 operand goes to the matrix cores as
// two or three 16-bit planes, and the fp32 accuracy of the gate, the projections, the scorer and the backward's weight and data
// gradients rests on what is written here.
//
// bf16x6.  x = x1 + x2 + x3 EXACTLY, three bf16 planes (8 + 8 + 8 significant bits):
//     x1 = x with its low 16 bits cleared,  x2 = (x - x1) with its low 16 bits cleared,  x3 = x - x1 - x2.
//   Both subtractions are exact in fp32 (each removes leading bits of its left operand), and x3 has at most 8 significant bits, so its
//   low half is zero: a bf16.  Six of the nine plane products are kept; what is dropped is of the size of one fp32 rounding
//   (edge_gate_bf.hip and DESIGN.md explain and measure it).
//
// fp16x3.  x = x1 + x2 / 2048 + rx, two fp16 planes (11 + 11 significant bits):
//     x1 = RN16(x),  x2 = RN16((x - x1) * 2048),  |rx| <= 2^-22 |x|.
//   x - x1 is exact in fp32 and so are both products with 2048, which is why the fma form below, fma(x1, -2048, x * 2048), is the same
//   value.  The second plane is stored SCALED by 2^11 so that it is an fp16 normal whenever the first is; its two products go to a
//   second accumulator (or, with the third plane x1 * 2048, to the same one) and are folded in with 2^-11.  |x| beyond 65504 makes x1
//   inf and the output NaN: loud, never a wrong finite value.  The derivation and the measured error are in edge_tile_f16.hip's header,
//   the error model restated in numpy in tests/test_f16x3_model.py.
//
// Each split's arithmetic is written once, on its smallest unit - a float PAIR for fp16 (v_cvt_pk_f16_f32 works on pairs), one
// element for bf16 (v_perm_b32 then packs pairs) - and the 4- and 8-wide forms the kernels call are loops over it.  The forms differ
// only in the ORDER they hand the same operations to the scheduler, and that order is kept as the kernels were tuned with it:
// several of them sit at 212-256 VGPRs, where another order spills.
#pragma once
#include "common.h"

namespace gnnome {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// one lane's share of a 32x32x16 MFMA operand (eight consecutive k), as it leaves a split or LDS
__device__ __forceinline__ bf16x8 as_bf16x8(const uint4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ f16x8 as_f16x8(const uint4 v) { return __builtin_bit_cast(f16x8, v); }

// ---- bf16x6 ----

// element 2j in the low half, 2j + 1 in the high half: (even >> 16) | (odd & 0xFFFF0000), one v_perm_b32
__device__ __forceinline__ unsigned bf16_pack_hi(unsigned odd, unsigned even) { return __builtin_amdgcn_perm(odd, even, 0x07060302u); }

// the arithmetic, one element: the three planes' values as fp32 bit patterns whose low halves are zero
__device__ __forceinline__ void bf16_split1(const float x, unsigned& h, unsigned& m, unsigned& l) {
    h = __float_as_uint(x) & 0xFFFF0000u;
    const float r = x - __uint_as_float(h);        // exact
    m = __float_as_uint(r) & 0xFFFF0000u;
    l = __float_as_uint(r - __uint_as_float(m));   // exact, <= 8 significant bits: a bf16
}

// one float4 -> three 8-byte groups
__device__ __forceinline__ void bf16_split4(const f32x4 x, uint2& p1, uint2& p2, uint2& p3) {
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bf16_split1(x[j], h[j], m[j], l[j]);
    p1 = make_uint2(bf16_pack_hi(h[1], h[0]), bf16_pack_hi(h[3], h[2]));
    p2 = make_uint2(bf16_pack_hi(m[1], m[0]), bf16_pack_hi(m[3], m[2]));
    p3 = make_uint2(bf16_pack_hi(l[1], l[0]), bf16_pack_hi(l[3], l[2]));
}

// eight floats -> one MFMA operand per plane.  All eight elements first, then the packs, plane by plane: the order the register
// allocation of k_linear_bf2 and k_edge_gate_bf was tuned with (two bf16_split4 in a row cost k_linear_bf2<128> four VGPRs).
__device__ __forceinline__ void bf16_split8(const f32x4 lo, const f32x4 hi, uint4& p1, uint4& p2, uint4& p3) {
    unsigned h[8], m[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bf16_split1(j < 4 ? lo[j] : hi[j - 4], h[j], m[j], l[j]);
    p1 = make_uint4(bf16_pack_hi(h[1], h[0]), bf16_pack_hi(h[3], h[2]), bf16_pack_hi(h[5], h[4]), bf16_pack_hi(h[7], h[6]));
    p2 = make_uint4(bf16_pack_hi(m[1], m[0]), bf16_pack_hi(m[3], m[2]), bf16_pack_hi(m[5], m[4]), bf16_pack_hi(m[7], m[6]));
    p3 = make_uint4(bf16_pack_hi(l[1], l[0]), bf16_pack_hi(l[3], l[2]), bf16_pack_hi(l[5], l[4]), bf16_pack_hi(l[7], l[6]));
}

// ---- fp16x3 ----

constexpr float kLoScale = 2048.f, kLoInv = 1.0f / 2048.f;

// one float pair -> its pair in each of the two planes
__device__ __forceinline__ void f16_split2(const f32x2 v, f16x2& x1, f16x2& x2) {
    x1 = __builtin_convertvector(v, f16x2);
    const f32x2 big = v * kLoScale;
    const f32x2 r = {__builtin_fmaf((float)x1[0], -kLoScale, big[0]), __builtin_fmaf((float)x1[1], -kLoScale, big[1])};   // exact
    x2 = __builtin_convertvector(r, f16x2);
}
// the optional third plane x1 * 2048 (mode 3 at H = 256: all three products in ONE accumulator).  Exact while |x| < 32, which the
// caller's scale sees to, a subnormal x1 included.
__device__ __forceinline__ f16x2 f16_plane1x(const f16x2 x1) {
    return __builtin_convertvector(f32x2{(float)x1[0], (float)x1[1]} * kLoScale, f16x2);
}

__device__ __forceinline__ void f16_split4(const f32x4 x, uint2& p1, uint2& p2) {
    f16x2 a[2], b[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) f16_split2(f32x2{x[2 * j], x[2 * j + 1]}, a[j], b[j]);
    p1 = make_uint2(__builtin_bit_cast(unsigned, a[0]), __builtin_bit_cast(unsigned, a[1]));
    p2 = make_uint2(__builtin_bit_cast(unsigned, b[0]), __builtin_bit_cast(unsigned, b[1]));
}
// with the third plane
__device__ __forceinline__ void f16_split4x(const f32x4 x, uint2& p1, uint2& p2, uint2& p1x) {
    f16x2 a[2], b[2], ax[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        f16_split2(f32x2{x[2 * j], x[2 * j + 1]}, a[j], b[j]);
        ax[j] = f16_plane1x(a[j]);
    }
    p1 = make_uint2(__builtin_bit_cast(unsigned, a[0]), __builtin_bit_cast(unsigned, a[1]));
    p2 = make_uint2(__builtin_bit_cast(unsigned, b[0]), __builtin_bit_cast(unsigned, b[1]));
    p1x = make_uint2(__builtin_bit_cast(unsigned, ax[0]), __builtin_bit_cast(unsigned, ax[1]));
}
// eight floats -> one MFMA operand per plane, as four 32-bit words or as the MFMA's own vector type
__device__ __forceinline__ void f16_split8(const f32x4 lo, const f32x4 hi, uint4& p1, uint4& p2) {
    unsigned a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f16x2 x1, x2;
        f16_split2(j < 2 ? f32x2{lo[2 * j], lo[2 * j + 1]} : f32x2{hi[2 * j - 4], hi[2 * j - 3]}, x1, x2);
        a[j] = __builtin_bit_cast(unsigned, x1);
        b[j] = __builtin_bit_cast(unsigned, x2);
    }
    p1 = make_uint4(a[0], a[1], a[2], a[3]);
    p2 = make_uint4(b[0], b[1], b[2], b[3]);
}
__device__ __forceinline__ void f16_split8(const f32x4 lo, const f32x4 hi, f16x8& p1, f16x8& p2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f16x2 x1, x2;
        f16_split2(j < 2 ? f32x2{lo[2 * j], lo[2 * j + 1]} : f32x2{hi[2 * j - 4], hi[2 * j - 3]}, x1, x2);
        p1[2 * j] = x1[0];
        p1[2 * j + 1] = x1[1];
        p2[2 * j] = x2[0];
        p2[2 * j + 1] = x2[1];
    }
}

}  // namespace gnnome
