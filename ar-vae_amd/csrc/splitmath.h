// The split-operand arithmetic of every MFMA kernel: the only definition of the vector types, the power-of-two scale, the two
// splits, the LDS operand reads and the product orders.  (The per-tensor maxima that feed the scale: amax.h.)
//
// Every product on the hot path runs on one of two arithmetics:
//   SCALED TWO-TERM fp16   s x = h + l, h = fp16(s x), l = fp16(s x - h); a product is l h', h l', h h'          (split2, MFMA3)
//   THREE-TERM bf16        x = hi + mid + lo, each the bf16 of what the terms before left; six partial products    (split3, MFMA6)
// tests/test_two_term_arithmetic.py and tests/test_three_term_arithmetic.py model exactly the functions and macros of this file.
#pragma once
#include "common.h"

namespace arvae {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ---- the scale -------------------------------------------------------------------------------------------------------------------
// fp16 has 5 exponent bits, so a two-term operand is multiplied by the power of two s that brings the largest magnitude of its
// tensor (or row, or wave's slice: whatever factors out of the dot product) into [2^14, 2^15); the result is multiplied by the
// inverse scales of both operands (exact).
struct Pow2 { float s, inv; };
// from the bit pattern of max |X| (0: an all-zero tensor, any scale will do)
__host__ __device__ __forceinline__ Pow2 pow2_for(unsigned amax_bits) {
    int e = (int)((amax_bits >> 23) & 0xffu);                    // biased exponent: 2^(e - 127) <= max |X| < 2^(e - 126)
    e = e < 16 ? 16 : e;                                         // (denormal / zero maxima: scale 2^125, nothing overflows)
    Pow2 r;
    const unsigned sb = (unsigned)(268 - e) << 23, ib = (unsigned)(e - 14) << 23;     // 2^(14 - (e - 127)) and its inverse
#if defined(__HIP_DEVICE_COMPILE__)
    r.s = __builtin_bit_cast(float, sb); r.inv = __builtin_bit_cast(float, ib);
#else
    memcpy(&r.s, &sb, 4); memcpy(&r.inv, &ib, 4);
#endif
    return r;
}
__device__ __forceinline__ Pow2 pow2_for(float amax) { return pow2_for(__builtin_bit_cast(unsigned, amax)); }

// ---- the two-term split ----------------------------------------------------------------------------------------------------------
// h + l reproduces s x to 2^-22 relative for every element within 2^16 of the maximum and to 2^-39 of that maximum below; of a
// product's four partial products l l' <= 2^-22 is dropped.  Measured against float64 the results sit at 0.7e-7 relative L2 for
// K = 512 dot products -- the three-term bf16 split measured 0.6e-7, an fp32 FMA chain 2-3e-7 -- at half the MFMAs and two thirds
// of the LDS operand bytes of the three-term split.
//
// two values -> packed (h, l) pairs, low half of a dword = first value; eight single-issue instructions per pair (no packed-f32
// instruction: a loader wave runs beside an MFMA wave, and a packed-f32 instruction costs the partner three of the ~3.5 issue
// slots it gets per MFMA, tools/probes/coissue.hip).  A five-instruction form on the mixed-precision FMA (v_fma_mixlo / mixhi_f16
// for h, v_fma_mix_f32 with h as its fp16 addend for the residual) passed every test and measured SLOWER in the loader waves
// (1.3 against 1.1 us per tile of down32p_kernel): those encodings do not co-issue beside the partner's MFMAs either.
// PIN: two empty asm statements make the scaled values and the residuals registers of their own at that point, which keeps the
// compiler from folding the split into its neighbours (the convolutions' loader waves were tuned with them).  The GRU recurrences
// were written and tuned without: pinned, 39 of their kernels compile differently (gru_seq_fwd_h2_kernel<128, 4>: 196 VGPRs instead
// of 142), so every call in gru_seq.hip passes PIN = false.  The arithmetic is the same either way.
template <bool PIN = true> __device__ __forceinline__ void split2(float x0, float x1, float s, unsigned &hi, unsigned &lo) {
    float y0 = x0 * s, y1 = x1 * s;
    if constexpr (PIN) asm volatile("" : "+v"(y0), "+v"(y1));
    const f32x2 y = {y0, y1};
    const f16x2 h = __builtin_convertvector(y, f16x2);           // v_cvt_pk_f16_f32, round to nearest even
    hi = __builtin_bit_cast(unsigned, h);
    float r0 = y0 - (float)h.x, r1 = y1 - (float)h.y;            // exact
    if constexpr (PIN) asm volatile("" : "+v"(r0), "+v"(r1));
    const f32x2 r = {r0, r1};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
}
// eight values -> their (h, l) operand registers
template <bool PIN = true> __device__ __forceinline__ void split2_8(const float (&x)[8], float s, f16x8 &hi, f16x8 &lo) {
    i32x4 h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned a, b;
        split2<PIN>(x[2 * j], x[2 * j + 1], s, a, b);
        h[j] = (int)a; l[j] = (int)b;
    }
    hi = __builtin_bit_cast(f16x8, h); lo = __builtin_bit_cast(f16x8, l);
}
// one value -> its two terms into the two LDS planes (plane stride in ushorts) ...
template <bool PIN = true> __device__ __forceinline__ void store_split2(unsigned short *p, int plane, float x, float s) {
    unsigned a, b;
    split2<PIN>(x, 0.f, s, a, b);
    p[0] = (unsigned short)a; p[plane] = (unsigned short)b;
}
// ... and two values (rows `rowpitch` apart in every plane) for the price of one split
template <bool PIN = true>
__device__ __forceinline__ void store_split2(unsigned short *p, int rowpitch, int plane, float x0, float x1, float s) {
    unsigned a, b;
    split2<PIN>(x0, x1, s, a, b);
    p[0] = (unsigned short)a; p[rowpitch] = (unsigned short)(a >> 16);
    p[plane] = (unsigned short)b; p[plane + rowpitch] = (unsigned short)(b >> 16);
}
// four consecutive values -> 8 bytes in each of the two LDS planes
__device__ __forceinline__ void store_split2_x4(unsigned short *d, int plane, const float4 &v, float s) {
    unsigned h0, l0, h1, l1;
    split2(v.x, v.y, s, h0, l0);
    split2(v.z, v.w, s, h1, l1);
    *reinterpret_cast<uint2 *>(d) = uint2{h0, h1};
    *reinterpret_cast<uint2 *>(d + plane) = uint2{l0, l1};
}

// ---- the three-term split --------------------------------------------------------------------------------------------------------
// fp32 pair -> three bf16 terms each (hi + mid + lo exact to 2^-26), packed (first value in the low half); no scale: bf16 has the
// exponent range of fp32
__device__ __forceinline__ void split3(float x0, float x1, unsigned &hi, unsigned &mid, unsigned &lo) {
    const f32x2 x = {x0, x1};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2));
    const f32x2 r = {x0 - __builtin_bit_cast(float, hi << 16), x1 - __builtin_bit_cast(float, hi & 0xffff0000u)};
    mid = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
    const f32x2 q = {r.x - __builtin_bit_cast(float, mid << 16), r.y - __builtin_bit_cast(float, mid & 0xffff0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(q, bf16x2));
}
__device__ __forceinline__ void split3_8(const float (&x)[8], bf16x8 &hi, bf16x8 &mid, bf16x8 &lo) {
    i32x4 h, m, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned a, b, c;
        split3(x[2 * j], x[2 * j + 1], a, b, c);
        h[j] = (int)a; m[j] = (int)b; l[j] = (int)c;
    }
    hi = __builtin_bit_cast(bf16x8, h); mid = __builtin_bit_cast(bf16x8, m); lo = __builtin_bit_cast(bf16x8, l);
}
// one value / two values -> the three LDS planes, as store_split2
__device__ __forceinline__ void store_split3(unsigned short *p, int plane, float x) {
    unsigned a, b, c;
    split3(x, 0.f, a, b, c);
    p[0] = (unsigned short)a; p[plane] = (unsigned short)b; p[2 * plane] = (unsigned short)c;
}
__device__ __forceinline__ void store_split3(unsigned short *p, int rowpitch, int plane, float x0, float x1) {
    unsigned a, b, c;
    split3(x0, x1, a, b, c);
    p[0] = (unsigned short)a; p[rowpitch] = (unsigned short)(a >> 16);
    p[plane] = (unsigned short)b; p[plane + rowpitch] = (unsigned short)(b >> 16);
    p[2 * plane] = (unsigned short)c; p[2 * plane + rowpitch] = (unsigned short)(c >> 16);
}
// four consecutive values -> 8 bytes in each of the three LDS planes.  Split and store are two calls because the compiler's
// schedule follows the order of the source: x3tile.h splits BEFORE it works out the address, conv64.hip's row kernel after.
struct Split3x4 { uint2 hi, mid, lo; };
__device__ __forceinline__ Split3x4 split3_x4(const float4 &v) {
    Split3x4 t;
    split3(v.x, v.y, t.hi.x, t.mid.x, t.lo.x);
    split3(v.z, v.w, t.hi.y, t.mid.y, t.lo.y);
    return t;
}
__device__ __forceinline__ void store_split3_x4(unsigned short *d, int plane, const Split3x4 &t) {
    *reinterpret_cast<uint2 *>(d) = t.hi;
    *reinterpret_cast<uint2 *>(d + plane) = t.mid;
    *reinterpret_cast<uint2 *>(d + 2 * plane) = t.lo;
}

// ---- the operand reads: T = f16x8 or bf16x8 --------------------------------------------------------------------------------------
// eight consecutive 16-bit values of one row: one ds_read_b128
template <class T> __device__ __forceinline__ T lds_x8(const void *p) { return __builtin_bit_cast(T, *reinterpret_cast<const i32x4 *>(p)); }
// eight values of one COLUMN of a "K x rows" image through the transposing read (ds_read_b64_tr_b16): p0 and p1 are this lane's
// addresses in the two 4-row blocks
template <class T> __device__ __forceinline__ T lds_tr_x8(const void *p0, const void *p1) {
    typedef __attribute__((address_space(3))) s16x4 *lds_ptr;
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p0);
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p1);
    return __builtin_bit_cast(T, (s16x8)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- the product orders ----------------------------------------------------------------------------------------------------------
// acc += A . B for one k-step.  Always SMALLEST FIRST: the partial products differ by 2^-8 (bf16) or 2^-11 (fp16) per term, and the
// fp32 accumulator rounds every addition to its own magnitude -- added last, the small products would be rounded at the magnitude
// of h h'; added first they are summed among their like and enter the large one as a whole.
//   two-term:    l h', h l', h h'                               (l l' <= 2^-22 is dropped)
//   three-term:  l h', h l', m m', m h', h m', h h'             (the six products >= 2^-18; m l', l m', l l' are dropped)
// The convolutions and GEMMs use 32 x 32 x 16 tiles, the GRU recurrences 16 x 16 x 32 (16 batch rows per workgroup).
#define MFMA_H(ACC, W, A) ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(W, A, ACC, 0, 0, 0)      // one product; callers order them
#define H2_MFMA3(ACC, AH, AL, BH, BL) MFMA_H(ACC, AL, BH); MFMA_H(ACC, AH, BL); MFMA_H(ACC, AH, BH)
#define X3_MFMA6(ACC, AH, AM, AL, BH, BM, BL)                                      \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AL, BH, ACC, 0, 0, 0);           \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH, BL, ACC, 0, 0, 0);           \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AM, BM, ACC, 0, 0, 0);           \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AM, BH, ACC, 0, 0, 0);           \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH, BM, ACC, 0, 0, 0);           \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH, BH, ACC, 0, 0, 0)
// the GRU's: one accumulator ...
#define GRU_MFMA3(ACC, AH, AL, WH, WL)                                                 \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(AL, WH, ACC, 0, 0, 0);                \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, WL, ACC, 0, 0, 0);                \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, WH, ACC, 0, 0, 0)
#define GRU_MFMA6(ACC, AH, AM, AL, WH, WM, WL)                                         \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AL, WH, ACC, 0, 0, 0);               \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, WL, ACC, 0, 0, 0);               \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AM, WM, ACC, 0, 0, 0);               \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AM, WH, ACC, 0, 0, 0);               \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, WM, ACC, 0, 0, 0);               \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, WH, ACC, 0, 0, 0)
// ... and three independent accumulators, product-major: consecutive MFMAs never hit the same accumulator (a dependent 16x16x32
// MFMA waits for its predecessor's result, about twice the issue interval), every accumulator still sees its products in order.
// K3: accumulator i takes A operand i (three k-steps); X3: one A operand for all three (the three gates)
#define GRU_MFMA3K3(A0, A1, A2, H0, L0, H1, L1, H2, L2, WH0, WL0, WH1, WL1, WH2, WL2)                                              \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(L0, WH0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(L1, WH1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(L2, WH2, A2, 0, 0, 0);                                                            \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(H0, WL0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(H1, WL1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(H2, WL2, A2, 0, 0, 0);                                                            \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(H0, WH0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(H1, WH1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(H2, WH2, A2, 0, 0, 0)
#define GRU_MFMA3X3(A0, A1, A2, AH, AL, WH0, WL0, WH1, WL1, WH2, WL2) \
    GRU_MFMA3K3(A0, A1, A2, AH, AL, AH, AL, AH, AL, WH0, WL0, WH1, WL1, WH2, WL2)
#define GRU_MFMA6X3(A0, A1, A2, H0, M0, L0, H1, M1, L1, H2, M2, L2, WH0, WM0, WL0, WH1, WM1, WL1, WH2, WM2, WL2)                 \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(L0, WH0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(L1, WH1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(L2, WH2, A2, 0, 0, 0);                                                          \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H0, WL0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H1, WL1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H2, WL2, A2, 0, 0, 0);                                                          \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(M0, WM0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(M1, WM1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(M2, WM2, A2, 0, 0, 0);                                                          \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(M0, WH0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(M1, WH1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(M2, WH2, A2, 0, 0, 0);                                                          \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H0, WM0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H1, WM1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H2, WM2, A2, 0, 0, 0);                                                          \
    A0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H0, WH0, A0, 0, 0, 0); A1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H1, WH1, A1, 0, 0, 0); \
    A2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(H2, WH2, A2, 0, 0, 0)

}  // namespace arvae
