// The streamed-weights GRU tile of hidden sizes 256 and 512: what the whole-sequence recurrences (gru_wide.hip), the free-running
// tick decoder (tick_wide.hip) and the beam search (beam_wide.hip) share.  A workgroup of GWT_WAVES = 4 waves owns GWT_RT = 32 batch rows x 16 hidden units and ALL THREE
// GATES of those units.  The waves split the K dimension of a GEMM, each on v_mfma_f32_16x16x32_bf16 with THREE-TERM bf16 operands
// split in registers on the way from memory (splitmath.h), two 16-row blocks per wave against the same weight registers.  The partial
// sums meet in LDS and are added in wave order 0, 1, 2, 3 (no float atomics: results are bit-identical from run to run); the
// epilogue is lane-local, two (row, unit) elements per lane, and its gate arithmetic follows GRU_ROUNDING (gru_common.h).
// All addressing is 64-bit.
#pragma once
#include "common.h"
#include "dispatch.h"
#include "splitmath.h"
#include "gru_common.h"

namespace arvae {

constexpr int GWT_RT = 32;                 // batch rows per workgroup
constexpr int GWT_WAVES = 4;               // waves per workgroup: each a quarter of K

// the built hidden sizes: f(std::integral_constant<int, H>{}) and true for one of them, false for any other
template <class F> inline bool gwt_with_hidden(int hidden, F &&f) { return with_int<256, 512>(hidden, static_cast<F &&>(f)); }
inline bool gwt_hidden_built(int hidden) {
    return gwt_with_hidden(hidden, [](auto) {});
}
inline bool gwt_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// eight consecutive floats (16-byte aligned) -> their three bf16 operand registers; MASK: times keep_scale and the eight keep bytes,
// (keep_scale * x) * m in fp32 before the split (scale_mask_kernel's product)
template <bool MASK>
__device__ __forceinline__ void gwt_load_split(const float *p, const uint8_t *m, float keep_scale, bf16x8 &hi, bf16x8 &mid, bf16x8 &lo) {
    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(p), v1 = *reinterpret_cast<const f32x4 *>(p + 4);
    float x[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    if constexpr (MASK) {
        const uchar4 m0 = *reinterpret_cast<const uchar4 *>(m), m1 = *reinterpret_cast<const uchar4 *>(m + 4);
        const float k[8] = {(float)m0.x, (float)m0.y, (float)m0.z, (float)m0.w, (float)m1.x, (float)m1.y, (float)m1.z, (float)m1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (keep_scale * x[i]) * k[i];
    }
    split3_8(x, hi, mid, lo);
}
__device__ __forceinline__ void gwt_load_split(const float *p, bf16x8 &hi, bf16x8 &mid, bf16x8 &lo) {
    gwt_load_split<false>(p, nullptr, 1.f, hi, mid, lo);
}

// a wave's quarter of K = H of  acc[rb][g] += a[src[rb]][:] . wmat[g H + unit tile][:]^T, the lane's operand row of either 16-row
// block given by the caller (src[rb]: a row of `a` and of the keep-mask; beam_wide.hip reads a beam's parent's state this way):
// A: lane (col, quad) holds row src[rb] as row `col` of block rb, k = 8 quad .. 8 quad + 7 of the k-step.
// B: lane (col, quad) holds unit `col` of the tile, the same k; B[k][n] = wmat[g H + unit][k].
template <int H, bool MASK>
__device__ __forceinline__ void gwt_gemm3_rows(f32x4 (&acc)[2][3], const float *a, int64_t a_stride, const uint8_t *m, float keep_scale,
                                               const float *wmat, const int64_t (&src)[2], int unit0, int w, int col, int quad) {
    constexpr int KW = H / GWT_WAVES, KS = KW / 32;           // a wave's share of K, its MFMA k-steps
    static_assert(KS >= 1, "whole k-steps per wave");
    const float *a_src[2];
    const uint8_t *m_src[2] = {nullptr, nullptr};
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        a_src[rb] = a + src[rb] * a_stride + w * KW + 8 * quad;
        if constexpr (MASK) m_src[rb] = m + src[rb] * H + w * KW + 8 * quad;
    }
    const float *w_src = wmat + (int64_t)(unit0 + col) * H + w * KW + 8 * quad;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 ah[2], am[2], al[2], wh[3], wm[3], wl[3];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) gwt_load_split<MASK>(a_src[rb] + 32 * ks, MASK ? m_src[rb] + 32 * ks : nullptr, keep_scale, ah[rb], am[rb], al[rb]);
#pragma unroll
        for (int g = 0; g < 3; ++g) gwt_load_split(w_src + (int64_t)g * H * H + 32 * ks, wh[g], wm[g], wl[g]);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            GRU_MFMA6X3(acc[rb][0], acc[rb][1], acc[rb][2], ah[rb], am[rb], al[rb], ah[rb], am[rb], al[rb], ah[rb], am[rb], al[rb],
                        wh[0], wm[0], wl[0], wh[1], wm[1], wl[1], wh[2], wm[2], wl[2]);
        }
    }
}

// gwt_gemm3_rows on the tile's own rows: block rb's row `col` is row0 + 16 rb + col; rows past R repeat row R - 1.
template <int H, bool MASK>
__device__ __forceinline__ void gwt_gemm3(f32x4 (&acc)[2][3], const float *a, int64_t a_stride, const uint8_t *m, float keep_scale,
                                          const float *wmat, int row0, int unit0, int R, int w, int col, int quad) {
    const int64_t src[2] = {min(row0 + col, R - 1), min(row0 + 16 + col, R - 1)};
    gwt_gemm3_rows<H, MASK>(acc, a, a_stride, m, keep_scale, wmat, src, unit0, w, col, quad);
}

// The epilogue's elements: wave w takes row block w & 1 and elements 2 (w >> 1), 2 (w >> 1) + 1 of every lane's 16 x 16 result
// registers (tile rows 4 quad + i, as in gru_seq.hip), i.e. two batch rows of one hidden unit per lane.  Rows past R repeat row
// R - 1 as operands and are not live: they store nothing.
struct GwtElems {
    int rb, i0, unit;
    int64_t row[2];
    bool live[2];
};
__device__ __forceinline__ GwtElems gwt_elems(int w, int lane, int row0, int unit0, int R) {
    GwtElems e;
    e.rb = w & 1;
    e.i0 = 2 * (w >> 1);
    e.unit = unit0 + (lane & 15);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int r = row0 + 16 * e.rb + 4 * (lane >> 4) + e.i0 + k;
        e.live[k] = r < R;
        e.row[k] = e.live[k] ? r : R - 1;
    }
    return e;
}

// The waves' partial sums in LDS, NG accumulators per row block (8 KB each), and element i (GwtElems: i0, i0 + 1) of accumulator g of
// row block rb summed over the waves
template <int NG> using GwtRed = float[GWT_WAVES][2][NG][64][4];
template <int NG> __device__ __forceinline__ float gwt_wave_sum(const GwtRed<NG> &red, int rb, int g, int lane, int i) {
#pragma clang fp contract(off)
    float sum = red[0][rb][g][lane][i];
#pragma unroll
    for (int q = 1; q < GWT_WAVES; ++q) sum = sum + red[q][rb][g][lane][i];                            // wave order: deterministic
    return sum;
}

// One element of the forward step from its gate sums (the arithmetic of gru_seq_fwd_h2_kernel's element loop)
struct GwtGates {
    float r, z, n, ghn, hn;
};
__device__ __forceinline__ GwtGates gwt_gates(float gh_r, float gh_z, float gh_n, float gi_r, float gi_z, float gi_n, float bh_r, float bh_z,
                                              float bh_n, float h_prev) {
#pragma clang fp contract(off)               // GRU_ROUNDING (gru_common.h)
    GwtGates o;
    o.r = fast_sigmoid((gh_r + gi_r) + bh_r);
    o.z = fast_sigmoid((gh_z + gi_z) + bh_z);
    o.ghn = gh_n + bh_n;
    o.n = fast_tanh(__builtin_fmaf(o.r, o.ghn, gi_n));
    o.hn = __builtin_fmaf(o.z, h_prev, (1.f - o.z) * o.n);
    return o;
}

}  // namespace arvae
