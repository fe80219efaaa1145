// Device helpers the GRU kernel families share: the whole-sequence recurrences (gru_seq.hip) and the free-running tick decoder
// (tick_decoder.hip), and the host's choice of batch rows per workgroup both launch with.
#pragma once
#include "diag.h"
#include "common.h"
#include "splitmath.h"

namespace arvae {

// reciprocals on v_rcp_f32 (1 ulp): __frcp_rn is a correctly rounded division -- v_div_scale x 2, v_rcp, four fused steps,
// v_div_fmas, v_div_fixup -- and three of them per hidden unit and step were ~10 % of the forward recurrence's instructions
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) {
    // 1 - 2 / (1 + e^{2x}); saturates correctly at both ends (e -> inf gives 1, e -> 0 gives -1)
    return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x));
}

// GRU_ROUNDING: every batch row is an independent recurrence, so a row's results must not depend on the rows-per-workgroup
// instantiation that happens to run it.  The element arithmetic of gru_seq.hip therefore leaves no rounding to the compiler:
// `#pragma clang fp contract(off)` heads each element loop and the fused operations are written as __builtin_fmaf.  Left to the
// compiler, gru_seq_fwd_h2_kernel<H, 4> computed the new state as round((1 - z) n) + round(z h) (one packed multiply, one add)
// and <H, 8> as fma(z, h, round((1 - z) n)): the same rows one ulp apart between a 256-row and a 261-row batch
// (tests/test_gru_recurrences_float64.py holds the widths to each other bit for bit).
//
// Addressing of the recurrences' per-step memory operations: raw buffer operations, byte offset = a SCALAR part (the step's
// t * R * row pitch: one s_mul per array and step) + a per-lane part (row * pitch + unit: one v_mad_u32_u24 per operation).  With
// 64-bit pointer arithmetic each of a step's ~40 loads and stores cost 6-10 vector instructions -- half of what a wave executes
// per step in kernels that are bound by exactly that (16-32 workgroups on the chip, every step a chain of dependent phases).
// A null array is an empty range: its loads return zero and its stores are dropped, no branch; a lane drops a store with the
// per-lane offset GRU_DEAD (the hardware checks the per-lane offset + the instruction's immediate against the range; the scalar
// offset is NOT checked -- a step without an operation selects the empty range instead).  The entry points bound the arrays at
// GRU_RANGE bytes.
constexpr int GRU_RANGE = 0x7fff0000, GRU_DEAD = 0x7fff0000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gru_rsrc(const void *p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, p != nullptr ? GRU_RANGE : 0, 0x00020000);
}
__device__ __forceinline__ float gru_ld(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f32x4 gru_ld4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
__device__ __forceinline__ void gru_st(float v, __amdgpu_buffer_rsrc_t r, int voff, int soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff, soff, 0);
}
__device__ __forceinline__ int gru_off(int row, int pitch_bytes, int base_bytes) { return (int)__umul24(row, pitch_bytes) + base_bytes; }

template <int CTRL> __device__ __forceinline__ float dpp_max(float v) {
    const float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
    return fmaxf(v, o);
}
// maximum over the 16 lanes of a quad (a DPP row), in every lane: quad permutes, the half row and the row mirrored
__device__ __forceinline__ float row16_max(float v) {
    v = dpp_max<0xB1>(v);
    v = dpp_max<0x4E>(v);
    v = dpp_max<0x141>(v);
    return dpp_max<0x140>(v);
}
// Quad q's lanes receive element q of the f32x4 their column's lane in quad 0 holds (three swaps of register halves / quarters): the
// four live rows of a 16 x 16 MFMA result, one per lane.
// (inline assembly: through __builtin_amdgcn_permlane16_swap / _permlane32_swap this compiler fed the first swap the SAME register
// twice when only one half of the builtin's result pair was used, and declared the other three accumulator registers dead -- quads 1-3
// then received element 0; tools/probes/permlane_swap.hip shows the instructions themselves do what the ISA says.  The s_nop in front
// covers an MFMA result read by a vector instruction the compiler's hazard recogniser does not see: 8 passes + 2.)
__device__ __forceinline__ float spread_rows(const f32x4 &a) {
    float x0 = a[0], x1 = a[1], x2 = a[2], x3 = a[3];
    asm volatile("s_nop 15\n\t"
                 "v_permlane16_swap_b32 %0, %1\n\t"              // x0 = [a0.q0 | a1.q0 | a0.q2 | a1.q2]
                 "v_permlane16_swap_b32 %2, %3\n\t"              // x2 = [a2.q0 | a3.q0 | a2.q2 | a3.q2]
                 "s_nop 1\n\t"
                 "v_permlane32_swap_b32 %0, %2\n\t"              // x0 = [a0.q0 | a1.q0 | a2.q0 | a3.q0]
                 "s_nop 1"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
    return x0;
}

// RW 8: quads 0 and 1 hold the eight live rows; their elements 2 and 3 go to quads 2 and 3 (one swap of register halves each)
__device__ __forceinline__ void spread_pairs(const f32x4 &a, float &o0, float &o1) {
    float x0 = a[0], x1 = a[1], x2 = a[2], x3 = a[3];
    asm volatile("s_nop 15\n\t"
                 "v_permlane32_swap_b32 %0, %2\n\t"              // x0 = [a0.q0 | a0.q1 | a2.q0 | a2.q1]
                 "v_permlane32_swap_b32 %1, %3\n\t"              // x1 = [a1.q0 | a1.q1 | a3.q0 | a3.q1]
                 "s_nop 1"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
    o0 = x0;
    o1 = x1;
}
// E = RW / 4 elements per lane: the tile row of a lane's element i, the tile row a lane reads its A operand from (rows past the live
// ones repeat them), a 16 x 16 result's values for the lane's elements
template <int E> __device__ __forceinline__ int gru_lrow(int quad, int i) {
    return E == 4 ? 4 * quad + i : E == 2 ? 4 * (quad & 1) + 2 * (quad >> 1) + i : quad;
}
template <int E> __device__ __forceinline__ int gru_arow(int col) { return E == 4 ? col : E == 2 ? (col & 7) : (col & 3); }
template <int E> __device__ __forceinline__ void gru_elems(const f32x4 &acc, float (&out)[E]) {
    if constexpr (E == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = acc[i];
    } else if constexpr (E == 2) {
        spread_pairs(acc, out[0], out[1]);
    } else {
        out[0] = spread_rows(acc);
    }
}

// RW: batch rows per workgroup, 16, 8 or 4.  A recurrence is a chain of T dependent steps whose length is the instruction stream of one
// wave between two barriers, and most of that stream is per (row, hidden unit) ELEMENT work: projections in,
// gates, the state's split and its LDS writes, h and the saved gates out -- four elements per lane when a workgroup owns 16 rows.
// With 4 rows per workgroup the 16 x 16 MFMA tile is three quarters empty (the matrix pipe was idle anyway), the four live rows of
// a result go out to the four quads (spread_rows) and every lane does ONE element per step; four times the workgroups, on a chip
// that the recurrences of a 256-measure batch fill to an eighth.  The host picks the smallest of 4, 8, 16 whose workgroups are all on
// the chip at once (8: two elements per lane, the live rows in quads 0 and 1).
// ARVAE_GRU_WIDE=1 (diagnostic build): always sixteen, as through round 4
inline int gru_rows_per_wg(int rows, int nseq) {
    static const bool wide = diag_env("ARVAE_GRU_WIDE") != nullptr;
    if (wide) return 16;
    for (int rw = 4; rw < 16; rw *= 2)
        if ((int64_t)((rows + rw - 1) / rw) * nseq <= device_cu_count()) return rw;
    return 16;
}

}  // namespace arvae
