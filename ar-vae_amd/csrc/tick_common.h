// What the one-launch tick decoders share (tick_decoder.hip: the free-running pass; beam_decoder.hip: the beam search): the recurrent
// matrices' two-term fp16 layout and its prep launches, the matrices' scales, the DPP row sum and the pitch of a row of logits in LDS.
#pragma once
#include "common.h"
#include "splitmath.h"
#include "gru_common.h"

namespace arvae {

// sum over the 16 lanes of a DPP row by the pairings of row16_max: both lanes of a pair add the same two values, so every lane ends
// with the same bits
template <int CTRL> __device__ __forceinline__ float dpp_pair_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v) {
    v = dpp_pair_add<0xB1>(v);
    v = dpp_pair_add<0x4E>(v);
    v = dpp_pair_add<0x141>(v);
    return dpp_pair_add<0x140>(v);
}

constexpr int FLT_LS = 68;                                     // floats between the logits' rows in LDS (16-byte reads, rows on their own banks)
constexpr int TICK_MAX_LAYERS = 4;
// the recurrent matrices of a free-running pass, in the order the kernels stream them: W_hh0, then per upper layer l its W_ih_l
// (2l - 1) and W_hh_l (2l); three for tick_free_run_h2_kernel, 2L - 1 for tick_free_run_layers_kernel
struct TickPrep {
    const float *w[2 * TICK_MAX_LAYERS - 1];
    int nmat;
    uint4 *out;
};

// largest magnitude of each matrix (one workgroup per matrix) -> wmax[matrix], behind the packed weights: the kernels' weight scales
// (round 5; a fixed 2^8 before, which overflowed fp16 for |w| >= 255)
template <int H>
__global__ __launch_bounds__(1024) void tick_amax_kernel(TickPrep p, float *__restrict__ wmax) {
    __shared__ float red[16];
    const float *w = p.w[blockIdx.x];
    float m = 0.f;
    for (int i = threadIdx.x; i < 3 * H * H / 4; i += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(w + 4 * i);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int q = 0; q < 16; ++q) t = fmaxf(t, red[q]);
        wmax[blockIdx.x] = t;
    }
}
// matrix m's scale: W_hh0 its own, an upper layer's pair (2l - 1, 2l) one between them (their products with the layer's operands share
// accumulators)
__device__ __forceinline__ Pow2 tick_scale(const float *wmax, int m) {
    const int first = ((m + 1) >> 1) * 2 - 1;
    return pow2_for(m == 0 ? wmax[0] : fmaxf(wmax[first], wmax[first + 1]));
}
// every matrix as scaled two-term fp16 in the per-lane order the kernels stream: uint4 ((m * KS + ks) * NW + w) * 6 + g * 2 + term of
// 64 lanes each, matrix major
template <int H>
__global__ __launch_bounds__(256) void tick_prep_kernel(TickPrep p, const float *__restrict__ wmax) {
    constexpr int NW = H / 16, KS = H / 32;
    const int tid = blockIdx.x * 256 + threadIdx.x;
    const int lane = tid & 63;
    int rest = tid >> 6;
    const int g = rest % 3; rest /= 3;
    const int w = rest % NW; rest /= NW;
    const int ks = rest % KS;
    const int m = rest / KS;
    if (m >= p.nmat) return;
    const int col = lane & 15, quad = lane >> 4;
    const float *src = p.w[m] + (int64_t)(g * H + 16 * w + col) * H + 32 * ks + 8 * quad;
    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(src), v1 = *reinterpret_cast<const f32x4 *>(src + 4);
    const float x[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    f16x8 hi, lo;
    split2_8<false>(x, tick_scale(wmax, m).s, hi, lo);
    uint4 *dst = p.out + ((int64_t)((m * KS + ks) * NW + w) * 6 + g * 2) * 64 + lane;
    dst[0] = __builtin_bit_cast(uint4, hi);
    dst[64] = __builtin_bit_cast(uint4, lo);
}

// the two prep launches of a call: the matrices' maxima behind the two-term layout (wmax = ws + 3 nmat H^2 floats), then the layout
template <int HH>
static void tick_prep_launch(const TickPrep &tp, float *ws, hipStream_t st) {
    float *wmax = ws + (int64_t)3 * tp.nmat * HH * HH;
    const int items = tp.nmat * (HH / 32) * (HH / 16) * 3 * 64;
    ARVAE_LAUNCH(tick_amax_kernel<HH>, dim3(tp.nmat), dim3(1024), 0, st, tp, wmax);
    ARVAE_LAUNCH(tick_prep_kernel<HH>, dim3((items + 255) / 256), dim3(256), 0, st, tp, wmax);
}

}  // namespace arvae
