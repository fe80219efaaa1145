// Free-running pass of the two-layer tick decoder at hidden sizes 256 and 512 with STREAMED weights: one library call enqueues every
// tick on the caller's stream, THREE LAUNCHES PER TICK (layer 0, layer 1, logits + pick).  tick_decoder.hip keeps the recurrent
// weights in registers and one workgroup walks all ticks of its rows; at these sizes the weights do not fit (gru_wide.hip), the units
// of a row are spread over many workgroups, and a tick needs every unit of the tick before it, so gru_wide.hip's rule holds: the
// step boundary is the launch boundary, no kernel waits for another workgroup (no flags, no spin loops, no grid barrier, no
// cooperative launch), and the call neither allocates nor synchronises nor reads back.  A launch per step cannot hang.
//
// Rows = batch (the fed-back note carries across beats, so the beats are not independent here).  Per tick t = tpb * beat + j:
//   layer 0   gru_wide_fwd_step_kernel's tiling and arithmetic (32 rows x 16 units x three gates per workgroup, four waves split K,
//             three-term bf16 operands, partial sums added in wave order, GRU_ROUNDING); the input projection is never materialised:
//             gi0 = ptab[previous note] + gib[beat * B + row], read and added in the epilogue.  h_prev = h0_l0[beat] at j == 0.
//   layer 1   the same tile; gi1 = (h_l0' (.) keep-mask * keep_scale) W_ih1^T and gh1 = h_l1_prev W_hh1^T in one launch, one K loop
//             each, gi_n and gh_n kept apart.  The keep-mask is applied to the operand in fp32 before the split: (keep_scale * x) * m,
//             scale_mask_kernel's product.
//   out       16 rows x the whole vocabulary per workgroup: logits = relu(W_out h_l1' + b_out) with the waves splitting the
//             vocabulary's 16-note tiles (each its whole K: nothing to add across waves), then the rows' picks from LDS.
// The states of a tick live in the workspace (two buffers per layer: a launch reads the tick before while other workgroups write
// this one), and so does the int32 previous note of every row.
//
// The pick is sequence.hip's row kernels' on the same logits, bit for bit: the maximum, e_v = expf((l_v - max) * inv_t), and every
// sum of e in INDEX ORDER, as row_sample_kernel / row_sample_filtered_kernel add them.  What those kernels recompute per use (e_v,
// a note's rank and the mass ordered before it) is computed once per note by all 256 threads and kept in LDS -- the same values,
// since every one of them is a function of the row's logits alone -- and the sums that fix the result are walked by one thread per
// row in the row kernels' order.  No expression here pairs a multiplication with an addition, so there is nothing to contract.
//
// All addressing is 64-bit.  Rows past the batch repeat row B - 1 as operands and store nothing; notes past the vocabulary repeat
// note V - 1 as operands and are never read back.
#include <cmath>
#include "common.h"
#include "dispatch.h"
#include "splitmath.h"
#include "gru_common.h"

namespace arvae {

constexpr int TW_RT = 32;                  // batch rows per workgroup of the two recurrence kernels (GW_RT of gru_wide.hip)
constexpr int TW_WAVES = 4;
constexpr int TW_ORT = 16;                 // batch rows per workgroup of the logits + pick kernel
constexpr int TW_VMAX = 128;               // notes: eight 16-note tiles, two per wave

enum { TW_ARGMAX = 0, TW_SAMPLE = 1, TW_FILTERED = 2 };

// GRU_MFMA6X3's six products (splitmath.h), in its order, on one accumulator
#define TW_MFMA6(ACC, AH, AM, AL, WH, WM, WL)                                    \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AL, WH, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, WL, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AM, WM, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AM, WH, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, WM, ACC, 0, 0, 0);         \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, WH, ACC, 0, 0, 0)

struct TickWide {
    const float *w_hh0, *b_hh0, *w_ih1, *b_ih1, *w_hh1, *b_hh1, *w_out, *b_out;
    const float *h0_l0, *h0_l1, *gib, *ptab, *uniforms;
    const uint8_t *mask, *allow;           // keep-mask [ticks][B][H]; allowed notes (a filter's: both strides 0; a plan's)
    float *hs0, *hs1;                      // workspace: the layers' states, [2][B][H] each
    int *prev;                             // workspace: the rows' previous notes
    int64_t *tokens;
    float *logits;                         // [B][ticks][V] or null
    int64_t h0_stride, allow_row, allow_tick;
    float keep_scale, inv_t, top_p;
    int batch, tpb, ticks, vocab, top_k;
};

// eight consecutive floats (16-byte aligned) -> their three bf16 operand registers; MASK: times keep_scale and the eight keep bytes
template <bool MASK>
__device__ __forceinline__ void tw_load_split(const float *p, const uint8_t *m, float keep_scale, bf16x8 &hi, bf16x8 &mid, bf16x8 &lo) {
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

// a wave's quarter of K of  acc[rb][g] += a[rows of block rb][:] . wmat[g H + unit tile][:]^T  (gru_wide_fwd_step_kernel's loop):
// A: lane (col, quad) holds row `col` of a 16-row block, k = 8 quad .. 8 quad + 7 of the k-step; rows past R repeat row R - 1.
// B: lane (col, quad) holds unit `col` of the tile, the same k.
template <int H, bool MASK>
__device__ __forceinline__ void tw_gemm3(f32x4 (&acc)[2][3], const float *a, int64_t a_stride, const uint8_t *m, float keep_scale,
                                         const float *wmat, int row0, int unit0, int R, int w, int col, int quad) {
    constexpr int KW = H / TW_WAVES, KS = KW / 32;
    static_assert(KS >= 1, "whole k-steps per wave");
    const float *a_src[2];
    const uint8_t *m_src[2] = {nullptr, nullptr};
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const int64_t r = min(row0 + 16 * rb + col, R - 1);
        a_src[rb] = a + r * a_stride + w * KW + 8 * quad;
        if constexpr (MASK) m_src[rb] = m + r * H + w * KW + 8 * quad;
    }
    const float *w_src = wmat + (int64_t)(unit0 + col) * H + w * KW + 8 * quad;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 ah[2], am[2], al[2], wh[3], wm[3], wl[3];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) tw_load_split<MASK>(a_src[rb] + 32 * ks, MASK ? m_src[rb] + 32 * ks : nullptr, keep_scale, ah[rb], am[rb], al[rb]);
#pragma unroll
        for (int g = 0; g < 3; ++g) tw_load_split<false>(w_src + (int64_t)g * H * H + 32 * ks, nullptr, 1.f, wh[g], wm[g], wl[g]);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            GRU_MFMA6X3(acc[rb][0], acc[rb][1], acc[rb][2], ah[rb], am[rb], al[rb], ah[rb], am[rb], al[rb], ah[rb], am[rb], al[rb],
                        wh[0], wm[0], wl[0], wh[1], wm[1], wl[1], wh[2], wm[2], wl[2]);
        }
    }
}

// The epilogue's elements (gw_elems of gru_wide.hip): wave w takes row block w & 1 and elements 2 (w >> 1), 2 (w >> 1) + 1 of every
// lane's 16 x 16 result registers (tile rows 4 quad + i), i.e. two batch rows of one hidden unit per lane.
struct TwElems {
    int rb, i0, unit;
    int64_t row[2];
    bool live[2];
};
__device__ __forceinline__ TwElems tw_elems(int w, int lane, int row0, int unit0, int R) {
    TwElems e;
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

// ------------------------------------------------------------------------------------------------------------------
// Layer 0 of tick t: gh = h_prev . W_hh0^T for the tile, gi = ptab[previous note] + gib[beat], then r, z, n, h'.
template <int H>
__global__ __launch_bounds__(64 * TW_WAVES) void tick_wide_l0_kernel(TickWide p, int t) {
    constexpr int NU = H / 16;
    static_assert(NU % 8 == 0, "unit tiles in multiples of the XCD count");
    __shared__ __attribute__((aligned(16))) float red[TW_WAVES][2][3][64][4];           // 24 KB
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * TW_RT, unit0 = 16 * (blockIdx.x % NU);
    const int R = p.batch, beat = t / p.tpb;
    const bool restart = t % p.tpb == 0;
    const float *hp = restart ? p.h0_l0 + (int64_t)beat * R * p.h0_stride : p.hs0 + (int64_t)((t + 1) & 1) * R * H;
    const int64_t hp_stride = restart ? p.h0_stride : H;
    float *out = p.hs0 + (int64_t)(t & 1) * R * H;

    // the epilogue's operands are requested first: they arrive while the GEMM runs
    const TwElems e = tw_elems(w, lane, row0, unit0, R);
    float gi[2][3], hprev[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t note = t == 0 ? p.vocab : p.prev[e.row[k]];
        const float *a = p.ptab + note * (3 * H) + e.unit, *b = p.gib + ((int64_t)beat * R + e.row[k]) * (3 * H) + e.unit;
#pragma unroll
        for (int g = 0; g < 3; ++g) gi[k][g] = a[g * H] + b[g * H];
        hprev[k] = hp[e.row[k] * hp_stride + e.unit];
    }
    const float bh_r = p.b_hh0[e.unit], bh_z = p.b_hh0[H + e.unit], bh_n = p.b_hh0[2 * H + e.unit];

    f32x4 acc[2][3];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[rb][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    tw_gemm3<H, false>(acc, hp, hp_stride, nullptr, 1.f, p.w_hh0, row0, unit0, R, w, col, quad);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int g = 0; g < 3; ++g) *reinterpret_cast<f32x4 *>(red[w][rb][g][lane]) = acc[rb][g];
    lds_barrier();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma clang fp contract(off)               // GRU_ROUNDING (gru_common.h)
        float gh[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            float sum = red[0][e.rb][g][lane][e.i0 + k];
#pragma unroll
            for (int q = 1; q < TW_WAVES; ++q) sum = sum + red[q][e.rb][g][lane][e.i0 + k];           // wave order: deterministic
            gh[g] = sum;
        }
        const float r = fast_sigmoid((gh[0] + gi[k][0]) + bh_r);
        const float z = fast_sigmoid((gh[1] + gi[k][1]) + bh_z);
        const float ghn = gh[2] + bh_n;
        const float n = fast_tanh(__builtin_fmaf(r, ghn, gi[k][2]));
        const float hn = __builtin_fmaf(z, hprev[k], (1.f - z) * n);
        if (e.live[k]) out[e.row[k] * H + e.unit] = hn;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Layer 1 of tick t: gi = (h_l0' (.) keep-mask * keep_scale) . W_ih1^T + b_ih1 and gh = h_l1_prev . W_hh1^T + b_hh1, then the gates.
template <int H, bool MASK>
__global__ __launch_bounds__(64 * TW_WAVES) void tick_wide_l1_kernel(TickWide p, int t) {
    constexpr int NU = H / 16;
    __shared__ __attribute__((aligned(16))) float red[TW_WAVES][2][6][64][4];           // 48 KB: gates 0-2 of gi, 3-5 of gh
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * TW_RT, unit0 = 16 * (blockIdx.x % NU);
    const int R = p.batch, beat = t / p.tpb;
    const bool restart = t % p.tpb == 0;
    const float *x = p.hs0 + (int64_t)(t & 1) * R * H;                                   // layer 0's state of this tick
    const float *hp = restart ? p.h0_l1 + (int64_t)beat * R * p.h0_stride : p.hs1 + (int64_t)((t + 1) & 1) * R * H;
    const int64_t hp_stride = restart ? p.h0_stride : H;
    float *out = p.hs1 + (int64_t)(t & 1) * R * H;

    const TwElems e = tw_elems(w, lane, row0, unit0, R);
    float hprev[2], bi[3], bh[3];
#pragma unroll
    for (int k = 0; k < 2; ++k) hprev[k] = hp[e.row[k] * hp_stride + e.unit];
#pragma unroll
    for (int g = 0; g < 3; ++g) { bi[g] = p.b_ih1[g * H + e.unit]; bh[g] = p.b_hh1[g * H + e.unit]; }

    f32x4 acc[2][3];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[rb][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (half == 0) tw_gemm3<H, MASK>(acc, x, H, MASK ? p.mask + (int64_t)t * R * H : nullptr, p.keep_scale, p.w_ih1, row0, unit0, R, w, col, quad);
        else tw_gemm3<H, false>(acc, hp, hp_stride, nullptr, 1.f, p.w_hh1, row0, unit0, R, w, col, quad);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 3; ++g) *reinterpret_cast<f32x4 *>(red[w][rb][3 * half + g][lane]) = acc[rb][g];
    }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma clang fp contract(off)               // GRU_ROUNDING (gru_common.h)
        float s[6];
#pragma unroll
        for (int g = 0; g < 6; ++g) {
            float sum = red[0][e.rb][g][lane][e.i0 + k];
#pragma unroll
            for (int q = 1; q < TW_WAVES; ++q) sum = sum + red[q][e.rb][g][lane][e.i0 + k];           // wave order: deterministic
            s[g] = sum;
        }
        const float gi_r = s[0] + bi[0], gi_z = s[1] + bi[1], gi_n = s[2] + bi[2];
        const float r = fast_sigmoid((s[3] + gi_r) + bh[0]);
        const float z = fast_sigmoid((s[4] + gi_z) + bh[1]);
        const float ghn = s[5] + bh[2];
        const float n = fast_tanh(__builtin_fmaf(r, ghn, gi_n));
        const float hn = __builtin_fmaf(z, hprev[k], (1.f - z) * n);
        if (e.live[k]) out[e.row[k] * H + e.unit] = hn;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Logits of tick t for 16 rows and the rows' picks.  Wave w computes the 16-note tiles w and w + 4 over the whole K.
template <int H, int PICK>
__global__ __launch_bounds__(64 * TW_WAVES) void tick_wide_out_kernel(TickWide p, int t) {
    constexpr int KS = H / 32;
    __shared__ float lg[TW_ORT][TW_VMAX + 1];                  // the logits; with PICK >= 1 also:
    __shared__ float ev[TW_ORT][TW_VMAX + 1];                  //   e_v (0 for a note that is not allowed)
    __shared__ float bf[TW_ORT][TW_VMAX + 1];                  //   the e of the notes ordered before v, in index order
    __shared__ short rk[TW_ORT][TW_VMAX + 2];                  //   v's rank among the allowed notes
    __shared__ uint8_t on[TW_ORT][TW_VMAX + 4];                //   v is allowed
    __shared__ float mxs[TW_ORT];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int R = p.batch, V = p.vocab, row0 = blockIdx.x * TW_ORT;
    const int ntile = (V + 15) / 16;
    const float *hs = p.hs1 + (int64_t)(t & 1) * R * H;       // layer 1's state of this tick

    {
        const float *a_src = hs + (int64_t)min(row0 + col, R - 1) * H + 8 * quad;
        const float *w_src[2];
        bool have[2];
        f32x4 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            have[i] = w + 4 * i < ntile;                       // (uniform over the wave)
            w_src[i] = p.w_out + (int64_t)min(16 * (w + 4 * i) + col, V - 1) * H + 8 * quad;
            acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (have[0]) {
#pragma unroll 4
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 ah, am, al, wh, wm, wl;
                tw_load_split<false>(a_src + 32 * ks, nullptr, 1.f, ah, am, al);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (!have[i]) continue;
                    tw_load_split<false>(w_src[i] + 32 * ks, nullptr, 1.f, wh, wm, wl);
                    TW_MFMA6(acc[i], ah, am, al, wh, wm, wl);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int v = 16 * (w + 4 * i) + col;
            if (!have[i] || v >= V) continue;
            const float b = p.b_out[v];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = 4 * quad + k;
                const float l = fmaxf(acc[i][k] + b, 0.f);
                lg[r][v] = l;
                if (p.logits != nullptr && row0 + r < R) p.logits[((int64_t)(row0 + r) * p.ticks + t) * V + v] = l;
            }
        }
    }
    __syncthreads();

    const int tid = threadIdx.x;
    const int64_t grow = min(row0 + tid, R - 1);               // (the picking threads: tid < TW_ORT)
    const bool picks = tid < TW_ORT && row0 + tid < R;
    int arg = 0;
    if constexpr (PICK == TW_ARGMAX) {                         // row_argmax_kernel
        if (picks) {
            float mx = lg[tid][0];
            for (int j = 1; j < V; ++j)
                if (lg[tid][j] > mx) { mx = lg[tid][j]; arg = j; }
        }
    } else {
        const float inv_t = p.inv_t;
        if constexpr (PICK == TW_FILTERED) {
            for (int i = tid; i < TW_ORT * V; i += 64 * TW_WAVES) {
                const int r = i / V, j = i - r * V;
                const uint8_t *allow = p.allow != nullptr ? p.allow + (int64_t)min(row0 + r, R - 1) * p.allow_row + (int64_t)t * p.allow_tick : nullptr;
                on[r][j] = allow == nullptr || allow[j] != 0;
            }
            __syncthreads();
        }
        if (tid < TW_ORT) {
            float mx;
            if constexpr (PICK == TW_FILTERED) {
                mx = -INFINITY;
                for (int j = 0; j < V; ++j)
                    if (on[tid][j]) mx = fmaxf(mx, lg[tid][j]);
            } else {
                mx = lg[tid][0];
                for (int j = 1; j < V; ++j) mx = fmaxf(mx, lg[tid][j]);
            }
            mxs[tid] = mx;
        }
        __syncthreads();
        for (int i = tid; i < TW_ORT * V; i += 64 * TW_WAVES) {
            const int r = i / V, j = i - r * V;
            const bool live = PICK != TW_FILTERED || on[r][j];
            ev[r][j] = live ? expf((lg[r][j] - mxs[r]) * inv_t) : 0.f;
        }
        __syncthreads();
        if constexpr (PICK == TW_SAMPLE) {                     // row_sample_kernel
            if (picks) {
                float total = 0.f;
                for (int j = 0; j < V; ++j) total += ev[tid][j];
                const float target = p.uniforms[grow * p.ticks + t] * total;
                float c = 0.f;
                arg = V - 1;
                for (int j = 0; j < V; ++j) {
                    c += ev[tid][j];
                    if (c >= target) { arg = j; break; }
                }
            }
        } else {                                               // row_sample_filtered_kernel
            for (int i = tid; i < TW_ORT * V; i += 64 * TW_WAVES) {
                const int r = i / V, j = i - r * V;
                if (!on[r][j]) continue;
                const float lj = lg[r][j];
                int rank = 0;
                float before = 0.f;
                for (int n = 0; n < V; ++n) {
                    const float ln = lg[r][n];
                    const bool first = on[r][n] && (ln > lj || (ln == lj && n < j));
                    rank += first ? 1 : 0;
                    before += first ? ev[r][n] : 0.f;
                }
                rk[r][j] = (short)rank;
                bf[r][j] = before;
            }
            __syncthreads();
            if (picks) {
                const int top_k = p.top_k;
                const float top_p = p.top_p;
                float s = 0.f;
                for (int j = 0; j < V; ++j)
                    if (on[tid][j] && rk[tid][j] < top_k) s += ev[tid][j];
                const float cut = top_p * s;
                float cut_l = INFINITY;
                int cut_i = -1;
                for (int j = 0; j < V; ++j) {
                    if (!on[tid][j]) continue;
                    const float lj = lg[tid][j];
                    const bool keep = rk[tid][j] < top_k && (top_p >= 1.f || bf[tid][j] < cut);
                    if (keep && (lj < cut_l || (lj == cut_l && j > cut_i))) { cut_l = lj; cut_i = j; }
                }
                auto kept = [&](int j) { return on[tid][j] && (lg[tid][j] > cut_l || (lg[tid][j] == cut_l && j <= cut_i)); };
                float total = 0.f;
                for (int j = 0; j < V; ++j)
                    if (kept(j)) total += ev[tid][j];
                const float target = p.uniforms[grow * p.ticks + t] * total;
                float c = 0.f;
                for (int j = 0; j < V; ++j) {
                    if (!kept(j)) continue;
                    c += ev[tid][j];
                    arg = j;                                   // (the walk repeats the total's additions: it ends on a survivor)
                    if (c >= target) break;
                }
            }
        }
    }
    if (picks) {
        p.tokens[grow * p.ticks + t] = arg;
        p.prev[grow] = arg;
    }
}

static bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }
static int64_t tw_prev_floats(int64_t batch) { return (batch + 3) / 4 * 4; }

}  // namespace arvae

using namespace arvae;

extern "C" int arvae_tick_free_run_wide_supported(int32_t hidden, int32_t vocab) {
    return (hidden == 256 || hidden == 512) && vocab >= 2 && vocab <= TW_VMAX;
}

// the two layers' states of a tick, twice (the tick before is read while this one is written), and the rows' previous notes
extern "C" int64_t arvae_tick_free_run_wide_ws_floats(int32_t batch, int32_t hidden, int32_t vocab) {
    if (batch < 1 || !arvae_tick_free_run_wide_supported(hidden, vocab)) return -1;
    return 4 * (int64_t)batch * hidden + tw_prev_floats(batch);
}

extern "C" int arvae_tick_free_run_wide(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                        const float *gib, const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch,
                                        int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms,
                                        float inv_temperature, const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan,
                                        int64_t *tokens, float *logits_out, float *ws, arvae_stream_t stream) {
    ARVAE_REQUIRE(wts && h0_l0 && h0_l1 && gib && ptab && tokens, "tick_free_run_wide: null pointer");
    ARVAE_REQUIRE(wts->w_hh0 && wts->b_hh0 && wts->w_ih1 && wts->b_ih1 && wts->w_hh1 && wts->b_hh1 && wts->w_out && wts->b_out,
                  "tick_free_run_wide: null weight pointer");
    ARVAE_REQUIRE(batch >= 1 && beats >= 1 && ticks_per_beat >= 1, "tick_free_run_wide: empty problem");
    ARVAE_REQUIRE((int64_t)beats * ticks_per_beat <= INT32_MAX, "tick_free_run_wide: %lld ticks", (long long)beats * ticks_per_beat);
    ARVAE_REQUIRE(hidden == 256 || hidden == 512, "tick_free_run_wide: hidden size %d is not built (256, 512)", hidden);
    ARVAE_REQUIRE(arvae_tick_free_run_wide_supported(hidden, vocab), "tick_free_run_wide: a vocabulary of %d notes is outside [2, %d]", vocab,
                  TW_VMAX);
    ARVAE_REQUIRE(std::isfinite(inv_temperature) && inv_temperature > 0.f,
                  "tick_free_run_wide: inverse temperature %f is not a positive finite number", (double)inv_temperature);
    int pick = uniforms != nullptr ? TW_SAMPLE : TW_ARGMAX, top_k = vocab;
    if (filter != nullptr || plan != nullptr) {
        bool active = false;
        if (const int rc = sample_filter_check("tick_free_run_wide", filter, vocab, &top_k, &active)) return rc;
        ARVAE_REQUIRE(uniforms != nullptr, "tick_free_run_wide: null uniforms");
        ARVAE_REQUIRE(mask == nullptr, "tick_free_run_wide: a dropout keep-mask was given together with a filter or a plan (generation runs "
                                       "with dropout off)");
        if (plan != nullptr) {
            ARVAE_REQUIRE(filter->allow == nullptr, "tick_free_run_wide: filter->allow is set (with a plan the allowed mask is folded into the plan)");
            if (const int rc = note_plan_check("tick_free_run_wide", plan, (int64_t)beats * ticks_per_beat, vocab)) return rc;
        }
        if (active || plan != nullptr) pick = TW_FILTERED;
    }
    ARVAE_REQUIRE(ws != nullptr && aligned16(ws), "tick_free_run_wide: workspace missing or not 16-byte aligned (arvae_tick_free_run_wide_ws_floats)");
    ARVAE_REQUIRE(aligned16(wts->w_hh0) && aligned16(wts->w_ih1) && aligned16(wts->w_hh1) && aligned16(wts->w_out) && aligned16(h0_l0) &&
                      aligned16(h0_l1),
                  "tick_free_run_wide: w_hh0, w_ih1, w_hh1, w_out, h0_l0 and h0_l1 must be 16-byte aligned");
    ARVAE_REQUIRE(h0_stride % 4 == 0 && (h0_stride == 0 || h0_stride >= hidden),
                  "tick_free_run_wide: h0_stride %lld is no multiple of 4 floats or below the hidden size", (long long)h0_stride);
    ARVAE_REQUIRE(mask == nullptr || (reinterpret_cast<uintptr_t>(mask) & 3u) == 0, "tick_free_run_wide: the keep-mask must be 4-byte aligned");

    TickWide p{};
    p.w_hh0 = wts->w_hh0; p.b_hh0 = wts->b_hh0; p.w_ih1 = wts->w_ih1; p.b_ih1 = wts->b_ih1;
    p.w_hh1 = wts->w_hh1; p.b_hh1 = wts->b_hh1; p.w_out = wts->w_out; p.b_out = wts->b_out;
    p.h0_l0 = h0_l0; p.h0_l1 = h0_l1; p.h0_stride = h0_stride != 0 ? h0_stride : hidden; p.gib = gib; p.ptab = ptab;
    p.uniforms = uniforms; p.mask = mask; p.keep_scale = keep_scale; p.inv_t = inv_temperature;
    p.batch = batch; p.tpb = ticks_per_beat; p.ticks = beats * ticks_per_beat; p.vocab = vocab;
    p.tokens = tokens; p.logits = logits_out;
    p.hs0 = ws; p.hs1 = ws + 2 * (int64_t)batch * hidden;
    p.prev = reinterpret_cast<int *>(ws + 4 * (int64_t)batch * hidden);
    p.top_k = top_k; p.top_p = filter != nullptr ? filter->top_p : 1.f;
    if (plan != nullptr) { p.allow = plan->allow; p.allow_row = plan->row_stride; p.allow_tick = plan->tick_stride; }
    else if (filter != nullptr) p.allow = filter->allow;

    hipStream_t st = as_stream(stream);
    const dim3 block(64 * TW_WAVES), grid((batch + TW_RT - 1) / TW_RT * (hidden / 16)), grid_out((batch + TW_ORT - 1) / TW_ORT);
    const bool known = with_int<256, 512>(hidden, [&](auto HH) {
        constexpr int H = decltype(HH)::value;
        for (int t = 0; t < p.ticks; ++t) {
            ARVAE_LAUNCH((tick_wide_l0_kernel<H>), grid, block, 0, st, p, t);
            if (mask != nullptr) ARVAE_LAUNCH((tick_wide_l1_kernel<H, true>), grid, block, 0, st, p, t);
            else ARVAE_LAUNCH((tick_wide_l1_kernel<H, false>), grid, block, 0, st, p, t);
            if (pick == TW_ARGMAX) ARVAE_LAUNCH((tick_wide_out_kernel<H, TW_ARGMAX>), grid_out, block, 0, st, p, t);
            else if (pick == TW_SAMPLE) ARVAE_LAUNCH((tick_wide_out_kernel<H, TW_SAMPLE>), grid_out, block, 0, st, p, t);
            else ARVAE_LAUNCH((tick_wide_out_kernel<H, TW_FILTERED>), grid_out, block, 0, st, p, t);
        }
    });
    ARVAE_REQUIRE(known, "tick_free_run_wide: no kernel for hidden size %d", hidden);
    return check_launch("tick_wide_out_kernel");
}
