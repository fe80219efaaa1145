// Whole-sequence GRU kernels of the MeasureVAE path: all T time steps of one GRU layer (any number of independent
// directions / parameter sets) in ONE launch, forward and backward-through-time.
//
// Reference: nn.GRU inside measurevae/encoder.py:27-34,113-118 (2-layer bidirectional, 24 ticks) and
// measurevae/decoder.py:338-368,436-525 (beat RNN 4 steps, tick RNN 6 steps per beat), gate order r | z | n:
//     r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(gi_n + r * gh_n);  h' = (1-z)*n + z*h
// with gi = W_ih x + b_ih computed for all time steps by one dense launch beforehand and gh = W_hh h + b_hh here.
//
// Every batch row is an independent recurrence, so a workgroup owns 16 rows for the whole sequence and never talks
// to another workgroup: H/16 waves, wave w owns hidden units [16w, 16w+16) of all three gates and keeps its
// 3 x 16 x H slice of W_hh in registers (96 VGPRs at H = 128) for all T steps.  Per step: h (16 x H, LDS, double
// buffered) times the slice on v_mfma_f32_16x16x4_f32 (the 16x16 result tile = 4 rows x 1 unit per lane for each
// gate, so the gate math is lane-local), the new h goes back to LDS, one barrier.  gi of the next step is prefetched
// while the MFMAs run.  The backward kernel keeps W_hh^T the same way and carries dL/dh in registers.
//
// The weight gradients (dW_hh = dgh^T h_prev, dW_ih = dgi^T x) and the input gradients are ordinary dense launches
// over all T*R rows afterwards (ops.py).
#include <algorithm>
#include <cmath>
#include "diag.h"
#include "common.h"
#include "dispatch.h"
#include "splitmath.h"
#include "gru_common.h"
#include "gru_mask.h"
#include "stamps.h"

namespace arvae {

constexpr int GRU_SEQ_MAX = 4;

struct GruSeq {
    // forward
    const float *gi;        // [T][R][3H]  (gi_tstride floats between steps; 0 = the same block every step)
    int64_t gi_tstride;
    const float *w_hh;      // [3H][H]
    const float *b_hh;      // [3H]
    const float *h0;        // [R][H] or null (zeros)
    float *h_all;           // h of step t, row r, unit j at h_all[(t*R + r) * h_stride + j]
    int64_t h_stride;
    float *saved;           // [T][R][H][4] : r, z, n, gh_n
    int reverse;            // process t = T-1 .. 0
    // backward
    const float *dh_all;    // gradient w.r.t. h_all, same addressing with dh_stride; may be null
    int64_t dh_stride;
    float *dgi;             // [T][R][3H]
    float *dgh;             // [T][R][3H]
    float *dh0;             // [R][H] or null
    const float *dh_last;   // gradient w.r.t. the final state (h of the last processed step), [R] rows of dh_last_stride; may be null
    int64_t dh_last_stride;
    float *h_prev_out;      // [T][R][H]: h entering step t (the operand of the W_hh weight gradient); may be null
    // merged projections (both directions of a layer as ONE GEMM write / read [T][R][ndir * 3H]): floats between two rows of gi /
    // of dgi (fill_batch sets 3H when the caller leaves them 0)
    int64_t gi_rstride, dgi_rstride;
    float *h_fin;           // forward, optional: the state after the last processed step, row r at h_fin + r * h_fin_stride
    int64_t h_fin_stride;
    int64_t h0_stride, dh0_stride;   // floats between two rows of h0 / dh0 (fill_batch: H when the caller leaves them 0)
    // dropout on the sequence's output (gru_mask.h; the fp16 two-term kernels only): mask null = none
    const uint8_t *mask;
    float keep;
    float *h_masked;
    int hm_stride, mk_tstride, mk_rstride, mk_gstride, mk_group;
};
struct GruSeqBatch {
    GruSeq seq[GRU_SEQ_MAX];
};

#ifdef ARVAE_STAMPS_GRU
// diagnostic build only (stamps.h): cycles per phase of a step + the step count, of the LAST forward or backward launch: thread 0 /
ARVAE_STAMP_TABLE(gru, 1, 5, 1)                                // wave GRU_STAMP_WAVE of the first workgroup
#define GSTAMP_BEGIN() PhaseSums<4> ph
#define GSTAMP(k) ph.mark(k)
#define GSTAMP_DEPEND(v) stamp_depend(v)
#define GSTAMP_WAIT(what) stamp_wait_##what()
#define GSTAMP_END(wave, steps) do { if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 64 * (wave)) ph.flush(g_gru_stamps, steps); } while (0)
#else
#define GSTAMP_BEGIN()
#define GSTAMP(k)
#define GSTAMP_DEPEND(v)
#define GSTAMP_WAIT(what)
#define GSTAMP_END(wave, steps)
#endif
// ------------------------------------------------------------------------------------------------------------------
// The forward recurrence on the fp16 MFMA with SCALED TWO-TERM operands (the arithmetic of splitmath.h): s x = h + l with
// h = fp16(s x), l = fp16(s x - h), a product = the three partial products l h', h l', h h' on v_mfma_f32_16x16x32_f16, smallest
// first -- half the MFMAs and two thirds of the LDS operand bytes of the three-term bf16 split at the same accuracy (2^-22 per
// product; measured against float64: splitmath.h).  fp16 has 5 exponent bits, so the scales must place the operands.
// The SEQUENCE kernels take every scale from the data (round 5): W_hh's slice of a wave its own power of two (a column's scale
// factors out of the dot product), the state the workgroup's max(1, max |h0|) -- a bound for the whole sequence, h_t being a convex
// combination of a tanh output and h_(t-1) --, the backward pass's gradients a scale per batch row and step (gru_seq_bwd_h2_kernel):
// nothing can overflow.  The FREE-RUNNING decoder (tick_decoder.hip) takes its scales from the data as well: the matrices' from their
// maxima (tick_amax_kernel, one launch in front of the weight prep; W_ih_l and W_hh_l share a scale because their products share
// accumulators), the states' per beat from the workgroup's rows (a beat's states are convex combinations of tanh outputs and the
// beat's initial state; an upper layer's input is the state below times 0 or the keep scale).
// (RW: batch rows per workgroup, 16, 8 or 4 -- gru_common.h, gru_rows_per_wg)
template <int H, int RW>
__global__ __launch_bounds__(H * 4) void gru_seq_fwd_h2_kernel(GruSeqBatch batch, int T, int R) {
    static_assert(RW == 16 || RW == 8 || RW == 4, "16, 8 or 4 rows: four, two or one per lane");
    constexpr int E = RW / 4;              // elements (rows) per lane
    constexpr int KS = H / 32;             // MFMA k-steps of 32
    constexpr int HP = H + 8;              // LDS row pitch in bf16 elements (16 bytes of padding)
    constexpr int PLANE = 16 * HP;
    __shared__ __attribute__((aligned(16))) unsigned short hbuf[2][2 * PLANE];
    __shared__ float h0max[H / 16];
    const GruSeq &s = batch.seq[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int unit = 16 * w + col;
    const int row0 = blockIdx.x * RW;

    // W_hh's slice of this wave as two fp16 terms at the wave's own scale (round 5: the slice's largest magnitude just below 2^15;
    // through round 4 a fixed 2^8, which overflowed fp16 for |w| >= 255)
    f16x8 wh[3][KS], wl[3][KS];
    float w_inv;
    {
        float x[3][KS][8], m = 0.f;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const float *src = s.w_hh + (int64_t)(g * H + unit) * H + 32 * ks + 8 * quad;
                const f32x4 v0 = *reinterpret_cast<const f32x4 *>(src), v1 = *reinterpret_cast<const f32x4 *>(src + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[g][ks][j] = v0[j]; x[g][ks][4 + j] = v1[j];
                    m = fmaxf(m, fmaxf(fabsf(v0[j]), fabsf(v1[j])));
                }
            }
        m = row16_max(m);
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const Pow2 sw = pow2_for(m);
        w_inv = sw.inv;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) split2_8<false>(x[g][ks], sw.s, wh[g][ks], wl[g][ks]);
    }
    const float bh_r = s.b_hh[unit], bh_z = s.b_hh[H + unit], bh_n = s.b_hh[2 * H + unit];

    int rows[E];
    bool live[E];
    float h[E];
    auto lrow = [&](int i) { return gru_lrow<E>(quad, i); };                  // the tile row of this lane's element i
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int r = row0 + lrow(i);
        live[i] = r < R;
        rows[i] = live[i] ? r : R - 1;
        h[i] = (s.h0 != nullptr && live[i]) ? s.h0[(int64_t)rows[i] * s.h0_stride + unit] : 0.f;
    }
    // The state's scale: every h_t is a convex combination of a tanh output and h_(t-1), so |h_t| <= max(1, max |h0|) for the whole
    // sequence -- the workgroup's rows' largest |h0| (or 1) goes just below 2^15 (through round 4 a fixed 2^4: fp16 overflow for an
    // initial state beyond 4094, and the decoder's comes out of a SELU layer)
    float h_s, unscale;
    {
        float m = 1.f;
#pragma unroll
        for (int i = 0; i < E; ++i) m = fmaxf(m, fabsf(h[i]));
        m = row16_max(m);
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        if (lane == 0) h0max[w] = m;
        lds_barrier();
#pragma unroll
        for (int q = 0; q < H / 16; ++q) m = fmaxf(m, h0max[q]);
        const Pow2 sh = pow2_for(m);
        h_s = sh.s;
        unscale = sh.inv * w_inv;
    }
#pragma unroll
    for (int i = 0; i < E; ++i) store_split2<false>(&hbuf[0][lrow(i) * HP + unit], PLANE, h[i], h_s);
    // per-step memory operations as raw buffer operations (gru_rsrc): a scalar step offset + one per-lane offset per array and row
    // (the running 64-bit pointers this kernel had cost 24 registers and a 64-bit add each per step; the first and last step's
    // missing operations were branches).  A dead row's stores go beyond the range.
    const __amdgpu_buffer_rsrc_t rs_gi = gru_rsrc(s.gi), rs_h = gru_rsrc(s.h_all), rs_sv = gru_rsrc(s.saved), rs_none = gru_rsrc(nullptr);
    const int reverse = s.reverse, unit4 = 4 * unit;
    const int gi_tp = 4 * (int)s.gi_tstride, h_tp = 4 * R * (int)s.h_stride;
    // dropout on the output (gru_mask.h): the keep byte of the CURRENT step is requested with the step's other traffic, the masked
    // copy of a step's h leaves one step later beside h.  No mask: an empty range (loads return 0, the stores are dropped).
    const __amdgpu_buffer_rsrc_t rs_mk = gru_rsrc(s.mask), rs_hm = gru_rsrc(s.mask != nullptr ? s.h_masked : nullptr);
    const int mk_tp = s.mk_tstride, hm_tp = 4 * R * s.hm_stride;
    const float keep_scale = s.keep;
    int mk_o[E], hm_o[E];
    unsigned mk_cur[E];
    float keep_hm[E];
    int gi_o[E], h_o[E], sv_o[E];
    float gi_next[E][3];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        gi_o[i] = gru_off(rows[i], 4 * (int)s.gi_rstride, unit4);
        h_o[i] = live[i] ? gru_off(rows[i], 4 * (int)s.h_stride, unit4) : GRU_DEAD;
        sv_o[i] = live[i] ? gru_off(rows[i], 16 * H, 4 * unit4) : GRU_DEAD;
        mk_o[i] = s.mk_group > 0 ? (rows[i] / s.mk_group) * s.mk_gstride + (rows[i] % s.mk_group) * s.mk_rstride + unit : rows[i] * s.mk_rstride + unit;
        hm_o[i] = live[i] ? gru_off(rows[i], 4 * s.hm_stride, unit4) : GRU_DEAD;
        mk_cur[i] = 0;
        keep_hm[i] = 0.f;
        const int so = (reverse ? T - 1 : 0) * gi_tp;
        gi_next[i][0] = gru_ld(rs_gi, gi_o[i], so); gi_next[i][1] = gru_ld(rs_gi, gi_o[i] + 4 * H, so); gi_next[i][2] = gru_ld(rs_gi, gi_o[i] + 8 * H, so);
    }
    lds_barrier();
    f32x4 keep_sv[E];                        // results of the previous step, stored after the barrier
    float keep_h[E];
    int keep_t = -1;
    GSTAMP_BEGIN();

    for (int step = 0; step < T; ++step) {
        const int t = s.reverse ? T - 1 - step : step;
        const int cur = step & 1;
        float gi[E][3];
#pragma unroll
        for (int i = 0; i < E; ++i)
#pragma unroll
            for (int g = 0; g < 3; ++g) gi[i][g] = gi_next[i][g];
        GSTAMP(0);
        f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const unsigned short *hb = &hbuf[cur][gru_arow<E>(col) * HP + 8 * quad];
        // Row i's share of the step's memory traffic (next step's three input projections in, the previous step's h and saved
        // gates out) is issued BEHIND the MFMAs of k-step i, with a scheduling barrier pinning it there: as one block in front
        // of the MFMAs it was 1200 of the step's 6000 cycles (tools/stamp.py gru), all of it issue time of an in-order wave
        // while the matrix pipe sat idle.
        // next step's projections (the last step reads its own again); the previous step's results (none in step 0: the empty range)
        const int tn = step + 1 < T ? (reverse ? t - 1 : t + 1) : t;
        const int kt = keep_t >= 0 ? keep_t : 0;
        const int so_gi = tn * gi_tp, so_h = kt * h_tp, so_sv = kt * R * (16 * H);
        const __amdgpu_buffer_rsrc_t rs_hs = keep_t >= 0 ? rs_h : rs_none, rs_svs = keep_t >= 0 ? rs_sv : rs_none;
        const __amdgpu_buffer_rsrc_t rs_hms = keep_t >= 0 ? rs_hm : rs_none;
        const int so_mk = t * mk_tp, so_hm = kt * hm_tp;
        auto row_traffic = [&](int i) __attribute__((always_inline)) {
            gi_next[i][0] = gru_ld(rs_gi, gi_o[i], so_gi); gi_next[i][1] = gru_ld(rs_gi, gi_o[i] + 4 * H, so_gi);
            gi_next[i][2] = gru_ld(rs_gi, gi_o[i] + 8 * H, so_gi);
            gru_st(keep_h[i], rs_hs, h_o[i], so_h);
            gru_st(keep_hm[i], rs_hms, hm_o[i], so_hm);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, keep_sv[i]), rs_svs, sv_o[i], so_sv, 0);
            mk_cur[i] = __builtin_amdgcn_raw_buffer_load_b8(rs_mk, mk_o[i], so_mk, 0);
        };
        static_assert(KS <= 4, "one row's traffic per k-step; rows left over go last");
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f16x8 ah = lds_x8<f16x8>(hb + 32 * ks), al = lds_x8<f16x8>(hb + PLANE + 32 * ks);
            GRU_MFMA3X3(acc[0], acc[1], acc[2], ah, al, wh[0][ks], wl[0][ks], wh[1][ks], wl[1][ks], wh[2][ks], wl[2][ks]);
            __builtin_amdgcn_sched_barrier(0);
            if (ks < E) row_traffic(ks);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = KS; i < E; ++i) row_traffic(i);
        GSTAMP_DEPEND(acc[0][0] + acc[1][0] + acc[2][3]);
        GSTAMP_WAIT(all);
        GSTAMP(1);
        float av[3][E];                      // the gates' products of this lane's elements
#pragma unroll
        for (int g = 0; g < 3; ++g) gru_elems<E>(acc[g], av[g]);
#pragma unroll
        for (int i = 0; i < E; ++i) {
#pragma clang fp contract(off)               // GRU_ROUNDING (gru_common.h): the fused operations are the ones written as such
            const float r = fast_sigmoid(__builtin_fmaf(av[0][i], unscale, gi[i][0]) + bh_r);
            const float z = fast_sigmoid(__builtin_fmaf(av[1][i], unscale, gi[i][1]) + bh_z);
            const float ghn = __builtin_fmaf(av[2][i], unscale, bh_n);
            const float n = fast_tanh(__builtin_fmaf(r, ghn, gi[i][2]));
            const float hn = __builtin_fmaf(z, h[i], (1.f - z) * n);
            h[i] = hn;
            keep_h[i] = hn;
            keep_hm[i] = mk_cur[i] != 0 ? keep_scale * hn : 0.f;
            keep_sv[i] = f32x4{r, z, n, ghn};
        }
        if constexpr (E >= 2) {
#pragma unroll
            for (int i = 0; i < E; i += 2) store_split2<false>(&hbuf[cur ^ 1][lrow(i) * HP + unit], HP, PLANE, h[i], h[i + 1], h_s);
        } else {
            store_split2<false>(&hbuf[cur ^ 1][quad * HP + unit], PLANE, h[0], h_s);
        }
        keep_t = t;
        GSTAMP_WAIT(lds);                        // the LDS writes are done
        GSTAMP(2);
        lds_barrier();
        GSTAMP(3);
    }
    GSTAMP_END(0, T);
#pragma unroll
    for (int i = 0; i < E; ++i)
        if (live[i]) {
            gru_st(keep_h[i], rs_h, h_o[i], keep_t * h_tp);
            gru_st(keep_hm[i], rs_hm, hm_o[i], keep_t * hm_tp);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, keep_sv[i]), rs_sv, sv_o[i], keep_t * R * (16 * H), 0);
            if (s.h_fin != nullptr) s.h_fin[(int64_t)rows[i] * s.h_fin_stride + unit] = keep_h[i];
        }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward through time.  Per step (in the reverse of the forward's processing order):
//   g = dh_all[t] + carry;  dpn = g (1-z)(1-n^2);  dpz = g (h_prev - n) z (1-z);  dpr = dpn gh_n r (1-r)
//   dgi = [dpr, dpz, dpn];  dgh = [dpr, dpz, dpn r];  carry = g z + dgh . W_hh
//
// The backward recurrence on the bf16 MFMA at fp32 accuracy (the three-term split of splitmath.h; the diagnostic build's
// ARVAE_GRU_BF16_BWD form): W_hh is split once into hi + mid + lo bf16 terms per lane (144 VGPRs at H = 128), dgh is split
// when it is written to LDS as three bf16 planes, and a multiply-add is the six partial products >= 2^-18 on
// v_mfma_f32_16x16x32_bf16 (16 cycles each instead of 8 x 32 for the fp32 16x16x4), smallest first.
// (RW: batch rows per workgroup, 16 or 4 -- see gru_seq_fwd_h2_kernel)
template <int H, int RW>
__global__ __launch_bounds__(H * 4) void gru_seq_bwd_x3_kernel(GruSeqBatch batch, int T, int R) {
    static_assert(RW == 16 || RW == 8 || RW == 4, "16, 8 or 4 rows: four, two or one per lane");
    constexpr int E = RW / 4;              // elements (rows) per lane
    constexpr int KS = 3 * H / 32;
    constexpr int DP = 3 * H + 8;           // LDS row pitch in bf16 elements
    constexpr int PLANE = 16 * DP;
    __shared__ __attribute__((aligned(16))) unsigned short dbuf[2][3 * PLANE];
    const GruSeq &s = batch.seq[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int unit = 16 * w + col;
    const int row0 = blockIdx.x * RW;

    // B[k = c][n = unit] = W_hh[c][unit], c = 32 ks + 8 quad + j
    bf16x8 wh[KS], wm[KS], wl[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = s.w_hh[(int64_t)(32 * ks + 8 * quad + j) * H + unit];
        split3_8(x, wh[ks], wm[ks], wl[ks]);
    }

    int rows[E];
    bool live[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int r = row0 + gru_lrow<E>(quad, i);
        live[i] = r < R;
        rows[i] = live[i] ? r : R - 1;
    }
    float carry[E];
#pragma unroll
    for (int i = 0; i < E; ++i)
        carry[i] = (s.dh_last != nullptr && live[i]) ? s.dh_last[(int64_t)rows[i] * s.dh_last_stride + unit] : 0.f;

    // the step's arrays as buffer resources (gru_rsrc), their row pitches in bytes
    const __amdgpu_buffer_rsrc_t rs_dh = gru_rsrc(s.dh_all), rs_sv = gru_rsrc(s.saved), rs_hall = gru_rsrc(s.h_all), rs_h0 = gru_rsrc(s.h0);
    const __amdgpu_buffer_rsrc_t rs_dgi = gru_rsrc(s.dgi), rs_dgh = gru_rsrc(s.dgh), rs_hpo = gru_rsrc(s.h_prev_out);
    const int reverse = s.reverse, unit4 = 4 * unit;
    const int dh_p = 4 * (int)s.dh_stride, h_p = 4 * (int)s.h_stride, h0_p = 4 * (int)s.h0_stride, dgi_p = 4 * (int)s.dgi_rstride;
    float nx[E][6];                          // dh, r, z, n, gh_n, h_prev of the next step
    auto fetch = [&](int step) {
        const int t = reverse ? step : T - 1 - step;
        const bool has_prev = step + 1 < T;
        const int tp = reverse ? t + 1 : t - 1;
        const __amdgpu_buffer_rsrc_t rs_hp = has_prev ? rs_hall : rs_h0;
        const int hp_p = has_prev ? h_p : h0_p, hp_s = has_prev ? tp * R * h_p : 0;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            nx[i][0] = gru_ld(rs_dh, gru_off(rows[i], dh_p, unit4), t * R * dh_p);
            const f32x4 sv = gru_ld4(rs_sv, gru_off(rows[i], 16 * H, 4 * unit4), t * R * (16 * H));
            nx[i][1] = sv[0]; nx[i][2] = sv[1]; nx[i][3] = sv[2]; nx[i][4] = sv[3];
            nx[i][5] = gru_ld(rs_hp, gru_off(rows[i], hp_p, unit4), hp_s);
        }
    };
    fetch(0);
    GSTAMP_BEGIN();

    for (int step = 0; step < T; ++step) {
        const int t = reverse ? step : T - 1 - step;
        const int cur = step & 1;
        float gz[E], o_gi[E][3], o_hn[E], o_hp[E];
        GSTAMP_DEPEND(nx[0][0] + nx[E - 1][5] + nx[E / 2][3]);
        GSTAMP_WAIT(all);
        GSTAMP(0);
#pragma unroll
        for (int i = 0; i < E; ++i) {
#pragma clang fp contract(off)               // GRU_ROUNDING (gru_common.h)
            const float g = live[i] ? nx[i][0] + carry[i] : 0.f;
            const float r = nx[i][1], z = nx[i][2], n = nx[i][3], ghn = nx[i][4], hp = nx[i][5];
            const float dpn = g * (1.f - z) * __builtin_fmaf(-n, n, 1.f);
            const float dpz = g * (hp - n) * z * (1.f - z);
            const float dpr = dpn * ghn * r * (1.f - r);
            const float dhn = dpn * r;
            gz[i] = g * z;
            o_gi[i][0] = dpr; o_gi[i][1] = dpz; o_gi[i][2] = dpn; o_hn[i] = dhn; o_hp[i] = hp;
        }
        if constexpr (E >= 2) {
#pragma unroll
            for (int i = 0; i < E; i += 2) {
                unsigned short *d = &dbuf[cur][gru_lrow<E>(quad, i) * DP + unit];
                store_split3(d, DP, PLANE, o_gi[i][0], o_gi[i + 1][0]);
                store_split3(d + H, DP, PLANE, o_gi[i][1], o_gi[i + 1][1]);
                store_split3(d + 2 * H, DP, PLANE, o_hn[i], o_hn[i + 1]);
            }
        } else {
            unsigned short *d = &dbuf[cur][quad * DP + unit];
            store_split3(d, PLANE, o_gi[0][0]);
            store_split3(d + H, PLANE, o_gi[0][1]);
            store_split3(d + 2 * H, PLANE, o_hn[0]);
        }
        GSTAMP_WAIT(lds);
        GSTAMP(1);
        if (step + 1 < T) fetch(step + 1);
        lds_barrier();
        GSTAMP(2);
        f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const unsigned short *db = &dbuf[cur][gru_arow<E>(col) * DP + 8 * quad];
        static_assert(KS % 3 == 0 && KS / 3 <= 4, "three k-steps at a time, one per accumulator; one row's stores behind each group");
        // row i's gradients of this step leave BEHIND the MFMAs of k-step group i (pinned: see gru_seq_fwd_h2_kernel)
        auto row_stores = [&](int i) __attribute__((always_inline)) {
            if (live[i]) {
                const int og = gru_off(rows[i], dgi_p, unit4), sg = t * R * dgi_p;
                const int o = gru_off(rows[i], 12 * H, unit4), so = t * R * (12 * H);
                gru_st(o_gi[i][0], rs_dgi, og, sg); gru_st(o_gi[i][1], rs_dgi, og + 4 * H, sg); gru_st(o_gi[i][2], rs_dgi, og + 8 * H, sg);
                gru_st(o_gi[i][0], rs_dgh, o, so); gru_st(o_gi[i][1], rs_dgh, o + 4 * H, so); gru_st(o_hn[i], rs_dgh, o + 8 * H, so);
                gru_st(o_hp[i], rs_hpo, gru_off(rows[i], 4 * H, unit4), t * R * (4 * H));
            }
        };
#pragma unroll
        for (int ks = 0; ks < KS; ks += 3) {
            const bf16x8 ah0 = lds_x8<bf16x8>(db + 32 * ks), am0 = lds_x8<bf16x8>(db + PLANE + 32 * ks), al0 = lds_x8<bf16x8>(db + 2 * PLANE + 32 * ks);
            const bf16x8 ah1 = lds_x8<bf16x8>(db + 32 * (ks + 1)), am1 = lds_x8<bf16x8>(db + PLANE + 32 * (ks + 1)), al1 = lds_x8<bf16x8>(db + 2 * PLANE + 32 * (ks + 1));
            const bf16x8 ah2 = lds_x8<bf16x8>(db + 32 * (ks + 2)), am2 = lds_x8<bf16x8>(db + PLANE + 32 * (ks + 2)), al2 = lds_x8<bf16x8>(db + 2 * PLANE + 32 * (ks + 2));
            GRU_MFMA6X3(acc[0], acc[1], acc[2], ah0, am0, al0, ah1, am1, al1, ah2, am2, al2, wh[ks], wm[ks], wl[ks], wh[ks + 1], wm[ks + 1],
                        wl[ks + 1], wh[ks + 2], wm[ks + 2], wl[ks + 2]);
            __builtin_amdgcn_sched_barrier(0);
            if (ks / 3 < E) row_stores(ks / 3);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = KS / 3; i < E; ++i) row_stores(i);
        {
            const f32x4 sum = {acc[0][0] + acc[1][0] + acc[2][0], acc[0][1] + acc[1][1] + acc[2][1], acc[0][2] + acc[1][2] + acc[2][2],
                               acc[0][3] + acc[1][3] + acc[2][3]};
            float cs[E];
            gru_elems<E>(sum, cs);
#pragma unroll
            for (int i = 0; i < E; ++i) carry[i] = gz[i] + cs[i];
        }
        GSTAMP_DEPEND(carry[0] + carry[E - 1]);
        GSTAMP(3);
    }
    GSTAMP_END(GRU_STAMP_WAVE, T);
    if (s.dh0 != nullptr)
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (live[i]) s.dh0[(int64_t)rows[i] * s.dh0_stride + unit] = carry[i];
}

// The backward recurrence on scaled two-term fp16 (round 5).  Its operand -- a step's (dpr, dpz, dhn) per batch row -- is a gradient:
// no magnitude known beforehand, and it moves over the time steps (what kept this kernel on the three-term bf16 split in round 4).
// With one element per lane (RW 4) the recurrence became MFMA-bound -- 72 dependent-free 16x16x32 MFMAs per wave and step at 32
// cycles, two waves per SIMD: 4600 of a step's cycles -- so half the products are worth a second barrier: every batch ROW gets its own
// power-of-two scale each step (a row's scale factors out of its dot products), the largest magnitude of the row's 3 H values brought
// to [2^14, 2^15): a 16-lane butterfly per wave, one LDS slot per (row, wave), a barrier, NW slots read back.  Nothing can overflow
// (the scaled maximum is below 2^15 by construction), a row whose gradient is 1e-9 keeps the same 22 bits as one at 1e+3, and W_hh^T
// gets a per-wave scale from its own slice's maximum in the prologue (a column's scale factors out as well) instead of the fixed 2^8.
template <int H, int RW>
__global__ __launch_bounds__(H * 4) void gru_seq_bwd_h2_kernel(GruSeqBatch batch, int T, int R) {
    static_assert(RW == 16 || RW == 8 || RW == 4, "16, 8 or 4 rows: four, two or one per lane");
    constexpr int E = RW / 4;              // elements (rows) per lane
    constexpr int NW = H / 16;             // waves
    constexpr int KS = 3 * H / 32;
    constexpr int DP = 3 * H + 8;           // LDS row pitch in fp16 elements
    constexpr int PLANE = 16 * DP;
    constexpr int MW = NW < 4 ? 4 : NW;     // slots per row of the maxima (16-byte reads)
    __shared__ __attribute__((aligned(16))) unsigned short dbuf[2 * PLANE];
    __shared__ __attribute__((aligned(16))) float rmax[16][MW];
    const GruSeq &s = batch.seq[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int unit = 16 * w + col;
    const int row0 = blockIdx.x * RW;

    // B[k = c][n = unit] = W_hh[c][unit], c = 32 ks + 8 quad + j: two fp16 terms at this wave's own scale
    f16x8 wh[KS], wl[KS];
    float w_inv;
    {
        float x[KS][8], m = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                x[ks][j] = s.w_hh[(int64_t)(32 * ks + 8 * quad + j) * H + unit];
                m = fmaxf(m, fabsf(x[ks][j]));
            }
        m = row16_max(m);
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const Pow2 sw = pow2_for(m);
        w_inv = sw.inv;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) split2_8<false>(x[ks], sw.s, wh[ks], wl[ks]);
    }
    if (MW > NW && threadIdx.x < 16 * (MW - NW)) rmax[threadIdx.x / (MW - NW)][NW + threadIdx.x % (MW - NW)] = 0.f;   // (slots no wave writes)

    auto lrow = [&](int i) { return gru_lrow<E>(quad, i); };                  // the tile row of this lane's element i
    int rows[E];
    bool live[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int r = row0 + lrow(i);
        live[i] = r < R;
        rows[i] = live[i] ? r : R - 1;
    }
    float carry[E];
#pragma unroll
    for (int i = 0; i < E; ++i)
        carry[i] = (s.dh_last != nullptr && live[i]) ? s.dh_last[(int64_t)rows[i] * s.dh_last_stride + unit] : 0.f;

    // the step's arrays as buffer resources (gru_rsrc), their row pitches in bytes
    const __amdgpu_buffer_rsrc_t rs_dh = gru_rsrc(s.dh_all), rs_sv = gru_rsrc(s.saved), rs_hall = gru_rsrc(s.h_all), rs_h0 = gru_rsrc(s.h0);
    const __amdgpu_buffer_rsrc_t rs_dgi = gru_rsrc(s.dgi), rs_dgh = gru_rsrc(s.dgh), rs_hpo = gru_rsrc(s.h_prev_out);
    const int reverse = s.reverse, unit4 = 4 * unit;
    const int dh_p = 4 * (int)s.dh_stride, h_p = 4 * (int)s.h_stride, h0_p = 4 * (int)s.h0_stride, dgi_p = 4 * (int)s.dgi_rstride;
    float nx[E][6];                          // dh, r, z, n, gh_n, h_prev of the next step
    // dropout on the sequence's output (gru_mask.h): dh_all is then the gradient w.r.t. keep * mask * h
    const bool masked = s.mask != nullptr;
    const __amdgpu_buffer_rsrc_t rs_mk = gru_rsrc(s.mask);
    const float keep_scale = s.keep;
    int mk_o[E];
    unsigned mk_nx[E];
#pragma unroll
    for (int i = 0; i < E; ++i)
        mk_o[i] = s.mk_group > 0 ? (rows[i] / s.mk_group) * s.mk_gstride + (rows[i] % s.mk_group) * s.mk_rstride + unit : rows[i] * s.mk_rstride + unit;
    auto fetch = [&](int step) {
        const int t = reverse ? step : T - 1 - step;
        const bool has_prev = step + 1 < T;
        const int tp = reverse ? t + 1 : t - 1;
        const __amdgpu_buffer_rsrc_t rs_hp = has_prev ? rs_hall : rs_h0;
        const int hp_p = has_prev ? h_p : h0_p, hp_s = has_prev ? tp * R * h_p : 0;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            nx[i][0] = gru_ld(rs_dh, gru_off(rows[i], dh_p, unit4), t * R * dh_p);
            mk_nx[i] = __builtin_amdgcn_raw_buffer_load_b8(rs_mk, mk_o[i], t * s.mk_tstride, 0);
            const f32x4 sv = gru_ld4(rs_sv, gru_off(rows[i], 16 * H, 4 * unit4), t * R * (16 * H));
            nx[i][1] = sv[0]; nx[i][2] = sv[1]; nx[i][3] = sv[2]; nx[i][4] = sv[3];
            nx[i][5] = gru_ld(rs_hp, gru_off(rows[i], hp_p, unit4), hp_s);
        }
    };
    fetch(0);

    for (int step = 0; step < T; ++step) {
        const int t = reverse ? step : T - 1 - step;
        float gz[E], o_gi[E][3], o_hn[E], o_hp[E];
#pragma unroll
        for (int i = 0; i < E; ++i) {
#pragma clang fp contract(off)               // GRU_ROUNDING (gru_common.h)
            const float dh = masked ? (mk_nx[i] != 0 ? keep_scale * nx[i][0] : 0.f) : nx[i][0];
            const float g = live[i] ? dh + carry[i] : 0.f;
            const float r = nx[i][1], z = nx[i][2], n = nx[i][3], ghn = nx[i][4], hp = nx[i][5];
            const float dpn = g * (1.f - z) * __builtin_fmaf(-n, n, 1.f);
            const float dpz = g * (hp - n) * z * (1.f - z);
            const float dpr = dpn * ghn * r * (1.f - r);
            const float dhn = dpn * r;
            gz[i] = g * z;
            o_gi[i][0] = dpr; o_gi[i][1] = dpz; o_gi[i][2] = dpn; o_hn[i] = dhn; o_hp[i] = hp;
            const float m = row16_max(fmaxf(fmaxf(fabsf(dpr), fabsf(dpz)), fabsf(dhn)));
            if (col == 0) rmax[lrow(i)][w] = m;
        }
        if (step + 1 < T) fetch(step + 1);
        lds_barrier();                       // the rows' maxima are in LDS; every read of the previous step's operand image is done
        float unscale[E];
#pragma unroll
        for (int i = 0; i < E; ++i) {
            float m = 0.f;
#pragma unroll
            for (int q = 0; q < MW; q += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(&rmax[lrow(i)][q]);
                m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
            }
            const Pow2 sc = pow2_for(m);
            unscale[i] = sc.inv * w_inv;
            unsigned short *d = &dbuf[lrow(i) * DP + unit];
            store_split2<false>(d, PLANE, o_gi[i][0], sc.s);
            store_split2<false>(d + H, PLANE, o_gi[i][1], sc.s);
            store_split2<false>(d + 2 * H, PLANE, o_hn[i], sc.s);
        }
        lds_barrier();                       // the operand image is written; the maxima have been read
        f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const unsigned short *db = &dbuf[gru_arow<E>(col) * DP + 8 * quad];
        static_assert(KS % 3 == 0 && KS / 3 <= 4, "three k-steps at a time, one per accumulator; one row's stores behind each group");
        // row i's gradients of this step leave BEHIND the MFMAs of k-step group i (pinned: see gru_seq_fwd_h2_kernel)
        auto row_stores = [&](int i) __attribute__((always_inline)) {
            if (live[i]) {
                const int og = gru_off(rows[i], dgi_p, unit4), sg = t * R * dgi_p;
                const int o = gru_off(rows[i], 12 * H, unit4), so = t * R * (12 * H);
                gru_st(o_gi[i][0], rs_dgi, og, sg); gru_st(o_gi[i][1], rs_dgi, og + 4 * H, sg); gru_st(o_gi[i][2], rs_dgi, og + 8 * H, sg);
                gru_st(o_gi[i][0], rs_dgh, o, so); gru_st(o_gi[i][1], rs_dgh, o + 4 * H, so); gru_st(o_hn[i], rs_dgh, o + 8 * H, so);
                gru_st(o_hp[i], rs_hpo, gru_off(rows[i], 4 * H, unit4), t * R * (4 * H));
            }
        };
#pragma unroll
        for (int ks = 0; ks < KS; ks += 3) {
            const f16x8 ah0 = lds_x8<f16x8>(db + 32 * ks), al0 = lds_x8<f16x8>(db + PLANE + 32 * ks);
            const f16x8 ah1 = lds_x8<f16x8>(db + 32 * (ks + 1)), al1 = lds_x8<f16x8>(db + PLANE + 32 * (ks + 1));
            const f16x8 ah2 = lds_x8<f16x8>(db + 32 * (ks + 2)), al2 = lds_x8<f16x8>(db + PLANE + 32 * (ks + 2));
            GRU_MFMA3K3(acc[0], acc[1], acc[2], ah0, al0, ah1, al1, ah2, al2, wh[ks], wl[ks], wh[ks + 1], wl[ks + 1], wh[ks + 2], wl[ks + 2]);
            __builtin_amdgcn_sched_barrier(0);
            if (ks / 3 < E) row_stores(ks / 3);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = KS / 3; i < E; ++i) row_stores(i);
        {
            const f32x4 sum = {acc[0][0] + acc[1][0] + acc[2][0], acc[0][1] + acc[1][1] + acc[2][1], acc[0][2] + acc[1][2] + acc[2][2],
                               acc[0][3] + acc[1][3] + acc[2][3]};
            float cs[E];
            gru_elems<E>(sum, cs);
#pragma unroll
            for (int i = 0; i < E; ++i) carry[i] = __builtin_fmaf(cs[i], unscale[i], gz[i]);
        }
    }
    if (s.dh0 != nullptr)
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (live[i]) s.dh0[(int64_t)rows[i] * s.dh0_stride + unit] = carry[i];
}

static int fill_batch(GruSeqBatch *b, const arvae_gru_seq_t *seqs, int nseq, int hidden, const GruSeqMask *masks = nullptr) {
    for (int i = 0; i < nseq; ++i) {
        const arvae_gru_seq_t &q = seqs[i];
        GruSeq &s = b->seq[i];
        if (masks != nullptr && masks[i].mask != nullptr) {
            const GruSeqMask &k = masks[i];
            s.mask = k.mask; s.keep = k.keep; s.h_masked = k.h_masked; s.hm_stride = (int)k.hm_stride;
            s.mk_tstride = (int)k.tstride; s.mk_rstride = (int)k.rstride; s.mk_gstride = (int)k.gstride; s.mk_group = k.group;
        }
        s.gi = q.gi; s.gi_tstride = q.gi_tstride; s.w_hh = q.w_hh; s.b_hh = q.b_hh; s.h0 = q.h0;
        s.h_all = q.h_all; s.h_stride = q.h_stride; s.saved = q.saved; s.reverse = q.reverse;
        s.dh_all = q.dh_all; s.dh_stride = q.dh_stride; s.dgi = q.dgi; s.dgh = q.dgh; s.dh0 = q.dh0;
        s.dh_last = q.dh_last; s.dh_last_stride = q.dh_last_stride; s.h_prev_out = q.h_prev_out;
        s.gi_rstride = q.gi_rstride != 0 ? q.gi_rstride : 3 * hidden;
        s.dgi_rstride = q.dgi_rstride != 0 ? q.dgi_rstride : 3 * hidden;
        s.h_fin = q.h_fin; s.h_fin_stride = q.h_fin_stride;
        s.h0_stride = q.h0_stride != 0 ? q.h0_stride : hidden;
        s.dh0_stride = q.dh0_stride != 0 ? q.dh0_stride : hidden;
    }
    return 0;
}

}  // namespace arvae

using namespace arvae;

// f(hidden size, rows per workgroup) as constants; false: a hidden size that is not built (arvae_gru_seq_supported) or a row width
// gru_rows_per_wg() does not return
template <class F> static bool gru_with_shape(int hidden, int rw, F &&f) {
    bool rw_known = false;
    const bool h_known = with_int<128, 64, 32>(hidden, [&](auto HH) { rw_known = with_int<4, 8, 16>(rw, [&](auto RW) { f(HH, RW); }); });
    return h_known && rw_known;
}

// ARVAE_GRU_BF16_BWD=1 (diagnostic build): the backward recurrence on the three-term bf16 split, as through round 4
static bool gru_bf16_backward() {
    static const bool on = diag_env("ARVAE_GRU_BF16_BWD") != nullptr;
    return on;
}

extern "C" int arvae_gru_seq_supported(int32_t hidden) { return hidden == 32 || hidden == 64 || hidden == 128; }

static bool any_mask(const GruSeqMask *masks, int nseq) {
    for (int i = 0; masks != nullptr && i < nseq; ++i)
        if (masks[i].mask != nullptr) return true;
    return false;
}
namespace arvae {
bool gru_seq_masks_supported() { return !gru_bf16_backward(); }
}  // namespace arvae

extern "C" int arvae_gru_seq_fwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden,
                                 arvae_stream_t stream) {
    return gru_seq_fwd_masked(seqs, nullptr, nseq, steps, rows, hidden, stream);
}

int arvae::gru_seq_fwd_masked(const arvae_gru_seq_t *seqs, const GruSeqMask *masks, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden,
                              arvae_stream_t stream) {
    ARVAE_REQUIRE(seqs != nullptr && nseq >= 1 && nseq <= GRU_SEQ_MAX, "gru_seq_fwd: 1..%d sequences per launch", GRU_SEQ_MAX);
    ARVAE_REQUIRE(!any_mask(masks, nseq) || gru_seq_masks_supported(), "gru_seq_fwd: output dropout needs the fp16 two-term kernels");
    for (int i = 0; masks != nullptr && i < nseq; ++i)
        ARVAE_REQUIRE(masks[i].mask == nullptr || (masks[i].h_masked != nullptr && masks[i].hm_stride >= hidden && masks[i].group >= 0),
                      "gru_seq_fwd: a masked sequence needs its output buffer");
    ARVAE_REQUIRE(steps >= 1 && rows >= 1, "gru_seq_fwd: empty sequence");
    ARVAE_REQUIRE(arvae_gru_seq_supported(hidden), "gru_seq_fwd: hidden size %d is not built (32, 64, 128)", hidden);
    for (int i = 0; i < nseq; ++i)
        ARVAE_REQUIRE(seqs[i].gi && seqs[i].w_hh && seqs[i].b_hh && seqs[i].h_all && seqs[i].saved, "gru_seq_fwd: null pointer");
    GruSeqBatch b{};
    fill_batch(&b, seqs, nseq, hidden, masks);
    // (the recurrence addresses its arrays with 32-bit byte offsets: gru_rsrc)
    for (int i = 0; i < nseq; ++i) {
        const GruSeq &q = b.seq[i];
        const int64_t gi_bytes = 4 * ((int64_t)steps * q.gi_tstride + (int64_t)rows * q.gi_rstride);
        const int64_t h_bytes = 4 * (int64_t)steps * rows * std::max<int64_t>(q.h_stride, 4 * (int64_t)hidden);
        ARVAE_REQUIRE(gi_bytes < GRU_RANGE && h_bytes < GRU_RANGE, "gru_seq_fwd: %d steps x %d rows do not fit 2 GB per array", steps, rows);
    }
    hipStream_t st = as_stream(stream);
    const int rw = gru_rows_per_wg(rows, nseq);
    const bool known = gru_with_shape(hidden, rw, [&](auto HH, auto RW) {
        constexpr int H = decltype(HH)::value, R = decltype(RW)::value;
        ARVAE_LAUNCH((gru_seq_fwd_h2_kernel<H, R>), dim3((rows + R - 1) / R, nseq), dim3(4 * H), 0, st, b, steps, rows);
    });
    ARVAE_REQUIRE(known, "gru_seq_fwd: no kernel for hidden size %d at %d rows per workgroup", hidden, rw);
    return check_launch("gru_seq_fwd_kernel");
}

extern "C" int arvae_gru_seq_bwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden,
                                 arvae_stream_t stream) {
    return gru_seq_bwd_masked(seqs, nullptr, nseq, steps, rows, hidden, stream);
}

int arvae::gru_seq_bwd_masked(const arvae_gru_seq_t *seqs, const GruSeqMask *masks, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden,
                              arvae_stream_t stream) {
    ARVAE_REQUIRE(seqs != nullptr && nseq >= 1 && nseq <= GRU_SEQ_MAX, "gru_seq_bwd: 1..%d sequences per launch", GRU_SEQ_MAX);
    ARVAE_REQUIRE(!any_mask(masks, nseq) || gru_seq_masks_supported(), "gru_seq_bwd: output dropout needs the fp16 two-term kernels");
    for (int i = 0; masks != nullptr && i < nseq; ++i)
        ARVAE_REQUIRE(masks[i].mask == nullptr || seqs[i].dh_all != nullptr, "gru_seq_bwd: a masked sequence needs the gradient of its output");
    ARVAE_REQUIRE(steps >= 1 && rows >= 1, "gru_seq_bwd: empty sequence");
    ARVAE_REQUIRE(arvae_gru_seq_supported(hidden), "gru_seq_bwd: hidden size %d is not built (32, 64, 128)", hidden);
    for (int i = 0; i < nseq; ++i)
        ARVAE_REQUIRE(seqs[i].w_hh && seqs[i].h_all && seqs[i].saved && seqs[i].dgi && seqs[i].dgh, "gru_seq_bwd: null pointer");
    GruSeqBatch b{};
    fill_batch(&b, seqs, nseq, hidden, masks);
    // (the recurrence addresses its arrays with 32-bit byte offsets: gru_rsrc)
    const int64_t span = (int64_t)steps * rows * 4;
    for (int i = 0; i < nseq; ++i) {
        const GruSeq &q = b.seq[i];
        const int64_t widest = std::max<int64_t>({q.dh_stride, q.h_stride, q.h0_stride, q.dgi_rstride, 4 * (int64_t)hidden});
        ARVAE_REQUIRE(span * widest < GRU_RANGE, "gru_seq_bwd: %d steps x %d rows of %lld floats do not fit 2 GB per array", steps, rows,
                      (long long)widest);
    }
    hipStream_t st = as_stream(stream);
    const int rw = gru_rows_per_wg(rows, nseq);
    const bool known = gru_bf16_backward() ? gru_with_shape(hidden, rw, [&](auto HH, auto RW) {
        constexpr int H = decltype(HH)::value, R = decltype(RW)::value;
        ARVAE_LAUNCH((gru_seq_bwd_x3_kernel<H, R>), dim3((rows + R - 1) / R, nseq), dim3(4 * H), 0, st, b, steps, rows);
    }) : gru_with_shape(hidden, rw, [&](auto HH, auto RW) {
        constexpr int H = decltype(HH)::value, R = decltype(RW)::value;
        ARVAE_LAUNCH((gru_seq_bwd_h2_kernel<H, R>), dim3((rows + R - 1) / R, nseq), dim3(4 * H), 0, st, b, steps, rows);
    });
    ARVAE_REQUIRE(known, "gru_seq_bwd: no kernel for hidden size %d at %d rows per workgroup", hidden, rw);
    return check_launch("gru_seq_bwd_kernel");
}

