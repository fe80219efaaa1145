// Whole-sequence GRU recurrences at hidden sizes 256 and 512 with STREAMED weights: one library call runs all T steps of up to
// GRU_WIDE_MAX independent sequences, ONE LAUNCH PER TIME STEP on the caller's stream.
//
// gru_seq.hip keeps a wave's slice of W_hh in registers for the whole sequence; at H = 256 that slice is 192 VGPRs as two fp16
// terms and at H = 512 W_hh is larger than a CU's register file, so these sizes read W_hh from memory (the XCD's L2) every step.
// A step needs every unit of the previous state, and the units of a row are spread over many workgroups here, so the step
// boundary is the launch boundary: no kernel of this file waits for another workgroup (no flags, no spin loops, no grid barrier,
// no cooperative launch).  A launch per step cannot hang.
//
// Tiling, forward and backward alike: the tile of gru_wide_tile.h (GWT_RT = 32 batch rows x 16 hidden units x ALL THREE GATES per
// workgroup of four waves, so the gate arithmetic needs no other workgroup) on one sequence (blockIdx.y).  The four waves split
// the K dimension of the step's GEMM: K = H forward, gh = h_prev . W_hh^T (gwt_gemm3); K = 3H backward, dgh' . W_hh (this file's
// loop).  The three-term bf16 operands have no scale: bf16 has fp32's exponent range, so W_hh entries of several hundred and
// states of several thousand stay finite.
// blockIdx.x = row tile * (H / 16) + unit tile: workgroups are dealt round-robin over the 8 XCDs, H / 16 is a multiple of 8, so
// the workgroups of one unit tile share an XCD and its L2 holds only that XCD's eighth of W_hh.
//
// All addressing is 64-bit pointer arithmetic (a few operations per lane and launch), so there is no 2 GB-per-array limit.
#include <algorithm>
#include "gru_wide_tile.h"

namespace arvae {

constexpr int GRU_WIDE_MAX = 4;            // sequences per call (GRU_SEQ_MAX of gru_seq.hip)

// arvae_gru_seq_t with the strides fill_wide() has filled in
struct GruWideSeq {
    const float *gi, *w_hh, *b_hh, *h0, *dh_all, *dh_last;
    float *h_all, *saved, *dgi, *dgh, *dh0, *h_prev_out, *h_fin;
    int64_t gi_tstride, gi_rstride, h_stride, h0_stride, dh_stride, dh_last_stride, dgi_rstride, h_fin_stride, dh0_stride;
    int reverse;
};
struct GruWideBatch {
    GruWideSeq seq[GRU_WIDE_MAX];
};

// ------------------------------------------------------------------------------------------------------------------
// One forward step: gh = h_prev . W_hh^T + b_hh for the tile, then r, z, n, h' (the arithmetic of gru_seq_fwd_h2_kernel's element
// loop).  h_prev is h0 (or zeros: no GEMM at all) at the first processed step, h_all of the step processed before afterwards.
// Writes h_all[t], saved[t] (r, z, n, gh_n per (row, unit): gru_seq.hip's layout) and, at the last processed step, h_fin.
template <int H>
__global__ __launch_bounds__(64 * GWT_WAVES) void gru_wide_fwd_step_kernel(GruWideBatch batch, int T, int R, int step) {
    constexpr int NU = H / 16;             // unit tiles
    static_assert(NU % 8 == 0, "unit tiles in multiples of the XCD count");
    __shared__ __attribute__((aligned(16))) GwtRed<3> red;                              // 24 KB
    const GruWideSeq &s = batch.seq[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * GWT_RT, unit0 = 16 * (blockIdx.x % NU);
    const int t = s.reverse ? T - 1 - step : step;
    const float *hp;                       // the state entering this step, row pitch hp_stride; null = zeros
    int64_t hp_stride;
    if (step == 0) {
        hp = s.h0; hp_stride = s.h0_stride;
    } else {
        hp = s.h_all + (int64_t)(s.reverse ? t + 1 : t - 1) * R * s.h_stride; hp_stride = s.h_stride;
    }

    // the epilogue's operands are requested first: they arrive while the GEMM runs
    const GwtElems e = gwt_elems(w, lane, row0, unit0, R);
    float gi[2][3], hprev[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float *g = s.gi + (int64_t)t * s.gi_tstride + e.row[k] * s.gi_rstride + e.unit;
        gi[k][0] = g[0]; gi[k][1] = g[H]; gi[k][2] = g[2 * H];
        hprev[k] = hp != nullptr ? hp[e.row[k] * hp_stride + e.unit] : 0.f;
    }
    const float bh_r = s.b_hh[e.unit], bh_z = s.b_hh[H + e.unit], bh_n = s.b_hh[2 * H + e.unit];

    float gh[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (hp != nullptr) {                   // (uniform over the workgroup)
        f32x4 acc[2][3];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[rb][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        gwt_gemm3<H, false>(acc, hp, hp_stride, nullptr, 1.f, s.w_hh, row0, unit0, R, w, col, quad);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 3; ++g) *reinterpret_cast<f32x4 *>(red[w][rb][g][lane]) = acc[rb][g];
        lds_barrier();
        // gwt_wave_sum's additions in this file's own text, here and in the backward kernel: through the helper the compiler merges
        // the two elements' LDS reads into 64-bit ones (6 and 2 read instructions where these kernels were measured with 12 and 4)
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
#pragma clang fp contract(off)
                float sum = red[0][e.rb][g][lane][e.i0 + k];
#pragma unroll
                for (int q = 1; q < GWT_WAVES; ++q) sum = sum + red[q][e.rb][g][lane][e.i0 + k];      // wave order: deterministic
                gh[k][g] = sum;
            }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const GwtGates o = gwt_gates(gh[k][0], gh[k][1], gh[k][2], gi[k][0], gi[k][1], gi[k][2], bh_r, bh_z, bh_n, hprev[k]);
        if (e.live[k]) {
            const int64_t tr = (int64_t)t * R + e.row[k];
            s.h_all[tr * s.h_stride + e.unit] = o.hn;
            *reinterpret_cast<f32x4 *>(s.saved + (tr * H + e.unit) * 4) = f32x4{o.r, o.z, o.n, o.ghn};
            if (step == T - 1 && s.h_fin != nullptr) s.h_fin[e.row[k] * s.h_fin_stride + e.unit] = o.hn;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// One backward step, in the reverse of the forward's processing order (step 0 .. T - 1; step T is the tail that only writes dh0):
//   carry = dh_last                                  at step 0
//         = z' (.) g' + dgh' . W_hh                  afterwards ((') = the step processed just before; z' (.) g' comes from the
//                                                    workspace's ping-pong buffer, dgh' from the dgh array itself)
//   g = dh_all[t] + carry;  dpn = g (1-z)(1-n^2);  dpz = g (h_prev - n) z (1-z);  dpr = dpn gh_n r (1-r)
//   dgi[t] = [dpr, dpz, dpn];  dgh[t] = [dpr, dpz, dpn r];  h_prev_out[t] = h_prev;  carry_out = g z
// (the element arithmetic of gru_seq_bwd_x3_kernel).  B[k = c][n = unit] = W_hh[c][unit], c over the 3H gate columns.
template <int H>
__global__ __launch_bounds__(64 * GWT_WAVES) void gru_wide_bwd_step_kernel(GruWideBatch batch, int T, int R, int step, const float *carry_in,
                                                                           float *carry_out) {
    constexpr int NU = H / 16;
    constexpr int KW = 3 * H / GWT_WAVES;  // a wave's share of K = 3H
    constexpr int KS = KW / 32;
    static_assert(NU % 8 == 0 && KS % 3 == 0, "three k-steps at a time, one per accumulator");
    __shared__ __attribute__((aligned(16))) GwtRed<1> red;                              // 8 KB
    const GruWideSeq &s = batch.seq[blockIdx.y];
    if (step == T && s.dh0 == nullptr) return;                                          // (uniform: the tail of a sequence without dh0)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * GWT_RT, unit0 = 16 * (blockIdx.x % NU);
    const int64_t seq_off = (int64_t)blockIdx.y * R * H;
    const GwtElems e = gwt_elems(w, lane, row0, unit0, R);

    // the epilogue's operands first
    const int t = step < T ? (s.reverse ? step : T - 1 - step) : 0;
    const bool has_prev = step + 1 < T;    // the forward pass entered step t with h_all of another step (else with h0)
    float dh[2], hp[2], c_in[2];
    f32x4 sv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t tr = (int64_t)t * R + e.row[k];
        dh[k] = (step < T && s.dh_all != nullptr) ? s.dh_all[tr * s.dh_stride + e.unit] : 0.f;
        sv[k] = step < T ? *reinterpret_cast<const f32x4 *>(s.saved + (tr * H + e.unit) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (step >= T) hp[k] = 0.f;
        else if (has_prev) hp[k] = s.h_all[((int64_t)(s.reverse ? t + 1 : t - 1) * R + e.row[k]) * s.h_stride + e.unit];
        else hp[k] = s.h0 != nullptr ? s.h0[e.row[k] * s.h0_stride + e.unit] : 0.f;
        if (step == 0) c_in[k] = s.dh_last != nullptr ? s.dh_last[e.row[k] * s.dh_last_stride + e.unit] : 0.f;
        else c_in[k] = carry_in[seq_off + e.row[k] * H + e.unit];
    }

    float carry[2] = {c_in[0], c_in[1]};
    if (step > 0) {                        // (uniform)
        const int tq = s.reverse ? step - 1 : T - step;                                 // the step processed just before
        f32x4 acc[2][3];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[rb][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *a_src[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
            a_src[rb] = s.dgh + ((int64_t)tq * R + min(row0 + 16 * rb + col, R - 1)) * (3 * H) + w * KW + 8 * quad;
        const float *w_src = s.w_hh + (int64_t)(w * KW + 8 * quad) * H + unit0 + col;
#pragma unroll
        for (int ks = 0; ks < KS; ks += 3) {
            bf16x8 ah[2][3], am[2][3], al[2][3], wh[3], wm[3], wl[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float x[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = w_src[(int64_t)(32 * (ks + j) + i) * H];
                split3_8(x, wh[j], wm[j], wl[j]);
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) gwt_load_split(a_src[rb] + 32 * (ks + j), ah[rb][j], am[rb][j], al[rb][j]);
            }
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                GRU_MFMA6X3(acc[rb][0], acc[rb][1], acc[rb][2], ah[rb][0], am[rb][0], al[rb][0], ah[rb][1], am[rb][1], al[rb][1], ah[rb][2],
                            am[rb][2], al[rb][2], wh[0], wm[0], wl[0], wh[1], wm[1], wl[1], wh[2], wm[2], wl[2]);
            }
        }
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
#pragma clang fp contract(off)
            *reinterpret_cast<f32x4 *>(red[w][rb][0][lane]) = (acc[rb][0] + acc[rb][1]) + acc[rb][2];
        }
        lds_barrier();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma clang fp contract(off)
            float sum = red[0][e.rb][0][lane][e.i0 + k];
#pragma unroll
            for (int q = 1; q < GWT_WAVES; ++q) sum = sum + red[q][e.rb][0][lane][e.i0 + k];          // wave order: deterministic
            carry[k] = c_in[k] + sum;
        }
    }
    if (step == T) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (e.live[k]) s.dh0[e.row[k] * s.dh0_stride + e.unit] = carry[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma clang fp contract(off)               // GRU_ROUNDING (gru_common.h)
        const float g = dh[k] + carry[k];
        const float r = sv[k][0], z = sv[k][1], n = sv[k][2], ghn = sv[k][3];
        const float dpn = g * (1.f - z) * __builtin_fmaf(-n, n, 1.f);
        const float dpz = g * (hp[k] - n) * z * (1.f - z);
        const float dpr = dpn * ghn * r * (1.f - r);
        const float dhn = dpn * r;
        if (e.live[k]) {
            const int64_t tr = (int64_t)t * R + e.row[k];
            float *dgi = s.dgi + tr * s.dgi_rstride + e.unit, *dgh = s.dgh + tr * (3 * H) + e.unit;
            dgi[0] = dpr; dgi[H] = dpz; dgi[2 * H] = dpn;
            dgh[0] = dpr; dgh[H] = dpz; dgh[2 * H] = dhn;
            if (s.h_prev_out != nullptr) s.h_prev_out[tr * H + e.unit] = hp[k];
            carry_out[seq_off + e.row[k] * H + e.unit] = g * z;
        }
    }
}

static void fill_wide(GruWideBatch *b, const arvae_gru_seq_t *seqs, int nseq, int hidden) {
    for (int i = 0; i < nseq; ++i) {
        const arvae_gru_seq_t &q = seqs[i];
        GruWideSeq &s = b->seq[i];
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
}

}  // namespace arvae

using namespace arvae;

extern "C" int arvae_gru_seq_wide_supported(int32_t hidden) { return gwt_hidden_built(hidden); }

// the backward pass's carried z (.) g: two buffers of [nseq][rows][hidden]
extern "C" int64_t arvae_gru_seq_wide_ws_floats(int32_t nseq, int32_t rows, int32_t hidden) {
    if (nseq < 1 || nseq > GRU_WIDE_MAX || rows < 1 || !arvae_gru_seq_wide_supported(hidden)) return -1;
    return 2 * (int64_t)nseq * rows * hidden;
}

extern "C" int arvae_gru_seq_wide_fwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden, float *ws,
                                      arvae_stream_t stream) {
    ARVAE_REQUIRE(seqs != nullptr && nseq >= 1 && nseq <= GRU_WIDE_MAX, "gru_seq_wide_fwd: 1..%d sequences per call", GRU_WIDE_MAX);
    ARVAE_REQUIRE(steps >= 1 && rows >= 1, "gru_seq_wide_fwd: empty sequence");
    ARVAE_REQUIRE(arvae_gru_seq_wide_supported(hidden), "gru_seq_wide_fwd: hidden size %d is not built (256, 512)", hidden);
    ARVAE_REQUIRE(ws != nullptr && gwt_aligned16(ws), "gru_seq_wide_fwd: workspace missing or not 16-byte aligned (arvae_gru_seq_wide_ws_floats)");
    for (int i = 0; i < nseq; ++i)
        ARVAE_REQUIRE(seqs[i].gi && seqs[i].w_hh && seqs[i].b_hh && seqs[i].h_all && seqs[i].saved, "gru_seq_wide_fwd: null pointer");
    GruWideBatch b{};
    fill_wide(&b, seqs, nseq, hidden);
    for (int i = 0; i < nseq; ++i) {
        const GruWideSeq &q = b.seq[i];
        ARVAE_REQUIRE(gwt_aligned16(q.w_hh) && gwt_aligned16(q.h_all) && gwt_aligned16(q.h0) && gwt_aligned16(q.saved) &&
                          q.h_stride % 4 == 0 && q.h0_stride % 4 == 0,
                      "gru_seq_wide_fwd: w_hh, h_all, h0 and saved must be 16-byte aligned, h_stride and h0_stride multiples of 4 floats");
        ARVAE_REQUIRE(q.h_stride >= hidden, "gru_seq_wide_fwd: h_stride %lld is below the hidden size", (long long)q.h_stride);
    }
    hipStream_t st = as_stream(stream);
    const dim3 grid((rows + GWT_RT - 1) / GWT_RT * (hidden / 16), nseq), block(64 * GWT_WAVES);
    const bool known = gwt_with_hidden(hidden, [&](auto HH) {
        constexpr int H = decltype(HH)::value;
        for (int step = 0; step < steps; ++step) ARVAE_LAUNCH((gru_wide_fwd_step_kernel<H>), grid, block, 0, st, b, steps, rows, step);
    });
    ARVAE_REQUIRE(known, "gru_seq_wide_fwd: no kernel for hidden size %d", hidden);
    return check_launch("gru_wide_fwd_step_kernel");
}

extern "C" int arvae_gru_seq_wide_bwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden, float *ws,
                                      arvae_stream_t stream) {
    ARVAE_REQUIRE(seqs != nullptr && nseq >= 1 && nseq <= GRU_WIDE_MAX, "gru_seq_wide_bwd: 1..%d sequences per call", GRU_WIDE_MAX);
    ARVAE_REQUIRE(steps >= 1 && rows >= 1, "gru_seq_wide_bwd: empty sequence");
    ARVAE_REQUIRE(arvae_gru_seq_wide_supported(hidden), "gru_seq_wide_bwd: hidden size %d is not built (256, 512)", hidden);
    ARVAE_REQUIRE(ws != nullptr && gwt_aligned16(ws), "gru_seq_wide_bwd: workspace missing or not 16-byte aligned (arvae_gru_seq_wide_ws_floats)");
    for (int i = 0; i < nseq; ++i)
        ARVAE_REQUIRE(seqs[i].w_hh && seqs[i].h_all && seqs[i].saved && seqs[i].dgi && seqs[i].dgh, "gru_seq_wide_bwd: null pointer");
    GruWideBatch b{};
    fill_wide(&b, seqs, nseq, hidden);
    bool any_dh0 = false;
    for (int i = 0; i < nseq; ++i) {
        const GruWideSeq &q = b.seq[i];
        ARVAE_REQUIRE(gwt_aligned16(q.dgh) && gwt_aligned16(q.saved), "gru_seq_wide_bwd: dgh and saved must be 16-byte aligned");
        ARVAE_REQUIRE(q.h_stride >= hidden, "gru_seq_wide_bwd: h_stride %lld is below the hidden size", (long long)q.h_stride);
        any_dh0 = any_dh0 || q.dh0 != nullptr;
    }
    hipStream_t st = as_stream(stream);
    const dim3 grid((rows + GWT_RT - 1) / GWT_RT * (hidden / 16), nseq), block(64 * GWT_WAVES);
    const int64_t half = (int64_t)nseq * rows * hidden;
    const bool known = gwt_with_hidden(hidden, [&](auto HH) {
        constexpr int H = decltype(HH)::value;
        // step T: the tail, which only completes the carry into dh0
        for (int step = 0; step < steps + (any_dh0 ? 1 : 0); ++step)
            ARVAE_LAUNCH((gru_wide_bwd_step_kernel<H>), grid, block, 0, st, b, steps, rows, step, (const float *)(ws + ((step + 1) & 1) * half),
                         ws + (step & 1) * half);
    });
    ARVAE_REQUIRE(known, "gru_seq_wide_bwd: no kernel for hidden size %d", hidden);
    return check_launch("gru_wide_bwd_step_kernel");
}
