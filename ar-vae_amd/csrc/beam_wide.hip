// Beam search of the two-layer tick decoder at hidden sizes 256 and 512 with STREAMED weights: one library call enqueues the whole
// search on the caller's stream, FOUR LAUNCHES PER TICK (layer 0, layer 1, logits, selection), one launch before the first tick (the
// zero scores tick 0 reads) and one after the last (the backtracking).  beam_decoder.hip's one-launch kernel keeps the recurrent
// weights in registers and stops at hidden 128; here tick_wide.hip's rule holds unchanged: the step boundary is the launch boundary, no
// kernel waits for another workgroup (no flags, no spin loops, no grid barrier, no cooperative launch), and the call neither allocates
// nor synchronises nor reads back.  A launch per step cannot hang, and a captured graph can hold the call.
//
// Rows = batch * width, row r = code * W + k.  Per tick t = tpb * beat + j:
//   layer 0    tick_wide_l0_kernel's tiling and arithmetic (the tile of gru_wide_tile.h), with two index indirections: h_prev of row
//              (code, k) is the state of row (code, parent[t - 1][code][k]), in the GEMM's operand loads (gwt_gemm3_rows) and in the
//              epilogue alike, and the fed-back note is notes[t - 1][code][k] (the start row `vocab` at t == 0).  No gather launch and
//              no copy of the states.  At j == 0 every beam of a code reads h0[beat][code]; gib is read at row beat * B + code.
//   layer 1    tick_wide_l1_kernel<H, false>'s, x read directly, h_prev through the same parent map.
//   logits     tick_wide_out_kernel's GEMM, 16 rows x the whole vocabulary per workgroup: relu(W_out h_l1' + b_out) to the tick's slab
//              of the workspace (stream order makes reusing it safe) and, where given, to logits_out[:, t].
//   selection  beam_decoder.hip's beam_select_kernel, unchanged, on that slab (beam_select.h): the plain, planned and grouped searches
//              are by construction those of arvae_beam_select, _planned and _groups, dead slots, tie order and the penalised key included.
// The selection takes contiguous (codes, W) arrays, so the history of the search (parents, notes, scores) is kept TICK-MAJOR in the
// workspace; the backtracking launch walks it and writes it out in the (B, ticks, W) layout of the one-launch entry points.
//
// All addressing is 64-bit.  Rows past B * W repeat the last row as operands and store nothing; a parent or a note read back from
// the history is clamped into its range before it indexes anything.
#include <algorithm>
#include <cmath>
#include "gru_wide_tile.h"
#include "beam_select.h"

namespace arvae {

constexpr int BW_ORT = 16;                 // rows per workgroup of the logits kernel
constexpr int BW_VMAX = 128;               // notes: eight 16-note tiles, two per wave

struct BeamWide {
    const float *w_hh0, *b_hh0, *w_ih1, *b_ih1, *w_hh1, *b_hh1, *w_out, *b_out;
    const float *h0_l0, *h0_l1, *gib, *ptab;
    float *hs0, *hs1;                      // workspace: the layers' states, [2][rows][H] each
    float *slab;                           // workspace: a tick's logits [rows][V]
    int *par;                              // workspace: the history, tick-major [ticks][rows]
    int64_t *note;
    float *sc;
    float *logits;                         // [B][ticks][W][V] or null
    int64_t h0_stride;
    int batch, width, rows, tpb, ticks, vocab;
};

// the row of the previous states that row r = (code, k) continues at tick t: its code's row of the beat's initial states at a
// restart, else its parent's row of the tick before
__device__ __forceinline__ int64_t bw_prev_row(const BeamWide &p, int t, bool restart, int r) {
    const int code = r / p.width;
    if (restart) return code;
    const int k = p.par[(int64_t)(t - 1) * p.rows + r];
    return code * p.width + min(max(k, 0), p.width - 1);
}

// ------------------------------------------------------------------------------------------------------------------
// Layer 0 of tick t: gh = h_prev . W_hh0^T for the tile, gi = ptab[previous note] + gib[beat][code], then r, z, n, h'.
template <int H>
__global__ __launch_bounds__(64 * GWT_WAVES) void beam_wide_l0_kernel(BeamWide p, int t) {
    constexpr int NU = H / 16;
    static_assert(NU % 8 == 0, "unit tiles in multiples of the XCD count");
    __shared__ __attribute__((aligned(16))) GwtRed<3> red;                              // 24 KB
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * GWT_RT, unit0 = 16 * (blockIdx.x % NU);
    const int R = p.rows, beat = t / p.tpb;
    const bool restart = t % p.tpb == 0;
    const float *hp = restart ? p.h0_l0 + (int64_t)beat * p.batch * p.h0_stride : p.hs0 + (int64_t)((t + 1) & 1) * R * H;
    const int64_t hp_stride = restart ? p.h0_stride : H;
    float *out = p.hs0 + (int64_t)(t & 1) * R * H;

    // the epilogue's operands are requested first: they arrive while the GEMM runs
    const GwtElems e = gwt_elems(w, lane, row0, unit0, R);
    float gi[2][3], hprev[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t code = (int)e.row[k] / p.width;
        const int64_t note = t == 0 ? p.vocab : min(max((int)p.note[(int64_t)(t - 1) * R + e.row[k]], 0), p.vocab - 1);
        const float *a = p.ptab + note * (3 * H) + e.unit, *b = p.gib + ((int64_t)beat * p.batch + code) * (3 * H) + e.unit;
#pragma unroll
        for (int g = 0; g < 3; ++g) gi[k][g] = a[g * H] + b[g * H];
        hprev[k] = hp[bw_prev_row(p, t, restart, (int)e.row[k]) * hp_stride + e.unit];
    }
    const float bh_r = p.b_hh0[e.unit], bh_z = p.b_hh0[H + e.unit], bh_n = p.b_hh0[2 * H + e.unit];
    const int64_t src[2] = {bw_prev_row(p, t, restart, min(row0 + col, R - 1)), bw_prev_row(p, t, restart, min(row0 + 16 + col, R - 1))};

    f32x4 acc[2][3];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[rb][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    gwt_gemm3_rows<H, false>(acc, hp, hp_stride, nullptr, 1.f, p.w_hh0, src, unit0, w, col, quad);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int g = 0; g < 3; ++g) *reinterpret_cast<f32x4 *>(red[w][rb][g][lane]) = acc[rb][g];
    lds_barrier();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float gh[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) gh[g] = gwt_wave_sum<3>(red, e.rb, g, lane, e.i0 + k);
        const GwtGates o = gwt_gates(gh[0], gh[1], gh[2], gi[k][0], gi[k][1], gi[k][2], bh_r, bh_z, bh_n, hprev[k]);
        if (e.live[k]) out[e.row[k] * H + e.unit] = o.hn;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Layer 1 of tick t: gi = h_l0' . W_ih1^T + b_ih1 and gh = h_l1_prev . W_hh1^T + b_hh1, then the gates.
template <int H>
__global__ __launch_bounds__(64 * GWT_WAVES) void beam_wide_l1_kernel(BeamWide p, int t) {
    constexpr int NU = H / 16;
    __shared__ __attribute__((aligned(16))) GwtRed<6> red;                              // 48 KB: gates 0-2 of gi, 3-5 of gh
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * GWT_RT, unit0 = 16 * (blockIdx.x % NU);
    const int R = p.rows, beat = t / p.tpb;
    const bool restart = t % p.tpb == 0;
    const float *x = p.hs0 + (int64_t)(t & 1) * R * H;                                   // layer 0's state of this tick
    const float *hp = restart ? p.h0_l1 + (int64_t)beat * p.batch * p.h0_stride : p.hs1 + (int64_t)((t + 1) & 1) * R * H;
    const int64_t hp_stride = restart ? p.h0_stride : H;
    float *out = p.hs1 + (int64_t)(t & 1) * R * H;

    const GwtElems e = gwt_elems(w, lane, row0, unit0, R);
    float hprev[2], bi[3], bh[3];
#pragma unroll
    for (int k = 0; k < 2; ++k) hprev[k] = hp[bw_prev_row(p, t, restart, (int)e.row[k]) * hp_stride + e.unit];
#pragma unroll
    for (int g = 0; g < 3; ++g) { bi[g] = p.b_ih1[g * H + e.unit]; bh[g] = p.b_hh1[g * H + e.unit]; }
    const int64_t src[2] = {bw_prev_row(p, t, restart, min(row0 + col, R - 1)), bw_prev_row(p, t, restart, min(row0 + 16 + col, R - 1))};

    f32x4 acc[2][3];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[rb][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (half == 0) gwt_gemm3<H, false>(acc, x, H, nullptr, 1.f, p.w_ih1, row0, unit0, R, w, col, quad);
        else gwt_gemm3_rows<H, false>(acc, hp, hp_stride, nullptr, 1.f, p.w_hh1, src, unit0, w, col, quad);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int g = 0; g < 3; ++g) *reinterpret_cast<f32x4 *>(red[w][rb][3 * half + g][lane]) = acc[rb][g];
    }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        float s[6];
#pragma unroll
        for (int g = 0; g < 6; ++g) s[g] = gwt_wave_sum<6>(red, e.rb, g, lane, e.i0 + k);
        const GwtGates o = gwt_gates(s[3], s[4], s[5], s[0] + bi[0], s[1] + bi[1], s[2] + bi[2], bh[0], bh[1], bh[2], hprev[k]);
        if (e.live[k]) out[e.row[k] * H + e.unit] = o.hn;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Logits of tick t for 16 rows: tick_wide_out_kernel's products in its order (wave w computes the 16-note tiles w and w + 4 over the
// whole K: nothing to add across waves), stored to the slab and, where given, to logits_out[code][t][k].
template <int H>
__global__ __launch_bounds__(64 * GWT_WAVES) void beam_wide_logits_kernel(BeamWide p, int t) {
    constexpr int KS = H / 32;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int R = p.rows, V = p.vocab, row0 = blockIdx.x * BW_ORT;
    const int ntile = (V + 15) / 16;
    const float *hs = p.hs1 + (int64_t)(t & 1) * R * H;       // layer 1's state of this tick

    const float *a_src = hs + (int64_t)min(row0 + col, R - 1) * H + 8 * quad;
    const float *w_src[2];
    bool have[2];
    f32x4 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        have[i] = w + 4 * i < ntile;                           // (uniform over the wave)
        w_src[i] = p.w_out + (int64_t)min(16 * (w + 4 * i) + col, V - 1) * H + 8 * quad;
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (!have[0]) return;
#pragma unroll 4
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 ah, am, al, wh, wm, wl;
        gwt_load_split(a_src + 32 * ks, ah, am, al);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (!have[i]) continue;
            gwt_load_split(w_src[i] + 32 * ks, wh, wm, wl);
            GRU_MFMA6(acc[i], ah, am, al, wh, wm, wl);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int v = 16 * (w + 4 * i) + col;
        if (!have[i] || v >= V) continue;
        const float b = p.b_out[v];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = row0 + 4 * quad + k;
            if (r >= R) continue;
            const float l = fmaxf(acc[i][k] + b, 0.f);
            p.slab[(int64_t)r * V + v] = l;
            if (p.logits != nullptr) {
                const int64_t code = r / p.width, beam = r % p.width;
                p.logits[((code * p.ticks + t) * p.width + beam) * V + v] = l;
            }
        }
    }
}

// the scores (and log_probs) that tick 0's selection reads: zeros
__global__ __launch_bounds__(256) void beam_wide_zero_kernel(float *zero, int rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows) zero[i] = 0.f;
}

// After the last tick, one thread per (code, beam j of the last tick): its row of the tick-major history to the (B, ticks, W) layout,
// the walk over the parents to sequences (B, W, ticks), its last score (and log_prob)
__global__ __launch_bounds__(256) void beam_wide_backtrack_kernel(BeamWide p, const float *lp_last, int *parents, int64_t *tokens,
                                                                  float *scores_hist, int64_t *sequences, float *scores,
                                                                  float *log_probs) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= p.rows) return;
    const int W = p.width, T = p.ticks;
    const int64_t code = (int)r / W, j = (int)r % W;
    int at = (int)j;
    for (int t = T - 1; t >= 0; --t) {
        const int64_t tick = (int64_t)t * p.rows, o = (code * T + t) * W + j;
        parents[o] = p.par[tick + r];
        tokens[o] = p.note[tick + r];
        scores_hist[o] = p.sc[tick + r];
        sequences[r * T + t] = p.note[tick + code * W + at];
        at = min(max(p.par[tick + code * W + at], 0), W - 1);
    }
    scores[r] = p.sc[(int64_t)(T - 1) * p.rows + r];
    if (log_probs != nullptr) log_probs[r] = lp_last[r];
}

static int64_t bw_pad(int64_t floats) { return (floats + 3) / 4 * 4; }        // every part of the workspace starts 16-byte aligned

}  // namespace arvae

using namespace arvae;

extern "C" int arvae_tick_beam_search_wide_supported(int32_t hidden, int32_t vocab, int32_t width, int32_t groups) {
    return gwt_hidden_built(hidden) && vocab >= 2 && vocab <= BW_VMAX && width >= 1 && width <= BEAM_MAX_WIDTH && groups >= 0 &&
           groups <= width && (groups == 0 || width % groups == 0);
}

// the two layers' states of a tick, twice; a tick's logits; the zeros tick 0 reads; the groups' log_probs, twice; the history
extern "C" int64_t arvae_tick_beam_search_wide_ws_floats(int32_t batch, int32_t ticks, int32_t hidden, int32_t vocab, int32_t width) {
    if (batch < 1 || ticks < 1 || !arvae_tick_beam_search_wide_supported(hidden, vocab, width, 0)) return -1;
    const int64_t rows = (int64_t)batch * width;
    if (rows > INT32_MAX) return -1;
    return 4 * rows * hidden + bw_pad(rows * vocab) + 3 * bw_pad(rows) + 4 * bw_pad(ticks * rows);
}

// the three searches: plan null = the mask and its count, else the plan (no count: dead slots exist); groups 0 = not grouped, else the
// planned search in that many groups (log_probs then required)
static int beam_wide_launch(const char *who, const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                            const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden,
                            int32_t vocab, int32_t width, const uint8_t *allow, int32_t allowed, const arvae_note_plan_t *plan,
                            int32_t groups, float penalty, int32_t *parents, int64_t *tokens, float *scores_hist, int64_t *sequences,
                            float *scores, float *log_probs, float *logits_out, float *ws, arvae_stream_t stream) {
    ARVAE_REQUIRE(wts && h0_l0 && h0_l1 && gib && ptab, "%s: null pointer", who);
    ARVAE_REQUIRE(wts->w_hh0 && wts->b_hh0 && wts->w_ih1 && wts->b_ih1 && wts->w_hh1 && wts->b_hh1 && wts->w_out && wts->b_out,
                  "%s: null weight pointer", who);
    ARVAE_REQUIRE(parents && tokens && scores_hist && sequences && scores, "%s: null output pointer", who);
    ARVAE_REQUIRE(batch >= 1 && beats >= 1 && ticks_per_beat >= 1, "%s: empty problem", who);
    ARVAE_REQUIRE((int64_t)beats * ticks_per_beat <= INT32_MAX, "%s: %lld ticks", who, (long long)beats * ticks_per_beat);
    ARVAE_REQUIRE(gwt_hidden_built(hidden), "%s: hidden size %d is not built (256, 512)", who, hidden);
    ARVAE_REQUIRE(vocab >= 2 && vocab <= BW_VMAX, "%s: a vocabulary of %d notes is outside [2, %d]", who, vocab, BW_VMAX);
    const int32_t ticks = beats * ticks_per_beat;
    ARVAE_REQUIRE(groups == 0 || log_probs != nullptr, "%s: null log_probs", who);
    if (plan == nullptr) {
        if (const int rc = beam_width_check(who, width, vocab, allow, allowed)) return rc;
    } else {
        ARVAE_REQUIRE(width >= 1 && width <= BEAM_MAX_WIDTH, "%s: width %d is outside [1, %d]", who, width, BEAM_MAX_WIDTH);
        if (const int rc = note_plan_check(who, plan, ticks, vocab)) return rc;
    }
    ARVAE_REQUIRE((int64_t)batch * width <= INT32_MAX, "%s: %lld rows", who, (long long)batch * width);
    ARVAE_REQUIRE(ws != nullptr && gwt_aligned16(ws), "%s: workspace missing or not 16-byte aligned (arvae_tick_beam_search_wide_ws_floats)",
                  who);
    ARVAE_REQUIRE(gwt_aligned16(wts->w_hh0) && gwt_aligned16(wts->w_ih1) && gwt_aligned16(wts->w_hh1) && gwt_aligned16(wts->w_out) &&
                      gwt_aligned16(h0_l0) && gwt_aligned16(h0_l1),
                  "%s: w_hh0, w_ih1, w_hh1, w_out, h0_l0 and h0_l1 must be 16-byte aligned", who);
    ARVAE_REQUIRE(h0_stride % 4 == 0 && (h0_stride == 0 || h0_stride >= hidden),
                  "%s: h0_stride %lld is no multiple of 4 floats or below the hidden size", who, (long long)h0_stride);

    const int64_t rows = (int64_t)batch * width, hist = bw_pad(ticks * rows);
    BeamWide p{};
    p.w_hh0 = wts->w_hh0; p.b_hh0 = wts->b_hh0; p.w_ih1 = wts->w_ih1; p.b_ih1 = wts->b_ih1;
    p.w_hh1 = wts->w_hh1; p.b_hh1 = wts->b_hh1; p.w_out = wts->w_out; p.b_out = wts->b_out;
    p.h0_l0 = h0_l0; p.h0_l1 = h0_l1; p.h0_stride = h0_stride != 0 ? h0_stride : hidden; p.gib = gib; p.ptab = ptab;
    p.batch = batch; p.width = width; p.rows = (int)rows; p.tpb = ticks_per_beat; p.ticks = ticks; p.vocab = vocab;
    p.logits = logits_out;
    p.hs0 = ws; p.hs1 = p.hs0 + 2 * rows * hidden; p.slab = p.hs1 + 2 * rows * hidden;
    float *zero = p.slab + bw_pad(rows * vocab), *lp = zero + bw_pad(rows);            // lp: [2][bw_pad(rows)]
    p.sc = lp + 2 * bw_pad(rows);
    p.par = reinterpret_cast<int *>(p.sc + hist);
    p.note = reinterpret_cast<int64_t *>(p.sc + 2 * hist);

    hipStream_t st = as_stream(stream);
    const dim3 block(64 * GWT_WAVES), grid((p.rows + GWT_RT - 1) / GWT_RT * (hidden / 16)), grid_out((p.rows + BW_ORT - 1) / BW_ORT);
    const dim3 flat((p.rows + 255) / 256);
    const int gsel = groups != 0 ? groups : 1;
    const bool known = gwt_with_hidden(hidden, [&](auto HH) {
        constexpr int H = decltype(HH)::value;
        ARVAE_LAUNCH(beam_wide_zero_kernel, flat, dim3(256), 0, st, zero, p.rows);
        for (int t = 0; t < ticks; ++t) {
            ARVAE_LAUNCH((beam_wide_l0_kernel<H>), grid, block, 0, st, p, t);
            ARVAE_LAUNCH((beam_wide_l1_kernel<H>), grid, block, 0, st, p, t);
            ARVAE_LAUNCH((beam_wide_logits_kernel<H>), grid_out, block, 0, st, p, t);
            const int64_t at = (int64_t)t * rows;
            const float *sc_in = t == 0 ? zero : p.sc + (at - rows);
            const float *lp_in = groups == 0 ? nullptr : t == 0 ? zero : lp + ((t - 1) & 1) * bw_pad(rows);
            float *lp_out = groups == 0 ? nullptr : lp + (t & 1) * bw_pad(rows);
            const int live = std::min(t == 0 ? 1 : width, width / gsel);               // (tick 0: one live beam, per group)
            const uint8_t *mask = plan != nullptr ? plan->allow + t * plan->tick_stride : allow;
            beam_select_launch(p.slab, sc_in, batch, width, vocab, live, mask, plan != nullptr ? plan->row_stride : 0, p.par + at,
                               p.note + at, p.sc + at, gsel, groups != 0 ? penalty : 0.f, lp_in, lp_out, st);
        }
        ARVAE_LAUNCH(beam_wide_backtrack_kernel, flat, dim3(256), 0, st, p, lp + ((ticks - 1) & 1) * bw_pad(rows), parents, tokens,
                     scores_hist, sequences, scores, groups != 0 ? log_probs : (float *)nullptr);
    });
    ARVAE_REQUIRE(known, "%s: no kernel for hidden size %d", who, hidden);
    return check_launch("beam_wide_backtrack_kernel");
}

extern "C" int arvae_tick_beam_search_wide(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                           const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat,
                                           int32_t hidden, int32_t vocab, int32_t width, const uint8_t *allow, int32_t allowed,
                                           int32_t *parents, int64_t *tokens, float *scores_hist, int64_t *sequences, float *scores,
                                           float *logits_out, float *ws, arvae_stream_t stream) {
    return beam_wide_launch("tick_beam_search_wide", wts, h0_l0, h0_l1, h0_stride, gib, ptab, batch, beats, ticks_per_beat, hidden, vocab,
                            width, allow, allowed, nullptr, 0, 0.f, parents, tokens, scores_hist, sequences, scores, nullptr, logits_out,
                            ws, stream);
}

extern "C" int arvae_tick_beam_search_wide_planned(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1,
                                                   int64_t h0_stride, const float *gib, const float *ptab, int32_t batch, int32_t beats,
                                                   int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int32_t width,
                                                   const arvae_note_plan_t *plan, int32_t *parents, int64_t *tokens, float *scores_hist,
                                                   int64_t *sequences, float *scores, float *logits_out, float *ws, arvae_stream_t stream) {
    ARVAE_REQUIRE(plan != nullptr, "tick_beam_search_wide_planned: null plan");
    return beam_wide_launch("tick_beam_search_wide_planned", wts, h0_l0, h0_l1, h0_stride, gib, ptab, batch, beats, ticks_per_beat, hidden,
                            vocab, width, nullptr, vocab, plan, 0, 0.f, parents, tokens, scores_hist, sequences, scores, nullptr,
                            logits_out, ws, stream);
}

extern "C" int arvae_tick_beam_search_wide_groups(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1,
                                                  int64_t h0_stride, const float *gib, const float *ptab, int32_t batch, int32_t beats,
                                                  int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int32_t width, int32_t groups,
                                                  float penalty, const arvae_note_plan_t *plan, int32_t *parents, int64_t *tokens,
                                                  float *scores_hist, int64_t *sequences, float *scores, float *log_probs,
                                                  float *logits_out, float *ws, arvae_stream_t stream) {
    ARVAE_REQUIRE(plan != nullptr, "tick_beam_search_wide_groups: null plan");
    if (const int rc = beam_groups_check("tick_beam_search_wide_groups", width, groups, penalty)) return rc;
    return beam_wide_launch("tick_beam_search_wide_groups", wts, h0_l0, h0_l1, h0_stride, gib, ptab, batch, beats, ticks_per_beat, hidden,
                            vocab, width, nullptr, vocab, plan, groups, penalty, parents, tokens, scores_hist, sequences, scores,
                            log_probs, logits_out, ws, stream);
}
