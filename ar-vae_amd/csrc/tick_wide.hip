// Free-running pass of the two-layer tick decoder at hidden sizes 256 and 512 with STREAMED weights: one library call enqueues every
// tick on the caller's stream, THREE LAUNCHES PER TICK (layer 0, layer 1, logits + pick).  tick_decoder.hip keeps the recurrent
// weights in registers and one workgroup walks all ticks of its rows; at these sizes the weights do not fit (gru_wide.hip), the units
// of a row are spread over many workgroups, and a tick needs every unit of the tick before it, so gru_wide.hip's rule holds: the
// step boundary is the launch boundary, no kernel waits for another workgroup (no flags, no spin loops, no grid barrier, no
// cooperative launch), and the call neither allocates nor synchronises nor reads back.  A launch per step cannot hang.
//
// Rows = batch (the fed-back note carries across beats, so the beats are not independent here).  Per tick t = tpb * beat + j:
//   layer 0   gru_wide_fwd_step_kernel's tiling and arithmetic, the tile of gru_wide_tile.h (32 rows x 16 units x three gates per
//             workgroup, four waves split K, three-term bf16 operands, partial sums added in wave order, GRU_ROUNDING); the input
//             projection is never materialised: gi0 = ptab[previous note] + gib[beat * B + row], read and added in the epilogue.
//             h_prev = h0_l0[beat] at j == 0.
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
#include "gru_wide_tile.h"

namespace arvae {

constexpr int TW_ORT = 16;                 // batch rows per workgroup of the logits + pick kernel (the recurrence kernels': GWT_RT)
constexpr int TW_VMAX = 128;               // notes: eight 16-note tiles, two per wave

enum { TW_ARGMAX = 0, TW_SAMPLE = 1, TW_FILTERED = 2 };

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

// ------------------------------------------------------------------------------------------------------------------
// Layer 0 of tick t: gh = h_prev . W_hh0^T for the tile, gi = ptab[previous note] + gib[beat], then r, z, n, h'.
template <int H>
__global__ __launch_bounds__(64 * GWT_WAVES) void tick_wide_l0_kernel(TickWide p, int t) {
    constexpr int NU = H / 16;
    static_assert(NU % 8 == 0, "unit tiles in multiples of the XCD count");
    __shared__ __attribute__((aligned(16))) GwtRed<3> red;                              // 24 KB
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * GWT_RT, unit0 = 16 * (blockIdx.x % NU);
    const int R = p.batch, beat = t / p.tpb;
    const bool restart = t % p.tpb == 0;
    const float *hp = restart ? p.h0_l0 + (int64_t)beat * R * p.h0_stride : p.hs0 + (int64_t)((t + 1) & 1) * R * H;
    const int64_t hp_stride = restart ? p.h0_stride : H;
    float *out = p.hs0 + (int64_t)(t & 1) * R * H;

    // the epilogue's operands are requested first: they arrive while the GEMM runs
    const GwtElems e = gwt_elems(w, lane, row0, unit0, R);
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
    gwt_gemm3<H, false>(acc, hp, hp_stride, nullptr, 1.f, p.w_hh0, row0, unit0, R, w, col, quad);
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
// Layer 1 of tick t: gi = (h_l0' (.) keep-mask * keep_scale) . W_ih1^T + b_ih1 and gh = h_l1_prev . W_hh1^T + b_hh1, then the gates.
template <int H, bool MASK>
__global__ __launch_bounds__(64 * GWT_WAVES) void tick_wide_l1_kernel(TickWide p, int t) {
    constexpr int NU = H / 16;
    __shared__ __attribute__((aligned(16))) GwtRed<6> red;                              // 48 KB: gates 0-2 of gi, 3-5 of gh
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int row0 = (blockIdx.x / NU) * GWT_RT, unit0 = 16 * (blockIdx.x % NU);
    const int R = p.batch, beat = t / p.tpb;
    const bool restart = t % p.tpb == 0;
    const float *x = p.hs0 + (int64_t)(t & 1) * R * H;                                   // layer 0's state of this tick
    const float *hp = restart ? p.h0_l1 + (int64_t)beat * R * p.h0_stride : p.hs1 + (int64_t)((t + 1) & 1) * R * H;
    const int64_t hp_stride = restart ? p.h0_stride : H;
    float *out = p.hs1 + (int64_t)(t & 1) * R * H;

    const GwtElems e = gwt_elems(w, lane, row0, unit0, R);
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
        if (half == 0) gwt_gemm3<H, MASK>(acc, x, H, MASK ? p.mask + (int64_t)t * R * H : nullptr, p.keep_scale, p.w_ih1, row0, unit0, R, w, col, quad);
        else gwt_gemm3<H, false>(acc, hp, hp_stride, nullptr, 1.f, p.w_hh1, row0, unit0, R, w, col, quad);
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
// Logits of tick t for 16 rows and the rows' picks.  Wave w computes the 16-note tiles w and w + 4 over the whole K.
template <int H, int PICK>
__global__ __launch_bounds__(64 * GWT_WAVES) void tick_wide_out_kernel(TickWide p, int t) {
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
                gwt_load_split(a_src + 32 * ks, ah, am, al);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (!have[i]) continue;
                    gwt_load_split(w_src[i] + 32 * ks, wh, wm, wl);
                    GRU_MFMA6(acc[i], ah, am, al, wh, wm, wl);
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
            for (int i = tid; i < TW_ORT * V; i += 64 * GWT_WAVES) {
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
        for (int i = tid; i < TW_ORT * V; i += 64 * GWT_WAVES) {
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
            for (int i = tid; i < TW_ORT * V; i += 64 * GWT_WAVES) {
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

static int64_t tw_prev_floats(int64_t batch) { return (batch + 3) / 4 * 4; }

}  // namespace arvae

using namespace arvae;

extern "C" int arvae_tick_free_run_wide_supported(int32_t hidden, int32_t vocab) {
    return gwt_hidden_built(hidden) && vocab >= 2 && vocab <= TW_VMAX;
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
    ARVAE_REQUIRE(gwt_hidden_built(hidden), "tick_free_run_wide: hidden size %d is not built (256, 512)", hidden);
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
    ARVAE_REQUIRE(ws != nullptr && gwt_aligned16(ws), "tick_free_run_wide: workspace missing or not 16-byte aligned (arvae_tick_free_run_wide_ws_floats)");
    ARVAE_REQUIRE(gwt_aligned16(wts->w_hh0) && gwt_aligned16(wts->w_ih1) && gwt_aligned16(wts->w_hh1) && gwt_aligned16(wts->w_out) && gwt_aligned16(h0_l0) &&
                      gwt_aligned16(h0_l1),
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
    const dim3 block(64 * GWT_WAVES), grid((batch + GWT_RT - 1) / GWT_RT * (hidden / 16)), grid_out((batch + TW_ORT - 1) / TW_ORT);
    const bool known = gwt_with_hidden(hidden, [&](auto HH) {
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
