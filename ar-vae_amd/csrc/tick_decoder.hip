// Free-running tick decoder of the MeasureVAE path: the argmax- or multinomial-feedback pass of the hierarchical decoder
// (measurevae/decoder.py:459-525 with teacher forcing off: the embedding of the previous tick's note is the next input) in ONE launch
// that returns only the tokens.  The differentiable graph is then evaluated on those tokens by the whole-sequence kernels of
// gru_seq.hip (the pick is not differentiated), so nothing else has to be saved here.
//
// Every batch row is an independent 24-tick recurrence: a workgroup owns its rows for the whole pass, H/16 waves, wave w owns hidden
// units [16w, 16w+16).  Per tick:   gi0 = gib[beat][row] + ptab[previous token]      (both precomputed by dense launches)
//   layer 0: gh0 = W_hh0 h0 -> gates -> h0' ; mid = h0' * keep-mask * scale
//   layer 1: r,z: W_ih1 mid + W_hh1 h1 in one accumulator each; n: the two products apart -> gates -> h1'
//   logits = relu(W_out h1' + b_out) on waves 0..ceil(V/16)-1, the row's pick (PICK_ARGMAX: lowest index on ties) through DPP rows
//            and LDS -> token, fed back.  (PICK_MULTINOMIAL: a drawn note; PICK_FILTERED: drawn among the notes a mask, a top-k and a
//            nucleus cut leave -- tick_filtered_pick; PICK_PLANNED: the same with the mask read per (row, tick) from a note plan, so
//            that a tick with one allowed note forces it and the forced note is what the next tick is fed: infilling.)
// The products run on the fp16 MFMA with the scaled two-term operands of gru_seq_fwd_h2_kernel (splitmath.h); the recurrent matrices
// are split and laid out for streaming by one prep pair per call (tick_amax_kernel, tick_prep_kernel) into the caller's workspace.
// Two kernels: tick_free_run_h2_kernel for the reference's two layers, tick_free_run_layers_kernel behind it for one, three and four.
#include <algorithm>
#include <cmath>
#include "diag.h"
#include "common.h"
#include "dispatch.h"
#include "splitmath.h"
#include "gru_common.h"
#include "stamps.h"
#include "tick_common.h"

namespace arvae {

#ifdef ARVAE_STAMPS_TICK
// diagnostic build only (stamps.h): cycles per phase of a tick + the tick count, wave GRU_STAMP_WAVE of workgroup 0; a mark waits for
ARVAE_STAMP_TABLE(tick, 1, 9, 1)                               // the wave's LDS traffic first
#define TSTAMP_BEGIN() PhaseSums<8> tph
#define TSTAMP(k) do { stamp_wait_lds(); tph.mark(k); } while (0)
#define TSTAMP_DEPEND(v) stamp_depend(v)
#define TSTAMP_END(ticks) do { if (blockIdx.x == 0 && threadIdx.x == 64 * GRU_STAMP_WAVE) tph.flush(g_tick_stamps, ticks); } while (0)
#else
#define TSTAMP_BEGIN()
#define TSTAMP(k)
#define TSTAMP_DEPEND(v)
#define TSTAMP_END(ticks)
#endif

struct TickFreeRun {
    const float *w_hh0, *b_hh0, *w_ih1, *b_ih1, *w_hh1, *b_hh1, *w_out, *b_out;
    const float *h0_l0, *h0_l1;    // [beats*B] rows of H values h0_stride floats apart, row = beat*B + b
    int64_t h0_stride;
    const float *gib;              // [beats*B][3H]
    const float *ptab;             // [V+1][3H]; row V = the start token
    const uint8_t *mask;           // [beats*tpb][B][H] or null
    float keep_scale;
    int batch, beats, tpb, vocab;
    int64_t *tokens;               // [B][beats*tpb]
};

// one stage of a (value, index) argmax inside a 16-lane DPP row: the partner lane's pair through a DPP move, larger value wins,
// equal values keep the lower index (commutative and associative: any sequence of pairings that connects the 16 lanes gives the
// row's maximum with its lowest index in every lane)
template <int CTRL>
__device__ __forceinline__ void tick_argmax_stage(float &v, int &ix) {
    const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
    const int oi = __builtin_amdgcn_update_dpp(0, ix, CTRL, 0xf, 0xf, true);
    const bool take = ov > v || (ov == v && oi < ix);
    v = take ? ov : v;
    ix = take ? oi : ix;
}

// inclusive prefix sum over the 16 lanes of a DPP row, in every lane: four row shifts (lanes the shift leaves without a source add 0)
template <int CTRL> __device__ __forceinline__ float dpp_shr_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_prefix(float v) {
    v = dpp_shr_add<0x111>(v);
    v = dpp_shr_add<0x112>(v);
    v = dpp_shr_add<0x114>(v);
    return dpp_shr_add<0x118>(v);
}

// what the free-running kernel feeds back (measurevae/decoder.py:502-516): the top-1 note, or a note drawn from softmax(logits / T)
// PICK_FILTERED: the multinomial draw over the notes a mask, a top-k and a nucleus (top-p) cut leave (generation only: no keep-masks)
// PICK_PLANNED: PICK_FILTERED's draw with the allowed notes read per (row, tick) from a note plan (arvae_note_plan_t): infilling
constexpr int PICK_ARGMAX = 0, PICK_MULTINOMIAL = 1, PICK_FILTERED = 2, PICK_PLANNED = 3;
// the draws of PICK_MULTINOMIAL: u [batch][ticks] in (0, 1] and 1 / T (null and unused for PICK_ARGMAX)
struct TickSample {
    const float *u;
    float inv_t;
};
// PICK_FILTERED's: the draws, top_k in [1, vocab] (the entry points turn 0 = off into vocab), top_p in (0, 1] (1 = off) and the allowed
// notes' bytes [vocab] (null: all).  A type of its own, so that the other picks' kernel arguments stay what they were.
struct TickFilter {
    const float *u;
    float inv_t;
    int top_k;
    float top_p;
    const uint8_t *allow;
};
// PICK_PLANNED's: the draws and the cuts as TickFilter's; allow[row * row_stride + tick * tick_stride + note] != 0: the note may be
// emitted by that row at that tick (strides in bytes, 0 = the same for every row / tick).  Again a type of its own.
struct TickPlan {
    const float *u;
    float inv_t;
    int top_k;
    float top_p;
    const uint8_t *allow;
    int64_t row_stride, tick_stride;
};
template <int PICK> struct TickPick { using type = TickSample; };
template <> struct TickPick<PICK_FILTERED> { using type = TickFilter; };
template <> struct TickPick<PICK_PLANNED> { using type = TickPlan; };
// the picks that publish a row's logits to LDS and rank them behind the barrier (tick_filtered_pick)
template <int PICK> constexpr bool tick_row_pick = PICK == PICK_FILTERED || PICK == PICK_PLANNED;
// the cuts of either as tick_filtered_pick takes them (it does not read `allow`: the banned notes are -1 in the row by then)
__device__ __forceinline__ const TickFilter &tick_cuts(const TickFilter &f) { return f; }
__device__ __forceinline__ TickFilter tick_cuts(const TickPlan &f) { return TickFilter{f.u, f.inv_t, f.top_k, f.top_p, nullptr}; }

// PICK_FILTERED behind the barrier.  The tile waves have published the row's logits to LDS: `lg` = the row's FLT_LS floats, banned
// notes and notes past the vocabulary as -1 (below every relu output), columns past the last tile -1 from the kernel's start.  The 16
// lanes of a DPP row share the row; lane `col` owns notes col, 16 + col, 32 + col, 48 + col.  Order: descending logit, ties to the
// lower index (the argmax pick's rule), on the logits' bits as integers (non-negative floats order as their bits; the sign bit is
// cleared, so that a -0 is a 0).  One walk over the row's `nnote` notes (LDS broadcast reads, 16 bytes each) gives each owned note
// v its rank (how many notes are ordered before it) and the sum of e_n = exp((l_n - M) / T) over those notes; v survives iff it is
// allowed, rank < top_k and that sum < top_p * S, S = the sum of e over the notes top_k leaves (row16_sum: the same bits in every
// lane).  The sums grow with the rank (float addition is monotone), so the survivors are a leading run of the order, and the first
// note's sum is 0 < top_p * S: it always survives.  The draw is arvae_tick_free_run_sampled's over the survivors in index order:
// e's inclusive prefixes tile by tile (row16_prefix, a tile's total = its last lane's prefix carried into the next), the first
// SURVIVING note whose prefix reaches u * (the last survivor's prefix).  Nothing allowed: note 0.
__device__ __forceinline__ int tick_filtered_pick(const float *lg, int col, int quad, int nnote, float u, const TickFilter &f, int vocab) {
    float lv[4], before[4] = {0.f, 0.f, 0.f, 0.f};
    int key[4], rank[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        lv[c] = lg[16 * c + col];
        key[c] = lv[c] >= 0.f ? (__builtin_bit_cast(int, lv[c]) & 0x7fffffff) : -1;
    }
    const float big = row16_max(fmaxf(fmaxf(lv[0], lv[1]), fmaxf(lv[2], lv[3])));
    for (int n4 = 0; n4 < nnote; n4 += 4) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(lg + n4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n4 + j;
            const float ln = q[j];                             // (a scalar copy of the element: tools/probes/bitcast_vector_element.hip)
            const int kn = ln >= 0.f ? (__builtin_bit_cast(int, ln) & 0x7fffffff) : -1;
            const float en = __expf((ln - big) * f.inv_t);     // (a banned note is ordered before no allowed one: its e is never added)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool first = kn > key[c] || (kn == key[c] && n < 16 * c + col);
                rank[c] += first ? 1 : 0;
                before[c] += first ? en : 0.f;
            }
        }
    }
    float e[4];
    bool keep[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        keep[c] = key[c] >= 0 && rank[c] < f.top_k;
        e[c] = keep[c] ? __expf((lv[c] - big) * f.inv_t) : 0.f;
    }
    const float cut = f.top_p * row16_sum((e[0] + e[1]) + (e[2] + e[3]));
    float run = 0.f, pre[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        keep[c] = keep[c] && (f.top_p >= 1.f || before[c] < cut);
        pre[c] = run + row16_prefix(keep[c] ? e[c] : 0.f);
        run = __shfl(pre[c], 15, 16);                          // the tile's last prefix: the next tile's base
    }
    // C_last is the LAST SURVIVOR's own prefix, not lane 15's: the four shifts of row16_prefix add a lane's terms in an order that
    // depends on the lane, so a lane behind the last survivor can hold the same sum one ulp higher, and u = 1 against that value
    // would be reached by no survivor.  u * (its own prefix) <= that prefix for u <= 1: the last survivor always reaches the target.
    int last = -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int bits = (int)((unsigned)(__ballot(keep[c]) >> (16 * quad)) & 0xffffu);
        last = bits != 0 ? 16 * c + 31 - __clz(bits) : last;
    }
    float mine = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) mine = (last >> 4) == c ? pre[c] : mine;
    const float target = u * __shfl(mine, last & 15, 16);
    int ix = max(last, 0);                                     // (not finite: no test below holds, the last survivor; no survivor: note 0)
#pragma unroll
    for (int c = 3; c >= 0; --c) {
        const unsigned long long reached = __ballot(keep[c] && pre[c] >= target);
        const int bits = (int)((unsigned)(reached >> (16 * quad)) & 0xffffu);
        ix = bits != 0 ? 16 * c + __ffs(bits) - 1 : ix;
    }
    return min(ix, vocab - 1);
}

// ------------------------------------------------------------------------------------------------------------------
// The two-layer kernel (the reference's tick RNN as configured: the flagship workload).
// (RW: batch rows per workgroup, 16 or 4 -- one element per lane and four times the workgroups, as gru_seq_fwd_h2_kernel: the gates,
// the token's projections, the state splits and the rows' argmax are per-element work; the weight stream per workgroup is unchanged)
//
// PICK_MULTINOMIAL replaces the two halves of the pick, at the same two barriers.  Behind the logits a wave holds, per row, its tile's
// 16 notes in one DPP row: it takes the tile's maximum m_c (row16_max), e_v = exp((l_v - m_c) / T) (0 for notes past the
// vocabulary) and the 16 inclusive prefixes of e (row16_prefix), and publishes m_c, the 16 prefixes and (as the last of them) the
// tile's sum to LDS.  Behind the barrier every lane rescales the at most four tile sums to the row's maximum M = max_c m_c
// (s_c = exp((m_c - M) / T) <= 1, the tile that holds M keeps its e = 1: the total is >= 1), accumulates them tile by tile
// (S_c = fma(sum_c, s_c, S_(c-1))), takes target = u * S_last, the first tile with S_c >= target, and in it the first note
// with fma(prefix_k, s_c, S_(c-1)) >= target: lane `col` tests note `col`, the lowest set ballot bit of the row is the note.  A
// tile's sum is the prefix of its last note INSIDE the vocabulary, so that note's test is the expression that made S_c and the
// tile's search ends on a note that exists; S_last >= u * S_last (u clamped to [0, 1]) ends the tiles'.
template <int H, bool MASKED, int RW, int PICK>
__global__ __launch_bounds__(H * 4) void tick_free_run_h2_kernel(TickFreeRun p, const uint4 *__restrict__ packed, typename TickPick<PICK>::type smp) {
    static_assert(RW == 16 || RW == 8 || RW == 4, "16, 8 or 4 rows: four, two or one per lane");
    constexpr int E = RW / 4;
    constexpr int NW = H / 16, KS = H / 32, KQ = H / 16;
    constexpr int NGG = 9 * KS;                    // weight groups per tick: (matrix, k-step, gate), 3 x 16 bytes per lane each
    constexpr int RS = NGG % 6 == 0 ? 6 : 3;       // register ring of groups; RS - 1 groups are in flight
    constexpr int PFD = RS - 1;
    constexpr int HP = H + 8, PLANE = 16 * HP, HS = H + 4;
    __shared__ __attribute__((aligned(16))) unsigned short hA0[2][2 * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short hA1[2][2 * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short midp[2 * PLANE];
    __shared__ __attribute__((aligned(16))) float h1f[16][HS];
    __shared__ __attribute__((aligned(16))) float wout_s[64][HS];
    __shared__ float cand_v[4][16];
    __shared__ float hmax[H / 16];
    __shared__ int cand_i[4][16];
    __shared__ float smp_max[4][16];               // PICK_MULTINOMIAL: [tile][row] maximum, [tile][row][note] inclusive prefixes of e
    __shared__ float smp_pre[4][16][16];
    __shared__ __attribute__((aligned(16))) float flt_lg[tick_row_pick<PICK> ? 16 * FLT_LS : 4];   // PICK_FILTERED, PICK_PLANNED: [row] the logits
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int unit = 16 * w + col;
    const int row0 = blockIdx.x * RW;
    const int B = p.batch;
    const int ntile = (p.vocab + 15) / 16;

    // weight stream: one buffer resource, one per-lane byte offset, the group's offset as the scalar offset of each
    // load -- per-load 64-bit addresses would be hoisted out of the tick loop into 200+ VGPRs
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(packed), 0, 3 * KS * NW * 6 * 64 * 16, 0x00020000);
    const int wlane = (w * 6 * 64 + lane) * 16;
    f16x8 wb[RS][2];
    auto fetch = [&](int gg) {                     // gg = (matrix * KS + ks) * 3 + gate, compile-time at every call site
        const int g = gg / 3, gate = gg % 3;
#pragma unroll
        for (int term = 0; term < 2; ++term)
            wb[gg % RS][term] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wlane, (g * NW * 6 + gate * 2 + term) * 64 * 16, 0));
    };
#pragma unroll
    for (int d = 0; d < PFD; ++d) fetch(d % NGG);

    for (int e = threadIdx.x; e < 64 * H; e += H * 4) {       // note projection weights -> LDS (rows >= vocab: zeros)
        const int n = e / H, k = e - n * H;
        wout_s[n][k] = n < p.vocab ? p.w_out[(int64_t)n * H + k] : 0.f;
    }
    const float b0r = p.b_hh0[unit], b0z = p.b_hh0[H + unit], b0n = p.b_hh0[2 * H + unit];
    const float b1r = p.b_ih1[unit] + p.b_hh1[unit], b1z = p.b_ih1[H + unit] + p.b_hh1[H + unit];
    const float b1in = p.b_ih1[2 * H + unit], b1hn = p.b_hh1[2 * H + unit];
    const int note = 16 * w + col;
    const bool note_ok = w < ntile && note < p.vocab;
    const float bout = note_ok ? p.b_out[note] : 0.f;
    bool note_on = note_ok;                                    // PICK_FILTERED: the note may be emitted
    if constexpr (PICK == PICK_FILTERED) {
        if (note_ok && smp.allow != nullptr) note_on = smp.allow[note] != 0;
    }
    if constexpr (tick_row_pick<PICK>) {
        for (int e = threadIdx.x; e < 16 * FLT_LS; e += H * 4) flt_lg[e] = -1.f;    // (columns past the last tile stay -1)
    }

    auto lrow = [&](int i) { return gru_lrow<E>(quad, i); };                  // the tile row of this lane's element i
    int rows[E];
    bool live[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int r = row0 + lrow(i);
        live[i] = r < B;
        rows[i] = live[i] ? r : B - 1;
    }
    float h0[E], h1[E], gb[E][3];
    int tok[E];
#pragma unroll
    for (int i = 0; i < E; ++i) tok[i] = p.vocab;
    const int ticks = p.beats * p.tpb;
    // operand scales from the data (round 5): the matrices' from their maxima (tick_amax_kernel, behind the packed weights), the
    // states' per beat from the workgroup's rows -- every state of a beat is a convex combination of tanh outputs and the beat's
    // initial state, the layer-1 input is a layer-0 state times a keep byte's 0 or keep_scale
    const float *wmax = reinterpret_cast<const float *>(packed) + 9 * H * H;
    const float w0_inv = tick_scale(wmax, 0).inv, w12_inv = tick_scale(wmax, 1).inv;
    const float keep_bound = MASKED ? fmaxf(p.keep_scale, 1.f) : 1.f;
    float h_s = 1.f, us0 = 1.f, us12 = 1.f;                   // (set at every beat's start: tick 0 starts one)
    const int arow = gru_arow<E>(col);
    const int aoff = arow * HP + 8 * quad;                    // this lane's A-operand offset inside a plane
    auto elems = [&](const f32x4 &acc, float (&out)[E]) __attribute__((always_inline)) { gru_elems<E>(acc, out); };
    // layer 0's recurrent product W_hh0 h0 of a tick does not wait for the tick's token: it is multiplied at the END of the previous
    // tick, under the logits and the argmax (three waves' latency chain of ~3500 cycles, during which the workgroup's weight
    // stream -- what bounds the layers: 590 KB per tick at the CU's 64 bytes per clock -- stood still; tools/stamp.py tick).
    // A beat's first tick starts from the beat's own state and multiplies at its top, as every tick did.
    f32x4 acc0[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    // the 3 KS weight groups of matrix 0 against the state image `ab`; piece(g) runs behind group g
    auto layer0 = [&](const unsigned short *ab, auto piece) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 3; ++q) acc0[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f16x8 ah = lds_x8<f16x8>(ab + 32 * ks), al = lds_x8<f16x8>(ab + PLANE + 32 * ks);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int gg = (0 * KS + ks) * 3 + q;
                fetch((gg + PFD) % NGG);
                __builtin_amdgcn_sched_barrier(0);
                GRU_MFMA3(acc0[q], ah, al, wb[gg % RS][0], wb[gg % RS][1]);
                __builtin_amdgcn_sched_barrier(0);
                piece(gg);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    auto no_piece = [](int) __attribute__((always_inline)) {};
    TSTAMP_BEGIN();
    for (int t = 0; t < ticks; ++t) {
        const int cur = t & 1;
        const int beat = t / p.tpb;
        const bool beat_start = t % p.tpb == 0;
        if (beat_start) {
            lds_barrier();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int64_t br = (int64_t)beat * B + rows[i];
                h0[i] = p.h0_l0[br * p.h0_stride + unit];
                h1[i] = p.h0_l1[br * p.h0_stride + unit];
                const float *g = p.gib + br * 3 * H + unit;
                gb[i][0] = g[0]; gb[i][1] = g[H]; gb[i][2] = g[2 * H];
            }
            {   // the beat's state scale: max(keep bound, keep bound * |h0|, |h1|) over the workgroup's rows just below 2^15
                float mx = keep_bound;
#pragma unroll
                for (int i = 0; i < E; ++i) mx = fmaxf(mx, fmaxf(keep_bound * fabsf(h0[i]), fabsf(h1[i])));
                mx = row16_max(mx);
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                if (lane == 0) hmax[w] = mx;
                lds_barrier();
#pragma unroll
                for (int q = 0; q < H / 16; ++q) mx = fmaxf(mx, hmax[q]);
                const Pow2 sh = pow2_for(mx);
                h_s = sh.s;
                us0 = sh.inv * w0_inv;
                us12 = sh.inv * w12_inv;
            }
#pragma unroll
            for (int i = 0; i < E; ++i) {
                store_split2<false>(&hA0[cur][lrow(i) * HP + unit], PLANE, h0[i], h_s);
                store_split2<false>(&hA1[cur][lrow(i) * HP + unit], PLANE, h1[i], h_s);
            }
            lds_barrier();
        }
        float gi[E][3], keep[E];
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const float *pt = p.ptab + (int64_t)tok[i] * 3 * H + unit;
            gi[i][0] = gb[i][0] + pt[0]; gi[i][1] = gb[i][1] + pt[H]; gi[i][2] = gb[i][2] + pt[2 * H];
            keep[i] = MASKED ? p.keep_scale * (float)p.mask[((int64_t)t * B + rows[i]) * H + unit] : 1.f;
        }
        float un[E];                                           // this tick's draws of the lane's rows (PICK_MULTINOMIAL, PICK_FILTERED)
        if constexpr (PICK != PICK_ARGMAX) {
#pragma unroll
            for (int i = 0; i < E; ++i) un[i] = fminf(fmaxf(smp.u[(int64_t)rows[i] * ticks + t], 0.f), 1.f);
        }
        // PICK_PLANNED: the tick's plan bytes of the lane's note, one per row element, requested here at the tick's top: they do not
        // depend on the recurrence, so their latency lies under the layers' products and not in front of the logits' barrier.  Raw
        // until the logits are published (converted here they would be waited for at once)
        [[maybe_unused]] unsigned plan_b[PICK == PICK_PLANNED ? E : 1];
        if constexpr (PICK == PICK_PLANNED) {
#pragma unroll
            for (int i = 0; i < E; ++i) plan_b[i] = smp.allow[rows[i] * smp.row_stride + t * smp.tick_stride + (note_ok ? note : 0)];
        }
        TSTAMP(0);                                             // tick top: a beat's state; the token's projections requested
        // ---- layer 0: matrix 0 (multiplied at the end of the previous tick unless a beat starts)
        {
            if (beat_start) layer0(&hA0[cur][aoff], no_piece);
            TSTAMP_DEPEND(acc0[0][0] + acc0[1][1] + acc0[2][3]);
            TSTAMP(1);                                         // layer 0 at the top (a beat's first tick only)
            float ar[E], az[E], an[E];
            elems(acc0[0], ar); elems(acc0[1], az); elems(acc0[2], an);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float r = fast_sigmoid(gi[i][0] + ar[i] * us0 + b0r);
                const float z = fast_sigmoid(gi[i][1] + az[i] * us0 + b0z);
                const float n = fast_tanh(gi[i][2] + r * (an[i] * us0 + b0n));
                h0[i] = (1.f - z) * n + z * h0[i];
                store_split2<false>(&hA0[cur ^ 1][lrow(i) * HP + unit], PLANE, h0[i], h_s);
                store_split2<false>(&midp[lrow(i) * HP + unit], PLANE, h0[i] * keep[i], h_s);
            }
        }
        TSTAMP(2);                                             // layer 0 gates (wait for the projections) + LDS writes
        lds_barrier();
        TSTAMP(3);
        // ---- layer 1: matrix 1 (W_ih1 on mid), matrix 2 (W_hh1 on h1); r and z share an accumulator
        {
            f32x4 a1[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // r, z, i_n, h_n
#pragma unroll
            for (int m = 1; m <= 2; ++m) {
                const unsigned short *ab = m == 1 ? &midp[aoff] : &hA1[cur][aoff];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const f16x8 ah = lds_x8<f16x8>(ab + 32 * ks), al = lds_x8<f16x8>(ab + PLANE + 32 * ks);
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const int gg = (m * KS + ks) * 3 + q;
                        fetch((gg + PFD) % NGG);
                        __builtin_amdgcn_sched_barrier(0);
                        GRU_MFMA3(a1[q == 2 ? m + 1 : q], ah, al, wb[gg % RS][0], wb[gg % RS][1]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            TSTAMP_DEPEND(a1[0][0] + a1[1][1] + a1[2][3] + a1[3][2]);
            TSTAMP(4);                                         // layer 1: operand reads + MFMAs behind the weight stream
            float ar[E], az[E], ai[E], ah[E];
            elems(a1[0], ar); elems(a1[1], az); elems(a1[2], ai); elems(a1[3], ah);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float r = fast_sigmoid(ar[i] * us12 + b1r);
                const float z = fast_sigmoid(az[i] * us12 + b1z);
                const float n = fast_tanh(ai[i] * us12 + b1in + r * (ah[i] * us12 + b1hn));
                h1[i] = (1.f - z) * n + z * h1[i];
                store_split2<false>(&hA1[cur ^ 1][lrow(i) * HP + unit], PLANE, h1[i], h_s);
                h1f[lrow(i)][unit] = h1[i];
            }
        }
        TSTAMP(5);                                             // layer 1 gates + LDS writes
        lds_barrier();
        // ---- logits (fp32 MFMA, weights in LDS) + row argmax on the first waves; on every wave the NEXT tick's layer 0
        {
            const bool pre = t + 1 < ticks && (t + 1) % p.tpb != 0;
            const unsigned short *ab_next = &hA0[cur ^ 1][aoff];
            if (w < ntile) {
                f32x4 lg = {0.f, 0.f, 0.f, 0.f};
                auto logits_step = [&](int kq) __attribute__((always_inline)) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(&h1f[arow][16 * kq + 4 * quad]);
                    const f32x4 b = *reinterpret_cast<const f32x4 *>(&wout_s[note][16 * kq + 4 * quad]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) lg = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], lg, 0, 0, 0);
                };
                // the four rows' (value, lowest index) maxima over the tile's 16 notes = one DPP row each: lane pairings on the
                // vector ALU (quad permutes, then the half-row and the row mirrored) instead of four ds_bpermute round trips per
                // row; stage by stage over the four rows (four independent chains), one block of candidate writes
                auto argmax_rows = [&]() __attribute__((always_inline)) {
                    float v[E], lv[E];
                    int ix[E];
                    elems(lg, lv);
                    if constexpr (PICK == PICK_MULTINOMIAL) {
                        // the tile's maximum, e relative to it and e's prefixes per row; stage by stage over the rows, as below
                        float mx[E], pre[E];
#pragma unroll
                        for (int i = 0; i < E; ++i) { v[i] = note_ok ? fmaxf(lv[i] + bout, 0.f) : -1.f; mx[i] = row16_max(v[i]); }
#pragma unroll
                        for (int i = 0; i < E; ++i) pre[i] = note_ok ? __expf((v[i] - mx[i]) * smp.inv_t) : 0.f;
#pragma unroll
                        for (int i = 0; i < E; ++i) pre[i] = row16_prefix(pre[i]);
#pragma unroll
                        for (int i = 0; i < E; ++i) smp_pre[w][lrow(i)][col] = pre[i];
                        if (col == 0) {
#pragma unroll
                            for (int i = 0; i < E; ++i) smp_max[w][lrow(i)] = mx[i];
                        }
                        return;
                    }
                    if constexpr (PICK == PICK_FILTERED) {     // the row's logits to LDS; every lane ranks and draws behind the barrier
#pragma unroll
                        for (int i = 0; i < E; ++i) flt_lg[lrow(i) * FLT_LS + note] = note_on ? fmaxf(lv[i] + bout, 0.f) : -1.f;
                        return;
                    }
                    if constexpr (PICK == PICK_PLANNED) {      // the same, the note's flag this row's at this tick
#pragma unroll
                        for (int i = 0; i < E; ++i) flt_lg[lrow(i) * FLT_LS + note] = note_ok && plan_b[i] != 0 ? fmaxf(lv[i] + bout, 0.f) : -1.f;
                        return;
                    }
#pragma unroll
                    for (int i = 0; i < E; ++i) { v[i] = note_ok ? fmaxf(lv[i] + bout, 0.f) : -1.f; ix[i] = note; }
#pragma unroll
                    for (int i = 0; i < E; ++i) tick_argmax_stage<0xB1>(v[i], ix[i]);
#pragma unroll
                    for (int i = 0; i < E; ++i) tick_argmax_stage<0x4E>(v[i], ix[i]);
#pragma unroll
                    for (int i = 0; i < E; ++i) tick_argmax_stage<0x141>(v[i], ix[i]);
#pragma unroll
                    for (int i = 0; i < E; ++i) tick_argmax_stage<0x140>(v[i], ix[i]);
                    if (col == 0) {
#pragma unroll
                        for (int i = 0; i < E; ++i) { cand_v[w][lrow(i)] = v[i]; cand_i[w][lrow(i)] = ix[i]; }
                    }
                };
                constexpr int NG0 = 3 * KS;
                if (pre) {
                    // the logits' k-steps behind matrix 0's first groups, the rows' argmax behind the next one
                    layer0(ab_next, [&](int g) __attribute__((always_inline)) {
                        if (g < KQ) logits_step(g);
                        else if (g == KQ) argmax_rows();
                    });
                    if (NG0 <= KQ) argmax_rows();
                } else {
#pragma unroll
                    for (int kq = 0; kq < KQ; ++kq) logits_step(kq);
                    argmax_rows();
                }
            } else if (pre) {
                layer0(ab_next, no_piece);
            }
            TSTAMP_DEPEND(acc0[0][0] + acc0[1][1] + acc0[2][3]);
        }
        TSTAMP(6);                                             // barrier + logits / argmax (first waves) + the next tick's layer 0
        lds_barrier();
        if constexpr (PICK == PICK_MULTINOMIAL) {
            // tile sums rescaled to the row's maximum -> the tile, then the note inside it (one lane per note, the quad's ballot bits)
            int tile[E];
            float base[E], scale[E], target[E];
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int r = lrow(i);
                float m[4], sum[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool on = c < ntile;
                    m[c] = on ? smp_max[c][r] : -1.f;
                    sum[c] = on ? smp_pre[c][r][min(15, p.vocab - 1 - 16 * c)] : 0.f;    // the tile's last note's own prefix
                }
                const float big = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
                float sc[4], run[5];
                run[0] = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sc[c] = __expf((m[c] - big) * smp.inv_t);
                    run[c + 1] = __builtin_fmaf(sum[c], sc[c], run[c]);
                }
                target[i] = un[i] * run[4];                    // (tiles past the vocabulary add 0: run[4] is the last live tile's)
                tile[i] = 0; base[i] = run[0]; scale[i] = sc[0];
#pragma unroll
                for (int c = 1; c < 4; ++c) {
                    const bool next = run[c] < target[i];      // tile c - 1 ends below the target: the note lies further on
                    tile[i] = next ? c : tile[i];
                    base[i] = next ? run[c] : base[i];
                    scale[i] = next ? sc[c] : scale[i];
                }
            }
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float ck = __builtin_fmaf(smp_pre[tile[i]][lrow(i)][col], scale[i], base[i]);
                const unsigned long long reached = __ballot(ck >= target[i]);
                // (a row whose logits are not finite compares false everywhere: clamped to a note that exists)
                const int ix = min(max(16 * tile[i] + __ffs((int)((unsigned)(reached >> (16 * quad)) & 0xffffu)) - 1, 0), p.vocab - 1);
                tok[i] = ix;
                if (w == 0 && col == 0 && live[i]) p.tokens[(int64_t)rows[i] * ticks + t] = ix;
            }
        } else if constexpr (tick_row_pick<PICK>) {
            const auto cuts = tick_cuts(smp);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int ix = tick_filtered_pick(&flt_lg[lrow(i) * FLT_LS], col, quad, 16 * ntile, un[i], cuts, p.vocab);
                tok[i] = ix;
                if (w == 0 && col == 0 && live[i]) p.tokens[(int64_t)rows[i] * ticks + t] = ix;
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int r = lrow(i);
                float v = cand_v[0][r];
                int ix = cand_i[0][r];
                for (int c = 1; c < ntile; ++c) {
                    const float ov = cand_v[c][r];
                    const int oi = cand_i[c][r];
                    const bool take = ov > v;                  // later tiles hold larger indices: ties keep the earlier
                    v = take ? ov : v;
                    ix = take ? oi : ix;
                }
                tok[i] = ix;
                if (w == 0 && col == 0 && live[i]) p.tokens[(int64_t)rows[i] * ticks + t] = ix;
            }
        }
        TSTAMP(7);                                             // barrier + the tiles' candidates -> token
    }
    TSTAMP_END(ticks);
}

// ------------------------------------------------------------------------------------------------------------------
// The free-running tick decoder for layer counts other than two (nn.GRU(num_layers = L), measurevae/decoder.py:331-363): the contract of
// tick_free_run_h2_kernel -- pre-multiplied layer-0 projections, state restart per beat, tokens as the only output, the same two picks --
// with the layer stack a template parameter.  Two layers keep their own kernel above.  What differs from it (the reading aid for
// DESIGN.md section 4, item 55):
//   1. no layer-0 product under the logits: every tick multiplies W_hh0 h0 at its top (at L = 1 there is nothing else to hide it
//      behind, at L >= 3 the stream of 2L - 1 matrices is what bounds a tick);
//   2. NMID boundary planes instead of the one midp: two from L = 3 on, alternating, because a layer's gates write the next
//      boundary while other waves still read the last;
//   3. the per-beat state scale is taken over ALL L initial states of the workgroup's rows (one h_s for every layer), where the
//      two-layer kernel takes it over its two.
//   matrices 0 .. 2L-2 of the packed workspace: W_hh0, then per upper layer l its W_ih_l (2l - 1) and W_hh_l (2l), every one as
//   scaled two-term fp16 in the per-lane order of tick_prep_kernel, streamed through one register ring across the tick;
//   scales: W_hh0 its own, W_ih_l and W_hh_l one between them (r and z share accumulators), the states one per beat = the maximum
//   over the workgroup's rows of ALL L initial states (times the keep scale: a boundary's operand is a state times 0 or keep_scale);
//   boundary l -> l + 1 has its own keep-mask [ticks][B][H], l major; the logits read the TOP layer's state (layer 0's at L = 1).
// A workgroup owns its RW rows for the whole sequence: LDS barriers only, nothing waits on another workgroup.
// LDS (bytes): per layer the two state images of two fp16 planes, one boundary operand (two from L = 3 on, alternating: a layer's gates
// write the next boundary while other waves still read the last), the top state in fp32, W_out, the pick's scratch: 64032 at L = 1,
// H = 128; 62992 / 72208 at L = 3 / 4, H = 64 (multinomial) of the 163840 a workgroup may hold.
// Offered for L = 1 at every hidden size and L = 3, 4 up to hidden 64 (arvae_tick_free_run_layers_supported).
struct TickStack {
    const float *b_ih[TICK_MAX_LAYERS], *b_hh[TICK_MAX_LAYERS];    // (b_ih[0] unused: part of gib)
    const float *w_out, *b_out;
    const float *h0[TICK_MAX_LAYERS];                              // per layer [beats*B] rows of H values h0_stride floats apart
    int64_t h0_stride;
    const float *gib, *ptab;                                       // as TickFreeRun
    const uint8_t *mask;                                           // [L-1][beats*tpb][B][H] or null
    float keep_scale;
    int batch, beats, tpb, vocab;
    int64_t *tokens;
};

template <int H, int L, int RW, int PICK>
__global__ __launch_bounds__(H * 4) void tick_free_run_layers_kernel(TickStack p, const uint4 *__restrict__ packed, typename TickPick<PICK>::type smp) {
    static_assert(RW == 16 || RW == 8 || RW == 4, "16, 8 or 4 rows: four, two or one per lane");
    static_assert(L >= 1 && L <= TICK_MAX_LAYERS, "layer count");
    constexpr int E = RW / 4;
    constexpr int NW = H / 16, KS = H / 32, KQ = H / 16, M = 2 * L - 1;
    constexpr int NGG = 3 * M * KS;                // weight groups per tick: (matrix, k-step, gate), 2 x 16 bytes per lane each
    constexpr int RS = NGG % 6 == 0 ? 6 : 3;       // register ring of groups; RS - 1 groups are in flight
    constexpr int PFD = RS - 1;
    constexpr int HP = H + 8, PLANE = 16 * HP, HS = H + 4;
    constexpr int NMID = L > 2 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) unsigned short hA[L][2][2 * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short midp[NMID][2 * PLANE];
    __shared__ __attribute__((aligned(16))) float topf[16][HS];
    __shared__ __attribute__((aligned(16))) float wout_s[64][HS];
    __shared__ float cand_v[4][16];
    __shared__ float hmax[H / 16];
    __shared__ int cand_i[4][16];
    __shared__ float smp_max[4][16];
    __shared__ float smp_pre[4][16][16];
    __shared__ __attribute__((aligned(16))) float flt_lg[tick_row_pick<PICK> ? 16 * FLT_LS : 4];   // PICK_FILTERED, PICK_PLANNED: [row] the logits
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int unit = 16 * w + col;
    const int row0 = blockIdx.x * RW;
    const int B = p.batch;
    const int ntile = (p.vocab + 15) / 16;

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(packed), 0, M * KS * NW * 6 * 64 * 16, 0x00020000);
    const int wlane = (w * 6 * 64 + lane) * 16;
    f16x8 wb[RS][2];
    auto fetch = [&](int gg) {                     // gg = (matrix * KS + ks) * 3 + gate, compile-time at every call site
        const int g = gg / 3, gate = gg % 3;
#pragma unroll
        for (int term = 0; term < 2; ++term)
            wb[gg % RS][term] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wlane, (g * NW * 6 + gate * 2 + term) * 64 * 16, 0));
    };
#pragma unroll
    for (int d = 0; d < PFD; ++d) fetch(d % NGG);

    for (int e = threadIdx.x; e < 64 * H; e += H * 4) {       // note projection weights -> LDS (rows >= vocab: zeros)
        const int n = e / H, k = e - n * H;
        wout_s[n][k] = n < p.vocab ? p.w_out[(int64_t)n * H + k] : 0.f;
    }
    // layer 0: b_hh alone (b_ih is inside gib); upper layers: r and z take b_ih + b_hh, n keeps them apart
    float br[L], bz[L], bin[L], bhn[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const float *bh = p.b_hh[l];
        br[l] = bh[unit]; bz[l] = bh[H + unit]; bhn[l] = bh[2 * H + unit]; bin[l] = 0.f;
        if (l > 0) {
            const float *bi = p.b_ih[l];
            br[l] += bi[unit]; bz[l] += bi[H + unit]; bin[l] = bi[2 * H + unit];
        }
    }
    const int note = 16 * w + col;
    const bool note_ok = w < ntile && note < p.vocab;
    const float bout = note_ok ? p.b_out[note] : 0.f;
    bool note_on = note_ok;                                    // PICK_FILTERED: the note may be emitted
    if constexpr (PICK == PICK_FILTERED) {
        if (note_ok && smp.allow != nullptr) note_on = smp.allow[note] != 0;
    }
    if constexpr (tick_row_pick<PICK>) {
        for (int e = threadIdx.x; e < 16 * FLT_LS; e += H * 4) flt_lg[e] = -1.f;    // (columns past the last tile stay -1)
    }

    auto lrow = [&](int i) { return gru_lrow<E>(quad, i); };
    int rows[E];
    bool live[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int r = row0 + lrow(i);
        live[i] = r < B;
        rows[i] = live[i] ? r : B - 1;
    }
    float h[L][E], gb[E][3];
    int tok[E];
#pragma unroll
    for (int i = 0; i < E; ++i) tok[i] = p.vocab;
    const int ticks = p.beats * p.tpb;
    const bool masked = p.mask != nullptr;
    const uint8_t *mask_bytes = masked ? p.mask : reinterpret_cast<const uint8_t *>(p.gib);
    const float *wmax = reinterpret_cast<const float *>(packed) + 3 * M * H * H;
    float w_inv[L];
#pragma unroll
    for (int l = 0; l < L; ++l) w_inv[l] = tick_scale(wmax, 2 * l).inv;
    const float keep_bound = masked ? fmaxf(p.keep_scale, 1.f) : 1.f;
    float h_s = 1.f, us[L];
#pragma unroll
    for (int l = 0; l < L; ++l) us[l] = 1.f;
    const int arow = gru_arow<E>(col);
    const int aoff = arow * HP + 8 * quad;
    auto elems = [&](const f32x4 &acc, float (&out)[E]) __attribute__((always_inline)) { gru_elems<E>(acc, out); };
    // matrix m's 3 KS groups against the state image `ab`: gate q of every k-step into acc[q == 2 ? nslot : q]
    auto product = [&](auto mc, const unsigned short *ab, f32x4 (&acc)[4], int nslot) __attribute__((always_inline)) {
        constexpr int m = decltype(mc)::value;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f16x8 ah = lds_x8<f16x8>(ab + 32 * ks), al = lds_x8<f16x8>(ab + PLANE + 32 * ks);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int gg = (m * KS + ks) * 3 + q;
                fetch((gg + PFD) % NGG);
                __builtin_amdgcn_sched_barrier(0);
                GRU_MFMA3(acc[q == 2 ? nslot : q], ah, al, wb[gg % RS][0], wb[gg % RS][1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // layer l's new state of the lane's elements -> its next image, the boundary above it (times the keep byte) or, on top, the logits' fp32 operand
    auto publish = [&](auto lc, int nxt, const unsigned (&keep)[E]) __attribute__((always_inline)) {
        constexpr int l = decltype(lc)::value;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            store_split2<false>(&hA[l][nxt][lrow(i) * HP + unit], PLANE, h[l][i], h_s);
            if constexpr (l < L - 1) {
                const float factor = masked ? p.keep_scale * (float)keep[i] : 1.f;
                store_split2<false>(&midp[l % NMID][lrow(i) * HP + unit], PLANE, h[l][i] * factor, h_s);
            }
            else topf[lrow(i)][unit] = h[l][i];
        }
    };
    auto upper_layer = [&](auto lc, int cur, const unsigned (&keep)[E]) __attribute__((always_inline)) {
        constexpr int l = decltype(lc)::value;
        f32x4 a1[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};   // r, z, i_n, h_n
        product(std::integral_constant<int, 2 * l - 1>{}, &midp[(l - 1) % NMID][aoff], a1, 2);
        product(std::integral_constant<int, 2 * l>{}, &hA[l][cur][aoff], a1, 3);
        float ar[E], az[E], ai[E], ah[E];
        elems(a1[0], ar); elems(a1[1], az); elems(a1[2], ai); elems(a1[3], ah);
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const float r = fast_sigmoid(ar[i] * us[l] + br[l]);
            const float z = fast_sigmoid(az[i] * us[l] + bz[l]);
            const float n = fast_tanh(ai[i] * us[l] + bin[l] + r * (ah[i] * us[l] + bhn[l]));
            h[l][i] = (1.f - z) * n + z * h[l][i];
        }
        publish(lc, cur ^ 1, keep);
        lds_barrier();
    };

    for (int t = 0; t < ticks; ++t) {
        const int cur = t & 1;
        const int beat = t / p.tpb;
        if (t % p.tpb == 0) {                                  // the states restart at every beat
            lds_barrier();
            float mx = 1.f;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int64_t brow = (int64_t)beat * B + rows[i];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    h[l][i] = p.h0[l][brow * p.h0_stride + unit];
                    mx = fmaxf(mx, fabsf(h[l][i]));
                }
                const float *g = p.gib + brow * 3 * H + unit;
                gb[i][0] = g[0]; gb[i][1] = g[H]; gb[i][2] = g[2 * H];
            }
            mx = row16_max(mx * keep_bound);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            if (lane == 0) hmax[w] = mx;
            lds_barrier();
#pragma unroll
            for (int q = 0; q < H / 16; ++q) mx = fmaxf(mx, hmax[q]);
            const Pow2 sh = pow2_for(mx);
            h_s = sh.s;
#pragma unroll
            for (int l = 0; l < L; ++l) us[l] = sh.inv * w_inv[l];
#pragma unroll
            for (int i = 0; i < E; ++i)
#pragma unroll
                for (int l = 0; l < L; ++l) store_split2<false>(&hA[l][cur][lrow(i) * HP + unit], PLANE, h[l][i], h_s);
            lds_barrier();
        }
        // the token's projections and every boundary's keep bytes are requested here, in front of the tick's weight stream, so that
        // no weight group waits on their account: they are older than the tick's weight loads in the in-order counter.  The bytes stay
        // raw until `publish` turns them into factors -- converted here they would be waited for at once, a round trip per tick in
        // front of the first group.  No branch around the byte loads (a load under a run-time test is followed by a full drain):
        // without masks they read byte 0 of the projections and the select in `publish` drops it
        float gi[E][3];
        unsigned keep[L > 1 ? L - 1 : 1][E];
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const float *pt = p.ptab + (int64_t)tok[i] * 3 * H + unit;
            gi[i][0] = gb[i][0] + pt[0]; gi[i][1] = gb[i][1] + pt[H]; gi[i][2] = gb[i][2] + pt[2 * H];
#pragma unroll
            for (int l = 0; l < (L > 1 ? L - 1 : 1); ++l) {
                keep[l][i] = 1u;
                if constexpr (L > 1) {
                    const int64_t at = masked ? (((int64_t)l * ticks + t) * B + rows[i]) * H + unit : 0;
                    keep[l][i] = mask_bytes[at];
                }
            }
        }
        float un[E];
        if constexpr (PICK != PICK_ARGMAX) {
#pragma unroll
            for (int i = 0; i < E; ++i) un[i] = fminf(fmaxf(smp.u[(int64_t)rows[i] * ticks + t], 0.f), 1.f);
        }
        // PICK_PLANNED: the tick's plan bytes of the lane's note, one per row element, requested here at the tick's top: they do not
        // depend on the recurrence, so their latency lies under the layers' products and not in front of the logits' barrier.  Raw
        // until the logits are published (converted here they would be waited for at once)
        [[maybe_unused]] unsigned plan_b[PICK == PICK_PLANNED ? E : 1];
        if constexpr (PICK == PICK_PLANNED) {
#pragma unroll
            for (int i = 0; i < E; ++i) plan_b[i] = smp.allow[rows[i] * smp.row_stride + t * smp.tick_stride + (note_ok ? note : 0)];
        }
        // ---- layer 0: matrix 0 on its own state, the input projections from the token
        {
            f32x4 a0[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            product(std::integral_constant<int, 0>{}, &hA[0][cur][aoff], a0, 2);
            float ar[E], az[E], an[E];
            elems(a0[0], ar); elems(a0[1], az); elems(a0[2], an);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float r = fast_sigmoid(gi[i][0] + ar[i] * us[0] + br[0]);
                const float z = fast_sigmoid(gi[i][1] + az[i] * us[0] + bz[0]);
                const float n = fast_tanh(gi[i][2] + r * (an[i] * us[0] + bhn[0]));
                h[0][i] = (1.f - z) * n + z * h[0][i];
            }
            publish(std::integral_constant<int, 0>{}, cur ^ 1, keep[0]);
            lds_barrier();
        }
        // ---- upper layers: W_ih_l on the boundary below, W_hh_l on the layer's own state
        // (the top layer publishes no boundary: its keep argument is not read)
        if constexpr (L > 1) upper_layer(std::integral_constant<int, 1>{}, cur, keep[L > 2 ? 1 : 0]);
        if constexpr (L > 2) upper_layer(std::integral_constant<int, 2>{}, cur, keep[L > 3 ? 2 : 0]);
        if constexpr (L > 3) upper_layer(std::integral_constant<int, 3>{}, cur, keep[0]);
        // ---- logits (fp32 MFMA, weights in LDS) and the tiles' half of the pick on the first waves
        if (w < ntile) {
            f32x4 lg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kq = 0; kq < KQ; ++kq) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(&topf[arow][16 * kq + 4 * quad]);
                const f32x4 b = *reinterpret_cast<const f32x4 *>(&wout_s[note][16 * kq + 4 * quad]);
#pragma unroll
                for (int j = 0; j < 4; ++j) lg = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], lg, 0, 0, 0);
            }
            float v[E], lv[E];
            elems(lg, lv);
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = note_ok ? fmaxf(lv[i] + bout, 0.f) : -1.f;
            if constexpr (PICK == PICK_MULTINOMIAL) {          // the tile's maximum, e relative to it and e's prefixes per row
                float mx[E], pre[E];
#pragma unroll
                for (int i = 0; i < E; ++i) mx[i] = row16_max(v[i]);
#pragma unroll
                for (int i = 0; i < E; ++i) pre[i] = note_ok ? __expf((v[i] - mx[i]) * smp.inv_t) : 0.f;
#pragma unroll
                for (int i = 0; i < E; ++i) pre[i] = row16_prefix(pre[i]);
#pragma unroll
                for (int i = 0; i < E; ++i) smp_pre[w][lrow(i)][col] = pre[i];
                if (col == 0) {
#pragma unroll
                    for (int i = 0; i < E; ++i) smp_max[w][lrow(i)] = mx[i];
                }
            } else if constexpr (PICK == PICK_FILTERED) {      // the row's logits to LDS, banned notes as -1
#pragma unroll
                for (int i = 0; i < E; ++i) flt_lg[lrow(i) * FLT_LS + note] = note_on ? v[i] : -1.f;
            } else if constexpr (PICK == PICK_PLANNED) {       // the same, the note's flag this row's at this tick
#pragma unroll
                for (int i = 0; i < E; ++i) flt_lg[lrow(i) * FLT_LS + note] = note_ok && plan_b[i] != 0 ? v[i] : -1.f;
            } else {
                int ix[E];
#pragma unroll
                for (int i = 0; i < E; ++i) ix[i] = note;
#pragma unroll
                for (int i = 0; i < E; ++i) tick_argmax_stage<0xB1>(v[i], ix[i]);
#pragma unroll
                for (int i = 0; i < E; ++i) tick_argmax_stage<0x4E>(v[i], ix[i]);
#pragma unroll
                for (int i = 0; i < E; ++i) tick_argmax_stage<0x141>(v[i], ix[i]);
#pragma unroll
                for (int i = 0; i < E; ++i) tick_argmax_stage<0x140>(v[i], ix[i]);
                if (col == 0) {
#pragma unroll
                    for (int i = 0; i < E; ++i) { cand_v[w][lrow(i)] = v[i]; cand_i[w][lrow(i)] = ix[i]; }
                }
            }
        }
        lds_barrier();
        // ---- the rows' half of the pick, on every lane (the arithmetic of tick_free_run_h2_kernel)
        if constexpr (PICK == PICK_MULTINOMIAL) {
            int tile[E];
            float base[E], scale[E], target[E];
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int r = lrow(i);
                float m[4], sum[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool on = c < ntile;
                    m[c] = on ? smp_max[c][r] : -1.f;
                    sum[c] = on ? smp_pre[c][r][min(15, p.vocab - 1 - 16 * c)] : 0.f;
                }
                const float big = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
                float sc[4], run[5];
                run[0] = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sc[c] = __expf((m[c] - big) * smp.inv_t);
                    run[c + 1] = __builtin_fmaf(sum[c], sc[c], run[c]);
                }
                target[i] = un[i] * run[4];
                tile[i] = 0; base[i] = run[0]; scale[i] = sc[0];
#pragma unroll
                for (int c = 1; c < 4; ++c) {
                    const bool next = run[c] < target[i];
                    tile[i] = next ? c : tile[i];
                    base[i] = next ? run[c] : base[i];
                    scale[i] = next ? sc[c] : scale[i];
                }
            }
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float ck = __builtin_fmaf(smp_pre[tile[i]][lrow(i)][col], scale[i], base[i]);
                const unsigned long long reached = __ballot(ck >= target[i]);
                const int ix = min(max(16 * tile[i] + __ffs((int)((unsigned)(reached >> (16 * quad)) & 0xffffu)) - 1, 0), p.vocab - 1);
                tok[i] = ix;
                if (w == 0 && col == 0 && live[i]) p.tokens[(int64_t)rows[i] * ticks + t] = ix;
            }
        } else if constexpr (tick_row_pick<PICK>) {
            const auto cuts = tick_cuts(smp);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int ix = tick_filtered_pick(&flt_lg[lrow(i) * FLT_LS], col, quad, 16 * ntile, un[i], cuts, p.vocab);
                tok[i] = ix;
                if (w == 0 && col == 0 && live[i]) p.tokens[(int64_t)rows[i] * ticks + t] = ix;
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int r = lrow(i);
                float v = cand_v[0][r];
                int ix = cand_i[0][r];
                for (int c = 1; c < ntile; ++c) {
                    const float ov = cand_v[c][r];
                    const int oi = cand_i[c][r];
                    const bool take = ov > v;                  // later tiles hold larger indices: ties keep the earlier
                    v = take ? ov : v;
                    ix = take ? oi : ix;
                }
                tok[i] = ix;
                if (w == 0 && col == 0 && live[i]) p.tokens[(int64_t)rows[i] * ticks + t] = ix;
            }
        }
    }
}


}  // namespace arvae

using namespace arvae;

extern "C" int64_t arvae_tick_free_run_ws_floats(int32_t hidden) {
    // three matrices [3H][H] as three 16-bit terms each (tick_prep_kernel writes two of them and the scales behind)
    return arvae_gru_seq_supported(hidden) ? (int64_t)3 * 3 * hidden * hidden * 3 / 2 : 0;
}

extern "C" int arvae_tick_free_run_supported(int32_t hidden, int32_t vocab) {
    return arvae_gru_seq_supported(hidden) && vocab >= 1 && vocab <= 64 && vocab <= 16 * (hidden / 16);
}

// false (here and in tick_stack_launch): a row width gru_rows_per_wg() does not return
template <int HH, bool MM>
static bool tick_h2_launch(const TickFreeRun &p, const TickPrep &tp, float *ws, int rw, const TickSample &smp, hipStream_t st) {
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    const dim3 gr((p.batch + rw - 1) / rw);
    tick_prep_launch<HH>(tp, ws, st);
    return with_int<4, 8, 16>(rw, [&](auto RW) {
        with_bool(smp.u != nullptr, [&](auto DRAW) {
            constexpr int PICK = decltype(DRAW)::value ? PICK_MULTINOMIAL : PICK_ARGMAX;
            ARVAE_LAUNCH((tick_free_run_h2_kernel<HH, MM, decltype(RW)::value, PICK>), gr, dim3(4 * HH), 0, st, p, packed, smp);
        });
    });
}

// PICK_FILTERED: generation runs with dropout off, so only the unmasked kernels exist
template <int HH>
static bool tick_h2_launch_filtered(const TickFreeRun &p, const TickPrep &tp, float *ws, int rw, const TickFilter &flt, hipStream_t st) {
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    const dim3 gr((p.batch + rw - 1) / rw);
    tick_prep_launch<HH>(tp, ws, st);
    return with_int<4, 8, 16>(rw, [&](auto RW) {
        ARVAE_LAUNCH((tick_free_run_h2_kernel<HH, false, decltype(RW)::value, PICK_FILTERED>), gr, dim3(4 * HH), 0, st, p, packed, flt);
    });
}

// PICK_PLANNED: as PICK_FILTERED, unmasked kernels only
template <int HH>
static bool tick_h2_launch_planned(const TickFreeRun &p, const TickPrep &tp, float *ws, int rw, const TickPlan &pl, hipStream_t st) {
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    const dim3 gr((p.batch + rw - 1) / rw);
    tick_prep_launch<HH>(tp, ws, st);
    return with_int<4, 8, 16>(rw, [&](auto RW) {
        ARVAE_LAUNCH((tick_free_run_h2_kernel<HH, false, decltype(RW)::value, PICK_PLANNED>), gr, dim3(4 * HH), 0, st, p, packed, pl);
    });
}

// uniforms null: the top-1 note is fed back; else a note drawn at uniforms [batch][ticks] from softmax(logits * inv_temperature), with
// flt (its draws those of `uniforms`) over the notes the filter leaves, with pl over the notes its plan leaves per (row, tick)
static int tick_free_run_launch(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride, const float *gib,
                                const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch, int32_t beats,
                                int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms, float inv_temperature,
                                int64_t *tokens, float *ws, arvae_stream_t stream, const TickFilter *flt = nullptr,
                                const TickPlan *pl = nullptr) {
    ARVAE_REQUIRE(wts && h0_l0 && h0_l1 && gib && ptab && tokens, "tick_free_run: null pointer");
    ARVAE_REQUIRE(wts->w_hh0 && wts->b_hh0 && wts->w_ih1 && wts->b_ih1 && wts->w_hh1 && wts->b_hh1 && wts->w_out && wts->b_out,
                  "tick_free_run: null weight pointer");
    ARVAE_REQUIRE(batch >= 1 && beats >= 1 && ticks_per_beat >= 1, "tick_free_run: empty problem");
    ARVAE_REQUIRE(arvae_gru_seq_supported(hidden), "tick_free_run: hidden size %d is not built (32, 64, 128)", hidden);
    ARVAE_REQUIRE(arvae_tick_free_run_supported(hidden, vocab), "tick_free_run: vocabulary of %d notes not supported at hidden size %d",
                  vocab, hidden);
    ARVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "tick_free_run: workspace must be 16-byte aligned");
    TickFreeRun p{};
    p.w_hh0 = wts->w_hh0; p.b_hh0 = wts->b_hh0; p.w_ih1 = wts->w_ih1; p.b_ih1 = wts->b_ih1;
    p.w_hh1 = wts->w_hh1; p.b_hh1 = wts->b_hh1; p.w_out = wts->w_out; p.b_out = wts->b_out;
    p.h0_l0 = h0_l0; p.h0_l1 = h0_l1; p.h0_stride = h0_stride != 0 ? h0_stride : hidden; p.gib = gib; p.ptab = ptab; p.mask = mask; p.keep_scale = keep_scale;
    p.batch = batch; p.beats = beats; p.tpb = ticks_per_beat; p.vocab = vocab; p.tokens = tokens;
    TickPrep tp{};
    tp.w[0] = wts->w_hh0; tp.w[1] = wts->w_ih1; tp.w[2] = wts->w_hh1;
    tp.nmat = 3;
    tp.out = reinterpret_cast<uint4 *>(ws);
    hipStream_t st = as_stream(stream);
    const int rw = gru_rows_per_wg(batch, 1);
    const TickSample smp{uniforms, inv_temperature};
    bool rw_known = false;
    const bool h_known = with_int<128, 64, 32>(hidden, [&](auto HH) {
        if (pl != nullptr) rw_known = tick_h2_launch_planned<decltype(HH)::value>(p, tp, ws, rw, *pl, st);
        else if (flt != nullptr) rw_known = tick_h2_launch_filtered<decltype(HH)::value>(p, tp, ws, rw, *flt, st);
        else with_bool(mask != nullptr, [&](auto MM) { rw_known = tick_h2_launch<decltype(HH)::value, decltype(MM)::value>(p, tp, ws, rw, smp, st); });
    });
    ARVAE_REQUIRE(h_known && rw_known, "tick_free_run: no kernel for hidden size %d at %d rows per workgroup", hidden, rw);
    return check_launch("tick_free_run_h2_kernel");
}

extern "C" int arvae_tick_free_run(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride, const float *gib,
                                   const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch, int32_t beats,
                                   int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int64_t *tokens, float *ws,
                                   arvae_stream_t stream) {
    ARVAE_REQUIRE(ws != nullptr, "tick_free_run: null workspace (arvae_tick_free_run_ws_floats)");
    return tick_free_run_launch(wts, h0_l0, h0_l1, h0_stride, gib, ptab, mask, keep_scale, batch, beats, ticks_per_beat, hidden, vocab,
                                nullptr, 1.f, tokens, ws, stream);
}

extern "C" int arvae_tick_free_run_sampled(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                           const float *gib, const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch,
                                           int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms,
                                           float inv_temperature, int64_t *tokens, float *ws, arvae_stream_t stream) {
    ARVAE_REQUIRE(uniforms != nullptr, "tick_free_run_sampled: null uniforms");
    ARVAE_REQUIRE(ws != nullptr, "tick_free_run_sampled: the sampled pass needs the workspace (arvae_tick_free_run_ws_floats)");
    ARVAE_REQUIRE(std::isfinite(inv_temperature) && inv_temperature > 0.f,
                  "tick_free_run_sampled: inverse temperature %f is not a positive finite number", (double)inv_temperature);
    return tick_free_run_launch(wts, h0_l0, h0_l1, h0_stride, gib, ptab, mask, keep_scale, batch, beats, ticks_per_beat, hidden, vocab,
                                uniforms, inv_temperature, tokens, ws, stream);
}

extern "C" int arvae_tick_free_run_filtered(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                            const float *gib, const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch,
                                            int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms,
                                            float inv_temperature, const arvae_sample_filter_t *filter, int64_t *tokens, float *ws,
                                            arvae_stream_t stream) {
    int top_k = 0;
    bool active = false;
    if (const int rc = sample_filter_check("tick_free_run_filtered", filter, vocab, &top_k, &active)) return rc;
    ARVAE_REQUIRE(uniforms != nullptr, "tick_free_run_filtered: null uniforms");
    ARVAE_REQUIRE(mask == nullptr, "tick_free_run_filtered: a dropout keep-mask was given (generation runs with dropout off: the filtered "
                                   "kernels are built without masks)");
    if (!active)
        return arvae_tick_free_run_sampled(wts, h0_l0, h0_l1, h0_stride, gib, ptab, nullptr, keep_scale, batch, beats, ticks_per_beat, hidden,
                                           vocab, uniforms, inv_temperature, tokens, ws, stream);
    ARVAE_REQUIRE(ws != nullptr, "tick_free_run_filtered: null workspace (arvae_tick_free_run_ws_floats)");
    ARVAE_REQUIRE(std::isfinite(inv_temperature) && inv_temperature > 0.f,
                  "tick_free_run_filtered: inverse temperature %f is not a positive finite number", (double)inv_temperature);
    const TickFilter flt{uniforms, inv_temperature, top_k, filter->top_p, filter->allow};
    return tick_free_run_launch(wts, h0_l0, h0_l1, h0_stride, gib, ptab, nullptr, keep_scale, batch, beats, ticks_per_beat, hidden, vocab,
                                uniforms, inv_temperature, tokens, ws, stream, &flt);
}

// what the two planned free runs check beyond the filtered ones, and their kernel argument: the plan, no mask inside the filter
static int tick_plan_arg(const char *who, const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan, const uint8_t *mask,
                         const float *uniforms, float inv_temperature, int32_t beats, int32_t ticks_per_beat, int32_t vocab, TickPlan *out) {
    int top_k = 0;
    bool active = false;
    if (const int rc = sample_filter_check(who, filter, vocab, &top_k, &active)) return rc;
    ARVAE_REQUIRE(filter->allow == nullptr, "%s: filter->allow is set (with a plan the allowed mask is folded into the plan)", who);
    ARVAE_REQUIRE(beats >= 1 && ticks_per_beat >= 1, "%s: empty problem", who);
    if (const int rc = note_plan_check(who, plan, (int64_t)beats * ticks_per_beat, vocab)) return rc;
    ARVAE_REQUIRE(uniforms != nullptr, "%s: null uniforms", who);
    ARVAE_REQUIRE(mask == nullptr, "%s: a dropout keep-mask was given together with a plan (generation runs with dropout off: the planned "
                                   "kernels are built without masks)", who);
    ARVAE_REQUIRE(std::isfinite(inv_temperature) && inv_temperature > 0.f, "%s: inverse temperature %f is not a positive finite number", who,
                  (double)inv_temperature);
    *out = TickPlan{uniforms, inv_temperature, top_k, filter->top_p, plan->allow, plan->row_stride, plan->tick_stride};
    return ARVAE_OK;
}

extern "C" int arvae_tick_free_run_planned(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                           const float *gib, const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch,
                                           int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms,
                                           float inv_temperature, const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan,
                                           int64_t *tokens, float *ws, arvae_stream_t stream) {
    TickPlan pl{};
    if (const int rc = tick_plan_arg("tick_free_run_planned", filter, plan, mask, uniforms, inv_temperature, beats, ticks_per_beat, vocab, &pl))
        return rc;
    ARVAE_REQUIRE(ws != nullptr, "tick_free_run_planned: null workspace (arvae_tick_free_run_ws_floats)");
    return tick_free_run_launch(wts, h0_l0, h0_l1, h0_stride, gib, ptab, nullptr, keep_scale, batch, beats, ticks_per_beat, hidden, vocab,
                                uniforms, inv_temperature, tokens, ws, stream, nullptr, &pl);
}

// ---- layer counts other than two (tick_free_run_layers_kernel) ----------------------------------------------------
static int tick_stack_matrices(int layers) { return 2 * layers - 1; }

extern "C" int arvae_tick_free_run_layers_supported(int32_t hidden, int32_t vocab, int32_t layers) {
    // hidden 128 with three or four layers is NOT offered: those instantiations fed back wrong notes in a few per cent of the rows,
    // differently from run to run, and the cause is not found: such stacks go tick by tick
    if (hidden == 128 && layers >= 3) return 0;
    return arvae_tick_free_run_supported(hidden, vocab) && (layers == 1 || layers == 3 || layers == 4);
}

extern "C" int64_t arvae_tick_free_run_layers_ws_floats(int32_t hidden, int32_t layers) {
    // 2L - 1 matrices [3H][H] as two 16-bit terms each, and their maxima behind (padded to a 16-byte multiple)
    if (!arvae_gru_seq_supported(hidden) || layers < 1 || layers > TICK_MAX_LAYERS) return 0;
    return (int64_t)tick_stack_matrices(layers) * 3 * hidden * hidden + 8;
}

template <int HH, int LL>
static bool tick_stack_launch(const TickStack &p, const TickPrep &tp, float *ws, int rw, const TickSample &smp, hipStream_t st) {
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    const dim3 gr((p.batch + rw - 1) / rw);
    tick_prep_launch<HH>(tp, ws, st);
    return with_int<4, 8, 16>(rw, [&](auto RW) {
        with_bool(smp.u != nullptr, [&](auto DRAW) {
            constexpr int PICK = decltype(DRAW)::value ? PICK_MULTINOMIAL : PICK_ARGMAX;
            ARVAE_LAUNCH((tick_free_run_layers_kernel<HH, LL, decltype(RW)::value, PICK>), gr, dim3(4 * HH), 0, st, p, packed, smp);
        });
    });
}

template <int HH, int LL>
static bool tick_stack_launch_filtered(const TickStack &p, const TickPrep &tp, float *ws, int rw, const TickFilter &flt, hipStream_t st) {
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    const dim3 gr((p.batch + rw - 1) / rw);
    tick_prep_launch<HH>(tp, ws, st);
    return with_int<4, 8, 16>(rw, [&](auto RW) {
        ARVAE_LAUNCH((tick_free_run_layers_kernel<HH, LL, decltype(RW)::value, PICK_FILTERED>), gr, dim3(4 * HH), 0, st, p, packed, flt);
    });
}

template <int HH, int LL>
static bool tick_stack_launch_planned(const TickStack &p, const TickPrep &tp, float *ws, int rw, const TickPlan &pl, hipStream_t st) {
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    const dim3 gr((p.batch + rw - 1) / rw);
    tick_prep_launch<HH>(tp, ws, st);
    return with_int<4, 8, 16>(rw, [&](auto RW) {
        ARVAE_LAUNCH((tick_free_run_layers_kernel<HH, LL, decltype(RW)::value, PICK_PLANNED>), gr, dim3(4 * HH), 0, st, p, packed, pl);
    });
}

// pl: PICK_PLANNED; flt: PICK_FILTERED over its cuts (its draws those of `uniforms`), else the pick `uniforms` selects
static int tick_layers_launch(const arvae_tick_stack_t *stack, const float *gib, const float *ptab, const uint8_t *mask, float keep_scale,
                              int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms,
                              float inv_temperature, int64_t *tokens, float *ws, arvae_stream_t stream, const TickFilter *flt,
                              const TickPlan *pl = nullptr) {
    ARVAE_REQUIRE(stack && gib && ptab && tokens, "tick_free_run_layers: null pointer");
    ARVAE_REQUIRE(ws != nullptr, "tick_free_run_layers: null workspace (arvae_tick_free_run_layers_ws_floats)");
    const int layers = stack->layers;
    ARVAE_REQUIRE(layers >= 1 && layers <= ARVAE_TICK_MAX_LAYERS, "tick_free_run_layers: %d layers (1 .. %d)", layers, ARVAE_TICK_MAX_LAYERS);
    ARVAE_REQUIRE(batch >= 1 && beats >= 1 && ticks_per_beat >= 1, "tick_free_run_layers: empty problem");
    ARVAE_REQUIRE(arvae_gru_seq_supported(hidden), "tick_free_run_layers: hidden size %d is not built (32, 64, 128)", hidden);
    ARVAE_REQUIRE(arvae_tick_free_run_supported(hidden, vocab), "tick_free_run_layers: vocabulary of %d notes not supported at hidden size %d",
                  vocab, hidden);
    ARVAE_REQUIRE(arvae_tick_free_run_layers_supported(hidden, vocab, layers),
                  "tick_free_run_layers: %d layers at hidden size %d are not offered (1, 3, 4 layers, three and four up to hidden 64; "
                  "two layers: arvae_tick_free_run)", layers, hidden);
    ARVAE_REQUIRE(stack->w_out && stack->b_out, "tick_free_run_layers: null weight pointer");
    for (int l = 0; l < layers; ++l) {
        ARVAE_REQUIRE(stack->w_hh[l] && stack->b_hh[l] && stack->h0[l], "tick_free_run_layers: null pointer in layer %d", l);
        ARVAE_REQUIRE(l == 0 || (stack->w_ih[l] && stack->b_ih[l]), "tick_free_run_layers: null input weights in layer %d", l);
    }
    ARVAE_REQUIRE(stack->h0_stride == 0 || stack->h0_stride >= hidden, "tick_free_run_layers: h0_stride %lld is below the hidden size %d",
                  (long long)stack->h0_stride, hidden);
    ARVAE_REQUIRE(mask == nullptr || layers == 1 || (std::isfinite(keep_scale) && keep_scale >= 0.f),
                  "tick_free_run_layers: keep scale %f is not a finite non-negative number", (double)keep_scale);
    ARVAE_REQUIRE(uniforms == nullptr || (std::isfinite(inv_temperature) && inv_temperature > 0.f),
                  "tick_free_run_layers: inverse temperature %f is not a positive finite number", (double)inv_temperature);
    ARVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "tick_free_run_layers: workspace must be 16-byte aligned");
    TickStack p{};
    TickPrep tp{};
    tp.nmat = tick_stack_matrices(layers);
    tp.out = reinterpret_cast<uint4 *>(ws);
    for (int l = 0; l < layers; ++l) {
        p.b_ih[l] = stack->b_ih[l]; p.b_hh[l] = stack->b_hh[l]; p.h0[l] = stack->h0[l];
        tp.w[2 * l] = stack->w_hh[l];
        if (l > 0) tp.w[2 * l - 1] = stack->w_ih[l];
    }
    p.w_out = stack->w_out; p.b_out = stack->b_out;
    p.h0_stride = stack->h0_stride != 0 ? stack->h0_stride : hidden;
    p.gib = gib; p.ptab = ptab; p.mask = layers > 1 ? mask : nullptr; p.keep_scale = keep_scale;
    p.batch = batch; p.beats = beats; p.tpb = ticks_per_beat; p.vocab = vocab; p.tokens = tokens;
    hipStream_t st = as_stream(stream);
    const int rw = gru_rows_per_wg(batch, 1);
    const TickSample smp{uniforms, uniforms != nullptr ? inv_temperature : 1.f};
    bool launched = false;
    with_int<1, 3, 4>(layers, [&](auto LL) {
        with_int<128, 64, 32>(hidden, [&](auto HH) {
            constexpr int H = decltype(HH)::value, L = decltype(LL)::value;
            // (hidden 128 with three or four layers is not built: arvae_tick_free_run_layers_supported)
            if constexpr (H != 128 || L == 1)
                launched = pl != nullptr    ? tick_stack_launch_planned<H, L>(p, tp, ws, rw, *pl, st)
                           : flt != nullptr ? tick_stack_launch_filtered<H, L>(p, tp, ws, rw, *flt, st)
                                            : tick_stack_launch<H, L>(p, tp, ws, rw, smp, st);
        });
    });
    ARVAE_REQUIRE(launched, "tick_free_run_layers: no kernel for %d layers of hidden size %d at %d rows per workgroup", layers, hidden, rw);
    return check_launch("tick_free_run_layers_kernel");
}

extern "C" int arvae_tick_free_run_layers(const arvae_tick_stack_t *stack, const float *gib, const float *ptab, const uint8_t *mask,
                                          float keep_scale, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden,
                                          int32_t vocab, const float *uniforms, float inv_temperature, int64_t *tokens, float *ws,
                                          arvae_stream_t stream) {
    return tick_layers_launch(stack, gib, ptab, mask, keep_scale, batch, beats, ticks_per_beat, hidden, vocab, uniforms, inv_temperature,
                              tokens, ws, stream, nullptr);
}

extern "C" int arvae_tick_free_run_layers_filtered(const arvae_tick_stack_t *stack, const float *gib, const float *ptab, const uint8_t *mask,
                                                   float keep_scale, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden,
                                                   int32_t vocab, const float *uniforms, float inv_temperature,
                                                   const arvae_sample_filter_t *filter, int64_t *tokens, float *ws, arvae_stream_t stream) {
    int top_k = 0;
    bool active = false;
    if (const int rc = sample_filter_check("tick_free_run_layers_filtered", filter, vocab, &top_k, &active)) return rc;
    ARVAE_REQUIRE(uniforms != nullptr, "tick_free_run_layers_filtered: null uniforms");
    ARVAE_REQUIRE(mask == nullptr, "tick_free_run_layers_filtered: dropout keep-masks were given (generation runs with dropout off: the "
                                   "filtered kernels are built without masks)");
    const TickFilter flt{uniforms, inv_temperature, top_k, filter->top_p, filter->allow};
    return tick_layers_launch(stack, gib, ptab, nullptr, keep_scale, batch, beats, ticks_per_beat, hidden, vocab, uniforms, inv_temperature,
                              tokens, ws, stream, active ? &flt : nullptr);
}

extern "C" int arvae_tick_free_run_layers_planned(const arvae_tick_stack_t *stack, const float *gib, const float *ptab, const uint8_t *mask,
                                                  float keep_scale, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden,
                                                  int32_t vocab, const float *uniforms, float inv_temperature,
                                                  const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan, int64_t *tokens,
                                                  float *ws, arvae_stream_t stream) {
    TickPlan pl{};
    if (const int rc = tick_plan_arg("tick_free_run_layers_planned", filter, plan, mask, uniforms, inv_temperature, beats, ticks_per_beat,
                                     vocab, &pl))
        return rc;
    return tick_layers_launch(stack, gib, ptab, nullptr, keep_scale, batch, beats, ticks_per_beat, hidden, vocab, uniforms, inv_temperature,
                              tokens, ws, stream, nullptr, &pl);
}
