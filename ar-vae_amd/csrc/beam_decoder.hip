// Beam search of the MeasureVAE tick decoder (generation; beyond the reference): the W most likely measures of a latent code instead
// of the locally most likely note, and the log-probability of a given measure.  The semantics: include/arvae_hip.h, "Beam search".
//
//   tick_beam_search_kernel   the whole search in ONE launch for the reference's two-layer tick RNN: tick_free_run_h2_kernel's
//                             recurrence (tick_decoder.hip) over the W beams of every code as adjacent rows of a workgroup's tile, and
//                             between a tick's logits and the next tick's input projection the selection and the row permutation;
//   beam_select_kernel        the selection alone on given logits, any vocabulary: the tick-by-tick path (ARVAE_TICK_STEPWISE=1, other
//                             layer counts and hidden sizes, more than 64 notes), the on-device yardstick of the one-launch kernel,
//                             and through beam_select_launch (beam_select.h) every tick of beam_wide.hip's search at 256 / 512;
//   sequence_log_prob_kernel  sum over t of the masked log-softmax of given logits at given tokens.
// All three also serve a note plan (include/arvae_hip.h, "Note plans": the allowed notes per (code, tick)); the one-launch kernel has an
// instantiation of its own for it, in which a code may hold fewer than W finite hypotheses (dead slots).  The one-launch kernel and
// beam_select_kernel also serve the beams in groups (include/arvae_hip.h, "Diverse beam search"): a further instantiation on the
// planned form, and a group loop in the row kernel.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include "diag.h"
#include "common.h"
#include "dispatch.h"
#include "splitmath.h"
#include "gru_common.h"
#include "tick_common.h"
#include "beam_select.h"

namespace arvae {

typedef int beam_i32x4 __attribute__((ext_vector_type(4)));
constexpr int BEAM_MAX_TICKS = 32;                             // the one-launch kernel keeps a measure's history in LDS

// the order of the candidates (score c, beam k, note v): c descending as floats, ties to the lower k, then the lower v as integers
__device__ __forceinline__ bool beam_before(float ca, int ka, int va, float cb, int kb, int vb) {
    return ca > cb || (ca == cb && (ka < kb || (ka == kb && va < vb)));
}

// the key of the diverse search, c - penalty * float(n): the product and the difference each rounded.  Contraction is off inside this
// function alone (the compiler would otherwise fuse the two into fma(-penalty, n, c)); everything around it keeps the file's default
__device__ __forceinline__ float beam_penalised(float c, float penalty, int n) {
#pragma clang fp contract(off)
    const float pay = penalty * (float)n;
    return c - pay;
}

// ------------------------------------------------------------------------------------------------------------------
// One wave per code.  Per live beam k: M_k = the allowed maximum, S_k = the sum of exp(l - M_k) over the allowed notes (every lane its
// notes in index order, then the xor butterfly: both lanes of a pair add the same two values, so every lane holds the same bits), lane
// k keeps (M_k, log S_k, score_k).  Then W rounds: every lane takes the first of its candidates that is ordered behind the previous
// round's pick, the butterfly the first among the lanes.  No allowed candidate left (arvae_beam_select rules it out; under a note plan
// a forced tick or dead beams bring it about): a dead slot -- the group's first beam, the code's first allowed note (note 0 without
// one), -inf.
// allow_stride: bytes between the codes' masks (a note plan's tick; 0: one mask for every code).
// groups G (include/arvae_hip.h, "Diverse beam search"): the groups of width / G beams are served one after the other, each over its
// own beams (`live`: the live ones of EVERY group, its first) with the rounds above; a candidate's key is c - penalty * n_v, n_v the
// number of finite picks with note v that the earlier groups of this call made (their notes in LDS, at most 15).  G = 1: no pick is
// ever counted and the key is c.  logp_in / logp_out (both or neither): the beams' unpenalised sums, carried beside the scores.
__global__ __launch_bounds__(64) void beam_select_kernel(const float *__restrict__ logits, const float *__restrict__ scores_in, int width,
                                                         int vocab, int live, const uint8_t *__restrict__ allow_all, int64_t allow_stride,
                                                         int *__restrict__ parents, int64_t *__restrict__ notes,
                                                         float *__restrict__ scores_out, int groups, float penalty,
                                                         const float *__restrict__ logp_in, float *__restrict__ logp_out) {
    __shared__ int pick_note[BEAM_MAX_WIDTH];
    const int code = blockIdx.x, lane = threadIdx.x;
    const int gw = width / groups;
    const float *base = logits + (int64_t)code * width * vocab;
    const uint8_t *allow = allow_all != nullptr ? allow_all + code * allow_stride : nullptr;
    auto on = [&](int v) { return allow == nullptr || allow[v] != 0; };
    int first_on = vocab;
    for (int v = lane; v < vocab; v += 64)
        if (on(v)) { first_on = v; break; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first_on = min(first_on, __shfl_xor(first_on, off, 64));
    first_on = first_on < vocab ? first_on : 0;
    float my_m = 0.f, my_ls = 0.f, my_sc = -INFINITY, my_lp = -INFINITY;
    for (int k = 0; k < width; ++k) {
        if (k % gw >= live) continue;
        const float *row = base + (int64_t)k * vocab;
        float m = -INFINITY;
        for (int v = lane; v < vocab; v += 64)
            if (on(v)) m = fmaxf(m, row[v]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        float s = 0.f;
        for (int v = lane; v < vocab; v += 64)
            if (on(v)) s += expf(row[v] - m);
        s = wave_sum(s);
        if (lane == k) {
            my_m = m; my_ls = logf(s); my_sc = scores_in[(int64_t)code * width + k];
            if (logp_in != nullptr) my_lp = logp_in[(int64_t)code * width + k];
        }
    }
    int seen = 0, made = 0;                                    // the picks the current group counts / those made so far (wave-uniform)
    for (int g = 0; g < groups; ++g) {
        const int k0 = g * gw;
        float pc = INFINITY;
        int pk = -1, pv = -1;
        for (int j = 0; j < gw; ++j) {
            float bc = -INFINITY;
            int bk = 0, bv = 0;
            bool found = false;
            for (int k = k0; k < k0 + live; ++k) {
                const float m = __shfl(my_m, k, 64), ls = __shfl(my_ls, k, 64), sc = __shfl(my_sc, k, 64);
                const float *row = base + (int64_t)k * vocab;
                for (int v = lane; v < vocab; v += 64) {
                    if (!on(v)) continue;
                    float c = sc + ((row[v] - m) - ls);
                    if (seen > 0) {
                        int n = 0;
                        for (int q = 0; q < seen; ++q) n += pick_note[q] == v ? 1 : 0;
                        c = beam_penalised(c, penalty, n);
                    }
                    if (!beam_before(pc, pk, pv, c, k, v)) continue;       // taken in an earlier round (or not a number)
                    if (!found || beam_before(c, k, v, bc, bk, bv)) { bc = c; bk = k; bv = v; found = true; }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float oc = __shfl_xor(bc, off, 64);
                const int ok = __shfl_xor(bk, off, 64), ov = __shfl_xor(bv, off, 64);
                const bool of = __shfl_xor((int)found, off, 64) != 0;
                const bool take = of && (!found || beam_before(oc, ok, ov, bc, bk, bv));
                bc = take ? oc : bc; bk = take ? ok : bk; bv = take ? ov : bv;
                found = found || of;
            }
            if (!found) { bc = -INFINITY; bk = k0; bv = first_on; }
            float lp = -INFINITY;
            if (logp_out != nullptr) {
                const float m = __shfl(my_m, bk, 64), ls = __shfl(my_ls, bk, 64), plp = __shfl(my_lp, bk, 64);
                if (found) lp = plp + ((base[(int64_t)bk * vocab + bv] - m) - ls);
            }
            if (lane == 0) {
                parents[(int64_t)code * width + k0 + j] = bk;
                notes[(int64_t)code * width + k0 + j] = bv;
                scores_out[(int64_t)code * width + k0 + j] = bc;
                if (logp_out != nullptr) logp_out[(int64_t)code * width + k0 + j] = lp;
                if (groups > 1 && bc > -INFINITY && made < BEAM_MAX_WIDTH) pick_note[made] = bv;
            }
            made += groups > 1 && bc > -INFINITY ? 1 : 0;
            pc = bc; pk = bk; pv = bv;
        }
        if (groups > 1) {
            __syncthreads();                                   // (one wave: the picks' notes are in LDS before the next group counts them)
            seen = made;
        }
    }
}

void beam_select_launch(const float *logits, const float *scores_in, int codes, int width, int vocab, int live, const uint8_t *allow,
                        int64_t allow_stride, int *parents, int64_t *notes, float *scores_out, int groups, float penalty,
                        const float *logp_in, float *logp_out, hipStream_t stream) {
    ARVAE_LAUNCH(beam_select_kernel, dim3(codes), dim3(64), 0, stream, logits, scores_in, width, vocab, live, allow, allow_stride, parents,
                 notes, scores_out, groups, penalty, logp_in, logp_out);
}

// One wave per row r: lane t (and t + 64, ...) takes tick t's masked log-softmax at the token -- the allowed maximum, the sum of
// exp(l - M) over the allowed notes in index order with a compensated (Kahan) running sum, (l_tok - M) - log S -- and adds its ticks in
// order; the butterfly adds the lanes.  A token outside the vocabulary or not allowed: -inf.
__global__ __launch_bounds__(64) void sequence_log_prob_kernel(const float *__restrict__ w, const int64_t *__restrict__ tokens, int steps,
                                                               int vocab, const uint8_t *__restrict__ allow_all, int64_t row_stride,
                                                               int64_t tick_stride, float *__restrict__ out) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, lane = threadIdx.x;
    float acc = 0.f;
    for (int t = lane; t < steps; t += 64) {
        // (a note plan: the mask of this row at this tick; the strides are 0 for the one mask of arvae_sequence_log_prob)
        const uint8_t *allow = allow_all != nullptr ? allow_all + r * row_stride + t * tick_stride : nullptr;
        auto on = [&](int v) { return allow == nullptr || allow[v] != 0; };
        const float *row = w + ((int64_t)r * steps + t) * vocab;
        const int64_t tok = tokens[(int64_t)r * steps + t];
        float lp = -INFINITY;
        if (tok >= 0 && tok < vocab && on((int)tok)) {
            float m = -INFINITY;
            for (int v = 0; v < vocab; ++v)
                if (on(v)) m = fmaxf(m, row[v]);
            float s = 0.f, comp = 0.f;
            for (int v = 0; v < vocab; ++v) {
                if (!on(v)) continue;
                const float y = expf(row[v] - m) - comp;
                const float sum = s + y;
                comp = (sum - s) - y;
                s = sum;
            }
            lp = (row[tok] - m) - logf(s);
        }
        acc += lp;
    }
    acc = wave_sum(acc);
    if (lane == 0) out[r] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
struct TickBeam {
    const float *w_hh0, *b_hh0, *w_ih1, *b_ih1, *w_hh1, *b_hh1, *w_out, *b_out;
    const float *h0_l0, *h0_l1;    // [beats*B] rows of H values h0_stride floats apart, row = beat*B + code
    int64_t h0_stride;
    const float *gib;              // [beats*B][3H]
    const float *ptab;             // [V+1][3H]; row V = the start token
    const uint8_t *allow;          // [V] or null
    int batch, beats, tpb, vocab, width, wshift;               // wshift: log2 of the padded width WP (the rows a code takes in a tile)
    int *parents;                  // [B][ticks][W]
    int64_t *tokens;               // [B][ticks][W]
    float *scores_hist;            // [B][ticks][W]
    int64_t *sequences;            // [B][W][ticks]
    float *scores;                 // [B][W]
};

// TickBeam with a note plan (arvae_note_plan_t) in place of `allow`: the allowed notes of code b at tick t are plan[b * row_stride +
// t * tick_stride + v] != 0.  A type of its own, so that the unplanned kernel's arguments stay what they were.
struct TickBeamPlanned : TickBeam {
    const uint8_t *plan;
    int64_t row_stride, tick_stride;
};

// TickBeamPlanned served in `groups` groups of `gwidth` = width / groups beams (include/arvae_hip.h, "Diverse beam search").  Again a
// type of its own: the two searches above keep their arguments and their code.
struct TickBeamGroups : TickBeamPlanned {
    int groups, gwidth;
    float penalty;
    float *log_probs;              // [B][W]
};

// The recurrence is tick_free_run_h2_kernel's (the same operands, products and gates in the same order: width 1 feeds back the argmax
// run's notes), over tile rows r = (code, beam k): code = r >> wshift of the workgroup's RW >> wshift codes, k = r & (WP - 1); beams
// k >= W of a padded width are dead (score -inf, never a parent).  What differs:
//   * layer 0's product W_hh0 h0 runs at every tick's top, not under the previous tick's pick: it has to wait for the permutation;
//   * layer 0's new state also goes to LDS as floats (h0f, as h1f), the logits of a row to `lgs` (banned notes and notes past the
//     vocabulary -1, below every relu output);
//   * behind the logits' barrier the selection in two stages, a barrier between them.  Stage 1, spread over the waves by (row, logits
//     tile): a row's candidates c_v = score + ((l_v - M) - log S) (expf / logf; M, S over the allowed notes, row16_sum: the same bits in
//     every lane) to `cnd`, each note's rank inside its row by beam_before (one walk, as tick_filtered_pick), the row's first W to
//     `top`.  Stage 2, spread over all lanes: a code's first W are among its W rows' first W each, so every (row, slot) entry counts
//     the entries of its code ordered before it, and the entry of rank j < W is new beam j: parent, note and score to LDS and to the
//     history;
//   * behind the next barrier every lane takes its rows' parents' states from h0f / h1f and rebuilds the split images.
// After the last tick one lane per beam walks the history in LDS backwards and writes the sequence.
//
// P = TickBeamPlanned (PLAN): a lane reads its note's plan byte of its rows' codes at every tick's top (under the layers' products),
// and the selection holds with FEWER than W allowed notes in a row and fewer than W finite candidates in a code:
//   * stage 1 marks the notes outside A(b, t) (and past the vocabulary) in `cnd` as NaN, which no comparison orders before anything:
//     an allowed note's rank counts allowed notes only.  The marked notes take the slots behind the row's allowed ones as FILLERS
//     (-inf, the row's first allowed note), so that every row still writes all its W slots at every tick and nothing stale is read;
//   * stage 2 orders the entries by (c, k, slot) -- inside a row the slots ARE the (c, v) order, so for finite entries this is
//     (c, k, v) -- which keeps equal fillers apart, and counts the slots below W only: the W * W entries of a code then have
//     distinct ranks and the ranks 0 .. W - 1 are each written once.  Entries of -inf are DEAD beams: behind every finite one, their
//     notes inside A(b, t), their score -inf for good (-inf + logp).
//
// P = TickBeamGroups (GROUPS, on the planned form): the two stages run once per group g, a barrier between the groups.  In group g's
// turn the "code" of both stages is the pair (code, g): the rows k in [g W', (g + 1) W') of the code, W' = gwidth slots a row, W' new
// beams at the rows g W' + rank.
//   * `cnt` [codes of the tile][64] counts, per note, the finite picks the earlier groups made at this tick: zeroed at the tick's
//     top, raised by stage 2 (an LDS add per finite pick).  Stage 1's key is a = c - penalty * float(cnt[v]) (the product rounded on
//     its own), and it is what the ranks, `top` and the new score take; group 0 reads zeros, so a = c exactly.
//   * stage 1 forms the candidates of every row in every turn (a row outside group g writes `cnd` only, bits nobody reads: its own
//     turn writes them again) but walks and writes `top` for the rows of group g alone; a wave none of whose rows is in group g skips
//     the unit.  (Keeping a row's M and log S from turn 0 in LDS for the later turns was measured and bought nothing: DESIGN.md
//     item 61.)  The last turn's picks raise no count: nobody reads it.
//   * a second float per row, `logp_s` (the unpenalised sum), is carried like `score_s`: stage 1 puts logp_s[k] + logp_v beside the
//     key (`top_l`), stage 2 hands the winner's to its new row.  Rows of group g are written in turn g only, after stage 1 of that
//     turn has read them.
template <int H, int RW, class P>
__global__ __launch_bounds__(H * 4) void tick_beam_search_kernel(P p, const uint4 *__restrict__ packed) {
    static_assert(RW == 16 || RW == 8 || RW == 4, "16, 8 or 4 rows: four, two or one per lane");
    constexpr bool PLAN = std::is_base_of<TickBeamPlanned, P>::value;
    constexpr bool GROUPS = std::is_same<P, TickBeamGroups>::value;
    constexpr int E = RW / 4;
    constexpr int NW = H / 16, KS = H / 32, KQ = H / 16;
    constexpr int NGG = 9 * KS;
    constexpr int RS = NGG % 6 == 0 ? 6 : 3;
    constexpr int PFD = RS - 1;
    constexpr int HP = H + 8, PLANE = 16 * HP, HS = H + 4;
    __shared__ __attribute__((aligned(16))) unsigned short hA0[2][2 * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short hA1[2][2 * PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short midp[2 * PLANE];
    __shared__ __attribute__((aligned(16))) float h0f[16][HS];
    __shared__ __attribute__((aligned(16))) float h1f[16][HS];
    __shared__ __attribute__((aligned(16))) float wout_s[64][HS];
    __shared__ __attribute__((aligned(16))) float lgs[16 * FLT_LS];
    __shared__ __attribute__((aligned(16))) float cnd[16 * FLT_LS];
    __shared__ __attribute__((aligned(16))) float top_c[16][BEAM_MAX_WIDTH];
    __shared__ __attribute__((aligned(16))) int top_v[16][BEAM_MAX_WIDTH];
    __shared__ float score_s[16];
    __shared__ int sel_par[16], sel_note[16];
    __shared__ unsigned char hist_p[BEAM_MAX_TICKS][16], hist_v[BEAM_MAX_TICKS][16];
    __shared__ float hmax[H / 16];
    // GROUPS only (the other instantiations never name them, so they take no LDS there)
    __shared__ __attribute__((aligned(16))) float top_l[16][BEAM_MAX_WIDTH];
    __shared__ float logp_s[16];
    __shared__ int cnt[16][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15, quad = lane >> 4;
    const int unit = 16 * w + col;
    const int B = p.batch, W = p.width, wsh = p.wshift, WP = 1 << wsh;
    const int code0 = blockIdx.x * (RW >> wsh);
    const int ntile = (p.vocab + 15) / 16;
    int WS = W, NG = 1;                                        // the slots a row fills and the new beams of a stage-2 "code"; the turns
    [[maybe_unused]] float lam = 0.f;
    if constexpr (GROUPS) { WS = p.gwidth; NG = p.groups; lam = p.penalty; }

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(packed), 0, 3 * KS * NW * 6 * 64 * 16, 0x00020000);
    const int wlane = (w * 6 * 64 + lane) * 16;
    f16x8 wb[RS][2];
    auto fetch = [&](int gg) {
        const int g = gg / 3, gate = gg % 3;
#pragma unroll
        for (int term = 0; term < 2; ++term)
            wb[gg % RS][term] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wlane, (g * NW * 6 + gate * 2 + term) * 64 * 16, 0));
    };
#pragma unroll
    for (int d = 0; d < PFD; ++d) fetch(d % NGG);

    for (int e = threadIdx.x; e < 64 * H; e += H * 4) {
        const int n = e / H, k = e - n * H;
        wout_s[n][k] = n < p.vocab ? p.w_out[(int64_t)n * H + k] : 0.f;
    }
    for (int e = threadIdx.x; e < 16 * FLT_LS; e += H * 4) { lgs[e] = -1.f; cnd[e] = -INFINITY; }
    for (int e = threadIdx.x; e < 16 * BEAM_MAX_WIDTH; e += H * 4) { (&top_c[0][0])[e] = -INFINITY; (&top_v[0][0])[e] = 0; }
    if (threadIdx.x < 16) {
        const int k = threadIdx.x & (WP - 1);
        if constexpr (GROUPS) {                                // tick 0: the first beam of every group is live
            const bool head = k < W && k % WS == 0;
            score_s[threadIdx.x] = head ? 0.f : -INFINITY;
            logp_s[threadIdx.x] = head ? 0.f : -INFINITY;
        } else {
            score_s[threadIdx.x] = k == 0 ? 0.f : -INFINITY;   // tick 0: one live beam
        }
        sel_par[threadIdx.x] = k;                              // (dead beams keep themselves and note 0)
        sel_note[threadIdx.x] = 0;
    }
    if constexpr (GROUPS)
        for (int e = threadIdx.x; e < 16 * BEAM_MAX_WIDTH; e += H * 4) (&top_l[0][0])[e] = -INFINITY;
    const float b0r = p.b_hh0[unit], b0z = p.b_hh0[H + unit], b0n = p.b_hh0[2 * H + unit];
    const float b1r = p.b_ih1[unit] + p.b_hh1[unit], b1z = p.b_ih1[H + unit] + p.b_hh1[H + unit];
    const float b1in = p.b_ih1[2 * H + unit], b1hn = p.b_hh1[2 * H + unit];
    const int note = 16 * w + col;
    const bool note_ok = w < ntile && note < p.vocab;
    const float bout = note_ok ? p.b_out[note] : 0.f;
    bool note_on = note_ok;
    if constexpr (!PLAN) note_on = note_ok && (p.allow == nullptr || p.allow[note] != 0);

    auto lrow = [&](int i) { return gru_lrow<E>(quad, i); };
    int rows[E];                                               // the code whose inputs the lane's element i reads
#pragma unroll
    for (int i = 0; i < E; ++i) rows[i] = min(code0 + (lrow(i) >> wsh), B - 1);
    float h0[E], h1[E], gb[E][3];
    int tok[E];
#pragma unroll
    for (int i = 0; i < E; ++i) tok[i] = p.vocab;
    const int ticks = p.beats * p.tpb;
    const float *wmax = reinterpret_cast<const float *>(packed) + 9 * H * H;
    const float w0_inv = tick_scale(wmax, 0).inv, w12_inv = tick_scale(wmax, 1).inv;
    float h_s = 1.f, us0 = 1.f, us12 = 1.f;
    const int arow = gru_arow<E>(col);
    const int aoff = arow * HP + 8 * quad;
    auto elems = [&](const f32x4 &acc, float (&out)[E]) __attribute__((always_inline)) { gru_elems<E>(acc, out); };
    for (int t = 0; t < ticks; ++t) {
        const int cur = t & 1;
        const int beat = t / p.tpb;
        if (t % p.tpb == 0) {
            lds_barrier();
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int64_t br = (int64_t)beat * B + rows[i];
                h0[i] = p.h0_l0[br * p.h0_stride + unit];
                h1[i] = p.h0_l1[br * p.h0_stride + unit];
                const float *g = p.gib + br * 3 * H + unit;
                gb[i][0] = g[0]; gb[i][1] = g[H]; gb[i][2] = g[2 * H];
            }
            {   // the beat's state scale, as tick_free_run_h2_kernel (no keep-masks)
                float mx = 1.f;
#pragma unroll
                for (int i = 0; i < E; ++i) mx = fmaxf(mx, fmaxf(fabsf(h0[i]), fabsf(h1[i])));
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
        float gi[E][3];
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const float *pt = p.ptab + (int64_t)tok[i] * 3 * H + unit;
            gi[i][0] = gb[i][0] + pt[0]; gi[i][1] = gb[i][1] + pt[H]; gi[i][2] = gb[i][2] + pt[2 * H];
        }
        [[maybe_unused]] unsigned plan_b[PLAN ? E : 1];        // PLAN: the tick's plan bytes of the lane's note, raw until the logits
        if constexpr (PLAN) {
#pragma unroll
            for (int i = 0; i < E; ++i) plan_b[i] = p.plan[rows[i] * p.row_stride + t * p.tick_stride + (note_ok ? note : 0)];
        }
        if constexpr (GROUPS)                                  // (last read two barriers ago, next read behind the logits' barrier)
            for (int e = threadIdx.x; e < 16 * 64; e += H * 4) (&cnt[0][0])[e] = 0;
        // ---- layer 0: matrix 0
        {
            f32x4 acc0[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            const unsigned short *ab = &hA0[cur][aoff];
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
                }
            }
            float ar[E], az[E], an[E];
            elems(acc0[0], ar); elems(acc0[1], az); elems(acc0[2], an);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float r = fast_sigmoid(gi[i][0] + ar[i] * us0 + b0r);
                const float z = fast_sigmoid(gi[i][1] + az[i] * us0 + b0z);
                const float n = fast_tanh(gi[i][2] + r * (an[i] * us0 + b0n));
                h0[i] = (1.f - z) * n + z * h0[i];
                store_split2<false>(&hA0[cur ^ 1][lrow(i) * HP + unit], PLANE, h0[i], h_s);
                store_split2<false>(&midp[lrow(i) * HP + unit], PLANE, h0[i], h_s);
                h0f[lrow(i)][unit] = h0[i];
            }
        }
        lds_barrier();
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
        lds_barrier();
        // ---- logits (fp32 MFMA, weights in LDS) on the first waves -> lgs
        if (w < ntile) {
            f32x4 lg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kq = 0; kq < KQ; ++kq) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(&h1f[arow][16 * kq + 4 * quad]);
                const f32x4 b = *reinterpret_cast<const f32x4 *>(&wout_s[note][16 * kq + 4 * quad]);
#pragma unroll
                for (int j = 0; j < 4; ++j) lg = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], lg, 0, 0, 0);
            }
            float lv[E];
            elems(lg, lv);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                bool on = note_on;
                if constexpr (PLAN) on = note_ok && plan_b[i] != 0;
                lgs[lrow(i) * FLT_LS + note] = on ? fmaxf(lv[i] + bout, 0.f) : -1.f;
            }
        }
        lds_barrier();
        // ---- selection, stage 1: a row's candidates and each note's rank inside its row.  Unit (element i, tile q) on wave
        // (4 i + q) mod NW: the wave forms ALL the row's candidates itself (the waves that share a row write the same bits to cnd),
        // then walks the row for its tile's 16 notes.  GROUPS: turn g of NG, the rows of group g (above)
        for (int g = 0;; ++g) {
            for (int u = w; u < 4 * E; u += NW) {
                const int i = u >> 2, tq = u & 3;
                if (tq >= ntile) continue;
                const int r = lrow(i);
                [[maybe_unused]] bool in_turn = true;
                if constexpr (GROUPS) {
                    in_turn = (r & (WP - 1)) / WS == g;
                    if (__ballot(in_turn) == 0) continue;
                }
                float lv[4], c[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) lv[q] = lgs[r * FLT_LS + 16 * q + col];
                const float big = row16_max(fmaxf(fmaxf(lv[0], lv[1]), fmaxf(lv[2], lv[3])));
                float e[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) e[q] = lv[q] >= 0.f ? expf(lv[q] - big) : 0.f;
                const float ls = logf(row16_sum((e[0] + e[1]) + (e[2] + e[3])));
                const float sc = score_s[r];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c[q] = lv[q] >= 0.f ? sc + ((lv[q] - big) - ls) : (PLAN ? __builtin_nanf("") : -INFINITY);
                    if constexpr (GROUPS) c[q] = beam_penalised(c[q], lam, cnt[r >> wsh][16 * q + col]);
                    cnd[r * FLT_LS + 16 * q + col] = c[q];
                }
                [[maybe_unused]] float lpm = -INFINITY;            // GROUPS: the unpenalised sum of (row, the lane's note)
                if constexpr (GROUPS) {
                    float lvm = lv[0];
#pragma unroll
                    for (int q = 1; q < 4; ++q) lvm = tq == q ? lv[q] : lvm;
                    lpm = logp_s[r] + ((lvm - big) - ls);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                float mine = c[0];
#pragma unroll
                for (int q = 1; q < 4; ++q) mine = tq == q ? c[q] : mine;
                const int v = 16 * tq + col;
                if constexpr (PLAN) {
                    int first_on = 0;                              // the row's first allowed note (the quad's 16 lanes hold the row)
#pragma unroll
                    for (int q = 3; q >= 0; --q) {
                        const int bits = (int)((unsigned)(__ballot(lv[q] >= 0.f) >> (16 * quad)) & 0xffffu);
                        first_on = bits != 0 ? 16 * q + __ffs(bits) - 1 : first_on;
                    }
                    int rank = 0, nal = 0, nbad = 0;
#pragma unroll 4
                    for (int n4 = 0; n4 < 16 * ntile; n4 += 4) {
                        const f32x4 q4 = *reinterpret_cast<const f32x4 *>(&cnd[r * FLT_LS + n4]);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float cn = q4[j];
                            const bool bad = cn != cn;
                            rank += (cn > mine || (cn == mine && n4 + j < v)) ? 1 : 0;
                            nal += bad ? 0 : 1;
                            nbad += bad && n4 + j < v ? 1 : 0;
                        }
                    }
                    const bool filler = mine != mine;
                    const int slot = filler ? nal + nbad : rank;
                    if constexpr (GROUPS) {
                        if (slot < WS && in_turn) {
                            top_c[r][slot] = filler ? -INFINITY : mine;
                            top_v[r][slot] = filler ? first_on : v;
                            top_l[r][slot] = filler ? -INFINITY : lpm;
                        }
                    } else {
                        if (slot < W) { top_c[r][slot] = filler ? -INFINITY : mine; top_v[r][slot] = filler ? first_on : v; }
                    }
                    continue;
                }
                int rank = 0;
#pragma unroll 4
                for (int n4 = 0; n4 < 16 * ntile; n4 += 4) {
                    const f32x4 q4 = *reinterpret_cast<const f32x4 *>(&cnd[r * FLT_LS + n4]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float cn = q4[j];
                        rank += (cn > mine || (cn == mine && n4 + j < v)) ? 1 : 0;
                    }
                }
                if (rank < W) { top_c[r][rank] = mine; top_v[r][rank] = v; }
            }
            lds_barrier();
            // ---- stage 2: a code's first W are among its W rows' first W each (top: every row's in its own order, slots >= W -inf).
            // Every (row, slot) entry counts the entries of its code ordered before it, Q lanes an entry (each a share of the code's
            // rows, 16 slots a row in four 16-byte reads), the lanes' counts added by the xor butterfly; rank j < W: new beam j
            {
                constexpr int NT = 4 * H;
                const int nent = RW << wsh;
                int qsh = 0;
                while ((nent << (qsh + 1)) <= NT && qsh < wsh) ++qsh;
                const int Q = 1 << qsh, span = WP >> qsh, per = NT >> qsh;
                const int part = threadIdx.x & (Q - 1);
                for (int e0 = 0; e0 < nent; e0 += per) {
                    const int en = e0 + ((int)threadIdx.x >> qsh);
                    const bool in = en < nent;
                    const int r = in ? en >> wsh : 0, s = en & (WP - 1);
                    const int k = r & (WP - 1), cb = r & ~(WP - 1);
                    const float c = top_c[r][s];
                    const int v = top_v[r][s];
                    int rank = 0;
                    int klo = part * span, khi = min((part + 1) * span, W);
                    if constexpr (GROUPS) { klo = max(klo, g * WS); khi = min(khi, (g + 1) * WS); }
                    for (int k2 = klo; k2 < khi; ++k2) {
                        const f32x4 *pc = reinterpret_cast<const f32x4 *>(&top_c[cb + k2][0]);
                        const beam_i32x4 *pv = reinterpret_cast<const beam_i32x4 *>(&top_v[cb + k2][0]);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const f32x4 c4 = pc[j];
                            const beam_i32x4 v4 = pv[j];
#pragma unroll
                            for (int m = 0; m < 4; ++m) {
                                const float c2 = c4[m];
                                const int v2 = v4[m];
                                if constexpr (PLAN) {
                                    const int s2 = 4 * j + m;
                                    rank += s2 < WS && (c2 > c || (c2 == c && (k2 < k || (k2 == k && s2 < s)))) ? 1 : 0;
                                } else {
                                    rank += beam_before(c2, k2, v2, c, k, v) ? 1 : 0;
                                }
                            }
                        }
                    }
                    for (int off = 1; off < Q; off <<= 1) rank += __shfl_xor(rank, off, 64);
                    if (!in || part != 0 || k >= W || s >= WS || rank >= WS) continue;
                    if constexpr (GROUPS) {
                        if (k < g * WS || k >= (g + 1) * WS) continue;
                        rank += g * WS;                            // the new beam's index inside its code
                        logp_s[cb + rank] = top_l[r][s];
                        if (c > -INFINITY && g + 1 < NG)       // a finite pick: the groups behind this one pay for its note
                            __hip_atomic_fetch_add(&cnt[r >> wsh][min(v, 63)], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    const int nr = cb + rank, vv = min(v, p.vocab - 1);
                    sel_par[nr] = k;
                    sel_note[nr] = vv;
                    score_s[nr] = c;                               // (read by stage 1 only: free by now)
                    hist_p[t][nr] = (unsigned char)k;
                    hist_v[t][nr] = (unsigned char)vv;
                    const int code = code0 + (r >> wsh);
                    if (code < B) {
                        const int64_t o = ((int64_t)code * ticks + t) * W + rank;
                        p.parents[o] = k;
                        p.tokens[o] = vv;
                        p.scores_hist[o] = c;
                    }
                }
            }
            if constexpr (!GROUPS) break;
            else {
                if (g + 1 >= NG) break;
                lds_barrier();                                     // the next group's stage 1 reads cnt
            }
        }
        lds_barrier();
        // ---- every beam takes its parent's states and its note
        const bool carry = t + 1 < ticks && (t + 1) % p.tpb != 0;      // (a beat's first tick restarts every beam from the beat's states)
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const int r = lrow(i);
            const int pr = ((r >> wsh) << wsh) + sel_par[r];
            tok[i] = sel_note[r];
            if (carry) {
                h0[i] = h0f[pr][unit];
                h1[i] = h1f[pr][unit];
                store_split2<false>(&hA0[cur ^ 1][r * HP + unit], PLANE, h0[i], h_s);
                store_split2<false>(&hA1[cur ^ 1][r * HP + unit], PLANE, h1[i], h_s);
            }
        }
        lds_barrier();
    }
    if (threadIdx.x < RW) {
        const int r = threadIdx.x, k = r & (WP - 1), cb = (r >> wsh) << wsh;
        const int code = code0 + (r >> wsh);
        if (code < B && k < W) {
            int at = k;
            for (int t = ticks - 1; t >= 0; --t) {
                p.sequences[((int64_t)code * W + k) * ticks + t] = hist_v[t][cb + at];
                at = hist_p[t][cb + at];
            }
            p.scores[(int64_t)code * W + k] = score_s[r];
            if constexpr (GROUPS) p.log_probs[(int64_t)code * W + k] = logp_s[r];
        }
    }
}

}  // namespace arvae

using namespace arvae;

// what the three entry points check of a width and a mask: 1 <= width <= 16, the mask's count given by the host (the mask lives on the
// device) and at least `width` notes allowed, so that `width` distinct hypotheses exist after the first tick
int arvae::beam_width_check(const char *who, int32_t width, int32_t vocab, const uint8_t *allow, int32_t allowed) {
    ARVAE_REQUIRE(width >= 1 && width <= BEAM_MAX_WIDTH, "%s: width %d is outside [1, %d]", who, width, BEAM_MAX_WIDTH);
    ARVAE_REQUIRE(vocab >= 1, "%s: vocab %d is not positive", who, vocab);
    ARVAE_REQUIRE(allowed >= 1 && allowed <= vocab, "%s: allowed %d is outside [1, vocab = %d]", who, allowed, vocab);
    ARVAE_REQUIRE(allow != nullptr || allowed == vocab, "%s: allowed %d without a mask (allow is null: allowed must be vocab = %d)", who,
                  allowed, vocab);
    ARVAE_REQUIRE(width <= allowed, "%s: width %d is above the %d allowed notes", who, width, allowed);
    return ARVAE_OK;
}

extern "C" int arvae_beam_select(const float *logits, const float *scores_in, int32_t codes, int32_t width, int32_t vocab, int32_t live,
                                 const uint8_t *allow, int32_t allowed, int32_t *parents, int64_t *notes, float *scores_out,
                                 arvae_stream_t stream) {
    ARVAE_REQUIRE(logits && scores_in && parents && notes && scores_out, "beam_select: null pointer");
    ARVAE_REQUIRE(codes >= 1, "beam_select: codes %d is not positive", codes);
    if (const int rc = beam_width_check("beam_select", width, vocab, allow, allowed)) return rc;
    ARVAE_REQUIRE(live >= 1 && live <= width, "beam_select: live %d is outside [1, width = %d]", live, width);
    ARVAE_REQUIRE((int64_t)live * allowed >= width, "beam_select: %d live beams of %d allowed notes give fewer than width = %d candidates",
                  live, allowed, width);
    beam_select_launch(logits, scores_in, codes, width, vocab, live, allow, 0, parents, notes, scores_out, 1, 0.f, nullptr, nullptr,
                       as_stream(stream));
    return check_launch("beam_select_kernel");
}

extern "C" int arvae_beam_select_planned(const float *logits, const float *scores_in, int32_t codes, int32_t width, int32_t vocab, int32_t live,
                                         const arvae_note_plan_t *plan, int32_t ticks, int32_t tick, int32_t *parents, int64_t *notes,
                                         float *scores_out, arvae_stream_t stream) {
    ARVAE_REQUIRE(logits && scores_in && parents && notes && scores_out, "beam_select_planned: null pointer");
    ARVAE_REQUIRE(codes >= 1, "beam_select_planned: codes %d is not positive", codes);
    ARVAE_REQUIRE(width >= 1 && width <= BEAM_MAX_WIDTH, "beam_select_planned: width %d is outside [1, %d]", width, BEAM_MAX_WIDTH);
    ARVAE_REQUIRE(vocab >= 1, "beam_select_planned: vocab %d is not positive", vocab);
    ARVAE_REQUIRE(live >= 1 && live <= width, "beam_select_planned: live %d is outside [1, width = %d]", live, width);
    if (const int rc = note_plan_check("beam_select_planned", plan, ticks, vocab)) return rc;
    ARVAE_REQUIRE(tick >= 0 && tick < ticks, "beam_select_planned: tick %d is outside [0, %d)", tick, ticks);
    beam_select_launch(logits, scores_in, codes, width, vocab, live, plan->allow + tick * plan->tick_stride, plan->row_stride, parents,
                       notes, scores_out, 1, 0.f, nullptr, nullptr, as_stream(stream));
    return check_launch("beam_select_kernel");
}

// what the grouped entry points check of (width, groups, penalty)
int arvae::beam_groups_check(const char *who, int32_t width, int32_t groups, float penalty) {
    ARVAE_REQUIRE(width >= 1 && width <= BEAM_MAX_WIDTH, "%s: width %d is outside [1, %d]", who, width, BEAM_MAX_WIDTH);
    ARVAE_REQUIRE(groups >= 1 && groups <= width, "%s: groups %d is outside [1, width = %d]", who, groups, width);
    ARVAE_REQUIRE(width % groups == 0, "%s: groups %d does not divide width %d", who, groups, width);
    ARVAE_REQUIRE(std::isfinite(penalty) && penalty >= 0.f, "%s: penalty %g is not a finite number >= 0", who, (double)penalty);
    return ARVAE_OK;
}

extern "C" int arvae_beam_select_groups(const float *logits, const float *scores_in, const float *logp_in, int32_t codes, int32_t width,
                                        int32_t groups, float penalty, int32_t vocab, int32_t live, const arvae_note_plan_t *plan,
                                        int32_t ticks, int32_t tick, int32_t *parents, int64_t *notes, float *scores_out, float *logp_out,
                                        arvae_stream_t stream) {
    ARVAE_REQUIRE(logits && scores_in && logp_in && parents && notes && scores_out && logp_out, "beam_select_groups: null pointer");
    ARVAE_REQUIRE(codes >= 1, "beam_select_groups: codes %d is not positive", codes);
    if (const int rc = beam_groups_check("beam_select_groups", width, groups, penalty)) return rc;
    ARVAE_REQUIRE(vocab >= 1, "beam_select_groups: vocab %d is not positive", vocab);
    ARVAE_REQUIRE(live >= 1 && live <= width / groups, "beam_select_groups: live %d is outside [1, width / groups = %d]", live,
                  width / groups);
    if (const int rc = note_plan_check("beam_select_groups", plan, ticks, vocab)) return rc;
    ARVAE_REQUIRE(tick >= 0 && tick < ticks, "beam_select_groups: tick %d is outside [0, %d)", tick, ticks);
    beam_select_launch(logits, scores_in, codes, width, vocab, live, plan->allow + tick * plan->tick_stride, plan->row_stride, parents,
                       notes, scores_out, groups, penalty, logp_in, logp_out, as_stream(stream));
    return check_launch("beam_select_kernel");
}

extern "C" int arvae_sequence_log_prob(const float *weights, const int64_t *tokens, int32_t rows, int32_t steps, int32_t vocab,
                                       const uint8_t *allow, float *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(weights && tokens && out, "sequence_log_prob: null pointer");
    ARVAE_REQUIRE(rows >= 1, "sequence_log_prob: rows %d is not positive", rows);
    ARVAE_REQUIRE(steps >= 1, "sequence_log_prob: steps %d is not positive", steps);
    ARVAE_REQUIRE(vocab >= 1, "sequence_log_prob: vocab %d is not positive", vocab);
    ARVAE_LAUNCH(sequence_log_prob_kernel, dim3(rows), dim3(64), 0, as_stream(stream), weights, tokens, steps, vocab, allow, (int64_t)0,
                 (int64_t)0, out);
    return check_launch("sequence_log_prob_kernel");
}

extern "C" int arvae_sequence_log_prob_planned(const float *weights, const int64_t *tokens, int32_t rows, int32_t steps, int32_t vocab,
                                               const arvae_note_plan_t *plan, float *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(weights && tokens && out, "sequence_log_prob_planned: null pointer");
    ARVAE_REQUIRE(rows >= 1, "sequence_log_prob_planned: rows %d is not positive", rows);
    ARVAE_REQUIRE(steps >= 1, "sequence_log_prob_planned: steps %d is not positive", steps);
    ARVAE_REQUIRE(vocab >= 1, "sequence_log_prob_planned: vocab %d is not positive", vocab);
    if (const int rc = note_plan_check("sequence_log_prob_planned", plan, steps, vocab)) return rc;
    ARVAE_LAUNCH(sequence_log_prob_kernel, dim3(rows), dim3(64), 0, as_stream(stream), weights, tokens, steps, vocab, plan->allow,
                 plan->row_stride, plan->tick_stride, out);
    return check_launch("sequence_log_prob_kernel");
}

extern "C" int arvae_tick_beam_search_supported(int32_t hidden, int32_t vocab, int32_t width) {
    return arvae_tick_free_run_supported(hidden, vocab) && width >= 1 && width <= BEAM_MAX_WIDTH;
}

extern "C" int arvae_tick_beam_search_groups_supported(int32_t hidden, int32_t vocab, int32_t width, int32_t groups) {
    return arvae_tick_beam_search_supported(hidden, vocab, width) && groups >= 1 && groups <= width && width % groups == 0;
}

extern "C" int64_t arvae_tick_beam_search_ws_floats(int32_t hidden) { return arvae_tick_free_run_ws_floats(hidden); }

// the three one-launch searches: plan null = arvae_tick_beam_search's mask and count, else the plan (no count: dead slots exist);
// groups 0 = not grouped, else the planned search in that many groups (log_probs then required)
static int tick_beam_search_launch(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                   const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat,
                                   int32_t hidden, int32_t vocab, int32_t width, const uint8_t *allow, int32_t allowed,
                                   const arvae_note_plan_t *plan, int32_t *parents, int64_t *tokens, float *scores_hist,
                                   int64_t *sequences, float *scores, float *ws, arvae_stream_t stream, int32_t groups = 0,
                                   float penalty = 0.f, float *log_probs = nullptr) {
    ARVAE_REQUIRE(wts && h0_l0 && h0_l1 && gib && ptab, "tick_beam_search: null pointer");
    ARVAE_REQUIRE(wts->w_hh0 && wts->b_hh0 && wts->w_ih1 && wts->b_ih1 && wts->w_hh1 && wts->b_hh1 && wts->w_out && wts->b_out,
                  "tick_beam_search: null weight pointer");
    ARVAE_REQUIRE(parents && tokens && scores_hist && sequences && scores, "tick_beam_search: null output pointer");
    ARVAE_REQUIRE(ws != nullptr, "tick_beam_search: null workspace (arvae_tick_beam_search_ws_floats)");
    ARVAE_REQUIRE(batch >= 1 && beats >= 1 && ticks_per_beat >= 1, "tick_beam_search: empty problem");
    ARVAE_REQUIRE(beats * (int64_t)ticks_per_beat <= BEAM_MAX_TICKS, "tick_beam_search: %lld ticks are above the %d the kernel keeps",
                  (long long)beats * ticks_per_beat, BEAM_MAX_TICKS);
    ARVAE_REQUIRE(arvae_gru_seq_supported(hidden), "tick_beam_search: hidden size %d is not built (32, 64, 128)", hidden);
    ARVAE_REQUIRE(arvae_tick_free_run_supported(hidden, vocab), "tick_beam_search: vocab of %d notes not supported at hidden size %d",
                  vocab, hidden);
    if (plan == nullptr) {
        if (const int rc = beam_width_check("tick_beam_search", width, vocab, allow, allowed)) return rc;
    } else {
        ARVAE_REQUIRE(width >= 1 && width <= BEAM_MAX_WIDTH, "tick_beam_search: width %d is outside [1, %d]", width, BEAM_MAX_WIDTH);
        if (const int rc = note_plan_check("tick_beam_search_planned", plan, (int64_t)beats * ticks_per_beat, vocab)) return rc;
    }
    ARVAE_REQUIRE(arvae_tick_beam_search_supported(hidden, vocab, width), "tick_beam_search: width %d at hidden size %d is not offered",
                  width, hidden);
    ARVAE_REQUIRE(h0_stride == 0 || h0_stride >= hidden, "tick_beam_search: h0_stride %lld is below the hidden size %d",
                  (long long)h0_stride, hidden);
    ARVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "tick_beam_search: workspace must be 16-byte aligned");
    TickBeamGroups p{};
    p.w_hh0 = wts->w_hh0; p.b_hh0 = wts->b_hh0; p.w_ih1 = wts->w_ih1; p.b_ih1 = wts->b_ih1;
    p.w_hh1 = wts->w_hh1; p.b_hh1 = wts->b_hh1; p.w_out = wts->w_out; p.b_out = wts->b_out;
    p.h0_l0 = h0_l0; p.h0_l1 = h0_l1; p.h0_stride = h0_stride != 0 ? h0_stride : hidden; p.gib = gib; p.ptab = ptab; p.allow = allow;
    p.batch = batch; p.beats = beats; p.tpb = ticks_per_beat; p.vocab = vocab; p.width = width;
    while ((1 << p.wshift) < width) ++p.wshift;
    p.parents = parents; p.tokens = tokens; p.scores_hist = scores_hist; p.sequences = sequences; p.scores = scores;
    if (plan != nullptr) { p.plan = plan->allow; p.row_stride = plan->row_stride; p.tick_stride = plan->tick_stride; }
    if (groups != 0) { p.groups = groups; p.gwidth = width / groups; p.penalty = penalty; p.log_probs = log_probs; }
    TickPrep tp{};
    tp.w[0] = wts->w_hh0; tp.w[1] = wts->w_ih1; tp.w[2] = wts->w_hh1;
    tp.nmat = 3;
    tp.out = reinterpret_cast<uint4 *>(ws);
    hipStream_t st = as_stream(stream);
    // a workgroup owns whole codes: the rows per workgroup for batch * WP rows, and at least one code's WP
    const int wp = 1 << p.wshift;
    const int rw = std::max(gru_rows_per_wg(batch * wp, 1), std::max(wp, 4));
    const dim3 gr((batch + rw / wp - 1) / (rw / wp));
    const uint4 *packed = reinterpret_cast<const uint4 *>(ws);
    bool rw_known = false;
    const bool h_known = with_int<128, 64, 32>(hidden, [&](auto HH) {
        tick_prep_launch<decltype(HH)::value>(tp, ws, st);
        rw_known = with_int<4, 8, 16>(rw, [&](auto RW) {
            constexpr int H = decltype(HH)::value, R = decltype(RW)::value;
            if (groups != 0) ARVAE_LAUNCH((tick_beam_search_kernel<H, R, TickBeamGroups>), gr, dim3(4 * H), 0, st, p, packed);
            else if (plan != nullptr)
                ARVAE_LAUNCH((tick_beam_search_kernel<H, R, TickBeamPlanned>), gr, dim3(4 * H), 0, st,
                             static_cast<const TickBeamPlanned &>(p), packed);
            else ARVAE_LAUNCH((tick_beam_search_kernel<H, R, TickBeam>), gr, dim3(4 * H), 0, st, static_cast<const TickBeam &>(p), packed);
        });
    });
    ARVAE_REQUIRE(h_known && rw_known, "tick_beam_search: no kernel for hidden size %d at %d rows per workgroup", hidden, rw);
    return check_launch("tick_beam_search_kernel");
}

extern "C" int arvae_tick_beam_search(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                      const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat,
                                      int32_t hidden, int32_t vocab, int32_t width, const uint8_t *allow, int32_t allowed,
                                      int32_t *parents, int64_t *tokens, float *scores_hist, int64_t *sequences, float *scores, float *ws,
                                      arvae_stream_t stream) {
    return tick_beam_search_launch(wts, h0_l0, h0_l1, h0_stride, gib, ptab, batch, beats, ticks_per_beat, hidden, vocab, width, allow,
                                   allowed, nullptr, parents, tokens, scores_hist, sequences, scores, ws, stream);
}

extern "C" int arvae_tick_beam_search_planned(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                              const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat,
                                              int32_t hidden, int32_t vocab, int32_t width, const arvae_note_plan_t *plan,
                                              int32_t *parents, int64_t *tokens, float *scores_hist, int64_t *sequences, float *scores,
                                              float *ws, arvae_stream_t stream) {
    ARVAE_REQUIRE(plan != nullptr, "tick_beam_search_planned: null plan");
    return tick_beam_search_launch(wts, h0_l0, h0_l1, h0_stride, gib, ptab, batch, beats, ticks_per_beat, hidden, vocab, width, nullptr,
                                   vocab, plan, parents, tokens, scores_hist, sequences, scores, ws, stream);
}

extern "C" int arvae_tick_beam_search_groups(const arvae_tick_weights_t *wts, const float *h0_l0, const float *h0_l1, int64_t h0_stride,
                                             const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat,
                                             int32_t hidden, int32_t vocab, int32_t width, int32_t groups, float penalty,
                                             const arvae_note_plan_t *plan, int32_t *parents, int64_t *tokens, float *scores_hist,
                                             int64_t *sequences, float *scores, float *log_probs, float *ws, arvae_stream_t stream) {
    ARVAE_REQUIRE(plan != nullptr, "tick_beam_search_groups: null plan");
    if (const int rc = beam_groups_check("tick_beam_search_groups", width, groups, penalty)) return rc;
    ARVAE_REQUIRE(log_probs != nullptr, "tick_beam_search_groups: null log_probs");
    return tick_beam_search_launch(wts, h0_l0, h0_l1, h0_stride, gib, ptab, batch, beats, ticks_per_beat, hidden, vocab, width, nullptr,
                                   vocab, plan, parents, tokens, scores_hist, sequences, scores, ws, stream, groups, penalty, log_probs);
}
