// What a decoded measure sounds and looks like: vocabulary indices -> note events (arvae_measure_notes) and -> the bytes of
// piano-roll figures (arvae_render_pianoroll), one launch each.  Time is counted in twelfths of a quarter note: tick t of a
// measure lies in beat t / 6 at sub-position s = t % 6, starts at twelfth 12 (t / 6) + {0, 3, 4, 6, 8, 9}[s] and lasts
// {3, 1, 2, 2, 1, 3}[s] of them (TICK_VALUES and compute_tick_durations of the reference's bar_dataset_helpers.py, times 12).
// An element begins at every tick that does not hold the slur and lasts to the next such tick or the measure's end
// (tensor_to_m21score, bar_dataset.py:224-254); measures do not tie into each other (concatenate_scores, :256-268).
// Both kernels walk back over slurs from the tick they stand on: a measure has few ticks and its row stays in the cache.
#include <cmath>
#include "common.h"

namespace arvae {

// twelfth at which tick t starts; t = T gives the measure's length 2 T
__device__ __forceinline__ int tick_twelfth(int t) {
    const int beat = t / 6, s = t - beat * 6;
    return 12 * beat + (int)((0x986430u >> (4 * s)) & 15u);
}
// the tick of a beat that holds twelfth w (0..11) of it: 0 0 0 1 2 2 3 3 4 5 5 5
__device__ __forceinline__ int twelfth_tick(int w) { return (int)((0x555433221000ull >> (4 * w)) & 15ull); }

struct NoteTables {
    const int32_t *midi;
    const uint8_t *is_note;
    int32_t vocab, slur;
};

// the element that covers tick t of a measure: its first tick (-1 inside leading slurs) and its MIDI pitch (0: silence)
__device__ __forceinline__ void covering_element(const int64_t *__restrict__ row, int t, const NoteTables &nt, int &start, int &pitch) {
    start = -1;
    pitch = 0;
    for (int s = t; s >= 0; --s) {
        const int64_t x = row[s];
        if (x == nt.slur) continue;
        start = s;
        if (x >= 0 && x < nt.vocab && nt.is_note[x]) pitch = nt.midi[x];      // (a token outside [0, V) indexes nothing)
        return;
    }
}

// the first tick after t that begins an element, or T
__device__ __forceinline__ int next_element(const int64_t *__restrict__ row, int t, int T, int32_t slur) {
    int e = t + 1;
    while (e < T && row[e] == slur) ++e;
    return e;
}

__global__ __launch_bounds__(256) void measure_notes_kernel(const int64_t *__restrict__ score, int64_t items, int T, NoteTables nt,
                                                            int32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / T;
        const int t = (int)(i - m * T);
        const int64_t *row = score + m * T;
        int start, pitch;
        covering_element(row, t, nt, start, pitch);
        int length = 0;
        if (start == t) length = tick_twelfth(next_element(row, t, T, nt.slur)) - tick_twelfth(t);
        out[i * 3 + 0] = pitch;
        out[i * 3 + 1] = start;
        out[i * 3 + 2] = length;
    }
}

struct RollGeom {
    int64_t total;                 // bytes of all figures
    uint32_t frame_bytes;          // H * W * 3 < 2^31
    uint32_t lead;                 // bytes between the 4-byte boundary below `out` and `out` (0..3)
    uint32_t H, roll_w, gap, measure_w, beat_w, ppt, mark, panel_cell;
    int32_t K, T, pitch_hi, dot_radius;
    float vmin, vmax;
    FastDiv by_row, by_measure, by_ppt, by_ppp, by_cell;      // 3 W, measure_w, px_per_twelfth, px_per_pitch, panel_cell
};

// shade 0..127 of roll pixel (y, x) of figure f: the first layer that applies (onset mark, note, measure line, beat line, even pitch)
__device__ __forceinline__ uint32_t roll_shade(const RollGeom &g, const NoteTables &nt, const int64_t *__restrict__ score, int64_t f,
                                               uint32_t y, uint32_t x) {
    uint32_t k, xin;
    g.by_measure.divmod(x, k, xin);                      // (k < K: x < roll_w = K measure_w)
    const int w = (int)g.by_ppt.div(xin);                // twelfth of the measure
    const int beat = w / 12;
    const int t = beat * 6 + twelfth_tick(w - beat * 12);
    const int p = g.pitch_hi - (int)g.by_ppp.div(y);     // the MIDI pitch of this pixel row
    int start, pitch;
    covering_element(score + (f * g.K + k) * g.T, t, nt, start, pitch);
    if (pitch > 0) {
        const uint32_t from = xin - (uint32_t)tick_twelfth(start) * g.ppt;      // pixel columns since the element began
        if (from < g.mark && p >= pitch - 1 && p <= pitch + 1) return 127;
        if (p == pitch) return 90;
    }
    if (xin == 0) return 100;
    if (xin % g.beat_w == 0) return 50;
    return (p & 1) ? 0 : 30;
}

// 1 where panel pixel (y, px) lies on the disc of its cell's measure
__device__ __forceinline__ bool panel_disc(const RollGeom &g, const float *__restrict__ values, int64_t f, uint32_t y, uint32_t px) {
    const uint32_t k = g.by_cell.div(px);                // (k < K: px < K panel_cell)
    const float value = values[f * g.K + k];
    if (!isfinite(value)) return false;
    float c = 0.5f;
    if (g.vmax != g.vmin) c = __fdiv_rn(__fsub_rn(value, g.vmin), __fsub_rn(g.vmax, g.vmin));
    c = fminf(fmaxf(c, 0.f), 1.f);
    const int row = (int)g.H - 1 - (int)floorf(__fadd_rn(__fmul_rn(c, (float)(g.H - 1)), 0.5f));
    const int dx = (int)px - (int)(k * g.panel_cell + g.panel_cell / 2), dy = (int)y - row;
    if (dx > g.dot_radius || dx < -g.dot_radius || dy > g.dot_radius || dy < -g.dot_radius) return false;      // (keeps the squares small)
    return dx * dx + dy * dy <= g.dot_radius * g.dot_radius;
}

// white -> matplotlib's darkest "Blues" (8, 48, 107)
__device__ __forceinline__ uint32_t blues(uint32_t v, uint32_t channel) {
    const uint32_t dark = channel == 0 ? 8u : (channel == 1 ? 48u : 107u);
    return 255u - (v * (255u - dark) + 63u) / 127u;
}

// as render_frames_kernel: word i covers the bytes [4 i - lead, 4 i - lead + 4) of the output; whole words leave as one aligned
// dword store, the words cut by the output's first or last byte as byte stores
__global__ __launch_bounds__(256) void render_pianoroll_kernel(RollGeom g, NoteTables nt, const int64_t *__restrict__ score,
                                                               const float *__restrict__ values, uint8_t *__restrict__ out, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int64_t first = i * 4 - g.lead;
        const int64_t lo = first < 0 ? 0 : first;
        int64_t f = lo / g.frame_bytes;
        uint32_t r = (uint32_t)(lo - f * g.frame_bytes);
        uint32_t word = 0, shade = 0;
        bool have = false;                  // shade is that of the pixel byte r - 1 belongs to
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t at = first + j;
            if (at < 0 || at >= g.total) continue;
            uint32_t y, in_row;
            g.by_row.divmod(r, y, in_row);
            const uint32_t x = in_row / 3, channel = in_row - 3 * x;
            if (!have || channel == 0) {    // 0..127: the roll's shade; 128: white; 129: black
                if (x < g.roll_w) shade = roll_shade(g, nt, score, f, y, x);
                else if (x < g.roll_w + g.gap) shade = 128;
                else shade = panel_disc(g, values, f, y, x - g.roll_w - g.gap) ? 129 : 128;
            }
            have = true;
            const uint32_t b = shade < 128 ? blues(shade, channel) : (shade == 128 ? 255u : 0u);
            word |= b << (8 * j);
            if (++r == g.frame_bytes) {
                r = 0;
                ++f;
                have = false;
            }
        }
        if (first >= 0 && first + 4 <= g.total) {
            *reinterpret_cast<uint32_t *>(out + first) = word;          // out + first = (out - lead) + 4 i: aligned
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (first + j >= 0 && first + j < g.total) out[first + j] = (uint8_t)(word >> (8 * j));
        }
    }
}

// H, the roll's and the frame's width and the frame's bytes; false with a message when an argument is bad or the frame has 2^31
// bytes or more
static bool roll_geometry(const char *who, int K, int T, int pitch_lo, int pitch_hi, int px_per_twelfth, int px_per_pitch, int with_panel,
                          int panel_cell, int gap, int64_t *h, int64_t *roll_w, int64_t *w, int64_t *bytes) {
    if (K <= 0 || T <= 0 || T % 6 != 0) {
        fail(ARVAE_E_INVALID, "%s: %d measures of %d ticks (both positive, the ticks a multiple of 6)", who, K, T);
        return false;
    }
    if (pitch_lo < 0 || pitch_hi > 127 || pitch_hi < pitch_lo) {
        fail(ARVAE_E_INVALID, "%s: pitches %d..%d (0 <= pitch_lo <= pitch_hi <= 127)", who, pitch_lo, pitch_hi);
        return false;
    }
    if (px_per_twelfth <= 0 || px_per_pitch <= 0) {
        fail(ARVAE_E_INVALID, "%s: px_per_twelfth %d and px_per_pitch %d must be positive", who, px_per_twelfth, px_per_pitch);
        return false;
    }
    if (with_panel && (panel_cell <= 0 || gap < 0)) {
        fail(ARVAE_E_INVALID, "%s: panel_cell %d must be positive, gap %d not negative", who, panel_cell, gap);
        return false;
    }
    const int64_t big = (int64_t)1 << 31;
    *h = (int64_t)(pitch_hi - pitch_lo + 1) * px_per_pitch;             // below 2^7 * 2^31
    const int64_t measure_w = (int64_t)(T / 6) * 12 * px_per_twelfth;   // below 2^29 * 2^4 * 2^31: no overflow; checked next
    bool fits = *h < big && measure_w < big;
    *roll_w = fits ? measure_w * K : 0;
    fits = fits && *roll_w < big;
    *w = *roll_w;
    if (fits && with_panel) *w += (int64_t)gap + (int64_t)K * panel_cell;       // below 2^31 + 2^31 + 2^62
    fits = fits && *w < big && *w * 3 < big && *h * (*w * 3) < big;
    if (!fits) {
        fail(ARVAE_E_INVALID, "%s: a figure of %d measures at %d x %d pixels a twelfth and a pitch has 2^31 bytes or more", who, K,
             px_per_twelfth, px_per_pitch);
        return false;
    }
    *bytes = *h * *w * 3;
    return true;
}

}  // namespace arvae

using namespace arvae;

extern "C" int arvae_measure_notes(const int64_t *score, int64_t M, int32_t T, const int32_t *midi_lut, const uint8_t *is_note, int32_t V,
                                   int32_t slur, int32_t *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(score && midi_lut && is_note && out, "measure_notes: null pointer");
    ARVAE_REQUIRE(M > 0 && T > 0 && T % 6 == 0, "measure_notes: %lld measures of %d ticks (both positive, the ticks a multiple of 6)",
                  (long long)M, T);
    ARVAE_REQUIRE(V > 0 && slur >= 0 && slur < V, "measure_notes: slur index %d outside the vocabulary [0, %d)", slur, V);
    ARVAE_REQUIRE(M <= ((int64_t)1 << 31) / T, "measure_notes: %lld x %d ticks are 2^31 or more", (long long)M, T);
    const int64_t items = M * T;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const NoteTables nt{midi_lut, is_note, V, slur};
    ARVAE_LAUNCH(measure_notes_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), score, items, T, nt, out);
    return check_launch("measure_notes");
}

extern "C" int64_t arvae_render_pianoroll_bytes(int32_t K, int32_t T, int32_t pitch_lo, int32_t pitch_hi, int32_t px_per_twelfth,
                                                int32_t px_per_pitch, int32_t with_panel, int32_t panel_cell, int32_t gap) {
    int64_t h, roll_w, w, bytes;
    return roll_geometry("render_pianoroll_bytes", K, T, pitch_lo, pitch_hi, px_per_twelfth, px_per_pitch, with_panel, panel_cell, gap, &h,
                         &roll_w, &w, &bytes) ? bytes : -1;
}

extern "C" int arvae_render_pianoroll(const int64_t *score, int32_t F, int32_t K, int32_t T, const int32_t *midi_lut, const uint8_t *is_note,
                                      int32_t V, int32_t slur, const float *values, float vmin, float vmax, int32_t pitch_lo,
                                      int32_t pitch_hi, int32_t px_per_twelfth, int32_t px_per_pitch, int32_t mark, int32_t panel_cell,
                                      int32_t gap, int32_t dot_radius, uint8_t *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(score && midi_lut && is_note && out, "render_pianoroll: null pointer");
    ARVAE_REQUIRE(F > 0, "render_pianoroll: %d figures must be positive", F);
    ARVAE_REQUIRE(V > 0 && slur >= 0 && slur < V, "render_pianoroll: slur index %d outside the vocabulary [0, %d)", slur, V);
    ARVAE_REQUIRE(mark >= 0, "render_pianoroll: mark %d must not be negative", mark);
    int64_t h, roll_w, w, bytes;
    if (!roll_geometry("render_pianoroll", K, T, pitch_lo, pitch_hi, px_per_twelfth, px_per_pitch, values != nullptr, panel_cell, gap, &h,
                       &roll_w, &w, &bytes))
        return ARVAE_E_INVALID;
    if (values) {
        ARVAE_REQUIRE(((uintptr_t)values & 3) == 0, "render_pianoroll: values must be 4-byte aligned");
        ARVAE_REQUIRE(dot_radius >= 0 && dot_radius < 32768, "render_pianoroll: dot_radius %d outside [0, 32768)", dot_radius);
        ARVAE_REQUIRE(std::isfinite(vmin) && std::isfinite(vmax) && vmin <= vmax, "render_pianoroll: vmin %f and vmax %f must be finite and ordered",
                      (double)vmin, (double)vmax);
    }
    ARVAE_REQUIRE((((uintptr_t)score & 7) | ((uintptr_t)midi_lut & 3)) == 0, "render_pianoroll: score and midi_lut must be aligned");

    RollGeom g;
    g.total = bytes * F;
    g.frame_bytes = (uint32_t)bytes;
    g.lead = (uint32_t)((uintptr_t)out & 3);
    g.H = (uint32_t)h;
    g.roll_w = (uint32_t)roll_w;
    g.gap = values ? (uint32_t)gap : 0u;
    g.measure_w = (uint32_t)(roll_w / K);
    g.beat_w = 12u * (uint32_t)px_per_twelfth;
    g.ppt = (uint32_t)px_per_twelfth;
    g.mark = (uint32_t)mark;
    g.panel_cell = values ? (uint32_t)panel_cell : 1u;
    g.K = K;
    g.T = T;
    g.pitch_hi = pitch_hi;
    g.dot_radius = dot_radius;
    g.vmin = vmin;
    g.vmax = vmax;
    g.by_row = FastDiv((uint32_t)(w * 3));
    g.by_measure = FastDiv(g.measure_w);
    g.by_ppt = FastDiv(g.ppt);
    g.by_ppp = FastDiv((uint32_t)px_per_pitch);
    g.by_cell = FastDiv(g.panel_cell);

    const int64_t words = (g.total + g.lead + 3) / 4;
    int64_t blocks = (words + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const NoteTables nt{midi_lut, is_note, V, slur};
    ARVAE_LAUNCH(render_pianoroll_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), g, nt, score, values, out, words);
    return check_launch("render_pianoroll");
}
