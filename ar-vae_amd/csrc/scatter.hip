// Latent-space scatter figures (the reference's utils/plotting.py:41-63 plot_dim): N points with a value each -> the bytes of a
// figure, F figures in one launch.  A block owns a 16 x 16 tile of one figure's canvas, one pixel a thread.  Tiles that touch the
// plot area walk the figure's points in index order, 256 at a time: every lane maps one point to its fixed-point pixel position
// (1/16 pixel) and tests its disc against the tile; the hits are compacted into LDS in index order (ballot and prefix count over
// the 64-lane wavefront, the waves' counts summed in wave order), and every pixel thread blends the compacted list in that order.
// The picture is therefore a function of the input order alone; there are no atomics.  The two floating-point steps (coordinate ->
// 1/16 pixel, value -> colour index) are chains of individually rounded fp32 operations; coverage and blending are integers.
// Everything outside the plot area -- frame, colour bar, tick marks and text -- is drawn from the layout and a by-value table of
// marks (glyph cells and tick marks) that the caller laid out on the host: the kernel only blits them.
#include <cmath>
#include "common.h"

namespace arvae {

constexpr int kTile = 16;                    // a tile is kTile x kTile pixels = one block of 256 threads
constexpr int kRowBytes = kTile * 3;
constexpr float kFar = 1048576.f;            // positions of 2^20 sixteenths and more lie 65536 pixels off: never on a canvas
// the layout, in pixels: [left] 56 | frame | plot | frame | 10 | bar frame | bar 12 | bar frame | ticks and labels 43 [right]
//                        [top] 10 | frame | plot | frame | ticks 4, labels, title 27 [bottom]
constexpr int kLeft = 57, kTop = 11, kBarGap = 12, kBarW = 12, kRight = 56, kBottom = 28, kMinPlot = 16;

// matplotlib's viridis at 256 levels (CC0 data), a colour as 0x00BBGGRR
__device__ const uint32_t kViridis[256] = {
    0x540144, 0x550244, 0x570344, 0x580545, 0x5a0645, 0x5b0845, 0x5c0946, 0x5e0b46,
    0x5f0c46, 0x610e46, 0x620f47, 0x631147, 0x651247, 0x661447, 0x671547, 0x691647,
    0x6a1847, 0x6b1948, 0x6c1a48, 0x6e1c48, 0x6f1d48, 0x701e48, 0x712048, 0x722148,
    0x732248, 0x742348, 0x752547, 0x762647, 0x772747, 0x782847, 0x792a47, 0x7a2b47,
    0x7b2c47, 0x7c2d46, 0x7c2f46, 0x7d3046, 0x7e3146, 0x7f3245, 0x7f3445, 0x803545,
    0x813645, 0x813744, 0x823944, 0x833a43, 0x833b43, 0x843c43, 0x843d42, 0x853e42,
    0x854042, 0x864141, 0x864241, 0x874340, 0x874440, 0x87453f, 0x88473f, 0x88483e,
    0x89493e, 0x894a3d, 0x894b3d, 0x894c3d, 0x8a4d3c, 0x8a4e3c, 0x8a503b, 0x8a513b,
    0x8b523a, 0x8b533a, 0x8b5439, 0x8b5539, 0x8b5638, 0x8c5738, 0x8c5837, 0x8c5937,
    0x8c5a36, 0x8c5b36, 0x8c5c35, 0x8c5d35, 0x8d5e34, 0x8d5f34, 0x8d6033, 0x8d6133,
    0x8d6232, 0x8d6332, 0x8d6431, 0x8d6531, 0x8d6631, 0x8d6730, 0x8d6830, 0x8d692f,
    0x8d6a2f, 0x8e6b2e, 0x8e6c2e, 0x8e6d2e, 0x8e6e2d, 0x8e6f2d, 0x8e702c, 0x8e712c,
    0x8e722c, 0x8e732b, 0x8e742b, 0x8e752a, 0x8e762a, 0x8e772a, 0x8e7829, 0x8e7929,
    0x8e7a28, 0x8e7a28, 0x8e7b28, 0x8e7c27, 0x8e7d27, 0x8e7e27, 0x8e7f26, 0x8e8026,
    0x8e8126, 0x8e8225, 0x8d8325, 0x8d8424, 0x8d8524, 0x8d8624, 0x8d8723, 0x8d8823,
    0x8d8923, 0x8d8922, 0x8d8a22, 0x8d8b22, 0x8d8c21, 0x8c8d21, 0x8c8e21, 0x8c8f20,
    0x8c9020, 0x8c9120, 0x8c921f, 0x8b931f, 0x8b941f, 0x8b951f, 0x8b961f, 0x8a971e,
    0x8a981e, 0x8a991e, 0x8a991e, 0x899a1e, 0x899b1e, 0x899c1e, 0x889d1e, 0x889e1e,
    0x889f1e, 0x87a01e, 0x87a11f, 0x86a21f, 0x86a31f, 0x85a420, 0x85a520, 0x85a621,
    0x84a721, 0x84a722, 0x83a823, 0x82a923, 0x82aa24, 0x81ab25, 0x81ac26, 0x80ad27,
    0x7fae28, 0x7faf29, 0x7eb02a, 0x7db12b, 0x7db12c, 0x7cb22e, 0x7bb32f, 0x7ab430,
    0x7ab532, 0x79b633, 0x78b735, 0x77b836, 0x76b938, 0x76b939, 0x75ba3b, 0x74bb3d,
    0x73bc3e, 0x72bd40, 0x71be42, 0x70be44, 0x6fbf45, 0x6ec047, 0x6dc149, 0x6cc24b,
    0x6bc24d, 0x69c34f, 0x68c451, 0x67c553, 0x66c655, 0x65c657, 0x64c759, 0x62c85b,
    0x61c95e, 0x60c960, 0x5fca62, 0x5dcb64, 0x5ccc67, 0x5bcc69, 0x59cd6b, 0x58ce6d,
    0x56ce70, 0x55cf72, 0x54d074, 0x52d077, 0x51d179, 0x4fd27c, 0x4ed27e, 0x4cd381,
    0x4bd383, 0x49d486, 0x47d588, 0x46d58b, 0x44d68d, 0x43d690, 0x41d792, 0x3fd795,
    0x3ed897, 0x3cd89a, 0x3ad99d, 0x38d99f, 0x37daa2, 0x35daa5, 0x33dba7, 0x32dbaa,
    0x30dcad, 0x2edcaf, 0x2cddb2, 0x2bddb5, 0x29ddb7, 0x27deba, 0x26debd, 0x24dfbf,
    0x22dfc2, 0x21dfc5, 0x1fe0c7, 0x1ee0ca, 0x1de0cd, 0x1ce1cf, 0x1be1d2, 0x1ae1d4,
    0x19e2d7, 0x18e2da, 0x18e2dc, 0x18e3df, 0x18e3e1, 0x18e3e4, 0x19e4e7, 0x19e4e9,
    0x1ae4ec, 0x1be5ee, 0x1ce5f1, 0x1ee5f3, 0x1fe6f6, 0x21e6f8, 0x22e6fa, 0x24e7fd,
};

// the font: 5 x 7 cells of the glyphs "0123456789-.: dimenso" in this order, bit 5 row + column set where the pixel is inked
__device__ const uint64_t kFont[ARVAE_SCATTER_GLYPHS] = {
    0x3a33ae62eull, 0x3884210c4ull, 0x7c444422eull, 0x3a306422eull, 0x211f4a988ull, 0x3a3083c3full, 0x3a317842eull,
    0x10842221full, 0x3a317462eull, 0x3a10f462eull, 0x000070000ull, 0x18c000000ull, 0x00c6018c0ull, 0x000000000ull,
    0x7a318fa10ull, 0x388421804ull, 0x56b5aac00ull, 0x383f8b800ull, 0x46319b400ull, 0x3e0e0f800ull, 0x3a318b800ull,
};

struct ScatterFigure {
    float xlo, kx, ylo, ky;        // position in sixteenths = (coordinate - lo) * k, k = 16 * extent / (hi - lo)
    float vmin, vden;              // colour = (value - vmin) / vden; vden = 0: the middle colour
};

struct ScatterParams {
    int64_t n;                     // points of a figure
    uint32_t frame_bytes;          // H * W * 3 < 2^31
    int32_t W, H, px0, py0, pw, ph, bar_x, bar_w, tiles_x, r16, alpha, n_marks;
    ScatterFigure fig[ARVAE_SCATTER_MAX_FIGURES];
    arvae_scatter_mark_t marks[ARVAE_SCATTER_MAX_MARKS];
};

// width and height of a mark's cell: an upright glyph, a glyph turned a quarter to the left, the two tick marks
__host__ __device__ __forceinline__ void mark_cell(int glyph, int rot, int &w, int &h) {
    if (glyph == ARVAE_SCATTER_TICK_X) { w = 1; h = 4; }
    else if (glyph == ARVAE_SCATTER_TICK_Y) { w = 4; h = 1; }
    else if (rot) { w = 7; h = 5; }
    else { w = 5; h = 7; }
}

__device__ __forceinline__ uint32_t value_colour(float v, const ScatterFigure &g) {
    if (g.vden == 0.f) return kViridis[128];
    float c = __fdiv_rn(__fsub_rn(v, g.vmin), g.vden);
    c = fminf(fmaxf(c, 0.f), 1.f);
    return kViridis[(int)floorf(__fadd_rn(__fmul_rn(c, 255.f), 0.5f))];
}

// a channel in 1/256ths under a marker of colour `col` (0..255) at alpha a / 256
__device__ __forceinline__ uint32_t blend(uint32_t c, uint32_t col, uint32_t a) { return (c * (256u - a) + col * 256u * a + 128u) >> 8; }

__global__ __launch_bounds__(256) void render_scatter_kernel(ScatterParams p, const float2 *__restrict__ points,
                                                             const float *__restrict__ values, uint8_t *__restrict__ out) {
    __shared__ int32_t hit_x[256], hit_y[256];
    __shared__ uint32_t hit_rgb[256];
    __shared__ int32_t wave_hits[4];
    __shared__ uint8_t tile_bytes[kTile * kRowBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.y;
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    const int x0 = tx * kTile, y0 = ty * kTile;
    const int x = x0 + (tid & 15), y = y0 + (tid >> 4);
    const bool inside = x >= p.px0 && x < p.px0 + p.pw && y >= p.py0 && y < p.py0 + p.ph;
    uint32_t rgb = 0xffffffu;

    if (x0 < p.px0 + p.pw && x0 + kTile > p.px0 && y0 < p.py0 + p.ph && y0 + kTile > p.py0) {      // the tile touches the plot area
        const ScatterFigure g = p.fig[f];
        // sixteenths from the plot area's corner: this pixel's centre, and the centres a disc must reach to touch the tile
        const int cx = 16 * (x - p.px0) + 8, cy = 16 * (y - p.py0) + 8;
        const int lo_x = 16 * (x0 - p.px0) + 8 - p.r16, hi_x = 16 * (x0 + kTile - 1 - p.px0) + 8 + p.r16;
        const int lo_y = 16 * (y0 - p.py0) + 8 - p.r16, hi_y = 16 * (y0 + kTile - 1 - p.py0) + 8 + p.r16;
        const int r2 = p.r16 * p.r16;
        const float2 *pts = points + (int64_t)f * p.n;
        const float *val = values + (int64_t)f * p.n;
        uint32_t c0 = 255u * 256u, c1 = c0, c2 = c0;
        for (int64_t base = 0; base < p.n; base += 256) {
            const int64_t i = base + tid;
            bool hit = false;
            int px = 0, py = 0;
            uint32_t colour = 0;
            if (i < p.n) {
                const float2 q = pts[i];
                const float v = val[i];
                const float qx = __fmul_rn(__fsub_rn(q.x, g.xlo), g.kx), qy = __fmul_rn(__fsub_rn(q.y, g.ylo), g.ky);
                if (qx > -kFar && qx < kFar && qy > -kFar && qy < kFar && isfinite(v)) {      // (a NaN compares false)
                    px = (int)floorf(__fadd_rn(qx, 0.5f));
                    py = 16 * p.ph - (int)floorf(__fadd_rn(qy, 0.5f));
                    hit = px >= lo_x && px <= hi_x && py >= lo_y && py <= hi_y;
                    if (hit) colour = value_colour(v, g);
                }
            }
            const uint64_t mask = __ballot(hit);
            if (lane == 0) wave_hits[wave] = __popcll(mask);
            __syncthreads();
            int at = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (w < wave) at += wave_hits[w];
                total += wave_hits[w];
            }
            if (hit) {
                hit_x[at] = px;
                hit_y[at] = py;
                hit_rgb[at] = colour;
            }
            __syncthreads();
            if (inside) {
                for (int k = 0; k < total; ++k) {
                    const int dx = cx - hit_x[k], dy = cy - hit_y[k];      // (|dx|, |dy| <= 240 + r16: no overflow)
                    if (dx * dx + dy * dy <= r2) {
                        const uint32_t col = hit_rgb[k];
                        c0 = blend(c0, col & 255u, (uint32_t)p.alpha);
                        c1 = blend(c1, (col >> 8) & 255u, (uint32_t)p.alpha);
                        c2 = blend(c2, (col >> 16) & 255u, (uint32_t)p.alpha);
                    }
                }
            }
            // (the next round writes wave_hits before its first barrier and the list after it: both were last read before the
            // barrier above or inside this round's loop, which every wave leaves before it reaches the next round's first barrier)
        }
        if (inside) rgb = ((c0 + 128u) >> 8) | (((c1 + 128u) >> 8) << 8) | (((c2 + 128u) >> 8) << 16);
    }
    if (!inside) {
        const bool rows = y >= p.py0 - 1 && y <= p.py0 + p.ph;
        if (rows && x >= p.px0 - 1 && x <= p.px0 + p.pw) {
            rgb = 0;                                     // the plot's frame
        } else if (rows && x >= p.bar_x - 1 && x <= p.bar_x + p.bar_w) {
            rgb = 0;                                     // the bar's frame, and inside it the table from bottom to top
            if (x >= p.bar_x && x < p.bar_x + p.bar_w && y >= p.py0 && y < p.py0 + p.ph)
                rgb = kViridis[((p.ph - 1 - (y - p.py0)) * 255 + (p.ph - 1) / 2) / (p.ph - 1)];
        } else {
            for (int m = 0; m < p.n_marks; ++m) {
                const arvae_scatter_mark_t mk = p.marks[m];
                if (mk.figure >= 0 && mk.figure != f) continue;
                int w, h;
                mark_cell(mk.glyph, mk.rot, w, h);
                if (mk.x >= x0 + kTile || mk.x + w <= x0 || mk.y >= y0 + kTile || mk.y + h <= y0) continue;      // (the same for the whole block)
                const int dx = x - mk.x, dy = y - mk.y;
                if (dx < 0 || dx >= w || dy < 0 || dy >= h) continue;
                if (mk.glyph >= ARVAE_SCATTER_GLYPHS) {
                    rgb = 0;
                } else {
                    const int col = mk.rot ? 4 - dy : dx, row = mk.rot ? dx : dy;
                    if ((kFont[mk.glyph] >> (row * 5 + col)) & 1ull) rgb = 0;
                }
            }
        }
    }

    // the tile's bytes leave row by row, as render_frames_kernel's do: slot k of a row covers the aligned dword k of the row's
    // bytes; a dword the row owns whole is one store, the row's first and last bytes beside it are byte stores
    uint8_t *cell = tile_bytes + (tid >> 4) * kRowBytes + (tid & 15) * 3;
    cell[0] = (uint8_t)rgb;
    cell[1] = (uint8_t)(rgb >> 8);
    cell[2] = (uint8_t)(rgb >> 16);
    __syncthreads();
    const int row = tid >> 4, slot = tid & 15;
    if (y0 + row < p.H) {
        const int cols = p.W - x0 < kTile ? p.W - x0 : kTile;
        const int len = 3 * cols;
        uint8_t *dst = out + (int64_t)f * p.frame_bytes + ((int64_t)(y0 + row) * p.W + x0) * 3;
        const int first = 4 * slot - (int)((uintptr_t)dst & 3);       // (lead + len <= 51: slots 0..12 cover the row)
        const uint8_t *src = tile_bytes + row * kRowBytes;
        if (first >= 0 && first + 4 <= len) {
            *reinterpret_cast<uint32_t *>(dst + first) = (uint32_t)src[first] | ((uint32_t)src[first + 1] << 8) |
                                                         ((uint32_t)src[first + 2] << 16) | ((uint32_t)src[first + 3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (first + j >= 0 && first + j < len) dst[first + j] = src[first + j];
        }
    }
}

struct ScatterGeometry {
    int32_t px0, py0, pw, ph, bar_x, bar_w;
};

// where the plot area and the colour bar lie on a canvas; false with a message when the canvas or the radius is bad
static bool scatter_geometry(const char *who, int width, int height, int radius, ScatterGeometry *g) {
    if (width <= 0 || height <= 0 || width >= 32768 || height >= 32768) {
        fail(ARVAE_E_INVALID, "%s: a canvas of %d x %d pixels (both in [1, 32768))", who, width, height);
        return false;
    }
    g->px0 = kLeft;
    g->py0 = kTop;
    g->pw = width - kLeft - kBarGap - kRight;
    g->ph = height - kTop - kBottom;
    g->bar_x = kLeft + g->pw + kBarGap;
    g->bar_w = kBarW;
    if (g->pw < kMinPlot || g->ph < kMinPlot) {
        fail(ARVAE_E_INVALID, "%s: a canvas of %d x %d pixels leaves a plot area of %d x %d beside the margins (at least %d x %d)", who,
             width, height, g->pw, g->ph, kMinPlot, kMinPlot);
        return false;
    }
    if (radius < 1 || radius > 64) {
        fail(ARVAE_E_INVALID, "%s: radius %d outside [1, 64]", who, radius);
        return false;
    }
    if ((int64_t)width * height * 3 >= ((int64_t)1 << 31)) {
        fail(ARVAE_E_INVALID, "%s: a figure of %d x %d pixels has 2^31 bytes or more", who, width, height);
        return false;
    }
    return true;
}

}  // namespace arvae

using namespace arvae;

extern "C" int64_t arvae_render_scatter_bytes(int32_t width, int32_t height, int32_t radius, int32_t *geometry) {
    ScatterGeometry g;
    if (!scatter_geometry("render_scatter_bytes", width, height, radius, &g)) return -1;
    if (geometry) {
        const int32_t v[6] = {g.px0, g.py0, g.pw, g.ph, g.bar_x, g.bar_w};
        for (int i = 0; i < 6; ++i) geometry[i] = v[i];
    }
    return (int64_t)width * height * 3;
}

extern "C" int arvae_render_scatter(const float *points, const float *values, int32_t F, int64_t N, const float *limits, int32_t width,
                                    int32_t height, int32_t radius, int32_t alpha256, const arvae_scatter_mark_t *marks,
                                    int32_t n_marks, uint8_t *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(limits && out && (N == 0 || (points && values)) && (n_marks == 0 || marks), "render_scatter: null pointer");
    ARVAE_REQUIRE(F >= 1 && F <= ARVAE_SCATTER_MAX_FIGURES, "render_scatter: %d figures outside [1, %d]", F, ARVAE_SCATTER_MAX_FIGURES);
    ARVAE_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "render_scatter: %lld points a figure outside [0, 2^31)", (long long)N);
    ARVAE_REQUIRE((((uintptr_t)points & 7) | ((uintptr_t)values & 3)) == 0, "render_scatter: points must be 8-byte, values 4-byte aligned");
    ARVAE_REQUIRE(alpha256 >= 0 && alpha256 <= 256, "render_scatter: alpha %d / 256 outside [0, 1]", alpha256);
    ARVAE_REQUIRE(n_marks >= 0 && n_marks <= ARVAE_SCATTER_MAX_MARKS, "render_scatter: %d marks outside the table's capacity [0, %d]", n_marks,
                  ARVAE_SCATTER_MAX_MARKS);
    ScatterParams p;
    ScatterGeometry g;
    if (!scatter_geometry("render_scatter", width, height, radius, &g)) return ARVAE_E_INVALID;
    for (int f = 0; f < F; ++f) {
        const float *l = limits + 6 * f;
        for (int a = 0; a < 2; ++a) {
            const float lo = l[2 * a], hi = l[2 * a + 1];
            ARVAE_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo),
                          "render_scatter: figure %d: %s limits %g and %g (finite, lo < hi)", f, a ? "y" : "x", (double)lo, (double)hi);
        }
        ARVAE_REQUIRE(std::isfinite(l[4]) && std::isfinite(l[5]) && l[4] <= l[5] && std::isfinite(l[5] - l[4]),
                      "render_scatter: figure %d: vmin %g and vmax %g must be finite and ordered", f, (double)l[4], (double)l[5]);
        // (one division and one subtraction each, rounded to fp32: numpy's float32 gives the same bits)
        p.fig[f].xlo = l[0];
        p.fig[f].kx = (float)(16 * g.pw) / (l[1] - l[0]);
        p.fig[f].ylo = l[2];
        p.fig[f].ky = (float)(16 * g.ph) / (l[3] - l[2]);
        p.fig[f].vmin = l[4];
        p.fig[f].vden = l[5] - l[4];
    }
    for (int f = F; f < ARVAE_SCATTER_MAX_FIGURES; ++f) p.fig[f] = ScatterFigure{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int m = 0; m < ARVAE_SCATTER_MAX_MARKS; ++m) {
        if (m >= n_marks) {
            p.marks[m] = arvae_scatter_mark_t{0, 0, 0, 0, 0};
            continue;
        }
        const arvae_scatter_mark_t mk = marks[m];
        ARVAE_REQUIRE(mk.glyph <= ARVAE_SCATTER_TICK_Y && mk.rot <= 1 && (mk.rot == 0 || mk.glyph < ARVAE_SCATTER_GLYPHS),
                      "render_scatter: mark %d: glyph %d, turned %d", m, mk.glyph, mk.rot);
        ARVAE_REQUIRE(mk.figure >= -1 && mk.figure < F, "render_scatter: mark %d belongs to figure %d of %d (-1: all)", m, mk.figure, F);
        int w, h;
        mark_cell(mk.glyph, mk.rot, w, h);
        ARVAE_REQUIRE(mk.x >= 0 && mk.y >= 0 && mk.x + w <= width && mk.y + h <= height,
                      "render_scatter: mark %d at (%d, %d) does not lie on the canvas of %d x %d", m, mk.x, mk.y, width, height);
        p.marks[m] = mk;
    }
    p.n = N;
    p.frame_bytes = (uint32_t)((int64_t)width * height * 3);
    p.W = width;
    p.H = height;
    p.px0 = g.px0;
    p.py0 = g.py0;
    p.pw = g.pw;
    p.ph = g.ph;
    p.bar_x = g.bar_x;
    p.bar_w = g.bar_w;
    p.tiles_x = (width + kTile - 1) / kTile;
    p.r16 = 16 * radius;
    p.alpha = alpha256;
    p.n_marks = n_marks;
    const int tiles_y = (height + kTile - 1) / kTile;
    ARVAE_LAUNCH(render_scatter_kernel, dim3((unsigned)(p.tiles_x * tiles_y), (unsigned)F), dim3(256), 0, as_stream(stream), p,
                 reinterpret_cast<const float2 *>(points), values, out);
    return check_launch("render_scatter");
}
