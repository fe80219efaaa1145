// Figures of the image models: decoder outputs -> the bytes of image grids (latent-traversal GIF frames, PNG grids) in one launch.
// sigmoid, torchvision's make_grid and .mul(255).clamp(0, 255).byte() in one pass over the OUTPUT: a frame is a flat byte array
// [Hg][Wg][C]; a thread produces four consecutive bytes and decodes for each its (frame, y, x) to a cell of the grid or to padding.
#include "common.h"

namespace arvae {

struct RenderGeom {
    int64_t n_images, total;       // source images; bytes of all frames
    uint32_t frame_bytes;          // Hg * Wg * C < 2^31
    uint32_t h, w, padding, cells_per_frame, xmaps;
    uint32_t lead;                 // bytes between the 4-byte boundary below `out` and `out` (0..3)
    uint32_t pad_byte;
    int32_t flags;
    FastDiv by_row, by_chan, by_cell_h, by_cell_w;      // Wg * C, C, h + padding, w + padding
};

__device__ __forceinline__ uint32_t quantise(float v, int32_t flags) {
    if (flags & ARVAE_RENDER_SRC_LOGITS) v = __fdiv_rn(1.f, 1.f + expf(-v));      // exactly 1 from 20 on: expf(-20) < 2^-24
    float t = __fmul_rn(255.f, v);                       // (no fused multiply-add: the product is rounded as torch's mul is)
    if (flags & ARVAE_RENDER_ROUND) t = __fadd_rn(t, 0.5f);
    return (uint32_t)fminf(fmaxf(t, 0.f), 255.f);        // (a NaN clamps to 0)
}

// byte r of frame f
__device__ __forceinline__ uint32_t render_byte(const RenderGeom &g, const float *__restrict__ src, const int32_t *__restrict__ cells,
                                                int64_t f, uint32_t r) {
    uint32_t y, in_row;
    g.by_row.divmod(r, y, in_row);
    const uint32_t x = g.by_chan.div(in_row);
    if (y < g.padding || x < g.padding) return g.pad_byte;
    uint32_t cy, iy, cx, ix;
    g.by_cell_h.divmod(y - g.padding, cy, iy);
    g.by_cell_w.divmod(x - g.padding, cx, ix);           // (cx < xmaps: x - padding < xmaps (w + padding))
    if (iy >= g.h || ix >= g.w) return g.pad_byte;
    const uint32_t k = cy * g.xmaps + cx;
    if (k >= g.cells_per_frame) return g.pad_byte;       // ragged last row
    const int32_t img = cells[f * g.cells_per_frame + k];
    if (img < 0 || (int64_t)img >= g.n_images) return g.pad_byte;
    return quantise(src[((int64_t)img * g.h + iy) * g.w + ix], g.flags);
}

// word i covers the bytes [4 i - lead, 4 i - lead + 4) of the output: whole words leave as one aligned dword store, the
// words cut by the output's first or last byte as byte stores
__global__ __launch_bounds__(256) void render_frames_kernel(RenderGeom g, const float *__restrict__ src, const int32_t *__restrict__ cells,
                                                            uint8_t *__restrict__ out, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) {
        const int64_t first = i * 4 - g.lead;
        const int64_t lo = first < 0 ? 0 : first;
        int64_t f = lo / g.frame_bytes;
        uint32_t r = (uint32_t)(lo - f * g.frame_bytes);
        uint32_t word = 0, b = 0;
        bool have = false;                  // b is byte r - 1 of the same frame
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t at = first + j;
            if (at < 0 || at >= g.total) continue;
            // the three channels of a pixel are equal: byte r repeats byte r - 1 unless it starts a pixel (rows are whole pixels)
            if (!(have && g.by_chan.d == 3 && r % 3 != 0)) b = render_byte(g, src, cells, f, r);
            have = true;
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

// Hg, Wg and the frame's bytes; false with a message when an argument is bad or the frame has 2^31 bytes or more
static bool frame_geometry(const char *who, int h, int w, int cells_per_frame, int nrow, int padding, int channels, int64_t *hg,
                           int64_t *wg, int64_t *xmaps_out, int64_t *bytes) {
    if (h <= 0 || w <= 0 || cells_per_frame <= 0 || nrow <= 0 || padding < 0) {
        fail(ARVAE_E_INVALID, "%s: h %d, w %d, cells_per_frame %d and nrow %d must be positive, padding %d not negative", who, h, w,
             cells_per_frame, nrow, padding);
        return false;
    }
    if (channels != 1 && channels != 3) {
        fail(ARVAE_E_INVALID, "%s: %d channels (1 or 3)", who, channels);
        return false;
    }
    const int64_t xmaps = nrow < cells_per_frame ? nrow : cells_per_frame;
    const int64_t ymaps = (cells_per_frame + xmaps - 1) / xmaps;
    const int64_t big = (int64_t)1 << 31;
    *hg = ymaps * ((int64_t)h + padding) + padding;      // each below 2^31 * 2^32
    *wg = xmaps * ((int64_t)w + padding) + padding;
    *xmaps_out = xmaps;
    if (*hg >= big || *wg * channels >= big || *hg * (*wg * channels) >= big) {
        fail(ARVAE_E_INVALID, "%s: a frame of %lld x %lld x %d has 2^31 bytes or more", who, (long long)*hg, (long long)*wg, channels);
        return false;
    }
    *bytes = *hg * *wg * channels;
    return true;
}

}  // namespace arvae

using namespace arvae;

extern "C" int64_t arvae_render_frame_bytes(int h, int w, int cells_per_frame, int nrow, int padding, int channels) {
    int64_t hg, wg, xmaps, bytes;
    return frame_geometry("render_frame_bytes", h, w, cells_per_frame, nrow, padding, channels, &hg, &wg, &xmaps, &bytes) ? bytes : -1;
}

extern "C" int arvae_render_frames(const float *src, int64_t n_images, int h, int w, const int32_t *cells, int n_frames,
                                   int cells_per_frame, int nrow, int padding, float pad_value, int flags, uint8_t *out,
                                   arvae_stream_t stream) {
    ARVAE_REQUIRE(src && cells && out, "render_frames: null pointer");
    ARVAE_REQUIRE(n_images > 0 && n_frames > 0, "render_frames: %lld images and %d frames must be positive", (long long)n_images, n_frames);
    ARVAE_REQUIRE((flags & ~(ARVAE_RENDER_SRC_LOGITS | ARVAE_RENDER_ROUND | ARVAE_RENDER_RGB)) == 0, "render_frames: unknown flag bits in %d",
                  flags);
    ARVAE_REQUIRE((((uintptr_t)src | (uintptr_t)cells) & 3) == 0, "render_frames: src and cells must be 4-byte aligned");
    const int channels = (flags & ARVAE_RENDER_RGB) ? 3 : 1;
    int64_t hg, wg, xmaps, bytes;
    if (!frame_geometry("render_frames", h, w, cells_per_frame, nrow, padding, channels, &hg, &wg, &xmaps, &bytes)) return ARVAE_E_INVALID;

    RenderGeom g;
    g.n_images = n_images;
    g.total = bytes * n_frames;
    g.frame_bytes = (uint32_t)bytes;
    g.h = (uint32_t)h;
    g.w = (uint32_t)w;
    g.padding = (uint32_t)padding;
    g.cells_per_frame = (uint32_t)cells_per_frame;
    g.xmaps = (uint32_t)xmaps;
    g.lead = (uint32_t)((uintptr_t)out & 3);
    // the quantiser of the kernel on the host: 255 * pad_value and the sum are exact in double, so each cast rounds once
    float t = (float)(255.0 * (double)pad_value);
    if (flags & ARVAE_RENDER_ROUND) t = (float)((double)t + 0.5);
    g.pad_byte = t >= 255.f ? 255u : (t > 0.f ? (uint32_t)t : 0u);      // (a NaN gives 0, as in the kernel)
    g.flags = flags;
    g.by_row = FastDiv((uint32_t)(wg * channels));
    g.by_chan = FastDiv((uint32_t)channels);
    g.by_cell_h = FastDiv((uint32_t)(h + padding));
    g.by_cell_w = FastDiv((uint32_t)(w + padding));

    const int64_t words = (g.total + g.lead + 3) / 4;
    int64_t blocks = (words + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    ARVAE_LAUNCH(render_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), g, src, cells, out, words);
    return check_launch("render_frames");
}
