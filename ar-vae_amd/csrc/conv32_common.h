// Shared geometry of the 32-channel conv kernels (conv32.hip and its headers): LDS pitches, tiles, the epilogue record, raw
// buffer access and the prepared-weight layout.  Their arithmetic -- the scaled two-term fp16 split -- is splitmath.h, the
// per-tensor maxima that scale it amax.h.
#pragma once
#include "common.h"
#include "splitmath.h"
#include "amax.h"

#include <type_traits>

namespace arvae {

constexpr int C32 = 32;
constexpr int PSB2 = 36;                // LDS pixel stride in dwords of the packed two-term image (terms at +0, +16 dwords, 4 pad):
                                        // conflict-free 16-byte reads for pixel walks of stride 1 and 2 (eight lanes per clock:
                                        // 36 rc and 72 rc mod 64 are eight disjoint groups of four banks)
constexpr int PSB = 20;                 // LDS pixel stride in dwords of one 16-bit plane (16 payload + 4 pad: conflict-free
                                        // 16-byte reads for pixel walks of stride 1 and 2)
constexpr int WGRAD_PSB_H = 24, WGRAD_PSB_L = 16;   // plane pitches of wgrad32x_kernel (see there)
constexpr int PIXB = C32 * 4;           // bytes of one 32-channel pixel
constexpr unsigned OOB = 0x7fffffffu;   // byte offset beyond any tensor here: loads return 0, stores are dropped

// tile geometry per lo-resolution size LO (hi = 2*LO): PX lo pixels = PX/32 MFMA tiles of full-width rows (TC == LO):
//   LO 16, PX 128: 8 rows of one image      LO 8, PX 128: two whole images      LO 4, PX 128: eight whole images
//   LO 4, PX 32: two whole images (the small-problem variant: 4x more tiles when 128-pixel tiles leave CUs idle)
template <int LO, int PX = 128> struct Tile {
    static constexpr int ROWS = PX / LO;
    static constexpr int TI = ROWS > LO ? ROWS / LO : 1, TR = ROWS > LO ? LO : ROWS, TC = LO;
};

// lo pixel p of a tile -> (image, row, col) inside the tile; in memory pixel p sits p*PIXB after the tile start
template <int LO, int PX = 128> __device__ __forceinline__ constexpr void tile_pixel(int p, int &img, int &r, int &c) {
    using T = Tile<LO, PX>;
    c = p % T::TC;
    r = (p / T::TC) % T::TR;
    img = p / (T::TC * T::TR);
}
template <int LO, int PX = 128> __device__ __forceinline__ void tile_origin(int tile, int &img0, int &r0) {
    using T = Tile<LO, PX>;
    constexpr int TILES_PER_IMG = LO / T::TR;
    img0 = (T::TI == 1) ? tile / TILES_PER_IMG : tile * T::TI;
    r0 = (T::TI == 1) ? (tile % TILES_PER_IMG) * T::TR : 0;
}
// compile-time loop: f(std::integral_constant<int, I>) for I in [0, N); keeps every register-array index static
template <int I, int N, class F> __device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// epilogue modes (one template parameter: a ReLU layer is never gated and vice versa)
enum { EP_PLAIN = 0, EP_RELU = 1, EP_GATE_F = 2, EP_GATE_B = 3 };
struct Ep32 {
    const float *bias;          // per output channel or null
    const float *gate;          // EP_GATE_F: saved activation of the OUTPUT location: result *= (gate > 0)
    const uint16_t *gate_bits;  // EP_GATE_B: the same as sign bits (common.h: relu_bits16)
    uint16_t *bits_out;         // EP_RELU: sign bits of the result for a later gated kernel, may be null
    float *out;
    const uint4 *wprep;         // this layer's weights split and laid out per lane (conv32_prep_block), with their inverse scale
    const unsigned *amax_in;    // AMAX array of the input tensor
    unsigned *amax_out;         // AMAX array of `out`, or null (nobody multiplies it on the matrix pipe)
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void buf_store4(float4 v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    f32x4 q;
    q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, q), r, (int)off, 0, 0);
}

__device__ __forceinline__ unsigned buf_load_u16(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, (int)off, 0, 0);
}
__device__ __forceinline__ void buf_store_u16(unsigned v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, r, (int)off, 0, 0);
}

// Per-layer prepared weights (conv32_prep_block, prep32.h, once per training step): the scaled two-term split of wt in per-lane
// MFMA operand order, 16 bytes per (slot, lane) with lanes contiguous, followed by the inverse of the layer's weight scale.
//   DOWN part: [kh 2][slot 32 = (tap 8 = kyl*4 + kx, c 2, term 2)][lane 64], ky = 2 kh + kyl: lane (rc, half) holds the input
//              channels c*16 + half*8 + j of wt[clo = rc][.][ky][kx]
//   UP part:   [class 4][slot 16 = (ty, tx, c, term)][lane 64]
//   tail:      one uint4 whose first dword is the inverse weight scale (float)
constexpr int PREP_DOWN_SLOTS = 32, PREP_UP_SLOTS = 16;
constexpr int PREP_DOWN_UINT4 = 2 * PREP_DOWN_SLOTS * 64, PREP_UP_UINT4 = 4 * PREP_UP_SLOTS * 64;
constexpr int PREP_FLOATS = (PREP_DOWN_UINT4 + PREP_UP_UINT4 + 1) * 4;
__device__ __forceinline__ float prep_inv_scale(const uint4 *wprep) {
    return __builtin_bit_cast(float, wprep[PREP_DOWN_UINT4 + PREP_UP_UINT4].x);
}

// byte offset of a lane's (pixel, half) entry in a relu_bits16 array, from its byte offset pixel*128 + half*16
__device__ __forceinline__ unsigned bits_off(unsigned out_off, int half) { return (out_off >> 7) * 4 + half * 2; }

}  // namespace arvae
