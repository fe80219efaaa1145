// Tiles of the split-bf16 ("x3") MFMA GEMM kernels: an fp32 operand is carried as three bf16 terms (splitmath.h: split3) in
// three LDS planes, and a multiply-add is six partial products on v_mfma_f32_32x32x16_bf16 (X3_MFMA6: fp32-accurate, 2.7x fewer
// MFMA cycles than the fp32 MFMA).  Shared by dense.hip (rows GEMM) and conv64.hip.  This file is the tile GEOMETRY only.
#pragma once
#include "common.h"
#include "splitmath.h"

namespace arvae {

constexpr int RG_R = 32;                     // reduction indices per chunk
enum { RG_ROWSK = 0, RG_KROWS = 1 };         // operand memory order: reduction index contiguous / output index contiguous

constexpr int RG_XP = RG_R + 8;              // bf16 row pitch of the split planes (16 bytes of padding)
constexpr int RG_TRP = 96;                   // bf16 row pitch of a "K x rows" image (64 columns + padding: 192 bytes)

// A matrix [rows][K] as bf16 planes in memory for the wide tile GEMMs (dense.hip WidePlanes): TILED [K / 32][rows][32] -- the
// (32 reduction indices) x (all rows) block of one chunk is contiguous, whichever axis a product reduces along.  Element index
// of (row, k) inside a plane:
__host__ __device__ __forceinline__ int64_t x3_tiled_index(int64_t rows, int64_t row, int64_t k) { return ((k >> 5) * rows + row) * 32 + (k & 31); }

// One operand tile (TP output indices x RG_R reduction indices) as three bf16 planes.
//   "rows x K" (RG_ROWSK): [TP][RG_XP], reduction index contiguous; the MFMA operand (8 consecutive r per lane) is one
//   ds_read_b128.   "K x rows" (RG_KROWS): memory order kept, [RG_R][RG_TRP] with the output index contiguous (one 8-byte
//   write per plane) and read through ds_read_b64_tr_b16, the transposing read; the 192-byte row pitch puts the four rows
//   of a transposed block on disjoint banks.
template <int LAY, int TP>
struct X3Plane {
    // row pitch of a "K x rows" image: TP columns + padding that keeps the four rows of a transposed block on disjoint bank
    // quarters (192 bytes for 64 columns, 320 for 128: both 16 banks past a multiple of 32)
    static constexpr int TRP = (LAY == RG_KROWS && TP > 64) ? TP + 32 : RG_TRP;
    static constexpr int PLANE = LAY == RG_ROWSK ? TP * RG_XP : RG_R * TRP;
    // element idx of the tile's float4 grid (TP * RG_R / 4 of them): 4 values consecutive along the contiguous axis
    __device__ static __forceinline__ void commit(unsigned short *lds, int idx, const float4 &v) {
        const Split3x4 t = split3_x4(v);         // (before the address: splitmath.h)
        unsigned short *d;
        if (LAY == RG_ROWSK) d = lds + (idx / (RG_R / 4)) * RG_XP + 4 * (idx % (RG_R / 4));
        else d = lds + (idx / (TP / 4)) * TRP + 4 * (idx % (TP / 4));
        store_split3_x4(d, PLANE, t);
    }
    // this lane's MFMA operand (8 consecutive reduction indices 16 s + 8 (lane >> 5) .. of output index 32 w + (lane & 31))
    // of plane t; `base` = lane_base(w)
    __device__ static __forceinline__ int lane_base(int w) {
        const int lane = threadIdx.x & 63;
        if (LAY == RG_ROWSK) return (32 * w + (lane & 31)) * RG_XP + 8 * (lane >> 5);
        const int g16 = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;      // block row q, columns 4 pp .. 4 pp + 3
        return (8 * (g16 >> 1) + q) * TRP + 32 * w + 16 * (g16 & 1) + 4 * pp;
    }
    __device__ static __forceinline__ bf16x8 operand(const unsigned short *lds, int base, int t, int s) {
        if (LAY == RG_ROWSK) return lds_x8<bf16x8>(lds + t * PLANE + base + 16 * s);
        const unsigned short *p = lds + t * PLANE + base + 16 * s * TRP;
        return lds_tr_x8<bf16x8>(p, p + 4 * TRP);
    }
};

}  // namespace arvae
