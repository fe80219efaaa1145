// AMAX: a tensor's maximum magnitude travels with it as AMAX_N partial maxima (bit patterns of non-negative floats) and fixes the
// scale of its two-term split (splitmath.h: pow2_for).
// The kernel that WRITES a tensor publishes the maxima of what its G writer units stored (unit u -> entry u, and zeros into the
// entries u + G, u + 2 G, ... no unit owns: the whole array is rewritten by every launch -- no atomics, nothing to clear, the
// same array every time a captured graph replays); the kernels that READ it take the maximum of all AMAX_N entries (4 KB, four
// 16-byte loads per lane, from L2).  G <= AMAX_N is the launcher's business.
#pragma once
#include "splitmath.h"

namespace arvae {

constexpr int AMAX_N = 1024;
__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}
// m: this lane's maximum; every lane of the wave calls
__device__ __forceinline__ void amax_publish(unsigned *p, int unit, int units, float m) {
    if (p == nullptr) return;
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && unit < AMAX_N) {              // (units <= AMAX_N is the launcher's promise; never write past the array)
        p[unit] = __builtin_bit_cast(unsigned, m);
        for (int e = unit + units; e < AMAX_N; e += units) p[e] = 0u;
    }
}
__device__ __forceinline__ float amax4(const float4 &v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
// Reading one: the loads are issued FIRST in a kernel (amax_issue) -- memory returns loads in order, so whatever is requested
// after them (several tiles of prefetch) does not stand between them and their use -- and reduced where the scale is first
// needed (amax_scale); every lane of the wave calls both, the result is wave-uniform.
struct AmaxLoad { uint4 v[AMAX_N / 256]; };
__device__ __forceinline__ AmaxLoad amax_issue(const unsigned *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p) + (threadIdx.x & 63);
    AmaxLoad a;
#pragma unroll
    for (int i = 0; i < AMAX_N / 256; ++i) a.v[i] = q[64 * i];
    return a;
}
__device__ __forceinline__ Pow2 amax_scale(const AmaxLoad &a) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < AMAX_N / 256; ++i) m = max(max(m, a.v[i].x), max(max(a.v[i].y, a.v[i].z), a.v[i].w));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    return pow2_for((unsigned)__builtin_amdgcn_readfirstlane((int)m));
}

}  // namespace arvae
