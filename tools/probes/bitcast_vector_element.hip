// Probe: __builtin_bit_cast of an ELEMENT of an ext-vector value.  key_cast casts q[j] directly, key_copy casts a scalar copy.
// Compile to assembly and compare the two kernels:
//     hipcc --offload-arch=gfx950 -O3 -S --offload-device-only tools/probes/bitcast_vector_element.hip -o -
// With the compiler this repository is built with, key_cast takes the magnitude bits of element 0 for every j (its four selects all
// read the first register of the loaded vector), key_copy those of element j.  tick_filtered_pick (csrc/tick_decoder.hip) copies.
#include <hip/hip_runtime.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void key_cast(const f32x4 *in, int *out) {
    const f32x4 q = in[threadIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * threadIdx.x + j] = q[j] >= 0.f ? (__builtin_bit_cast(int, q[j]) & 0x7fffffff) : -1;
}

__global__ void key_copy(const f32x4 *in, int *out) {
    const f32x4 q = in[threadIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = q[j];
        out[4 * threadIdx.x + j] = v >= 0.f ? (__builtin_bit_cast(int, v) & 0x7fffffff) : -1;
    }
}
