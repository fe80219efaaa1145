// What the whole-model executor (plan.hip) reaches in link_gemm.hip besides the C-ABI link entry points (include/arvae_hip.h).
#pragma once
#include "common.h"

namespace arvae {

// data gradient of ConvTranspose2d(64 -> 1) with the producing layer's activation derivative / keep-mask in the epilogue
bool single_channel_down_gated_fits(const arvae_link_t *l);
int single_channel_down_gated(const arvae_link_t *link, const Operand &hi, const float *wt, const GateOp *gate, float *lo, hipStream_t s,
                              unsigned *amax_out);
// the forward form (bias, activation, keep-mask), with the result's maxima published
bool single_channel_down_fits(const arvae_link_t *l);
int single_channel_down(const arvae_link_t *link, const Operand &hi, const float *wt, const float *bias, int act, const uint8_t *mask,
                        float *lo, hipStream_t s, unsigned *amax_out);
// weight + bias gradients of a wide stride-1 link (conv64.h); amax_*: AMAX arrays of the operands when the caller has them
// (plain operands only), else null
int link_wgrad_conv64(const arvae_link_t *link, const Operand &lo, const Operand &hi, float *dwt, float *dbias, int bias_side, float *ws,
                      hipStream_t st, const unsigned *amax_lo, const unsigned *amax_hi);

}  // namespace arvae
