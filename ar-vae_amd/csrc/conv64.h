// Host entry points of the wide stride-1 convolutions (conv64.hip: the gathering kernels and the weight gradient; conv64s.hip:
// the row-staged kernel of the 64 <-> 64 channel layers and its split weights).
#pragma once
#include "common.h"

namespace arvae {

// links conv64.hip serves: k x k (<= 16 taps), stride 1, 32 | channels on the reduction side, channels-last, no permutation
bool conv64_fits(const arvae_link_t *l, bool up);
int64_t conv64_ws_floats(const arvae_link_t *l);
// lo = act(conv(hi) + bias) * mask (Conv2d forward / ConvTranspose2d data gradient) and hi = act(convT(lo) + bias) * mask.
// amax_in / amax_out: AMAX arrays (amax.h) of a plain source / of the result, or null; prepped: the layer's split
// weights (conv64s_prep_batch on this stream, this step), or null
int conv64_down(const arvae_link_t *l, const Operand &hi, const float *wt, const float *bias, int act, const uint8_t *mask,
                float *lo, float *ws, hipStream_t s, const GateOp *gate, const unsigned *amax_in = nullptr, unsigned *amax_out = nullptr,
                float *prepped = nullptr);
int conv64_up(const arvae_link_t *l, const Operand &lo, const float *wt, const float *bias, int act, const uint8_t *mask,
              float *hi, float *ws, hipStream_t s, const GateOp *gate, const unsigned *amax_in = nullptr, unsigned *amax_out = nullptr,
              float *prepped = nullptr);
bool conv64_wgrad_fits(const arvae_link_t *l);
int64_t conv64_wgrad_ws_floats(const arvae_link_t *l);
int conv64_wgrad(const arvae_link_t *l, const Operand &lo, const Operand &hi, float *dwt, float *ws, hipStream_t s,
                 const unsigned *amax_lo, const unsigned *amax_hi, float *dbias, int bias_side, bool *bias_done);

// conv64s.hip.  AMAX array of an operand as multiplied (count floats, a multiple of 4)
int conv64_operand_amax(const Operand &x, int64_t count, unsigned *out, hipStream_t s);
// 64 source channels, 64 or 4..32 (a multiple of 4) output channels, 4x4 taps, stride 1, channels-last without permutation
bool conv64s_fits(const arvae_link_t *l, bool up);
int64_t conv64s_ws_floats();
int conv64s_prep_batch(const float *const *wts, float *const *outs, const int *transposed, const int *q, int count, hipStream_t s);
// src [n][sh][sw][64] -> out [n][oh][ow][q]; source coordinate = output coordinate + sgn * k + off
int conv64s_run(const Operand &src, int n, int sh, int sw, int oh, int ow, int q, int sgn, int off, const float *wt, bool transposed,
                const float *bias, int act, const uint8_t *mask, float *out, float *ws, hipStream_t s, const char *what, const GateOp *gate,
                const unsigned *amax_in, unsigned *amax_out, bool prepped);

}  // namespace arvae
