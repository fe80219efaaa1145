// Host entry points of the specialised 32-channel k4 / s2 / p1 conv kernels (conv32.hip).  Operands are plain fp32 tensors that
// come with the AMAX array of their values and the layer's prepared weights (amax.h, conv32_common.h); a per-layer caller that has
// neither makes them in its workspace (conv32_scratch_floats, conv32_weight_prep, conv32_amax).
#pragma once
#include "common.h"
#include "reduce.h"
#include "midprep.h"
#include "regloss.h"

namespace arvae {

bool conv32_fits(const arvae_link_t *l);
// gate (float activation) or gate_bits (relu_bits16) select a gated epilogue; with relu, bits_out (may be null) receives the
// sign bits of the result
int conv32_down(const arvae_link_t *l, const Operand &hi, const float *bias, int relu, const float *gate, const uint16_t *gate_bits,
                uint16_t *bits_out, float *out, hipStream_t s, const float *wprep, const unsigned *amax_in, unsigned *amax_out);
int conv32_up(const arvae_link_t *l, const Operand &lo, const float *bias, int relu, const float *gate, const uint16_t *gate_bits,
              uint16_t *bits_out, float *out, hipStream_t s, const float *wprep, const unsigned *amax_in, unsigned *amax_out);
// two stacked ReLU layers (16x16 then 8x8 output) as one launch
bool conv32_down_chain_fits(const arvae_link_t *a, const arvae_link_t *b);
int conv32_down_chain(const arvae_link_t *a, const arvae_link_t *b, const float *hi, const unsigned *amax_in, const float *bias_a,
                      uint16_t *bits_a, float *out_a, const float *wprep_a, unsigned *amax_a, const float *bias_b, uint16_t *bits_b,
                      float *out_b, const float *wprep_b, unsigned *amax_b, hipStream_t s);
// conv32_up of a 4x4 -> 8x8 ReLU layer with the regulariser's workgroups riding in the same grid
bool conv32_up_reg_fits(const arvae_link_t *l);
int conv32_up_reg(const arvae_link_t *l, const Operand &lo, const float *bias, uint16_t *bits_out, float *out, const float *wprep,
                  const unsigned *amax_in, unsigned *amax_out, const RegArgs &reg, int r, hipStream_t s);

// floats of workspace per layer for conv32_weight_prep (up to 8 layers per launch); floats of scratch a caller WITHOUT prepared
// weights and maxima needs for one call
int64_t conv32_prep_floats();
int64_t conv32_scratch_floats();
int conv32_weight_prep(const float *const *wts, float *const *preps, int n_layers, hipStream_t s);
// the same together with the latent block's layout prep (midblock.h mid_prep_args): one launch
int conv32_weight_prep_with_mid(const float *const *wts, float *const *preps, int n_layers, const MidPrepArgs &mid, hipStream_t s);
// AMAX array of a plain tensor of `count` floats (a multiple of 4, 16-byte aligned)
int conv32_amax(const float *x, int64_t count, unsigned *out, hipStream_t s);

// weight gradient.  bias_mode: 0 none, 1 dbias[clo] += sum lo, 2 dbias[chi] += sum hi.  _partial leaves per-workgroup partial
// sums in `slab` and returns the reduction that finishes the layer as *job
int64_t conv32_wgrad_ws_floats(const arvae_link_t *l);
int conv32_wgrad(const arvae_link_t *l, const Operand &lo, const Operand &hi, float *dwt, float *dbias, int bias_mode,
                 float *slab, hipStream_t s, const unsigned *amax_lo, const unsigned *amax_hi);
int conv32_wgrad_partial(const arvae_link_t *l, const Operand &lo, const Operand &hi, float *dwt, float *dbias, int bias_mode,
                         float *slab, hipStream_t s, SlabJob *job, const unsigned *amax_lo, const unsigned *amax_hi);
// gated data gradient and weight-gradient partials in one launch.  c1_img / c1_slab / c1_job (all or none, conv32_pair_c1_fits):
// the single-channel first layer's weight gradient comes out of this launch too and the data gradient is NOT stored
bool conv32_pair_fits(const arvae_link_t *l, bool up, const float *gate, const uint16_t *gate_bits, int bias_mode);
bool conv32_pair_c1_fits(const arvae_link_t *l, bool up, const uint16_t *gate_bits);
int conv32_pair(const arvae_link_t *l, bool up, const float *g, const float *x_in, const float *gate, const uint16_t *gate_bits,
                float *d_in, const float *wprep, float *dwt, float *dbias, float *slab, hipStream_t s, SlabJob *job,
                const unsigned *amax_g, const unsigned *amax_x, unsigned *amax_out, const float *c1_img, float *c1_slab, SlabJob *c1_job);

}  // namespace arvae
