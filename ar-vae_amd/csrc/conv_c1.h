// Host entry points of the single-channel 64x64 image links (conv_c1.hip): the first encoder and the last decoder layer of the
// dSprites stack, and the 64-channel stride-1 ones of the Morpho-MNIST stack (conv_c1w_*).
#pragma once
#include "common.h"
#include "reduce.h"
#include "midprep.h"
#include "vae_finish.h"

namespace arvae {

bool conv_c1_fits(const arvae_link_t *l);
int conv_c1_down(const arvae_link_t *l, const Operand &img, const float *wt, const float *bias, int relu,
                 const float *gate, const uint16_t *gate_bits, uint16_t *bits_out, float *out, hipStream_t s, unsigned *amax_out);
// conv_c1_down (plain input, no gate) with the step's weight preparation riding in the same grid
int conv_c1_down_with_prep(const arvae_link_t *l, const Operand &img, const float *wt, const float *bias, int relu, uint16_t *bits_out,
                           float *out, const float *const *prep_wts, float *const *preps, int n_prep, const MidPrepArgs &mid,
                           hipStream_t s, unsigned *amax_out);
int conv_c1_up(const arvae_link_t *l, const float *lo, const float *wt, const float *bias, float *out, hipStream_t s);
// the same link with the reconstruction term fused in: logits -> out, per-workgroup (loss, correct) partial sums ->
// partial[2 * nb], d loss / d logits -> dlogits (may be null); *nb_out = conv_c1_up_recon_blocks(l).  fin / fin_dst: the
// finishing step's arguments to park in the workspace for the backward pass (vae_finish.h), or null
int conv_c1_up_recon_blocks(const arvae_link_t *l);
int conv_c1_up_recon(const arvae_link_t *l, const float *lo, const float *wt, const float *bias, float *out, const float *x,
                     int dist, float *partial, float *dlogits, hipStream_t s, int *nb_out, const VaeFinishArgs *fin = nullptr,
                     VaeFinishArgs *fin_dst = nullptr);
// a parked finishing step as a launch of its own
int vae_finish_deferred(const VaeFinishArgs *fin_dev, hipStream_t s);

// weight gradient: workgroups (= slabs) of the partial-sum launch, its workspace, and the launch with / without the reduction
int wgrad_c1_groups(const arvae_link_t *l);
int64_t conv_c1_wgrad_ws_floats(const arvae_link_t *l);
int conv_c1_wgrad(const arvae_link_t *l, const Operand &lo, const Operand &img, float *dwt, float *dbias, int bias_mode,
                  float *slab, hipStream_t s);
int conv_c1_wgrad_partial(const arvae_link_t *l, const Operand &lo, const Operand &img, float *dwt, float *dbias,
                          int bias_mode, float *slab, hipStream_t s, SlabJob *job);
// gated data gradient of the forward-UP link + its weight-gradient partials in one launch; finish: a parked finishing step
// (device pointer) that rides in it as one more workgroup, or null
bool conv_c1_pair_fits(const arvae_link_t *l);
int conv_c1_pair(const arvae_link_t *l, const Operand &g_img, const float *wt, const float *gate, const uint16_t *gate_bits, float *d_lo,
                 const Operand &w_lo, float *dwt, float *dbias, int bias_mode, float *slab, hipStream_t s, SlabJob *job,
                 unsigned *amax_out, const VaeFinishArgs *finish = nullptr);

bool conv_c1w_fits(const arvae_link_t *l);
int64_t conv_c1w_wgrad_ws_floats(const arvae_link_t *l);
int conv_c1w_wgrad(const arvae_link_t *l, const Operand &lo, const Operand &img, float *dwt, float *dbias, int bias_mode,
                   float *slab, hipStream_t s);

}  // namespace arvae
