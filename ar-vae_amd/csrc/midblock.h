// The latent block (trailing Linear layers of the encoder, heads + reparameterisation, leading Linear layers of the decoder) as
// one launch per pass (midblock.hip), optionally with the conv layers on either side of it (MidFold, midprep.h).
#pragma once
#include "common.h"
#include "midprep.h"

namespace arvae {

// trailing Linear layers of the encoder / leading Linear layers of the decoder that the block covers (false: block not usable)
bool mid_fusable(const arvae_image_vae_t *m, int *ne_out, int *nd_out);
// floats of workspace for the prepped matrices of the block's layers, and the prep launch's arguments alone (plan.hip hands them
// to the launch that also splits the 32-channel conv weights)
int64_t mid_prep_floats(const arvae_image_vae_t *m);
void mid_prep_args(const arvae_image_vae_t *m, const float *params, float *prep_ws, MidPrepArgs *out, int batch);
// split-reduction workspace of the wide layers' tile GEMMs
int64_t mid_wide_ws_floats(const arvae_image_vae_t *m, int batch);
// the conv layers on either side of the block computed by its clustered kernels; floats of weight-gradient slabs each needs
bool mid_fold_fits(const arvae_image_vae_t *m, int batch);
int64_t mid_fold_slab_floats(const arvae_image_vae_t *m, int batch);
// (1) weight layout prep unless prep_done, (2) the forward block.  enc_y / dec_y: saved outputs of the block's layers.
int mid_forward(const arvae_image_vae_t *m, int batch, const float *params, float *prep_ws, const float *x0, float *const *enc_y,
                float *const *dec_y, const float *eps, float *mu, float *log_std, float *sigma, float *z, hipStream_t s, bool prep_done,
                unsigned *amax_out, const MidFold *fold, float *wide_ws);
int mid_backward(const arvae_image_vae_t *m, int batch, const float *params, float *prep_ws, float *const *enc_y, float *const *dec_y,
                 float *const *enc_g, float *const *dec_g, const float *g_out, int g_is_pre, const float *gate0, float *d_x0,
                 const float *eps, const float *mu, const float *sigma, const float *dz_reg, const float *dz_extra, const float *g_loss,
                 const float *kl, const float *cap, float beta, float reg_scale, float *d_mu, float *d_ls, hipStream_t s,
                 unsigned *amax_out, const MidFold *fold, float *wide_ws);
// the wide layers' weight gradients, called behind mid_backward.  *took: bit 0 / 1 = the first encoder / last decoder layer was
// done here (the caller keeps them out of the grouped launch)
int mid_wide_wgrad(const arvae_image_vae_t *m, int batch, const float *params, float *prep_ws, float *wide_ws, const float *x0,
                   const float *g_last_pre, float *grads, hipStream_t s, int *took);

}  // namespace arvae
