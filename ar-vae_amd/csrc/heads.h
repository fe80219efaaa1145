// Fused encoder heads + reparameterisation (heads.hip).
#pragma once
#include "common.h"

namespace arvae {

// both heads are plain Linear layers on the same hidden vector, small enough for the fused kernels
bool heads_fusable(const arvae_layer_t *hm, const arvae_layer_t *hl, int zdim);
// the decoder's first layer can ride in the heads kernels: a plain Linear layer on z, no dropout
bool heads_next_fusable(const arvae_layer_t *l, int zdim);
int heads_latent_fwd(const arvae_layer_t *hm, const arvae_layer_t *hl, int batch, int zdim, const float *params,
                     const float *hidden, const float *eps, float *mu, float *log_std, float *sigma, float *z, hipStream_t s,
                     const arvae_image_vae_t *rng_model = nullptr, const arvae_layer_t *next = nullptr, float *next_out = nullptr);
int heads_latent_bwd(const arvae_layer_t *hm, const arvae_layer_t *hl, int batch, int zdim, const float *params,
                     const float *g_z, const float *dz_reg, const float *dz_extra, const float *mu, const float *sigma,
                     const float *eps, const float *g_loss, const float *kl, const float *cap, float beta, float reg_scale,
                     const float *gate, float *d_mu, float *d_ls, float *d_hidden, hipStream_t s, const arvae_layer_t *next = nullptr,
                     const float *next_g = nullptr);

}  // namespace arvae
