// Loss-term pieces (losses.hip): per-block partial sums of the reconstruction terms and the regulariser, and the finishing step.
#pragma once
#include "common.h"
#include "attributes.h"
#include "regloss.h"
#include "vae_finish.h"

namespace arvae {

// per-block partial sums of the reconstruction term (+ d/dlogits); the block count through *nb_out
int recon_partial_blocks(int64_t count);
int recon_partials(const float *logits, const float *x, int64_t count, int64_t batch, int32_t dist, float *ws,
                   float *dlogits, hipStream_t s, int *nb_out);
// the token term: rows in the tick RNN's sequence order against the score's (batch, tick) targets
int token_recon_blocks(int64_t rows);
int token_recon_partials(const float *weights, const int64_t *score, int batch, int beats, int tpb, int32_t vocab, float *ws,
                         float *dweights, hipStream_t s, int *nb_out, const AttrArgs *attr);
// per-row partial sums of the all-pairs regulariser into ws = [row_loss | row_grad]; park / park_dst: a deferred finishing step's
// arguments for this launch to store in the workspace (vae_finish.h), or null
int reg_partials(const float *z_rows, const float *lab_rows, int64_t n_rows, const float *z_cols, const float *lab_cols,
                 int64_t n_cols, int64_t ldz, int64_t ldl, const RegDims &rd, int32_t r, float delta, float *ws,
                 hipStream_t s, const VaeFinishArgs *park = nullptr, VaeFinishArgs *park_dst = nullptr);
VaeFinishArgs vae_finish_args(const float *rec_partial, int nb, int64_t batch, int64_t pix, const float *mu, const float *sigma,
                              int64_t zdim, float beta, const float *cap, const float *reg_ws, int64_t n_cols, int64_t ldz,
                              const int32_t *dims, int32_t r, float gamma, float delta, float reg_scale, float *dz, float *rec_out,
                              float *kld_out, float *reg_out, float *scalars, int64_t rec_rows);
int vae_finish(const float *rec_partial, int nb, int64_t batch, int64_t pix, const float *mu, const float *sigma,
               int64_t zdim, float beta, const float *cap, const float *reg_ws, int64_t n_cols, int64_t ldz,
               const int32_t *dims, int32_t r, float gamma, float delta, float reg_scale, float *dz, float *rec_out,
               float *kld_out, float *reg_out, float *scalars, hipStream_t s, int64_t rec_rows = 0);

}  // namespace arvae
