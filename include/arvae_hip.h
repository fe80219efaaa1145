/* arvae_hip.h -- C-ABI of libarvae_hip.so, the MI355X (gfx950) AR-VAE training-path library.
 *
 * The reference (ashispati/ar-vae) has no FFI / plugin interface: its hot path is stock PyTorch ops
 * called from Python classes.  This header is therefore the boundary a
 * maintainer binds INSTEAD of those torch calls; every entry point cites the reference call site it
 * replaces (paths relative to the reference repo).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller unless the
 *    parameter is documented as "host".  The library allocates no device memory (every scratch buffer is a caller
 *    workspace whose size an arvae_*_ws_floats function reports) and no call depends on state left by another, so the
 *    forward (main thread) and backward (autograd thread) may call concurrently.  What is process-wide: the once-per-kernel
 *    registration of dynamic LDS sizes (hipFuncSetAttribute behind std::call_once), the device's CU count (queried once), the
 *    run-time binding of RCCL (arvae_comm_*) and the opt-in timeline of arvae_profile_begin/_end.  The library reads NO
 *    environment variable: its diagnostic switches exist only in the -DARVAE_DIAG build (libarvae_hip_diag.so, csrc/diag.h).
 *  - `stream` is a hipStream_t passed as void*; calls only enqueue work and never synchronise.
 *  - return value: 0 = ok, <0 = error (ARVAE_E_*); arvae_last_error_string() gives the thread-local text.
 *  - tensors are fp32, contiguous, CHANNELS-LAST: activations [N, H, W, C]; a 1-channel image
 *    [N,1,H,W] is bit-identical in both layouts.  Weights keep the reference's state_dict layouts.
 *  - "accumulates" means the kernel ADDS into the buffer (caller zeroes it: Trainer.zero_grad()).
 */
#ifndef ARVAE_HIP_H
#define ARVAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARVAE_ABI_VERSION 16  /* 16: arvae_resnet18_* (inference of the Morpho-MNIST ResNet-18 digit classifier: digit_pred_acc of imagevae/image_vae_trainer.py:319-368), and, added without a new number (symbols only), arvae_sample_filter_t, arvae_row_sample_filtered, arvae_tick_free_run_filtered, arvae_tick_free_run_layers_filtered (top-k, nucleus and note-mask sampling of the free-running decoder), and arvae_gru_seq_wide_supported / _ws_floats / arvae_gru_seq_wide_fwd / _bwd (the whole-sequence GRU recurrences at hidden sizes 256 and 512: streamed weights, one launch per time step); 15: arvae_tick_stack_t, arvae_tick_free_run_layers_supported / _ws_floats / arvae_tick_free_run_layers (the free-running tick decoder for GRU stacks of 1, 3 or 4 layers: --num_decoder_layers); 14: arvae_philox_uniform, arvae_row_sample, arvae_tick_free_run_sampled (multinomial feedback of the hierarchical decoder: measurevae/decoder.py:372,431-434,502-505); 13: arvae_wide_dense_ws_floats / arvae_wide_dense (the latent block's wide tile GEMMs as per-layer calls); 12: arvae_ksg_ws_bytes / arvae_ksg_mi (the KSG mutual-information estimator of the disentanglement metrics, fp64); 11: arvae_philox_keep_masks (several Dropout masks, one launch); arvae_adam_step(status): the update is skipped while the sticky status word is set (a pass that reported a failed hand-off never reaches the weights), ARVAE_STATUS_* re-coded so that the word survives a float SUM all-reduce beside the gradients; 10: arvae_comm_init(timeout_ms); arvae_image_vae_t.status / .flags (a sticky device status word: an in-launch hand-off between workgroups that gives up says so there instead of hanging; ARVAE_VAE_NO_CLUSTER keeps the pass on kernels without such hand-offs); 9: arvae_measure_vae_* (whole-model MeasureVAE step), row strides for h0 / dh0 / the beat embeddings (arvae_gru_seq_t, arvae_tick_*); 8: arvae_gru_seq_t.gi_rstride / dgi_rstride / h_fin (merged input projections of a bidirectional layer, final states written by the sequence launch); 7: arvae_comm_* (the data-parallel step's collectives: RCCL on the launch stream, owned by the library); 6: the 32-channel k4 s2 p1 links need caller workspace too (arvae_link_ws_floats / arvae_link_wgrad_ws_floats: the layer's weights as scaled fp16 terms and the operands' maxima); 5: arvae_adam_step(zero_grad), arvae_image_vae_finish, arvae_image_vae_t.milestones (events the executors record for the data-parallel caller's collectives); 4: arvae_philox_* and in-kernel eps (arvae_image_vae_t.rng_*), arvae_tick_free_run_supported, caller workspace for arvae_link_down/up (arvae_link_ws_floats); 3: arvae_gru_seq_*, embed_bwd workspace; 2: arvae_image_vae_backward reg_fused == 2 (unit regulariser gradient in dz_extra) */

#define ARVAE_OK 0
#define ARVAE_E_INVALID (-1)  /* bad argument (null pointer, size out of range, unsupported shape) */
#define ARVAE_E_LAUNCH (-2)   /* hipLaunch / runtime error; text in arvae_last_error_string()        */
#define ARVAE_E_NODEVICE (-3) /* no HIP device visible to this process                              */
#define ARVAE_E_COMM (-4)     /* RCCL missing or a collective / communicator call failed            */

/* activation fused into a producing kernel / differentiated in a consuming one */
#define ARVAE_ACT_NONE 0
#define ARVAE_ACT_RELU 1 /* nn.ReLU  (imagevae/dsprites_vae.py:13-46)                              */
#define ARVAE_ACT_SELU 2 /* nn.SELU  (imagevae/mnist_vae.py:17-45, measurevae/encoder.py:39-51)    */

#define ARVAE_RECON_BERNOULLI 0
#define ARVAE_RECON_GAUSSIAN 1

typedef void *arvae_stream_t;

int arvae_abi_version(void);
const char *arvae_last_error_string(void);
/* number of HIP devices visible (0 on a CPU-only host; never initialises a context) */
int arvae_device_count(void);

/* Opt-in kernel timeline for benchmarking (off by default, no cost when off): after arvae_profile_begin
 * every kernel the library launches on `stream` is followed by a HIP event on that stream; a kernel's
 * duration is the time since the previous event.  arvae_profile_end stops recording, synchronises on
 * the last event and writes one text line per kernel label: "<label>\t<launches>\t<total ms>\n";
 * it returns the buffer size needed.  Labels name the __global__ function (e.g. "up32<16>"). */
int arvae_profile_begin(arvae_stream_t stream);
int64_t arvae_profile_end(char *out, int64_t cap);

/* ------------------------------------------------------------------------------------------------
 * Strided "link" between a HI-resolution tensor hi[N,HH,HW,CHI] and a LO-resolution tensor
 * lo[N,LH,LW,CLO] through a weight wt[CLO][CHI][KH][KW]:
 *     lo(n,ly,lx,clo) <-> hi(n, ly*stride - pad + ky, lx*stride - pad + kx, chi)
 * One link serves six roles of the reference's layers:
 *   nn.Conv2d            (weight [Cout,Cin,KH,KW]: CLO=Cout, CHI=Cin)   forward = DOWN, dgrad = UP
 *   nn.ConvTranspose2d   (weight [Cin,Cout,KH,KW]: CLO=Cin,  CHI=Cout)  forward = UP,   dgrad = DOWN
 *   nn.Linear            (weight [out,in]: KH=KW=HH=HW=LH=LW=1, CLO=out, CHI=in) forward = DOWN
 * and the weight gradient of all three = WGRAD.
 * Replaces: imagevae/dsprites_vae.py:12-46, imagevae/mnist_vae.py:16-47 (layers) as executed by
 * imagevae/mnist_vae.py:59-72 (encode/decode) and their autograd backward (utils/trainer.py:140).
 *
 * hi_perm_c/hi_perm_hw (and lo_*): when >0 the channel index of that tensor is a FLATTENED NCHW
 * feature index f = c*hw + p of a [C=perm_c, HW=perm_hw] map that is stored channels-last, i.e. it
 * lives at memory channel p*perm_c + c.  This is how `hidden.view(B,-1)` (mnist_vae.py:61) and
 * `.view(B,-1,inter,inter)` (mnist_vae.py:70) are honoured without a transpose pass.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n;
    int32_t hh, hw, chi;
    int32_t lh, lw, clo;
    int32_t kh, kw, stride, pad;
    int32_t hi_perm_c, hi_perm_hw;
    int32_t lo_perm_c, lo_perm_hw;
} arvae_link_t;

/* An operand read by a kernel.  Plain tensor: y = mask = NULL.  Gradient operand: the value used is
 *   v * act'(y) * (mask ? 2*mask : 1)
 * where y is the SAVED OUTPUT of the layer that produced the tensor v is the gradient of (act' is
 * evaluated from the output: ReLU y>0; SELU y>0 ? scale : y + scale*alpha; with dropout the saved
 * output is act(.)*2*mask so act' is taken at y/2) and mask the uint8 keep-mask of nn.Dropout(0.5). */
typedef struct {
    const float *v;
    const float *y;
    const uint8_t *mask;
    int32_t act;
} arvae_operand_t;

/* Floats of caller workspace arvae_link_down / arvae_link_up need for this link (0 for most geometries; the wide stride-1
 * convolutions re-order their weights to [out channel][tap][in channel] there before the product; the 32-channel k4 s2 p1
 * links split their weights into scaled fp16 terms there and keep the input's per-workgroup maxima).  Independent of n. */
int64_t arvae_link_ws_floats(const arvae_link_t *link);

/* lo = epilogue( sum_{ky,kx,chi} hi * wt + bias[clo] );  epilogue = act, then *2*out_mask if given.
 * bias may be NULL.  ws: arvae_link_ws_floats(link) floats, 16-byte aligned (may be NULL when that is 0); its contents are
 * scratch of this call only. */
int arvae_link_down(const arvae_link_t *link, const arvae_operand_t *hi, const float *wt,
                    const float *bias, int32_t out_act, const uint8_t *out_mask, float *lo, float *ws,
                    arvae_stream_t stream);

/* hi = epilogue( sum_{ky,kx,clo} lo * wt + bias[chi] ), the adjoint map of arvae_link_down. */
int arvae_link_up(const arvae_link_t *link, const arvae_operand_t *lo, const float *wt,
                  const float *bias, int32_t out_act, const uint8_t *out_mask, float *hi, float *ws,
                  arvae_stream_t stream);

/* dwt[clo][chi][ky][kx] += sum_{n,ly,lx} lo * hi   (accumulates).  The batch is split over workgroups;
 * partial tiles go to `ws` (arvae_link_wgrad_ws_floats(link) floats, may be 0 -> ws unused) and are summed
 * in a fixed order: bitwise reproducible, no float atomics.
 * The bias gradient rides along: bias_side 1: dbias[clo] += sum_pixels lo (nn.Conv2d / nn.Linear, whose
 * output is the lo tensor); 2: dbias[chi] += sum_pixels hi (nn.ConvTranspose2d); 0: none (dbias unused). */
int64_t arvae_link_wgrad_ws_floats(const arvae_link_t *link);
int arvae_link_wgrad(const arvae_link_t *link, const arvae_operand_t *lo, const arvae_operand_t *hi,
                     float *dwt, float *dbias, int32_t bias_side, float *ws, arvae_stream_t stream);

/* out[c] += sum_rows operand[row, c]  for a [rows, channels] channels-last view (bias gradients).
 * perm_c/perm_hw as in arvae_link_t (out is indexed by the flattened NCHW feature).
 * ws: arvae_channel_sum_ws_floats(rows, channels) floats. */
int64_t arvae_channel_sum_ws_floats(int64_t rows, int32_t channels);
int arvae_channel_sum(const arvae_operand_t *g, int64_t rows, int32_t channels, int32_t perm_c,
                      int32_t perm_hw, float *out, float *ws, arvae_stream_t stream);

/* Weight (and bias) gradients of several nn.Linear layers in one launch: dw[n_out][n_in] += g^T x, dbias += column sums
 * of g (NULL: skip), g = the layer's output gradient as an operand (activation derivative / keep-mask folded in). */
typedef struct arvae_dense_wgrad_job {
    arvae_operand_t g;        /* [rows][n_out] */
    const float *x;           /* [rows][n_in] layer input */
    float *dw;                /* accumulated */
    float *dbias;             /* accumulated, or NULL */
    int32_t rows, n_in, n_out, reserved;
} arvae_dense_wgrad_job_t;
int arvae_dense_wgrad_batch(const arvae_dense_wgrad_job_t *jobs, int32_t njobs, arvae_stream_t stream);

/* out[i] = value of the operand with act'(y) and the keep-mask folded in: a plain copy of a gradient operand. */
int arvae_operand_apply(const arvae_operand_t *g, int64_t count, float *out, arvae_stream_t stream);

/* One product of a WIDE nn.Linear layer (one side >= 1024 features, the other a multiple of 32; link->n rows) on the three-term
 * bf16 tile kernels the whole-model executor's latent block uses for it, with nothing of the block around it (tests, profiling):
 *   mode 0: out[n][clo] = x . W^T (+ bias)    mode 1: out[n][chi] = g . W    mode 2: dw += g^T x, dbias += column sums of g (or NULL)
 * x [n][chi], g [n][clo], out in channels-last memory order under the link's permutations; w [clo][chi], dw in feature order.
 * The product whose reduction runs over the wide side is a split reduction whose consumer adds the bias: bias must be NULL there.
 * ws: arvae_wide_dense_ws_floats() floats, 16-byte aligned. */
int64_t arvae_wide_dense_ws_floats(const arvae_link_t *link);
int arvae_wide_dense(const arvae_link_t *link, int32_t mode, const float *x, const float *g, const float *w, const float *bias,
                     float *out, float *dw, float *dbias, float *ws, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Latent head.  Replaces z_dist = Normal(mu, exp(log_std)); z = z_dist.rsample()
 * (imagevae/mnist_vae.py:65,74-87; measurevae/encoder.py:123, measure_vae.py:115-123) with the noise
 * eps as an explicit input:  sigma = exp(log_std),  z = mu + eps * sigma.
 * ------------------------------------------------------------------------------------------------ */
int arvae_latent_fwd(const float *mu, const float *log_std, const float *eps, int64_t count,
                     float *sigma, float *z, arvae_stream_t stream);
/* d_mu += ... is NOT accumulated: d_mu = g_z, d_log_std = (g_z*eps + g_sigma)*sigma (g_sigma may be NULL) */
int arvae_latent_bwd(const float *g_z, const float *g_sigma, const float *eps, const float *sigma,
                     int64_t count, float *d_mu, float *d_log_std, arvae_stream_t stream);

/* beta-KL term.  Replaces Trainer.compute_kld_loss (utils/trainer.py:354-367):
 *   kl = mean_b sum_z 0.5*((s/s0)^2 + ((mu-m0)/s0)^2 - 1 - log((s/s0)^2));  out[0] = beta*|kl - c|,
 *   out[1] = kl.  prior_mu/prior_sigma NULL = standard normal.  `capacity` is a 1-element device
 *   tensor (the reference keeps c as a tensor: image_vae_trainer.py:94) or NULL for c = 0.
 * bwd: d_mu, d_sigma = g[0] * d out[0] / d(mu, sigma)  (g is a 1-element device tensor). */
int arvae_kld_fwd(const float *mu, const float *sigma, const float *prior_mu, const float *prior_sigma,
                  int64_t batch, int64_t zdim, float beta, const float *capacity, float *out,
                  arvae_stream_t stream);
int arvae_kld_bwd(const float *g, const float *mu, const float *sigma, const float *prior_mu,
                  const float *prior_sigma, int64_t batch, int64_t zdim, float beta, const float *kl_out,
                  const float *capacity, float *d_mu, float *d_sigma, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attribute-regularisation loss over all pairs.  Replaces the per-dimension Python loop
 * (imagevae/image_vae_trainer.py:171-180, measurevae/measure_vae_trainer.py:135-139) over
 * Trainer.compute_reg_loss / reg_loss_sign (utils/trainer.py:369-403), all R dims in one launch:
 *   loss = sum_r gamma/NC^2 * sum_{i in rows, j in cols} | tanh(delta*(z_i - z_j)) - sign(a_i - a_j) |
 *   dz[i, dims[r]] = 2*gamma*delta/NC^2 * sum_j (1 - t_ij^2) * sgn(t_ij - s_ij)      (other columns 0)
 * Rows are this rank's samples, cols the (all-gathered) global batch; single GPU: cols == rows.
 * dims: HOST array of R DISTINCT latent/label column indices (z[:,d] pairs with labels[:,d]); an index listed twice is
 * ARVAE_E_INVALID here and as a model's reg_dims (dz has one entry per column: the second share would be lost).
 * ws: device scratch of arvae_reg_loss_ws_floats(n_rows, R) floats.  loss_out: 1 float.
 * dz: [n_rows, ldz] fully written (gradient for unit upstream gradient), may be NULL.
 * ------------------------------------------------------------------------------------------------ */
int64_t arvae_reg_loss_ws_floats(int64_t n_rows, int32_t r);
int arvae_reg_loss(const float *z_rows, const float *lab_rows, int64_t n_rows, const float *z_cols,
                   const float *lab_cols, int64_t n_cols, int64_t ldz, int64_t ldl, const int32_t *dims,
                   int32_t r, float gamma, float delta, float *ws, float *loss_out, float *dz,
                   arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction terms.
 * Image: replaces ImageVAETrainer.reconstruction_loss + mean_accuracy
 * (imagevae/image_vae_trainer.py:623-655).  out[0] = sum_all(term)/batch, out[1] = pixel accuracy.
 * dlogits (optional) = d out[0] / d logits.  ws: arvae_recon_ws_floats(count) floats.
 * ------------------------------------------------------------------------------------------------ */
int64_t arvae_recon_ws_floats(int64_t count);
int arvae_image_recon(const float *logits, const float *x, int64_t count, int64_t batch, int32_t dist,
                      float *ws, float *out, float *dlogits, arvae_stream_t stream);

/* Measure: replaces Trainer.mean_crossentropy_loss + Trainer.mean_accuracy
 * (utils/trainer.py:247-282) on [rows, V] ReLU-ed logits and int64 targets.
 * out[0] = mean CE, out[1] = top-1 accuracy (lowest index on ties).  dweights optional. */
int arvae_token_recon(const float *weights, const int64_t *targets, int64_t rows, int32_t vocab,
                      float *ws, float *out, float *dweights, arvae_stream_t stream);

/* y[i] = g[0] * x[i]   (chain rule through a scalar loss term) */
int arvae_scale_by_scalar(const float *g, const float *x, int64_t count, float *y, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Adam over one flat fp32 arena.  Replaces torch.optim.Adam(...).step() (utils/trainer.py:31-34,
 * 170-174) with defaults beta1=.9 beta2=.999 eps=1e-8, no weight decay, no amsgrad:
 *   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * Hyper-parameters are doubles (as torch holds them: 1-beta2 is formed in double, then rounded).
 * `step` is the 1-based step number t.  grad_scale multiplies g first (1/world_size after a SUM
 * all-reduce; 1 otherwise).  zero_grad != 0: g is cleared once it has been consumed, i.e. the update and the NEXT
 * step's Trainer.zero_grad() (utils/trainer.py:136) are one kernel.
 * status (optional, NULL: none): device words the caller owns.  status[0] is the sticky status word of the passes that
 * produced g (arvae_image_vae_t.status, ARVAE_STATUS_*); while it is non-zero the launch changes NOTHING in p, m, v -- the
 * gradient of a pass whose in-launch hand-off gave up is undefined and must not reach the weights (the reference would have
 * raised at its per-step host read of the loss, utils/trainer.py:145-147; this build reads the word once per epoch) -- it
 * still clears g when zero_grad is set, and adds one to status[4], the count of skipped updates: the caller that finally
 * reads the word takes that many steps back off its step counter, so the bias corrections continue where the last
 * APPLIED update left them.
 * ------------------------------------------------------------------------------------------------ */
int arvae_adam_step(float *p, float *g, float *m, float *v, int64_t count, int64_t step, double lr, double beta1,
                    double beta2, double eps, float grad_scale, int32_t zero_grad, uint32_t *status,
                    arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MeasureVAE building blocks (GRU encoder / hierarchical GRU decoder over 24-tick measures).
 * The GEMMs of nn.GRU (W_ih x and W_hh h, measurevae/encoder.py:27-34,115; decoder.py:338-368,504) run on
 * arvae_link_down with a dense link; these are the non-GEMM pieces.
 * ------------------------------------------------------------------------------------------------ */
/* GRU gate math of one time step.  gi = W_ih x + b_ih, gh = W_hh h + b_hh as [batch, 3*hidden] (gates r|z|n);
 * h_prev [batch, hidden] or NULL (zeros).  saved (optional, for the backward): 4*batch*hidden floats (r, z, n, gh_n). */
int arvae_gru_gates_fwd(const float *gi, const float *gh, const float *h_prev, int32_t batch, int32_t hidden,
                        float *h_new, float *saved, arvae_stream_t stream);
/* dh = d/d h_new.  Writes dgi, dgh [batch, 3*hidden] and dh_prev = dh * z (the direct path; the caller adds W_hh^T dgh). */
int arvae_gru_gates_bwd(const float *dh, const float *saved, const float *h_prev, int32_t batch, int32_t hidden,
                        float *dgi, float *dgh, float *dh_prev, arvae_stream_t stream);

/* Whole-sequence GRU layer: all `steps` time steps of one nn.GRU layer (measurevae/encoder.py:27-34,113-118 two-layer
 * bidirectional over 24 ticks; measurevae/decoder.py:338-368 beat RNN, :436-525 tick RNN) in one launch, forward and
 * backward-through-time.  `gi` holds the input projections W_ih x + b_ih of every step (one dense launch beforehand);
 * the recurrence h -> W_hh h + b_hh -> gates runs inside the kernel, 16 batch rows per workgroup with W_hh in registers.
 * Up to 4 independent parameter sets / directions per launch (e.g. the forward and reverse directions of a layer).
 * Built for hidden sizes 32, 64 and 128 (arvae_gru_seq_supported); the per-step kernels above serve any other size. */
typedef struct arvae_gru_seq {
    const float *gi;      /* [steps][rows][3*hidden], gi_tstride floats between steps (0: one block reused every step) */
    int64_t gi_tstride;
    const float *w_hh;    /* [3*hidden][hidden] */
    const float *b_hh;    /* [3*hidden] */
    const float *h0;      /* [rows][hidden] or NULL (zeros) */
    float *h_all;         /* output: h of (step t, row r) at h_all[(t*rows + r) * h_stride + 0..hidden) */
    int64_t h_stride;
    float *saved;         /* [steps][rows][hidden][4] (layout private to the kernels): written by fwd, read by bwd */
    int32_t reverse;      /* process t = steps-1 .. 0 (the `_reverse` direction of a bidirectional layer) */
    int32_t reserved;
    const float *dh_all;  /* bwd: gradient w.r.t. h_all, addressed like h_all with dh_stride; NULL = zeros */
    int64_t dh_stride;
    float *dgi;           /* bwd out: [steps][rows][3*hidden] gradient w.r.t. gi */
    float *dgh;           /* bwd out: [steps][rows][3*hidden] gradient w.r.t. W_hh h + b_hh */
    float *dh0;           /* bwd out: [rows][hidden] gradient w.r.t. h0, or NULL */
    const float *dh_last; /* bwd: gradient w.r.t. the final state (h_n of nn.GRU: h of the last processed step), row r at
                             dh_last + r*dh_last_stride; NULL = zeros */
    int64_t dh_last_stride;
    float *h_prev_out;    /* bwd out, optional: [steps][rows][hidden], the state entering each step (operand of dW_hh) */
    /* both directions of a bidirectional layer share ONE input projection [steps][rows][2 * 3*hidden] (measurevae/encoder.py:27-34:
     * nn.GRU applies W_ih of both directions to the same input): floats between two rows of gi / of dgi; 0 = 3*hidden */
    int64_t gi_rstride, dgi_rstride;
    float *h_fin;         /* fwd out, optional: the state after the last processed step (nn.GRU's h_n), row r at h_fin + r*h_fin_stride */
    int64_t h_fin_stride;
    /* floats between two rows of h0 / of dh0; 0 = hidden.  Lets the initial states be column blocks of the Linear layer's output that
     * makes them (measurevae/decoder.py:388-406 view(B, 2, H)) and their gradients column blocks of that layer's output gradient */
    int64_t h0_stride, dh0_stride;
} arvae_gru_seq_t;
int arvae_gru_seq_supported(int32_t hidden);
int arvae_gru_seq_fwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden,
                      arvae_stream_t stream);
int arvae_gru_seq_bwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden,
                      arvae_stream_t stream);

/* The same recurrences at the hidden sizes the resident-weights kernels above are not built for: 256 and 512
 * (arvae_gru_seq_wide_supported; MeasureVAE's own default is a 512-wide encoder and decoder).  W_hh is streamed from memory
 * every step, and a call issues ONE LAUNCH PER TIME STEP on `stream` (the backward one more when any sequence has dh0): a step
 * needs every unit of the previous state, and no kernel waits for another workgroup.  Descriptor, outputs and the layout of
 * `saved` are those of arvae_gru_seq_fwd / _bwd; arrays are addressed with 64-bit offsets (no 2 GB limit).  w_hh, h_all, h0,
 * saved and dgh must be 16-byte aligned, h_stride and h0_stride multiples of 4 floats.
 * ws: arvae_gru_seq_wide_ws_floats(nseq, rows, hidden) floats of caller scratch, 16-byte aligned, contents irrelevant on entry
 * (-1: bad arguments); both calls take it, the backward carries the state's gradient between its launches in it.
 * The calls neither allocate nor synchronise nor read back: a captured graph can hold them.  Results are bit-identical
 * from run to run (no float atomics). */
int arvae_gru_seq_wide_supported(int32_t hidden);
int64_t arvae_gru_seq_wide_ws_floats(int32_t nseq, int32_t rows, int32_t hidden);
int arvae_gru_seq_wide_fwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden, float *ws,
                           arvae_stream_t stream);
int arvae_gru_seq_wide_bwd(const arvae_gru_seq_t *seqs, int32_t nseq, int32_t steps, int32_t rows, int32_t hidden, float *ws,
                           arvae_stream_t stream);

/* Free-running pass of the tick decoder (measurevae/decoder.py:459-525 without teacher forcing): 2-layer GRU, note
 * projection + ReLU, top-1 note (lowest index on ties) embedded as the next input, hidden state restarted from
 * h0_l0 / h0_l1 [beats*batch][hidden] (row = beat*batch + b) at every beat.  One launch, returns only the tokens
 * [batch][beats*ticks_per_beat]; the caller evaluates the differentiable graph on them with arvae_gru_seq_*.
 * The layer-0 input projection arrives pre-multiplied: gib [beats*batch][3*hidden] = W_ih0[:, E:] beat_emb + b_ih0 and
 * ptab [vocab+1][3*hidden] = W_ih0[:, :E] applied to the embedding table, row `vocab` = the learned start vector x_0.
 * mask: optional keep-mask [beats*ticks_per_beat][batch][hidden] of nn.GRU's inter-layer dropout, scaled by keep_scale.
 * ws: arvae_tick_free_run_ws_floats(hidden) floats, 16-byte aligned, required (the recurrent weights re-laid out for streaming). */
typedef struct arvae_tick_weights {
    const float *w_hh0, *b_hh0;     /* rnn_tick layer 0 recurrent weights */
    const float *w_ih1, *b_ih1, *w_hh1, *b_hh1;   /* layer 1 */
    const float *w_out, *b_out;     /* tick_emb_to_note_emb [vocab][hidden] */
} arvae_tick_weights_t;
int64_t arvae_tick_free_run_ws_floats(int32_t hidden);
/* 1 when arvae_tick_free_run is built for this (hidden, vocab): hidden in {32, 64, 128} and vocab <= min(64, 16*(hidden/16));
 * otherwise the caller runs the decoder tick by tick (arvae_gru_gates_fwd + arvae_row_argmax), as the reference does
 * (measurevae/decoder.py:469-525). */
int arvae_tick_free_run_supported(int32_t hidden, int32_t vocab);
int arvae_tick_free_run(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1, int64_t h0_stride /* 0 = hidden */,
                        const float *gib,
                        const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch, int32_t beats,
                        int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int64_t *tokens, float *ws,
                        arvae_stream_t stream);
/* The same pass with MULTINOMIAL feedback (decoder.sampling == 'multinomial', measurevae/decoder.py:431-434,502-505:
 * torch.multinomial(softmax(probs), 1) is the next input), the draw an explicit input: uniforms [batch][beats*ticks_per_beat] in (0, 1]
 * (arvae_philox_uniform, or the caller's own).  With l_v = relu(W_out h1 + b_out)_v, e_v = exp((l_v - max_v l_v) * inv_temperature) and
 * C_k = sum_{v <= k} e_v, the note of a row at a tick is the smallest k with C_k >= u * C_{vocab-1}; inv_temperature = 1 is the
 * reference's softmax(probs).  The total is the last prefix value itself, so a note in [0, vocab) always exists.  Needs the
 * workspace (ws == NULL: ARVAE_E_INVALID); same shapes as arvae_tick_free_run_supported. */
int arvae_tick_free_run_sampled(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1, int64_t h0_stride /* 0 = hidden */,
                                const float *gib, const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch, int32_t beats,
                                int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms, float inv_temperature,
                                int64_t *tokens, float *ws, arvae_stream_t stream);

/* The free-running pass for tick RNNs of OTHER layer counts than two (nn.GRU(num_layers = layers), measurevae/decoder.py:331-363;
 * two layers: arvae_tick_free_run above).  The same contract: gib / ptab pre-multiplied with layer 0's input weights, the states of
 * all layers restarted from h0[l] [beats*batch][hidden] (row = beat*batch + b, rows h0_stride floats apart) at every beat, the
 * note projection + ReLU on the TOP layer's state (layer 0's when layers == 1), tokens [batch][beats*ticks_per_beat] the only output.
 * mask: optional keep-masks of the layers-1 layer boundaries, [layers-1][beats*ticks_per_beat][batch][hidden], boundary (l -> l+1)
 * at index l, scaled by keep_scale (ignored when layers == 1).  uniforms NULL: the top-1 note is fed back (lowest index on ties);
 * else [batch][beats*ticks_per_beat] in (0, 1] and inv_temperature, the draw of arvae_tick_free_run_sampled.
 * w_ih[0] / b_ih[0] are not read.  ws: arvae_tick_free_run_layers_ws_floats(hidden, layers) floats, 16-byte aligned, required. */
#define ARVAE_TICK_MAX_LAYERS 4
typedef struct arvae_tick_stack {
    int32_t layers, reserved;
    const float *w_ih[ARVAE_TICK_MAX_LAYERS], *w_hh[ARVAE_TICK_MAX_LAYERS];   /* rnn_tick weight_ih_l{k} / weight_hh_l{k} [3*hidden][hidden] */
    const float *b_ih[ARVAE_TICK_MAX_LAYERS], *b_hh[ARVAE_TICK_MAX_LAYERS];
    const float *w_out, *b_out;                /* tick_emb_to_note_emb [vocab][hidden] */
    const float *h0[ARVAE_TICK_MAX_LAYERS];    /* initial states per layer */
    int64_t h0_stride;                         /* 0 = hidden */
} arvae_tick_stack_t;
/* 1 when arvae_tick_free_run_layers is offered for (hidden, vocab, layers): the shapes of arvae_tick_free_run_supported, layers in
 * {1, 3, 4}, and three or four layers only up to hidden 64; otherwise the caller runs the decoder tick by tick. */
int arvae_tick_free_run_layers_supported(int32_t hidden, int32_t vocab, int32_t layers);
int64_t arvae_tick_free_run_layers_ws_floats(int32_t hidden, int32_t layers);
int arvae_tick_free_run_layers(const arvae_tick_stack_t *stack, const float *gib, const float *ptab, const uint8_t *mask,
                               float keep_scale, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab,
                               const float *uniforms, float inv_temperature, int64_t *tokens, float *ws, arvae_stream_t stream);

/* nn.Embedding (measurevae/encoder.py:36-37,111; decoder.py:18,516): out row (b,t) = table[idx[b][t]];
 * time_major: rows ordered (t, b) instead of (b, t).  embed_bwd adds to (accumulate != 0) or overwrites dtable, in a fixed summation order, and needs
 * a workspace of arvae_embed_bwd_ws_floats() floats.  `table` may also be a per-vocabulary PROJECTION table: a Linear layer
 * applied to embedded tokens is a lookup of table W^T + b (the encoder's layer-0 input projection of both directions,
 * 768 columns at hidden 128: encoder.py:27-37,111-114 computes it per position) -- any `dim`; rows wider than 128 take a
 * column-parallel segment-sum kernel in embed_bwd (vocab * 1 KB + 256 B of LDS <= 64 KB).
 * An index outside [0, vocab) is read from, and credited to, the nearest valid row (0 or vocab - 1) in every form: forward and
 * backward, any dim, either row order; the int64 is clamped before it is narrowed.  arvae_tick_gi_fwd / _bwd clamp a fed-back
 * token the same way (row `vocab`, x_0, is reached at tick 0 only). */
int arvae_embed_fwd(const int64_t *idx, const float *table, int32_t batch, int32_t steps, int32_t dim, int32_t vocab,
                    int32_t time_major, float *out, arvae_stream_t stream);
int64_t arvae_embed_bwd_ws_floats(int32_t batch, int32_t steps, int32_t dim, int32_t vocab);
int arvae_embed_bwd(const int64_t *idx, const float *g, int32_t batch, int32_t steps, int32_t dim, int32_t vocab,
                    int32_t time_major, float *dtable, int32_t accumulate /* 0: dtable is overwritten */, float *ws,
                    arvae_stream_t stream);

/* The tick RNN's layer-0 input projection, re-associated (measurevae/decoder.py:459-505 applies W_ih0 to [embedding of the previous
 * note | beat embedding] at each of the 24 ticks x batch positions).  The note half takes vocab + 1 distinct values (the vocabulary's
 * embeddings and the learned start vector x_0), the beat half one per (beat, measure), so ONE small product G = X W_ih0^T over
 *     x_small [vocab + 1 + rows][emb + hidden] = [table | 0] (vocab rows), [x_0 | 0] (1 row), [0 | beat_emb] (rows = beats*batch)
 * (arvae_tick_rows_fwd builds it; G by arvae_link_down) gives every tick's projection as a gather:
 *     gi[(j*beats + beat)*batch + b][:] = G[prev][:] + G[vocab + 1 + beat*batch + b][:] + bias[:],
 *     prev = tokens[b][ticks_per_beat*beat + j - 1], or row `vocab` (x_0) at tick 0            (arvae_tick_gi_fwd)
 * in the row order the tick RNN's sequence launches take (arvae_gru_seq_*: ticks_per_beat steps over beats*batch rows).
 * Backward: arvae_tick_gi_bwd sums the per-tick gradients dgi into dg_small [vocab + 1 + rows][cols] (OVERWRITTEN: per previous
 * note in a fixed order, per beat row over its ticks); dx_small = dg_small W_ih0 (arvae_link_up) is split by arvae_tick_rows_bwd
 * into the table's and x_0's gradients (ADDED; either may be NULL) and the beat embedding's (written).
 * cols (= 3 * hidden of the tick RNN) must be a multiple of 4; ws: arvae_tick_gi_bwd_ws_floats(vocab, cols) floats. */
int arvae_tick_rows_fwd(const float *table, const float *x0, const float *beat_emb, int64_t beat_emb_stride /* floats between rows, 0 = hidden */,
                        int32_t vocab, int32_t emb, int32_t hidden, int32_t rows, float *x_small, arvae_stream_t stream);
int arvae_tick_rows_bwd(const float *dx_small, int32_t vocab, int32_t emb, int32_t hidden, int32_t rows, float *dtable, float *dx0,
                        float *dbeat_emb, int64_t dbeat_emb_stride /* 0 = hidden */, arvae_stream_t stream);
int arvae_tick_gi_fwd(const float *g_small, const int64_t *tokens, const float *bias, int32_t batch, int32_t beats,
                      int32_t ticks_per_beat, int32_t vocab, int32_t cols, float *gi, arvae_stream_t stream);
int64_t arvae_tick_gi_bwd_ws_floats(int32_t vocab, int32_t cols);
int arvae_tick_gi_bwd(const float *dgi, const int64_t *tokens, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t vocab,
                      int32_t cols, float *dg_small, float *ws, arvae_stream_t stream);

/* top-1 index per row, lowest index on ties (the decoder's argmax feedback, measurevae/decoder.py:506-507) */
int arvae_row_argmax(const float *w, int32_t rows, int32_t cols, int64_t *idx, arvae_stream_t stream);
/* one index per row drawn from softmax(w[r] * inv_temperature) by inverting its CDF at u[r] in (0, 1] (the decoder's multinomial
 * feedback tick by tick, measurevae/decoder.py:502-505; the semantics of arvae_tick_free_run_sampled on given logits): the smallest
 * k with C_k >= u[r] * C_{cols-1}.  Any cols >= 1; inv_temperature finite and > 0. */
int arvae_row_sample(const float *w, int32_t rows, int32_t cols, const float *u, float inv_temperature, int64_t *idx,
                     arvae_stream_t stream);


/* Filtered sampling of the free-running decoder (generation; beyond the reference): a top-k cut, a nucleus (top-p) cut and a mask of
 * the notes that may be emitted, one definition for the three entry points below.  Per row, with logits l_v (the tick kernels':
 * relu(W_out h + b_out)_v) and T = 1 / inv_temperature:
 *   allowed set A: allow[v] != 0 (allow: DEVICE pointer to vocab bytes; NULL = every note);
 *   order: the allowed notes by descending l, ties to the lower index (the argmax pick's rule); rank(v) = v's position in it;
 *   top_k in [1, vocab], 0 = off: v survives iff rank(v) < top_k;
 *   e_v = exp((l_v - max_A l) / T), S = the sum of e over the allowed notes that survive top_k;
 *   top_p in (0, 1], 1 = off: v survives iff mass_before(v) < top_p, mass_before(v) = (the sum of e_u over the notes ordered before
 *   v) / S; the first note of the order always survives;
 *   draw: arvae_tick_free_run_sampled's over the survivors in index order: C_k the running sum of e, the note is the smallest
 *   surviving k with C_k >= u * C_last.
 * A token in [0, vocab) comes back for ANY input, a mask that allows nothing included (note 0 then): "in range, no fault"; callers
 * reject such a mask themselves.  ARVAE_E_INVALID with a message: top_k outside [0, vocab], top_p not in (0, 1] or not finite, null
 * uniforms, and for the tick calls a dropout keep-mask (generation runs with dropout off: the filtered kernels are built without
 * masks).  With no filter active (top_k 0 or vocab, top_p 1, allow NULL) the calls forward to arvae_row_sample /
 * arvae_tick_free_run_sampled / arvae_tick_free_run_layers: the same tokens bit for bit.  Shapes: those of
 * arvae_tick_free_run_supported / arvae_tick_free_run_layers_supported; arvae_row_sample_filtered takes any cols >= 1 (top_k against
 * cols).  Every other argument as in the unfiltered call. */
typedef struct arvae_sample_filter {
    int32_t top_k;          /* 0 = off */
    float top_p;            /* 1 = off */
    const uint8_t *allow;   /* device, [vocab] bytes; NULL = every note */
} arvae_sample_filter_t;
int arvae_row_sample_filtered(const float *w, int32_t rows, int32_t cols, const float *u, float inv_temperature,
                              const arvae_sample_filter_t *filter, int64_t *idx, arvae_stream_t stream);
int arvae_tick_free_run_filtered(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1, int64_t h0_stride /* 0 = hidden */,
                                 const float *gib, const float *ptab, const uint8_t *mask /* must be NULL */, float keep_scale, int32_t batch,
                                 int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms,
                                 float inv_temperature, const arvae_sample_filter_t *filter, int64_t *tokens, float *ws,
                                 arvae_stream_t stream);
int arvae_tick_free_run_layers_filtered(const arvae_tick_stack_t *stack, const float *gib, const float *ptab,
                                        const uint8_t *mask /* must be NULL */, float keep_scale, int32_t batch, int32_t beats,
                                        int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms, float inv_temperature,
                                        const arvae_sample_filter_t *filter, int64_t *tokens, float *ws, arvae_stream_t stream);

/* Beam search of the free-running decoder (generation; beyond the reference): the `width` most likely measures of a latent code,
 * and the log-probability of a given measure.  One definition for the entry points below.
 *   Inputs per code: the tick RNN's inputs as for arvae_tick_free_run, width W in [1, 16], allow: DEVICE pointer to vocab bytes
 *   (NULL = every note) and `allowed` = the number of notes it allows, counted by the host (vocab when allow is NULL).  W <= allowed:
 *   otherwise fewer than W distinct hypotheses exist after tick 0 (ARVAE_E_INVALID).
 *   A beam is (score, previous note, tick-GRU states).  At tick t, for every live beam k:
 *     1. logits l = relu(W_out h + b_out), exactly as the free-running kernel forms them;
 *     2. logp_v = (l_v - M) - log(sum over allowed u of exp(l_u - M)), M = max over allowed u of l_u: the log-softmax over the
 *        allowed notes only (the renormalisation of the filtered draw);
 *     3. candidate (k, v) for allowed v: c = score_k + logp_v in fp32;
 *     4. the candidates of a code are ordered by c descending (compared as floats), ties to the lower k, then the lower v (as
 *        integers: the argmax pick's rule extended).  New beam j is the j-th candidate: beam k's states after tick t, note v as its
 *        previous note, score c.
 *   At tick 0 only beam 0 is live (score 0; the others -inf, never a parent).  At a beat's first tick every beam restarts from that
 *   beat's initial states, as the decoder does.  All hypotheses have beats*ticks_per_beat ticks: no length normalisation.
 *   Outputs: the per-tick history parents [batch][ticks][W] int32, tokens [batch][ticks][W] int64, scores_hist [batch][ticks][W];
 *   the backtracked sequences [batch][W][ticks] int64, best first, and their scores [batch][W] (the last tick's).  By construction the
 *   W sequences of a code are distinct and their scores non-increasing in j; W = 1 is the argmax free run.
 * arvae_beam_select: step 2 to 4 on given logits [codes*width][vocab] (row = code*width + k) and scores_in [codes][width], of which the
 *   first `live` beams of every code are read (1 at tick 0, width afterwards; live * allowed >= width) -> parents / notes / scores_out
 *   [codes][width].  Any vocab >= 1: the tick-by-tick path.
 * arvae_sequence_log_prob: out[r] = sum over t of logp (step 2) of weights [rows][steps][vocab] at tokens [rows][steps]; fp32, sums in a
 *   fixed order.  A token outside [0, vocab) or not allowed gives -inf.
 * arvae_tick_beam_search: the whole search in one launch, for the two-layer tick RNN at the shapes of
 *   arvae_tick_beam_search_supported(hidden, vocab, width) (those of arvae_tick_free_run_supported, every width in [1, 16]) and at most
 *   32 ticks; ws: arvae_tick_beam_search_ws_floats(hidden) floats, 16-byte aligned, required.  No keep-masks: generation runs with
 *   dropout off.  Every bad argument is refused with a message before any launch. */
int arvae_beam_select(const float *logits, const float *scores_in, int32_t codes, int32_t width, int32_t vocab, int32_t live,
                      const uint8_t *allow, int32_t allowed, int32_t *parents, int64_t *notes, float *scores_out, arvae_stream_t stream);
int arvae_sequence_log_prob(const float *weights, const int64_t *tokens, int32_t rows, int32_t steps, int32_t vocab, const uint8_t *allow,
                            float *out, arvae_stream_t stream);
int arvae_tick_beam_search_supported(int32_t hidden, int32_t vocab, int32_t width);
int64_t arvae_tick_beam_search_ws_floats(int32_t hidden);
int arvae_tick_beam_search(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1, int64_t h0_stride /* 0 = hidden */,
                           const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden,
                           int32_t vocab, int32_t width, const uint8_t *allow, int32_t allowed, int32_t *parents, int64_t *tokens,
                           float *scores_hist, int64_t *sequences, float *scores, float *ws, arvae_stream_t stream);

/* Note plans of the free-running decoder (generation; beyond the reference): an allowed-note mask per (row, tick) instead of one per
 * call, honoured by every decode mode.  One definition for the entry points below.
 *   allow: DEVICE pointer to bytes, allow[b * row_stride + t * tick_stride + v] != 0: note v may be emitted for row b at tick t.  The
 *   strides are in bytes; the dense form [batch][ticks][vocab] has tick_stride = vocab and row_stride = ticks * vocab, and 0 broadcasts
 *   (row_stride 0: one plan for every row; tick_stride 0: one mask for every tick).  Nothing else is accepted.
 *   A(b, t) = {v : allow[b, t, v] != 0}; the caller folds an `allowed` mask into the plan (filter->allow must be NULL here) and makes
 *   sure that no A(b, t) is empty (an empty one gives a note in range, no fault: the first note).
 *   Draws: arvae_sample_filter_t's rule with A(b, t) as the allowed set: the maximum, the ranks, S, mass_before and the draw are taken
 *   among the notes of A(b, t).  top_k = 1 is the plan's argmax (the allowed note with the largest logit, ties to the lower index;
 *   the draw u is then without effect).  One allowed note forces it; the forced note is what the recurrence is fed.
 *   Beam search: the candidates of code b at tick t are (k, v), v in A(b, t); logp is the log-softmax over A(b, t) (a forced tick adds
 *   exactly 0).  Fewer than W finite candidates may exist: the slots without one are DEAD -- score -inf, listed behind every finite
 *   hypothesis, never displacing one, every token they carry inside its tick's A(b, t); their parent and note are otherwise not
 *   promised.  No width <= allowed requirement.
 *   arvae_sequence_log_prob_planned: the sum over t of the log-softmax over A(r, t) at the token; a token outside A(r, t): -inf.
 * The tick-by-tick forms (arvae_row_sample_planned, arvae_beam_select_planned) take the whole plan, `ticks` (the dense row stride is
 * ticks * vocab) and the tick they serve.  ARVAE_E_INVALID with a message before any launch: a null plan or mask, a stride that is
 * neither 0 nor the dense value, a tick outside [0, ticks), filter->allow set, dropout keep-masks (generation runs with dropout off),
 * and whatever the unplanned call refuses.  Shapes: those of the unplanned calls. */
typedef struct arvae_note_plan {
    const uint8_t *allow;   /* device bytes */
    int64_t row_stride;     /* bytes between rows: ticks * vocab, or 0 = every row the same */
    int64_t tick_stride;    /* bytes between ticks: vocab, or 0 = every tick the same */
} arvae_note_plan_t;
int arvae_row_sample_planned(const float *w, int32_t rows, int32_t cols, const float *u, float inv_temperature,
                             const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan, int32_t ticks, int32_t tick, int64_t *idx,
                             arvae_stream_t stream);
int arvae_tick_free_run_planned(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1, int64_t h0_stride /* 0 = hidden */,
                                const float *gib, const float *ptab, const uint8_t *mask /* must be NULL */, float keep_scale, int32_t batch,
                                int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms,
                                float inv_temperature, const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan, int64_t *tokens,
                                float *ws, arvae_stream_t stream);
int arvae_tick_free_run_layers_planned(const arvae_tick_stack_t *stack, const float *gib, const float *ptab,
                                       const uint8_t *mask /* must be NULL */, float keep_scale, int32_t batch, int32_t beats,
                                       int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms, float inv_temperature,
                                       const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan, int64_t *tokens, float *ws,
                                       arvae_stream_t stream);
int arvae_beam_select_planned(const float *logits, const float *scores_in, int32_t codes, int32_t width, int32_t vocab, int32_t live,
                              const arvae_note_plan_t *plan, int32_t ticks, int32_t tick, int32_t *parents, int64_t *notes,
                              float *scores_out, arvae_stream_t stream);
int arvae_sequence_log_prob_planned(const float *weights, const int64_t *tokens, int32_t rows, int32_t steps, int32_t vocab,
                                    const arvae_note_plan_t *plan, float *out, arvae_stream_t stream);
int arvae_tick_beam_search_planned(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1,
                                   int64_t h0_stride /* 0 = hidden */, const float *gib, const float *ptab, int32_t batch, int32_t beats,
                                   int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int32_t width, const arvae_note_plan_t *plan,
                                   int32_t *parents, int64_t *tokens, float *scores_hist, int64_t *sequences, float *scores, float *ws,
                                   arvae_stream_t stream);

/* The free-running pass of the two-layer tick decoder at the hidden sizes of arvae_gru_seq_wide_supported (256, 512), every pick in
 * one entry point.  Inputs as for arvae_tick_free_run (gib / ptab pre-multiplied, the states restarted from h0_l0 / h0_l1 at every
 * beat), any vocab in [2, 128] (arvae_tick_free_run_wide_supported).  The weights are streamed from memory and a call issues THREE
 * LAUNCHES PER TICK on `stream` (layer 0, layer 1, logits + pick): a tick needs every unit of the tick before it, and no kernel
 * waits for another workgroup.  The call neither allocates nor synchronises nor reads back: a captured graph can hold it; results
 * are bit-identical from run to run.
 *   The pick of a (row, tick) is what the row entry points above compute on that tick's logits, bit for bit:
 *     uniforms NULL, filter NULL, plan NULL     arvae_row_argmax
 *     uniforms, filter NULL, plan NULL          arvae_row_sample at uniforms[row][tick] and inv_temperature
 *     uniforms, filter, plan NULL               arvae_row_sample_filtered (a filter that cuts nothing: arvae_row_sample)
 *     uniforms, filter, plan                    arvae_row_sample_planned at that tick; top_k = 1 is the plan's argmax
 *   mask: the keep-mask [ticks][batch][hidden] of nn.GRU's inter-layer dropout, scaled by keep_scale (the training pass's; argmax
 *   and unfiltered draws only); NULL for generation.
 *   tokens [batch][ticks] int64; logits_out: NULL, or [batch][ticks][vocab] = the logits relu(W_out h_l1 + b_out) every pick was
 *   made from.
 *   ws: arvae_tick_free_run_wide_ws_floats(batch, hidden, vocab) floats of caller scratch, 16-byte aligned, contents irrelevant on
 *   entry (-1: bad arguments): the two layers' states of the tick before and of this one, and the rows' previous notes.
 * ARVAE_E_INVALID with a message before any launch: a mask together with a filter or a plan, a filter or a plan without uniforms, an
 * inv_temperature that is not positive and finite, w_hh0 / w_ih1 / w_hh1 / w_out / h0_l0 / h0_l1 / ws not 16-byte aligned, an
 * h0_stride that is no multiple of 4 floats, and whatever arvae_row_sample_filtered / arvae_row_sample_planned refuse of a filter
 * or a plan. */
int arvae_tick_free_run_wide_supported(int32_t hidden, int32_t vocab);
int64_t arvae_tick_free_run_wide_ws_floats(int32_t batch, int32_t hidden, int32_t vocab);
int arvae_tick_free_run_wide(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1, int64_t h0_stride /* 0 = hidden */,
                             const float *gib, const float *ptab, const uint8_t *mask, float keep_scale, int32_t batch, int32_t beats,
                             int32_t ticks_per_beat, int32_t hidden, int32_t vocab, const float *uniforms, float inv_temperature,
                             const arvae_sample_filter_t *filter, const arvae_note_plan_t *plan, int64_t *tokens, float *logits_out,
                             float *ws, arvae_stream_t stream);

/* Diverse beam search of the free-running decoder (generation; beyond the reference; Vijayakumar et al. 2016): the W beams of a code
 * in G groups that are served in order at every tick, a group paying `penalty` for every earlier-group beam that has just taken the
 * same note -- a few DIFFERENT likely measures instead of the W most likely ones.  One definition for the entry points below.
 *   Inputs per code: everything arvae_tick_beam_search_planned takes (the allowed notes always as a note plan A(b, t): a uniform mask
 *   is the plan with both strides 0, "every note" a mask of vocab ones with both strides 0), width W in [1, 16], groups G with
 *   1 <= G <= W and G dividing W, penalty: a finite fp32 >= 0.
 *   Group g holds the beams g W' .. (g + 1) W' - 1, W' = W / G.  A beam carries `score` (what it is ranked by), `logp` (the sum of its
 *   notes' log-softmax), its previous note and its states.  At tick 0 only the first beam of each group is live (score 0, logp 0).
 *   At tick t the groups are served in order; for group g:
 *     1. n_v = the number of beams chosen AT THIS TICK by the groups 0 .. g - 1 of the same code that have a finite score and note v;
 *     2. the candidates are (k, v), k in group g, v in A(b, t); logp_v is the planned search's log-softmax over A(b, t);
 *     3. the key a = (score_k + logp_v) - penalty * float(n_v) in fp32, in that order, each operation rounded (no fused multiply-add);
 *     4. the group's new beams are its first W' candidates by (a descending, k ascending, v ascending); new beam j of the group takes
 *        parent k (the index within the code), note v, score = a and logp = logp_k + logp_v;
 *     5. slots without a finite candidate are dead as in the planned search -- score and logp -inf, listed last WITHIN THEIR GROUP,
 *        their tokens inside the plan, their parent inside the group -- and are never counted in n_v.
 *   Outputs: parents [batch][ticks][W] int32 (always a beam of the same group), tokens [batch][ticks][W] int64, scores_hist
 *   [batch][ticks][W] (the ranking scores); sequences [batch][W][ticks] group-major, best first within a group; scores [batch][W] (the
 *   last tick's ranking scores) and log_probs [batch][W] = log p(x | z) over the plan.
 *   Consequences: G = 1 is the planned search.  Group 0 never pays (n_v = 0 gives a = c exactly): it is the planned search of width
 *   W'.  With penalty 0 every group repeats group 0.  scores - log_probs = -penalty * (the sum over t of n_t(v_t) along the path).
 * arvae_beam_select_groups: one tick's selection on given logits [codes*W][vocab], scores_in and logp_in [codes][W] -- of every group
 *   the first `live` beams are read (1 at tick 0, W' afterwards) -> parents / notes / scores_out / logp_out [codes][W]; the whole plan,
 *   `ticks` and the tick as arvae_beam_select_planned.  Any vocab >= 1: the tick-by-tick path.
 * arvae_tick_beam_search_groups: the whole search in one launch at the shapes of arvae_tick_beam_search_groups_supported(hidden,
 *   vocab, width, groups) = those of the planned search with G dividing W; ws as arvae_tick_beam_search.
 * ARVAE_E_INVALID with a message before any launch: groups < 1 or above the width or not dividing it, a penalty that is negative or
 * not finite, a null log_probs (logp_in / logp_out), and whatever the planned call refuses. */
int arvae_beam_select_groups(const float *logits, const float *scores_in, const float *logp_in, int32_t codes, int32_t width,
                             int32_t groups, float penalty, int32_t vocab, int32_t live, const arvae_note_plan_t *plan, int32_t ticks,
                             int32_t tick, int32_t *parents, int64_t *notes, float *scores_out, float *logp_out, arvae_stream_t stream);
int arvae_tick_beam_search_groups_supported(int32_t hidden, int32_t vocab, int32_t width, int32_t groups);
int arvae_tick_beam_search_groups(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1,
                                  int64_t h0_stride /* 0 = hidden */, const float *gib, const float *ptab, int32_t batch, int32_t beats,
                                  int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int32_t width, int32_t groups, float penalty,
                                  const arvae_note_plan_t *plan, int32_t *parents, int64_t *tokens, float *scores_hist,
                                  int64_t *sequences, float *scores, float *log_probs, float *ws, arvae_stream_t stream);

/* Beam search at the hidden sizes of arvae_gru_seq_wide_supported (256, 512): the three searches above ("Beam search", "Note plans",
 * "Diverse beam search": the same inputs, outputs and meanings) for the two-layer tick RNN with streamed weights, any vocab in
 * [2, 128], every width in [1, 16], groups dividing the width (arvae_tick_beam_search_wide_supported; groups 0 or 1: not grouped),
 * any number of ticks.  One call issues FOUR LAUNCHES PER TICK on `stream` (layer 0, layer 1, logits, selection), one before the first
 * tick and one after the last: a tick needs every unit of the tick before it, and no kernel waits for another workgroup.  The call
 * neither allocates nor synchronises nor reads back: a captured graph can hold it; results are bit-identical from run to run.
 *   Rows are code * W + k.  A beam's previous states are read from its parent's row (an index in the loads: no gather, no copy); the
 *   recurrence is arvae_tick_free_run_wide's, bit for bit (W = 1 is its argmax run), and the selection of tick t is
 *   arvae_beam_select / _planned / _groups on that tick's logits, the scores (and log_probs) of the tick before (zeros at tick 0) and
 *   live = 1 at tick 0, else W (grouped: at most W / G), bit for bit.
 *   logits_out: NULL, or [batch][ticks][W][vocab] = the logits every tick's selection was made from.
 *   ws: arvae_tick_beam_search_wide_ws_floats(batch, ticks, hidden, vocab, width) floats of caller scratch, 16-byte aligned, contents
 *   irrelevant on entry (-1: bad arguments): the states of two ticks, a tick's logits and the history of the search, tick-major.
 * ARVAE_E_INVALID with a message before any launch: w_hh0 / w_ih1 / w_hh1 / w_out / h0_l0 / h0_l1 / ws not 16-byte aligned, an
 * h0_stride that is no multiple of 4 floats, and whatever the one-launch searches refuse of a width, a mask, a plan or groups. */
int arvae_tick_beam_search_wide_supported(int32_t hidden, int32_t vocab, int32_t width, int32_t groups);
int64_t arvae_tick_beam_search_wide_ws_floats(int32_t batch, int32_t ticks, int32_t hidden, int32_t vocab, int32_t width);
int arvae_tick_beam_search_wide(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1, int64_t h0_stride /* 0 = hidden */,
                                const float *gib, const float *ptab, int32_t batch, int32_t beats, int32_t ticks_per_beat, int32_t hidden,
                                int32_t vocab, int32_t width, const uint8_t *allow, int32_t allowed, int32_t *parents, int64_t *tokens,
                                float *scores_hist, int64_t *sequences, float *scores, float *logits_out, float *ws,
                                arvae_stream_t stream);
int arvae_tick_beam_search_wide_planned(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1,
                                        int64_t h0_stride /* 0 = hidden */, const float *gib, const float *ptab, int32_t batch,
                                        int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int32_t width,
                                        const arvae_note_plan_t *plan, int32_t *parents, int64_t *tokens, float *scores_hist,
                                        int64_t *sequences, float *scores, float *logits_out, float *ws, arvae_stream_t stream);
int arvae_tick_beam_search_wide_groups(const arvae_tick_weights_t *weights, const float *h0_l0, const float *h0_l1,
                                       int64_t h0_stride /* 0 = hidden */, const float *gib, const float *ptab, int32_t batch,
                                       int32_t beats, int32_t ticks_per_beat, int32_t hidden, int32_t vocab, int32_t width, int32_t groups,
                                       float penalty, const arvae_note_plan_t *plan, int32_t *parents, int64_t *tokens,
                                       float *scores_hist, int64_t *sequences, float *scores, float *log_probs, float *logits_out,
                                       float *ws, arvae_stream_t stream);

/* out[r] = [a[r] | b[r]] (torch.cat along dim 1/2, decoder.py:503) and its adjoint (db optionally accumulated) */
int arvae_concat_cols(const float *a, const float *b, int64_t rows, int32_t ca, int32_t cb, float *out,
                      arvae_stream_t stream);
int arvae_split_cols(const float *g, int64_t rows, int32_t ca, int32_t cb, float *da, float *db, int32_t accumulate_b,
                     arvae_stream_t stream);

/* y = alpha * x * mask (mask NULL = 1), optionally added to y: inter-layer GRU dropout and gradient sums */
int arvae_scale_mask(const float *x, const uint8_t *mask, float alpha, int64_t count, int32_t accumulate, float *y,
                     arvae_stream_t stream);
/* y[r][:] = v[:]  (the learned start vectors x_0 / b_0 expanded over the batch, decoder.py:459-463,485-489) */
int arvae_broadcast_rows(const float *v, int64_t rows, int32_t cols, float *y, arvae_stream_t stream);

/* Minibatch assembly from a device-resident uint8 image set: out[b][:] = scale * src[idx[b]][:] as fp32.
 * Replaces the host-side float32 copy of the whole dSprites / MNIST set and the DataLoader's per-batch H2D copy
 * (data/dataloaders/dsprites_dataset.py:38-53 `images.astype('float32')`, mnist_dataset.py:60-82 `/ 255.0`).
 * src [n_rows, row_elems] uint8 (row_elems % 4 == 0), idx [count] int64 row numbers (out-of-range rows give zeros). */
int arvae_gather_rows_u8(const uint8_t *src, int64_t n_rows, int64_t row_elems, const int64_t *idx, int64_t count,
                         float scale, float *out, arvae_stream_t stream);

/* Figures of the image models (added under ABI 16: symbols only).  One launch turns decoder outputs into the bytes of
 * n_frames image grids: sigmoid, grid assembly and the cast to bytes in one pass.  Replaces torch.sigmoid +
 * torchvision.utils.make_grid + .mul(255).clamp(0, 255).byte().permute(1, 2, 0) of create_latent_gifs, and the save_image
 * calls of the plot_latent_* methods (imagevae/image_vae_trainer.py:405-552).
 *   src    [n_images, h, w] fp32
 *   cells  [n_frames, cells_per_frame] int32: the source image of every cell of every frame; -1 (or any index outside
 *          [0, n_images)) leaves the cell blank, i.e. filled with the pad value
 *   out    [n_frames, Hg, Wg, C] uint8 (what PIL.Image.fromarray takes), any alignment; C = 3 with ARVAE_RENDER_RGB, else 1
 * Grid geometry of make_grid: xmaps = min(nrow, cells_per_frame), ymaps = ceil(cells_per_frame / xmaps),
 * Hg = ymaps (h + padding) + padding, Wg = xmaps (w + padding) + padding; cell k's top-left corner is
 * (padding + (k / xmaps)(h + padding), padding + (k % xmaps)(w + padding)); the cells of a ragged last row are pad.
 * flags:
 *   ARVAE_RENDER_SRC_LOGITS  v = 1 / (1 + expf(-src)) (exactly 1 from src = 20 on); otherwise v = src
 *   ARVAE_RENDER_ROUND       byte = floor(255 v + 0.5) clamped to [0, 255] (save_image); otherwise 255 v clamped and truncated
 *                            (the .byte() of the GIF code).  Product and sum are rounded to fp32 one after the other.
 *   ARVAE_RENDER_RGB         three equal channels (make_grid's expansion of a 1-channel image)
 * The pad byte is the same quantiser applied to pad_value.
 * arvae_render_frame_bytes: Hg * Wg * channels, or -1 (bad argument, channels outside {1, 3}, or 2^31 bytes and more:
 * such a frame cannot be rendered). */
#define ARVAE_RENDER_SRC_LOGITS 1
#define ARVAE_RENDER_ROUND 2
#define ARVAE_RENDER_RGB 4
int64_t arvae_render_frame_bytes(int h, int w, int cells_per_frame, int nrow, int padding, int channels);
int arvae_render_frames(const float *src, int64_t n_images, int h, int w, const int32_t *cells, int n_frames,
                        int cells_per_frame, int nrow, int padding, float pad_value, int flags, uint8_t *out,
                        arvae_stream_t stream);

/* Decoded measures as note events and as piano-roll figures (added under ABI 16: symbols only; csrc/pianoroll.hip).  Integer
 * restatement of tensor_to_m21score / concatenate_scores (data/dataloaders/bar_dataset.py:224-268) and of the shaded roll of
 * plot_pianoroll_from_midi (utils/plotting.py:307-362).  Time is counted in twelfths of a quarter note: tick t of a measure lies in
 * beat t / 6 at sub-position s = t % 6, starts at twelfth 12 (t / 6) + {0, 3, 4, 6, 8, 9}[s] and lasts {3, 1, 2, 2, 1, 3}[s]; a measure
 * of T ticks (T % 6 == 0) has 2 T twelfths.  An element begins at every tick whose token is not `slur` and lasts to the next such
 * tick or the measure's end; leading slurs are silence, nothing ties across measures, an element sounds only where is_note marks
 * its token, and a token outside [0, V) is silence and indexes no table.
 *
 * arvae_measure_notes: score [M, T] int64 -> out [M, T, 3] int32, per tick
 *   pitch   the MIDI number sounding during the tick, 0 = silence
 *   start   the tick at which that element began, -1 inside leading slurs
 *   length  on a tick that begins an element its duration in twelfths, 0 elsewhere
 *
 * arvae_render_pianoroll: score [F, K, T] -> out [F, H, W, 3] uint8 (any alignment), F figures of K measures in one launch.
 *   H = (pitch_hi - pitch_lo + 1) px_per_pitch, row 0 at pitch_hi; the roll is K (T / 6) 12 px_per_twelfth pixels wide; with
 *   `values` (fp32 [F, K], may be null) a white gap of `gap` pixels and a panel of K panel_cell pixels follow it.
 *   Roll pixel: shade v from the first layer that applies -- 127 on the first `mark` pixel columns of a sounding element (no
 *   further than the element reaches) on the rows of pitch - 1 .. pitch + 1; 90 on the element's extent on the rows of its pitch;
 *   100 on a measure's first column; 50 on a beat's first column; 30 on the rows of even pitches; else 0 -- and
 *   channel = 255 - (v (255 - dark) + 63) / 127 with dark = (8, 48, 107).  Rows outside [pitch_lo, pitch_hi] do not exist.
 *   Panel: measure k gets a black disc dx^2 + dy^2 <= dot_radius^2 (inside its own cell of panel_cell columns) around column
 *   k panel_cell + panel_cell / 2 and row H - 1 - (int)floorf(c (H - 1) + 0.5f), c = (value - vmin) / (vmax - vmin) clamped to
 *   [0, 1] (0.5 when vmax == vmin), each operation rounded to fp32 by itself; a non-finite value draws no disc.
 * arvae_render_pianoroll_bytes: H * W * 3, or -1 (bad argument, or 2^31 bytes and more: such a figure cannot be rendered). */
int arvae_measure_notes(const int64_t *score, int64_t M, int32_t T, const int32_t *midi_lut, const uint8_t *is_note, int32_t V,
                        int32_t slur, int32_t *out, arvae_stream_t stream);
int64_t arvae_render_pianoroll_bytes(int32_t K, int32_t T, int32_t pitch_lo, int32_t pitch_hi, int32_t px_per_twelfth,
                                     int32_t px_per_pitch, int32_t with_panel, int32_t panel_cell, int32_t gap);
int arvae_render_pianoroll(const int64_t *score, int32_t F, int32_t K, int32_t T, const int32_t *midi_lut, const uint8_t *is_note,
                           int32_t V, int32_t slur, const float *values, float vmin, float vmax, int32_t pitch_lo,
                           int32_t pitch_hi, int32_t px_per_twelfth, int32_t px_per_pitch, int32_t mark, int32_t panel_cell,
                           int32_t gap, int32_t dot_radius, uint8_t *out, arvae_stream_t stream);

/* Latent-space scatter figures (added under ABI 16: symbols only; csrc/scatter.hip): N points with a value each -> the bytes of a
 * figure, F figures in one launch.  Replaces the matplotlib scatter of plot_dim (utils/plotting.py:41-63) behind plot_data_dist
 * and MeasureVAETrainer.plot_latent_surface.  The look is this library's own:
 *   canvas  width x height, white.  The plot area is pw x ph = (width - 125) x (height - 39) pixels with its first pixel at
 *           (px0, py0) = (57, 11) and a black frame one pixel wide around it; a colour bar of bar_w = 12 columns and ph rows starts
 *           at column bar_x = px0 + pw + 12, framed likewise, row j of it (from the top) showing table entry
 *           ((ph - 1 - j) 255 + (ph - 1) / 2) / (ph - 1).
 *   marker  point i of figure f lies at X = (int)floorf((x - xlo) * kx + 0.5f) sixteenths of a pixel from the plot area's left edge,
 *           kx = (float)(16 pw) / (xhi - xlo), and Y = 16 ph - (int)floorf((y - ylo) * ky + 0.5f) from its top edge, every operation
 *           rounded to fp32 by itself.  It covers the pixels (i, j) of the plot area with
 *           (16 i + 8 - X)^2 + (16 j + 8 - Y)^2 <= (16 radius)^2: markers are clipped at the frame.  Its colour is entry
 *           (int)floorf(c * 255.f + 0.5f) of matplotlib's 256-level viridis table, c = (value - vmin) / (vmax - vmin) clamped to
 *           [0, 1]; entry 128 when vmax == vmin.  A point whose value is not finite, or whose position is not inside
 *           (-2^20, 2^20) sixteenths on both axes (a non-finite coordinate among them), draws nothing.
 *   blend   a channel is held in 1/256ths, white = 255 * 256; the markers that cover a pixel change it in the order of the input,
 *           c = (c (256 - a) + 256 colour a + 128) >> 8 with a = alpha256, and the byte written is (c + 128) >> 8: the later
 *           point is on top, and the picture depends on the order of the points alone.
 *   marks   everything else is a table of at most ARVAE_SCATTER_MAX_MARKS cells laid out by the caller, on the host: a glyph of the
 *           5 x 7 font "0123456789-.: dimenso" (glyph = its index there; rot = 1: turned a quarter to the left, a cell of 7 x 5
 *           whose columns are the glyph's rows and whose rows, from the bottom, its columns), a tick mark below an axis
 *           (ARVAE_SCATTER_TICK_X, 1 x 4) or beside one (ARVAE_SCATTER_TICK_Y, 4 x 1).  (x, y) is the cell's top-left pixel; `figure`
 *           the figure it belongs to, -1 for all.  Marks are black and drawn outside the two frames only.
 * points [F, N, 2] fp32 (8-byte aligned), values [F, N] fp32, both on the device (null allowed when N = 0); limits [F][6] on the
 * HOST: xlo, xhi, ylo, yhi, vmin, vmax per figure (finite, lo < hi, vmin <= vmax); marks on the HOST; out [F, height, width, 3]
 * uint8 on the device, any alignment.  F <= ARVAE_SCATTER_MAX_FIGURES, 1 <= radius <= 64, 0 <= alpha256 <= 256.
 * arvae_render_scatter_bytes: height * width * 3, or -1 (a canvas too small for the margins or with 2^31 bytes and more, a bad
 * radius); `geometry`, unless null, receives px0, py0, pw, ph, bar_x, bar_w. */
#define ARVAE_SCATTER_MAX_FIGURES 16
#define ARVAE_SCATTER_MAX_MARKS 384
#define ARVAE_SCATTER_GLYPHS 21
#define ARVAE_SCATTER_TICK_X 21
#define ARVAE_SCATTER_TICK_Y 22
typedef struct {
    int16_t x, y;
    uint8_t glyph, rot;
    int16_t figure;
} arvae_scatter_mark_t;
int64_t arvae_render_scatter_bytes(int32_t width, int32_t height, int32_t radius, int32_t *geometry);
int arvae_render_scatter(const float *points, const float *values, int32_t F, int64_t N, const float *limits, int32_t width,
                         int32_t height, int32_t radius, int32_t alpha256, const arvae_scatter_mark_t *marks, int32_t n_marks,
                         uint8_t *out, arvae_stream_t stream);

/* Attribute labels of a batch of measures.  Replaces MeasureVAETrainer.compute_attribute_labels
 * (measurevae/measure_vae_trainer.py:167-186 -> data/dataloaders/bar_dataset.py:338-500):
 *   out[b] = [rhythmic complexity, pitch range/26, note density, contour/26]
 * midi_lut / is_note / is_density_note: per-vocabulary tables (is_density_note also counts the `None` symbol,
 * bar_dataset.py:348-356); rhythm_weights[steps] = RHY_COMPLEXITY_COEFFS (bar_dataset_helpers.py:21-30),
 * rhythm_norm their sum. */
int arvae_measure_attributes(const int64_t *score, int32_t batch, int32_t steps, const int32_t *midi_lut,
                             const uint8_t *is_note, const uint8_t *is_density_note, int32_t vocab,
                             const float *rhythm_weights, float rhythm_norm, float *out, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-model step for the conv VAEs: ONE call enqueues every kernel of the forward pass (+ loss terms)
 * or of the backward pass, so the host does no per-layer work.  Replaces, as a unit,
 *   ImageVAETrainer.loss_and_acc_for_batch (imagevae/image_vae_trainer.py:137-217)
 *     = MnistVAE.forward (imagevae/mnist_vae.py:89-105) + reconstruction_loss + compute_kld_loss
 *       + the compute_reg_loss loop + mean_accuracy,
 *   and loss.backward() (utils/trainer.py:140) for that graph.
 * The model is described layer by layer; weights/biases are float offsets into ONE parameter arena and
 * gradients accumulate at the same offsets of a gradient arena (the trainer's flat Adam arenas).
 * ------------------------------------------------------------------------------------------------ */
#define ARVAE_MAX_LAYERS 8

typedef struct {
    arvae_link_t link;    /* geometry; link.n is ignored (the batch is a call argument)               */
    int32_t is_up;        /* 0: forward is DOWN (nn.Conv2d / nn.Linear), 1: UP (nn.ConvTranspose2d)   */
    int32_t act;          /* ARVAE_ACT_* applied after the bias                                        */
    int32_t dropout;      /* 1: nn.Dropout(0.5) follows (a keep-mask is consumed in train mode)        */
    int32_t reserved;
    int64_t w_off, b_off; /* float offsets of weight and bias in the parameter / gradient arenas       */
} arvae_layer_t;

struct arvae_milestones;
typedef struct {
    int32_t n_enc, n_dec;                 /* encoder layers up to the hidden vector; decoder layers z -> logits */
    arvae_layer_t enc[ARVAE_MAX_LAYERS];
    arvae_layer_t dec[ARVAE_MAX_LAYERS];
    arvae_layer_t head_mu, head_log_std;  /* dense heads on the encoder's hidden vector               */
    int32_t zdim;
    int32_t recon_dist;                   /* ARVAE_RECON_*                                             */
    int32_t n_reg;                        /* regularised dims (0: no attribute regularisation)         */
    int32_t reg_dims[16];
    float beta, gamma, delta;
    /* rng_eps != 0: arvae_image_vae_forward DRAWS the reparameterisation noise itself (Philox4x32-10, arvae_philox_normal's
     * stream for the same seed / offset / step / dev_step) inside the fused heads kernel and WRITES it to `eps`, which the
     * backward pass then reads; 0: `eps` is an input (parity runs with explicit noise). */
    int32_t rng_eps;
    uint32_t rng_offset, rng_step;
    uint64_t rng_seed;
    const uint32_t *rng_dev_step;
    /* Optional (NULL: none).  hipEvent_t handles, created by the caller, which the executors RECORD on `stream` as soon as a
     * result that other work may start from is complete -- so that a data-parallel caller can start its RCCL collectives on
     * a side stream while the rest of the pass still runs (the reference is single-process: SURVEY.md section 8(e), "one
     * all-gather between encoder forward and the reg kernel", "all-reduce overlapped with the tail of backward").  Every
     * non-NULL event is recorded exactly once per call (at the end of the pass if the executor has no earlier point for it).
     *   z_ready       arvae_image_vae_forward : mu / sigma / z are final (the decoder's launches follow)
     *   dec_grads     arvae_image_vae_backward: the gradients of every conv layer of the DECODER are final in `grads`
     *   linear_grads  arvae_image_vae_backward: the gradients of every Linear layer and of the two heads are final
     * With dec_grads / linear_grads set, the backward pass finishes those gradients early (the decoder layers' slab
     * reduction and the grouped Linear weight gradients are launched where their inputs are complete instead of at the end
     * of the pass: one launch more). */
    const struct arvae_milestones *milestones;
    /* Optional (NULL: none).  ONE device word the caller owns and zeroes once; the passes only ever OR bits into it
     * (ARVAE_STATUS_*).  The latent block of the dSprites-shaped model runs on clusters of workgroups that hand activations to
     * each other inside a launch (csrc/midcluster.hip); a hand-off whose partners never arrive -- they cannot all become
     * resident, e.g. many processes on one device -- gives up after a bounded poll, sets its bit and the launch ends: the
     * results of THAT pass are then undefined.  The caller reads the word where it synchronises anyway (the reference reads
     * its loss every step, utils/trainer.py:145-147; this build once per epoch), raises, and sets ARVAE_VAE_NO_CLUSTER in
     * `flags` for every later call. */
    uint32_t *status;
    int32_t flags;        /* ARVAE_VAE_* */
    int32_t reserved;
} arvae_image_vae_t;

/* The word is zero or a NORMAL POSITIVE fp32 bit pattern (2.0 .. 3.75: ARVAE_STATUS_SET + code bits in the top of the
 * mantissa), so that a data-parallel caller can keep it in the tail of the buffer it SUM all-reduces as floats
 * (ar-vae_amd/optim.py: the guard slot behind the gradient arena): a failure on one rank then reaches every rank's word
 * with the gradients it polluted, and every rank's arvae_adam_step skips the same update.  After such a sum only
 * "non-zero" is meaningful; on the rank that failed (and on a single rank) the code bits read back exactly. */
#define ARVAE_STATUS_SET 0x40000000u
#define ARVAE_STATUS_HANDOFF_FWD (ARVAE_STATUS_SET | (1u << 20))    /* a hand-off of the clustered latent block's forward launch gave up */
#define ARVAE_STATUS_HANDOFF_BWD (ARVAE_STATUS_SET | (2u << 20))    /* ... of its backward launch                                         */
#define ARVAE_STATUS_HANDOFF_TICKET (ARVAE_STATUS_SET | (4u << 20)) /* a workgroup found no place in any cluster (corrupt ticket heads)   */
#define ARVAE_VAE_NO_CLUSTER 1         /* flags: the latent block on the row kernels (no in-launch hand-offs)  */
/* flags (ABI 11), a TRAINING step only: arvae_image_vae_forward leaves the pass's finishing step -- the sums that become
 * scalars[] (loss, its terms, accuracy), the KL mean and the regulariser's z-gradient, ~9 us of one workgroup with the chip idle
 * -- to arvae_image_vae_backward, whose first launch carries it as one more workgroup (or which launches it first thing where that
 * launch is of another kind).  Until the backward call has run, scalars[0 .. 7] read as NaN.  Set the same flag for both calls
 * of a step; never for a forward pass no backward pass follows. */
#define ARVAE_VAE_DEFER_FINISH 2

typedef struct arvae_milestones {
    void *z_ready, *dec_grads, *linear_grads;
} arvae_milestones_t;

/* scalars written by the forward pass (device array of ARVAE_VAE_NSCALARS floats) */
#define ARVAE_VAE_LOSS 0   /* recon + dist + reg_scale*reg                                              */
#define ARVAE_VAE_RECON 1
#define ARVAE_VAE_DIST 2   /* beta * |kl - c|                                                            */
#define ARVAE_VAE_REG 3    /* reg_scale * (sum over dims of the row-block regularisation loss)          */
#define ARVAE_VAE_ACC 4
#define ARVAE_VAE_KL 5
#define ARVAE_VAE_NSCALARS 8

int64_t arvae_image_vae_ws_floats(const arvae_image_vae_t *model, int32_t batch, int64_t n_cols);

/* Forward + loss terms.  x [batch, H, W, 1]; labels [batch, ld_labels]; eps [batch, zdim] (WRITTEN when model->rng_eps);
 * masks: HOST array with one device uint8 keep-mask per dropout layer (encoder first), or NULL (eval).
 * z_cols/lab_cols [n_cols, ...]: all-gathered columns for the data-parallel row-block regularisation
 * (NULL: this batch is the whole batch); they index dims 0..n_reg-1 compactly when given.
 * n_cols: 0 = the regulariser runs on this batch alone; > 0 with z_cols/lab_cols; -1 = no regulariser in this call (the
 * caller evaluates it on z); -2 = neither the regulariser nor the scalars: arvae_image_vae_finish completes the pass.
 * reg_scale multiplies the regularisation term (world size under data parallelism, else 1).
 * Outputs: scalars[ARVAE_VAE_NSCALARS], mu/sigma/z [batch, zdim], logits [batch, H, W, 1].
 * Everything the backward pass needs stays in ws. */
int arvae_image_vae_forward(const arvae_image_vae_t *model, int32_t batch, const float *params, const float *x,
                            const float *labels, int64_t ld_labels, const float *eps,
                            const uint8_t *const *masks, const float *capacity, const float *z_cols,
                            const float *lab_cols, int64_t n_cols, float reg_scale, float *ws, float *scalars,
                            float *mu, float *sigma, float *z, float *logits, arvae_stream_t stream);

/* Data-parallel completion of a forward pass that was called with n_cols == -2 ("the caller finishes"): the regulariser of
 * this rank's rows against the columns GATHERED from every rank (whole rows: z_cols [n_cols, zdim], lab_cols [n_cols,
 * ld_labels], n_cols = world size x batch), then the pass's scalars exactly as the forward pass
 * would have written them: scalars[ARVAE_VAE_REG] = reg_scale x the row-block term.  The backward pass follows with
 * reg_fused == 1 and the same reg_scale.  (The reference evaluates the term on one process: utils/trainer.py:369-403.) */
int arvae_image_vae_finish(const arvae_image_vae_t *model, int32_t batch, const float *labels, int64_t ld_labels,
                           const float *capacity, const float *z_cols, const float *lab_cols, int64_t n_cols,
                           float reg_scale, float *ws, float *scalars, const float *mu, const float *sigma, const float *z,
                           arvae_stream_t stream);

/* Backward of scalars[ARVAE_VAE_LOSS] times g_loss[0] (device scalar): parameter gradients ACCUMULATE into
 * grads at the layers' offsets.  Must follow arvae_image_vae_forward on the same ws, with the same
 * x / eps / masks / capacity and that call's mu / sigma / z / logits outputs.
 * reg_fused: 1 when the forward evaluated the regularisation term itself (n_cols >= 0); 0: no regulariser here;
 *            2: dz_extra holds the regulariser's gradient w.r.t. z for UNIT upstream (arvae_reg_loss's dz, evaluated
 *            by a data-parallel caller on its row block against the gathered columns): it is scaled by
 *            g_loss[0] * reg_scale here.
 * dz_extra: with reg_fused 0 or 1 an optional extra gradient w.r.t. z [batch, zdim], ALREADY multiplied by the
 *            upstream gradient. */
int arvae_image_vae_backward(const arvae_image_vae_t *model, int32_t batch, const float *params, float *grads,
                             const float *x, const float *eps, const uint8_t *const *masks,
                             const float *capacity, const float *mu, const float *sigma, const float *z,
                             const float *logits, const float *g_loss, const float *dz_extra,
                             int32_t reg_fused, float reg_scale, float *ws, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-model step for MeasureVAE: ONE call enqueues every kernel of the forward pass (+ loss terms) or of the backward pass
 * (about 45 / 45 launches at the reference configuration), so the host does no per-layer work.  Replaces, as a unit,
 *   MeasureVAETrainer.loss_and_acc_for_batch (measurevae/measure_vae_trainer.py:85-140)
 *     = MeasureVAE.forward (measurevae/measure_vae.py:97-131: Encoder.forward, encoder.py:108-124; HierarchicalDecoder.forward,
 *       decoder.py:408-525) + mean_crossentropy_loss + compute_kld_loss + compute_attribute_labels + the compute_reg_loss loop
 *       + mean_accuracy,
 *   and loss.backward() (utils/trainer.py:140) for that graph.
 * The model is the reference configuration's shape: a 2-layer bidirectional GRU encoder, two 2-layer heads, a 2-layer beat GRU and
 * a 2-layer tick GRU with teacher-forced or argmax-fed inputs.  Parameters are float offsets into ONE parameter arena, gradients
 * ACCUMULATE at the same offsets of a gradient arena (the trainer's flat Adam arenas).  Three pairs of tensors must lie back to
 * back in the arenas, because one product applies both (ar-vae_amd/measure_vae.py MeasureVAE.arena_parameters):
 *   per encoder layer  weight_ih_l{k} | weight_ih_l{k}_reverse   and   bias_ih_l{k} | bias_ih_l{k}_reverse,
 *   linear_mean.0 | linear_log_std.0 (weights, biases),  beat_emb_to_tick_rnn_hidden.0 | beat_emb_to_tick_rnn_input.0.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t vocab, emb;                       /* note vocabulary, note_embedding_dim                                         */
    int32_t enc_hidden, dec_hidden, zdim;     /* hidden sizes must be built as sequence kernels (arvae_gru_seq_supported)     */
    int32_t steps, beats, ticks_per_beat;     /* 24 = 4 * 6 in the reference; steps == beats * ticks_per_beat                 */
    /* float offsets into the parameter / gradient arenas */
    int64_t enc_table;                        /* encoder.note_embedding_layer.weight [vocab][emb]                             */
    int64_t enc_w_ih[2], enc_b_ih[2];         /* per layer: the forward direction's; the reverse direction's follows directly  */
    int64_t enc_w_hh[2][2], enc_b_hh[2][2];   /* [layer][direction]                                                           */
    int64_t head_w0, head_b0;                 /* linear_mean.0 followed directly by linear_log_std.0                          */
    int64_t mean_w2, mean_b2, lstd_w2, lstd_b2;
    int64_t dec_table, x0, b0;                /* decoder.note_embedding_layer.weight, x_0 [emb], b_0 [1]                       */
    int64_t z2beat_w, z2beat_b;               /* z_to_beat_rnn_input.0                                                        */
    int64_t beat_w_ih[2], beat_b_ih[2], beat_w_hh[2], beat_b_hh[2];
    int64_t tick_init_w, tick_init_b;         /* beat_emb_to_tick_rnn_hidden.0 followed directly by beat_emb_to_tick_rnn_input.0 */
    int64_t tick_w_ih[2], tick_b_ih[2], tick_w_hh[2], tick_b_hh[2];
    int64_t out_w, out_b;                     /* tick_emb_to_note_emb.0                                                       */
    float enc_dropout, dec_dropout;           /* p of nn.GRU(dropout = p); applied when the call is given keep-masks          */
    int32_t n_reg;                            /* regularised dims (0: no attribute regularisation)                            */
    int32_t reg_dims[16];                     /* z[:, d] pairs with attribute column d (d < 4)                                */
    float beta, gamma, delta;
    /* rng_draw != 0: the forward pass DRAWS the encoder keep-mask, eps and the decoder keep-masks itself (arvae_philox_* streams
     * rng_offset[0..2] of rng_seed / rng_step / rng_dev_step) and WRITES them to the caller's buffers, which the backward pass then
     * reads; 0: they are inputs (parity runs with explicit noise and masks). */
    int32_t rng_draw;
    uint32_t rng_offset[3], rng_step;
    uint64_t rng_seed;
    const uint32_t *rng_dev_step;
} arvae_measure_vae_t;

/* the per-vocabulary tables of arvae_measure_attributes */
typedef struct {
    const int32_t *midi_lut;
    const uint8_t *is_note, *is_density_note;
    const float *rhythm_weights;
    float rhythm_norm;
} arvae_measure_tables_t;

int64_t arvae_measure_vae_ws_floats(const arvae_measure_vae_t *model, int32_t batch);

/* Forward + loss terms.  score [batch][steps] int64; eps [batch][zdim]; enc_mask [steps][batch][2*enc_hidden] and dec_mask
 * [beats + steps][batch][dec_hidden] uint8 keep-masks of the GRUs' inter-layer dropout (beat RNN's first), both NULL = evaluation
 * mode (no dropout); eps / masks are WRITTEN when model->rng_draw.  teacher_forced: the tick RNN is fed the score's notes
 * (decoder.py:427-428,510-512), else its own argmax (one free-running launch, not differentiated: decoder.py:506-516).
 * capacity: 1-element device tensor or NULL (c = 0).  tables: needed when model->n_reg > 0.
 * Outputs: scalars[ARVAE_VAE_NSCALARS] (loss = cross entropy + beta |KL - c| + sum_d gamma reg_d; ARVAE_VAE_ACC = top-1 accuracy),
 * mu / sigma / z [batch][zdim], tokens [batch][steps] = the notes fed back (the score when teacher_forced).
 * Everything the backward pass needs stays in ws (arvae_measure_vae_ws_floats floats, 16-byte aligned). */
int arvae_measure_vae_forward(const arvae_measure_vae_t *model, int32_t batch, const float *params, const int64_t *score,
                              float *eps, uint8_t *enc_mask, uint8_t *dec_mask, int32_t teacher_forced, const float *capacity,
                              const arvae_measure_tables_t *tables, float *ws, float *scalars, float *mu, float *sigma, float *z,
                              int64_t *tokens, float *labels /* [batch][4] attribute labels out, or NULL */, int32_t defer_finish,
                              arvae_stream_t stream);

/* Data-parallel completion of a forward pass called with defer_finish != 0 (which stops before the regulariser and the scalars): the
 * regulariser of this rank's rows against the columns GATHERED from every rank (z_cols [n_cols][zdim], lab_cols [n_cols][4],
 * n_cols = world size x batch: SURVEY.md section 8(e)), then the pass's scalars exactly as the forward pass would have written them,
 * scalars[ARVAE_VAE_REG] = reg_scale x the row-block term (reg_scale = world size).  The backward pass follows with the same reg_scale.
 * (The reference evaluates the term on one process: utils/trainer.py:369-403, measurevae/measure_vae_trainer.py:129-137.) */
int arvae_measure_vae_finish(const arvae_measure_vae_t *model, int32_t batch, const float *capacity, const float *z_cols,
                             const float *lab_cols, int64_t n_cols, float reg_scale, float *ws, float *scalars, const float *mu,
                             const float *sigma, const float *z, const float *labels, arvae_stream_t stream);

/* Backward of scalars[ARVAE_VAE_LOSS] times g_loss[0] (device scalar): parameter gradients ACCUMULATE into grads at the model's
 * offsets.  Must follow arvae_measure_vae_forward on the same ws, with the same score / eps / masks / capacity and that call's
 * mu / sigma / z / tokens / scalars outputs. */
int arvae_measure_vae_backward(const arvae_measure_vae_t *model, int32_t batch, const float *params, float *grads,
                               const int64_t *score, const float *eps, const uint8_t *enc_mask, const uint8_t *dec_mask,
                               const float *capacity, const float *mu, const float *sigma, const float *z, const int64_t *tokens,
                               const float *scalars, const float *g_loss, float reg_scale /* 1, or the world size after _finish */,
                               float *ws, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Random draws of the path: eps of z_dist.rsample() (imagevae/mnist_vae.py:79, measurevae/measure_vae.py:116) and the
 * keep-masks of nn.Dropout(0.5) / nn.GRU(dropout=0.5) (imagevae/mnist_vae.py:16-47, measurevae/encoder.py:27-34,
 * decoder.py:338-368) from a counter-based Philox4x32-10 generator: element i of a draw is a pure function of
 * (seed, offset = index of the draw inside the step, step + *dev_step, i).  dev_step (optional device word) lets a captured
 * HIP graph advance the stream by itself.  The reference draws from torch's global generator instead; parity runs pass
 * explicit eps / masks, so only the distribution has to agree (tests: known-answer vectors, moments, determinism).
 * arvae_philox_normal: one N(0,1) value per element (Box-Muller).  arvae_philox_keep_mask: uint8 1 with probability
 * keep_prob (quantised to 1/256), out 16-byte aligned.  arvae_philox_keep_masks: up to 8 such masks (the five Dropout(0.5)
 * layers of imagevae/mnist_vae.py:16-47) as ONE launch; mask j is draw offsets[j] of the step: the same bytes as
 * arvae_philox_keep_mask(outs[j], counts[j], keep_prob, seed, offsets[j], step, dev_step).
 * ------------------------------------------------------------------------------------------------ */
int arvae_philox_normal(float *out, int64_t count, uint64_t seed, uint32_t offset, uint32_t step, const uint32_t *dev_step,
                        arvae_stream_t stream);
/* one u in (0, 1] per element: (x + 1) * 2^-32 of the first word x of the element's own block, the word arvae_philox_normal's radius
 * takes (the draws of torch.multinomial, measurevae/decoder.py:502-505, as an explicit buffer) */
int arvae_philox_uniform(float *out, int64_t count, uint64_t seed, uint32_t offset, uint32_t step, const uint32_t *dev_step,
                         arvae_stream_t stream);
int arvae_philox_keep_mask(uint8_t *out, int64_t count, float keep_prob, uint64_t seed, uint32_t offset, uint32_t step,
                           const uint32_t *dev_step, arvae_stream_t stream);
int arvae_philox_keep_masks(int32_t n_masks, uint8_t *const *outs, const int64_t *counts, float keep_prob, uint64_t seed,
                            const uint32_t *offsets, uint32_t step, const uint32_t *dev_step, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Debug-mode failure checks (off by default; the Python side runs them with ARVAE_CHECK=1 and raises ValueError as the
 * reference does): number of NaN / infinite values of a parameter arena (measurevae/encoder.py:101-106,
 * decoder.py:420-425) and number of note indices outside [lo, hi) (Decoder.check_index, decoder.py:30-41), ADDED to the
 * device word `flag` (the caller zeroes it; integer adds, so the count is exact).
 * ------------------------------------------------------------------------------------------------ */
int arvae_count_nonfinite(const float *values, int64_t count, int32_t *flag, arvae_stream_t stream);
int arvae_count_out_of_range(const int64_t *indices, int64_t count, int64_t lo, int64_t hi, int32_t *flag,
                             arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel exchange of a row-sharded training step (the reference is single-process, so
 * there is no call site to replace -- these run where the sharded step needs what the reference reads from one batch):
 *   - all-gather of the regularised latent / label columns: the attribute term averages over ALL pairs of the global batch
 *     (Trainer.reg_loss_sign, utils/trainer.py:378-403), each rank evaluates its row block against the gathered columns;
 *   - SUM all-reduce of the flat gradient arena between loss.backward() and optimizer.step() (utils/trainer.py:140-147),
 *     arvae_adam_step then applies 1 / world through grad_scale;
 *   - broadcast of rank 0's parameters / shuffling order when training starts (utils/trainer.py:39-64 builds them on one
 *     process), MAX / MIN reductions for timing and for agreeing on a fallback.
 * The collectives are RCCL calls enqueued on `stream` like any kernel of this library: nothing synchronises, nothing is
 * polled by a helper thread, and a stream capture records them into the same HIP graph as the kernels around them.
 * RCCL is resolved at run time (the librccl.so.1 already loaded in the process, else the system one): a single-GPU
 * process never loads it.  One communicator = one device; every rank of the job calls arvae_comm_init together.
 * A communicator is caller-owned state (create / destroy), not library state.
 *
 *   arvae_comm_available  -> RCCL's version code (> 0) or ARVAE_E_COMM with the reason in arvae_last_error_string()
 *   arvae_comm_unique_id  -> ARVAE_COMM_ID_BYTES host bytes; rank 0 creates them, the caller's launcher (a TCP store, MPI, a
 *                            file) hands them to every other rank
 *   arvae_comm_init       -> waits until all `world` ranks have joined, on the CURRENT HIP device, for at most timeout_ms
 *                            (0: no deadline); ARVAE_E_COMM after the deadline: RCCL cannot be called back from a half-built
 *                            communicator, so the process must exit then
 *   arvae_comm_async_error-> 0, or ARVAE_E_COMM once the communicator has failed asynchronously (a peer died)
 * dtype: ARVAE_COMM_*; `count` in elements (per rank for the all-gather: recv holds world x count, rank-major).
 * all_reduce and broadcast work in place.
 * ------------------------------------------------------------------------------------------------ */
#define ARVAE_COMM_ID_BYTES 128
#define ARVAE_COMM_F32 0
#define ARVAE_COMM_F64 1
#define ARVAE_COMM_I64 2
#define ARVAE_COMM_U8 3
#define ARVAE_COMM_SUM 0
#define ARVAE_COMM_MAX 1
#define ARVAE_COMM_MIN 2
typedef struct arvae_comm_s *arvae_comm_t;
int arvae_comm_available(void);
int arvae_comm_unique_id(void *id_out /* host */);
int arvae_comm_init(const void *id /* host */, int32_t rank, int32_t world, int32_t timeout_ms, arvae_comm_t *out /* host */);
int arvae_comm_destroy(arvae_comm_t comm);
int arvae_comm_abort(arvae_comm_t comm);
int arvae_comm_rank(arvae_comm_t comm);
int arvae_comm_world(arvae_comm_t comm);
int arvae_comm_async_error(arvae_comm_t comm);
int arvae_comm_all_gather(arvae_comm_t comm, const void *send, void *recv, int64_t count, int32_t dtype,
                          arvae_stream_t stream);
int arvae_comm_all_reduce(arvae_comm_t comm, void *buf, int64_t count, int32_t dtype, int32_t op, arvae_stream_t stream);
int arvae_comm_broadcast(arvae_comm_t comm, void *buf, int64_t count, int32_t dtype, int32_t root, arvae_stream_t stream);
/* the collectives enqueued by this thread between the two calls go out as ONE RCCL launch (ncclGroupStart / ncclGroupEnd):
 * the z and the label all-gather of a step */
int arvae_comm_group_begin(void);
int arvae_comm_group_end(void);

/* ------------------------------------------------------------------------------------------------
 * KSG (Kraskov-Stoegbauer-Grassberger) mutual information of the disentanglement metrics, in fp64.
 * Replaces: sklearn.feature_selection.mutual_info_regression as called by utils/evaluation.py (interpretability, modularity,
 * MIG and its entropies); the caller does sklearn's scaling and tie-breaking noise on the host (arvae_amd.evaluation) and
 * this call reproduces its _compute_mi_cc for each column, bit for bit in the radii and counts:
 *   r_i  = nextafter(k-th smallest max(|x_j - x_i|, |y_j - y_i|) over j != i, 0)
 *   nx_i = #{j : |x_j - x_i| <= r_i} - 1,  ny_i likewise with y
 *   mi   = max(0, psi(n) + psi(k) - mean psi(nx + 1) - mean psi(ny + 1))
 * x: p columns of n values, column c at x + c * ldx (ldx >= n); y: n values shared by the p columns; 1 <= k <= 8, k < n.
 * ws: arvae_ksg_ws_bytes(n, p) bytes.  mi_out[p].  radius_out / nx_out / ny_out: optional [p][n] (NULL = not written).
 * Deterministic: per-workgroup partial sums, then a fixed-order reduction (no float atomics).
 * ------------------------------------------------------------------------------------------------ */
int64_t arvae_ksg_ws_bytes(int64_t n, int32_t p);
int arvae_ksg_mi(const double *x, int64_t ldx, int32_t p, const double *y, int64_t n, int32_t k, void *ws, double *mi_out,
                 double *radius_out, int32_t *nx_out, int32_t *ny_out, arvae_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The Morpho-MNIST digit classifier: inference of a torchvision ResNet-18 (BasicBlock, [2,2,2,2], 10 classes, 1-channel 7x7
 * stem, AvgPool2d(1)) at 28 x 28, batch-norm in evaluation mode (eps 1e-5, running statistics) folded into the convolutions.
 * Replaces: imagevae/mnist_resnet.py:18-19 as called by imagevae/image_vae_trainer.py:657-666 (digit_pred_acc).
 * Activations are NHWC; weights keep the state_dict layout [C_out, C_in, K, K].  csrc/resnet18.hip.
 *
 * One convolution: cin, cout in {64, 128, 256, 512}; (ksize 3, pad 1) or (ksize 1, pad 0); stride 1 or 2; hin, win <= 64;
 * hout = (hin + 2 pad - ksize) / stride + 1.  out = [relu](conv(x, w') + b' [+ residual]) with w' = w gamma / sqrt(var + eps),
 * b' = beta - mean gamma / sqrt(var + eps) computed in float64 (all four bn pointers NULL: w' = w, b' = 0).  Only the LIVE taps --
 * those that read a pixel inside the input for some output pixel -- are packed and multiplied; arvae_resnet18_live_taps returns
 * their number and writes their indices ky * ksize + kx to taps[<= 9] (host memory, may be NULL).
 * prep: arvae_resnet18_conv_prep_floats(geom) floats, 16-byte aligned, written by _conv_prepare and read by _conv.
 * residual (optional) and out: [n, hout, wout, cout]; out aliases neither input.  Products on the three-term bf16 MFMA arithmetic,
 * fp32 accumulation in a fixed order: the same input gives the same bits.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t hin, win, cin, hout, wout, cout, ksize, stride, pad, reserved;
} arvae_resnet18_conv_t;
int32_t arvae_resnet18_live_taps(const arvae_resnet18_conv_t *geom /* host */, int32_t *taps /* host */);
int64_t arvae_resnet18_conv_prep_floats(const arvae_resnet18_conv_t *geom /* host */);
int arvae_resnet18_conv_prepare(const arvae_resnet18_conv_t *geom /* host */, const float *w, const float *bn_w, const float *bn_b,
                                const float *bn_mean, const float *bn_var, float *prep, arvae_stream_t stream);
int arvae_resnet18_conv(const arvae_resnet18_conv_t *geom /* host */, const float *prep, const float *x, int32_t n,
                        const float *residual, int32_t relu, float *out, arvae_stream_t stream);
/* the stem: conv 7x7 stride 2 pad 3 of x[n,1,28,28] with w[64,1,7,7], BN folded as above, + b', optional ReLU -> out[n,14,14,64] */
int64_t arvae_resnet18_stem_prep_floats(void);
int arvae_resnet18_stem_prepare(const float *w, const float *bn_w, const float *bn_b, const float *bn_mean, const float *bn_var,
                                float *prep, arvae_stream_t stream);
int arvae_resnet18_stem(const float *prep, const float *x, int32_t n, int32_t relu, float *out, arvae_stream_t stream);
/* max-pool 3x3 stride 2 pad 1 of x[n,h,w,c] (c a multiple of 4) -> out[n,(h-1)/2+1,(w-1)/2+1,c]; padding counts as -inf */
int arvae_resnet18_maxpool(const float *x, int32_t n, int32_t h, int32_t w, int32_t c, float *out, arvae_stream_t stream);
/* logits = feat[n,512] fc_w[10,512]^T + fc_b; probs = softmax(logits); pred = argmax (lowest index on an exact tie).
 * logits, probs, pred: each optional */
int arvae_resnet18_head(const float *fc_w, const float *fc_b, const float *feat, int32_t n, float *logits, float *probs, int64_t *pred,
                        arvae_stream_t stream);
/* The whole network.  The 19 convolutions after the stem in execution order: layerL.B.conv1, [layerL.0.downsample.0,] layerL.B.conv2
 * for L = 1..4, B = 0, 1 (the downsample where L >= 2, B = 0), each with the batch-norm that follows it; stem_bn and the bn_*
 * tables are weight, bias, running_mean, running_var.
 * arvae_resnet18_prepare writes arvae_resnet18_prep_floats() floats (call it again after ANY change of a weight or statistic);
 * arvae_resnet18_forward runs x[n,1,28,28] through 22 launches with ws of arvae_resnet18_ws_floats(n) floats and writes
 * logits[n,10], probs[n,10] and pred[n] (each optional, one required). */
typedef struct {
    const float *stem_w, *stem_bn[4];
    const float *conv_w[19], *bn_w[19], *bn_b[19], *bn_mean[19], *bn_var[19];
    const float *fc_w, *fc_b;
} arvae_resnet18_weights_t;
int64_t arvae_resnet18_prep_floats(void);
int arvae_resnet18_prepare(const arvae_resnet18_weights_t *weights /* host */, float *prep, arvae_stream_t stream);
int64_t arvae_resnet18_ws_floats(int32_t n);
int arvae_resnet18_forward(const float *prep, const float *x, int32_t n, float *logits, float *probs, int64_t *pred, float *ws,
                           arvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ARVAE_HIP_H */
