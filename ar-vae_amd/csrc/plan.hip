// Whole-model forward / backward executors for the conv AR-VAEs (see include/arvae_hip.h): one host call
// enqueues every kernel of a pass on the caller's stream.  Host-side sequencing only -- the math lives in
// the link / dense / loss kernels, reached through the same C-ABI entry points a per-layer caller uses.
#include "diag.h"
#include "common.h"
#include "dense.h"
#include "reduce.h"
#include "midprep.h"
#include "regloss.h"
#include "vae_finish.h"
#include "amax.h"
#include "conv32.h"
#include "conv_c1.h"
#include "conv64.h"
#include "link.h"
#include "heads.h"
#include "midblock.h"
#include "losses.h"

namespace arvae {

// ---- small glue kernels ---------------------------------------------------------------------------
// gradient of the loss w.r.t. (mu, log_std) from: the decoder path g_z (already times g), the
// regularisation gradient dz_reg (unit upstream, scaled by g*reg_scale here), an optional external
// z gradient, and the beta-KL term; sigma = exp(log_std), z = mu + eps*sigma.
__global__ __launch_bounds__(256) void latent_bwd_full_kernel(const float *__restrict__ g_z, const float *__restrict__ dz_reg,
                                                               const float *__restrict__ dz_extra, const float *__restrict__ mu,
                                                               const float *__restrict__ sigma, const float *__restrict__ eps,
                                                               const float *__restrict__ g_loss, const float *__restrict__ kl,
                                                               const float *__restrict__ cap, float beta, float inv_batch,
                                                               float reg_scale, int64_t count, float *__restrict__ d_mu,
                                                               float *__restrict__ d_ls) {
    const float g = g_loss[0];
    const float diff = kl[0] - (cap != nullptr ? cap[0] : 0.f);
    const float k = g * beta * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * inv_batch;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        float gz = g_z[i];
        if (dz_reg != nullptr) gz += g * reg_scale * dz_reg[i];
        if (dz_extra != nullptr) gz += dz_extra[i];
        const float s = sigma[i];
        d_mu[i] = gz + k * mu[i];
        d_ls[i] = (gz * eps[i] + k * (s - 1.f / s)) * s;
    }
}

// a += b, optionally gated by the saved ReLU output the gradient belongs to
__global__ __launch_bounds__(256) void add_inplace_kernel(float *__restrict__ a, const float *__restrict__ b,
                                                           const float *__restrict__ gate, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const float v = a[i] + b[i];
        a[i] = (gate == nullptr || gate[i] > 0.f) ? v : 0.f;
    }
}

// ---- workspace layout ------------------------------------------------------------------------------
static inline int64_t up4(int64_t v) { return (v + 3) / 4 * 4; }

static inline int64_t out_elems(const arvae_layer_t &l, int64_t n) {
    return l.is_up ? n * l.link.hh * l.link.hw * l.link.chi : n * l.link.lh * l.link.lw * l.link.clo;
}
static inline int64_t in_elems(const arvae_layer_t &l, int64_t n) {
    return l.is_up ? n * l.link.lh * l.link.lw * l.link.clo : n * l.link.hh * l.link.hw * l.link.chi;
}

// the forms of a layer description every use below starts from
static inline arvae_link_t with_batch(const arvae_layer_t &l, int64_t n) {
    arvae_link_t lk = l.link;
    lk.n = (int32_t)n;
    return lk;
}
// the layer's bias inside `base` (the parameter or the gradient arena), or null
template <class T> static inline T *bias_of(const arvae_layer_t &l, T *base) { return l.b_off >= 0 ? base + l.b_off : nullptr; }
// a layer of the wide stack (Morpho-MNIST's 64-channel stride-1 convolutions and their single-channel ends): none of the
// Linear / 32-channel / single-channel 64x64 families serves it
static inline bool wide_stack(const arvae_link_t *lk) { return !dense_fits(lk) && !conv32_fits(lk) && !conv_c1_fits(lk); }

// One layer's buffers as offsets into the workspace (-1: the layer has none)
struct LayerSlots {
    int64_t out;    // the layer's output (the last decoder layer has none: logits are external)
    int64_t keep;   // the gradient w.r.t. the output (kept until the end of the backward pass)
    int64_t slab;   // conv layers with a slab kernel: their own slab, so that all the reductions can run as one launch at the end
    // ReLU conv layers on the fast kernels also leave the sign bits of their output (relu_bits16, 4 bytes per pixel):
    // the backward pass gates with those instead of re-reading the 128-byte-per-pixel activation
    int64_t bits;
    // 32-channel conv layers: the weights split into bf16 terms in per-lane order, rebuilt at the start of every forward
    // pass by ONE launch and used by the layer's forward and data-gradient kernels
    int64_t wprep;
    // wide (64-channel, row-staged) conv layers: the split weights of both orientations ([0] Conv2d-forward, [1] transposed), made by
    // ONE launch at the start of the forward pass and used by the layer's forward and data-gradient launches
    int64_t wide[2];
    // AMAX arrays (amax.h: the partial maxima a tensor carries for the 32-channel kernels that scale it into fp16) of
    // the output and of the gradient w.r.t. it
    int64_t amax, gamax;
};
// the same as pointers (null: the layer has none), View below
struct LayerBufs {
    float *out, *keep, *slab;
    uint16_t *bits;
    float *wprep, *wide[2];
    unsigned *amax, *gamax;
};

struct Layout {
    LayerSlots enc[ARVAE_MAX_LAYERS], dec[ARVAE_MAX_LAYERS];
    // AMAX arrays of the two ping-pong gradient buffers, and two for a tensor that arrives without (the image, or what a kernel
    // outside the conv32 / conv_c1 / latent-block family wrote)
    int64_t ga_amax, gb_amax, tmp_amax, tmp2_amax;
    int64_t log_std, dlogits, dz_reg, d_mu, d_ls, g_a, g_b, slab, link_ws, mid_prep, mid_wide, fin_args, rec_ws, reg_ws, rec_out, kld_out, reg_out, total;
    int64_t slab_floats;
};

static int make_layout(const arvae_image_vae_t *m, int64_t n, Layout &L) {
    ARVAE_REQUIRE(m != nullptr && n > 0, "image_vae: null model or empty batch");
    ARVAE_REQUIRE(m->n_enc >= 1 && m->n_enc <= ARVAE_MAX_LAYERS && m->n_dec >= 1 && m->n_dec <= ARVAE_MAX_LAYERS,
                  "image_vae: layer counts out of range");
    ARVAE_REQUIRE(m->zdim > 0 && m->n_reg >= 0 && m->n_reg <= 16, "image_vae: bad zdim / n_reg");
    int64_t off = 0, gmax = 0, slab = 0, lws = 0;
    auto take = [&](int64_t count) { const int64_t o = off; off += up4(count); return o; };
    auto visit = [&](const arvae_layer_t &l) {
        const arvae_link_t lk = with_batch(l, n);
        const int64_t s = arvae_link_wgrad_ws_floats(&lk);
        if (s > slab) slab = s;
        if (arvae_link_ws_floats(&lk) > lws) lws = arvae_link_ws_floats(&lk);
        if (out_elems(l, n) > gmax) gmax = out_elems(l, n);
        if (in_elems(l, n) > gmax) gmax = in_elems(l, n);
    };
    auto wide = [&](const arvae_layer_t &l, int64_t (&slot)[2]) {
        const arvae_link_t lk = with_batch(l, n);
        for (int t = 0; t < 2; ++t) slot[t] = (wide_stack(&lk) && conv64_fits(&lk, t == 1) && conv64s_fits(&lk, t == 1)) ? take(conv64s_ws_floats()) : -1;
    };
    const LayerSlots none{-1, -1, -1, -1, -1, {-1, -1}, -1, -1};
    for (int i = 0; i < ARVAE_MAX_LAYERS; ++i) L.enc[i] = L.dec[i] = none;
    for (int i = 0; i < m->n_enc; ++i) wide(m->enc[i], L.enc[i].wide);
    for (int i = 0; i < m->n_dec; ++i) wide(m->dec[i], L.dec[i].wide);
    for (int i = 0; i < m->n_enc; ++i) { L.enc[i].out = take(out_elems(m->enc[i], n)); visit(m->enc[i]); }
    for (int i = 0; i < m->n_dec; ++i) {
        L.dec[i].out = (i + 1 < m->n_dec) ? take(out_elems(m->dec[i], n)) : -1;
        visit(m->dec[i]);
    }
    visit(m->head_mu);
    visit(m->head_log_std);
    // (a layer the clustered latent block may compute itself leaves one slab per workgroup of that grid: mid_fold_slab_floats)
    const int64_t fold_slab = mid_fold_slab_floats(m, (int)n);
    auto own_slab = [&](const arvae_layer_t &l) -> int64_t {
        const arvae_link_t lk = with_batch(l, n);
        if (!(conv32_fits(&lk) || conv_c1_fits(&lk))) return -1;
        const int64_t need = arvae_link_wgrad_ws_floats(&lk);
        return take((conv32_fits(&lk) && lk.lh == 4 && fold_slab > need) ? fold_slab : need);
    };
    auto own_bits = [&](const arvae_layer_t &l, int64_t wprep) -> int64_t {
        const arvae_link_t lk = with_batch(l, n);
        const bool fast = (conv32_fits(&lk) && wprep >= 0) || (conv_c1_fits(&lk) && !l.is_up);
        return (fast && l.act == ARVAE_ACT_RELU && !l.dropout) ? take(out_elems(l, n) / 32) : -1;
    };
    int n_prep = 0;
    auto own_prep = [&](const arvae_layer_t &l) -> int64_t {
        const arvae_link_t lk = with_batch(l, n);
        return (conv32_fits(&lk) && n_prep++ < 8) ? take(conv32_prep_floats()) : -1;
    };
    for (int i = 0; i < m->n_enc; ++i) L.enc[i].wprep = own_prep(m->enc[i]);
    for (int i = 0; i < m->n_dec; ++i) L.dec[i].wprep = own_prep(m->dec[i]);
    for (int i = 0; i < m->n_enc; ++i) L.enc[i].bits = own_bits(m->enc[i], L.enc[i].wprep);
    for (int i = 0; i < m->n_dec; ++i) L.dec[i].bits = own_bits(m->dec[i], L.dec[i].wprep);
    for (int i = 0; i < m->n_enc; ++i) L.enc[i].slab = own_slab(m->enc[i]);
    for (int i = 0; i < m->n_dec; ++i) L.dec[i].slab = own_slab(m->dec[i]);
    // every layer's output gradient has its own buffer: weight gradients run on a second stream (and the Linear ones
    // at the very end), so a gradient must not be overwritten two layers later
    for (int i = 0; i < m->n_enc; ++i) L.enc[i].keep = take(out_elems(m->enc[i], n));
    for (int i = 0; i < m->n_dec; ++i) L.dec[i].keep = take(out_elems(m->dec[i], n));
    for (int i = 0; i < m->n_enc; ++i) { L.enc[i].amax = take(AMAX_N); L.enc[i].gamax = take(AMAX_N); }
    for (int i = 0; i < m->n_dec; ++i) { L.dec[i].amax = take(AMAX_N); L.dec[i].gamax = take(AMAX_N); }
    L.ga_amax = take(AMAX_N);
    L.gb_amax = take(AMAX_N);
    L.tmp_amax = take(AMAX_N);
    L.tmp2_amax = take(AMAX_N);
    const int64_t bz = n * m->zdim;
    L.log_std = take(bz);
    L.dlogits = take(out_elems(m->dec[m->n_dec - 1], n));
    L.dz_reg = take(bz);
    L.d_mu = take(bz);
    L.d_ls = take(bz);
    L.g_a = take(gmax);
    L.g_b = take(gmax);
    L.slab_floats = slab;
    L.slab = take(slab);
    L.link_ws = take(lws);               // scratch of one arvae_link_down / _up call at a time (stream-ordered)
    L.mid_prep = take(mid_prep_floats(m));   // the latent block's matrices in the layout its kernels stream (midblock.hip)
    {
        const int64_t w = mid_wide_ws_floats(m, (int)n);     // partial products of the wide Linear layers' split reductions (dense.hip)
        L.mid_wide = w > 0 ? take(w) : -1;
    }
    static_assert(sizeof(VaeFinishArgs) <= 64 * sizeof(float), "the parked finishing step's arguments fit their workspace slot");
    L.fin_args = take(64);                // a deferred finishing step's arguments (ARVAE_VAE_DEFER_FINISH, vae_finish.h)
    L.rec_ws = take(arvae_recon_ws_floats(out_elems(m->dec[m->n_dec - 1], n)));
    L.reg_ws = take(arvae_reg_loss_ws_floats(n, m->n_reg > 0 ? m->n_reg : 1));
    L.rec_out = take(4);
    L.kld_out = take(4);
    L.reg_out = take(4);
    L.total = off;
    return ARVAE_OK;
}

// The workspace as the typed pointers the passes hand to the kernels: every offset of the layout is resolved here, and only here
// (-1 -> null)
struct View {
    LayerBufs enc[ARVAE_MAX_LAYERS], dec[ARVAE_MAX_LAYERS];
    unsigned *ga_amax, *gb_amax, *tmp_amax, *tmp2_amax;
    float *log_std, *dlogits, *dz_reg, *d_mu, *d_ls, *g_a, *g_b, *slab, *link_ws, *mid_prep, *mid_wide, *rec_ws, *reg_ws, *rec_out, *kld_out, *reg_out;
    VaeFinishArgs *fin_args;

    View(float *ws, const Layout &L) {
        auto F = [&](int64_t off) { return off >= 0 ? ws + off : nullptr; };
        auto U = [&](int64_t off) { return reinterpret_cast<unsigned *>(F(off)); };
        auto layer = [&](const LayerSlots &s) {
            return LayerBufs{F(s.out), F(s.keep), F(s.slab), reinterpret_cast<uint16_t *>(F(s.bits)), F(s.wprep), {F(s.wide[0]), F(s.wide[1])},
                             U(s.amax), U(s.gamax)};
        };
        for (int i = 0; i < ARVAE_MAX_LAYERS; ++i) { enc[i] = layer(L.enc[i]); dec[i] = layer(L.dec[i]); }
        ga_amax = U(L.ga_amax); gb_amax = U(L.gb_amax); tmp_amax = U(L.tmp_amax); tmp2_amax = U(L.tmp2_amax);
        log_std = F(L.log_std); dlogits = F(L.dlogits); dz_reg = F(L.dz_reg); d_mu = F(L.d_mu); d_ls = F(L.d_ls);
        g_a = F(L.g_a); g_b = F(L.g_b);
        slab = L.slab_floats ? F(L.slab) : nullptr;      // (no layer needs the shared slab: nobody gets a pointer to zero floats)
        link_ws = F(L.link_ws); mid_prep = F(L.mid_prep); mid_wide = F(L.mid_wide);
        rec_ws = F(L.rec_ws); reg_ws = F(L.reg_ws); rec_out = F(L.rec_out); kld_out = F(L.kld_out); reg_out = F(L.reg_out);
        fin_args = reinterpret_cast<VaeFinishArgs *>(F(L.fin_args));
    }
};

// milestones (include/arvae_hip.h): record the caller's event on the pass's stream
static inline void mark(void *event, hipStream_t st) {
    if (event != nullptr) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(event), st);
}

// the last decoder layer is the single-channel transposed conv whose launch also sums the reconstruction term (conv_c1.hip
// up_c1_kernel<DIST, true>): the models a deferred finishing step exists for
static bool recon_is_fused(const arvae_image_vae_t *m) {
    const arvae_layer_t &last = m->dec[m->n_dec - 1];
    return last.is_up && last.act == ARVAE_ACT_NONE && last.dropout == 0 && conv_c1_fits(&last.link) && arvae_recon_ws_floats(0) >= 2 * 1024;
}
// ARVAE_VAE_DEFER_FINISH honoured: the forward pass parks the finishing step's arguments (its last launch stores them), the
// backward pass's first launch -- or a launch of its own right behind it -- runs it
static bool finish_deferred(const arvae_image_vae_t *m) { return (m->flags & ARVAE_VAE_DEFER_FINISH) != 0 && recon_is_fused(m); }

static arvae_operand_t plain(const float *v) { return arvae_operand_t{v, nullptr, nullptr, ARVAE_ACT_NONE}; }

// One layer of the forward pass.
struct LayerFwd {
    const arvae_layer_t *l;
    int32_t n;
    const float *params, *in;
    const uint8_t *mask;
    float *out;
    uint16_t *bits_out;                 // make_layout grants bits only to ReLU layers on the fast kernels
    float *link_ws;
    arvae_stream_t st;
    const float *wprep;
    const unsigned *in_amax;            // AMAX array of `in` or null (then one is made in tmp_amax when a kernel needs it)
    unsigned *tmp_amax;
    unsigned *out_amax;                 // where the maxima of `out` go when the kernel that runs can deliver them
    float *wide_prep;
    bool out_has;                       // result: out_amax was written
};

static int layer_forward(LayerFwd &a) {
    const arvae_layer_t &l = *a.l;
    const arvae_link_t lk = with_batch(l, a.n);
    const arvae_operand_t op = plain(a.in);
    const float *w = a.params + l.w_off, *b = bias_of(l, a.params);
    const unsigned *in_amax = a.in_amax;
    a.out_has = false;
    if (a.bits_out != nullptr) {
        hipStream_t hs = as_stream(a.st);
        a.out_has = true;
        if (conv32_fits(&lk)) {
            if (in_amax == nullptr) {
                if (int rc = conv32_amax(a.in, in_elems(l, a.n), a.tmp_amax, hs)) return rc;
                in_amax = a.tmp_amax;
            }
            return l.is_up ? conv32_up(&lk, make_operand(&op), b, 1, nullptr, nullptr, a.bits_out, a.out, hs, a.wprep, in_amax, a.out_amax)
                           : conv32_down(&lk, make_operand(&op), b, 1, nullptr, nullptr, a.bits_out, a.out, hs, a.wprep, in_amax, a.out_amax);
        }
        return conv_c1_down(&lk, make_operand(&op), w, b, 1, nullptr, nullptr, a.bits_out, a.out, hs, a.out_amax);
    }
    // the wide stride-1 convolutions (conv64s.hip runs the two-term fp16 arithmetic too): the input's maxima come along or are
    // taken once, into the input's own array (the layer's weight gradient reads them again); the row-staged kernel publishes
    // the output's
    if (conv64_fits(&lk, l.is_up != 0) && a.tmp_amax != nullptr && wide_stack(&lk)) {
        hipStream_t hs = as_stream(a.st);
        if (in_amax == nullptr && conv64s_fits(&lk, l.is_up != 0)) {
            if (int rc = conv32_amax(a.in, in_elems(l, a.n), a.tmp_amax, hs)) return rc;
            in_amax = a.tmp_amax;
        }
        a.out_has = a.out_amax != nullptr;               // (both the row-staged and the gathering kernel publish their output's maxima)
        return l.is_up ? conv64_up(&lk, make_operand(&op), w, b, l.act, a.mask, a.out, a.link_ws, hs, nullptr, in_amax, a.out_amax, a.wide_prep)
                       : conv64_down(&lk, make_operand(&op), w, b, l.act, a.mask, a.out, a.link_ws, hs, nullptr, in_amax, a.out_amax, a.wide_prep);
    }
    // the single-channel first layer of the wide stack (Conv2d(1, 64)): the same kernel arvae_link_down picks, with the maxima
    if (!l.is_up && a.out_amax != nullptr && wide_stack(&lk) && !conv64_fits(&lk, false) && single_channel_down_fits(&lk)) {
        a.out_has = true;
        return single_channel_down(&lk, make_operand(&op), w, b, l.act, a.mask, a.out, as_stream(a.st), a.out_amax);
    }
    return l.is_up ? arvae_link_up(&lk, &op, w, b, l.act, a.mask, a.out, a.link_ws, a.st)
                   : arvae_link_down(&lk, &op, w, b, l.act, a.mask, a.out, a.link_ws, a.st);
}

// One layer of the backward pass.
struct LayerBwd {
    const arvae_layer_t *l;
    int32_t n;
    const float *params;
    float *grads;
    const float *in, *out;
    const uint8_t *mask;
    const float *g;                     // gradient arriving at this layer: w.r.t. its pre-activation (g_is_pre) or w.r.t. its output
    bool g_is_pre;
    const float *g_scale;               // scalar the single-channel kernels multiply g by while loading it, or null
    // gate: when non-null, the saved ReLU output of the PRODUCER of `in`; the data gradient is then written as d_in * (gate > 0),
    // i.e. already w.r.t. the producer's pre-activation, so that the producer's dgrad and wgrad read ONE plain tensor instead of
    // re-deriving ReLU' twice.  gate_bits: the same as sign bits (relu_bits16), when the forward pass left them.
    // gate_op: the same for any activation / dropout mask of that producer (GateOp, common.h); honoured by the wide stride-1
    // convolution kernels (conv64.hip), which then also spare the next layer its in-place operand pass
    const float *gate;
    const uint16_t *gate_bits;
    const GateOp *gate_op;
    GateOp gate_store;                  // (what gate_op points to, when it is not null)
    float *d_in;                        // where the data gradient goes; null: only the weight gradient is wanted
    float *slab, *link_ws, *own_slab;
    DenseWgradBatch *defer;
    SlabReduceBatch *rdefer;
    arvae_stream_t st;
    const float *wprep;
    float *wide_prep;
    // g_amax / in_amax: AMAX arrays (amax.h) of g and of `in`, or null -- a 32-channel kernel that needs one then gets it
    // made in tmp_amax / tmp2_amax; din_amax: where the maxima of d_in go when the kernel that writes it delivers them (din_has)
    const unsigned *g_amax, *in_amax;
    unsigned *tmp_amax, *tmp2_amax, *din_amax;
    // c1_img / c1_slab / c1_job: this is the layer behind a single-channel first layer whose backward pass wants nothing but its
    // weight gradient: the paired launch of this layer computes that too and writes NO data gradient (conv32.hip, C1Wgrad);
    // c1_job->slab != nullptr afterwards says it did
    const float *c1_img;
    float *c1_slab;
    SlabJob *c1_job;
    const VaeFinishArgs *finish;        // (device pointer) the forward pass's deferred finishing step, for the launch that can carry it
    // results
    bool gated;                         // the gate was applied (a fast kernel with a gated epilogue was available)
    bool din_has;                       // din_amax was written
    bool finish_taken;                  // `finish` rode in this layer's launch
};

static int layer_backward(LayerBwd &a) {
    const arvae_layer_t &l = *a.l;
    const int32_t n = a.n;
    const arvae_link_t lk = with_batch(l, n);
    const arvae_stream_t st = a.st;
    const float *const g = a.g, *const in = a.in, *const gate = a.gate;
    const uint16_t *const gate_bits = a.gate_bits;
    float *const d_in = a.d_in;
    const unsigned *g_amax = a.g_amax, *in_amax = a.in_amax;
    a.gated = a.din_has = a.finish_taken = false;
    const bool c32 = conv32_fits(&lk) && a.wprep != nullptr && a.tmp_amax != nullptr && a.tmp2_amax != nullptr;
    auto need_g = [&]() -> int {
        if (g_amax != nullptr) return ARVAE_OK;
        g_amax = a.tmp_amax;
        return conv32_amax(g, out_elems(l, n), a.tmp_amax, as_stream(st));
    };
    auto need_in = [&]() -> int {
        if (in_amax != nullptr) return ARVAE_OK;
        in_amax = a.tmp2_amax;
        return conv32_amax(in, in_elems(l, n), a.tmp2_amax, as_stream(st));
    };
    arvae_operand_t gop = a.g_is_pre ? plain(g) : arvae_operand_t{g, a.out, a.mask, l.act};
    // The wide stride-1 convolutions gather their operands once per tap: fold the activation derivative / keep-mask into
    // the upstream gradient once, in place (it is this executor's scratch and has no other reader), and hand the data
    // gradient, the weight gradient and the bias sums ONE plain tensor instead of three tensors each (MNIST: 780 -> 520 us
    // per data-gradient launch).
    if (!a.g_is_pre && (a.mask != nullptr || l.act != ARVAE_ACT_NONE) && (conv64_fits(&lk, false) || conv64_fits(&lk, true))) {
        if (int rc = arvae_operand_apply(&gop, out_elems(l, n), const_cast<float *>(g), st)) return rc;
        gop = plain(g);
        g_amax = nullptr;                                    // (of what was there before)
    }
    const arvae_operand_t xin = plain(in);
    const float *w = a.params + l.w_off;
    float *dw = a.grads + l.w_off, *db = bias_of(l, a.grads);
    const int bias_mode = db ? (l.is_up ? 2 : 1) : 0;
    hipStream_t hs = as_stream(st);                     // (a second stream for the weight gradients measured 1-9 % slower in
                                                        // rounds 1 and 2 -- the big kernels cannot share a CU -- and was removed)
    const bool own_slab_free = a.rdefer != nullptr && a.own_slab != nullptr && a.rdefer->count < SLAB_BATCH_MAX;
    // 32-channel layers: gated data gradient and weight-gradient partials in one launch (conv32.hip, pair4_* / pair_*_wgrad_kernel)
    if (d_in != nullptr && own_slab_free && gop.y == nullptr && a.g_scale == nullptr && c32 &&
        conv32_pair_fits(&lk, l.is_up != 0, gate, gate_bits, bias_mode)) {
        SlabJob job;
        if (int rc = need_g()) return rc;
        if (int rc = need_in()) return rc;
        const bool c1 = a.c1_img != nullptr && a.c1_slab != nullptr && a.c1_job != nullptr && conv32_pair_c1_fits(&lk, l.is_up != 0, gate_bits);
        if (int rc = conv32_pair(&lk, l.is_up != 0, gop.v, in, gate, gate_bits, d_in, a.wprep, dw, db, a.own_slab, hs, &job, g_amax, in_amax,
                                  c1 ? nullptr : a.din_amax, c1 ? a.c1_img : nullptr, c1 ? a.c1_slab : nullptr, c1 ? a.c1_job : nullptr))
            return rc;
        slab_reduce_defer(a.rdefer, job);
        a.gated = true;
        a.din_has = !c1 && a.din_amax != nullptr;
        return ARVAE_OK;
    }
    const bool simple = gop.mask == nullptr && gop.act != ARVAE_ACT_SELU;
    // the single-channel forward-UP link (last decoder layer): gated data gradient and weight-gradient partials in one launch
    if (d_in != nullptr && l.is_up && gate != nullptr && simple && gop.y == nullptr && own_slab_free && conv_c1_pair_fits(&lk)) {
        Operand g_op = make_operand(&gop);
        g_op.scale = a.g_scale;
        SlabJob job;
        if (int rc = conv_c1_pair(&lk, g_op, w, gate_bits ? nullptr : gate, gate_bits, d_in, make_operand(&xin), dw, db, bias_mode, a.own_slab,
                                  hs, &job, a.din_amax, a.finish))
            return rc;
        a.finish_taken = a.finish != nullptr;
        slab_reduce_defer(a.rdefer, job);
        a.gated = true;
        a.din_has = a.din_amax != nullptr;
        return ARVAE_OK;
    }
    if (d_in != nullptr) {
        int rc;
        if (l.is_up) {                                   // forward UP  -> data gradient is a DOWN map
            if (gate != nullptr && gop.y == nullptr && c32) {
                if (int rc2 = need_g()) return rc2;
                rc = conv32_down(&lk, make_operand(&gop), nullptr, 0, gate_bits ? nullptr : gate, gate_bits, nullptr, d_in, hs, a.wprep,
                                 g_amax, a.din_amax);
                a.gated = true;
                a.din_has = a.din_amax != nullptr;
            } else if (gate != nullptr && simple && conv_c1_fits(&lk)) {
                Operand g_op = make_operand(&gop);
                g_op.scale = a.g_scale;
                rc = conv_c1_down(&lk, g_op, w, nullptr, 0, gate_bits ? nullptr : gate, gate_bits, nullptr, d_in, hs, a.din_amax);
                a.gated = true;
                a.din_has = a.din_amax != nullptr;
            } else if (a.gate_op != nullptr && !conv64_fits(&lk, false) && !conv_c1_fits(&lk) && single_channel_down_gated_fits(&lk)) {
                rc = single_channel_down_gated(&lk, make_operand(&gop), w, a.gate_op, d_in, hs, a.din_amax);
                a.gated = true;
                a.din_has = a.din_amax != nullptr && lk.n <= 1024;
            } else if (a.gate_op != nullptr && conv64s_fits(&lk, false)) {       // (the gathering kernel's scattered epilogue loses more than the operand pass costs)
                if (gop.y == nullptr && a.tmp_amax != nullptr)
                    if (int rc2 = need_g()) return rc2;
                rc = conv64_down(&lk, make_operand(&gop), w, nullptr, ARVAE_ACT_NONE, nullptr, d_in, a.link_ws, hs, a.gate_op,
                                 gop.y == nullptr ? g_amax : nullptr, a.din_amax, a.wide_prep);
                a.gated = true;
                a.din_has = a.din_amax != nullptr;
            } else {
                rc = arvae_link_down(&lk, &gop, w, nullptr, ARVAE_ACT_NONE, nullptr, d_in, a.link_ws, st);
            }
        } else {                                         // forward DOWN -> data gradient is an UP map
            if (gate != nullptr && gop.y == nullptr && c32) {
                if (int rc2 = need_g()) return rc2;
                rc = conv32_up(&lk, make_operand(&gop), nullptr, 0, gate_bits ? nullptr : gate, gate_bits, nullptr, d_in, hs, a.wprep,
                               g_amax, a.din_amax);
                a.gated = true;
                a.din_has = a.din_amax != nullptr;
            } else if (gate != nullptr && dense_fits(&lk)) {
                rc = dense_dgrad(&lk, make_operand(&gop), w, gate, d_in, hs);
                a.gated = true;
            } else if (a.gate_op != nullptr && conv64_fits(&lk, true)) {         // (conv64s.hip or the gathering kernel: both take the gate)
                // (both kernels scale a plain source by its maxima: the row-staged one and, since round 4, the gathering one)
                if (gop.y == nullptr && a.tmp_amax != nullptr)
                    if (int rc2 = need_g()) return rc2;
                rc = conv64_up(&lk, make_operand(&gop), w, nullptr, ARVAE_ACT_NONE, nullptr, d_in, a.link_ws, hs, a.gate_op,
                               gop.y == nullptr ? g_amax : nullptr, a.din_amax, a.wide_prep);
                a.gated = true;
                a.din_has = a.din_amax != nullptr;
            } else {
                rc = arvae_link_up(&lk, &gop, w, nullptr, ARVAE_ACT_NONE, nullptr, d_in, a.link_ws, st);
            }
        }
        if (rc) return rc;
    }
    // conv layers with a slab kernel and plain operands: partial sums now, reduction queued for the end of the pass
    if (own_slab_free && gop.y == nullptr && ((conv32_fits(&lk) && a.tmp_amax != nullptr && a.tmp2_amax != nullptr) || conv_c1_fits(&lk))) {
        Operand lo_op = make_operand(l.is_up ? &xin : &gop), hi_op = make_operand(l.is_up ? &gop : &xin);
        (l.is_up ? hi_op : lo_op).scale = a.g_scale;              // only the conv_c1 kernels honour it (checked by the caller)
        SlabJob job;
        if (conv32_fits(&lk)) {
            if (int rc = need_g()) return rc;
            if (int rc = need_in()) return rc;
        }
        // (the single-channel FIRST layer closes the pass: the Linear weight gradients queued so far ride in its launch, dense.hip)
        const int rc = conv32_fits(&lk) ? conv32_wgrad_partial(&lk, lo_op, hi_op, dw, db, bias_mode, a.own_slab, hs, &job,
                                                               l.is_up ? in_amax : g_amax, l.is_up ? g_amax : in_amax)
                       : (d_in == nullptr && !l.is_up && dense_wgrad_c1_fits(a.defer))
                           ? dense_wgrad_flush_with_c1(a.defer, &lk, lo_op, hi_op, dw, db, bias_mode, a.own_slab, hs, &job)
                           : conv_c1_wgrad_partial(&lk, lo_op, hi_op, dw, db, bias_mode, a.own_slab, hs, &job);
        if (rc) return rc;
        slab_reduce_defer(a.rdefer, job);
        return ARVAE_OK;
    }
    // the wide stride-1 layers' weight gradient (conv64.hip) takes the operands' maxima when they are plain tensors
    if (conv64_wgrad_fits(&lk) && wide_stack(&lk) && a.tmp_amax != nullptr && a.tmp2_amax != nullptr) {
        const bool g_plain = gop.y == nullptr;
        if (g_plain)
            if (int rc = need_g()) return rc;
        if (int rc = need_in()) return rc;
        const unsigned *ga = g_plain ? g_amax : nullptr;
        return l.is_up ? link_wgrad_conv64(&lk, make_operand(&xin), make_operand(&gop), dw, db, bias_mode, a.slab, hs, in_amax, ga)
                       : link_wgrad_conv64(&lk, make_operand(&gop), make_operand(&xin), dw, db, bias_mode, a.slab, hs, ga, in_amax);
    }
    if (l.is_up) return arvae_link_wgrad(&lk, &xin, &gop, dw, db, bias_mode, a.slab, st);
    if (a.defer != nullptr && dense_fits(&lk) && dense_wgrad_defer(a.defer, &lk, make_operand(&gop), in, dw, db)) return ARVAE_OK;
    return arvae_link_wgrad(&lk, &gop, &xin, dw, db, bias_mode, a.slab, st);
}

// Do the latent block's clustered kernels also compute the conv layers on either side of it in this pass (midblock.hip
// mid_fold_fits)?  One answer for the forward and the backward pass of a step: it depends on the model, the batch, the caller's
// flags and the workspace layout only.
static bool fold_conv_layers(const arvae_image_vae_t *m, const Layout &L, int batch, const uint8_t *const *masks, int mid_ne, int mid_nd) {
    const int e = m->n_enc - mid_ne - 1;
    return masks == nullptr && e >= 1 && mid_nd + 1 < m->n_dec && mid_fold_fits(m, batch) && L.dec[mid_nd].bits >= 0 &&
           L.enc[e].slab >= 0 && L.dec[mid_nd].slab >= 0 && L.dec[mid_nd + 1].wprep >= 0;
}

// the regulariser's dimension list as the kernels take it
static RegDims reg_dims_of(const arvae_image_vae_t *m) {
    RegDims rd;
    for (int i = 0; i < 16; ++i) rd.d[i] = i < m->n_reg ? m->reg_dims[i] : 0;
    return rd;
}

// The finishing step of a forward pass (vae_finish.h): where its inputs and outputs live is the same for every caller
struct Finish {
    const arvae_image_vae_t *m;
    const View &V;
    int32_t batch;
    int nb;                             // reconstruction partial pairs in V.rec_ws
    const float *mu, *sigma, *capacity;
    bool reg;                           // the regulariser's row partials are in V.reg_ws
    int64_t n_cols;
    float reg_scale;
    float *scalars;

    int64_t pix() const { return out_elems(m->dec[m->n_dec - 1], batch); }
    // as a launch of its own, now
    int run(hipStream_t st) const {
        return vae_finish(V.rec_ws, nb, batch, pix(), mu, sigma, m->zdim, m->beta, capacity, reg ? V.reg_ws : nullptr, n_cols, m->zdim,
                          m->reg_dims, m->n_reg, m->gamma, m->delta, reg_scale, V.dz_reg, V.rec_out, V.kld_out, V.reg_out, scalars, st);
    }
    // as arguments for a launch to park in the workspace (ARVAE_VAE_DEFER_FINISH)
    VaeFinishArgs args() const {
        return vae_finish_args(V.rec_ws, nb, batch, pix(), mu, sigma, m->zdim, m->beta, capacity, reg ? V.reg_ws : nullptr, n_cols, m->zdim,
                               m->reg_dims, m->n_reg, m->gamma, m->delta, reg_scale, V.dz_reg, V.rec_out, V.kld_out, V.reg_out, scalars, 0);
    }
};

}  // namespace arvae

using namespace arvae;

extern "C" int64_t arvae_image_vae_ws_floats(const arvae_image_vae_t *model, int32_t batch, int64_t n_cols) {
    (void)n_cols;                                            // (the layout does not depend on it)
    Layout L;
    if (make_layout(model, batch, L)) return -1;
    return L.total;
}

extern "C" int arvae_image_vae_forward(const arvae_image_vae_t *m, int32_t batch, const float *params, const float *x,
                                       const float *labels, int64_t ld_labels, const float *eps,
                                       const uint8_t *const *masks, const float *capacity, const float *z_cols,
                                       const float *lab_cols, int64_t n_cols, float reg_scale, float *ws,
                                       float *scalars, float *mu, float *sigma, float *z, float *logits,
                                       arvae_stream_t stream) {
    Layout L;
    if (int rc = make_layout(m, batch, L)) return rc;
    ARVAE_REQUIRE(params && x && eps && ws && scalars && mu && sigma && z && logits, "image_vae_forward: null pointer");
    ARVAE_REQUIRE(m->n_reg == 0 || n_cols < 0 || labels != nullptr, "image_vae_forward: labels needed for the reg loss");
    hipStream_t st = as_stream(stream);
    const View V(ws, L);
    int mi = 0;
    bool mid_prepped = false;
    int mid_ne = 0, mid_nd = 0;
    const bool mid = mid_fusable(m, &mid_ne, &mid_nd);
    int first = 0;                                           // first encoder layer the loop below still has to run
    {   // split the 32-channel conv weights once for this step's forward and backward kernels
        const float *wts[8];
        float *preps[8];
        int np = 0;
        for (int i = 0; i < m->n_enc; ++i)
            if (V.enc[i].wprep != nullptr) { wts[np] = params + m->enc[i].w_off; preps[np++] = V.enc[i].wprep; }
        for (int i = 0; i < m->n_dec; ++i)
            if (V.dec[i].wprep != nullptr) { wts[np] = params + m->dec[i].w_off; preps[np++] = V.dec[i].wprep; }
        // (together with the latent block's matrix layouts when that block runs: one prep launch per step -- or none: when
        // the first encoder layer is the single-channel convolution, the prep rides in ITS grid, conv_c1.hip)
        if (np > 0 && mid) {
            MidPrepArgs margs;
            mid_prep_args(m, params, V.mid_prep, &margs, batch);
            const arvae_layer_t &l0 = m->enc[0];
            const arvae_link_t lk0 = with_batch(l0, batch);
            static const bool no_pair = diag_env("ARVAE_NO_PAIR_PREP") != nullptr;     // diagnostic: the prep as its own launch
            if (!no_pair && m->n_enc - mid_ne > 1 && V.enc[0].bits != nullptr && V.enc[0].wprep == nullptr && !l0.is_up && conv_c1_fits(&lk0) &&
                !(masks != nullptr && l0.dropout)) {
                const arvae_operand_t op = plain(x);
                if (int rc = conv_c1_down_with_prep(&lk0, make_operand(&op), params + l0.w_off, bias_of(l0, params), 1, V.enc[0].bits,
                                                    V.enc[0].out, wts, preps, np, margs, st, V.enc[0].amax))
                    return rc;
                first = 1;
            } else if (int rc = conv32_weight_prep_with_mid(wts, preps, np, margs, st)) return rc;
            mid_prepped = true;
        } else if (int rc = conv32_weight_prep(wts, preps, np, st)) return rc;
    }
    {   // split the wide conv layers' weights, both orientations, once for this step's forward and data-gradient launches
        const float *wts[4 * ARVAE_MAX_LAYERS];
        float *outs[4 * ARVAE_MAX_LAYERS];
        int tr[4 * ARVAE_MAX_LAYERS], qs[4 * ARVAE_MAX_LAYERS], nj = 0;
        auto add = [&](const arvae_layer_t &l, const LayerBufs &b) {
            for (int t = 0; t < 2; ++t)
                if (b.wide[t] != nullptr) { wts[nj] = params + l.w_off; outs[nj] = b.wide[t]; tr[nj] = t; qs[nj] = t ? l.link.chi : l.link.clo; ++nj; }
        };
        for (int i = 0; i < m->n_enc; ++i) add(m->enc[i], V.enc[i]);
        for (int i = 0; i < m->n_dec; ++i) add(m->dec[i], V.dec[i]);
        if (int rc = conv64s_prep_batch(wts, outs, tr, qs, nj, st)) return rc;
    }
    // the conv layers on either side of the latent block inside its launches (midcluster.hip): the encoder loop stops one layer
    // earlier, the decoder loop starts one layer later
    const bool fold = mid && fold_conv_layers(m, L, batch, masks, mid_ne, mid_nd);
    const float *h = first ? V.enc[0].out : x;
    const unsigned *h_amax = first ? V.enc[0].amax : nullptr;   // AMAX array of h, when the kernel that wrote h delivered one
    // layer i of either stack through layer_forward, from h / h_amax into `out`; h_amax becomes the output's array, or null
    auto run_layer = [&](bool dec, int i, const uint8_t *mask, float *out) -> int {
        const arvae_layer_t &l = dec ? m->dec[i] : m->enc[i];
        const LayerBufs *B = dec ? V.dec : V.enc;
        LayerFwd a{};
        a.l = &l; a.n = batch; a.params = params; a.in = h; a.mask = mask; a.out = out;
        a.bits_out = B[i].bits; a.link_ws = V.link_ws; a.st = stream; a.wprep = B[i].wprep;
        // (a 32-channel layer's input keeps its AMAX array for the weight gradient: a missing one is made in the input's own slot)
        a.in_amax = h_amax; a.tmp_amax = i > 0 ? B[i - 1].amax : V.tmp_amax; a.out_amax = B[i].amax;
        a.wide_prep = B[i].wide[l.is_up ? 1 : 0];
        if (int rc = layer_forward(a)) return rc;
        h_amax = a.out_has ? B[i].amax : nullptr;
        return ARVAE_OK;
    };
    // a head on the per-layer path: a Linear layer with none of the conv layers' buffers
    auto run_head = [&](const arvae_layer_t &l, float *out) -> int {
        LayerFwd a{};
        a.l = &l; a.n = batch; a.params = params; a.in = h; a.out = out; a.link_ws = V.link_ws; a.st = stream;
        return layer_forward(a);
    };
    // encoder
    mi += first ? (m->enc[0].dropout != 0) : 0;
    const int enc_end = m->n_enc - mid_ne - (fold ? 1 : 0);
    for (int i = first; i < enc_end; ++i) {
        const uint8_t *mask = (masks != nullptr && m->enc[i].dropout) ? masks[mi] : nullptr;
        mi += m->enc[i].dropout != 0;
        // two stacked 32-channel ReLU layers (16x16 then 8x8 output) as ONE launch (conv32.hip chain_down_kernel)
        if (i + 1 < enc_end && mask == nullptr && !(masks != nullptr && m->enc[i + 1].dropout) && V.enc[i].bits != nullptr &&
            V.enc[i + 1].bits != nullptr && V.enc[i].wprep != nullptr && V.enc[i + 1].wprep != nullptr && h_amax != nullptr && !m->enc[i].is_up &&
            !m->enc[i + 1].is_up) {
            const arvae_layer_t &la = m->enc[i], &lb = m->enc[i + 1];
            const arvae_link_t lka = with_batch(la, batch), lkb = with_batch(lb, batch);
            if (conv32_down_chain_fits(&lka, &lkb)) {
                const LayerBufs &a = V.enc[i], &b = V.enc[i + 1];
                if (int rc = conv32_down_chain(&lka, &lkb, h, h_amax, bias_of(la, params), a.bits, a.out, a.wprep, a.amax, bias_of(lb, params),
                                               b.bits, b.out, b.wprep, b.amax, st))
                    return rc;
                ++i;
                h = b.out;
                h_amax = b.amax;
                continue;
            }
        }
        if (int rc = run_layer(false, i, mask, V.enc[i].out)) return rc;
        h = V.enc[i].out;
    }
    const int64_t bz = (int64_t)batch * m->zdim;
    bool heads_next = false;
    if (mid) {                                               // Linear stack + heads + reparameterisation + Linear stack: one launch
        float *enc_y[ARVAE_MAX_LAYERS], *dec_y[ARVAE_MAX_LAYERS];
        for (int i = 0; i < mid_ne; ++i) enc_y[i] = V.enc[m->n_enc - mid_ne + i].out;
        for (int i = 0; i < mid_nd; ++i) dec_y[i] = V.dec[i].out;
        MidFold mf{};
        if (fold) {
            mf.hi_e = h;                                         // the conv layer's input; its output is the block's x0
            mf.hi_d = V.dec[mid_nd].out;
            mf.hi_d_bits = reinterpret_cast<unsigned char *>(V.dec[mid_nd].bits);
            mf.hi_d_amax = V.dec[mid_nd].amax;
        }
        if (int rc = mid_forward(m, batch, params, V.mid_prep, fold ? V.enc[m->n_enc - mid_ne - 1].out : h, enc_y, dec_y, eps, mu,
                                 V.log_std, sigma, z, st, mid_prepped, V.dec[mid_nd - 1].amax, fold ? &mf : nullptr, V.mid_wide))
            return rc;
        h = fold ? V.dec[mid_nd].out : dec_y[mid_nd - 1];
        h_amax = fold ? V.dec[mid_nd].amax : V.dec[mid_nd - 1].amax;
    } else if (heads_fusable(&m->head_mu, &m->head_log_std, m->zdim)) {
        // the decoder's first Linear layer rides in the heads kernel when it can (heads.hip)
        heads_next = m->n_dec > 1 && heads_next_fusable(&m->dec[0], m->zdim) && !(masks != nullptr && m->dec[0].dropout);
        if (int rc = heads_latent_fwd(&m->head_mu, &m->head_log_std, batch, m->zdim, params, h, eps, mu, V.log_std,
                                      sigma, z, st, m, heads_next ? &m->dec[0] : nullptr, heads_next ? V.dec[0].out : nullptr))
            return rc;
    } else {
        if (m->rng_eps)                                      // no fused heads kernel for this model: draw eps first
            if (int rc = arvae_philox_normal(const_cast<float *>(eps), bz, m->rng_seed, m->rng_offset, m->rng_step,
                                             m->rng_dev_step, stream))
                return rc;
        if (int rc = run_head(m->head_mu, mu)) return rc;
        if (int rc = run_head(m->head_log_std, V.log_std)) return rc;
        if (int rc = arvae_latent_fwd(mu, V.log_std, eps, bz, sigma, z, stream)) return rc;
    }
    if (m->milestones != nullptr) mark(m->milestones->z_ready, st);   // mu / sigma / z are final: the caller's all-gather may start
    // decoder
    if (!mid) { h = heads_next ? V.dec[0].out : z; h_amax = nullptr; }
    const bool recon_fused = recon_is_fused(m);
    // the regulariser needs z and the labels only: when this rank's batch is the whole batch its workgroups ride in the grid
    // of the first decoder convolution (conv32.hip, up32x_reg_kernel) instead of a launch of their own after the decoder
    const bool reg_here = m->n_reg > 0 && n_cols >= 0;
    const bool defer_finish = finish_deferred(m) && n_cols != -2;
    bool reg_done = false;
    RegArgs reg_args{};
    if (reg_here) {
        for (int i = 0; i < m->n_reg; ++i)
            ARVAE_REQUIRE(m->reg_dims[i] >= 0 && m->reg_dims[i] < m->zdim && m->reg_dims[i] < ld_labels,
                          "image_vae_forward: reg dim %d outside z/labels", m->reg_dims[i]);
        ARVAE_REQUIRE(reg_dims_repeated(m->reg_dims, m->n_reg) < 0, "image_vae_forward: reg dim %d listed twice",
                      reg_dims_repeated(m->reg_dims, m->n_reg));
        const float *zc = z_cols != nullptr ? z_cols : z;
        const float *lc = lab_cols != nullptr ? lab_cols : labels;
        reg_args = RegArgs{z, labels, batch, zc, lc, z_cols != nullptr ? n_cols : (int64_t)batch, m->zdim, ld_labels, reg_dims_of(m),
                           m->delta, V.reg_ws, V.reg_ws + (int64_t)batch * m->n_reg};
    }
    Finish fin{m, V, batch, 0, mu, sigma, capacity, reg_here, reg_here ? reg_args.n_cols : (int64_t)batch, reg_scale, scalars};
    for (int i = mid ? mid_nd + (fold ? 1 : 0) : (heads_next ? 1 : 0); i < m->n_dec; ++i) {
        const arvae_layer_t &l = m->dec[i];
        const uint8_t *mask = (masks != nullptr && l.dropout) ? masks[mi] : nullptr;
        mi += l.dropout != 0;
        float *out = (i + 1 < m->n_dec) ? V.dec[i].out : logits;
        const arvae_link_t lk = with_batch(l, batch);
        if (reg_here && !reg_done && z_cols == nullptr && i + 1 < m->n_dec && l.is_up && l.act == ARVAE_ACT_RELU &&
            mask == nullptr && V.dec[i].bits != nullptr && V.dec[i].wprep != nullptr && h_amax != nullptr && conv32_up_reg_fits(&lk)) {
            const arvae_operand_t op = plain(h);
            if (int rc = conv32_up_reg(&lk, make_operand(&op), bias_of(l, params), V.dec[i].bits, out, V.dec[i].wprep, h_amax, V.dec[i].amax,
                                       reg_args, m->n_reg, st))
                return rc;
            reg_done = true;
            h_amax = V.dec[i].amax;
        } else if (i + 1 == m->n_dec && recon_fused) {             // last layer: logits + reconstruction partials in one kernel
            // a training step may leave the finishing step to its backward pass (ARVAE_VAE_DEFER_FINISH): this launch then parks
            // that step's arguments in the workspace and poisons the scalars (vae_finish.h)
            VaeFinishArgs fa{};
            if (defer_finish) {
                fin.nb = conv_c1_up_recon_blocks(&lk);
                fa = fin.args();
            }
            if (int rc = conv_c1_up_recon(&lk, h, params + l.w_off, bias_of(l, params), logits, x, m->recon_dist, V.rec_ws, V.dlogits, st,
                                          &fin.nb, defer_finish ? &fa : nullptr, V.fin_args))
                return rc;
            h_amax = nullptr;
        } else {
            if (int rc = run_layer(true, i, mask, out)) return rc;
        }
        h = out;
    }
    // loss terms: per-block partials of the reconstruction term and the regulariser, then one finishing workgroup
    if (!recon_fused)
        if (int rc = recon_partials(logits, x, fin.pix(), batch, m->recon_dist, V.rec_ws, V.dlogits, st, &fin.nb)) return rc;
    if (n_cols == -2) return ARVAE_OK;                       // the caller finishes the pass itself: arvae_image_vae_finish
    if (reg_here && !reg_done)
        if (int rc = reg_partials(z, labels, batch, reg_args.zc, reg_args.lc, fin.n_cols, m->zdim, ld_labels, reg_args.dims, m->n_reg, m->delta,
                                  V.reg_ws, st))
            return rc;
    if (defer_finish) return ARVAE_OK;                       // (arvae_image_vae_backward runs it: its arguments are parked in the workspace)
    return fin.run(st);
}

extern "C" int arvae_image_vae_finish(const arvae_image_vae_t *m, int32_t batch, const float *labels, int64_t ld_labels,
                                      const float *capacity, const float *z_cols, const float *lab_cols, int64_t n_cols,
                                      float reg_scale, float *ws, float *scalars, const float *mu, const float *sigma,
                                      const float *z, arvae_stream_t stream) {
    Layout L;
    if (int rc = make_layout(m, batch, L)) return rc;
    ARVAE_REQUIRE(ws && scalars && mu && sigma && z, "image_vae_finish: null pointer");
    ARVAE_REQUIRE(m->n_reg == 0 || (labels && z_cols && lab_cols && n_cols >= batch), "image_vae_finish: gathered columns needed");
    hipStream_t st = as_stream(stream);
    const View V(ws, L);
    const arvae_layer_t &last = m->dec[m->n_dec - 1];
    const arvae_link_t lk = with_batch(last, batch);
    const bool reg = m->n_reg > 0;
    // as arvae_image_vae_forward decides: the last layer's own reconstruction partials, or the stand-alone kernel's
    const Finish fin{m, V, batch, recon_is_fused(m) ? conv_c1_up_recon_blocks(&lk) : recon_partial_blocks(out_elems(last, batch)),
                     mu, sigma, capacity, reg, reg ? n_cols : (int64_t)batch, reg_scale, scalars};
    if (reg) {
        for (int i = 0; i < m->n_reg; ++i)
            ARVAE_REQUIRE(m->reg_dims[i] >= 0 && m->reg_dims[i] < m->zdim && m->reg_dims[i] < ld_labels,
                          "image_vae_finish: reg dim %d outside z/labels", m->reg_dims[i]);
        ARVAE_REQUIRE(reg_dims_repeated(m->reg_dims, m->n_reg) < 0, "image_vae_finish: reg dim %d listed twice",
                      reg_dims_repeated(m->reg_dims, m->n_reg));
        // the gathered columns index dims 0 .. zdim-1 / 0 .. ld_labels-1 like the local arrays (whole rows are gathered)
        // (a training step may leave the finishing step to its backward pass -- ARVAE_VAE_DEFER_FINISH, as in the single-rank forward
        // pass: the regulariser's launch, the last of this call, then parks that step's arguments and poisons the scalars)
        if (finish_deferred(m)) {
            const VaeFinishArgs fa = fin.args();
            return reg_partials(z, labels, batch, z_cols, lab_cols, n_cols, m->zdim, ld_labels, reg_dims_of(m), m->n_reg, m->delta, V.reg_ws, st,
                                &fa, V.fin_args);
        }
        if (int rc = reg_partials(z, labels, batch, z_cols, lab_cols, n_cols, m->zdim, ld_labels, reg_dims_of(m), m->n_reg, m->delta, V.reg_ws, st))
            return rc;
    }
    return fin.run(st);
}

extern "C" int arvae_image_vae_backward(const arvae_image_vae_t *m, int32_t batch, const float *params, float *grads,
                                        const float *x, const float *eps, const uint8_t *const *masks,
                                        const float *capacity, const float *mu, const float *sigma, const float *z,
                                        const float *logits, const float *g_loss, const float *dz_extra,
                                        int32_t reg_fused, float reg_scale, float *ws, arvae_stream_t stream) {
    Layout L;
    if (int rc = make_layout(m, batch, L)) return rc;
    ARVAE_REQUIRE(params && grads && x && eps && mu && sigma && z && logits && g_loss && ws,
                  "image_vae_backward: null pointer");
    hipStream_t st = as_stream(stream);
    const View V(ws, L);
    // AMAX array (amax.h) that belongs to a gradient buffer of this pass
    auto grad_amax = [&](const float *p) -> unsigned * {
        if (p == nullptr) return nullptr;
        for (int i = 0; i < m->n_enc; ++i) if (p == V.enc[i].keep) return V.enc[i].gamax;
        for (int i = 0; i < m->n_dec; ++i) if (p == V.dec[i].keep) return V.dec[i].gamax;
        return p == V.g_a ? V.ga_amax : p == V.g_b ? V.gb_amax : nullptr;
    };
    const unsigned *cur_amax = nullptr;                   // AMAX array of `cur`, when the kernel that wrote it delivered one
    // keep-mask index of every dropout layer, in forward order
    int enc_mask[ARVAE_MAX_LAYERS], dec_mask[ARVAE_MAX_LAYERS], mi = 0;
    for (int i = 0; i < m->n_enc; ++i) enc_mask[i] = m->enc[i].dropout ? mi++ : -1;
    for (int i = 0; i < m->n_dec; ++i) dec_mask[i] = m->dec[i].dropout ? mi++ : -1;
    auto mask_of = [&](int idx) -> const uint8_t * { return (masks != nullptr && idx >= 0) ? masks[idx] : nullptr; };

    DenseWgradBatch defer;
    defer.count = 0;
    SlabReduceBatch rdefer;
    rdefer.count = 0;
    // where the gradient for a layer's output is written: its own buffer `keep`, or (null: the gradient w.r.t. z) the ping-pong
    // buffer that does not hold the gradient being consumed
    auto grad_dst = [&](float *keep, const float *busy) -> float * {
        if (keep != nullptr) return keep;
        return busy == V.g_a ? V.g_b : V.g_a;
    };
    const int64_t pix = out_elems(m->dec[m->n_dec - 1], batch);
    const int64_t bz = (int64_t)batch * m->zdim;
    // d loss / d logits was left unscaled by the forward pass.  When the last layer runs on the conv_c1 kernels they
    // multiply by the upstream gradient while loading it; otherwise one elementwise pass makes the scaled copy.
    float *cur;
    const float *first_scale = nullptr;
    // A layer's ReLU can be folded into the data-gradient epilogue of its consumer when no dropout mask sits
    // between them; the gradient handed down is then w.r.t. the pre-activation.
    auto relu_gate = [&](const arvae_layer_t &producer, int mask_idx, const float *saved) -> const float * {
        return (producer.act == ARVAE_ACT_RELU && mask_of(mask_idx) == nullptr) ? saved : nullptr;
    };
    // the general form (any activation, dropout): used where relu_gate() has nothing to offer
    auto general_gate = [&](const arvae_layer_t &producer, int mask_idx, const float *saved, GateOp &go) -> const GateOp * {
        if (producer.act == ARVAE_ACT_NONE && mask_of(mask_idx) == nullptr) return nullptr;
        if (producer.act == ARVAE_ACT_RELU && mask_of(mask_idx) == nullptr) return nullptr;      // relu_gate covers it
        go.y = saved; go.mask = mask_of(mask_idx); go.act = producer.act;
        return &go;
    };
    bool pre = true;                                     // the last decoder layer has no activation
    // what every layer_backward call of this pass shares; `g` arrives w.r.t. the layer's pre-activation, nothing is gated
    auto common_args = [&](LayerBwd &a, const arvae_layer_t &l, const float *in, const float *g, float *d_in) {
        a = LayerBwd{};
        a.l = &l; a.n = batch; a.params = params; a.grads = grads; a.in = in; a.g = g; a.g_is_pre = true; a.d_in = d_in;
        a.slab = V.slab; a.link_ws = V.link_ws; a.defer = &defer; a.st = stream;
    };
    // layer i of the decoder / encoder: the gradient `cur` (pre, cur_amax) at its output, the data gradient into dst.  What the
    // PRODUCER of the layer's input left for it -- the saved output as the gate, its sign bits, its AMAX array -- is looked up here
    auto layer_args = [&](LayerBwd &a, bool dec, int i, float *dst) {
        const arvae_layer_t *layers = dec ? m->dec : m->enc;
        const LayerBufs *B = dec ? V.dec : V.enc;
        const int *mask_idx = dec ? dec_mask : enc_mask;
        const arvae_layer_t &l = layers[i];
        common_args(a, l, i > 0 ? B[i - 1].out : (dec ? z : x), cur, dst);
        a.out = (dec && i + 1 == m->n_dec) ? logits : B[i].out;
        a.mask = mask_of(mask_idx[i]);
        a.g_is_pre = pre;
        a.g_amax = cur_amax;
        if (i > 0) {
            a.gate = relu_gate(layers[i - 1], mask_idx[i - 1], a.in);
            a.gate_op = general_gate(layers[i - 1], mask_idx[i - 1], a.in, a.gate_store);
            a.gate_bits = a.gate != nullptr ? B[i - 1].bits : nullptr;
            // the forward pass left a valid AMAX array with the input of every 32-channel layer that ran on the fast kernels
            const arvae_link_t lk = with_batch(l, batch);
            const bool fast = B[i].bits != nullptr && B[i].wprep != nullptr;
            if (fast || (conv64s_fits(&lk, l.is_up != 0) && wide_stack(&lk))) a.in_amax = B[i - 1].amax;
        }
        a.own_slab = B[i].slab;
        a.rdefer = &rdefer;
        a.wprep = B[i].wprep;
        a.wide_prep = B[i].wide[l.is_up ? 0 : 1];
        a.tmp_amax = V.tmp_amax; a.tmp2_amax = V.tmp2_amax; a.din_amax = grad_amax(dst);
    };
    {
        const int li = m->n_dec - 1;
        const arvae_layer_t &last = m->dec[li];
        const arvae_link_t lk = with_batch(last, batch);
        const bool fold = last.is_up && conv_c1_fits(&lk) && mask_of(dec_mask[li]) == nullptr && li > 0 &&
                          relu_gate(m->dec[li - 1], dec_mask[li - 1], V.dec[li - 1].out) != nullptr && V.dec[li].slab != nullptr;
        if (fold) {
            cur = V.dlogits;
            first_scale = g_loss;
        } else {
            cur = grad_dst(V.dec[li].keep, nullptr);
            if (int rc = arvae_scale_by_scalar(g_loss, V.dlogits, pix, cur, stream)) return rc;
        }
    }
    int mid_ne = 0, mid_nd = 0;
    const bool mid = mid_fusable(m, &mid_ne, &mid_nd);
    // (as the forward pass decided: the conv layers on either side of the latent block inside its launches)
    const bool fold = mid && fold_conv_layers(m, L, batch, masks, mid_ne, mid_nd);
    // the forward pass left its finishing step (loss scalars, KL mean, the regulariser's z-gradient: the latent block below reads
    // the last two) to this call (ARVAE_VAE_DEFER_FINISH)
    bool finish_pending = finish_deferred(m);
    // decoder, last layer first (down to the latent block when that runs as one launch)
    const float *heads_next_g = nullptr;
    for (int i = m->n_dec - 1; i >= (mid ? mid_nd + (fold ? 1 : 0) : 0); --i) {
        float *dst = grad_dst(i > 0 ? V.dec[i - 1].keep : nullptr, cur);
        // the first decoder layer's data gradient (d z) is computed inside the heads kernel (heads.hip) when the gradient
        // that arrives here is already w.r.t. the layer's pre-activation: only its weight gradient is queued
        if (i == 0 && !mid && pre && m->n_dec > 1 && heads_fusable(&m->head_mu, &m->head_log_std, m->zdim) &&
            heads_next_fusable(&m->dec[0], m->zdim) && mask_of(dec_mask[0]) == nullptr) {
            heads_next_g = cur;
            dst = nullptr;
        }
        // (the last decoder layer's launch is the pass's first: it carries a deferred finishing step when it is the paired one)
        const bool carry = finish_pending && i == m->n_dec - 1;
        LayerBwd a;
        layer_args(a, true, i, dst);
        a.g_scale = i == m->n_dec - 1 ? first_scale : nullptr;
        a.finish = carry ? V.fin_args : nullptr;
        if (int rc = layer_backward(a)) return rc;
        if (carry) {
            if (!a.finish_taken)
                if (int rc = vae_finish_deferred(V.fin_args, st)) return rc;
            finish_pending = false;
        }
        pre = a.gated;
        if (heads_next_g == nullptr) { cur = dst; cur_amax = a.din_has ? grad_amax(dst) : nullptr; }
    }
    // data-parallel caller: finish the decoder's conv gradients now (their all-reduce then runs under the rest of the pass)
    const arvae_milestones *ms = m->milestones;
    bool dec_marked = false, lin_marked = false;
    if (ms != nullptr && ms->dec_grads != nullptr && defer.count == 0) {
        // (defer.count == 0: no Linear layer of the decoder went the per-layer way, so "decoder conv layers" is what is queued)
        if (int rc = slab_reduce_flush(&rdefer, st)) return rc;
        mark(ms->dec_grads, st);
        dec_marked = true;
    }
    // latent head (cur = gradient w.r.t. z from the decoder) and the two encoder heads:
    // d_hidden = W_mu^T d_mu + W_ls^T d_ls   (gated by the last encoder layer's ReLU when possible)
    const float *hidden = V.enc[m->n_enc - 1].out;
    // regulariser gradient w.r.t. z, unit upstream (scaled by g * reg_scale in the latent kernel): the forward's own
    // (reg_fused 1), or the caller's row-block evaluation against gathered columns (reg_fused 2, in dz_extra)
    const float *dz_reg = (reg_fused == 1 && m->n_reg > 0) ? V.dz_reg : reg_fused == 2 ? dz_extra : nullptr;
    if (reg_fused == 2) {
        ARVAE_REQUIRE(dz_extra != nullptr, "image_vae_backward: reg_fused 2 needs the unit regulariser gradient in dz_extra");
        dz_extra = nullptr;
    }
    const float *kl = V.kld_out + 1;                         // the KL mean the finishing step left
    const float *head_gate = relu_gate(m->enc[m->n_enc - 1], enc_mask[m->n_enc - 1], hidden);
    float *d_hidden = V.enc[m->n_enc - 1].keep;
    // a Linear layer's weight gradient from its pre-activation gradient and its input: into the grouped launch when it fits there
    auto queue_wgrad = [&](const arvae_layer_t &l, const float *g, const float *in) -> int {
        const arvae_link_t lk = with_batch(l, batch);
        float *dw = grads + l.w_off, *db = bias_of(l, grads);
        const arvae_operand_t gop = plain(g), xin = plain(in);
        if (dense_wgrad_defer(&defer, &lk, make_operand(&gop), in, dw, db)) return ARVAE_OK;
        return arvae_link_wgrad(&lk, &gop, &xin, dw, db, db ? 1 : 0, V.slab, stream);
    };
    int enc_from = m->n_enc - 1;                             // first encoder layer the per-layer loop below still has to visit
    if (mid) {
        // Linear stack of the decoder <- z <- heads <- Linear stack of the encoder: one launch (midblock.hip); it leaves each
        // layer's pre-activation gradient in that layer's keep buffer for the grouped weight-gradient launch
        const int e0 = m->n_enc - mid_ne;                    // index of the block's first encoder layer; e0 - 1 is a conv layer
        float *enc_y[ARVAE_MAX_LAYERS], *dec_y[ARVAE_MAX_LAYERS], *enc_g[ARVAE_MAX_LAYERS], *dec_g[ARVAE_MAX_LAYERS];
        for (int i = 0; i < mid_ne; ++i) { enc_y[i] = V.enc[e0 + i].out; enc_g[i] = V.enc[e0 + i].keep; }
        for (int i = 0; i < mid_nd; ++i) { dec_y[i] = V.dec[i].out; dec_g[i] = V.dec[i].keep; }
        const float *x0 = V.enc[e0 - 1].out;
        const float *gate0 = relu_gate(m->enc[e0 - 1], enc_mask[e0 - 1], x0);
        float *d_x0 = V.enc[e0 - 1].keep;
        const float *g_last = cur;                           // gradient arriving at the last Linear layer of the decoder
        MidFold mf{};
        if (fold) {
            // `cur` is the gradient at the transposed conv layer's output, left by the layer behind it: the block takes it from
            // there (it must be w.r.t. the pre-activation: that layer's data-gradient kernel gates with the sign bits the
            // forward launch wrote) and hands the gradient at the conv layer's INPUT on
            if (!pre) {
                // the layer behind it had no kernel with a gated epilogue (a layer without activation takes the per-layer link
                // kernels): fold the folded layer's ReLU into the gradient in place, as layer_backward does for the wide layers
                const arvae_layer_t &fd = m->dec[mid_nd];
                const arvae_operand_t gop{cur, V.dec[mid_nd].out, nullptr, fd.act};
                if (int rc = arvae_operand_apply(&gop, out_elems(fd, batch), cur, stream)) return rc;
                pre = true;
            }
            mf.hi_e = V.enc[e0 - 2].out;
            mf.g_hi_d = cur;
            mf.d_hi_e = V.enc[e0 - 2].keep;
            mf.d_hi_e_amax = V.enc[e0 - 2].gamax;
            mf.slab_e = V.enc[e0 - 1].slab;
            mf.slab_d = V.dec[mid_nd].slab;
        }
        if (int rc = mid_backward(m, batch, params, V.mid_prep, enc_y, dec_y, enc_g, dec_g, g_last, (pre || fold) ? 1 : 0, gate0, d_x0, eps,
                                  mu, sigma, dz_reg, dz_extra, g_loss, kl, capacity, m->beta, reg_scale, V.d_mu, V.d_ls, st,
                                  V.enc[e0 - 1].gamax, fold ? &mf : nullptr, V.mid_wide))
            return rc;
        if (fold) {                                          // the two layers' weight-gradient slabs: one per workgroup of the block's grid
            const int n_wg = (batch + 31) / 32;                  // one slab of sixteen tap blocks per cluster (reduce.h, SLAB_C32T)
            const arvae_layer_t &ce = m->enc[e0 - 1], &cd = m->dec[mid_nd];
            SlabJob je{mf.slab_e, grads + ce.w_off, bias_of(ce, grads), n_wg, SLAB_C32T, ce.b_off >= 0 ? 1 : 0};
            SlabJob jd{mf.slab_d, grads + cd.w_off, bias_of(cd, grads), n_wg, SLAB_C32T, cd.b_off >= 0 ? 2 : 0};
            ARVAE_REQUIRE(slab_reduce_defer(&rdefer, jd) && slab_reduce_defer(&rdefer, je), "image_vae_backward: too many slab reductions queued");
        }
        // weight gradients of the block's layers: (pre-activation gradient, layer input) pairs for the grouped launch
        // (the wide layers' own weight-gradient launch first: dense.hip wide_wgrad_x3_kernel, Morpho-MNIST's 2888-wide layers)
        int wide_took = 0;
        if (V.mid_wide != nullptr)
            if (int rc = mid_wide_wgrad(m, batch, params, V.mid_prep, V.mid_wide, x0, (pre && !fold) ? g_last : dec_g[mid_nd - 1], grads,
                                        st, &wide_took))
                return rc;
        for (int i = mid_nd - 1; i >= 0; --i) {
            if (i == mid_nd - 1 && (wide_took & 2)) continue;
            if (int rc = queue_wgrad(m->dec[i], (i == mid_nd - 1 && pre && !fold) ? g_last : dec_g[i], i > 0 ? dec_y[i - 1] : z)) return rc;
        }
        if (int rc = queue_wgrad(m->head_mu, V.d_mu, hidden)) return rc;
        if (int rc = queue_wgrad(m->head_log_std, V.d_ls, hidden)) return rc;
        for (int i = mid_ne - 1; i >= 0; --i) {
            if (i == 0 && (wide_took & 1)) continue;
            if (int rc = queue_wgrad(m->enc[e0 + i], enc_g[i], i > 0 ? enc_y[i - 1] : x0)) return rc;
        }
        cur = fold ? mf.d_hi_e : d_x0;
        cur_amax = grad_amax(cur);
        pre = fold ? true : gate0 != nullptr;                // (folded: gated by the conv layer's saved input inside the launch)
        enc_from = fold ? e0 - 2 : e0 - 1;
        if (ms != nullptr && ms->linear_grads != nullptr) {   // every Linear weight gradient is queued
            if (int rc = dense_wgrad_flush(&defer, st)) return rc;
            mark(ms->linear_grads, st);
            lin_marked = true;
        }
    } else if (heads_fusable(&m->head_mu, &m->head_log_std, m->zdim)) {
        if (int rc = heads_latent_bwd(&m->head_mu, &m->head_log_std, batch, m->zdim, params, heads_next_g != nullptr ? nullptr : cur,
                                      dz_reg, dz_extra, mu, sigma, eps, g_loss, kl, capacity, m->beta, reg_scale,
                                      head_gate, V.d_mu, V.d_ls, d_hidden, st,
                                      heads_next_g != nullptr ? &m->dec[0] : nullptr, heads_next_g))
            return rc;
        // weight gradients of the heads join the grouped launch
        if (int rc = queue_wgrad(m->head_mu, V.d_mu, hidden)) return rc;
        if (int rc = queue_wgrad(m->head_log_std, V.d_ls, hidden)) return rc;
        cur = d_hidden;
        cur_amax = nullptr;
        pre = head_gate != nullptr;
    } else {
        int64_t blocks = (bz + 255) / 256;
        if (blocks > 1024) blocks = 1024;
        ARVAE_LAUNCH(latent_bwd_full_kernel, dim3((unsigned)blocks), dim3(256), 0, st, cur, dz_reg, dz_extra, mu, sigma,
                           eps, g_loss, kl, capacity, m->beta, 1.f / (float)batch, reg_scale, bz,
                           V.d_mu, V.d_ls);
        if (int rc = check_launch("image_vae_backward(latent)")) return rc;
        cur = d_hidden;
        float *other = grad_dst(nullptr, cur);
        LayerBwd a;
        common_args(a, m->head_mu, hidden, V.d_mu, cur);
        if (int rc = layer_backward(a)) return rc;
        common_args(a, m->head_log_std, hidden, V.d_ls, other);
        if (int rc = layer_backward(a)) return rc;
        const int64_t hn = in_elems(m->head_mu, batch);
        int64_t blocks2 = (hn + 255) / 256;
        if (blocks2 > 2048) blocks2 = 2048;
        ARVAE_LAUNCH(add_inplace_kernel, dim3((unsigned)blocks2), dim3(256), 0, st, cur, other, head_gate, hn);
        if (int rc = check_launch("image_vae_backward(add)")) return rc;
        pre = head_gate != nullptr;
        cur_amax = nullptr;
    }
    // encoder, last layer first; the image itself needs no gradient
    // The first layer's backward pass is its weight gradient alone.  When it is the single-channel convolution and the layer behind
    // it runs the paired 16x16 launch, that launch computes it from the data gradient it holds and stores no data gradient at all
    // (conv32.hip, C1Wgrad: 67 MB less written and 67 MB less read per step at B = 512)
    SlabJob c1_job{};
    bool c1_possible = false;
    if (enc_from >= 1 && masks == nullptr && V.enc[0].slab != nullptr && V.enc[0].bits != nullptr) {
        const arvae_link_t lk0 = with_batch(m->enc[0], batch);
        c1_possible = !m->enc[0].is_up && m->enc[0].act == ARVAE_ACT_RELU && m->enc[0].dropout == 0 && conv_c1_fits(&lk0) && lk0.hh == 64 &&
                      lk0.hw == 64 && lk0.clo == 32 && m->enc[0].b_off >= 0;
    }
    for (int i = enc_from; i >= 0; --i) {
        if (i == 0 && c1_job.slab != nullptr) {                 // done inside layer 1's launch: queue its slab reduction
            c1_job.dwt = grads + m->enc[0].w_off;
            c1_job.dbias = grads + m->enc[0].b_off;
            ARVAE_REQUIRE(slab_reduce_defer(&rdefer, c1_job), "image_vae_backward: too many slab reductions queued");
            break;
        }
        float *dst = i > 0 ? grad_dst(V.enc[i - 1].keep, cur) : nullptr;
        LayerBwd a;
        layer_args(a, false, i, dst);
        if (i == 1 && c1_possible) { a.c1_img = x; a.c1_slab = V.enc[0].slab; a.c1_job = &c1_job; }
        if (int rc = layer_backward(a)) return rc;
        pre = a.gated;
        cur = dst;
        cur_amax = a.din_has ? grad_amax(dst) : nullptr;
    }
    // The two closing kernels are independent (disjoint gradients): the slab reduction streams ~55 MB from HBM while the
    // grouped Linear weight gradients are latency-bound in L2.  Side by side on a second stream they measured 22 us SLOWER
    // per step than back to back (fork / join events cost more than the overlap returns; round 2); as ONE grid with the tiles
    // dispatched first they co-reside on the CUs (dense.hip, dense_wgrad_slab_kernel: round 6).
    if (int rc = dense_wgrad_slab_flush(&defer, &rdefer, st)) return rc;
    if (ms != nullptr) {                                 // milestones with no earlier point: everything is final here
        if (!dec_marked) mark(ms->dec_grads, st);
        if (!lin_marked) mark(ms->linear_grads, st);
    }
    return ARVAE_OK;
}
