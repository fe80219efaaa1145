// Whole-model forward / backward executors for MeasureVAE (see include/arvae_hip.h, arvae_measure_vae_*): one host call
// enqueues every kernel of a pass on the caller's stream -- the GRU encoder, the latent head, the hierarchical decoder and
// all loss terms forward; the hand-chained adjoints of the same launches backward, parameter gradients accumulating straight
// into the gradient arena.  Host-side sequencing only: the math lives in the sequence / dense / loss kernels, reached through
// the entry points a per-layer caller uses (the Python path of ar-vae_amd/measure_vae.py issues the same launches one by one
// through autograd; tests/test_measure_executor.py holds the two against each other) and in the executor's own glue kernels
// (measure_kernels.h).  MvWs: one GruLayer record per GRU layer beside the buffers that belong to no layer.  MvPass: what an entry
// point derives once.  gru_fwd / gru_bwd fill a sequence descriptor from a layer record; dropout_fwd / dropout_bwd are the dropout
// in front of layer 1 of a stack; reg_and_finish is the regulariser and the finishing launch.
//
// Reference graph: measurevae/encoder.py:8-124, measurevae/decoder.py:309-525, measurevae/measure_vae.py:97-131,
// measurevae/measure_vae_trainer.py:85-140 (loss), utils/trainer.py:140 (backward).
#include "diag.h"
#include "launch.h"
#include "dense.h"
#include "regloss.h"
#include "gru_mask.h"
#include "attributes.h"
#include "rng.h"
#include "losses.h"
#include "sequence.h"
#include "measure_kernels.h"

namespace arvae {

static inline int64_t up4(int64_t v) { return (v + 3) / 4 * 4; }

static arvae_link_t dense_link(int n, int n_in, int n_out) {
    arvae_link_t l{};
    l.n = n;
    l.hh = l.hw = l.lh = l.lw = l.kh = l.kw = 1;
    l.stride = 1;
    l.chi = n_in;
    l.clo = n_out;
    return l;
}

static inline unsigned blocks_for(int64_t items, int cap = 2048) {
    const int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- workspace layout ------------------------------------------------------------------------------
// one GRU layer's buffers (the encoder's hold both directions side by side)
struct GruLayer {
    float *gi, *out, *saved;        // forward: input projection, h of every step, the recurrence's saved gates
    float *mid;                     //   layer 0: keep * mask * out, what layer 1 reads when dropping
    float *dgi, *dgh, *hprev;       // backward: gradients w.r.t. gi and W_hh h + b_hh, the state entering each step
    float *d_mid;                   //   layer 0: gradient w.r.t. mid, left by layer 1's input projection
    float *d_out;                   //   gradient w.r.t. out where it has a buffer of its own (decoder layer 1, encoder layer 0)
};
struct MvWs {
    GruLayer enc[2], beat[2], tick[2];
    // encoder
    float *ptab, *hidden, *h12, *hmu, *hls, *log_std;
    // decoder
    float *flatb, *x0b, *both, *xs, *gsm, *gib, *frws, *probs;
    int64_t *tgt;
    // loss terms
    float *dprobs, *rec_ws, *ce_out, *kld_out, *labels, *reg_ws, *reg_out, *dz_reg;
    // backward
    float *gpre, *dg_small, *tick_ws, *dx_small, *d_both, *d_x0, *d_flatb, *d_z, *d_mu, *d_ls, *d_hmu, *d_hls, *d_h12, *d_hidden;
    float *dptab, *embed_ws, *d_table, *wg_ws, *wg_long, *cs_ws;
    int64_t wg_long_floats;
};

struct MvDims {
    int b, t, nb, tpb, v, e, he, hd, z;
    int tb, rb, rt, ns;      // encoder rows T*B, beat rows nb*B, tick rows tpb*nb*B, rows of the small tick product
};

static MvDims dims_of(const arvae_measure_vae_t *m, int batch) {
    MvDims d{};
    d.b = batch; d.t = m->steps; d.nb = m->beats; d.tpb = m->ticks_per_beat; d.v = m->vocab; d.e = m->emb;
    d.he = m->enc_hidden; d.hd = m->dec_hidden; d.z = m->zdim;
    d.tb = d.t * batch; d.rb = d.nb * batch; d.rt = d.tpb * d.nb * batch; d.ns = d.v + 1 + d.rb;
    return d;
}

static int64_t carve(const arvae_measure_vae_t *m, int batch, float *base, MvWs *w) {
    const MvDims d = dims_of(m, batch);
    int64_t off = 0;
    auto take = [&](int64_t n) {
        float *p = base != nullptr ? base + off : nullptr;
        off += up4(n);
        return p;
    };
    // a layer's buffers, `units` = rows * steps * width of its output (both directions for the encoder)
    auto take_fwd = [&](GruLayer &l, int64_t gi_floats, int64_t units, bool has_mid) {
        l.gi = take(gi_floats); l.out = take(units); l.saved = take(4 * units);
        if (has_mid) l.mid = take(units);
    };
    auto take_bwd = [&](GruLayer &l, int64_t units) { l.dgi = take(3 * units); l.dgh = take(3 * units); l.hprev = take(units); };
    const int64_t TB = d.tb, RB = d.rb, RT = d.rt, B = d.b;
    w->ptab = take((int64_t)d.v * 6 * d.he);
    take_fwd(w->enc[0], TB * 6 * d.he, TB * 2 * d.he, true);
    take_fwd(w->enc[1], TB * 6 * d.he, TB * 2 * d.he, false);
    w->hidden = take(B * 4 * d.he);
    w->h12 = take(B * 4 * d.he);
    w->hmu = take(B * 2 * d.he);
    w->hls = take(B * 2 * d.he);
    w->log_std = take(B * d.z);
    w->flatb = take(B * 2 * d.hd);
    w->x0b = take(RB);
    take_fwd(w->beat[0], B * 3 * d.hd, RB * d.hd, true);          // (gi: one row block, the same input at every beat)
    take_fwd(w->beat[1], RB * 3 * d.hd, RB * d.hd, false);
    w->both = take(RB * 3 * d.hd);
    w->xs = take((int64_t)d.ns * (d.e + d.hd));
    w->gsm = take((int64_t)d.ns * 3 * d.hd);
    w->gib = take(RB * 3 * d.hd);
    w->frws = take(arvae_tick_free_run_ws_floats(d.hd));
    take_fwd(w->tick[0], RT * 3 * d.hd, RT * d.hd, true);
    take_fwd(w->tick[1], RT * 3 * d.hd, RT * d.hd, false);
    w->probs = take(RT * d.v);
    w->tgt = reinterpret_cast<int64_t *>(take(2 * RT));      // (16-byte aligned like every take: up4)
    w->dprobs = take(RT * d.v);
    w->rec_ws = take(arvae_recon_ws_floats(RT));
    w->ce_out = take(4);
    w->kld_out = take(4);
    w->labels = take(B * 4);
    w->reg_ws = take(arvae_reg_loss_ws_floats(B, m->n_reg > 0 ? m->n_reg : 1));
    w->reg_out = take(4);
    w->dz_reg = take(B * d.z);
    // backward
    w->gpre = take(RT * d.v);
    w->tick[1].d_out = take(RT * d.hd);
    take_bwd(w->tick[1], RT * d.hd);
    take_bwd(w->tick[0], RT * d.hd);
    w->tick[0].d_mid = take(RT * d.hd);
    w->dg_small = take((int64_t)d.ns * 3 * d.hd);
    w->tick_ws = take(arvae_tick_gi_bwd_ws_floats(d.v, 3 * d.hd));
    w->dx_small = take((int64_t)d.ns * (d.e + d.hd));
    w->d_both = take(RB * 3 * d.hd);
    w->beat[1].d_out = take(RB * d.hd);
    w->beat[0].d_mid = take(RB * d.hd);
    take_bwd(w->beat[1], RB * d.hd);
    take_bwd(w->beat[0], RB * d.hd);
    w->d_x0 = take(RB);
    w->d_flatb = take(B * 2 * d.hd);
    w->d_z = take(B * d.z);
    w->d_mu = take(B * d.z);
    w->d_ls = take(B * d.z);
    w->d_hmu = take(B * 2 * d.he);
    w->d_hls = take(B * 2 * d.he);
    w->d_h12 = take(B * 4 * d.he);
    w->d_hidden = take(B * 4 * d.he);
    take_bwd(w->enc[1], TB * 2 * d.he);
    take_bwd(w->enc[0], TB * 2 * d.he);
    w->enc[0].d_mid = take(TB * 2 * d.he);
    w->enc[0].d_out = take(TB * 2 * d.he);
    w->dptab = take((int64_t)d.v * 6 * d.he);
    w->embed_ws = take(arvae_embed_bwd_ws_floats(d.b, d.t, 6 * d.he, d.v));
    w->d_table = take((int64_t)d.v * d.e);
    // the whole-sequence weight gradients of the pass: the largest one's workspace (wg_ws, for one the row queue refuses), and every
    // one's row slices, kept until the one reduction at the end (wg_long).  `times` mirrors the lin_wgrad calls of
    // arvae_measure_vae_backward, whose order is the slices' order in wg_long
    const struct { int rows, n_in, n_out, times; } shapes[6] = {{d.tb, d.he, 3 * d.he, 4}, {d.tb, 2 * d.he, 6 * d.he, 1}, {d.rt, d.hd, 3 * d.hd, 3},
                                                                {d.rt, d.hd, d.v, 1}, {d.rb, d.hd, 3 * d.hd, 5}, {d.ns, d.e + d.hd, 3 * d.hd, 1}};
    int64_t wg = 0, lw = 0;
    for (const auto &q : shapes) {
        const arvae_link_t l = dense_link(q.rows, q.n_in, q.n_out);
        if (dense_wgrad_ws_floats(&l) > wg) wg = dense_wgrad_ws_floats(&l);
        lw += q.times * dense_wgrad_long_ws_floats(&l);
    }
    w->wg_ws = take(wg);
    w->wg_long_floats = lw;
    w->wg_long = take(lw);
    int64_t cs = arvae_channel_sum_ws_floats(d.v + 1, 3 * d.hd);
    if (arvae_channel_sum_ws_floats(d.rb, 1) > cs) cs = arvae_channel_sum_ws_floats(d.rb, 1);
    w->cs_ws = take(cs);
    return off;
}

static int check_model(const arvae_measure_vae_t *m, int batch, const char *what) {
    ARVAE_REQUIRE(m != nullptr && batch >= 1, "%s: null model or empty batch", what);
    ARVAE_REQUIRE(m->steps == m->beats * m->ticks_per_beat && m->steps >= 1, "%s: steps must be beats * ticks_per_beat", what);
    ARVAE_REQUIRE(arvae_gru_seq_supported(m->enc_hidden) && arvae_gru_seq_supported(m->dec_hidden),
                  "%s: hidden sizes %d / %d are not built as sequence kernels (32, 64, 128)", what, m->enc_hidden, m->dec_hidden);
    ARVAE_REQUIRE(m->vocab >= 1 && m->emb >= 1 && m->zdim >= 1, "%s: empty vocabulary / embedding / latent", what);
    ARVAE_REQUIRE(m->n_reg >= 0 && m->n_reg <= 16, "%s: at most 16 regularised dims", what);
    ARVAE_REQUIRE((int64_t)(m->vocab + 1) * 1024 + ((int64_t)m->steps * batch + 15) / 16 * 8 <= 65536,
                  "%s: vocabulary of %d notes at batch %d exceeds the segment sums' LDS", what, m->vocab, batch);
    return ARVAE_OK;
}

#define MV_TRY(expr)                 \
    do {                             \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

// ---- what one entry point derives once --------------------------------------------------------------
struct MvPass {
    const arvae_measure_vae_t *m;
    MvDims d;
    MvWs w;
    const float *P;                  // parameter arena
    float *G;                        // gradient arena (backward)
    arvae_stream_t stream;
    hipStream_t s;
    bool dropping;                   // training: the caller gave keep-masks
    float enc_keep, dec_keep;        // 1 / (1 - p); 1 when not dropping
    const uint8_t *enc_mask, *beat_mask, *tick_mask;      // dec_mask = [beat keep bytes (nb, B, Hd) | tick keep bytes (T, B, Hd)]
    // the dropout between two stacked GRU layers inside the lower layer's launches (gru_mask.h) instead of a launch of its own:
    // forward the recurrence stores the masked copy, backward it multiplies the gradient it loads by keep * mask
    bool fuse_masks;
};
static MvPass pass_of(const arvae_measure_vae_t *m, int batch, float *ws, const float *params, float *grads, const uint8_t *enc_mask,
                      const uint8_t *dec_mask, arvae_stream_t stream) {
    MvPass p{};
    p.m = m; p.d = dims_of(m, batch); p.P = params; p.G = grads; p.stream = stream; p.s = as_stream(stream);
    carve(m, batch, ws, &p.w);
    p.dropping = enc_mask != nullptr;
    p.enc_keep = p.dropping ? 1.f / (1.f - m->enc_dropout) : 1.f;
    p.dec_keep = p.dropping ? 1.f / (1.f - m->dec_dropout) : 1.f;
    p.enc_mask = enc_mask; p.beat_mask = dec_mask; p.tick_mask = p.dropping ? dec_mask + (int64_t)p.d.nb * p.d.b * p.d.hd : nullptr;
    p.fuse_masks = p.dropping && gru_seq_masks_supported() && diag_env("ARVAE_GRU_MASK_APART") == nullptr;
    return p;
}

static arvae_operand_t plain(const float *v) { return arvae_operand_t{v, nullptr, nullptr, ARVAE_ACT_NONE}; }
static arvae_operand_t gated(const float *v, const float *y, int act) { return arvae_operand_t{v, y, nullptr, act}; }

// y = act(x W^T + b) for `rows` rows
static int lin_fwd(int rows, int n_in, int n_out, const float *x, const float *w, const float *bias, int act, float *y, hipStream_t s) {
    const arvae_link_t l = dense_link(rows, n_in, n_out);
    return dense_fwd(&l, x, w, bias, act, y, s);
}
// dx = g W
static int lin_dgrad(int rows, int n_in, int n_out, const arvae_operand_t &g, const float *w, float *dx, hipStream_t s) {
    const arvae_link_t l = dense_link(rows, n_in, n_out);
    return dense_dgrad(&l, make_operand(&g), w, nullptr, dx, s);
}
// dw += g^T x, db += column sums of g: queued for the pass's one batched launch when the batch is short, else launched now
struct WgradQueues {
    DenseWgradBatch batch{};             // batch-sized layers: one launch of 32 x 32 tiles (dense_wgrad_batch_kernel)
    LongWgradQueue *rows = nullptr;      // whole-sequence layers: one row-sliced launch + one reduction
    float *ws = nullptr;                 // workspace of a long-batch gradient the row queue refuses
    WgradQueues() : rows(dense_wgrad_long_new()) {}
    ~WgradQueues() { dense_wgrad_long_delete(rows); }
};
static int lin_wgrad(WgradQueues *wq, int rows, int n_in, int n_out, const arvae_operand_t &g, const float *x, float *dw, float *db,
                     hipStream_t s) {
    const arvae_link_t l = dense_link(rows, n_in, n_out);
    DenseWgradBatch *q = &wq->batch;
    if (rows >= DENSE_SPLIT_MIN_ROWS) {
        if (dense_wgrad_long_defer(wq->rows, &l, make_operand(&g), x, dw, db)) return ARVAE_OK;
        return dense_wgrad(&l, make_operand(&g), x, dw, db, wq->ws, s);
    }
    if (dense_wgrad_defer(q, &l, make_operand(&g), x, dw, db)) return ARVAE_OK;
    if (int rc = dense_wgrad_flush(q, s)) return rc;            // the queue is full: launch what it holds, start the next one
    q->count = 0;
    return dense_wgrad_defer(q, &l, make_operand(&g), x, dw, db) ? ARVAE_OK : fail(ARVAE_E_INVALID, "measure_vae_backward: weight-gradient queue");
}

// ---- GRU sequence descriptors from a layer record ---------------------------------------------------
// one direction-less layer over `rows` rows: gi one block per step, h0 a column block of rows `h0_stride` floats wide (null: zeros)
static arvae_gru_seq_t gru_fwd(const GruLayer &l, int rows, int hidden, const float *w_hh, const float *b_hh, const float *h0,
                               int64_t h0_stride, int reverse = 0) {
    arvae_gru_seq_t g{};
    g.gi = l.gi; g.gi_tstride = (int64_t)rows * 3 * hidden;
    g.w_hh = w_hh; g.b_hh = b_hh; g.h0 = h0; g.h0_stride = h0_stride;
    g.h_all = l.out; g.h_stride = hidden; g.saved = l.saved;
    g.reverse = reverse;
    return g;
}
// its adjoint: d_out the gradient w.r.t. the layer's output (null: zeros), dh0 where the initial state's gradient lands
static arvae_gru_seq_t gru_bwd(const GruLayer &l, int hidden, const float *w_hh, const float *h0, float *dh0, int64_t h0_stride,
                               const float *d_out, int reverse = 0) {
    arvae_gru_seq_t g{};
    g.w_hh = w_hh; g.h0 = h0; g.h0_stride = h0_stride; g.h_all = l.out; g.h_stride = hidden; g.saved = l.saved;
    if (d_out != nullptr) { g.dh_all = d_out; g.dh_stride = hidden; }
    g.dgi = l.dgi; g.dgh = l.dgh; g.h_prev_out = l.hprev;
    g.dh0 = dh0; g.dh0_stride = h0_stride;
    g.reverse = reverse;
    return g;
}
// direction `dir` of encoder layer `layer`: the two directions share one input projection (rows of 6 He) and sit side by side
// in the layer's output (rows of 2 He); saved / dgh / hprev hold one direction after the other
static arvae_gru_seq_t enc_fwd(const MvPass &p, int layer, int dir) {
    const MvDims &d = p.d;
    const int He = d.he;
    arvae_gru_seq_t g = gru_fwd(p.w.enc[layer], d.b, He, p.P + p.m->enc_w_hh[layer][dir], p.P + p.m->enc_b_hh[layer][dir], nullptr, 0, dir);
    g.gi += dir * 3 * He; g.gi_tstride = (int64_t)d.b * 6 * He; g.gi_rstride = 6 * He;
    g.h_all += dir * He; g.h_stride = 2 * He;
    g.saved += (int64_t)dir * d.tb * 4 * He;
    g.h_fin = p.w.hidden + (2 * layer + dir) * He;      // h_n of nn.GRU: (l0 fwd, l0 rev, l1 fwd, l1 rev)
    g.h_fin_stride = 4 * He;
    return g;
}
static arvae_gru_seq_t enc_bwd(const MvPass &p, int layer, int dir, const float *d_out) {
    const MvDims &d = p.d;
    const int He = d.he;
    arvae_gru_seq_t g = gru_bwd(p.w.enc[layer], He, p.P + p.m->enc_w_hh[layer][dir], nullptr, nullptr, 0, d_out, dir);
    g.h_all += dir * He; g.h_stride = 2 * He;
    g.saved += (int64_t)dir * d.tb * 4 * He;
    if (d_out != nullptr) { g.dh_all += dir * He; g.dh_stride = 2 * He; }
    g.dh_last = p.w.d_hidden + (2 * layer + dir) * He;  // the final states' gradients enter each direction at its last processed step
    g.dh_last_stride = 4 * He;
    g.dgi += dir * 3 * He; g.dgi_rstride = 6 * He;
    g.dgh += (int64_t)dir * d.tb * 3 * He;
    g.h_prev_out += (int64_t)dir * d.tb * He;
    return g;
}

// ---- the dropout in front of layer 1 of a stack ------------------------------------------------------
// fused into layer 0's recurrence (gru_mask.h): keep bytes ordered (step, row, `width` units); h_masked the copy the forward
// recurrence stores (null backward: the recurrence scales the gradient it loads)
static GruSeqMask time_major_mask(const MvPass &p, const uint8_t *mask, float keep, int width, float *h_masked) {
    return GruSeqMask{mask, keep, h_masked, h_masked != nullptr ? width : 0, (int64_t)p.d.b * width, width, 0, 0};
}
// the tick stack's: its sequences' rows are (beat, measure) over ticks-in-beat steps, the keep bytes are ordered
// (tick = tpb * beat + j, measure) -- groups of B rows, one beat apart
static GruSeqMask tick_stack_mask(const MvPass &p, float *h_masked) {
    GruSeqMask g = time_major_mask(p, p.tick_mask, p.dec_keep, p.d.hd, h_masked);
    g.gstride = (int64_t)p.d.tpb * p.d.b * p.d.hd;
    g.group = p.d.b;
    return g;
}
// as a launch of its own: y = keep * mask * x over `count` floats (tick: x in the tick sequences' row order)
static int scale_mask_apart(const MvPass &p, const float *x, const uint8_t *mask, float keep, int64_t count, bool tick, float *y) {
    if (!tick) return arvae_scale_mask(x, mask, keep, count, 0, y, p.stream);
    const MvDims &d = p.d;
    ARVAE_LAUNCH(scale_mask_tick_kernel, dim3(blocks_for(count / 4)), dim3(256), 0, p.s, x, mask, keep, d.b, d.nb, d.tpb, d.hd / 4, y);
    return check_launch("scale_mask_tick_kernel");
}
// forward, after layer 0's launch: -> what layer 1's input projection reads.  Not dropping: layer 0's output; else its masked copy,
// which the recurrence stored itself when the masks are fused
static int dropout_fwd(const MvPass &p, const GruLayer &lo, const uint8_t *mask, float keep, int64_t count, bool tick, const float **reads) {
    *reads = p.dropping ? lo.mid : lo.out;
    if (!p.dropping || p.fuse_masks) return ARVAE_OK;
    return scale_mask_apart(p, lo.out, mask, keep, count, tick, lo.mid);
}
// backward, before layer 0's launch: -> what its recurrence reads as the gradient of its output.  lo.d_mid (left by layer 1's input
// projection) itself when not dropping or fused, else its masked copy in `apart`
static int dropout_bwd(const MvPass &p, const GruLayer &lo, const uint8_t *mask, float keep, int64_t count, bool tick, float *apart,
                       const float **reads) {
    *reads = lo.d_mid;
    if (!p.dropping || p.fuse_masks) return ARVAE_OK;
    *reads = apart;
    return scale_mask_apart(p, lo.d_mid, mask, keep, count, tick, apart);
}

// ---- regulariser + the pass's ONE finishing launch: the partial sums, beta-KL, the regulariser's gradient and the pass's scalars.
// The regulariser pairs this rank's rows (z, lab) with `n_cols` columns (z_cols, lab_cols: the same rows, or every rank's gathered)
static int reg_and_finish(const MvPass &p, const char *what, int nb, const float *capacity, const float *z, const float *lab,
                          const float *z_cols, const float *lab_cols, int64_t n_cols, float reg_scale, const float *mu, const float *sigma,
                          float *scalars) {
    const arvae_measure_vae_t *m = p.m;
    const MvDims &d = p.d;
    const MvWs &w = p.w;
    if (m->n_reg > 0) {
        RegDims rd;
        for (int i = 0; i < 16; ++i) rd.d[i] = i < m->n_reg ? m->reg_dims[i] : 0;
        for (int i = 0; i < m->n_reg; ++i)
            ARVAE_REQUIRE(m->reg_dims[i] >= 0 && m->reg_dims[i] < d.z && m->reg_dims[i] < 4, "%s: regularised dim %d outside z / the attributes",
                          what, m->reg_dims[i]);
        ARVAE_REQUIRE(reg_dims_repeated(m->reg_dims, m->n_reg) < 0, "%s: regularised dim %d listed twice", what,
                      reg_dims_repeated(m->reg_dims, m->n_reg));
        MV_TRY(reg_partials(z, lab, d.b, z_cols, lab_cols, n_cols, d.z, 4, rd, m->n_reg, m->delta, w.reg_ws, p.s));
    }
    return vae_finish(w.rec_ws, nb, d.b, d.rt, mu, sigma, d.z, m->beta, capacity, m->n_reg > 0 ? w.reg_ws : nullptr, n_cols, d.z, m->reg_dims,
                      m->n_reg, m->gamma, m->delta, reg_scale, w.dz_reg, w.ce_out, w.kld_out, w.reg_out, scalars, p.s, d.rt);
}

}  // namespace arvae

using namespace arvae;

extern "C" int64_t arvae_measure_vae_ws_floats(const arvae_measure_vae_t *model, int32_t batch) {
    if (check_model(model, batch, "measure_vae_ws_floats") != ARVAE_OK) return -1;
    MvWs w{};
    return carve(model, batch, nullptr, &w);
}

extern "C" int arvae_measure_vae_forward(const arvae_measure_vae_t *m, int32_t batch, const float *params, const int64_t *score,
                                         float *eps, uint8_t *enc_mask, uint8_t *dec_mask, int32_t teacher_forced,
                                         const float *capacity, const arvae_measure_tables_t *tables, float *ws, float *scalars,
                                         float *mu, float *sigma, float *z, int64_t *tokens, float *labels, int32_t defer_finish,
                                         arvae_stream_t stream) {
    MV_TRY(check_model(m, batch, "measure_vae_forward"));
    ARVAE_REQUIRE(params && score && eps && ws && scalars && mu && sigma && z && tokens, "measure_vae_forward: null pointer");
    ARVAE_REQUIRE((enc_mask == nullptr) == (dec_mask == nullptr), "measure_vae_forward: give both keep-masks (training) or neither (evaluation)");
    ARVAE_REQUIRE(m->n_reg == 0 || tables != nullptr, "measure_vae_forward: the regulariser needs the attribute tables");
    ARVAE_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "measure_vae_forward: workspace must be 16-byte aligned");
    ARVAE_REQUIRE(enc_mask == nullptr || (m->enc_dropout >= 0.f && m->enc_dropout < 1.f && m->dec_dropout >= 0.f && m->dec_dropout < 1.f),
                  "measure_vae_forward: dropout probabilities must be in [0, 1)");
    const MvPass p = pass_of(m, batch, ws, params, nullptr, enc_mask, dec_mask, stream);
    const MvDims &d = p.d;
    const MvWs &w = p.w;
    const float *P = p.P;
    const int He = d.he, Hd = d.hd;
    hipStream_t s = p.s;

    // ---- draws (csrc/rng.h): keep-masks and eps exactly as ops.keep_mask / ops.normal_noise make them, in the Python path's order
    if (m->rng_draw) {                                         // one launch (rng.hip: philox_draws)
        int kind[3], n = 0;
        void *out[3];
        int64_t cnt[3];
        float keep[3];
        uint32_t off[3];
        auto add = [&](int k, void *o, int64_t c, float kp, uint32_t of) { kind[n] = k; out[n] = o; cnt[n] = c; keep[n] = kp; off[n] = of; ++n; };
        if (p.dropping) add(1, enc_mask, (int64_t)d.tb * 2 * He, 1.f - m->enc_dropout, m->rng_offset[0]);
        add(0, eps, (int64_t)d.b * d.z, 1.f, m->rng_offset[1]);
        if (p.dropping) add(1, dec_mask, (int64_t)(d.nb + d.t) * d.b * Hd, 1.f - m->dec_dropout, m->rng_offset[2]);
        MV_TRY(philox_draws(n, kind, out, cnt, keep, off, m->rng_seed, m->rng_step, m->rng_dev_step, s));
    }

    // ---- encoder (encoder.py:108-124): layer 0's input projection by lookup, both directions side by side
    MV_TRY(lin_fwd(d.v, d.e, 6 * He, P + m->enc_table, P + m->enc_w_ih[0], P + m->enc_b_ih[0], ARVAE_ACT_NONE, w.ptab, s));
    // (the beat RNN's constant input -- a function of the parameters alone -- rides in this lookup's grid: attributes.h)
    const BeatInput bi{P + m->b0, P + m->beat_w_ih[0], P + m->beat_b_ih[0], d.b, 3 * Hd, d.rb, w.x0b, w.beat[0].gi};
    int beat_rc = ARVAE_OK;
    const bool beat_done = embed_fwd_with_beat(score, w.ptab, d.b, d.t, 6 * He, d.v, 1, w.enc[0].gi, bi, s, &beat_rc);
    if (beat_done) MV_TRY(beat_rc);
    else MV_TRY(arvae_embed_fwd(score, w.ptab, d.b, d.t, 6 * He, d.v, 1, w.enc[0].gi, stream));
    for (int layer = 0; layer < 2; ++layer) {
        if (layer == 1) {
            const float *src;
            MV_TRY(dropout_fwd(p, w.enc[0], enc_mask, p.enc_keep, (int64_t)d.tb * 2 * He, false, &src));
            MV_TRY(lin_fwd(d.tb, 2 * He, 6 * He, src, P + m->enc_w_ih[1], P + m->enc_b_ih[1], ARVAE_ACT_NONE, w.enc[1].gi, s));
        }
        arvae_gru_seq_t q[2];
        GruSeqMask qm[2] = {};
        for (int dir = 0; dir < 2; ++dir) {
            q[dir] = enc_fwd(p, layer, dir);
            if (layer == 0 && p.fuse_masks)                   // keep bytes (t, b, 2 He), this direction's half
                qm[dir] = time_major_mask(p, enc_mask + dir * He, p.enc_keep, 2 * He, w.enc[0].mid + dir * He);
        }
        MV_TRY(gru_seq_fwd_masked(q, qm, 2, d.t, d.b, He, stream));
    }
    // the two heads' first layers as one product, then mu / log_std and the reparameterised sample
    MV_TRY(lin_fwd(d.b, 4 * He, 4 * He, w.hidden, P + m->head_w0, P + m->head_b0, ARVAE_ACT_SELU, w.h12, s));
    if (measure_heads_fit(2 * He, d.z)) {                    // one launch (measure_heads_fwd_kernel)
        MeasureHeadsFwd hf{w.h12, P + m->mean_w2, P + m->mean_b2, P + m->lstd_w2, P + m->lstd_b2, eps, w.hmu, w.hls, mu, w.log_std, sigma, z,
                           d.b, 2 * He, d.z};
        const int lds = (MH_ROWS * 4 * He + 2 * d.z * (2 * He + 4) + MH_ROWS * 64) * 4;
        launch_lds<measure_heads_fwd_kernel>(dim3((d.b + MH_ROWS - 1) / MH_ROWS), dim3(256), lds, s, hf);
        MV_TRY(check_launch("measure_heads_fwd_kernel"));
    } else {
        MV_TRY(arvae_split_cols(w.h12, d.b, 2 * He, 2 * He, w.hmu, w.hls, 0, stream));
        MV_TRY(lin_fwd(d.b, 2 * He, d.z, w.hmu, P + m->mean_w2, P + m->mean_b2, ARVAE_ACT_NONE, mu, s));
        MV_TRY(lin_fwd(d.b, 2 * He, d.z, w.hls, P + m->lstd_w2, P + m->lstd_b2, ARVAE_ACT_NONE, w.log_std, s));
        MV_TRY(arvae_latent_fwd(mu, w.log_std, eps, (int64_t)d.b * d.z, sigma, z, stream));
    }

    // ---- beat RNN (decoder.py:436-457): the same input b_0 at every beat; initial states = flatb.view(B, 2, H)
    MV_TRY(lin_fwd(d.b, d.z, 2 * Hd, z, P + m->z2beat_w, P + m->z2beat_b, ARVAE_ACT_SELU, w.flatb, s));
    if (!beat_done) {
        ARVAE_LAUNCH(beat_input_kernel, dim3(blocks_for((int64_t)d.b * 3 * Hd + d.rb)), dim3(256), 0, s, bi);
        MV_TRY(check_launch("beat_input_kernel"));
    }
    arvae_gru_seq_t g = gru_fwd(w.beat[0], d.b, Hd, P + m->beat_w_hh[0], P + m->beat_b_hh[0], w.flatb, 2 * Hd);
    g.gi_tstride = 0;                                         // one block of gi, reused every step
    GruSeqMask gm = p.fuse_masks ? time_major_mask(p, p.beat_mask, p.dec_keep, Hd, w.beat[0].mid) : GruSeqMask{};
    MV_TRY(gru_seq_fwd_masked(&g, &gm, 1, d.nb, d.b, Hd, stream));
    const float *midb;
    MV_TRY(dropout_fwd(p, w.beat[0], p.beat_mask, p.dec_keep, (int64_t)d.rb * Hd, false, &midb));
    MV_TRY(lin_fwd(d.rb, Hd, 3 * Hd, midb, P + m->beat_w_ih[1], P + m->beat_b_ih[1], ARVAE_ACT_NONE, w.beat[1].gi, s));
    g = gru_fwd(w.beat[1], d.b, Hd, P + m->beat_w_hh[1], P + m->beat_b_hh[1], w.flatb + Hd, 2 * Hd);
    MV_TRY(arvae_gru_seq_fwd(&g, 1, d.nb, d.b, Hd, stream));

    // ---- tick RNN (decoder.py:459-525): the four beats as one 6-step sequence over beats*batch rows
    MV_TRY(lin_fwd(d.rb, Hd, 3 * Hd, w.beat[1].out, P + m->tick_init_w, P + m->tick_init_b, ARVAE_ACT_SELU, w.both, s));
    // its columns: [layer-0 initial state | layer-1 initial state | beat embedding], read in place through row strides
    const float *h0t0 = w.both, *h0t1 = w.both + Hd, *beat_emb = w.both + 2 * Hd;
    const int64_t both_ld = 3 * Hd;
    // layer 0's input projection by lookup: W_ih0 applied once to the vocabulary's embeddings, x_0 and the beat embeddings
    MV_TRY(arvae_tick_rows_fwd(P + m->dec_table, P + m->x0, beat_emb, both_ld, d.v, d.e, Hd, d.rb, w.xs, stream));
    MV_TRY(lin_fwd(d.ns, d.e + Hd, 3 * Hd, w.xs, P + m->tick_w_ih[0], nullptr, ARVAE_ACT_NONE, w.gsm, s));
    if (!teacher_forced) {
        // argmax feedback (not differentiated, decoder.py:506-516): the same small product holds the note table's and the beat
        // embeddings' projections the free-running launch reads
        ARVAE_REQUIRE(arvae_tick_free_run_supported(Hd, d.v), "measure_vae_forward: free-running decoder not built for hidden %d / %d notes",
                      Hd, d.v);
        ARVAE_LAUNCH(add_bias_rows_kernel, dim3(blocks_for((int64_t)d.rb * 3 * Hd / 4)), dim3(256), 0, s,
                     reinterpret_cast<const float4 *>(w.gsm + (int64_t)(d.v + 1) * 3 * Hd),
                     reinterpret_cast<const float4 *>(P + m->tick_b_ih[0]), (int64_t)d.rb, 3 * Hd / 4, reinterpret_cast<float4 *>(w.gib));
        MV_TRY(check_launch("add_bias_rows_kernel"));
        arvae_tick_weights_t tw{P + m->tick_w_hh[0], P + m->tick_b_hh[0], P + m->tick_w_ih[1], P + m->tick_b_ih[1],
                                P + m->tick_w_hh[1], P + m->tick_b_hh[1], P + m->out_w, P + m->out_b};
        MV_TRY(arvae_tick_free_run(&tw, h0t0, h0t1, both_ld, w.gib, w.gsm, p.tick_mask, p.dec_keep, d.b, d.nb, d.tpb, Hd, d.v, tokens, w.frws, stream));
    }
    // (teacher forcing: the notes fed back are the score's; their copy into `tokens` rides in the lookup launch)
    if (teacher_forced) {
        ARVAE_REQUIRE(tokens != score, "measure_vae_forward: tokens must not alias the score");
        MV_TRY(tick_gi_fwd_copy(w.gsm, score, P + m->tick_b_ih[0], d.b, d.nb, d.tpb, d.v, 3 * Hd, w.tick[0].gi, tokens, s));
    } else {
        MV_TRY(arvae_tick_gi_fwd(w.gsm, tokens, P + m->tick_b_ih[0], d.b, d.nb, d.tpb, d.v, 3 * Hd, w.tick[0].gi, stream));
    }
    g = gru_fwd(w.tick[0], d.rb, Hd, P + m->tick_w_hh[0], P + m->tick_b_hh[0], h0t0, both_ld);
    gm = p.fuse_masks ? tick_stack_mask(p, w.tick[0].mid) : GruSeqMask{};
    MV_TRY(gru_seq_fwd_masked(&g, &gm, 1, d.tpb, d.rb, Hd, stream));
    const float *midt;
    MV_TRY(dropout_fwd(p, w.tick[0], p.tick_mask, p.dec_keep, (int64_t)d.rt * Hd, true, &midt));
    MV_TRY(lin_fwd(d.rt, Hd, 3 * Hd, midt, P + m->tick_w_ih[1], P + m->tick_b_ih[1], ARVAE_ACT_NONE, w.tick[1].gi, s));
    g = gru_fwd(w.tick[1], d.rb, Hd, P + m->tick_w_hh[1], P + m->tick_b_hh[1], h0t1, both_ld);
    MV_TRY(arvae_gru_seq_fwd(&g, 1, d.tpb, d.rb, Hd, stream));
    MV_TRY(lin_fwd(d.rt, Hd, d.v, w.tick[1].out, P + m->out_w, P + m->out_b, ARVAE_ACT_RELU, w.probs, s));

    // ---- loss terms (measure_vae_trainer.py:85-140): cross entropy over the 24*B rows (in the sequence launches' row order, targets
    // looked up through it), the attribute labels and the regulariser's pair sums, then the finishing launch (reg_and_finish)
    int nb = 0;
    float *lab = labels != nullptr ? labels : w.labels;
    // (the attribute labels -- a function of the score alone -- ride in the cross-entropy launch's grid: attributes.h)
    const AttrArgs attr{score, d.b, d.t, tables != nullptr ? tables->midi_lut : nullptr, tables != nullptr ? tables->is_note : nullptr,
                        tables != nullptr ? tables->is_density_note : nullptr, d.v, tables != nullptr ? tables->rhythm_weights : nullptr,
                        tables != nullptr ? tables->rhythm_norm : 1.f, m->n_reg > 0 ? lab : nullptr};
    MV_TRY(token_recon_partials(w.probs, score, d.b, d.nb, d.tpb, d.v, w.rec_ws, w.dprobs, s, &nb, &attr));
    if (defer_finish) return ARVAE_OK;                   // data parallel: arvae_measure_vae_finish, once z and the labels are gathered
    return reg_and_finish(p, "measure_vae_forward", nb, capacity, z, lab, z, lab, d.b, 1.f, mu, sigma, scalars);
}

extern "C" int arvae_measure_vae_finish(const arvae_measure_vae_t *m, int32_t batch, const float *capacity, const float *z_cols,
                                        const float *lab_cols, int64_t n_cols, float reg_scale, float *ws, float *scalars, const float *mu,
                                        const float *sigma, const float *z, const float *labels, arvae_stream_t stream) {
    MV_TRY(check_model(m, batch, "measure_vae_finish"));
    ARVAE_REQUIRE(ws && scalars && mu && sigma && z, "measure_vae_finish: null pointer");
    ARVAE_REQUIRE(m->n_reg == 0 || (z_cols && lab_cols && labels && n_cols >= batch), "measure_vae_finish: the regulariser needs the gathered columns");
    const MvPass p = pass_of(m, batch, ws, nullptr, nullptr, nullptr, nullptr, stream);
    return reg_and_finish(p, "measure_vae_finish", token_recon_blocks(p.d.rt), capacity, z, labels, z_cols, lab_cols, n_cols, reg_scale, mu,
                          sigma, scalars);
}

extern "C" int arvae_measure_vae_backward(const arvae_measure_vae_t *m, int32_t batch, const float *params, float *grads,
                                          const int64_t *score, const float *eps, const uint8_t *enc_mask, const uint8_t *dec_mask,
                                          const float *capacity, const float *mu, const float *sigma, const float *z,
                                          const int64_t *tokens, const float *scalars, const float *g_loss, float reg_scale, float *ws,
                                          arvae_stream_t stream) {
    MV_TRY(check_model(m, batch, "measure_vae_backward"));
    ARVAE_REQUIRE(params && grads && score && eps && mu && sigma && z && tokens && scalars && g_loss && ws, "measure_vae_backward: null pointer");
    ARVAE_REQUIRE((enc_mask == nullptr) == (dec_mask == nullptr), "measure_vae_backward: give both keep-masks or neither");
    const MvPass p = pass_of(m, batch, ws, params, grads, enc_mask, dec_mask, stream);
    const MvDims &d = p.d;
    const MvWs &w = p.w;
    const float *P = p.P;
    float *G = p.G;
    const int He = d.he, Hd = d.hd;
    hipStream_t s = p.s;
    WgradQueues queue;
    dense_wgrad_long_begin(queue.rows, w.wg_long, w.wg_long_floats);
    queue.ws = w.wg_ws;

    // ---- note projection: d probs (cross entropy, unit upstream) times the upstream scalar, through the ReLU
    const int64_t np = (int64_t)d.rt * d.v;
    if (np % 4 == 0)
        ARVAE_LAUNCH(relu_gate_scale_kernel, dim3(blocks_for(np / 4)), dim3(256), 0, s, w.dprobs, w.probs, g_loss, np / 4, w.gpre);
    else
        ARVAE_LAUNCH(relu_gate_scale1_kernel, dim3(blocks_for(np)), dim3(256), 0, s, w.dprobs, w.probs, g_loss, np, w.gpre);
    MV_TRY(check_launch("relu_gate_scale_kernel"));
    MV_TRY(lin_dgrad(d.rt, Hd, d.v, plain(w.gpre), P + m->out_w, w.tick[1].d_out, s));
    MV_TRY(lin_wgrad(&queue, d.rt, Hd, d.v, plain(w.gpre), w.tick[1].out, G + m->out_w, G + m->out_b, s));

    // ---- tick RNN, layer 1 then layer 0: the initial states' gradients land in their columns of d_both
    const GruLayer &t0 = w.tick[0], &t1 = w.tick[1];
    arvae_gru_seq_t g = gru_bwd(t1, Hd, P + m->tick_w_hh[1], w.both + Hd, w.d_both + Hd, 3 * Hd, t1.d_out);
    MV_TRY(arvae_gru_seq_bwd(&g, 1, d.tpb, d.rb, Hd, stream));
    MV_TRY(lin_wgrad(&queue, d.rt, Hd, 3 * Hd, plain(t1.dgh), t1.hprev, G + m->tick_w_hh[1], G + m->tick_b_hh[1], s));
    MV_TRY(lin_dgrad(d.rt, Hd, 3 * Hd, plain(t1.dgi), P + m->tick_w_ih[1], t0.d_mid, s));
    MV_TRY(lin_wgrad(&queue, d.rt, Hd, 3 * Hd, plain(t1.dgi), p.dropping ? t0.mid : t0.out, G + m->tick_w_ih[1], G + m->tick_b_ih[1], s));
    const float *d_out0t;                                     // (apart: layer 1's output gradient is spent, its buffer takes the product)
    MV_TRY(dropout_bwd(p, t0, p.tick_mask, p.dec_keep, (int64_t)d.rt * Hd, true, t1.d_out, &d_out0t));
    GruSeqMask gm = p.fuse_masks ? tick_stack_mask(p, nullptr) : GruSeqMask{};
    g = gru_bwd(t0, Hd, P + m->tick_w_hh[0], w.both, w.d_both, 3 * Hd, d_out0t);
    MV_TRY(gru_seq_bwd_masked(&g, &gm, 1, d.tpb, d.rb, Hd, stream));
    MV_TRY(lin_wgrad(&queue, d.rt, Hd, 3 * Hd, plain(t0.dgh), t0.hprev, G + m->tick_w_hh[0], G + m->tick_b_hh[0], s));
    // layer 0's input projection: per-tick gradients summed per previous note and per beat row, then the small product's adjoints
    MV_TRY(arvae_tick_gi_bwd(t0.dgi, tokens, d.b, d.nb, d.tpb, d.v, 3 * Hd, w.dg_small, w.tick_ws, stream));
    // (every tick row carries the bias once and exactly one note entry: the bias gradient is the column sum of the note rows)
    // (its column sums -- the bias gradient -- wait for the pass's closing launch: grad_tail_kernel)
    MV_TRY(lin_wgrad(&queue, d.ns, d.e + Hd, 3 * Hd, plain(w.dg_small), w.xs, G + m->tick_w_ih[0], nullptr, s));
    MV_TRY(lin_dgrad(d.ns, d.e + Hd, 3 * Hd, plain(w.dg_small), P + m->tick_w_ih[0], w.dx_small, s));
    MV_TRY(arvae_tick_rows_bwd(w.dx_small, d.v, d.e, Hd, d.rb, G + m->dec_table, G + m->x0, w.d_both + 2 * Hd, 3 * Hd, stream));
    // initial states + beat-embedding input: one SELU layer on the beat outputs (d_both is complete: three column blocks)
    const GruLayer &b0 = w.beat[0], &b1 = w.beat[1];
    MV_TRY(lin_dgrad(d.rb, Hd, 3 * Hd, gated(w.d_both, w.both, ARVAE_ACT_SELU), P + m->tick_init_w, b1.d_out, s));
    MV_TRY(lin_wgrad(&queue, d.rb, Hd, 3 * Hd, gated(w.d_both, w.both, ARVAE_ACT_SELU), b1.out, G + m->tick_init_w, G + m->tick_init_b, s));

    // ---- beat RNN, layer 1 then layer 0 (their batch-sized weight gradients wait in the queue: separate buffers per layer)
    g = gru_bwd(b1, Hd, P + m->beat_w_hh[1], w.flatb + Hd, w.d_flatb + Hd, 2 * Hd, b1.d_out);
    MV_TRY(arvae_gru_seq_bwd(&g, 1, d.nb, d.b, Hd, stream));
    MV_TRY(lin_wgrad(&queue, d.rb, Hd, 3 * Hd, plain(b1.dgh), b1.hprev, G + m->beat_w_hh[1], G + m->beat_b_hh[1], s));
    MV_TRY(lin_dgrad(d.rb, Hd, 3 * Hd, plain(b1.dgi), P + m->beat_w_ih[1], b0.d_mid, s));
    MV_TRY(lin_wgrad(&queue, d.rb, Hd, 3 * Hd, plain(b1.dgi), p.dropping ? b0.mid : b0.out, G + m->beat_w_ih[1], G + m->beat_b_ih[1], s));
    const float *d_out0b;
    MV_TRY(dropout_bwd(p, b0, p.beat_mask, p.dec_keep, (int64_t)d.rb * Hd, false, b1.d_out, &d_out0b));
    gm = p.fuse_masks ? time_major_mask(p, p.beat_mask, p.dec_keep, Hd, nullptr) : GruSeqMask{};
    g = gru_bwd(b0, Hd, P + m->beat_w_hh[0], w.flatb, w.d_flatb, 2 * Hd, d_out0b);
    MV_TRY(gru_seq_bwd_masked(&g, &gm, 1, d.nb, d.b, Hd, stream));
    MV_TRY(lin_wgrad(&queue, d.rb, Hd, 3 * Hd, plain(b0.dgh), b0.hprev, G + m->beat_w_hh[0], G + m->beat_b_hh[0], s));
    // the constant input b_0 (decoder.py:436-440): the projection's gradients over all beats*batch rows (x0b holds b_0 once per row)
    MV_TRY(lin_wgrad(&queue, d.rb, 1, 3 * Hd, plain(b0.dgi), w.x0b, G + m->beat_w_ih[0], G + m->beat_b_ih[0], s));
    MV_TRY(lin_dgrad(d.rb, 1, 3 * Hd, plain(b0.dgi), P + m->beat_w_ih[0], w.d_x0, s));
    // (the gradient of b_0, the sum of d_x0, in grad_tail_kernel)
    MV_TRY(lin_dgrad(d.b, d.z, 2 * Hd, gated(w.d_flatb, w.flatb, ARVAE_ACT_SELU), P + m->z2beat_w, w.d_z, s));
    MV_TRY(lin_wgrad(&queue, d.b, d.z, 2 * Hd, gated(w.d_flatb, w.flatb, ARVAE_ACT_SELU), z, G + m->z2beat_w, G + m->z2beat_b, s));

    // ---- latent head: decoder path + regulariser + beta-KL -> (d mu, d log_std), then the heads' two layers
    const bool heads_fused = measure_heads_fit(2 * He, d.z);
    if (heads_fused) {                                        // (d mu, d log_std) and both heads' data gradients: one launch
        MeasureHeadsBwd hb{w.d_z, m->n_reg > 0 ? w.dz_reg : nullptr, mu, sigma, eps, g_loss, scalars + ARVAE_VAE_KL, capacity,
                           P + m->mean_w2, P + m->lstd_w2, m->beta, 1.f / (float)d.b, reg_scale, w.d_mu, w.d_ls, w.d_h12, d.b, 2 * He, d.z};
        ARVAE_LAUNCH(measure_heads_bwd_kernel, dim3((d.b + MH_ROWS - 1) / MH_ROWS), dim3(256), 0, s, hb);
        MV_TRY(check_launch("measure_heads_bwd_kernel"));
    } else {
        ARVAE_LAUNCH(measure_latent_bwd_kernel, dim3(blocks_for((int64_t)d.b * d.z)), dim3(256), 0, s, w.d_z, m->n_reg > 0 ? w.dz_reg : nullptr, mu,
                     sigma, eps, g_loss, scalars + ARVAE_VAE_KL, capacity, m->beta, 1.f / (float)d.b, reg_scale, (int64_t)d.b * d.z, w.d_mu, w.d_ls);
        MV_TRY(check_launch("measure_latent_bwd_kernel"));
        MV_TRY(lin_dgrad(d.b, 2 * He, d.z, plain(w.d_mu), P + m->mean_w2, w.d_hmu, s));
        MV_TRY(lin_dgrad(d.b, 2 * He, d.z, plain(w.d_ls), P + m->lstd_w2, w.d_hls, s));
    }
    MV_TRY(lin_wgrad(&queue, d.b, 2 * He, d.z, plain(w.d_mu), w.hmu, G + m->mean_w2, G + m->mean_b2, s));
    MV_TRY(lin_wgrad(&queue, d.b, 2 * He, d.z, plain(w.d_ls), w.hls, G + m->lstd_w2, G + m->lstd_b2, s));
    if (!heads_fused) MV_TRY(arvae_concat_cols(w.d_hmu, w.d_hls, d.b, 2 * He, 2 * He, w.d_h12, stream));
    MV_TRY(lin_dgrad(d.b, 4 * He, 4 * He, gated(w.d_h12, w.h12, ARVAE_ACT_SELU), P + m->head_w0, w.d_hidden, s));
    MV_TRY(lin_wgrad(&queue, d.b, 4 * He, 4 * He, gated(w.d_h12, w.h12, ARVAE_ACT_SELU), w.hidden, G + m->head_w0, G + m->head_b0, s));

    // ---- encoder, layer 1 then layer 0: layer 1 gets its gradient through the final states alone (enc_bwd: dh_last)
    for (int layer = 1; layer >= 0; --layer) {
        const GruLayer &e = w.enc[layer];
        const float *d_out = nullptr;
        GruSeqMask qm[2] = {};
        if (layer == 0) {
            MV_TRY(dropout_bwd(p, e, enc_mask, p.enc_keep, (int64_t)d.tb * 2 * He, false, e.d_out, &d_out));
            if (p.fuse_masks)
                for (int dir = 0; dir < 2; ++dir) qm[dir] = time_major_mask(p, enc_mask + dir * He, p.enc_keep, 2 * He, nullptr);
        }
        arvae_gru_seq_t q[2] = {enc_bwd(p, layer, 0, d_out), enc_bwd(p, layer, 1, d_out)};
        MV_TRY(gru_seq_bwd_masked(q, qm, 2, d.t, d.b, He, stream));
        for (int dir = 0; dir < 2; ++dir)
            MV_TRY(lin_wgrad(&queue, d.tb, He, 3 * He, plain(q[dir].dgh), q[dir].h_prev_out, G + m->enc_w_hh[layer][dir],
                             G + m->enc_b_hh[layer][dir], s));
        if (layer == 1) {
            MV_TRY(lin_wgrad(&queue, d.tb, 2 * He, 6 * He, plain(e.dgi), p.dropping ? w.enc[0].mid : w.enc[0].out, G + m->enc_w_ih[1],
                             G + m->enc_b_ih[1], s));
            MV_TRY(lin_dgrad(d.tb, 2 * He, 6 * He, plain(e.dgi), P + m->enc_w_ih[1], w.enc[0].d_mid, s));
        }
    }
    // layer 0's projection table: per-position gradients summed per token, then the small product's adjoints
    MV_TRY(arvae_embed_bwd(score, w.enc[0].dgi, d.b, d.t, 6 * He, d.v, 1, w.dptab, 0, w.embed_ws, stream));
    MV_TRY(lin_dgrad(d.v, d.e, 6 * He, plain(w.dptab), P + m->enc_w_ih[0], w.d_table, s));
    {
        GradTail t{w.dg_small, d.v + 1, 3 * Hd, G + m->tick_b_ih[0], (3 * Hd + 255) / 256, w.d_x0, d.rb, G + m->b0, w.d_table, d.v * d.e, G + m->enc_table};
        ARVAE_LAUNCH(grad_tail_kernel, dim3(t.cs_blocks + 1 + (t.add_n + 255) / 256), dim3(256), 0, s, t);
        MV_TRY(check_launch("grad_tail_kernel"));
    }
    MV_TRY(lin_wgrad(&queue, d.v, d.e, 6 * He, plain(w.dptab), P + m->enc_table, G + m->enc_w_ih[0], G + m->enc_b_ih[0], s));
    MV_TRY(dense_wgrad_long_flush(queue.rows, s));
    return dense_wgrad_flush(&queue.batch, s);
}
