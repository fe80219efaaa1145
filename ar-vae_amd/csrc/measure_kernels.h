// Kernel bodies of the MeasureVAE executor, for plan_measure.hip alone (in the manner of down32p.h / wgrad32r.h): the glue kernels
// between the sequence / dense / loss launches, the latent head's second layers as one launch per pass, the backward pass's closing launch.
#pragma once
#include "common.h"
#include "attributes.h"

namespace arvae {

// ---- glue kernels ----------------------------------------------------------------------------------
// rows of the tick RNN's sequence launches are ordered (tick-in-beat j, beat, measure b); the reference's tensors are ordered
// (tick t = tpb*beat + j, b) or (b, t).  y = alpha * x * mask with x in sequence order and the keep-mask in (t, b) order.
__global__ __launch_bounds__(256) void scale_mask_tick_kernel(const float *__restrict__ x, const uint8_t *__restrict__ mask, float alpha,
                                                               int batch, int beats, int tpb, int hid4, float *__restrict__ y) {
    const int64_t total = (int64_t)tpb * beats * batch * hid4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % hid4);
        int64_t r = i / hid4;
        const int b = (int)(r % batch);
        r /= batch;
        const int beat = (int)(r % beats), j = (int)(r / beats);
        const int64_t mrow = ((int64_t)(beat * tpb + j) * batch + b) * hid4 + c;
        const float4 v = reinterpret_cast<const float4 *>(x)[i];
        const uchar4 m = reinterpret_cast<const uchar4 *>(mask)[mrow];
        reinterpret_cast<float4 *>(y)[i] = make_float4(alpha * v.x * (float)m.x, alpha * v.y * (float)m.y, alpha * v.z * (float)m.z,
                                                       alpha * v.w * (float)m.w);
    }
}

// out = g[0] * d * (y > 0): the upstream scalar and the ReLU of the note projection folded into the cross-entropy gradient
__global__ __launch_bounds__(256) void relu_gate_scale_kernel(const float *__restrict__ d, const float *__restrict__ y,
                                                               const float *__restrict__ g, int64_t count4, float *__restrict__ out) {
    const float s = g[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count4; i += (int64_t)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4 *>(d)[i], a = reinterpret_cast<const float4 *>(y)[i];
        reinterpret_cast<float4 *>(out)[i] = make_float4(a.x > 0.f ? s * v.x : 0.f, a.y > 0.f ? s * v.y : 0.f, a.z > 0.f ? s * v.z : 0.f,
                                                         a.w > 0.f ? s * v.w : 0.f);
    }
}
__global__ __launch_bounds__(256) void relu_gate_scale1_kernel(const float *__restrict__ d, const float *__restrict__ y,
                                                                const float *__restrict__ g, int64_t count, float *__restrict__ out) {
    const float s = g[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
        out[i] = y[i] > 0.f ? s * d[i] : 0.f;
}

// y[r][:] = x[r][:] + bias[:]
__global__ __launch_bounds__(256) void add_bias_rows_kernel(const float4 *__restrict__ x, const float4 *__restrict__ bias, int64_t rows,
                                                             int cols4, float4 *__restrict__ y) {
    const int64_t total = rows * cols4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const float4 v = x[i], bb = bias[i % cols4];
        y[i] = make_float4(v.x + bb.x, v.y + bb.y, v.z + bb.z, v.w + bb.w);
    }
}

// gradient of the loss w.r.t. (mu, log_std): the decoder path g_z (already times the upstream scalar), the regulariser's unit
// gradient dz_reg and the beta-KL term; sigma = exp(log_std), z = mu + eps * sigma (measure_vae.py:115-123, utils/trainer.py:354-367)
__global__ __launch_bounds__(256) void measure_latent_bwd_kernel(const float *__restrict__ g_z, const float *__restrict__ dz_reg,
                                                                  const float *__restrict__ mu, const float *__restrict__ sigma,
                                                                  const float *__restrict__ eps, const float *__restrict__ g_loss,
                                                                  const float *__restrict__ kl, const float *__restrict__ cap, float beta,
                                                                  float inv_batch, float reg_scale, int64_t count, float *__restrict__ d_mu,
                                                                  float *__restrict__ d_ls) {
    const float g = g_loss[0];
    const float diff = kl[0] - (cap != nullptr ? cap[0] : 0.f);
    const float k = g * beta * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * inv_batch;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        float gz = g_z[i];
        if (dz_reg != nullptr) gz += g * reg_scale * dz_reg[i];
        const float s = sigma[i];
        d_mu[i] = gz + k * mu[i];
        d_ls[i] = (gz * eps[i] + k * (s - 1.f / s)) * s;
    }
}

// ---- the latent head's second layers + the reparameterised sample as ONE launch (forward), and their data gradients (backward).
// The two heads' first layers are one product h12 = [hmu | hls] (rows of 2 * hw floats); per row
//     mu = W_mu hmu + b_mu,   log_std = W_ls hls + b_ls,   sigma = exp(log_std),   z = mu + eps * sigma      (measure_vae.py:100-123)
// were a column split, two 5 us Linear launches and the sample; backward, the (d mu, d log_std) kernel, two data-gradient launches
// and a column concatenation.  MH_ROWS rows per workgroup, the 2 zdim weight rows in LDS (forward) or a thread's two weight
// columns in registers (backward); exact fp32 FMA chains.
constexpr int MH_ROWS = 4, MH_ZMAX = 32;
struct MeasureHeadsFwd {
    const float *h12, *w_mu, *b_mu, *w_ls, *b_ls, *eps;
    float *hmu, *hls, *mu, *log_std, *sigma, *z;      // hmu / hls: the halves of h12 as the weight gradients read them
    int batch, hw, zdim;                               // hw = width of one head's hidden vector (a multiple of 4)
};
__global__ __launch_bounds__(256) void measure_heads_fwd_kernel(MeasureHeadsFwd p) {
    extern __shared__ __attribute__((aligned(16))) float mh_lds[];
    const int ld = 2 * p.hw, ws = p.hw + 4, h4 = p.hw >> 2;
    float *hs = mh_lds, *wl = hs + MH_ROWS * ld, *outs = wl + 2 * p.zdim * ws;       // rows | 2 zdim weight rows | products
    const int row0 = blockIdx.x * MH_ROWS;
    for (int i = threadIdx.x; i < MH_ROWS * 2 * h4; i += 256) {
        const int r = i / (2 * h4), c4 = i - r * 2 * h4, row = row0 + r;
        const int rr = row < p.batch ? row : p.batch - 1;                               // clamped: unconditional load
        const float4 v = reinterpret_cast<const float4 *>(p.h12 + (int64_t)rr * ld)[c4];
        reinterpret_cast<float4 *>(hs + r * ld)[c4] = v;
        if (row < p.batch) {
            float *dst = c4 < h4 ? p.hmu + (int64_t)row * p.hw + 4 * c4 : p.hls + (int64_t)row * p.hw + 4 * (c4 - h4);
            *reinterpret_cast<float4 *>(dst) = v;
        }
    }
    for (int base = 0; base < 2 * p.zdim * h4; base += 8 * 256) {       // eight independent 16-byte loads per thread and round trip
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(base + u * 256 + (int)threadIdx.x, 2 * p.zdim * h4 - 1), j = i / h4, k = i - j * h4;
            const float *src = j < p.zdim ? p.w_mu + (int64_t)j * p.hw : p.w_ls + (int64_t)(j - p.zdim) * p.hw;
            v[u] = reinterpret_cast<const float4 *>(src)[k];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * 256 + (int)threadIdx.x, j = i / h4, k = i - j * h4;
            if (i < 2 * p.zdim * h4) reinterpret_cast<float4 *>(wl + j * ws)[k] = v[u];
        }
    }
    const int r = threadIdx.x >> 6, j = threadIdx.x & 63, row = row0 + r;
    const bool col_ok = j < 2 * p.zdim, lat = j < p.zdim && row < p.batch;
    const int64_t idx = lat ? (int64_t)row * p.zdim + j : 0;
    const float e = p.eps[idx];
    const int jc = col_ok ? j : 0;
    const float *bp = jc < p.zdim ? p.b_mu : p.b_ls;
    const float bias = bp != nullptr ? bp[jc < p.zdim ? jc : jc - p.zdim] : 0.f;
    __syncthreads();
    {
        const float4 *w = reinterpret_cast<const float4 *>(wl + jc * ws);
        const float4 *x = reinterpret_cast<const float4 *>(hs + r * ld + (jc < p.zdim ? 0 : p.hw));
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
        for (int k = 0; k < h4; ++k) {
            const float4 a = x[k], b = w[k];
            acc.x = fmaf(a.x, b.x, acc.x); acc.y = fmaf(a.y, b.y, acc.y);
            acc.z = fmaf(a.z, b.z, acc.z); acc.w = fmaf(a.w, b.w, acc.w);
        }
        outs[r * 64 + j] = (acc.x + acc.y) + (acc.z + acc.w) + bias;
    }
    __syncthreads();
    if (lat) {
        const float m = outs[r * 64 + j], l = outs[r * 64 + j + p.zdim];
        const float sg = expf(l);
        p.mu[idx] = m;
        p.log_std[idx] = l;
        p.sigma[idx] = sg;
        p.z[idx] = fmaf(e, sg, m);
    }
}

struct MeasureHeadsBwd {
    const float *g_z, *dz_reg, *mu, *sigma, *eps, *g_loss, *kl, *cap, *w_mu, *w_ls;
    float beta, inv_batch, reg_scale;
    float *d_mu, *d_ls, *d_h12;                        // d_h12 rows: [d hmu | d hls]
    int batch, hw, zdim;
};
// thread = one column of each head's hidden vector (hw <= 256 columns): its two weight columns in registers, the rows'
// (d mu, d log_std) through LDS
__global__ __launch_bounds__(256) void measure_heads_bwd_kernel(MeasureHeadsBwd p) {
    __shared__ float dm[MH_ROWS][MH_ZMAX], dl[MH_ROWS][MH_ZMAX];
    const int row0 = blockIdx.x * MH_ROWS, k = threadIdx.x;
    const bool kok = k < p.hw;
    float wm[MH_ZMAX], wls[MH_ZMAX];
#pragma unroll
    for (int j = 0; j < MH_ZMAX; ++j) {
        const bool ok = kok && j < p.zdim;
        wm[j] = ok ? p.w_mu[(int64_t)j * p.hw + k] : 0.f;
        wls[j] = ok ? p.w_ls[(int64_t)j * p.hw + k] : 0.f;
    }
    if (threadIdx.x < MH_ROWS * MH_ZMAX) {
        const int r = threadIdx.x / MH_ZMAX, j = threadIdx.x % MH_ZMAX, row = row0 + r;
        float a = 0.f, b = 0.f;
        if (row < p.batch && j < p.zdim) {
            const int64_t i = (int64_t)row * p.zdim + j;
            const float g = p.g_loss[0];
            const float diff = p.kl[0] - (p.cap != nullptr ? p.cap[0] : 0.f);
            const float kk = g * p.beta * (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) * p.inv_batch;
            float gz = p.g_z[i];
            if (p.dz_reg != nullptr) gz += g * p.reg_scale * p.dz_reg[i];
            const float sg = p.sigma[i];
            a = gz + kk * p.mu[i];
            b = (gz * p.eps[i] + kk * (sg - 1.f / sg)) * sg;
            p.d_mu[i] = a;
            p.d_ls[i] = b;
        }
        dm[r][j] = a;
        dl[r][j] = b;
    }
    __syncthreads();
    if (!kok) return;
#pragma unroll
    for (int r = 0; r < MH_ROWS; ++r) {
        if (row0 + r >= p.batch) break;
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int j = 0; j < MH_ZMAX; ++j) {
            a = fmaf(dm[r][j], wm[j], a);
            b = fmaf(dl[r][j], wls[j], b);
        }
        float *dst = p.d_h12 + (int64_t)(row0 + r) * 2 * p.hw;
        dst[k] = a;
        dst[p.hw + k] = b;
    }
}
static bool measure_heads_fit(int hw, int zdim) { return hw >= 4 && hw <= 256 && (hw & 3) == 0 && zdim >= 1 && zdim <= MH_ZMAX; }

// the beat RNN's constant input b_0 (decoder.py:436-440): its copies x0b[rows] (what the weight gradient reads) and its projection
// gi[b][c] = b_0 * w[c] + bias[c], the same row for every measure -- one launch instead of a broadcast and a 1-wide Linear layer
__global__ __launch_bounds__(256) void beat_input_kernel(BeatInput p) {
    beat_input_items(p, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}
// Three small sums that nothing in the pass waits for, as ONE launch at its end (round 5; each was a ~5 us launch of its own at the point
// where its operand appeared): the tick RNN's first bias gradient (column sums of the note rows), the gradient of b_0 (a sum over
// beats x batch numbers) and the encoder table's gradient added to the arena.  Workgroups [0, cs_blocks) the column sums, one the sum,
// the rest the addition; each job's own fixed order is what it was.
struct GradTail {
    const float *cs_x; int cs_rows, cs_cols; float *cs_dst; int cs_blocks;
    const float *sum_x; int sum_n; float *sum_dst;
    const float *add_x; int add_n; float *add_dst;
};
__global__ __launch_bounds__(256) void grad_tail_kernel(GradTail t) {
    __shared__ float red[256];
    const int b = blockIdx.x;
    if (b < t.cs_blocks) {
        const int c = b * 256 + threadIdx.x;
        if (c >= t.cs_cols) return;
        float a = 0.f;
        for (int r0 = 0; r0 < t.cs_rows; r0 += 16) {             // sixteen independent loads per round trip, summed in row order
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = t.cs_x[(int64_t)min(r0 + u, t.cs_rows - 1) * t.cs_cols + c];
#pragma unroll
            for (int u = 0; u < 16; ++u) a += r0 + u < t.cs_rows ? v[u] : 0.f;
        }
        t.cs_dst[c] += a;
    } else if (b == t.cs_blocks) {
        float a = 0.f;
        for (int i = threadIdx.x; i < t.sum_n; i += 256) a += t.sum_x[i];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) t.sum_dst[0] += red[0];
    } else {
        const int i = (b - t.cs_blocks - 1) * 256 + threadIdx.x;
        if (i < t.add_n) t.add_dst[i] += t.add_x[i];
    }
}

}  // namespace arvae
