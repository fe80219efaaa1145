// The Morpho-MNIST digit classifier (a torchvision ResNet-18 with a 1-channel stem, imagevae/mnist_resnet.py) as an inference
// pass at 28 x 28: BN folded into the convolutions once per weight change, 22 launches per forward, no LDS and no hand-off
// between workgroups anywhere (every launch is an ordinary grid).
//
//   stem      conv 7x7 s2 p3 (1 -> 64) + b' + ReLU            vector ALU (K = 49), one thread per output value
//   pool      max 3x3 s2 p1, padding = -inf                    one thread per 4 channels of an output pixel
//   19 convs  3x3 (s1 / s2, p1) and 1x1 s2, 64..512 channels   implicit GEMM on the THREE-TERM bf16 MFMA arithmetic (splitmath.h)
//   head      fc 512 -> 10 + softmax + argmax                  one wave per image
//
// The convolution kernel.  M = images x output pixels, N = C_out, K = live taps x C_in; a wave owns a 32-pixel x 64-channel
// tile (two 32 x 32 fp32 accumulators, 32 VGPRs), a workgroup is four such waves on consecutive pixel tiles of one channel group,
// and the waves never talk to each other.  Per k-step of 16 a lane reads the 8 consecutive input channels of its pixel and
// tap (two 16-byte loads of the NHWC activation, zero where the tap falls on padding or the pixel is past M), splits them into
// three bf16 terms in registers, and reads the weights' three terms for its two channel rows as six 16-byte loads of the prepared
// operand planes, which lie in exactly the per-lane order of the MFMA's A operand (a wave's load is 1 KB, contiguous).  12 MFMAs
// (2 accumulators x 6 partial products, smallest first) follow; the loads of the next k-step are issued before them.  No LDS: an
// operand is used by one wave only, and the weights that the four waves share come from L1/L2.
// THREE terms, not two: the two-term fp16 arithmetic needs the maximum of every activation tensor before it is read (amax.h),
// i.e. either a dependency of each launch on a reduction of its predecessor's output or a second pass; the activations here are
// sums of BN-folded convolutions and residuals whose range no one bounds.  bf16 has fp32's exponent range and needs no scale,
// the weights are split once at preparation, and at 66 MFLOP per image the pass is bound by launches and operand traffic, not
// by the matrix pipe.
// LIVE TAPS: a tap (ky, kx) is packed only if it reads a pixel inside the input for SOME output pixel -- 1 of 9 at 1 x 1 input, 4 of 9
// at 2 -> 1 (stride 2); at 2 x 2 stride 1 every tap is live for one of the four pixels, so all 9 stay and the kernel's
// per-(pixel, tap) predicate zeroes the 5 that fall on padding.  The kernel walks the packed list.
// Accumulation order is fixed (k ascending inside one accumulator, no atomics): the same input gives the same bits.
#include "common.h"
#include "splitmath.h"

namespace arvae {

constexpr int RN_CONVS = 19;
constexpr int RN_STEM_TAPS = 49, RN_STEM_C = 64, RN_STEM_HW = 14, RN_IMG = 28, RN_POOL_HW = 7, RN_FEAT = 512, RN_CLASSES = 10;
constexpr double RN_BN_EPS = 1e-5;

// ---- geometry ----------------------------------------------------------------------------------------------------------------
struct ConvPlan {
    int hin, win, cin, hout, wout, cout, stride, ntaps, csteps;      // csteps = cin / 16
    int dy[9], dx[9];                                                // live tap t reads (oy * stride + dy[t], ox * stride + dx[t])
    int ky[9], kx[9];
    FastDiv div_px, div_w;                                           // m -> image, pixel -> (oy, ox)
};

static bool conv_ok(const arvae_resnet18_conv_t *g) {
    if (g == nullptr) return false;
    const bool ch = (g->cin == 64 || g->cin == 128 || g->cin == 256 || g->cin == 512) &&
                    (g->cout == 64 || g->cout == 128 || g->cout == 256 || g->cout == 512);
    const bool k = (g->ksize == 3 && g->pad == 1) || (g->ksize == 1 && g->pad == 0);
    if (!ch || !k || (g->stride != 1 && g->stride != 2) || g->hin < 1 || g->win < 1 || g->hin > 64 || g->win > 64) return false;
    return g->hout == (g->hin + 2 * g->pad - g->ksize) / g->stride + 1 && g->wout == (g->win + 2 * g->pad - g->ksize) / g->stride + 1;
}

static bool tap_live(int k, int pad, int stride, int nin, int nout) {
    for (int o = 0; o < nout; ++o) {
        const int i = o * stride - pad + k;
        if (i >= 0 && i < nin) return true;
    }
    return false;
}

static ConvPlan make_plan(const arvae_resnet18_conv_t *g) {
    ConvPlan p{};
    p.hin = g->hin; p.win = g->win; p.cin = g->cin; p.hout = g->hout; p.wout = g->wout; p.cout = g->cout; p.stride = g->stride;
    p.csteps = g->cin / 16;
    for (int ky = 0; ky < g->ksize; ++ky)
        for (int kx = 0; kx < g->ksize; ++kx)
            if (tap_live(ky, g->pad, g->stride, g->hin, g->hout) && tap_live(kx, g->pad, g->stride, g->win, g->wout)) {
                p.ky[p.ntaps] = ky; p.kx[p.ntaps] = kx;
                p.dy[p.ntaps] = ky - g->pad; p.dx[p.ntaps] = kx - g->pad;
                ++p.ntaps;
            }
    p.div_px = FastDiv((uint32_t)(g->hout * g->wout));
    p.div_w = FastDiv((uint32_t)g->wout);
    return p;
}

// prepared form of one convolution: [cout / 64][k-step][2 row blocks][3 terms][64 lanes] x 8 bf16, then cout biases
static int64_t conv_plane_floats(const ConvPlan &p) { return (int64_t)p.cout * p.ntaps * p.cin * 3 / 2; }
static int64_t conv_prep_floats(const ConvPlan &p) { return conv_plane_floats(p) + p.cout; }

// ---- preparation ---------------------------------------------------------------------------------------------------------------
// BN folded in float64: scale = gamma / sqrt(var + eps), b' = beta - mean * scale (bn_w == nullptr: scale 1, b' 0)
__device__ __forceinline__ double bn_scale(const float *bn_w, const float *bn_var, int c) {
    return bn_w == nullptr ? 1.0 : (double)bn_w[c] / sqrt((double)bn_var[c] + (double)RN_BN_EPS);
}
__device__ __forceinline__ float bn_shift(const float *bn_w, const float *bn_b, const float *bn_mean, const float *bn_var, int c) {
    return bn_w == nullptr ? 0.f : (float)((double)bn_b[c] - (double)bn_mean[c] * bn_scale(bn_w, bn_var, c));
}

// one thread per (channel group, k-step, row block, lane): the 8 folded weights of that lane's operand register, three planes
__global__ __launch_bounds__(256) void resnet_conv_prep_kernel(ConvPlan p, int ksize, const float *__restrict__ w,
                                                               const float *__restrict__ bn_w, const float *__restrict__ bn_b,
                                                               const float *__restrict__ bn_mean, const float *__restrict__ bn_var,
                                                               uint4 *__restrict__ planes, float *__restrict__ bias) {
    const int ksteps = p.ntaps * p.csteps;
    const int total = (p.cout / 64) * ksteps * 2 * 64;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < p.cout) bias[idx] = bn_shift(bn_w, bn_b, bn_mean, bn_var, idx);
    if (idx >= total) return;
    const int lane = idx & 63, a = (idx >> 6) & 1, gs = idx >> 7;
    const int s = gs % ksteps, g = gs / ksteps;
    const int c = g * 64 + a * 32 + (lane & 31);
    const int t = s / p.csteps, ci0 = (s % p.csteps) * 16 + 8 * (lane >> 5);
    const double sc = bn_scale(bn_w, bn_var, c);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        v[j] = (float)((double)w[(((int64_t)c * p.cin + ci0 + j) * ksize + p.ky[t]) * ksize + p.kx[t]] * sc);
    bf16x8 h, m, l;
    split3_8(v, h, m, l);
    uint4 *dst = planes + ((int64_t)gs * 2 + a) * 3 * 64 + lane;
    dst[0] = __builtin_bit_cast(uint4, h);
    dst[64] = __builtin_bit_cast(uint4, m);
    dst[128] = __builtin_bit_cast(uint4, l);
}

// stem: w'[tap][c] (49 x 64) then 64 biases
__global__ __launch_bounds__(256) void resnet_stem_prep_kernel(const float *__restrict__ w, const float *__restrict__ bn_w,
                                                               const float *__restrict__ bn_b, const float *__restrict__ bn_mean,
                                                               const float *__restrict__ bn_var, float *__restrict__ prep) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < RN_STEM_C) prep[RN_STEM_TAPS * RN_STEM_C + idx] = bn_shift(bn_w, bn_b, bn_mean, bn_var, idx);
    if (idx >= RN_STEM_TAPS * RN_STEM_C) return;
    const int c = idx & 63, t = idx >> 6;
    prep[idx] = (float)((double)w[c * RN_STEM_TAPS + t] * bn_scale(bn_w, bn_var, c));
}

__global__ __launch_bounds__(256) void resnet_copy_kernel(const float *__restrict__ src, float *__restrict__ dst, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n) dst[idx] = src[idx];
}

// ---- the convolution -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resnet_conv_x3_kernel(ConvPlan p, int M, const uint4 *__restrict__ planes,
                                                             const float *__restrict__ bias, const float *__restrict__ x,
                                                             const float *__restrict__ res, int relu, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = (blockIdx.x * 4 + wave) * 32;
    if (m0 >= M) return;                                             // (no barrier below: a wave past the ragged end just leaves)
    const int col = lane & 31, half = lane >> 5;
    const int m = m0 + col;
    const bool mval = m < M;
    uint32_t img, px, oy, ox;
    p.div_px.divmod((uint32_t)(mval ? m : m0), img, px);
    p.div_w.divmod(px, oy, ox);
    const int ksteps = p.ntaps * p.csteps;
    const uint4 *wp = planes + (int64_t)blockIdx.y * ksteps * 384 + lane;
    f32x16 acc0 = {}, acc1 = {};
    // the operands of one k-step: 8 input channels of this lane's (pixel, tap) and the six weight registers.  A (pixel, tap) pair on
    // padding or past M reads pixel (0, 0) of its image -- in bounds -- and discards it: no branch around the loads.
    struct KStep { float4 v0, v1; uint4 w[6]; bool valid; };
    int t = 0, s = 0;
    const float *src = x;
    bool valid = false;
    auto enter_tap = [&]() {
        const int iy = (int)oy * p.stride + p.dy[t], ix = (int)ox * p.stride + p.dx[t];
        valid = mval && iy >= 0 && iy < p.hin && ix >= 0 && ix < p.win;
        src = x + (((int64_t)img * p.hin + (valid ? iy : 0)) * p.win + (valid ? ix : 0)) * p.cin + 8 * half;
    };
    auto fetch = [&](KStep &k) {
        k.v0 = *reinterpret_cast<const float4 *>(src);
        k.v1 = *reinterpret_cast<const float4 *>(src + 4);
#pragma unroll
        for (int i = 0; i < 6; ++i) k.w[i] = wp[64 * i];
        k.valid = valid;
    };
    enter_tap();
    KStep cur, nxt;
    fetch(cur);
    // software pipeline, depth 1: the loads of k-step ks + 1 are in flight while the 12 MFMAs of k-step ks issue
    for (int ks = 0; ks < ksteps; ++ks) {
        nxt = cur;
        if (ks + 1 < ksteps) {
            wp += 384;
            src += 16;
            if (++s == p.csteps) {
                s = 0;
                ++t;
                enter_tap();
            }
            fetch(nxt);
        }
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 v0 = cur.valid ? cur.v0 : z, v1 = cur.valid ? cur.v1 : z;
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        bf16x8 xh, xm, xl;
        split3_8(v, xh, xm, xl);
        X3_MFMA6(acc0, __builtin_bit_cast(bf16x8, cur.w[0]), __builtin_bit_cast(bf16x8, cur.w[1]), __builtin_bit_cast(bf16x8, cur.w[2]), xh,
                 xm, xl);
        X3_MFMA6(acc1, __builtin_bit_cast(bf16x8, cur.w[3]), __builtin_bit_cast(bf16x8, cur.w[4]), __builtin_bit_cast(bf16x8, cur.w[5]), xh,
                 xm, xl);
        cur = nxt;
    }
    if (!mval) return;
    // accumulator register 4 q + j holds channel row 8 q + 4 half + j of pixel column `col`: four consecutive channels per store
    const int64_t obase = (int64_t)m * p.cout + blockIdx.y * 64 + 4 * half;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const f32x16 &acc = a == 0 ? acc0 : acc1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = blockIdx.y * 64 + a * 32 + 8 * q + 4 * half;
            const float4 b = *reinterpret_cast<const float4 *>(bias + c);
            float4 r = make_float4(acc[4 * q] + b.x, acc[4 * q + 1] + b.y, acc[4 * q + 2] + b.z, acc[4 * q + 3] + b.w);
            const int64_t o = obase + a * 32 + 8 * q;
            if (res != nullptr) {
                const float4 e = *reinterpret_cast<const float4 *>(res + o);
                r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w;
            }
            if (relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
            *reinterpret_cast<float4 *>(out + o) = r;
        }
    }
}

// ---- stem, pool, head ----------------------------------------------------------------------------------------------------------
// one thread per output value (a wave = the 64 channels of one pixel: the image reads are wave-uniform).  Each of the 7 kernel
// rows is summed on its own and the 7 row sums are added in order: shorter chains than one of 49.
__global__ __launch_bounds__(256) void resnet_stem_kernel(const float *__restrict__ prep, const float *__restrict__ x, int64_t total,
                                                          int relu, float *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx & 63);
    const int64_t pix = idx >> 6;
    const int img = (int)(pix / (RN_STEM_HW * RN_STEM_HW)), r = (int)(pix % (RN_STEM_HW * RN_STEM_HW));
    const int oy = r / RN_STEM_HW, ox = r % RN_STEM_HW;
    const float *im = x + (int64_t)img * RN_IMG * RN_IMG;
    float sum = 0.f;
    for (int ky = 0; ky < 7; ++ky) {
        const int iy = 2 * oy - 3 + ky;
        if (iy < 0 || iy >= RN_IMG) continue;
        float row = 0.f;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const int ix = 2 * ox - 3 + kx;
            const float v = (ix >= 0 && ix < RN_IMG) ? im[iy * RN_IMG + ix] : 0.f;
            row = fmaf(v, prep[(ky * 7 + kx) * RN_STEM_C + c], row);
        }
        sum += row;
    }
    sum += prep[RN_STEM_TAPS * RN_STEM_C + c];
    out[idx] = relu ? fmaxf(sum, 0.f) : sum;
}

// max-pool 3x3 s2 p1 over NHWC, c a multiple of 4; a window position outside the input does not take part (padding = -inf)
__global__ __launch_bounds__(256) void resnet_maxpool_kernel(const float *__restrict__ x, int h, int w, int c, int ho, int wo, int64_t total,
                                                             float *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;             // one per (output pixel, 4 channels)
    if (idx >= total) return;
    const int c4 = c >> 2;
    const int cq = (int)(idx % c4);
    const int64_t pix = idx / c4;
    const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho);
    const int64_t img = pix / ((int64_t)wo * ho);
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= h) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= w) continue;
            const float4 v = *reinterpret_cast<const float4 *>(x + ((img * h + iy) * w + ix) * c + 4 * cq);
            best.x = fmaxf(best.x, v.x); best.y = fmaxf(best.y, v.y); best.z = fmaxf(best.z, v.z); best.w = fmaxf(best.w, v.w);
        }
    }
    *reinterpret_cast<float4 *>(out + pix * c + 4 * cq) = best;
}

// one wave per image: a lane sums 8 of the 512 features per class, the wave adds the 64 partial sums in a fixed butterfly, lane 0
// finishes (bias, softmax, argmax: the lowest index wins an exact tie)
__global__ __launch_bounds__(256) void resnet_head_kernel(const float *__restrict__ fc_w, const float *__restrict__ fc_b,
                                                          const float *__restrict__ feat, int n, float *__restrict__ logits,
                                                          float *__restrict__ probs, int64_t *__restrict__ pred) {
    const int lane = threadIdx.x & 63;
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (img >= n) return;
    const float4 f0 = *reinterpret_cast<const float4 *>(feat + (int64_t)img * RN_FEAT + 8 * lane);
    const float4 f1 = *reinterpret_cast<const float4 *>(feat + (int64_t)img * RN_FEAT + 8 * lane + 4);
    float z[RN_CLASSES];
#pragma unroll
    for (int k = 0; k < RN_CLASSES; ++k) {
        const float4 w0 = *reinterpret_cast<const float4 *>(fc_w + k * RN_FEAT + 8 * lane);
        const float4 w1 = *reinterpret_cast<const float4 *>(fc_w + k * RN_FEAT + 8 * lane + 4);
        float s = f0.x * w0.x;
        s = fmaf(f0.y, w0.y, s); s = fmaf(f0.z, w0.z, s); s = fmaf(f0.w, w0.w, s);
        s = fmaf(f1.x, w1.x, s); s = fmaf(f1.y, w1.y, s); s = fmaf(f1.z, w1.z, s); s = fmaf(f1.w, w1.w, s);
        z[k] = wave_sum(s);
    }
    if (lane != 0) return;
    float top = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < RN_CLASSES; ++k) {
        z[k] += fc_b[k];
        if (z[k] > top) { top = z[k]; arg = k; }
    }
    float e[RN_CLASSES], den = 0.f;
#pragma unroll
    for (int k = 0; k < RN_CLASSES; ++k) { e[k] = expf(z[k] - top); den += e[k]; }
#pragma unroll
    for (int k = 0; k < RN_CLASSES; ++k) {
        if (logits != nullptr) logits[(int64_t)img * RN_CLASSES + k] = z[k];
        if (probs != nullptr) probs[(int64_t)img * RN_CLASSES + k] = e[k] / den;
    }
    if (pred != nullptr) pred[img] = arg;
}

// ---- the network ----------------------------------------------------------------------------------------------------------------
// execution order; `in` / `res` / `out` index the four rotating activation buffers of the workspace (-1: no residual)
struct NetConv { int hin, cin, hout, cout, ksize, stride, in, res, out, relu; };
static const NetConv kNet[RN_CONVS] = {
    {7, 64, 7, 64, 3, 1, 0, -1, 1, 1},   {7, 64, 7, 64, 3, 1, 1, 0, 2, 1},        // layer1.0
    {7, 64, 7, 64, 3, 1, 2, -1, 1, 1},   {7, 64, 7, 64, 3, 1, 1, 2, 0, 1},        // layer1.1
    {7, 64, 4, 128, 3, 2, 0, -1, 1, 1},  {7, 64, 4, 128, 1, 2, 0, -1, 3, 0},  {4, 128, 4, 128, 3, 1, 1, 3, 2, 1},      // layer2.0
    {4, 128, 4, 128, 3, 1, 2, -1, 1, 1}, {4, 128, 4, 128, 3, 1, 1, 2, 0, 1},      // layer2.1
    {4, 128, 2, 256, 3, 2, 0, -1, 1, 1}, {4, 128, 2, 256, 1, 2, 0, -1, 3, 0}, {2, 256, 2, 256, 3, 1, 1, 3, 2, 1},      // layer3.0
    {2, 256, 2, 256, 3, 1, 2, -1, 1, 1}, {2, 256, 2, 256, 3, 1, 1, 2, 0, 1},      // layer3.1
    {2, 256, 1, 512, 3, 2, 0, -1, 1, 1}, {2, 256, 1, 512, 1, 2, 0, -1, 3, 0}, {1, 512, 1, 512, 3, 1, 1, 3, 2, 1},      // layer4.0
    {1, 512, 1, 512, 3, 1, 2, -1, 1, 1}, {1, 512, 1, 512, 3, 1, 1, 2, 0, 1},      // layer4.1
};
static arvae_resnet18_conv_t net_geom(int i) {
    const NetConv &c = kNet[i];
    return arvae_resnet18_conv_t{c.hin, c.hin, c.cin, c.hout, c.hout, c.cout, c.ksize, c.stride, c.ksize == 3 ? 1 : 0, 0};
}
constexpr int64_t RN_STEM_PREP = RN_STEM_TAPS * RN_STEM_C + RN_STEM_C;
constexpr int64_t RN_FC_PREP = RN_CLASSES * RN_FEAT + 12;                            // weight, bias (10, padded to 12)
static int64_t net_conv_offset(int i) {                                             // floats from the start of the prepared block
    int64_t off = RN_STEM_PREP;
    for (int j = 0; j < i; ++j) {
        const arvae_resnet18_conv_t g = net_geom(j);
        off += conv_prep_floats(make_plan(&g));
    }
    return off;
}
constexpr int64_t RN_ACT_STEM = (int64_t)RN_STEM_HW * RN_STEM_HW * RN_STEM_C;       // per image
constexpr int64_t RN_ACT_BUF = (int64_t)RN_POOL_HW * RN_POOL_HW * RN_STEM_C;        // the largest activation after the pool

static int launch_conv_prep(const ConvPlan &p, int ksize, const float *w, const float *bn_w, const float *bn_b, const float *bn_mean,
                            const float *bn_var, float *prep, hipStream_t s) {
    const int total = (p.cout / 64) * p.ntaps * p.csteps * 128;
    ARVAE_LAUNCH(resnet_conv_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, ksize, w, bn_w, bn_b, bn_mean, bn_var,
                 reinterpret_cast<uint4 *>(prep), prep + conv_plane_floats(p));
    return check_launch("resnet_conv_prep_kernel");
}
static int launch_conv(const ConvPlan &p, const float *prep, const float *x, int n, const float *res, int relu, float *out, hipStream_t s) {
    const int M = n * p.hout * p.wout;
    ARVAE_LAUNCH(resnet_conv_x3_kernel, dim3((unsigned)((M + 127) / 128), (unsigned)(p.cout / 64)), dim3(256), 0, s, p, M,
                 reinterpret_cast<const uint4 *>(prep), prep + conv_plane_floats(p), x, res, relu, out);
    return check_launch("resnet_conv_x3_kernel");
}
static int launch_stem(const float *prep, const float *x, int n, int relu, float *out, hipStream_t s) {
    const int64_t total = (int64_t)n * RN_ACT_STEM;
    ARVAE_LAUNCH(resnet_stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, prep, x, total, relu, out);
    return check_launch("resnet_stem_kernel");
}
static int launch_pool(const float *x, int n, int h, int w, int c, float *out, hipStream_t s) {
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const int64_t total = (int64_t)n * ho * wo * (c / 4);
    ARVAE_LAUNCH(resnet_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, h, w, c, ho, wo, total, out);
    return check_launch("resnet_maxpool_kernel");
}
static int launch_head(const float *fc_w, const float *fc_b, const float *feat, int n, float *logits, float *probs, int64_t *pred,
                       hipStream_t s) {
    ARVAE_LAUNCH(resnet_head_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, fc_w, fc_b, feat, n, logits, probs, pred);
    return check_launch("resnet_head_kernel");
}
constexpr int RN_MAX_BATCH = 1 << 16;                                              // 2^16 x 12544 stem outputs < 2^31 elements

}  // namespace arvae

using namespace arvae;

extern "C" int32_t arvae_resnet18_live_taps(const arvae_resnet18_conv_t *geom, int32_t *taps) {
    ARVAE_REQUIRE(conv_ok(geom), "resnet18_live_taps: unsupported convolution geometry");
    const ConvPlan p = make_plan(geom);
    if (taps != nullptr)
        for (int t = 0; t < p.ntaps; ++t) taps[t] = p.ky[t] * geom->ksize + p.kx[t];
    return p.ntaps;
}

extern "C" int64_t arvae_resnet18_conv_prep_floats(const arvae_resnet18_conv_t *geom) {
    ARVAE_REQUIRE(conv_ok(geom), "resnet18_conv_prep_floats: unsupported convolution geometry");
    return conv_prep_floats(make_plan(geom));
}

extern "C" int arvae_resnet18_conv_prepare(const arvae_resnet18_conv_t *geom, const float *w, const float *bn_w, const float *bn_b,
                                           const float *bn_mean, const float *bn_var, float *prep, arvae_stream_t stream) {
    ARVAE_REQUIRE(conv_ok(geom), "resnet18_conv_prepare: unsupported convolution geometry");
    ARVAE_REQUIRE(w && prep, "resnet18_conv_prepare: null pointer (w and prep are required)");
    ARVAE_REQUIRE((bn_w && bn_b && bn_mean && bn_var) || (!bn_w && !bn_b && !bn_mean && !bn_var),
                  "resnet18_conv_prepare: the four batch-norm tensors come together or not at all");
    return launch_conv_prep(make_plan(geom), geom->ksize, w, bn_w, bn_b, bn_mean, bn_var, prep, as_stream(stream));
}

extern "C" int arvae_resnet18_conv(const arvae_resnet18_conv_t *geom, const float *prep, const float *x, int32_t n, const float *residual,
                                   int32_t relu, float *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(conv_ok(geom), "resnet18_conv: unsupported convolution geometry");
    ARVAE_REQUIRE(prep && x && out, "resnet18_conv: null pointer (prep, x and out are required)");
    ARVAE_REQUIRE(n >= 1 && n <= RN_MAX_BATCH, "resnet18_conv: batch %d out of range 1..%d", (int)n, RN_MAX_BATCH);
    return launch_conv(make_plan(geom), prep, x, n, residual, relu, out, as_stream(stream));
}

extern "C" int64_t arvae_resnet18_stem_prep_floats(void) { return RN_STEM_PREP; }

extern "C" int arvae_resnet18_stem_prepare(const float *w, const float *bn_w, const float *bn_b, const float *bn_mean, const float *bn_var,
                                           float *prep, arvae_stream_t stream) {
    ARVAE_REQUIRE(w && prep, "resnet18_stem_prepare: null pointer (w and prep are required)");
    ARVAE_REQUIRE((bn_w && bn_b && bn_mean && bn_var) || (!bn_w && !bn_b && !bn_mean && !bn_var),
                  "resnet18_stem_prepare: the four batch-norm tensors come together or not at all");
    ARVAE_LAUNCH(resnet_stem_prep_kernel, dim3((RN_STEM_TAPS * RN_STEM_C + 255) / 256), dim3(256), 0, as_stream(stream), w, bn_w, bn_b,
                 bn_mean, bn_var, prep);
    return check_launch("resnet_stem_prep_kernel");
}

extern "C" int arvae_resnet18_stem(const float *prep, const float *x, int32_t n, int32_t relu, float *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(prep && x && out, "resnet18_stem: null pointer");
    ARVAE_REQUIRE(n >= 1 && n <= RN_MAX_BATCH, "resnet18_stem: batch %d out of range 1..%d", (int)n, RN_MAX_BATCH);
    return launch_stem(prep, x, n, relu, out, as_stream(stream));
}

extern "C" int arvae_resnet18_maxpool(const float *x, int32_t n, int32_t h, int32_t w, int32_t c, float *out, arvae_stream_t stream) {
    ARVAE_REQUIRE(x && out, "resnet18_maxpool: null pointer");
    ARVAE_REQUIRE(n >= 1 && n <= RN_MAX_BATCH && h >= 1 && w >= 1 && h <= 64 && w <= 64 && c >= 4 && c <= 512 && c % 4 == 0,
                  "resnet18_maxpool: n %d, h %d, w %d or c %d out of range (c a multiple of 4)", (int)n, (int)h, (int)w, (int)c);
    return launch_pool(x, n, h, w, c, out, as_stream(stream));
}

extern "C" int arvae_resnet18_head(const float *fc_w, const float *fc_b, const float *feat, int32_t n, float *logits, float *probs,
                                   int64_t *pred, arvae_stream_t stream) {
    ARVAE_REQUIRE(fc_w && fc_b && feat, "resnet18_head: null pointer (fc_w, fc_b and feat are required)");
    ARVAE_REQUIRE(n >= 1 && n <= RN_MAX_BATCH, "resnet18_head: batch %d out of range 1..%d", (int)n, RN_MAX_BATCH);
    return launch_head(fc_w, fc_b, feat, n, logits, probs, pred, as_stream(stream));
}

extern "C" int64_t arvae_resnet18_prep_floats(void) { return net_conv_offset(RN_CONVS) + RN_FC_PREP; }

extern "C" int arvae_resnet18_prepare(const arvae_resnet18_weights_t *w, float *prep, arvae_stream_t stream) {
    ARVAE_REQUIRE(w && prep, "resnet18_prepare: null pointer");
    ARVAE_REQUIRE(w->stem_w && w->fc_w && w->fc_b, "resnet18_prepare: null pointer in the weight table");
    for (int i = 0; i < 4; ++i) ARVAE_REQUIRE(w->stem_bn[i], "resnet18_prepare: null pointer in the weight table");
    for (int i = 0; i < RN_CONVS; ++i)
        ARVAE_REQUIRE(w->conv_w[i] && w->bn_w[i] && w->bn_b[i] && w->bn_mean[i] && w->bn_var[i],
                      "resnet18_prepare: null pointer in the weight table (convolution %d)", i);
    hipStream_t s = as_stream(stream);
    ARVAE_LAUNCH(resnet_stem_prep_kernel, dim3((RN_STEM_TAPS * RN_STEM_C + 255) / 256), dim3(256), 0, s, w->stem_w, w->stem_bn[0],
                 w->stem_bn[1], w->stem_bn[2], w->stem_bn[3], prep);
    int rc = check_launch("resnet_stem_prep_kernel");
    if (rc) return rc;
    for (int i = 0; i < RN_CONVS; ++i) {
        const arvae_resnet18_conv_t g = net_geom(i);
        rc = launch_conv_prep(make_plan(&g), g.ksize, w->conv_w[i], w->bn_w[i], w->bn_b[i], w->bn_mean[i], w->bn_var[i],
                              prep + net_conv_offset(i), s);
        if (rc) return rc;
    }
    float *fc = prep + net_conv_offset(RN_CONVS);
    ARVAE_LAUNCH(resnet_copy_kernel, dim3((RN_CLASSES * RN_FEAT + 255) / 256), dim3(256), 0, s, w->fc_w, fc, RN_CLASSES * RN_FEAT);
    rc = check_launch("resnet_copy_kernel");
    if (rc) return rc;
    ARVAE_LAUNCH(resnet_copy_kernel, dim3(1), dim3(256), 0, s, w->fc_b, fc + RN_CLASSES * RN_FEAT, RN_CLASSES);
    return check_launch("resnet_copy_kernel");
}

extern "C" int64_t arvae_resnet18_ws_floats(int32_t n) {
    ARVAE_REQUIRE(n >= 1 && n <= RN_MAX_BATCH, "resnet18_ws_floats: batch %d out of range 1..%d", (int)n, RN_MAX_BATCH);
    return (int64_t)n * (RN_ACT_STEM + 4 * RN_ACT_BUF);
}

extern "C" int arvae_resnet18_forward(const float *prep, const float *x, int32_t n, float *logits, float *probs, int64_t *pred, float *ws,
                                      arvae_stream_t stream) {
    ARVAE_REQUIRE(prep && x && ws, "resnet18_forward: null pointer (prep, x and ws are required)");
    ARVAE_REQUIRE(logits || probs || pred, "resnet18_forward: no output requested");
    ARVAE_REQUIRE(n >= 1 && n <= RN_MAX_BATCH, "resnet18_forward: batch %d out of range 1..%d", (int)n, RN_MAX_BATCH);
    hipStream_t s = as_stream(stream);
    float *stem = ws;
    float *buf[4];
    for (int i = 0; i < 4; ++i) buf[i] = ws + (int64_t)n * (RN_ACT_STEM + i * RN_ACT_BUF);
    int rc = launch_stem(prep, x, n, 1, stem, s);
    if (rc) return rc;
    rc = launch_pool(stem, n, RN_STEM_HW, RN_STEM_HW, RN_STEM_C, buf[0], s);
    if (rc) return rc;
    for (int i = 0; i < RN_CONVS; ++i) {
        const arvae_resnet18_conv_t g = net_geom(i);
        const NetConv &c = kNet[i];
        rc = launch_conv(make_plan(&g), prep + net_conv_offset(i), buf[c.in], n, c.res < 0 ? nullptr : buf[c.res], c.relu, buf[c.out], s);
        if (rc) return rc;
    }
    const float *fc = prep + net_conv_offset(RN_CONVS);
    return launch_head(fc, fc + RN_CLASSES * RN_FEAT, buf[0], n, logits, probs, pred, s);
}
