// Kraskov-Stoegbauer-Grassberger mutual information between each of p columns x_c and one target column y: the estimator behind
// the disentanglement metrics (reference utils/evaluation.py -> sklearn.feature_selection.mutual_info_regression, whose
// _compute_mi_cc this restates rule for rule, in fp64 throughout):
//   r_i  = nextafter(k-th smallest max(|x_j - x_i|, |y_j - y_i|) over j != i, 0)     (the query point is excluded by INDEX)
//   nx_i = #{j : |x_j - x_i| <= r_i} - 1,   ny_i likewise with y
//   mi   = max(0, psi(n) + psi(k) - mean psi(nx + 1) - mean psi(ny + 1))
// Every comparison is made on the computed difference fabs(a - b) (correctly rounded, so monotone), never on shifted bounds.
//
// One launch does both all-pairs passes.  A workgroup owns 256 query points and KSG_COLS columns; the points j stream through LDS
// in tiles of 256 (as the regulariser does, regloss.h).  Each thread first keeps a sorted top-K of the joint Chebyshev distance
// per column in registers (a branchless min/max insertion network; |y_j - y_i| is shared by the columns), then, with its own
// radii known, streams the tiles a second time and counts.  The workgroup writes one psi(nx+1) + psi(ny+1) partial per column
// into the workspace; ksg_finish_kernel sums the partials in a fixed order (no float atomics: bit-reproducible).
#include <math.h>

#include "common.h"

namespace arvae {

constexpr int KSG_THREADS = 256;
constexpr int KSG_TILE = 256;
constexpr int KSG_COLS = 4;
constexpr int KSG_MAX_K = 8;

// psi(m) for an integer m >= 1: H_{m-1} - gamma directly below 16, the asymptotic series above (truncation < 1e-18 there)
__device__ __forceinline__ double psi_int(int64_t m) {
    const double euler_gamma = 0.57721566490153286061;
    if (m < 16) {
        double h = 0.0;
        for (int t = 1; t < (int)m; ++t) h += 1.0 / (double)t;
        return h - euler_gamma;
    }
    const double x = (double)m, r = 1.0 / x, r2 = r * r;
    const double series = r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 - r2 * (691.0 / 32760))))));
    return log(x) - 0.5 * r - series;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int K>
__global__ __launch_bounds__(KSG_THREADS) void ksg_kernel(const double *__restrict__ x, int64_t ldx, int p, const double *__restrict__ y,
                                                         int n, double *__restrict__ partial, double *__restrict__ radius_out,
                                                         int32_t *__restrict__ nx_out, int32_t *__restrict__ ny_out) {
    __shared__ double ys[KSG_TILE];
    __shared__ double xs[KSG_COLS][KSG_TILE];
    __shared__ double red[KSG_COLS][KSG_THREADS / 64];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * KSG_THREADS + tid;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    const int c0 = blockIdx.y * KSG_COLS;
    int col[KSG_COLS];
#pragma unroll
    for (int c = 0; c < KSG_COLS; ++c) col[c] = min(c0 + c, p - 1);       // a group's missing columns repeat the last one
    const double yi = y[ii];
    double xi[KSG_COLS];
#pragma unroll
    for (int c = 0; c < KSG_COLS; ++c) xi[c] = x[(int64_t)col[c] * ldx + ii];

    auto load_tile = [&](int j0) {
        __syncthreads();
        const int j = j0 + tid;
        if (j < n) {
            ys[tid] = y[j];
#pragma unroll
            for (int c = 0; c < KSG_COLS; ++c) xs[c][tid] = x[(int64_t)col[c] * ldx + j];
        }
        __syncthreads();
    };

    // pass 1: the K smallest joint distances per column, ascending
    double best[KSG_COLS][K];
#pragma unroll
    for (int c = 0; c < KSG_COLS; ++c)
#pragma unroll
        for (int s = 0; s < K; ++s) best[c][s] = INFINITY;
    for (int j0 = 0; j0 < n; j0 += KSG_TILE) {
        load_tile(j0);
        const int cnt = min(KSG_TILE, n - j0);
        for (int t = 0; t < cnt; ++t) {
            const double dy = (j0 + t == i) ? INFINITY : fabs(ys[t] - yi);      // the point itself never counts as a neighbour
#pragma unroll
            for (int c = 0; c < KSG_COLS; ++c) {
                double d = fmax(fabs(xs[c][t] - xi[c]), dy);
#pragma unroll
                for (int s = 0; s < K; ++s) {
                    const double lo = fmin(best[c][s], d);
                    d = fmax(best[c][s], d);
                    best[c][s] = lo;
                }
            }
        }
    }
    double r[KSG_COLS];
#pragma unroll
    for (int c = 0; c < KSG_COLS; ++c) {
        const double kth = best[c][K - 1];
        // nextafter(kth, 0) for a finite kth >= 0
        r[c] = kth > 0.0 ? __longlong_as_double(__double_as_longlong(kth) - 1) : kth;
    }

    // pass 2: marginal counts within r (the point itself included, removed below)
    int nx[KSG_COLS], ny[KSG_COLS];
#pragma unroll
    for (int c = 0; c < KSG_COLS; ++c) nx[c] = ny[c] = 0;
    for (int j0 = 0; j0 < n; j0 += KSG_TILE) {
        load_tile(j0);
        const int cnt = min(KSG_TILE, n - j0);
        for (int t = 0; t < cnt; ++t) {
            const double dy = fabs(ys[t] - yi);
#pragma unroll
            for (int c = 0; c < KSG_COLS; ++c) {
                nx[c] += fabs(xs[c][t] - xi[c]) <= r[c] ? 1 : 0;
                ny[c] += dy <= r[c] ? 1 : 0;
            }
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < KSG_COLS; ++c) {
        const bool own = valid && c0 + c < p;
        const int mx = nx[c] - 1, my = ny[c] - 1;
        if (own) {
            const int64_t o = (int64_t)(c0 + c) * n + i;
            if (radius_out) radius_out[o] = r[c];
            if (nx_out) nx_out[o] = mx;
            if (ny_out) ny_out[o] = my;
        }
        const double v = wave_sum_f64(own ? psi_int(mx + 1) + psi_int(my + 1) : 0.0);
        if (lane == 0) red[c][wave] = v;
    }
    __syncthreads();
    if (tid < KSG_COLS && c0 + tid < p) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < KSG_THREADS / 64; ++w) s += red[tid][w];
        partial[(int64_t)(c0 + tid) * gridDim.x + blockIdx.x] = s;
    }
}

// one workgroup per column: the query blocks' partials in a fixed order -> mi_out[c]
__global__ __launch_bounds__(KSG_THREADS) void ksg_finish_kernel(const double *__restrict__ partial, int nqb, int n, int k,
                                                                double *__restrict__ mi_out) {
    __shared__ double red[KSG_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int b = tid; b < nqb; b += KSG_THREADS) s += partial[(int64_t)c * nqb + b];
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int w = 0; w < KSG_THREADS / 64; ++w) total += red[w];
        const double mi = psi_int(n) + psi_int(k) - total / (double)n;
        mi_out[c] = mi > 0.0 ? mi : 0.0;
    }
}

static int64_t ksg_query_blocks(int64_t n) { return (n + KSG_THREADS - 1) / KSG_THREADS; }

}  // namespace arvae

using namespace arvae;

extern "C" int64_t arvae_ksg_ws_bytes(int64_t n, int32_t p) {
    ARVAE_REQUIRE(n > 0 && n < INT32_MAX && p >= 1, "ksg_ws_bytes: n %lld or p %d out of range", (long long)n, (int)p);
    return ksg_query_blocks(n) * (int64_t)p * (int64_t)sizeof(double);
}

extern "C" int arvae_ksg_mi(const double *x, int64_t ldx, int32_t p, const double *y, int64_t n, int32_t k, void *ws, double *mi_out,
                            double *radius_out, int32_t *nx_out, int32_t *ny_out, arvae_stream_t stream) {
    ARVAE_REQUIRE(x && y && ws && mi_out, "ksg_mi: null pointer (x, y, ws and mi_out are required)");
    ARVAE_REQUIRE(p >= 1, "ksg_mi: p = %d columns, need at least 1", (int)p);
    ARVAE_REQUIRE(k >= 1 && k <= KSG_MAX_K, "ksg_mi: k = %d neighbours, supported 1..%d", (int)k, KSG_MAX_K);
    ARVAE_REQUIRE(n > k && n < INT32_MAX, "ksg_mi: n = %lld points, need k < n < 2^31", (long long)n);
    ARVAE_REQUIRE(ldx >= n, "ksg_mi: column stride ldx = %lld < n = %lld", (long long)ldx, (long long)n);
    const int64_t nqb = ksg_query_blocks(n);
    const dim3 grid((unsigned)nqb, (unsigned)((p + KSG_COLS - 1) / KSG_COLS));
    hipStream_t s = as_stream(stream);
    double *partial = static_cast<double *>(ws);
#define ARVAE_KSG_CASE(KK)                                                                                                   \
    case KK:                                                                                                                 \
        ARVAE_LAUNCH(ksg_kernel<KK>, grid, dim3(KSG_THREADS), 0, s, x, ldx, (int)p, y, (int)n, partial, radius_out, nx_out, ny_out); \
        break;
    switch (k) {
        ARVAE_KSG_CASE(1)
        ARVAE_KSG_CASE(2)
        ARVAE_KSG_CASE(3)
        ARVAE_KSG_CASE(4)
        ARVAE_KSG_CASE(5)
        ARVAE_KSG_CASE(6)
        ARVAE_KSG_CASE(7)
        ARVAE_KSG_CASE(8)
    }
#undef ARVAE_KSG_CASE
    int rc = check_launch("ksg_kernel");
    if (rc) return rc;
    ARVAE_LAUNCH(ksg_finish_kernel, dim3((unsigned)p), dim3(KSG_THREADS), 0, s, partial, (int)nqb, (int)n, (int)k, mi_out);
    return check_launch("ksg_finish_kernel");
}
