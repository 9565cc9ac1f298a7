// The discriminator heads (relu-sum pooling, the one-output linear layer) and the two losses (hinge, grid-cell) for gfx950.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// discriminator heads
// ------------------------------------------------------------------------------------------------
__global__ void relu_sum_hw_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int HW, int C) {
    GRID_STRIDE(i, (int64_t)N * C) {
        const int c = i % C;
        const int n = i / C;
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += fmaxf(x[((size_t)n * HW + p) * C + c], 0.f);
        y[i] = s;
    }
}

__global__ void relu_sum_hw_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int N,
                                       int HW, int C) {
    GRID_STRIDE(i, (int64_t)N * HW * C) {
        const int c = i % C;
        const int n = i / ((int64_t)HW * C);
        dx[i] = x[i] > 0.f ? dy[(size_t)n * C + c] : 0.f;
    }
}

__global__ void linear1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                   const float* __restrict__ scale, float* __restrict__ y, int C, int scale_group) {
    __shared__ float red[32];
    const int n = blockIdx.x;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) s = fmaf(x[(size_t)n * C + c], w[c], s);
    s = block_sum(s, red);
    if (threadIdx.x == 0) y[n] = s * (scale ? scale[n / scale_group] : 1.f) + (bias ? bias[0] : 0.f);
}

// one thread per (group, channel): dx rows of the group, the group's raw weight gradient; thread (0,0) also the bias gradient
__global__ void linear1_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                   const float* __restrict__ scale, float* __restrict__ dx, float* __restrict__ gw_raw,
                                   float* __restrict__ gb, int N, int C, int scale_group) {
    const int groups = N / scale_group;
    GRID_STRIDE(i, (int64_t)groups * C) {
        const int c = i % C, q = i / C;
        float g = 0.f;
        const float wc = w[c] * (scale ? scale[q] : 1.f);
        for (int n = q * scale_group; n < (q + 1) * scale_group; ++n) {
            const float d = dy[n];
            dx[(size_t)n * C + c] = d * wc;
            g = fmaf(d, x[(size_t)n * C + c], g);
        }
        gw_raw[(size_t)q * C + c] = g;
        if (i == 0 && gb) {
            float s = 0.f;
            for (int n = 0; n < N; ++n) s += dy[n];
            gb[0] = s;
        }
    }
}

// dst[t][n][i] = src[n][t][i]  (16-byte items)
__global__ void permute_nt_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, int N, int T, int64_t inner4) {
    const int64_t total = (int64_t)N * T * inner4;
    GRID_STRIDE(j, total) {
        const int64_t i = j % inner4;
        const int64_t r = j / inner4;
        const int n = r % N, t = r / N;
        dst[j] = src[((int64_t)n * T + t) * inner4 + i];
    }
}

// ------------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------------
__global__ void hinge_disc_kernel(const float* __restrict__ s_real, const float* __restrict__ s_gen, float* __restrict__ loss,
                                  float* __restrict__ d_real, float* __restrict__ d_gen, int n_real, int n_gen) {
    __shared__ float red[32];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < n_real; i += blockDim.x) {
        const float v = 1.f - s_real[i];
        a += fmaxf(v, 0.f);
        if (d_real) d_real[i] = v > 0.f ? -1.f / n_real : 0.f;
    }
    for (int i = threadIdx.x; i < n_gen; i += blockDim.x) {
        const float v = 1.f + s_gen[i];
        b += fmaxf(v, 0.f);
        if (d_gen) d_gen[i] = v > 0.f ? 1.f / n_gen : 0.f;
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) loss[0] = a / n_real + b / n_gen;
}

__global__ void grid_cell_kernel(const float* __restrict__ preds, int K, int64_t stride, const float* __restrict__ target,
                                 const float* __restrict__ weights, float cap, double* __restrict__ acc, float* __restrict__ dweight,
                                 int64_t n, int det) {
    __shared__ float red[32];
    float s = 0.f;
    const float invK = 1.f / (float)K;
    GRID_STRIDE(i, n) {
        float m = 0.f;
        for (int k = 0; k < K; ++k) m += preds[(size_t)k * stride + i];
        m *= invK;
        const float y = target[i];
        const float w = weights ? weights[i] : fmaxf(y + 1.f, cap);
        const float d = (m - y) * w;
        s += fabsf(d);
        if (dweight) dweight[i] = (d > 0.f ? w : (d < 0.f ? -w : 0.f)) * invK;
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        if (det) acc[1 + blockIdx.x] = (double)s;  // deterministic mode: grid_cell_finish_kernel adds the workgroups' sums in order
        else atomicAdd(acc, (double)s);
    }
}

__global__ __launch_bounds__(256) void grid_cell_finish_kernel(double* __restrict__ acc, float* __restrict__ loss, float mult, int nb) {
    // deterministic mode: the workgroups' sums acc[1 .. nb] in a fixed order - thread t takes rows b = t (mod 256) in increasing order,
    // thread 0 adds the 256 partial sums in thread order
    __shared__ double part[256];
    if (nb > 0) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nb; b += 256) a += acc[1 + b];
        part[threadIdx.x] = a;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int k = 0; k < 256; ++k) t += part[k];
            acc[0] += t;
        }
    }
    if (threadIdx.x != 0) return;
    loss[0] = (float)(acc[0] * (double)mult);
    acc[0] = 0.0;
}

}  // namespace

extern "C" int dgmr_relu_sum_hw_fwd(const float* x, float* y, int N, int HW, int C, void* stream) {
    DGMR_CHECK_ARG(x && y, "dgmr_relu_sum_hw_fwd: null pointer");
    hipLaunchKernelGGL(relu_sum_hw_fwd_kernel, dim3(ew_blocks((int64_t)N * C)), dim3(EW_THREADS), 0, ST, x, y, N, HW, C);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_relu_sum_hw_bwd(const float* dy, const float* x, float* dx, int N, int HW, int C, void* stream) {
    DGMR_CHECK_ARG(dy && x && dx, "dgmr_relu_sum_hw_bwd: null pointer");
    hipLaunchKernelGGL(relu_sum_hw_bwd_kernel, dim3(ew_blocks((int64_t)N * HW * C)), dim3(EW_THREADS), 0, ST, dy, x, dx, N, HW, C);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_linear1_fwd(const float* x, const float* w, const float* bias, const float* scale, float* y, int N, int C,
                                int scale_group, void* stream) {
    DGMR_CHECK_ARG(x && w && y, "dgmr_linear1_fwd: null pointer");
    if (scale_group < 1) scale_group = N;
    DGMR_CHECK_ARG(N % scale_group == 0, "dgmr_linear1_fwd: N=%d not divisible by scale_group=%d", N, scale_group);
    hipLaunchKernelGGL(linear1_fwd_kernel, dim3(N), dim3(256), 0, ST, x, w, bias, scale, y, C, scale_group);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_linear1_bwd(const float* dy, const float* x, const float* w, const float* scale, float* dx, float* gw_raw,
                                float* gb, int N, int C, int scale_group, void* stream) {
    DGMR_CHECK_ARG(dy && x && w && dx && gw_raw, "dgmr_linear1_bwd: null pointer");
    if (scale_group < 1) scale_group = N;
    DGMR_CHECK_ARG(N % scale_group == 0, "dgmr_linear1_bwd: N=%d not divisible by scale_group=%d", N, scale_group);
    const int64_t total = (int64_t)(N / scale_group) * C;
    hipLaunchKernelGGL(linear1_bwd_kernel, dim3(ew_blocks(total)), dim3(256), 0, ST, dy, x, w, scale, dx, gw_raw, gb, N, C,
                       scale_group);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_permute_nt(const float* src, float* dst, int N, int T, int64_t inner, void* stream) {
    DGMR_CHECK_ARG(src && dst && N > 0 && T > 0 && inner > 0 && inner % 4 == 0, "dgmr_permute_nt: bad args");
    const int64_t total = (int64_t)N * T * (inner / 4);
    hipLaunchKernelGGL(permute_nt_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, (const f32x4*)src, (f32x4*)dst, N, T,
                       inner / 4);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_hinge_disc(const float* s_real, const float* s_gen, float* loss, float* d_real, float* d_gen, int n_real,
                               int n_gen, void* stream) {
    DGMR_CHECK_ARG(s_real && s_gen && loss && n_real > 0 && n_gen > 0, "dgmr_hinge_disc: bad args");
    hipLaunchKernelGGL(hinge_disc_kernel, dim3(1), dim3(256), 0, ST, s_real, s_gen, loss, d_real, d_gen, n_real, n_gen);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t dgmr_grid_cell_acc_doubles(int64_t n) { return g_deterministic ? 1 + (int64_t)ew_blocks(n) : 1; }

extern "C" int dgmr_grid_cell_loss(const float* preds, int K, int64_t pred_stride, const float* target, const float* weights, float cap,
                                   double* acc, float* loss, float mult, float* dweight, int64_t n, void* stream) {
    DGMR_CHECK_ARG(preds && target && acc && loss && K > 0 && n > 0, "dgmr_grid_cell_loss: bad args");
    hipLaunchKernelGGL(grid_cell_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, ST, preds, K, pred_stride, target, weights, cap,
                       acc, dweight, n, g_deterministic);
    hipLaunchKernelGGL(grid_cell_finish_kernel, dim3(1), dim3(256), 0, ST, acc, loss, mult, g_deterministic ? ew_blocks(n) : 0);
    DGMR_CHECK_LAUNCH();
    return 0;
}
