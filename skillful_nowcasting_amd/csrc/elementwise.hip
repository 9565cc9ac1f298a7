// ConvGRU gating and the small elementwise kernels of the step, for gfx950: 16 bytes per lane where the length allows.
#include "common.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// ------------------------------------------------------------------------------------------------
// ConvGRU gating, elementwise
// ------------------------------------------------------------------------------------------------
__global__ void gru_gate_fwd_kernel(const f32x4* __restrict__ pr, const f32x4* __restrict__ h, f32x4* __restrict__ rh, int64_t n4) {
    GRID_STRIDE(i, n4) {
        const f32x4 p = pr[i], hv = h[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = sigmoidf_(p[j]) * hv[j];
        rh[i] = o;
    }
}

__global__ void gru_gate_bwd_kernel(const f32x4* __restrict__ d_rh, const f32x4* __restrict__ pr, const f32x4* __restrict__ h,
                                    f32x4* __restrict__ dpr, f32x4* __restrict__ dh, int64_t n4) {
    GRID_STRIDE(i, n4) {
        const f32x4 g = d_rh[i], p = pr[i], hv = h[i];
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = sigmoidf_(p[j]);
            a[j] = g[j] * hv[j] * s * (1.f - s);
            b[j] = g[j] * s;
        }
        dpr[i] = a;
        dh[i] = b;
    }
}

__global__ void gru_blend_fwd_kernel(const f32x4* __restrict__ pu, const f32x4* __restrict__ h, const f32x4* __restrict__ pc,
                                     f32x4* __restrict__ out, int64_t n4) {
    GRID_STRIDE(i, n4) {
        const f32x4 u = pu[i], hv = h[i], c = pc[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = sigmoidf_(u[j]);
            o[j] = s * hv[j] + (1.f - s) * fmaxf(c[j], 0.f);
        }
        out[i] = o;
    }
}

__global__ void gru_blend_bwd_kernel(const f32x4* __restrict__ dout, const f32x4* __restrict__ pu, const f32x4* __restrict__ h,
                                     const f32x4* __restrict__ pc, f32x4* __restrict__ dpu, f32x4* __restrict__ dh,
                                     f32x4* __restrict__ dpc, int64_t n4) {
    GRID_STRIDE(i, n4) {
        const f32x4 g = dout[i], u = pu[i], hv = h[i], c = pc[i];
        f32x4 a, b, d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = sigmoidf_(u[j]);
            const float rc = fmaxf(c[j], 0.f);
            a[j] = g[j] * (hv[j] - rc) * s * (1.f - s);
            b[j] = g[j] * s;
            d[j] = c[j] > 0.f ? g[j] * (1.f - s) : 0.f;
        }
        dpu[i] = a;
        dh[i] = b;
        dpc[i] = d;
    }
}

// count += number of NaN / Inf among x (exponent field all ones); integer atomics: order-independent
__global__ void nonfinite_count_kernel(const float* __restrict__ x, int64_t n, int32_t* __restrict__ count) {
    int bad = 0;
    GRID_STRIDE(i, n) bad += ((__float_as_uint(x[i]) & 0x7f800000u) == 0x7f800000u) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, bad);
}

__global__ void axpby_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, float alpha,
                             float beta, int64_t n) {
    GRID_STRIDE(i, n) y[i] = b ? alpha * a[i] + beta * b[i] : alpha * a[i];
}

__global__ void scale_by_dev_kernel(const float* __restrict__ x, const float* __restrict__ s, float host_scale,
                                    float* __restrict__ y, int64_t n) {
    const float f = s[0] * host_scale;
    GRID_STRIDE(i, n) y[i] = x[i] * f;
}

__global__ void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int64_t n) {
    GRID_STRIDE(i, n) dx[i] = x[i] > 0.f ? dy[i] : 0.f;
}

__global__ void fill_kernel(float* __restrict__ p, float v, int64_t n) { GRID_STRIDE(i, n) p[i] = v; }

}  // namespace

#define CHECK_N4(n) DGMR_CHECK_ARG((n) > 0 && (n) % 4 == 0, "%s: n=%lld must be a positive multiple of 4", __func__, (long long)(n))

extern "C" int dgmr_gru_gate_fwd(const float* pr, const float* h, float* rh, int64_t n, void* stream) {
    CHECK_N4(n);
    hipLaunchKernelGGL(gru_gate_fwd_kernel, dim3(ew_blocks(n / 4)), dim3(EW_THREADS), 0, ST, (const f32x4*)pr, (const f32x4*)h,
                       (f32x4*)rh, n / 4);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_gru_gate_bwd(const float* d_rh, const float* pr, const float* h, float* dpr, float* dh, int64_t n, void* stream) {
    CHECK_N4(n);
    hipLaunchKernelGGL(gru_gate_bwd_kernel, dim3(ew_blocks(n / 4)), dim3(EW_THREADS), 0, ST, (const f32x4*)d_rh, (const f32x4*)pr,
                       (const f32x4*)h, (f32x4*)dpr, (f32x4*)dh, n / 4);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_gru_blend_fwd(const float* pu, const float* h, const float* pc, float* out, int64_t n, void* stream) {
    CHECK_N4(n);
    hipLaunchKernelGGL(gru_blend_fwd_kernel, dim3(ew_blocks(n / 4)), dim3(EW_THREADS), 0, ST, (const f32x4*)pu, (const f32x4*)h,
                       (const f32x4*)pc, (f32x4*)out, n / 4);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_gru_blend_bwd(const float* dout, const float* pu, const float* h, const float* pc, float* dpu, float* dh,
                                  float* dpc, int64_t n, void* stream) {
    CHECK_N4(n);
    hipLaunchKernelGGL(gru_blend_bwd_kernel, dim3(ew_blocks(n / 4)), dim3(EW_THREADS), 0, ST, (const f32x4*)dout, (const f32x4*)pu,
                       (const f32x4*)h, (const f32x4*)pc, (f32x4*)dpu, (f32x4*)dh, (f32x4*)dpc, n / 4);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_nonfinite_count(const float* x, int64_t n, int32_t* count, void* stream) {
    DGMR_CHECK_ARG(x && count && n > 0, "dgmr_nonfinite_count: bad args");
    hipLaunchKernelGGL(nonfinite_count_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, ST, x, n, count);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_axpby(const float* a, const float* b, float* y, float alpha, float beta, int64_t n, void* stream) {
    DGMR_CHECK_ARG(a && y && n > 0, "dgmr_axpby: bad args");
    hipLaunchKernelGGL(axpby_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, ST, a, b, y, alpha, beta, n);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_scale_by_dev(const float* x, const float* s, float host_scale, float* y, int64_t n, void* stream) {
    DGMR_CHECK_ARG(x && s && y && n > 0, "dgmr_scale_by_dev: bad args");
    hipLaunchKernelGGL(scale_by_dev_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, ST, x, s, host_scale, y, n);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_relu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
    DGMR_CHECK_ARG(dy && x && dx && n > 0, "dgmr_relu_bwd: bad args");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, ST, dy, x, dx, n);
    DGMR_CHECK_LAUNCH();
    return 0;
}
extern "C" int dgmr_fill(float* p, float value, int64_t n, void* stream) {
    DGMR_CHECK_ARG(p && n > 0, "dgmr_fill: bad args");
    hipLaunchKernelGGL(fill_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, ST, p, value, n);
    DGMR_CHECK_LAUNCH();
    return 0;
}
