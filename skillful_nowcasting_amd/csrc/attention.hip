// ------------------------------------------------------------------------------------------------
// latent attention (dgmr/layers/Attention.py:9-20).  Tensors are one sample, channels-last [H][W][Cq]; the
// reference's einsum treats the NCHW view [Cq][H][W] as "[h w c]": position p = cq*H + y, feature = x.
// ------------------------------------------------------------------------------------------------
#include "common.h"

namespace {

__device__ __forceinline__ size_t att_addr(int p, int f, int Cq, int H, int W) {
    const int cq = p / H, y = p - cq * H;
    return ((size_t)y * W + f) * Cq + cq;
}

__global__ void attention_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                     float* __restrict__ beta, float* __restrict__ out, int Cq, int H, int W) {
    extern __shared__ float sh[];  // logits [L] + red[32]
    const int L = Cq * H, p = blockIdx.x;
    float* logit = sh;
    float* red = sh + L;
    float mx = -INFINITY;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        float s = 0.f;
        for (int f = 0; f < W; ++f) s = fmaf(q[att_addr(p, f, Cq, H, W)], k[att_addr(l, f, Cq, H, W)], s);
        logit[l] = s;
        mx = fmaxf(mx, s);
    }
    // block max
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = red[0];
    for (int i = 1; i < (int)((blockDim.x + 63) >> 6); ++i) mx = fmaxf(mx, red[i]);
    float sum = 0.f;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const float e = __expf(logit[l] - mx);
        logit[l] = e;
        sum += e;
    }
    sum = block_sum(sum, red);
    const float inv = 1.f / sum;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const float bv = logit[l] * inv;
        logit[l] = bv;
        beta[(size_t)p * L + l] = bv;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < W; f += blockDim.x) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) s = fmaf(logit[l], v[att_addr(l, f, Cq, H, W)], s);
        out[att_addr(p, f, Cq, H, W)] = s;
    }
}

// per query position p: dlogit[p][l] = beta*(dbeta - sum_l beta*dbeta) -> tmp ; dq[p][f] = sum_l dlogit*k[l][f]
__global__ void attention_bwd_q_kernel(const float* __restrict__ dout, const float* __restrict__ k, const float* __restrict__ v,
                                       const float* __restrict__ beta, float* __restrict__ dq, float* __restrict__ tmp, int Cq,
                                       int H, int W) {
    extern __shared__ float sh[];
    const int L = Cq * H, p = blockIdx.x;
    float* dl = sh;
    float* red = sh + L;
    float dot = 0.f;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        float s = 0.f;
        for (int f = 0; f < W; ++f) s = fmaf(dout[att_addr(p, f, Cq, H, W)], v[att_addr(l, f, Cq, H, W)], s);
        dl[l] = s;
        dot = fmaf(beta[(size_t)p * L + l], s, dot);
    }
    dot = block_sum(dot, red);
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const float g = beta[(size_t)p * L + l] * (dl[l] - dot);
        dl[l] = g;
        tmp[(size_t)p * L + l] = g;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < W; f += blockDim.x) {
        float s = 0.f;
        for (int l = 0; l < L; ++l) s = fmaf(dl[l], k[att_addr(l, f, Cq, H, W)], s);
        dq[att_addr(p, f, Cq, H, W)] = s;
    }
}

// per key position l: dk[l][f] = sum_p dlogit[p][l]*q[p][f]; dv[l][f] = sum_p beta[p][l]*dout[p][f]
__global__ void attention_bwd_kv_kernel(const float* __restrict__ dout, const float* __restrict__ q, const float* __restrict__ beta,
                                        const float* __restrict__ tmp, float* __restrict__ dk, float* __restrict__ dv, int Cq, int H,
                                        int W) {
    const int L = Cq * H, l = blockIdx.x;
    for (int f = threadIdx.x; f < W; f += blockDim.x) {
        float a = 0.f, b = 0.f;
        for (int p = 0; p < L; ++p) {
            a = fmaf(tmp[(size_t)p * L + l], q[att_addr(p, f, Cq, H, W)], a);
            b = fmaf(beta[(size_t)p * L + l], dout[att_addr(p, f, Cq, H, W)], b);
        }
        dk[att_addr(l, f, Cq, H, W)] = a;
        dv[att_addr(l, f, Cq, H, W)] = b;
    }
}

}  // namespace

extern "C" int dgmr_attention_fwd(const float* q, const float* k, const float* v, float* beta, float* out, int Cq, int H, int W,
                                  void* stream) {
    DGMR_CHECK_ARG(q && k && v && beta && out, "dgmr_attention_fwd: null pointer");
    const int L = Cq * H;
    hipLaunchKernelGGL(attention_fwd_kernel, dim3(L), dim3(256), (L + 32) * sizeof(float), ST, q, k, v, beta, out, Cq, H, W);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_attention_bwd(const float* dout, const float* q, const float* k, const float* v, const float* beta, float* dq,
                                  float* dk, float* dv, float* tmp, int Cq, int H, int W, void* stream) {
    DGMR_CHECK_ARG(dout && q && k && v && beta && dq && dk && dv && tmp, "dgmr_attention_bwd: null pointer");
    const int L = Cq * H;
    hipLaunchKernelGGL(attention_bwd_q_kernel, dim3(L), dim3(256), (L + 32) * sizeof(float), ST, dout, k, v, beta, dq, tmp, Cq, H, W);
    hipLaunchKernelGGL(attention_bwd_kv_kernel, dim3(L), dim3(64), 0, ST, dout, q, beta, tmp, dk, dv, Cq, H, W);
    DGMR_CHECK_LAUNCH();
    return 0;
}
