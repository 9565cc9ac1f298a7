// The optimiser of the DGMR step for gfx950: Adam for one tensor and for every tensor of an optimiser in one launch - plain, on
// clipped gradients (the gradient guard) and with the weight EMA in the same pass -, the guard's global gradient norm, and the
// evaluation swap.  All HBM-bound: one element function, one workgroup -> chunk mapping and one chunk walk serve every kernel.
#include <cmath>

#include "common.h"

namespace {

constexpr int ADAM_CHUNK = 4096;  // elements per workgroup of the multi-tensor kernels

struct AdamScalars {
    float w1 /* 1 - beta1 */, beta2, w2 /* 1 - beta2 */, eps;
};

// torch.optim.Adam's update, scalar for scalar (torch/optim/adam.py, _multi_tensor_adam): exp_avg.lerp_(grad, 1 - beta1);
// exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2); denom = sqrt(exp_avg_sq) / sqrt(bias_correction2) + eps;
// param.addcdiv_(exp_avg, denom, value = -lr / bias_correction1).  The scalars are formed in double on the host and rounded to
// float once, as torch does (1 - 0.999 in float arithmetic is 4.7e-5 off).  GUARDED: on g * coef, the product rounded to float on
// its own, as clip_grad_norm_'s g.mul_ stores it.  EVERY Adam kernel updates its elements through this function: that is what makes
// the per-tensor launch, the multi-tensor launch, the guarded one at coefficient 1 and the EMA one agree bit for bit.
template <bool GUARDED>
__device__ __forceinline__ void adam_element(float g, float coef, float& m, float& v, float& p, const AdamScalars& s, float step_size,
                                             float bc2_sqrt) {
    const float gi = GUARDED ? __fmul_rn(g, coef) : g, m0 = m;
    const float diff = gi - m0;
    const float mi = s.w1 < 0.5f ? fmaf(s.w1, diff, m0) : gi - diff * (1.f - s.w1);  // at::lerp
    const float vi = fmaf(s.w2 * gi, gi, s.beta2 * v);
    m = mi;
    v = vi;
    p -= step_size * (mi / (sqrtf(vi) / bc2_sqrt + s.eps));
}

// torch.optim.swa_utils.get_ema_multi_avg_fn: ema.lerp_(param, 1 - decay) towards the float just formed for p (at::lerp's two branches).
__device__ __forceinline__ void ema_element(float p, float& e, float we) {
    const float e0 = e;
    e = we < 0.5f ? fmaf(we, p - e0, e0) : p - (p - e0) * (1.f - we);
}

// Workgroup -> (descriptor, first element, elements left) when every tensor gets ceil(n / ADAM_CHUNK) workgroups: the last descriptor
// whose block0 <= b, by bisection.  Blocks count from descs[0].block0, so `descs` may be one parameter group's slice of a larger table.
struct AdamBlock {
    int t;
    int64_t i0, left;  // left > 0 by construction of block0
};
__device__ __forceinline__ AdamBlock adam_block(const dgmr_adam_desc* __restrict__ descs, int n_tensors) {
    const int b = blockIdx.x + descs[0].block0;
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].block0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const int64_t i0 = (int64_t)(b - descs[lo].block0) * ADAM_CHUNK;
    return {lo, i0, descs[lo].n - i0};
}

// One workgroup's chunk: f(r, x) on every element, in place.  r: the element of the read-only array `ro` (RO; the gradient), x[a]: that
// of the read-write array rw[a], a < NRW.  Thread t owns elements 4t .. 4t + 3 of each 1024-element quarter and calls f on them in
// element order (the gradient norm's bits depend on that), with the loads of all quarters in flight before the first call and the
// stores after it.  A whole chunk whose rw pointers are 16-byte aligned moves as f32x4; ro then moves the same way when it is aligned
// and dword by dword when it is a 4-byte aligned view into a flat gradient buffer.  Everything else (a tensor's last chunk, short
// tensors, parameters that are views) moves dword by dword, bounds-checked.
template <bool RO, int NRW, class F>
__device__ __forceinline__ void walk_chunk(const float* ro, float* const* rw, int64_t left, F f) {
    constexpr int Q = ADAM_CHUNK / 1024, N = NRW > 0 ? NRW : 1;
    const int lane = threadIdx.x * 4;
    f32x4 r[Q], x[N][Q];
    uintptr_t align = 0;
#pragma unroll
    for (int a = 0; a < NRW; ++a) align |= reinterpret_cast<uintptr_t>(rw[a]);
    const bool whole = left >= ADAM_CHUNK, wide = whole && (align & 15) == 0;
    if (wide) {
        if (RO && (reinterpret_cast<uintptr_t>(ro) & 15) == 0) {
#pragma unroll
            for (int k = 0; k < Q; ++k) r[k] = *reinterpret_cast<const f32x4*>(ro + k * 1024 + lane);
        } else if (RO) {
#pragma unroll
            for (int k = 0; k < Q; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) r[k][j] = ro[k * 1024 + lane + j];
        }
#pragma unroll
        for (int k = 0; k < Q; ++k)
#pragma unroll
            for (int a = 0; a < NRW; ++a) x[a][k] = *reinterpret_cast<const f32x4*>(rw[a] + k * 1024 + lane);
    } else {
#pragma unroll
        for (int k = 0; k < Q; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = k * 1024 + lane + j;
                if (RO) r[k][j] = i < left ? ro[i] : 0.f;
#pragma unroll
                for (int a = 0; a < NRW; ++a) x[a][k][j] = i < left ? rw[a][i] : 0.f;
            }
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!whole && k * 1024 + lane + j >= left) continue;
            float y[N];
#pragma unroll
            for (int a = 0; a < NRW; ++a) y[a] = x[a][k][j];
            f(RO ? r[k][j] : 0.f, y);
#pragma unroll
            for (int a = 0; a < NRW; ++a) x[a][k][j] = y[a];
            if (!wide)
#pragma unroll
                for (int a = 0; a < NRW; ++a) rw[a][k * 1024 + lane + j] = y[a];
        }
        if (wide)
#pragma unroll
            for (int a = 0; a < NRW; ++a) *reinterpret_cast<f32x4*>(rw[a] + k * 1024 + lane) = x[a][k];
    }
}

// One tensor per launch: the reference the multi-tensor tests compare against.
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                            AdamScalars s, float step_size, float bc2_sqrt) {
    GRID_STRIDE(i, n) adam_element<false>(g[i], 1.f, m[i], v[i], p[i], s, step_size, bc2_sqrt);
}

// Every tensor of an optimiser (or of one parameter group's slice of its table) in ONE launch, 28 bytes per element.  GUARDED: on
// g * guard->clip_coef, and nothing is stored when the guard says skip.  EMA: the shadow ema[t] (the array parallel to descs; NULL = no
// shadow, the tensor is updated as without EMA) moves in the same pass - 36 bytes per element, no second launch and no second read of p.
template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(256) void adam_multi_kernel(const dgmr_adam_desc* __restrict__ descs, float* const* __restrict__ ema,
                                                         int n_tensors, AdamScalars s, float we,
                                                         const dgmr_grad_guard* __restrict__ guard) {
    float coef = 1.f;
    if (GUARDED) {
        if (guard->skipped != 0) return;
        coef = guard->clip_coef;
    }
    const AdamBlock at = adam_block(descs, n_tensors);
    const dgmr_adam_desc d = descs[at.t];
    float* const e = EMA ? ema[at.t] : nullptr;
    float* const rw[4] = {d.p + at.i0, d.m + at.i0, d.v + at.i0, e ? e + at.i0 : nullptr};
    const auto adam = [&](float g, float* x) { adam_element<GUARDED>(g, coef, x[1], x[2], x[0], s, d.step_size, d.bc2_sqrt); };
    if (EMA && e)
        walk_chunk<true, 4>(d.g + at.i0, rw, at.left, [&](float g, float* x) {
            adam(g, x);
            ema_element(x[0], x[3], we);
        });
    else
        walk_chunk<true, 3>(d.g + at.i0, rw, at.left, adam);
}

// ------------------------------------------------------------------------------------------------
// gradient guard: global L2 norm (torch.nn.utils.clip_grad_norm_), clip coefficient, skip on NaN / Inf
// ------------------------------------------------------------------------------------------------
// Fixed-order sum over a 256-thread workgroup: xor butterfly inside each wave64, then the four wave sums in wave order.
__device__ __forceinline__ double block_sum_f64(double v, double* smem /* 4 doubles */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

// Stage 1, the workgroup -> chunk mapping of adam_multi_kernel: each thread adds the squares of its elements in walk_chunk's order,
// whichever load path brings them in.  fp32 -> double is exact and so is the square: one rounding per add.
__global__ __launch_bounds__(256) void grad_sq_partial_kernel(const dgmr_adam_desc* __restrict__ descs, int n_tensors,
                                                              double* __restrict__ partials) {
    __shared__ double red[4];
    const AdamBlock at = adam_block(descs, n_tensors);
    double s = 0.0;
    walk_chunk<true, 0>(descs[at.t].g + at.i0, nullptr, at.left, [&](float g, float*) { s += (double)g * (double)g; });
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// Stage 2, one workgroup per tensor: thread t adds the tensor's partials t, t + 256, ... in increasing order, then block_sum_f64.
__global__ __launch_bounds__(256) void grad_sq_tensor_kernel(const dgmr_adam_desc* __restrict__ descs, int n_tensors, int total_blocks,
                                                             const double* __restrict__ partials, double* __restrict__ tensor_sq) {
    __shared__ double red[4];
    const int t = blockIdx.x, first = descs[0].block0;
    const int b0 = descs[t].block0 - first, b1 = t + 1 < n_tensors ? descs[t + 1].block0 - first : total_blocks;
    double s = 0.0;
    for (int b = b0 + threadIdx.x; b < b1; b += 256) s += partials[b];
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) tensor_sq[t] = s;
}

// Stage 3, one workgroup: the tensors' sums added one after the other in table order (a few hundred adds; staged through LDS 256 at a
// time so that the loads are coalesced), then the guard record.  A plain running sum is unchanged by tensors whose gradient is all
// zero: flat gradient buffers, which give every parameter a (zero) gradient, yield the bits of the run where those have none.
__global__ __launch_bounds__(256) void grad_guard_finish_kernel(const double* __restrict__ tensor_sq, int n_tensors, float max_norm,
                                                                int skip_nonfinite, dgmr_grad_guard* __restrict__ guard) {
    __shared__ double tile[256];
    double s = 0.0;
    for (int t0 = 0; t0 < n_tensors; t0 += 256) {
        tile[threadIdx.x] = t0 + threadIdx.x < n_tensors ? tensor_sq[t0 + threadIdx.x] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0)
#pragma unroll 16
            for (int k = 0; k < 256; ++k) s += tile[k];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float total_norm = (float)sqrt(s);
    float coef = 1.f;
    if (max_norm > 0.f) {  // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0) in float; NaN passes through clamp
        coef = max_norm / (total_norm + 1e-6f);
        coef = coef > 1.f ? 1.f : coef;
    }
    const int skipped = skip_nonfinite && !isfinite(total_norm) ? 1 : 0;
    guard->total_norm = total_norm;
    guard->clip_coef = coef;
    guard->skipped = skipped;
    guard->skipped_total += skipped;
}

// p <-> shadow, every tensor in one launch (the evaluation swap: what swa_utils users do with AveragedModel.module, in place here
// because the modules' caches are keyed on the parameters' addresses).  Reads p, n and block0 of the descriptor only.
__global__ __launch_bounds__(256) void swap_multi_kernel(const dgmr_adam_desc* __restrict__ descs, float* const* __restrict__ ema,
                                                         int n_tensors) {
    const AdamBlock at = adam_block(descs, n_tensors);
    if (ema[at.t] == nullptr) return;
    float* const rw[2] = {descs[at.t].p + at.i0, ema[at.t] + at.i0};
    walk_chunk<false, 2>(nullptr, rw, at.left, [](float, float* x) {
        const float p = x[0];
        x[0] = x[1];
        x[1] = p;
    });
}

// The one place that picks the instantiation: a guard record -> GUARDED, a shadow array -> EMA.
int adam_multi(const dgmr_adam_desc* descs, float* const* ema, int n_tensors, int total_blocks, double beta1, double beta2, double eps,
               double ema_weight, const dgmr_grad_guard* guard, void* stream) {
    const auto kernel = guard ? (ema ? adam_multi_kernel<true, true> : adam_multi_kernel<true, false>)
                              : (ema ? adam_multi_kernel<false, true> : adam_multi_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(total_blocks), dim3(256), 0, ST, descs, ema, n_tensors,
                       AdamScalars{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps}, (float)ema_weight, guard);
    DGMR_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int dgmr_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                         int step, void* stream) {
    DGMR_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "dgmr_adam: bad args");
    DGMR_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "dgmr_adam: betas (%g, %g) out of [0, 1)", beta1, beta2);
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    hipLaunchKernelGGL(adam_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), 0, ST, p, g, m, v, n,
                       AdamScalars{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps}, (float)(lr / bc1),
                       (float)std::sqrt(bc2));
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_adam_chunk(void) { return ADAM_CHUNK; }

extern "C" int dgmr_adam_multi(const dgmr_adam_desc* descs, int n_tensors, int total_blocks, double beta1, double beta2, double eps,
                               void* stream) {
    DGMR_CHECK_ARG(descs && n_tensors > 0 && total_blocks > 0, "dgmr_adam_multi: bad args");
    return adam_multi(descs, nullptr, n_tensors, total_blocks, beta1, beta2, eps, 0.0, nullptr, stream);
}

extern "C" int dgmr_grad_norm_multi(const dgmr_adam_desc* descs, int n_tensors, int total_blocks, double* partials, double* tensor_sq,
                                    double max_norm, int skip_nonfinite, dgmr_grad_guard* guard, void* stream) {
    DGMR_CHECK_ARG(descs && partials && tensor_sq && guard, "dgmr_grad_norm_multi: null pointer");
    DGMR_CHECK_ARG(n_tensors > 0 && total_blocks > 0, "dgmr_grad_norm_multi: n_tensors=%d total_blocks=%d must be positive", n_tensors,
                   total_blocks);
    DGMR_CHECK_ARG(max_norm == max_norm, "dgmr_grad_norm_multi: max_norm is NaN");
    hipLaunchKernelGGL(grad_sq_partial_kernel, dim3(total_blocks), dim3(256), 0, ST, descs, n_tensors, partials);
    hipLaunchKernelGGL(grad_sq_tensor_kernel, dim3(n_tensors), dim3(256), 0, ST, descs, n_tensors, total_blocks, partials, tensor_sq);
    hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(256), 0, ST, tensor_sq, n_tensors, max_norm > 0.0 ? (float)max_norm : 0.f,
                       skip_nonfinite, guard);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_adam_multi_guarded(const dgmr_adam_desc* descs, int n_tensors, int total_blocks, double beta1, double beta2,
                                       double eps, const dgmr_grad_guard* guard, void* stream) {
    DGMR_CHECK_ARG(descs && guard, "dgmr_adam_multi_guarded: null pointer");
    DGMR_CHECK_ARG(n_tensors > 0 && total_blocks > 0, "dgmr_adam_multi_guarded: n_tensors=%d total_blocks=%d must be positive", n_tensors,
                   total_blocks);
    return adam_multi(descs, nullptr, n_tensors, total_blocks, beta1, beta2, eps, 0.0, guard, stream);
}

extern "C" int dgmr_adam_multi_ema(const dgmr_adam_desc* descs, float* const* ema, int n_tensors, int total_blocks, double beta1,
                                   double beta2, double eps, double ema_weight, const dgmr_grad_guard* guard, void* stream) {
    DGMR_CHECK_ARG(descs && ema, "dgmr_adam_multi_ema: null pointer");
    DGMR_CHECK_ARG(n_tensors > 0 && total_blocks > 0, "dgmr_adam_multi_ema: n_tensors=%d total_blocks=%d must be positive", n_tensors,
                   total_blocks);
    DGMR_CHECK_ARG(ema_weight >= 0.0 && ema_weight <= 1.0, "dgmr_adam_multi_ema: ema_weight=%g out of [0, 1]", ema_weight);  // (NaN too)
    return adam_multi(descs, ema, n_tensors, total_blocks, beta1, beta2, eps, ema_weight, guard, stream);
}

extern "C" int dgmr_swap_multi(const dgmr_adam_desc* descs, float* const* ema, int n_tensors, int total_blocks, void* stream) {
    DGMR_CHECK_ARG(descs && ema, "dgmr_swap_multi: null pointer");
    DGMR_CHECK_ARG(n_tensors > 0 && total_blocks > 0, "dgmr_swap_multi: n_tensors=%d total_blocks=%d must be positive", n_tensors,
                   total_blocks);
    hipLaunchKernelGGL(swap_multi_kernel, dim3(total_blocks), dim3(256), 0, ST, descs, ema, n_tensors);
    DGMR_CHECK_LAUNCH();
    return 0;
}
