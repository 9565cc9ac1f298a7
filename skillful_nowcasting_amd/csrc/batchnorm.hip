// Per-channel reductions over [G][R][C] and BatchNorm for gfx950: statistics, finalize, backward, column / row sums, repeats and the
// affine apply.  HBM-bound; the reductions accumulate in double so that E[x^2] - E[x]^2 stays accurate.
#include <type_traits>

#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// per-channel reductions over [G][R][C]
// ------------------------------------------------------------------------------------------------
// K: coef(int g, int c) -> the thread's loop-invariant coefficients; L: load(int64_t elem_index) -> the element's operands;
// A: acc(operands, coefficients, double& s0, double& s1).  A thread owns one (channel, row lane) and adds its rows in ascending order
// onto one chain; UNR is only how many rows' loads it issues before the additions of the first of them (1: a load, a wait and an
// addition per row - one 4-byte load in flight per lane, 2.8 TB/s with the chip to itself).
// Accumulation is in double from the first element on.  Batch variance is formed as E[x^2] - mean^2, which cancels by mean^2 / var:
// the discriminator heads normalise relu-sum features whose spread across the 8 ... 32 samples of a call is ~1 % of their mean
// (mean^2 / var ~ 1e4), and float partial sums (6e-8 x 1e4 = 6e-4 on rstd) put a 1e-3 ... 1e-2 error on every gradient behind the
// head (found by tests/test_gpu_stages.py::test_temporal_discriminator_backward_stages).  These kernels are HBM-bound either way.
constexpr int RED_UNR = 8;  // rows in flight per lane in the reductions and the two serial walks (dgmr_debug_flags 8192: 1)
template <int UNR, class K, class L, class A>
__device__ __forceinline__ void chan_reduce2(K coef, L load, A acc, int64_t R, int C, double* __restrict__ out /* [G][2][C] */, int det = 0) {
    __shared__ double l0[256], l1[256];
    const int g = blockIdx.y;
    const int64_t rows_per_block = (R + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = blockIdx.x * rows_per_block, r1 = min(R, r0 + rows_per_block);
    for (int cb = 0; cb < C; cb += 256) {
        const int Wd = min(256, C - cb);
        const int RL = 256 / Wd;
        const int c = cb + threadIdx.x % Wd, rl = threadIdx.x / Wd;
        double s0 = 0.0, s1 = 0.0;
        if (rl < RL) {
            const auto k = coef(g, c);
            const int64_t e0 = (int64_t)g * R * C + c, step = (int64_t)RL * C;  // element of row r: e0 + r * C
            int64_t r = r0 + rl;
            if constexpr (UNR > 1) {
                for (; r + (int64_t)(UNR - 1) * RL < r1; r += (int64_t)UNR * RL) {
                    decltype(load(e0)) v[UNR];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) v[u] = load(e0 + r * C + u * step);
#pragma unroll
                    for (int u = 0; u < UNR; ++u) acc(v[u], k, s0, s1);
                }
                if (r < r1) {  // the last, short batch: only rows below r1 are read
                    decltype(load(e0)) v[UNR - 1];
#pragma unroll
                    for (int u = 0; u < UNR - 1; ++u)
                        if (r + (int64_t)u * RL < r1) v[u] = load(e0 + r * C + u * step);
#pragma unroll
                    for (int u = 0; u < UNR - 1; ++u)
                        if (r + (int64_t)u * RL < r1) acc(v[u], k, s0, s1);
                }
            } else {
                for (; r < r1; r += RL) acc(load(e0 + r * C), k, s0, s1);
            }
        }
        l0[threadIdx.x] = s0;
        l1[threadIdx.x] = s1;
        __syncthreads();
        if (threadIdx.x < Wd) {
            double a0 = 0.0, a1 = 0.0;
            for (int k = 0; k < RL; ++k) {
                a0 += l0[threadIdx.x + k * Wd];
                a1 += l1[threadIdx.x + k * Wd];
            }
            if (det) {  // deterministic mode: row 1 + blockIdx.x of the caller's buffer; reduce_rows_finish_kernel adds the rows up in order
                double* row = out + (size_t)(1 + blockIdx.x) * gridDim.y * 2 * C;
                row[((size_t)g * 2 + 0) * C + c] = a0;
                row[((size_t)g * 2 + 1) * C + c] = a1;
            } else {
                atomicAdd(out + ((size_t)g * 2 + 0) * C + c, a0);
                atomicAdd(out + ((size_t)g * 2 + 1) * C + c, a1);
            }
        }
        __syncthreads();
    }
}

// out[j] += sum over rows b = 0 .. nb-1 of out[(1 + b) * n + j], in that order (deterministic mode of the per-channel reductions);
// UNR rows are loaded ahead of their additions
template <int UNR>
__global__ void reduce_rows_finish_kernel(double* __restrict__ out, int nb, int64_t n) {
    GRID_STRIDE(j, n) {
        double a = 0.0;
        int b = 0;
        if constexpr (UNR > 1)
            for (; b + UNR <= nb; b += UNR) {
                double v[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) v[u] = out[(size_t)(1 + b + u) * n + j];
#pragma unroll
                for (int u = 0; u < UNR; ++u) a += v[u];
            }
        for (; b < nb; ++b) a += out[(size_t)(1 + b) * n + j];
        out[j] += a;
    }
}

struct NoCoef {};

template <int UNR>
__global__ void bn_stats_kernel(const float* __restrict__ x, double* __restrict__ sums, int64_t R, int C, int det) {
    chan_reduce2<UNR>([](int, int) { return NoCoef{}; }, [&](int64_t i) { return x[i]; },
                      [](float xv, NoCoef, double& s0, double& s1) {
                          const double v = (double)xv;
                          s0 += v;
                          s1 = fma(v, v, s1);
                      },
                      R, C, sums, det);
}

// deterministic bn_partial_reduce: one workgroup per (32 columns, group); 8 row lanes sum rows r = lane (mod 8) in order, then in lane order
__global__ __launch_bounds__(256) void bn_partial_reduce_det_kernel(const float* __restrict__ partials, double* __restrict__ sums, int64_t R, int C2) {
    __shared__ double part[8][32];
    const int g = blockIdx.y, col = threadIdx.x & 31, lane = threadIdx.x >> 5;
    const int j = blockIdx.x * 32 + col;
    double a = 0.0;
    if (j < C2)
        for (int64_t r = lane; r < R; r += 8) a += (double)partials[((size_t)g * R + r) * C2 + j];
    part[lane][col] = a;
    __syncthreads();
    if (lane == 0 && j < C2) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += part[k][col];
        sums[(size_t)g * C2 + j] += t;
    }
}

// sums[g][k][c] += sum_r partials[(g*R + r)][k][c]: blockIdx.y = g, blockIdx.z = slice of the rows; one thread per (k, c)
__global__ void bn_partial_reduce_kernel(const float* __restrict__ partials, double* __restrict__ sums, int64_t R, int C2) {
    const int g = blockIdx.y;
    const int64_t per = (R + gridDim.z - 1) / gridDim.z;
    const int64_t r0 = blockIdx.z * per, r1 = min(R, r0 + per);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < C2; j += gridDim.x * blockDim.x) {
        double a = 0.0;
        for (int64_t r = r0; r < r1; ++r) a += (double)partials[((size_t)g * R + r) * C2 + j];
        atomicAdd(sums + (size_t)g * C2 + j, a);
    }
}

__global__ void bn_bwd_center_kernel(double* __restrict__ sums, const float* __restrict__ mean, const float* __restrict__ rstd, int GC,
                                     int C) {
    GRID_STRIDE(i, GC) {
        const int64_t g = i / C, c = i - g * C;
        double* s = sums + g * 2 * C;
        s[C + c] = (double)rstd[i] * (s[C + c] - (double)mean[i] * s[c]);
    }
}

struct GX {
    float g, x;
};
struct MeanRstd {
    float mean, rstd;
};

template <int UNR>
__global__ void bn_bwd_reduce_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ mean,
                                     const float* __restrict__ rstd, double* __restrict__ sums, int64_t R, int C, int det) {
    chan_reduce2<UNR>([&](int g, int c) { return MeanRstd{mean[(size_t)g * C + c], rstd[(size_t)g * C + c]}; },
                      [&](int64_t i) { return GX{gy[i], x[i]}; },
                      [](GX v, MeanRstd k, double& s0, double& s1) {
                          const float gv = v.g;
                          const float xh = (v.x - k.mean) * k.rstd;
                          s0 += (double)gv;
                          s1 = fma((double)gv, (double)xh, s1);
                      },
                      R, C, sums, det);
}

template <int UNR>
__global__ void colsum_kernel(const float* __restrict__ x, double* __restrict__ sums, int64_t R, int C, int det) {
    chan_reduce2<UNR>([](int, int) { return NoCoef{}; }, [&](int64_t i) { return x[i]; },
                      [](float xv, NoCoef, double& s0, double&) { s0 += (double)xv; }, R, C, sums, det);
}

// out[c] (+)= sum_r x[r][c] for FEW rows and MANY columns (one thread per 4 columns; colsum_kernel is for the opposite shape)
__global__ void sum_rows_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ out, int R, int64_t C4, int accumulate) {
    GRID_STRIDE(c, C4) {
        f32x4 s = accumulate ? out[c] : (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r) s += x[(int64_t)r * C4 + c];
        out[c] = s;
    }
}

// out[g][c] = sum_r w[(g*R + r) / rows_per_w] * x[g][r][c]  (w == nullptr: plain sums); blockIdx.y = g, one thread per 4 columns
__global__ void group_rowsum_kernel(const f32x4* __restrict__ x, const float* __restrict__ w, f32x4* __restrict__ out, int R, int64_t C4,
                                    int rows_per_w, int w_stride) {
    const int g = blockIdx.y;
    x += (int64_t)g * R * C4;
    out += (int64_t)g * C4;
    const int64_t wblock = C4 / w_stride;  // columns (in float4) that share one weight column
    GRID_STRIDE(c, C4) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        const int64_t wc = w_stride > 1 ? c / wblock : 0;
        for (int r = 0; r < R; ++r) {
            const float f = w ? w[(((int64_t)g * R + r) / rows_per_w) * w_stride + wc] : 1.f;
            s += f * x[(int64_t)r * C4 + c];
        }
        out[c] = s;
    }
}

// dst[(k*repeat + r)][:] = src[k][:]: every block of C4 float4 repeated `repeat` times in place ('k ... -> (k repeat) ...')
__global__ void repeat_interleave_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, int64_t C4, int repeat, int64_t total4) {
    GRID_STRIDE(i, total4) {
        const int64_t row = i / C4;
        dst[i] = src[(row / repeat) * C4 + (i - row * C4)];
    }
}

// dst[i][c] = src[c] for i < repeat  (einops 'b ... -> (repeat b) ...' with b == 1)
__global__ void repeat_rows_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, int64_t C4, int64_t total4) {
    GRID_STRIDE(i, total4) dst[i] = src[i % C4];
}

__global__ void colsum_finish_kernel(const double* __restrict__ sums, float* __restrict__ out, int C, int accumulate) {
    GRID_STRIDE(c, C) out[c] = (accumulate ? out[c] : 0.f) + (float)sums[c];
}

// (round 6) 64 channels x 16 group lanes per workgroup: the per-(group, channel) part - two double divisions, a double square root and a
// reciprocal: ~300 cycles - runs 16 groups at a time; only the running-statistics recurrence (two float multiply-adds per call, in the
// reference's call order) is sequential, one lane per channel reading (float) mean / unbiased variance back from LDS.  Before: one thread
// per channel walked all G groups (G = draws x steps, up to 108) - 29 us per launch, 103 launches per training step, on the forward
// passes' critical path.  Every expression is written in the contracted form the compiler had chosen for the old loop: bit-identical.
constexpr int BNF_C = 64, BNF_L = 16, BNF_Q = 64;  // channels per workgroup, group lanes, groups per LDS chunk
__global__ __launch_bounds__(BNF_C* BNF_L) void bn_finalize_kernel(const double* __restrict__ sums, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ rm,
                                                                   float* __restrict__ rv, int64_t* __restrict__ nbt,
                                                                   float* __restrict__ a, float* __restrict__ b,
                                                                   float* __restrict__ save_mean, float* __restrict__ save_rstd, int G,
                                                                   int64_t R, int C, float eps, float momentum,
                                                                   const int32_t* __restrict__ order) {
    __shared__ float s_mean[BNF_Q][BNF_C], s_unb[BNF_Q][BNF_C];
    const int cl = threadIdx.x & (BNF_C - 1), lane = threadIdx.x / BNF_C;
    const int c = blockIdx.x * BNF_C + cl;
    if (blockIdx.x == 0 && threadIdx.x == 0 && nbt && sums) nbt[0] += G;
    const bool cok = c < C;
    const float gm = (cok && gamma) ? gamma[c] : 1.f, bt = (cok && beta) ? beta[c] : 0.f;
    if (!sums) {  // eval: running statistics
        if (lane == 0 && cok) {
            const float mean = rm[c], rstd = 1.f / sqrtf(rv[c] + eps);
            a[c] = gm * rstd;
            b[c] = bt - mean * gm * rstd;
            if (save_mean) {
                save_mean[c] = mean;
                save_rstd[c] = rstd;
            }
        }
        return;
    }
    float rmc = 0.f, rvc = 0.f;
    if (lane == 0 && cok) {
        rmc = rm[c];
        rvc = rv[c];
    }
    const double Rd = (double)R, bessel = R > 1 ? (double)R / (double)(R - 1) : 1.0;
    const float keep = 1.f - momentum;
    for (int q0 = 0; q0 < G; q0 += BNF_Q) {
        const int nq = min(BNF_Q, G - q0);
        for (int qq = lane; qq < nq; qq += BNF_L) {
            // the q-th call of the module (the order in which the reference updates its running statistics) is group order[q] of the batch
            const int g = order ? order[q0 + qq] : q0 + qq;
            if (cok) {
                const double mean = sums[((size_t)g * 2 + 0) * C + c] / Rd;
                double var = fma(-mean, mean, sums[((size_t)g * 2 + 1) * C + c] / Rd);
                if (var < 0.0) var = 0.0;
                const float rstd = (float)(1.0 / sqrt(var + (double)eps));
                const float av = gm * rstd, mf = (float)mean;
                a[(size_t)g * C + c] = av;
                b[(size_t)g * C + c] = __fmaf_rn(-av, mf, bt);
                if (save_mean) {
                    save_mean[(size_t)g * C + c] = mf;
                    save_rstd[(size_t)g * C + c] = rstd;
                }
                s_mean[qq][cl] = mf;
                s_unb[qq][cl] = (float)(R > 1 ? bessel * var : var);
            }
        }
        __syncthreads();
        if (lane == 0 && cok)
            for (int qq = 0; qq < nq; ++qq) {
                rmc = __fmaf_rn(keep, rmc, __fmul_rn(momentum, s_mean[qq][cl]));
                rvc = __fmaf_rn(keep, rvc, __fmul_rn(momentum, s_unb[qq][cl]));
            }
        __syncthreads();
    }
    if (lane == 0 && cok) {
        rm[c] = rmc;
        rv[c] = rvc;
    }
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, const float* __restrict__ gamma,
                                    const double* __restrict__ sums, const float* __restrict__ dx_add, float* __restrict__ dx,
                                    int64_t R, int C, int train) {
    const int g = blockIdx.y;
    const int64_t n = R * C;
    const float invR = 1.f / (float)R;
    GRID_STRIDE(i, n) {
        const int c = i % C;
        const size_t gc = (size_t)g * C + c;
        const size_t idx = (size_t)g * n + i;
        const float gm = gamma ? gamma[c] : 1.f;
        const float rs = rstd[gc];
        float v = gy[idx];
        if (train) {
            const float xh = (x[idx] - mean[gc]) * rs;
            v = v - (float)sums[((size_t)g * 2 + 0) * C + c] * invR - xh * (float)sums[((size_t)g * 2 + 1) * C + c] * invR;
        }
        v *= gm * rs;
        if (dx_add) v += dx_add[idx];
        dx[idx] = v;
    }
}

// One float4 of the 16-byte kernel.  The scalar kernel's expression per element, v - k0 * invR - xh * k1 * invR, then * gr, then + dx_add,
// written out in the one contracted form the compiler had chosen for the former loop - v - rn(k0 * invR) first, then one fma of
// -invR and rn(xh * k1) onto it - with contraction off around it: left to the compiler, the instantiations and their predicated
// last passes came out in different forms (fma(-k0, invR, v) in some), a last-bit difference in 6 % of the elements.
typedef __attribute__((address_space(1))) f32x4 gf32x4;  // a float4 in global memory (a pointer rebuilt from two scalars keeps its space)
template <bool TRAIN>
__device__ __forceinline__ f32x4 bn_bwd_apply_quad(f32x4 v, const f32x4 xv, const f32x4 mn, const f32x4 rs, const f32x4 k0, const f32x4 k1,
                                                   const f32x4 gr, const float invR, const bool has_add, const gf32x4* add) {
#pragma clang fp contract(off)
    if constexpr (TRAIN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (xv[j] - mn[j]) * rs[j];
            v[j] = __builtin_fmaf(-invR, xh * k1[j], v[j] - k0[j] * invR);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= gr[j];
    if (has_add) v += __builtin_nontemporal_load(add);
    return v;
}

// The same, 16 bytes per lane: the grid stride is a multiple of C / 4, so a thread's channel quad - and its five coefficient quads -
// never change over its rows (the scalar kernel spends a 64-bit modulo and seven dependent loads per element: 4.3 TB/s of HBM
// traffic where a streaming kernel reaches ~6).  A lane keeps U rows in flight: per pass it issues the U float4 of gy and of x back to
// back (rows at or past n4 are not loaded), uses them in row order and stores U results; the first pass's loads are issued before
// the ~20 coefficient loads, so that round trip runs under the stream and not in front of it.  U = 1 on the former grid (two rows
// per lane, a workgroup of three serial round trips) is dgmr_debug_flags 8192: the tests' reference, and the A/B.  U = 2 is the
// default (61 VGPRs: eight waves per SIMD, resident beside a weight-gradient workgroup; DESIGN.md 7d: the step prefers it to 4 and 8).
template <int U, bool TRAIN>
__global__ __launch_bounds__(256) void bn_bwd_apply4_kernel(const f32x4* __restrict__ gy, const f32x4* __restrict__ x,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const double* __restrict__ sums,
                                                             const f32x4* __restrict__ dx_add, f32x4* __restrict__ dx,
                                                             int64_t n4, int C, float invR) {
    const int g = blockIdx.y;
    const int C4 = C >> 2;
    // a pass covers U * stride float4 from the uniform index p on; inside it a lane's rows sit at i0 + u * stride < 8 * 2^24 (the host
    // keeps gridDim.x <= 65536), so their byte offsets fit 32 bits and serve gy, x, dx_add and dx alike on a uniform 64-bit base
    const uint32_t i0 = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    const size_t base = (size_t)g * n4;
    // (the pass's base goes through readfirstlane: it stays one scalar pair per operand, with the lane's 32-bit offset beside it, where
    //  the loop optimiser otherwise keeps a 64-bit vector pointer per operand and row - 32 more registers at U = 4)
    const auto at = [](const f32x4* q, uint32_t bytes) {
        const uint64_t v = (uint64_t)q;
        // (the builtin returns int: both halves go through uint32_t, or a low half >= 2^31 sign-extends over the high one)
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
        return (gf32x4*)((((uint64_t)hi << 32) | lo) + bytes);
    };
    const bool has_add = dx_add != nullptr;
    const int64_t pass = (int64_t)U * stride;
    const int c = (int)(i0 % C4) * 4;
    f32x4 mn, rs, k0, k1, gr;
    // one pass from the uniform index p on.  FULL: every row of it lies below n4 for every lane (a uniform condition) - no predicates;
    // FIRST: the coefficient loads go between the pass's loads and their first use.  The rows live inside the pass: nothing is
    // carried from one to the next.
    const auto run = [&](int64_t p, auto full, auto first) {
        const uint32_t rem = (uint32_t)min(n4 - p, (int64_t)1 << 28);
        f32x4 gv[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (decltype(full)::value || i0 + u * stride < rem) {
                gv[u] = __builtin_nontemporal_load(at(gy + base + p, (i0 + u * stride) * 16u));
                if constexpr (TRAIN) xv[u] = __builtin_nontemporal_load(at(x + base + p, (i0 + u * stride) * 16u));
            }
        if constexpr (decltype(first)::value) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t gc = (size_t)g * C + c + j;
                rs[j] = rstd[gc];
                if constexpr (TRAIN) {
                    mn[j] = mean[gc];
                    k0[j] = (float)sums[((size_t)g * 2 + 0) * C + c + j];
                    k1[j] = (float)sums[((size_t)g * 2 + 1) * C + c + j];
                }
                gr[j] = (gamma ? gamma[c + j] : 1.f) * rs[j];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (decltype(full)::value || i0 + u * stride < rem) {
                const uint32_t bytes = (i0 + u * stride) * 16u;
                *at(dx + base + p, bytes) =
                    bn_bwd_apply_quad<TRAIN>(gv[u], xv[u], mn, rs, k0, k1, gr, invR, has_add, at(dx_add + base + p, bytes));
            }
    };
    const std::true_type yes;
    const std::false_type no;
    if (pass > n4) {  // less than one pass in all
        run(0, no, yes);
        return;
    }
    run(0, yes, yes);
    int64_t p = pass;
    for (; p + pass <= n4; p += pass) run(p, yes, no);
    if (p < n4) run(p, no, no);  // the ragged last pass
}

// one thread per channel walks the G groups in order; UNR groups' 2 UNR doubles are loaded ahead of their additions
template <int UNR>
__global__ void bn_param_grad_kernel(const double* __restrict__ sums, float* __restrict__ dgamma, float* __restrict__ dbeta, int G,
                                     int C) {
    GRID_STRIDE(c, C) {
        double s0 = 0.0, s1 = 0.0;
        int g = 0;
        if constexpr (UNR > 1)
            for (; g + UNR <= G; g += UNR) {
                double v0[UNR], v1[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    v0[u] = sums[((size_t)(g + u) * 2 + 0) * C + c];
                    v1[u] = sums[((size_t)(g + u) * 2 + 1) * C + c];
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    s0 += v0[u];
                    s1 += v1[u];
                }
            }
        for (; g < G; ++g) {
            s0 += sums[((size_t)g * 2 + 0) * C + c];
            s1 += sums[((size_t)g * 2 + 1) * C + c];
        }
        if (dbeta) dbeta[c] += (float)s0;
        if (dgamma) dgamma[c] += (float)s1;
    }
}

__global__ void affine_kernel(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b,
                              float* __restrict__ y, int64_t R, int C, int relu) {
    const int g = blockIdx.y;
    const int64_t n = R * C;
    GRID_STRIDE(i, n) {
        const int c = i % C;
        float v = fmaf(x[(size_t)g * n + i], a[(size_t)g * C + c], b[(size_t)g * C + c]);
        if (relu) v = fmaxf(v, 0.f);
        y[(size_t)g * n + i] = v;
    }
}

}  // namespace

// bn_param_grad_kernel for the units that hold BatchNorm backward sums of their own (head.hip); launch errors are the caller's to check
// dgmr_debug_flags 8192 (conv.hip sets it): the stream passes as they were - one row in flight per lane on the former grids (the
// tests' reference and the A/B; the same bits either way)
int g_bn_one_row = 0;
static inline bool one_row_in_flight() { return g_bn_one_row != 0; }
#define LAUNCH_UNR(kernel, grid, block, s, ...)                                             \
    do {                                                                                    \
        if (one_row_in_flight()) hipLaunchKernelGGL(kernel<1>, grid, block, 0, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<RED_UNR>, grid, block, 0, s, __VA_ARGS__);            \
    } while (0)

// DGMR_BN_ROWS = 2 / 4 / 8: rows a lane of bn_bwd_apply4_kernel keeps in flight (A/B; the same bits for every value)
static const int g_bn_rows = []() {
    const char* e = getenv("DGMR_BN_ROWS");
    const int u = e ? atoi(e) : 0;
    return (u == 2 || u == 4 || u == 8) ? u : 2;
}();
constexpr int BN_APPLY_WGS = 256 * 8;  // workgroups per launch of the multi-pass grid: 8 per CU

void launch_bn_param_grad(const double* sums, float* dgamma, float* dbeta, int G, int C, hipStream_t s) {
    LAUNCH_UNR(bn_param_grad_kernel, dim3((C + 255) / 256), dim3(256), s, sums, dgamma, dbeta, G, C);
}

static inline dim3 reduce_grid(int G, int64_t R) {
    int64_t bx = (R + 63) / 64;
    if (bx > 512) bx = 512;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)G);
}

// deterministic mode: row blocks of a [G][R][C] reduction = reduce_grid's, capped so that the (1 + nb) G 2 C doubles of the caller's buffer
// stay below 32 MB
static inline int det_blocks(int G, int64_t R, int C) {
    const int64_t n = (int64_t)G * 2 * C;
    const int64_t cap = std::max<int64_t>(1, (32ll << 20) / (n * 8));
    return (int)std::min<int64_t>(reduce_grid(G, R).x, cap);
}
extern "C" int64_t dgmr_reduce_doubles(int G, int64_t R, int C) {
    const int64_t n = (int64_t)std::max(G, 1) * 2 * C;
    return g_deterministic ? (1 + (int64_t)det_blocks(std::max(G, 1), R, C)) * n : n;
}
static inline dim3 reduce_grid_mode(int G, int64_t R, int C) {
    return g_deterministic ? dim3((unsigned)det_blocks(G, R, C), (unsigned)G) : reduce_grid(G, R);
}
static inline void reduce_finish(double* sums, int G, int64_t R, int C, hipStream_t s) {
    if (!g_deterministic) return;
    const int64_t n = (int64_t)G * 2 * C;
    LAUNCH_UNR(reduce_rows_finish_kernel, dim3(ew_blocks(n)), dim3(EW_THREADS), s, sums, det_blocks(G, R, C), n);
}

extern "C" int dgmr_bn_stats(const float* x, double* sums, int G, int64_t R, int C, void* stream) {
    DGMR_CHECK_ARG(x && sums && G > 0 && R > 0 && C > 0, "dgmr_bn_stats: bad args");
    LAUNCH_UNR(bn_stats_kernel, reduce_grid_mode(G, R, C), dim3(256), ST, x, sums, R, C, g_deterministic);
    reduce_finish(sums, G, R, C, ST);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_bn_partial_reduce(const float* partials, double* sums, int G, int64_t rows_per_group, int C, void* stream) {
    DGMR_CHECK_ARG(partials && sums && G > 0 && rows_per_group > 0 && C > 0, "dgmr_bn_partial_reduce: bad args");
    const int C2 = 2 * C;
    if (g_deterministic) {
        hipLaunchKernelGGL(bn_partial_reduce_det_kernel, dim3((C2 + 31) / 32, G), dim3(256), 0, ST, partials, sums, rows_per_group, C2);
        DGMR_CHECK_LAUNCH();
        return 0;
    }
    int zs = (int)std::min<int64_t>(64, (rows_per_group + 31) / 32);  // >= 32 rows per slice
    hipLaunchKernelGGL(bn_partial_reduce_kernel, dim3((C2 + 255) / 256, G, zs), dim3(256), 0, ST, partials, sums, rows_per_group, C2);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_bn_bwd_center(double* sums, const float* mean, const float* rstd, int G, int C, void* stream) {
    DGMR_CHECK_ARG(sums && mean && rstd && G > 0 && C > 0, "dgmr_bn_bwd_center: bad args");
    hipLaunchKernelGGL(bn_bwd_center_kernel, dim3(ew_blocks((int64_t)G * C)), dim3(EW_THREADS), 0, ST, sums, mean, rstd, G * C, C);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_bn_finalize(const double* sums, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                int64_t* num_batches_tracked, float* a, float* b, float* save_mean, float* save_rstd, int G,
                                int64_t R, int C, float eps, float momentum, const int32_t* order, void* stream) {
    DGMR_CHECK_ARG(running_mean && running_var && a && b, "dgmr_bn_finalize: null pointer");
    DGMR_CHECK_ARG(sums || G == 1, "dgmr_bn_finalize: eval mode needs G == 1");
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + BNF_C - 1) / BNF_C), dim3(BNF_C * BNF_L), 0, ST, sums, gamma, beta, running_mean, running_var,
                       num_batches_tracked, a, b, save_mean, save_rstd, G, R, C, eps, momentum, order);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_bn_bwd_reduce(const float* gy, const float* x, const float* mean, const float* rstd, double* sums, int G,
                                  int64_t R, int C, void* stream) {
    DGMR_CHECK_ARG(gy && x && mean && rstd && sums, "dgmr_bn_bwd_reduce: null pointer");
    LAUNCH_UNR(bn_bwd_reduce_kernel, reduce_grid_mode(G, R, C), dim3(256), ST, gy, x, mean, rstd, sums, R, C, g_deterministic);
    reduce_finish(sums, G, R, C, ST);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_bn_bwd_apply(const float* gy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                 const double* sums, const float* dx_add, float* dx, float* dgamma, float* dbeta, int G,
                                 int64_t R, int C, int train, void* stream) {
    DGMR_CHECK_ARG(gy && x && mean && rstd && sums && dx, "dgmr_bn_bwd_apply: null pointer");
    const int64_t n4 = R * C / 4;
    if (C % 4 == 0 && C / 4 <= 4096 && al16(gy) && al16(x) && al16(dx) && al16(dx_add)) {
        // blocks: a multiple of m = (C/4) / gcd(C/4, 256) so that blocks * 256 is a multiple of C/4
        const int C4 = C / 4;
        int a = C4, b = 256;
        while (b) { const int t = a % b; a = b; b = t; }
        const int m = C4 / a;
        const int U = one_row_in_flight() ? 1 : g_bn_rows;
        int64_t blocks;
        if (U == 1) {  // the former launch: ~2 float4 per thread per operand
            blocks = (n4 + 2 * 256 - 1) / (2 * 256);
            blocks = std::min<int64_t>(std::max<int64_t>((blocks + m - 1) / m * m, m), (int64_t)(65536 / m) * m);
        } else {  // one pass of U rows per lane where that covers the tensor, else BN_APPLY_WGS workgroups over grid.x * G and several passes
            blocks = (n4 + (int64_t)U * 256 - 1) / ((int64_t)U * 256);
            blocks = std::max<int64_t>((blocks + m - 1) / m * m, m);
            blocks = std::min<int64_t>(blocks, std::max<int64_t>(BN_APPLY_WGS / G / m * m, m));
        }
        const dim3 grid((unsigned)blocks, G);
#define BN_APPLY4(U_, T_)                                                                                                            \
    hipLaunchKernelGGL((bn_bwd_apply4_kernel<U_, T_>), grid, dim3(256), 0, ST, (const f32x4*)gy, (const f32x4*)x, mean, rstd, gamma, \
                       sums, (const f32x4*)dx_add, (f32x4*)dx, n4, C, 1.f / (float)R)
#define BN_APPLY4_U(U_)            \
    do {                           \
        if (train) BN_APPLY4(U_, true); \
        else BN_APPLY4(U_, false); \
    } while (0)
        switch (U) {
            case 1: BN_APPLY4_U(1); break;
            case 2: BN_APPLY4_U(2); break;
            case 4: BN_APPLY4_U(4); break;
            default: BN_APPLY4_U(8); break;
        }
#undef BN_APPLY4_U
#undef BN_APPLY4
    } else {
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_blocks(R * C), G), dim3(EW_THREADS), 0, ST, gy, x, mean, rstd, gamma, sums,
                           dx_add, dx, R, C, train);
    }
    if (dgamma || dbeta) launch_bn_param_grad(sums, dgamma, dbeta, G, C, ST);
    DGMR_CHECK_LAUNCH();
    return 0;
}

// few rows, many columns: dgmr_colsum runs parallel over columns, no atomics, and leaves `tmp` alone
static inline bool colsum_by_columns(int64_t R, int C) { return R <= 4096 && C >= 4096 && C % 4 == 0; }

extern "C" int64_t dgmr_colsum_tmp_doubles(int64_t R, int C) { return colsum_by_columns(R, C) ? 2 : dgmr_reduce_doubles(1, R, C); }

extern "C" int dgmr_colsum(const float* x, float* out, double* tmp, int64_t R, int C, int accumulate, void* stream) {
    DGMR_CHECK_ARG(x && out && tmp, "dgmr_colsum: null pointer");
    if (colsum_by_columns(R, C)) {
        hipLaunchKernelGGL(sum_rows_kernel, dim3(ew_blocks(C / 4)), dim3(EW_THREADS), 0, ST, (const f32x4*)x, (f32x4*)out, (int)R,
                           (int64_t)(C / 4), accumulate);
        DGMR_CHECK_LAUNCH();
        return 0;
    }
    (void)hipMemsetAsync(tmp, 0, sizeof(double) * 2 * C, ST);  // (deterministic mode: tmp holds dgmr_reduce_doubles(1, R, C) doubles)
    LAUNCH_UNR(colsum_kernel, reduce_grid_mode(1, R, C), dim3(256), ST, x, tmp, R, C, g_deterministic);
    reduce_finish(tmp, 1, R, C, ST);
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, ST, tmp, out, C, accumulate);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_group_rowsum(const float* x, const float* w, float* out, int groups, int rows, int64_t n, int rows_per_w,
                                 int w_stride, void* stream) {
    if (w_stride < 1) w_stride = 1;
    DGMR_CHECK_ARG(x && out && groups >= 1 && rows >= 1 && n > 0 && n % 4 == 0 && rows_per_w >= 1 && (n / 4) % w_stride == 0,
                   "dgmr_group_rowsum: groups=%d rows=%d n=%lld (multiple of 4) rows_per_w=%d w_stride=%d", groups, rows, (long long)n,
                   rows_per_w, w_stride);
    hipLaunchKernelGGL(group_rowsum_kernel, dim3(ew_blocks(n / 4), groups), dim3(EW_THREADS), 0, ST, (const f32x4*)x, w, (f32x4*)out,
                       rows, (int64_t)(n / 4), rows_per_w, w_stride);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_repeat_interleave(const float* src, float* dst, int64_t nblocks, int64_t block, int repeat, void* stream) {
    DGMR_CHECK_ARG(src && dst && nblocks > 0 && block > 0 && block % 4 == 0 && repeat >= 1,
                   "dgmr_repeat_interleave: nblocks=%lld block=%lld (multiple of 4) repeat=%d", (long long)nblocks, (long long)block, repeat);
    const int64_t total4 = nblocks * repeat * (block / 4);
    hipLaunchKernelGGL(repeat_interleave_kernel, dim3(ew_blocks(total4)), dim3(EW_THREADS), 0, ST, (const f32x4*)src, (f32x4*)dst,
                       (int64_t)(block / 4), repeat, total4);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_repeat_rows(const float* src, float* dst, int64_t n, int repeat, void* stream) {
    DGMR_CHECK_ARG(src && dst && n > 0 && n % 4 == 0 && repeat >= 1, "dgmr_repeat_rows: n=%lld (multiple of 4) repeat=%d", (long long)n,
                   repeat);
    hipLaunchKernelGGL(repeat_rows_kernel, dim3(ew_blocks(n / 4 * repeat)), dim3(EW_THREADS), 0, ST, (const f32x4*)src, (f32x4*)dst,
                       (int64_t)(n / 4), (int64_t)(n / 4) * repeat);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_affine(const float* x, const float* a, const float* b, float* y, int G, int64_t R, int C, int relu,
                           void* stream) {
    DGMR_CHECK_ARG(x && a && b && y, "dgmr_affine: null pointer");
    hipLaunchKernelGGL(affine_kernel, dim3(ew_blocks(R * C), G), dim3(EW_THREADS), 0, ST, x, a, b, y, R, C, relu);
    DGMR_CHECK_LAUNCH();
    return 0;
}
