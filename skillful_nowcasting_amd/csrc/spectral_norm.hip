// Spectral-norm power iteration for gfx950: one module call (dgmr_spectral_sigma) and every call sequence of a forward in three
// kinds of launch (dgmr_spectral_sigma_seq_multi).  Latency-bound mat-vecs, no MFMA; every sum in a fixed order.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// spectral norm
// ------------------------------------------------------------------------------------------------
// t[i] = sum_k w[i][k] * v[perm(k)].  (Round 5: the norms / dots over t that used to meet in float atomics on `scratch` are recomputed
// by their consumers in a fixed order - the first, traced forward of a module went through these kernels and was the last source of
// run-to-run differences; `scratch` stays in the signatures and is left untouched.)
__global__ void sn_rows_kernel(const float* __restrict__ w, const float* __restrict__ v, float* __restrict__ t, int K, int Cin, int taps) {
    __shared__ float red[32];
    const int i = blockIdx.x;
    const float* wr = w + (size_t)i * K;
    float s = 0.f;
    for (int k = threadIdx.x * 4; k < K; k += blockDim.x * 4) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
        const int tp = k / Cin, ci = k - tp * Cin;
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(wv[j], v[(size_t)(ci + j) * taps + tp], s);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) t[i] = s;
}

// sum_i a[i] * b[i] over n values, the same fixed order in every workgroup that calls it (strided per thread, then block_sum)
__device__ __forceinline__ float sn_dot_fixed(const float* __restrict__ a, const float* __restrict__ b, int n, float* red) {
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) q = fmaf(a[i], b[i], q);
    return block_sum(q, red);
}

// s[k] = sum_i w[i][k] * t[i] / max(||t||, eps); block 0 also writes u = t / max(||t||, eps); scratch[1] += s^2
__global__ void sn_cols_kernel(const float* __restrict__ w, const float* __restrict__ t, float* __restrict__ s_out,
                               float* __restrict__ u, float* __restrict__ u_save, float* __restrict__ scratch, int Cout, int K,
                               float eps) {
    __shared__ float part[4][64];
    __shared__ float red[32];
    const float inv = 1.f / fmaxf(sqrtf(sn_dot_fixed(t, t, Cout, red)), eps);
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + c;
    float s = 0.f;
    if (k < K)
        for (int i = rg; i < Cout; i += 4) s = fmaf(w[(size_t)i * K + k], t[i] * inv, s);
    part[rg][c] = s;
    __syncthreads();
    if (rg == 0 && k < K) s_out[k] = part[0][c] + part[1][c] + part[2][c] + part[3][c];
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < Cout; i += blockDim.x) {
            const float ui = t[i] * inv;
            u[i] = ui;
            if (u_save) u_save[i] = ui;
        }
}

// v[perm(k)] = s[k]/max(||s||,eps); inv_sigma = max(||s||,eps)/||s||^2   (sigma = u^T W v = ||s||^2 / max(||s||, eps))
__global__ void sn_finish_train_kernel(const float* __restrict__ s, float* __restrict__ v, float* __restrict__ v_save,
                                       float* __restrict__ inv_sigma, const float* __restrict__ scratch, int K, int Cin, int taps,
                                       float eps) {
    __shared__ float red[32];
    const float n2 = sn_dot_fixed(s, s, K, red);  // ||s||^2, recomputed by every workgroup in the same order
    const float d = fmaxf(sqrtf(n2), eps);
    const float inv = 1.f / d;
    GRID_STRIDE(k, K) {
        const int tp = k / Cin, ci = k - tp * Cin;
        const float vk = s[k] * inv;
        const size_t j = (size_t)ci * taps + tp;
        v[j] = vk;
        if (v_save) v_save[j] = vk;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) inv_sigma[0] = d / n2;
}

__global__ void sn_finish_eval_kernel(const float* __restrict__ u, const float* __restrict__ v, float* __restrict__ u_save,
                                      float* __restrict__ v_save, float* __restrict__ inv_sigma,
                                      const float* __restrict__ t, int Cout, int K) {
    __shared__ float red[32];
    const float sigma = sn_dot_fixed(u, t, Cout, red);  // u^T W v
    GRID_STRIDE(i, (int64_t)Cout + K) {
        if (i < Cout) {
            if (u_save) u_save[i] = u[i];
        } else if (v_save)
            v_save[i - Cout] = v[i - Cout];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) inv_sigma[0] = 1.f / sigma;
}

// ---- T calls of one spectral-norm module in one go ---------------------------------------------------------
// The reference runs one power iteration per module CALL (parametrizations.py:512-513); a sampler / discriminator
// conv is called once per forecast step / frame, i.e. T dependent iterations on the same W.  With A = W W^T
// ([Cout][Cout], cached per weight version) the chain never touches W again:
//     s_t = W^T u_t,  n_t^2 = u_t^T A u_t,  d_t = max(n_t, eps),  v_t = s_t / d_t,  sigma_t = n_t^2 / d_t,
//     u_{t+1} = W v_t / max(||W v_t||, eps) = (A u_t / d_t) / max(||A u_t|| / d_t, eps)
// so W is read twice per forward (t0 = W v_0 and S = W^T [u_1..u_T]) instead of 2T times.
constexpr int SN_TMAX = 32;

// ---- the same for MANY modules in three launches (all spectral-norm work of one generator / discriminator forward) ----
// Power iterations do not depend on activations, so a forward draws every module's call sequence up front: block -> module
// through the descriptors' block prefix sums; the chains of all modules run concurrently, one workgroup each.
__device__ __forceinline__ int sn_find(const dgmr_sn_desc* __restrict__ d, int n, int blk, bool rows) {
    int m = 0;
    while (m + 1 < n && blk >= (rows ? d[m + 1].row_block0 : d[m + 1].col_block0)) ++m;
    return m;
}

__global__ void sn_rows_multi_kernel(const dgmr_sn_desc* __restrict__ descs, int n, float* __restrict__ arena) {
    __shared__ float red[32];
    const int m = sn_find(descs, n, blockIdx.x, true);
    const dgmr_sn_desc d = descs[m];
    const int i = blockIdx.x - d.row_block0;
    const int K = d.Cin * d.taps;
    const float* wr = d.w + (size_t)i * K;
    float s = 0.f;
    for (int k = threadIdx.x * 4; k < K; k += blockDim.x * 4) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
        const int tp = k / d.Cin, ci = k - tp * d.Cin;
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(wv[j], d.v[(size_t)(ci + j) * d.taps + tp], s);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) arena[d.tmp_off + i] = s;
}

// One power iteration of EVERY module per launch.  The chain u_{t+1} ~ (W W^T) u_t is sequential in t, but one workgroup per module
// (the round-1 design) read a 1536 x 1536 Gram matrix through a single CU at ~30 GB/s: 0.3 ms per iteration, 1.4 ms per
// discriminator forward, all on the step's critical path.  Here launch t computes y_t = A u_t for all modules with 32 rows of A per
// workgroup (hundreds of workgroups, every A from L2 at full rate); the quantities that need the WHOLE vector - ||y||, u^T y - are
// recomputed at the start of launch t+1 by every workgroup of the module from y_{t-1} and u_{t-1} (a few thousand fmas, identical
// in every workgroup: same data, same reduction order), so no cross-workgroup hand-off exists inside a launch and the stream
// order is the only synchronisation.  ~6 us per launch instead of 80 ... 300 us per iteration.
//   t = 0:        u_0 = t0 / max(||t0||, eps)                               (t0 = W v, sn_rows_multi_kernel)
//   0 < t < T:    finish call t-1 (dnorm, 1/sigma) from (u_{t-1}, y_{t-1}); u_t = (y/d) / max(||y||/d, eps)
//   t = T:        finish call T-1; module's u <- u_{T-1}
// tmp region of a module: t0[Cout] | dnorm[T] | y[2][Cout] (double-buffered: launch t still reads y_{t-1} while writing y_t).
constexpr int SN_RB = 32;

__device__ __forceinline__ int sn_find_iter(const dgmr_sn_desc* __restrict__ d, int n, int blk) {
    int m = 0;
    while (m + 1 < n && blk >= d[m + 1].iter_block0) ++m;
    return m;
}

__global__ __launch_bounds__(256) void sn_iter_multi_kernel(const dgmr_sn_desc* __restrict__ descs, int n, float* __restrict__ arena,
                                                            int t) {
    extern __shared__ float sh[];  // u[Cout] | red[64]
    const int m = sn_find_iter(descs, n, blockIdx.x);
    const dgmr_sn_desc d = descs[m];
    const int Cout = d.Cout, T = d.T;
    if (t > T) return;
    const int rb = blockIdx.x - d.iter_block0;
    const float eps = d.eps;
    float* tmp = arena + d.tmp_off;
    const float* t0 = tmp;
    float* dnorm = tmp + Cout;
    float* Y = tmp + Cout + T;
    float* u_hist = arena + d.u_hist_off;
    float* inv_sigma = arena + d.inv_sigma_off;
    float* u = sh;
    float* red = sh + Cout;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (t == 0) {
        float q = 0.f;
        for (int i = threadIdx.x; i < Cout; i += blockDim.x) q = fmaf(t0[i], t0[i], q);
        q = block_sum(q, red);
        const float inv = 1.f / fmaxf(sqrtf(q), eps);
        for (int i = threadIdx.x; i < Cout; i += blockDim.x) u[i] = t0[i] * inv;
    } else {
        const int sp = d.perm ? d.perm[t - 1] : t - 1;
        const float* __restrict__ y = Y + ((t - 1) & 1) * Cout;
        const float* __restrict__ up = u_hist + (size_t)sp * Cout;
        float a = 0.f, b = 0.f;
        for (int i = threadIdx.x; i < Cout; i += blockDim.x) {
            const float yi = y[i];
            a = fmaf(up[i], yi, a);
            b = fmaf(yi, yi, b);
        }
        const float n2 = block_sum(a, red);
        const float y2 = block_sum(b, red + 32);
        const float dd = fmaxf(sqrtf(fmaxf(n2, 0.f)), eps);
        if (rb == 0 && threadIdx.x == 0) {
            dnorm[t - 1] = dd;
            inv_sigma[sp] = dd / n2;
        }
        if (t == T) {
            if (rb == 0)
                for (int i = threadIdx.x; i < Cout; i += blockDim.x) d.u[i] = up[i];
            return;
        }
        const float invd = 1.f / dd;
        const float inv = invd / fmaxf(sqrtf(y2) * invd, eps);
        for (int i = threadIdx.x; i < Cout; i += blockDim.x) u[i] = y[i] * inv;
    }
    __syncthreads();
    const int st = d.perm ? d.perm[t] : t;
    if (rb == 0)
        for (int i = threadIdx.x; i < Cout; i += blockDim.x) u_hist[(size_t)st * Cout + i] = u[i];
    // y_t[rows of this workgroup] = A[rows] . u_t : each wave takes rows r0 + wid, + nw, ...; four rows in flight per wave
    const float* __restrict__ A = d.gram;
    float* yo = Y + (t & 1) * Cout;
    const int r0 = rb * SN_RB, r1 = min(Cout, r0 + SN_RB);
    for (int i0 = r0 + wid; i0 < r1; i0 += 4 * nw) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = lane; j < Cout; j += 64) {
            const float uj = u[j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + r * nw;
                if (i < r1) s[r] = fmaf(A[(size_t)i * Cout + j], uj, s[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + r * nw;
            const float v = wave_sum(s[r]);
            if (lane == 0 && i < r1) yo[i] = v;
        }
    }
}

// (round 6) The row loop walks tiles of 64 rows: the tile's u values of all SN_TMAX calls are staged in LDS once ([row][call], read back
// as broadcast ds_read_b128) and the thread's 16 weights of the tile are fetched up front.  Before, every (row, call) pair cost a flat
// load through 64-bit vector address arithmetic and a branch - ten instructions per multiply-add, 1.0 - 1.2 ms per launch.  The sums are
// formed in the same order (rows rg, rg + 4, ... per call): bit-identical results.
__global__ __launch_bounds__(256) void sn_cols_multi_kernel(const dgmr_sn_desc* __restrict__ descs, int n, float* __restrict__ arena) {
    constexpr int RT = 64, US = SN_TMAX + 4;  // rows per tile; LDS row stride in floats (16-byte aligned rows)
    __shared__ float part[4][SN_TMAX][64];
    __shared__ __attribute__((aligned(16))) float ut[RT * US];
    const int m = sn_find(descs, n, blockIdx.x, false);
    const dgmr_sn_desc d = descs[m];
    const int Cout = d.Cout, T = d.T, K = d.Cin * d.taps;
    const float* __restrict__ u_hist = arena + d.u_hist_off;
    const float* __restrict__ dnorm = arena + d.tmp_off + Cout;
    float* v_hist = arena + d.v_hist_off;
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int k = (blockIdx.x - d.col_block0) * 64 + c;
    const bool kok = k < K;
    // sequences longer than SN_TMAX calls (batched generator draws: draws x forecast steps) go in chunks; W is re-read from L2
    for (int tc = 0; tc < T; tc += SN_TMAX) {
        const int Tc = min(SN_TMAX, T - tc);
        float acc[SN_TMAX];
#pragma unroll
        for (int t = 0; t < SN_TMAX; ++t) acc[t] = 0.f;
        for (int i0 = 0; i0 < Cout; i0 += RT) {
            __syncthreads();  // the previous tile (and the previous chunk's partial sums) have been consumed
            // calls t = rg, rg + 4, ...: 64 consecutive rows per wave and call (calls beyond the chunk read call tc: never used)
#pragma unroll
            for (int j = 0; j < SN_TMAX / 4; ++j) {
                const int t = rg + 4 * j;
                const int sl = t < Tc ? (d.perm ? d.perm[tc + t] : tc + t) : (d.perm ? d.perm[tc] : tc);
                ut[c * US + t] = i0 + c < Cout ? u_hist[(size_t)sl * Cout + i0 + c] : 0.f;
            }
            float wv[RT / 4];
#pragma unroll
            for (int r = 0; r < RT / 4; ++r) {
                const int i = i0 + rg + 4 * r;
                wv[r] = (kok && i < Cout) ? d.w[(size_t)i * K + k] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < RT / 4; ++r) {
                if (i0 + rg + 4 * r >= Cout) break;  // (wave-uniform)
                const float4* up = reinterpret_cast<const float4*>(ut + (rg + 4 * r) * US);
#pragma unroll
                for (int q = 0; q < SN_TMAX / 4; ++q) {
                    const float4 u4 = up[q];
                    acc[4 * q + 0] = fmaf(wv[r], u4.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = fmaf(wv[r], u4.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(wv[r], u4.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(wv[r], u4.w, acc[4 * q + 3]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < SN_TMAX; ++t) part[rg][t][c] = acc[t];
        __syncthreads();
        if (kok) {
            const int tp = k / d.Cin, ci = k - tp * d.Cin;
            const size_t j = (size_t)ci * d.taps + tp;
            for (int t = rg; t < Tc; t += 4) {
                const float sv = (part[0][t][c] + part[1][t][c] + part[2][t][c] + part[3][t][c]) / dnorm[tc + t];
                const int sl = d.perm ? d.perm[tc + t] : tc + t;
                v_hist[(size_t)sl * K + j] = sv;
                if (tc + t == T - 1) d.v[j] = sv;
            }
        }
    }
}

__global__ void zero_kernel(float* p, int n) {
    if (threadIdx.x < n) p[threadIdx.x] = 0.f;
}

}  // namespace

extern "C" int dgmr_spectral_sigma(const float* w, float* u, float* v, float* u_save, float* v_save, float* inv_sigma,
                                   float* scratch, float* tmp, int Cout, int Cin, int taps, float eps, int train, void* stream) {
    DGMR_CHECK_ARG(w && u && v && inv_sigma && scratch && tmp, "dgmr_spectral_sigma: null pointer");
    DGMR_CHECK_ARG(Cin % 4 == 0, "dgmr_spectral_sigma: Cin=%d must be a multiple of 4", Cin);
    const int K = Cin * taps;
    float* t = tmp;
    float* s = tmp + Cout;
    if (train) {
        hipLaunchKernelGGL(sn_rows_kernel, dim3(Cout), dim3(256), 0, ST, w, v, t, K, Cin, taps);
        hipLaunchKernelGGL(sn_cols_kernel, dim3((K + 63) / 64), dim3(256), 0, ST, w, t, s, u, u_save, scratch, Cout, K, eps);
        hipLaunchKernelGGL(sn_finish_train_kernel, dim3(std::min((K + 255) / 256, 64)), dim3(256), 0, ST, s, v, v_save, inv_sigma,
                           scratch, K, Cin, taps, eps);
    } else {
        hipLaunchKernelGGL(sn_rows_kernel, dim3(Cout), dim3(256), 0, ST, w, v, t, K, Cin, taps);
        hipLaunchKernelGGL(sn_finish_eval_kernel, dim3(std::min((Cout + K + 255) / 256, 64)), dim3(256), 0, ST, u, v, u_save, v_save,
                           inv_sigma, t, Cout, K);
    }
    hipLaunchKernelGGL(zero_kernel, dim3(1), dim3(64), 0, ST, scratch, 4);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_spectral_sigma_seq_multi(const dgmr_sn_desc* descs_dev, int n, int total_row_blocks, int total_col_blocks,
                                             int total_iter_blocks, int max_cout, int max_T, float* arena, void* stream) {
    DGMR_CHECK_ARG(descs_dev && arena && n > 0 && total_row_blocks > 0 && total_col_blocks > 0 && total_iter_blocks > 0,
                   "dgmr_spectral_sigma_seq_multi: bad args");
    DGMR_CHECK_ARG(max_cout > 0 && max_cout <= 8192, "dgmr_spectral_sigma_seq_multi: max_cout=%d", max_cout);
    DGMR_CHECK_ARG(max_T >= 1 && max_T <= 4096, "dgmr_spectral_sigma_seq_multi: max_T=%d", max_T);
    hipLaunchKernelGGL(sn_rows_multi_kernel, dim3(total_row_blocks), dim3(256), 0, ST, descs_dev, n, arena);
    for (int t = 0; t <= max_T; ++t)  // launch t: iteration t of every module that has one (t == T: its bookkeeping only)
        hipLaunchKernelGGL(sn_iter_multi_kernel, dim3(total_iter_blocks), dim3(256), (max_cout + 64) * sizeof(float), ST, descs_dev, n,
                           arena, t);
    hipLaunchKernelGGL(sn_cols_multi_kernel, dim3(total_col_blocks), dim3(256), 0, ST, descs_dev, n, arena);
    DGMR_CHECK_LAUNCH();
    return 0;
}
