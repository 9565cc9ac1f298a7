// Radially binned spectra of L x L windows on the transforms of fft_lds.h: the radially averaged power spectral density of the
// verification plots (spectra.py: dgmr_radial_psd) and, on the windows and bins of the stochastic ensemble's recursion
// (spectral_ar.hip), the radially binned cross-spectrum of two planes that the estimate of its rho(r) pools (stochastic.py:
// dgmr_lag_spectra; its section below says how).
//
// PSD.  The twiddle table is written by psd_twiddle_kernel to the head of the workspace; every kernel copies it to LDS.  The Nyquist
// column kx = L / 2 is never formed: its radius is >= L / 2 and such modes are dropped.  The column transforms then run over L / 2
// columns of L complex numbers.
//   L <= 128: psd_window_kernel, one workgroup per window, the half spectrum [L][L / 2 + 1] complex (66 KB at L = 128) stays in LDS.
//   L >= 256: psd_rows_kernel (32 rows per workgroup) writes the half spectrum transposed, [kx][y], to the workspace; psd_cols_kernel
//             (32 / 16 columns per workgroup at L = 256 / 512) transforms the columns and bins them in its epilogue; psd_finalize_kernel
//             adds the workgroups' bin partials of a window in index order.  Three launches on the stream per round of windows.
// Binning: the modes of bin r in column kx are the contiguous range of |ky| with r (r - 1) < kx^2 + ky^2 <= r (r + 1), found in
// integers.  Thread (r, j) adds the columns kx = j (mod P) of bin r in ascending kx and |ky| (+ky before -ky), |F|^2 formed in fp32
// and added in float64 with the Hermitian weight (2 for kx > 0, 1 for kx = 0); the P partials of a bin are added in j order.  No
// floating-point atomics: two calls give the same bits, whatever the workspace size.
#include "fft_lds.h"

namespace {

constexpr int64_t PSD_TABLE_BYTES = PSD_TW * 8;   // the head of the workspace
constexpr int64_t PSD_WS_CAP = 64ll << 20;        // dgmr_radial_psd_workspace never asks for more than this (or one window, if larger)
constexpr int PSD_ROWS = 32;                      // rows per workgroup of the two-pass row kernel

constexpr int psd_cols(int L) { return L == 256 ? 32 : 16; }  // columns per workgroup of the two-pass column kernel

__global__ __launch_bounds__(PSD_TW) void psd_twiddle_kernel(float2* __restrict__ tw) {
    const int k = threadIdx.x;
    double s, c;
    sincospi(-(double)k / 256.0, &s, &c);  // -2 pi k / 512
    tw[k] = make_float2((float)c, (float)s);
}

// Bin the columns kx0 ... kx0 + ncols - 1 held in LDS; addr(c, y) is the element of column kx0 + c and frequency ky = y (mod L).
// out[r] = sum of weight * |F|^2 over the modes of bin r in these columns, r < L / 2.  s_part: NT doubles.
template <int L, int NT, class Addr>
__device__ __forceinline__ void bin_modes(const float2* __restrict__ s, double* __restrict__ s_part, int kx0, int ncols, int tid,
                                          Addr addr, double* __restrict__ out) {
    constexpr int NB = L / 2, P = NT / NB;
    const int r = tid % NB, j = tid / NB;
    const int hi_all = r * (r + 1), lo_all = r == 0 ? -1 : r * (r - 1);
    double acc = 0.0;
    for (int c = j; c < ncols; c += P) {
        const int kx = kx0 + c;
        const int hi = hi_all - kx * kx, lo = lo_all - kx * kx;
        if (hi < 0) continue;
        const int kmax = isqrt_floor(hi);  // <= L / 2 - 1: r (r + 1) < (L / 2)^2
        const int kmin = lo < 0 ? 0 : isqrt_floor(lo) + 1;
        double col = 0.0;
        for (int ky = kmin; ky <= kmax; ++ky) {
            const float2 v = s[addr(c, ky)];
            col += (double)(v.x * v.x + v.y * v.y);
            if (ky > 0) {
                const float2 u = s[addr(c, L - ky)];
                col += (double)(u.x * u.x + u.y * u.y);
            }
        }
        acc += kx > 0 ? 2.0 * col : col;
    }
    s_part[j * NB + r] = acc;
    __syncthreads();
    if (tid < NB) {
        double v = s_part[tid];
#pragma unroll
        for (int jj = 1; jj < P; ++jj) v += s_part[jj * NB + tid];
        out[tid] = v;
    }
}

struct PsdGeom {
    const float* x;
    int64_t plane_stride;
    int W, wins_y, wins_x;
};

// window `id` (row-major over [N][wins_y][wins_x]) -> its first element
__device__ __forceinline__ const float* window_origin(const PsdGeom& g, int64_t id, int L) {
    const int per_plane = g.wins_y * g.wins_x;
    const int64_t n = id / per_plane;
    const int w = (int)(id - n * per_plane);
    const int wy = w / g.wins_x, wx = w - wy * g.wins_x;
    return g.x + n * g.plane_stride + (int64_t)wy * L * g.W + wx * L;
}

template <int L>
constexpr int psd_window_lds() { return L * (L / 2 + 1) * 8 + PSD_TW * 8 + psd_threads(L) * 8; }

template <int L>
__global__ __launch_bounds__(psd_threads(L)) void psd_window_kernel(PsdGeom g, const float2* __restrict__ tw_g, double* __restrict__ power,
                                                                   long long* __restrict__ missing) {
    constexpr int NT = psd_threads(L), NH = L / 2, RS = NH + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;            // [L][RS]
    float2* tw = s + L * RS;                  // [PSD_TW]
    double* s_part = (double*)(tw + PSD_TW);  // [NT]
    __shared__ int s_miss;
    const int tid = threadIdx.x;
    const int64_t id = blockIdx.x;
    for (int i = tid; i < PSD_TW; i += NT) tw[i] = tw_g[i];
    if (tid == 0) s_miss = 0;
    __syncthreads();
    const int miss = load_rows<L, L, RS, NT>(s, window_origin(g, id, L), g.W, tid);
    if (miss) atomicAdd(&s_miss, miss);
    __syncthreads();
    fft_dif<NH, L, 1, RS, NT>(s, tw, tid);
    real_split<L, L, RS, NT, false>(s, tw, tid);
    fft_dif<L, NH, RS, 1, NT>(s, tw, tid);
    bin_modes<L, NT>(s, s_part, 0, NH, tid,
                     [](int c, int y) { return brev<ilog2(L)>(y) * RS + brev<ilog2(NH)>(c); }, power + id * NH);
    if (tid == 0) missing[id] = s_miss;
}

template <int L>
constexpr int psd_rows_lds() { return PSD_ROWS * (L / 2 + 1) * 8 + PSD_TW * 8; }

// spec: [windows of this round][L / 2][L] complex, the half spectrum after the row pass, transposed
template <int L>
__global__ __launch_bounds__(512) void psd_rows_kernel(PsdGeom g, int64_t win0, const float2* __restrict__ tw_g, float2* __restrict__ spec,
                                                       unsigned long long* __restrict__ missing) {
    constexpr int NT = 512, NF = PSD_ROWS, NH = L / 2, RS = NH + 1, RB = L / NF;
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;  // [NF][RS]
    float2* tw = s + NF * RS;
    __shared__ int s_miss;
    const int tid = threadIdx.x;
    const int64_t gw = blockIdx.x / RB;
    const int y0 = (int)(blockIdx.x - gw * RB) * NF;
    for (int i = tid; i < PSD_TW; i += NT) tw[i] = tw_g[i];
    if (tid == 0) s_miss = 0;
    __syncthreads();
    const int miss = load_rows<L, NF, RS, NT>(s, window_origin(g, win0 + gw, L) + (int64_t)y0 * g.W, g.W, tid);
    if (miss) atomicAdd(&s_miss, miss);
    __syncthreads();
    fft_dif<NH, NF, 1, RS, NT>(s, tw, tid);
    real_split<L, NF, RS, NT, false>(s, tw, tid);
    float2* dst = spec + gw * NH * L + y0;
    for (int t = tid; t < NF * NH; t += NT) {
        const int f = t % NF, kx = t / NF;
        dst[(int64_t)kx * L + f] = s[f * RS + brev<ilog2(NH)>(kx)];
    }
    if (tid == 0 && s_miss) atomicAdd(&missing[win0 + gw], (unsigned long long)s_miss);
}

template <int L>
constexpr int psd_cols_lds() { return psd_cols(L) * (L + 1) * 8 + PSD_TW * 8 + 512 * 8; }

// part: [windows of this round][chunks of C columns][L / 2] float64 bin sums
template <int L>
__global__ __launch_bounds__(512) void psd_cols_kernel(const float2* __restrict__ spec, const float2* __restrict__ tw_g,
                                                       double* __restrict__ part) {
    constexpr int NT = 512, C = psd_cols(L), NH = L / 2, NCH = NH / C, RS = L + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;  // [C][RS]
    float2* tw = s + C * RS;
    double* s_part = (double*)(tw + PSD_TW);
    const int tid = threadIdx.x;
    const int64_t gw = blockIdx.x / NCH;
    const int kx0 = (int)(blockIdx.x - gw * NCH) * C;
    for (int i = tid; i < PSD_TW; i += NT) tw[i] = tw_g[i];
    const float2* src = spec + (gw * NH + kx0) * L;  // C columns of L complex numbers, one after the other
    for (int t = tid; t < C * NH; t += NT) {
        const int q = t % NH, c = t / NH;
        const f32x4 v = *(const f32x4*)(src + (int64_t)c * L + 2 * q);
        float2* d = s + c * RS + 2 * q;
        d[0] = make_float2(v.x, v.y);
        d[1] = make_float2(v.z, v.w);
    }
    __syncthreads();
    fft_dif<L, C, 1, RS, NT>(s, tw, tid);
    bin_modes<L, NT>(s, s_part, kx0, C, tid, [](int c, int y) { return c * RS + brev<ilog2(L)>(y); },
                     part + (int64_t)blockIdx.x * NH);
}

// power[win0 + g][r] = the chunks' partials in index order
__global__ __launch_bounds__(256) void psd_finalize_kernel(const double* __restrict__ part, int64_t items, int NB, int NCH, int64_t win0,
                                                           double* __restrict__ power) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= items) return;
    const int64_t gw = i / NB;
    const int r = (int)(i - gw * NB);
    const double* p = part + gw * NCH * NB + r;
    double v = p[0];
    for (int c = 1; c < NCH; ++c) v += p[(int64_t)c * NB];
    power[(win0 + gw) * NB + r] = v;
}

bool psd_size_ok(int L) { return L == 32 || L == 64 || L == 128 || L == 256 || L == 512; }

// bytes of workspace one window of the two-pass path takes in a round: the transposed half spectrum and the chunks' bin partials
int64_t psd_window_bytes(int L) {
    if (L < 256) return 0;
    return (int64_t)(L / 2) * L * 8 + (int64_t)((L / 2) / psd_cols(L)) * (L / 2) * 8;
}

int psd_check_shape(const char* fn, int64_t N, int H, int W, int L) {
    DGMR_CHECK_ARG(psd_size_ok(L), "%s: window L=%d is not one of 32, 64, 128, 256, 512", fn, L);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % L == 0 && W % L == 0, "%s: H=%d and W=%d must be positive multiples of the window L=%d", fn, H, W, L);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(N * (H / L) * (W / L) <= (1 << 30), "%s: %lld windows are out of range", fn, (long long)(N * (H / L) * (W / L)));
    return 0;
}

template <int L>
int psd_run_window(const PsdGeom& g, int64_t nwin, const float2* tw, double* power, int64_t* missing, hipStream_t st) {
    if (allow_lds(psd_window_kernel<L>, psd_window_lds<L>(), "dgmr_radial_psd") != 0) return -2;
    hipLaunchKernelGGL(psd_window_kernel<L>, dim3((unsigned)nwin), dim3(psd_threads(L)), psd_window_lds<L>(), st, g, tw, power,
                       (long long*)missing);
    return 0;
}

template <int L>
int psd_run_two_pass(const PsdGeom& g, int64_t nwin, int64_t per_round, const float2* tw, float2* spec, double* part, double* power,
                     int64_t* missing, hipStream_t st) {
    constexpr int NH = L / 2, NCH = NH / psd_cols(L), RB = L / PSD_ROWS;
    if (allow_lds(psd_rows_kernel<L>, psd_rows_lds<L>(), "dgmr_radial_psd") != 0 ||
        allow_lds(psd_cols_kernel<L>, psd_cols_lds<L>(), "dgmr_radial_psd") != 0)
        return -2;
    if (hipMemsetAsync(missing, 0, (size_t)nwin * sizeof(int64_t), st) != hipSuccess) {
        dgmr_set_error("dgmr_radial_psd: clearing the missing counts failed: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
    for (int64_t win0 = 0; win0 < nwin; win0 += per_round) {
        const int64_t G = std::min(per_round, nwin - win0);  // G * RB <= 2^30 * 16 / ... : per_round is capped by the caller
        hipLaunchKernelGGL(psd_rows_kernel<L>, dim3((unsigned)(G * RB)), dim3(512), psd_rows_lds<L>(), st, g, win0, tw, spec,
                           (unsigned long long*)missing);
        hipLaunchKernelGGL(psd_cols_kernel<L>, dim3((unsigned)(G * NCH)), dim3(512), psd_cols_lds<L>(), st, (const float2*)spec, tw, part);
        hipLaunchKernelGGL(psd_finalize_kernel, dim3(cdiv(G * NH, 256)), dim3(256), 0, st, (const double*)part, G * NH, NH, NCH, win0, power);
    }
    return 0;
}

// ---- lag spectra (stochastic.py: lag_spectra, estimate_rho) ----------------------------------------------------------------------------
// One workgroup per (plane, window), the four window classes of the recursion in one launch.  The `b` patch is transformed first and
// its half spectrum kept in registers (window_state(L) elements per thread, as spectral_ar_kernel holds X), the `a` patch is transformed
// in the same LDS buffer by the SAME code (one loop body, not unrolled: equal inputs give equal bits).  Every owned element is then
// overwritten by its fp32 terms - (|A|^2, |B|^2) for a first walk over the bins, Re(A conj B) for a second - and the walk is
// bin_modes' extended to r < L and to the Nyquist column: thread (r, j) adds the columns kx = j (mod 4) of bin r in ascending kx
// and |ky| (+ky before -ky; ky = -L / 2 once), in float64 with the Hermitian weight (2 for 0 < kx < L / 2, 1 for kx = 0 and L / 2);
// the four partials of a bin are added in j order through the transform buffer.  No atomics, no workspace.
struct LagGeom {
    const float* a;
    const float* b;
    double* sums;
    int64_t a_plane_stride, b_plane_stride;
    int H, W, wins_per_plane, wide;
};

template <int L>
constexpr int lag_lds() { return L * (L / 2 + 1) * 8 + PSD_TW * 8; }  // 3 * 4 * L doubles of partials fit into the transform buffer

// acc0, acc1: this thread's sums of the two components of s over the modes of bin tid % L in the columns kx = tid / L (mod 4)
template <int L>
__device__ __forceinline__ void lag_walk(const float2* __restrict__ s, int tid, double& acc0, double& acc1) {
    constexpr int NH = L / 2, RS = NH + 1, P = psd_threads(L) / L;
    const int r = tid % L, j = tid / L;
    const int hi_all = r * (r + 1), lo_all = r == 0 ? -1 : r * (r - 1);
    acc0 = 0.0, acc1 = 0.0;
    for (int kx = j; kx <= NH; kx += P) {
        const int hi = hi_all - kx * kx, lo = lo_all - kx * kx;
        if (hi < 0) break;  // (kx only grows)
        const int kmax = min(isqrt_floor(hi), NH);
        const int kmin = lo < 0 ? 0 : isqrt_floor(lo) + 1;
        const int col = kx < NH ? brev<ilog2(NH)>(kx) : NH;
        double c0 = 0.0, c1 = 0.0;
        for (int ky = kmin; ky <= kmax; ++ky) {
            if (ky < NH) {
                const float2 v = s[brev<ilog2(L)>(ky) * RS + col];
                c0 += (double)v.x, c1 += (double)v.y;
            }
            if (ky > 0) {  // -ky, which for ky = L / 2 is the Nyquist row itself
                const float2 u = s[brev<ilog2(L)>(L - ky) * RS + col];
                c0 += (double)u.x, c1 += (double)u.y;
            }
        }
        const bool twice = kx > 0 && kx < NH;
        acc0 += twice ? 2.0 * c0 : c0;
        acc1 += twice ? 2.0 * c1 : c1;
    }
}

template <int L>
__global__ __launch_bounds__(psd_threads(L)) void lag_spectra_kernel(LagGeom g) {
    constexpr int NT = psd_threads(L), TOTAL = L * (L / 2 + 1), NS = window_state(L), P = NT / L;
    static_assert(3 * P * L * 8 <= TOTAL * 8 && 3 * L <= NT, "the partials live in the transform buffer, one thread per (q, r) adds them");
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;  // [L][RS]
    float2* tw = s + TOTAL;         // [PSD_TW]
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x / g.wins_per_plane;
    int wi = (int)(blockIdx.x - n * g.wins_per_plane);
    // the window's class: the classes one after the other, row-major inside a class
    const int ny = g.H / L, nx = g.W / L;
    int cy = 0, cx = 0;
    for (int c = 0; c < 3; ++c) {
        const int count = (ny - cy) * (nx - cx);
        if (wi < count) break;
        wi -= count;
        window_class(c + 1, cy, cx);
    }
    int y0, x0;
    window_corner<L>(wi, nx - cx, cy, cx, y0, x0);  // nx - cx > 0: wi is inside this class
    fill_twiddles<NT>(tw, tid);
    __syncthreads();
    const int64_t origin = (int64_t)y0 * g.W + x0;
    float2 B[NS];
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const float* src = pass == 0 ? g.b + n * g.b_plane_stride : g.a + n * g.a_plane_stride;
        window_forward<L>(s, tw, src + origin, g.W, g.wide, tid);
        if (pass == 0) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const int e = tid + j * NT;
                B[j] = e < TOTAL ? s[e] : make_float2(0.f, 0.f);
            }
            __syncthreads();  // everyone holds its part of B before the buffer is loaded again
        }
    }
    float cross[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        cross[j] = 0.f;
        if (e < TOTAL) {
            const float2 av = s[e], bv = B[j];
            // one expression shape for the three terms: b == a gives three equal values, b == -a gives cross == -|A|^2
            s[e] = make_float2(fmaf(av.x, av.x, av.y * av.y), fmaf(bv.x, bv.x, bv.y * bv.y));
            cross[j] = fmaf(av.x, bv.x, av.y * bv.y);
        }
    }
    __syncthreads();
    double pa, pb, pc, unused;
    lag_walk<L>(s, tid, pa, pb);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        if (e < TOTAL) s[e] = make_float2(cross[j], 0.f);
    }
    __syncthreads();
    lag_walk<L>(s, tid, pc, unused);
    __syncthreads();
    double* part = (double*)psd_smem;  // [3][P][L]
    {
        const int r = tid % L, j = tid / L;
        part[(0 * P + j) * L + r] = pa;
        part[(1 * P + j) * L + r] = pb;
        part[(2 * P + j) * L + r] = pc;
    }
    __syncthreads();
    if (tid < 3 * L) {
        const int q = tid / L, r = tid - q * L;
        double v = part[(q * P) * L + r];
#pragma unroll
        for (int j = 1; j < P; ++j) v += part[(q * P + j) * L + r];
        g.sums[((int64_t)blockIdx.x * 3 + q) * L + r] = v;
    }
}

template <int L>
int lag_run(const LagGeom& g, int64_t blocks, hipStream_t st) {
    if (allow_lds(lag_spectra_kernel<L>, lag_lds<L>(), "dgmr_lag_spectra") != 0) return -2;
    hipLaunchKernelGGL(lag_spectra_kernel<L>, dim3((unsigned)blocks), dim3(psd_threads(L)), lag_lds<L>(), st, g);
    return 0;
}

}  // namespace

extern "C" int64_t dgmr_radial_psd_workspace(int64_t N, int H, int W, int L) {
    if (psd_check_shape("dgmr_radial_psd_workspace", N, H, W, L) != 0) return -1;
    const int64_t per_win = psd_window_bytes(L), nwin = N * (H / L) * (W / L);
    return PSD_TABLE_BYTES + std::min(nwin * per_win, std::max(PSD_WS_CAP - PSD_WS_CAP % std::max<int64_t>(per_win, 1), per_win));
}

extern "C" int dgmr_radial_psd(const float* x, int64_t plane_stride, int64_t N, int H, int W, int L, void* workspace,
                               int64_t workspace_bytes, double* power, int64_t* missing, void* stream) {
    if (psd_check_shape("dgmr_radial_psd", N, H, W, L) != 0) return -1;
    DGMR_CHECK_ARG(x && workspace && power && missing, "dgmr_radial_psd: null pointer");
    DGMR_CHECK_ARG(plane_stride >= (int64_t)H * W && plane_stride % 4 == 0 && plane_stride <= INT64_MAX / 4 / N,
                   "dgmr_radial_psd: plane_stride=%lld must be a multiple of 4 elements and at least H * W = %lld", (long long)plane_stride,
                   (long long)((int64_t)H * W));
    DGMR_CHECK_ARG((((uintptr_t)x | (uintptr_t)workspace) & 15) == 0, "dgmr_radial_psd: x and workspace must be 16-byte aligned");
    DGMR_CHECK_ARG((((uintptr_t)power | (uintptr_t)missing) & 7) == 0, "dgmr_radial_psd: power and missing must be 8-byte aligned");
    const int64_t per_win = psd_window_bytes(L), nwin = N * (H / L) * (W / L);
    DGMR_CHECK_ARG(workspace_bytes >= PSD_TABLE_BYTES + per_win,
                   "dgmr_radial_psd: workspace of %lld bytes, one window needs %lld (dgmr_radial_psd_workspace(1, L, L, L))",
                   (long long)workspace_bytes, (long long)(PSD_TABLE_BYTES + per_win));
    hipStream_t st = ST;
    float2* tw = (float2*)workspace;
    const PsdGeom g{x, plane_stride, W, H / L, W / L};
    hipLaunchKernelGGL(psd_twiddle_kernel, dim3(1), dim3(PSD_TW), 0, st, tw);
    int rc = 0;
    if (L < 256) {
        rc = L == 32 ? psd_run_window<32>(g, nwin, tw, power, missing, st)
             : L == 64 ? psd_run_window<64>(g, nwin, tw, power, missing, st)
                       : psd_run_window<128>(g, nwin, tw, power, missing, st);
    } else {
        // windows per round: what the workspace holds, at most 2^20 (grids stay far below 2^31 workgroups)
        const int64_t per_round = std::min<int64_t>(std::min((workspace_bytes - PSD_TABLE_BYTES) / per_win, nwin), 1 << 20);
        float2* spec = (float2*)((char*)workspace + PSD_TABLE_BYTES);
        double* part = (double*)(spec + per_round * (L / 2) * L);
        rc = L == 256 ? psd_run_two_pass<256>(g, nwin, per_round, tw, spec, part, power, missing, st)
                      : psd_run_two_pass<512>(g, nwin, per_round, tw, spec, part, power, missing, st);
    }
    if (rc != 0) return rc;
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_lag_spectra(const float* a, int64_t a_plane_stride, const float* b, int64_t b_plane_stride, int64_t N, int H, int W, int L,
                                double* sums, void* stream) {
    const char* fn = "dgmr_lag_spectra";
    DGMR_CHECK_ARG(L == 32 || L == 64 || L == 128, "%s: window L=%d is not one of 32, 64, 128", fn, L);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % L == 0 && W % L == 0, "%s: H=%d and W=%d must be positive multiples of the window L=%d", fn, H, W, L);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(a && b && sums, "%s: null pointer", fn);
    DGMR_CHECK_ARG(((uintptr_t)sums & 7) == 0, "%s: sums must be 8-byte aligned", fn);
    const int64_t plane = (int64_t)H * W, cap = INT64_MAX / 4 / N;
    DGMR_CHECK_ARG(a_plane_stride >= plane && a_plane_stride <= cap && b_plane_stride >= plane && b_plane_stride <= cap,
                   "%s: a_plane_stride=%lld and b_plane_stride=%lld must be at least H * W = %lld", fn, (long long)a_plane_stride,
                   (long long)b_plane_stride, (long long)plane);
    const int ny = H / L, nx = W / L;
    const int64_t wins = (int64_t)ny * nx + (int64_t)ny * (nx - 1) + (int64_t)(ny - 1) * nx + (int64_t)(ny - 1) * (nx - 1);
    DGMR_CHECK_ARG(N * wins <= (1 << 30), "%s: %lld windows are out of range", fn, (long long)(N * wins));
    const int wide = (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && a_plane_stride % 4 == 0 && b_plane_stride % 4 == 0;
    const LagGeom g{a, b, sums, a_plane_stride, b_plane_stride, H, W, (int)wins, wide};
    hipStream_t st = ST;
    const int rc = L == 32 ? lag_run<32>(g, N * wins, st) : L == 64 ? lag_run<64>(g, N * wins, st) : lag_run<128>(g, N * wins, st);
    if (rc != 0) return rc;
    DGMR_CHECK_LAUNCH();
    return 0;
}
