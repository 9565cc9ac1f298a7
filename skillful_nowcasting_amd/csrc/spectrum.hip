// The two remaining verification plots on the device (spectra.py, value.py): the radially averaged power spectral density of L x L
// windows (dgmr_radial_psd) and the exceedance table that reliability, Brier score, ROC points and economic value are derived from
// (dgmr_exceedance_table).  And, built on the PSD's transforms, the AR(1) noise windows of the stochastic advection ensemble
// (stochastic.py: dgmr_spectral_ar; its section below says how), the same with a second lag (dgmr_spectral_ar2) and, on the same
// windows and bins, the radially binned cross-spectrum of two planes that the estimate of the recursion's rho(r) pools
// (dgmr_lag_spectra; its section too).
//
// PSD.  fp32 radix-2 decimation-in-frequency transforms in LDS (two stages per pass and barrier), twiddles from a table of exp(-2 pi i k / 512) computed in double and
// rounded to fp32 (psd_twiddle_kernel writes it to the head of the workspace; every kernel copies it to LDS).  The input is real, so
// a row of L reals is transformed as L / 2 complex numbers z[m] = x[2m] + i x[2m + 1] - which is how a 16-byte load delivers them - and
// split afterwards:  X[k] = E[k] + W_L^k O[k],  E[k] = (Z[k] + conj Z[L/2 - k]) / 2,  O[k] = (Z[k] - conj Z[L/2 - k]) / 2i,
// for kx = 0 ... L / 2 - 1.  The Nyquist column kx = L / 2 is never formed: its radius is >= L / 2 and such modes are dropped.  The column
// transforms then run over L / 2 columns of L complex numbers.  Nothing is reordered: a DIF transform leaves frequency k at the
// bit-reversed position, and the binning addresses a mode by __brev.
//   L <= 128: psd_window_kernel, one workgroup per window, the half spectrum [L][L / 2 + 1] complex (66 KB at L = 128) stays in LDS.
//   L >= 256: psd_rows_kernel (32 rows per workgroup) writes the half spectrum transposed, [kx][y], to the workspace; psd_cols_kernel
//             (32 / 16 columns per workgroup at L = 256 / 512) transforms the columns and bins them in its epilogue; psd_finalize_kernel
//             adds the workgroups' bin partials of a window in index order.  Three launches on the stream per round of windows.
// LDS layout: in every batch of transforms the lanes of a wave run over the transforms, not over the butterflies of one, and the
// stride between transforms is either one element or an odd number of elements (rows are padded by one complex number), so at every
// butterfly distance the 32 lanes of an LDS lane group fall on 32 different 8-byte bank pairs.
// Binning: the modes of bin r in column kx are the contiguous range of |ky| with r (r - 1) < kx^2 + ky^2 <= r (r + 1), found in
// integers.  Thread (r, j) adds the columns kx = j (mod P) of bin r in ascending kx and |ky| (+ky before -ky), |F|^2 formed in fp32
// and added in float64 with the Hermitian weight (2 for kx > 0, 1 for kx = 0); the P partials of a bin are added in j order.  No
// floating-point atomics: two calls give the same bits, whatever the workspace size.
//
// Exceedance table.  One streaming read (16-byte loads) of the ensemble and the observation; per pixel and threshold the number of
// members that reach the threshold is the row, the observation's own exceedance the column of a per-workgroup histogram in LDS
// (at most 8 x 33 x 2 counters).  A wave adds the key of its first present lane once by ballot - in a radar field that is nearly
// everybody's key - and the other keys lane by lane; the workgroup adds its non-zero counters to the table with integer atomics.
#include "common.h"

namespace {

constexpr int PSD_TW = 256;                       // twiddle table: exp(-2 pi i k / 512), k < 256
constexpr int64_t PSD_TABLE_BYTES = PSD_TW * 8;   // the head of the workspace
constexpr int64_t PSD_WS_CAP = 64ll << 20;        // dgmr_radial_psd_workspace never asks for more than this (or one window, if larger)
constexpr int PSD_ROWS = 32;                      // rows per workgroup of the two-pass row kernel

constexpr int psd_threads(int L) { return L == 32 ? 128 : L == 64 ? 256 : 512; }
constexpr int psd_cols(int L) { return L == 256 ? 32 : 16; }  // columns per workgroup of the two-pass column kernel
constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

__global__ __launch_bounds__(PSD_TW) void psd_twiddle_kernel(float2* __restrict__ tw) {
    const int k = threadIdx.x;
    double s, c;
    sincospi(-(double)k / 256.0, &s, &c);  // -2 pi k / 512
    tw[k] = make_float2((float)c, (float)s);
}

template <int BITS>
__device__ __forceinline__ int brev(int v) { return (int)(__brev((unsigned int)v) >> (32 - BITS)); }

// NF in-place DIF transforms of length N: element e of transform f is s[f * SF + e * SE]; frequency k ends at element brev(k).
// Thread t takes transform t % NF (NF a power of two), so the lanes of a wave differ in f first.  Ends with a barrier.
template <int N, int NF, int SE, int SF, int NT>
__device__ __forceinline__ void fft_dif(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int TWS = 512 / N;
    int h = N / 2;
    // two radix-2 stages (distances h and h / 2) per pass over the data: the same operations in the same order, half the barriers
#pragma unroll 1
    for (; h >= 2; h >>= 2) {
        const int q = h >> 1, tstep = (N / (2 * h)) * TWS;
        for (int t = tid; t < NF * (N / 4); t += NT) {
            const int f = t % NF, j = t / NF;
            const int i = j & (q - 1);
            const int a = ((j - i) << 2) + i;  // < N - 3 q
            float2* p = s + f * SF + a * SE;
            const float2 x0 = p[0], x1 = p[q * SE], x2 = p[2 * q * SE], x3 = p[3 * q * SE];
            const float2 wa = tw[i * tstep], wb = tw[i * tstep + 128], wc = tw[2 * i * tstep];  // i tstep < 128
            const float2 y0 = make_float2(x0.x + x2.x, x0.y + x2.y), y1 = make_float2(x1.x + x3.x, x1.y + x3.y);
            const float ax = x0.x - x2.x, ay = x0.y - x2.y, bx = x1.x - x3.x, by = x1.y - x3.y;
            const float2 y2 = make_float2(ax * wa.x - ay * wa.y, ax * wa.y + ay * wa.x);
            const float2 y3 = make_float2(bx * wb.x - by * wb.y, bx * wb.y + by * wb.x);
            const float cx = y0.x - y1.x, cy = y0.y - y1.y, dx = y2.x - y3.x, dy = y2.y - y3.y;
            p[0] = make_float2(y0.x + y1.x, y0.y + y1.y);
            p[q * SE] = make_float2(cx * wc.x - cy * wc.y, cx * wc.y + cy * wc.x);
            p[2 * q * SE] = make_float2(y2.x + y3.x, y2.y + y3.y);
            p[3 * q * SE] = make_float2(dx * wc.x - dy * wc.y, dx * wc.y + dy * wc.x);
        }
        __syncthreads();
    }
#pragma unroll 1
    for (; h >= 1; h >>= 1) {
        const int tstep = (N / (2 * h)) * TWS;
        for (int t = tid; t < NF * (N / 2); t += NT) {
            const int f = t % NF, j = t / NF;
            const int i = j & (h - 1);
            const int a = ((j - i) << 1) + i;  // < N - h
            float2* p = s + f * SF + a * SE;
            float2* q = p + h * SE;
            const float2 u = *p, v = *q;
            const float2 w = tw[i * tstep];  // W_N^(i N / 2h): index < 256
            const float dx = u.x - v.x, dy = u.y - v.y;
            *p = make_float2(u.x + v.x, u.y + v.y);
            *q = make_float2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
        }
        __syncthreads();
    }
}

// Rows of L reals, transformed as L / 2 complex numbers (fft_dif: Z[k] at element brev(k)) -> X[kx], kx < L / 2, at element brev(kx).
template <int L, int NF, int SF, int NT>
__device__ __forceinline__ void real_split(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int NH = L / 2, BITS = ilog2(NH), TWS = 512 / L;
    for (int t = tid; t < NF * (NH / 2 + 1); t += NT) {
        const int f = t % NF, k = t / NF;  // k = 0 ... NH / 2 stands for the pair (k, NH - k)
        float2* row = s + f * SF;
        if (k == 0) {
            const float2 z = row[0];
            row[0] = make_float2(z.x + z.y, 0.f);
        } else {
            const int pa = brev<BITS>(k), pb = brev<BITS>(NH - k);
            const float2 za = row[pa], zb = row[pb];
            const float ex = 0.5f * (za.x + zb.x), ey = 0.5f * (za.y - zb.y);
            const float ox = 0.5f * (za.y + zb.y), oy = -0.5f * (za.x - zb.x);
            const float2 w = tw[k * TWS];
            const float tx = w.x * ox - w.y * oy, ty = w.x * oy + w.y * ox;
            row[pa] = make_float2(ex + tx, ey + ty);
            if (pb != pa) row[pb] = make_float2(ex - tx, ty - ey);  // X[NH - k] = conj(E[k] - W^k O[k])
        }
    }
    __syncthreads();
}

// NF rows of L fp32 values from `src` (row pitch W) to s[f * SF + m] = (x[2m], x[2m + 1]); a missing value (!(x >= 0)) is read as 0.
// -> this thread's number of missing values
template <int L, int NF, int SF, int NT>
__device__ __forceinline__ int load_rows(float2* __restrict__ s, const float* __restrict__ src, int W, int tid) {
    constexpr int Q = L / 4;
    int miss = 0;
    for (int t = tid; t < NF * Q; t += NT) {
        const int q = t % Q, f = t / Q;
        const f32x4 v = *(const f32x4*)(src + (int64_t)f * W + 4 * q);
        const bool p0 = v.x >= 0.f, p1 = v.y >= 0.f, p2 = v.z >= 0.f, p3 = v.w >= 0.f;
        miss += (p0 ? 0 : 1) + (p1 ? 0 : 1) + (p2 ? 0 : 1) + (p3 ? 0 : 1);
        float2* d = s + f * SF + 2 * q;  // (8-byte aligned only: SF is odd)
        d[0] = make_float2(p0 ? v.x : 0.f, p1 ? v.y : 0.f);
        d[1] = make_float2(p2 ? v.z : 0.f, p3 ? v.w : 0.f);
    }
    return miss;
}

__device__ __forceinline__ int isqrt_floor(int v) {  // v < 2^24
    int k = (int)sqrtf((float)v);
    while (k * k > v) --k;
    while ((k + 1) * (k + 1) <= v) ++k;
    return k;
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
    real_split<L, L, RS, NT>(s, tw, tid);
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
    real_split<L, NF, RS, NT>(s, tw, tid);
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

template <class K>
int psd_allow_lds(K kernel, int bytes) {
    if (bytes <= 64 * 1024) return 0;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        dgmr_set_error("dgmr_radial_psd: %d bytes of LDS per workgroup were refused: %s", bytes, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    return 0;
}

template <int L>
int psd_run_window(const PsdGeom& g, int64_t nwin, const float2* tw, double* power, int64_t* missing, hipStream_t st) {
    if (psd_allow_lds(psd_window_kernel<L>, psd_window_lds<L>()) != 0) return -2;
    hipLaunchKernelGGL(psd_window_kernel<L>, dim3((unsigned)nwin), dim3(psd_threads(L)), psd_window_lds<L>(), st, g, tw, power,
                       (long long*)missing);
    return 0;
}

template <int L>
int psd_run_two_pass(const PsdGeom& g, int64_t nwin, int64_t per_round, const float2* tw, float2* spec, double* part, double* power,
                     int64_t* missing, hipStream_t st) {
    constexpr int NH = L / 2, NCH = NH / psd_cols(L), RB = L / PSD_ROWS;
    if (psd_allow_lds(psd_rows_kernel<L>, psd_rows_lds<L>()) != 0 || psd_allow_lds(psd_cols_kernel<L>, psd_cols_lds<L>()) != 0) return -2;
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

// ---- spectral AR(1) noise windows (stochastic.py) --------------------------------------------------------------------------------------
// One workgroup per (plane, member, window of one class).  The window's half spectrum X [L][L / 2 + 1] and the noise amplitude
// g(r) |U| / L of every mode stay in registers through the T steps (element tid + j NT of the LDS layout belongs to thread tid:
// 17 elements x 4 registers at L = 128 and 512 threads); LDS holds one [L][L / 2 + 1] complex buffer (66 KB at L = 128) that every
// step fills with the white patch, transforms forward, overwrites with the updated state, transforms back and blends out - two
// workgroups share a CU.  The layout is the PSD kernel's, with the Nyquist column kx = L / 2 in the padding element of each row, so
// the column passes run over L / 2 + 1 columns.  The inverse of the DIF transform is a DIT that starts from the bit-reversed
// positions the DIF leaves: stage by stage the inverse butterfly (p, q) -> (p + q conj w, p - q conj w), which doubles the values -
// the factor L^2 of both axes is taken out by one exact multiplication in the store.  Twiddles: the table of psd_twiddle_kernel,
// computed by every workgroup for itself (256 double sincospi against T forward and inverse transforms).
// Blend: four launches, classes (0,0), (0,1), (1,0), (1,1) in stream order; the first stores value * weight, the others read, fma and
// write.  Windows of one class are disjoint, so no two workgroups of a launch touch one element: no atomics, the same bits every call.
struct ArGeom {
    const float* z0;
    const float* white;
    const float* rho;
    float* out;
    int64_t z0_plane_stride, white_member_stride, white_step_stride, out_member_stride, out_step_stride;
    int M, T, H, W, cy, cx, wins_y, wins_x;  // wins: the windows of this class per plane
    int wide_in, wide_out;                   // 16-byte accesses allowed for z0 and white / for out
};

constexpr int ar_state(int L) { return (L * (L / 2 + 1) + psd_threads(L) - 1) / psd_threads(L); }

template <int L>
constexpr int ar_lds() { return L * (L / 2 + 1) * 8 + PSD_TW * 8 + 4 * L * 4; }

// fft_dif undone: frequency k is read from element brev(k), sample n of 2^stages times the inverse lands at element n.
template <int N, int NF, int SE, int SF, int NT>
__device__ __forceinline__ void fft_dit_inverse(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int TWS = 512 / N;
    constexpr bool ODD = (ilog2(N) & 1) != 0;
    // fft_dif's passes backwards: its single last stage (distance 1, when log2 N is odd) first, then its two-stage passes from
    // the shortest distances to the longest, each pass undoing the stage of distance q = h / 2 and then the one of distance h
    if (ODD) {
        for (int t = tid; t < NF * (N / 2); t += NT) {
            const int f = t % NF, j = t / NF;
            float2* p = s + f * SF + 2 * j * SE;
            const float2 u = p[0], v = p[SE];  // twiddle 1
            p[0] = make_float2(u.x + v.x, u.y + v.y);
            p[SE] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int h = ODD ? 4 : 2; h <= N / 2; h <<= 2) {
        const int q = h >> 1, tstep = (N / (2 * h)) * TWS;
        for (int t = tid; t < NF * (N / 4); t += NT) {
            const int f = t % NF, j = t / NF;
            const int i = j & (q - 1);
            const int a = ((j - i) << 2) + i;  // < N - 3 q
            float2* p = s + f * SF + a * SE;
            const float2 z0 = p[0], z1 = p[q * SE], z2 = p[2 * q * SE], z3 = p[3 * q * SE];
            const float2 wa = tw[i * tstep], wb = tw[i * tstep + 128], wc = tw[2 * i * tstep];
            const float ax = z1.x * wc.x + z1.y * wc.y, ay = z1.y * wc.x - z1.x * wc.y;  // z1 conj(wc)
            const float bx = z3.x * wc.x + z3.y * wc.y, by = z3.y * wc.x - z3.x * wc.y;  // z3 conj(wc)
            const float2 y0 = make_float2(z0.x + ax, z0.y + ay), y1 = make_float2(z0.x - ax, z0.y - ay);
            const float2 y2 = make_float2(z2.x + bx, z2.y + by), y3 = make_float2(z2.x - bx, z2.y - by);
            const float cx = y2.x * wa.x + y2.y * wa.y, cy = y2.y * wa.x - y2.x * wa.y;  // y2 conj(wa)
            const float dx = y3.x * wb.x + y3.y * wb.y, dy = y3.y * wb.x - y3.x * wb.y;  // y3 conj(wb)
            p[0] = make_float2(y0.x + cx, y0.y + cy);
            p[q * SE] = make_float2(y1.x + dx, y1.y + dy);
            p[2 * q * SE] = make_float2(y0.x - cx, y0.y - cy);
            p[3 * q * SE] = make_float2(y1.x - dx, y1.y - dy);
        }
        __syncthreads();
    }
}

// real_split that also forms the Nyquist column: X[L / 2] = Re Z[0] - Im Z[0] goes to element L / 2 of the row.
template <int L, int NF, int SF, int NT>
__device__ __forceinline__ void real_split_nyquist(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int NH = L / 2, BITS = ilog2(NH), TWS = 512 / L;
    for (int t = tid; t < NF * (NH / 2 + 1); t += NT) {
        const int f = t % NF, k = t / NF;
        float2* row = s + f * SF;
        if (k == 0) {
            const float2 z = row[0];
            row[0] = make_float2(z.x + z.y, 0.f);
            row[NH] = make_float2(z.x - z.y, 0.f);
        } else {
            const int pa = brev<BITS>(k), pb = brev<BITS>(NH - k);
            const float2 za = row[pa], zb = row[pb];
            const float ex = 0.5f * (za.x + zb.x), ey = 0.5f * (za.y - zb.y);
            const float ox = 0.5f * (za.y + zb.y), oy = -0.5f * (za.x - zb.x);
            const float2 w = tw[k * TWS];
            const float tx = w.x * ox - w.y * oy, ty = w.x * oy + w.y * ox;
            row[pa] = make_float2(ex + tx, ey + ty);
            if (pb != pa) row[pb] = make_float2(ex - tx, ty - ey);
        }
    }
    __syncthreads();
}

// real_split_nyquist undone, up to a factor 2: X[kx] at element brev(kx) (kx = L / 2 at element L / 2) -> 2 Z[k] at element brev(k),
// Z the transform of z[m] = x[2m] + i x[2m + 1].  With S = X[k] + conj X[NH - k] and D = (X[k] - conj X[NH - k]) conj W_L^k:
// 2 Z[k] = S + i D,  2 Z[NH - k] = conj S + i conj D.  Only the real parts of X[0] and X[L / 2] enter: the result is real(ifft2).
template <int L, int NF, int SF, int NT>
__device__ __forceinline__ void real_merge(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int NH = L / 2, BITS = ilog2(NH), TWS = 512 / L;
    for (int t = tid; t < NF * (NH / 2 + 1); t += NT) {
        const int f = t % NF, k = t / NF;
        float2* row = s + f * SF;
        if (k == 0) {
            const float x0 = row[0].x, xn = row[NH].x;
            row[0] = make_float2(x0 + xn, x0 - xn);
        } else {
            const int pa = brev<BITS>(k), pb = brev<BITS>(NH - k);
            const float2 a = row[pa], b = row[pb];
            const float sx = a.x + b.x, sy = a.y - b.y;
            const float dx = a.x - b.x, dy = a.y + b.y;
            const float2 w = tw[k * TWS];
            const float tx = dx * w.x + dy * w.y, ty = dy * w.x - dx * w.y;  // D conj(w)
            row[pa] = make_float2(sx - ty, sy + tx);
            if (pb != pa) row[pb] = make_float2(sx + ty, tx - sy);
        }
    }
    __syncthreads();
}

// an L x L patch at `src` (row pitch W) -> s[y * RS + m] = (x[y][2m], x[y][2m + 1]), every value as it is
template <int L, int NT>
__device__ __forceinline__ void ar_load(float2* __restrict__ s, const float* __restrict__ src, int W, int wide, int tid) {
    constexpr int Q = L / 4, RS = L / 2 + 1;
    for (int t = tid; t < L * Q; t += NT) {
        const int q = t % Q, y = t / Q;
        const float* p = src + (int64_t)y * W + 4 * q;
        f32x4 v;
        if (wide) {
            v = *(const f32x4*)p;
        } else {
            v.x = p[0], v.y = p[1], v.z = p[2], v.w = p[3];
        }
        float2* d = s + y * RS + 2 * q;
        d[0] = make_float2(v.x, v.y);
        d[1] = make_float2(v.z, v.w);
    }
    __syncthreads();
}

template <int L>
__device__ __forceinline__ void ar_forward(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int NT = psd_threads(L), NH = L / 2, RS = NH + 1;
    fft_dif<NH, L, 1, RS, NT>(s, tw, tid);
    real_split_nyquist<L, L, RS, NT>(s, tw, tid);
    fft_dif<L, NH + 1, RS, 1, NT>(s, tw, tid);
}

template <int L>
__global__ __launch_bounds__(psd_threads(L)) void spectral_ar_kernel(ArGeom g) {
    constexpr int NT = psd_threads(L), NH = L / 2, RS = NH + 1, TOTAL = L * RS, NS = ar_state(L);
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;      // [L][RS]
    float2* tw = s + TOTAL;             // [PSD_TW]
    float* s_rho = (float*)(tw + PSD_TW);  // [L]
    float* s_gain = s_rho + L;          // [L]: sqrt(1 - rho^2)
    float* s_wy = s_gain + L;           // [L]: this window's blend weights down the rows ...
    float* s_wx = s_wy + L;             // [L]: ... and along them
    const int tid = threadIdx.x;
    const int per_plane = g.wins_y * g.wins_x;
    const int64_t n = blockIdx.x / per_plane;  // plane * M + member
    const int wi = (int)(blockIdx.x - n * per_plane);
    const int wy = wi / g.wins_x, wx = wi - wy * g.wins_x;
    const int y0 = wy * L + g.cy * NH, x0 = wx * L + g.cx * NH;  // y0 + L <= H, x0 + L <= W
    const int64_t p = n / g.M;
    for (int i = tid; i < PSD_TW; i += NT) {
        double sn, cs;
        sincospi(-(double)i / 256.0, &sn, &cs);
        tw[i] = make_float2((float)cs, (float)sn);
    }
    for (int i = tid; i < L; i += NT) {
        const float r = g.rho[i];
        s_rho[i] = r;
        s_gain[i] = (float)sqrt(fmax(fma(-(double)r, (double)r, 1.0), 0.0));
        // offset class: h(i) = sin^2(pi (i + 1/2) / L); aligned class: 1 - h of the offset window that covers the pixel, 1 in the
        // outer L / 2 of the frame where there is none
        const double sh = sinpi(((double)i + 0.5) / (double)L), sc = sinpi(((double)((i + NH) % L) + 0.5) / (double)L);
        const float h_own = (float)(sh * sh), h_other = (float)(sc * sc);
        const int Y = y0 + i, X = x0 + i;
        s_wy[i] = g.cy ? h_own : (Y < NH || Y >= g.H - NH) ? 1.f : 1.f - h_other;
        s_wx[i] = g.cx ? h_own : (X < NH || X >= g.W - NH) ? 1.f : 1.f - h_other;
    }
    __syncthreads();
    const int64_t origin = (int64_t)y0 * g.W + x0;
    ar_load<L, NT>(s, g.z0 + p * g.z0_plane_stride + origin, g.W, g.wide_in, tid);
    ar_forward<L>(s, tw, tid);
    float2 X[NS];
    float rho[NS], amp[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        X[j] = make_float2(0.f, 0.f);
        rho[j] = 0.f, amp[j] = 0.f;
        if (e < TOTAL) {
            const int row = e / RS, c = e - row * RS;
            int ky = brev<ilog2(L)>(row);
            ky = ky >= NH ? ky - L : ky;
            const int kx = c < NH ? brev<ilog2(NH)>(c) : NH;
            const int d2 = kx * kx + ky * ky;
            const int k = isqrt_floor(d2);
            const int r = d2 <= k * (k + 1) ? k : k + 1;  // r (r - 1) < d2 <= r (r + 1); r <= L / sqrt(2) + 1 < L
            X[j] = s[e];
            rho[j] = s_rho[r];
            amp[j] = s_gain[r] * (sqrtf(X[j].x * X[j].x + X[j].y * X[j].y) * (1.f / (float)L));
        }
    }
    const float* wh = g.white + n * g.white_member_stride + origin;
    float* out = g.out + n * g.out_member_stride + origin;
    constexpr float INV = 1.f / ((float)L * (float)L);
    for (int t = 0; t < g.T; ++t) {
        __syncthreads();  // the reads of the step before (or of the state) are done
        ar_load<L, NT>(s, wh + (int64_t)t * g.white_step_stride, g.W, g.wide_in, tid);
        ar_forward<L>(s, tw, tid);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int e = tid + j * NT;
            if (e < TOTAL) {
                const float2 v = s[e];
                X[j] = make_float2(fmaf(rho[j], X[j].x, amp[j] * v.x), fmaf(rho[j], X[j].y, amp[j] * v.y));
                s[e] = X[j];
            }
        }
        __syncthreads();
        fft_dit_inverse<L, NH + 1, RS, 1, NT>(s, tw, tid);
        real_merge<L, L, RS, NT>(s, tw, tid);
        fft_dit_inverse<NH, L, 1, RS, NT>(s, tw, tid);
        float* o = out + (int64_t)t * g.out_step_stride;
        const bool first = g.cy == 0 && g.cx == 0;
        for (int i = tid; i < L * (L / 4); i += NT) {
            const int q = i % (L / 4), y = i / (L / 4);
            const float2 a = s[y * RS + 2 * q], b = s[y * RS + 2 * q + 1];
            const float wrow = s_wy[y];
            const float w0 = wrow * s_wx[4 * q], w1 = wrow * s_wx[4 * q + 1], w2 = wrow * s_wx[4 * q + 2], w3 = wrow * s_wx[4 * q + 3];
            float* d = o + (int64_t)y * g.W + 4 * q;
            f32x4 v;
            if (first) {
                v.x = (a.x * INV) * w0, v.y = (a.y * INV) * w1, v.z = (b.x * INV) * w2, v.w = (b.y * INV) * w3;
            } else {
                if (g.wide_out) {
                    v = *(const f32x4*)d;
                } else {
                    v.x = d[0], v.y = d[1], v.z = d[2], v.w = d[3];
                }
                v.x = fmaf(a.x * INV, w0, v.x), v.y = fmaf(a.y * INV, w1, v.y), v.z = fmaf(b.x * INV, w2, v.z), v.w = fmaf(b.y * INV, w3, v.w);
            }
            if (g.wide_out) {
                *(f32x4*)d = v;
            } else {
                d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
            }
        }
    }
}

template <int L>
int ar_run(const ArGeom& g, int64_t blocks, hipStream_t st) {
    hipLaunchKernelGGL(spectral_ar_kernel<L>, dim3((unsigned)blocks), dim3(psd_threads(L)), ar_lds<L>(), st, g);
    return 0;
}

template <int L>
int ar_allow_lds() {
    if (ar_lds<L>() <= 64 * 1024) return 0;
    if (hipFuncSetAttribute((const void*)spectral_ar_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, ar_lds<L>()) != hipSuccess) {
        dgmr_set_error("dgmr_spectral_ar: %d bytes of LDS per workgroup were refused: %s", ar_lds<L>(), hipGetErrorString(hipGetLastError()));
        return -2;
    }
    return 0;
}

// ---- spectral AR(2) noise windows (stochastic.py: spectral_ar2) --------------------------------------------------------------------------
// spectral_ar_kernel with a second lag: X_t = phi1 X_(t-1) + phi2 X_(t-2) + g A Wh_t per mode, the coefficients per radial bin as
// passed (coef: [3][L] per plane, or one set for all).  Same workgroups, LDS buffer, transforms, blend and launches.  A thread holds
// BOTH spectra of its elements and the noise amplitude through the T steps: 5 registers per element, 85 at L = 128 (17 elements).
// phi1 and phi2 per element would make that 119, past the 128 that two workgroups of 512 threads on a CU may take, so they stay in
// two LDS tables of L floats and a thread keeps only the radial bin of each element, a byte (r < L <= 128), four to a register.
// zm1 is transformed first, in the same buffer, and kept as X_(t-2); then z0 as X_(t-1), which also gives the amplitude.
// Left to itself the compiler undoes the packing: it hoists the T-loop's invariants - the 17 extracted bins, the transforms'
// addresses - into registers of their own (184 VGPRs at L = 128: one workgroup per CU, 8.1 ms against spectral_ar's 5.0 ms on the
// 1536 x 1280, M = 8, T = 18 nowcast), and capped at 128 it spills them to scratch.  So every step starts from an opaque copy of
// the thread index and of the packed bins (two empty asm statements: no instruction, only a value the optimiser cannot follow across
// the iteration) and re-derives both, a few integer operations per element and step.  Allocation (code object metadata, no scratch
// at any L): 60 VGPRs at L = 32, 81 at L = 64, 122 at L = 128 - two workgroups per CU (4 waves per SIMD), as spectral_ar_kernel.
struct Ar2Geom {
    const float* z0;
    const float* zm1;
    const float* white;
    const float* coef;
    float* out;
    int64_t z0_plane_stride, zm1_plane_stride, coef_plane_stride, white_member_stride, white_step_stride, out_member_stride, out_step_stride;
    int M, T, H, W, cy, cx, wins_y, wins_x;  // wins: the windows of this class per plane
    int wide_in, wide_out;                   // 16-byte accesses allowed for z0, zm1 and white / for out
};

template <int L>
constexpr int ar2_lds() { return ar_lds<L>() + L * 4; }  // five rows of L floats: phi1, phi2, g and the two blend weight rows

template <int L>
__global__ __launch_bounds__(psd_threads(L), L == 128 ? 4 : 1) void spectral_ar2_kernel(Ar2Geom g) {  // (512 threads, 4 waves per SIMD)
    constexpr int NT = psd_threads(L), NH = L / 2, RS = NH + 1, TOTAL = L * RS, NS = ar_state(L), NB = (NS + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;           // [L][RS]
    float2* tw = s + TOTAL;                  // [PSD_TW]
    float* s_phi1 = (float*)(tw + PSD_TW);   // [L]
    float* s_phi2 = s_phi1 + L;              // [L]
    float* s_g = s_phi2 + L;                 // [L]
    float* s_wy = s_g + L;                   // [L]: this window's blend weights down the rows ...
    float* s_wx = s_wy + L;                  // [L]: ... and along them
    const int tid = threadIdx.x;
    const int per_plane = g.wins_y * g.wins_x;
    const int64_t n = blockIdx.x / per_plane;  // plane * M + member
    const int wi = (int)(blockIdx.x - n * per_plane);
    const int wy = wi / g.wins_x, wx = wi - wy * g.wins_x;
    const int y0 = wy * L + g.cy * NH, x0 = wx * L + g.cx * NH;  // y0 + L <= H, x0 + L <= W
    const int64_t p = n / g.M;
    for (int i = tid; i < PSD_TW; i += NT) {
        double sn, cs;
        sincospi(-(double)i / 256.0, &sn, &cs);
        tw[i] = make_float2((float)cs, (float)sn);
    }
    const float* coef = g.coef + p * g.coef_plane_stride;  // [3][L]
    for (int i = tid; i < L; i += NT) {
        s_phi1[i] = coef[i];
        s_phi2[i] = coef[L + i];
        s_g[i] = coef[2 * L + i];
        // the blend weights of spectral_ar_kernel
        const double sh = sinpi(((double)i + 0.5) / (double)L), sc = sinpi(((double)((i + NH) % L) + 0.5) / (double)L);
        const float h_own = (float)(sh * sh), h_other = (float)(sc * sc);
        const int Y = y0 + i, X = x0 + i;
        s_wy[i] = g.cy ? h_own : (Y < NH || Y >= g.H - NH) ? 1.f : 1.f - h_other;
        s_wx[i] = g.cx ? h_own : (X < NH || X >= g.W - NH) ? 1.f : 1.f - h_other;
    }
    __syncthreads();
    const int64_t origin = (int64_t)y0 * g.W + x0;
    float2 X1[NS], X2[NS];  // X_(t-1), X_(t-2)
    float amp[NS];
    unsigned int bins[NB];  // the radial bin of element j: byte j % 4 of bins[j / 4] (formed first: nothing else is live yet)
#pragma unroll
    for (int b = 0; b < NB; ++b) bins[b] = 0u;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        if (e < TOTAL) {
            const int row = e / RS, c = e - row * RS;
            int ky = brev<ilog2(L)>(row);
            ky = ky >= NH ? ky - L : ky;
            const int kx = c < NH ? brev<ilog2(NH)>(c) : NH;
            const int d2 = kx * kx + ky * ky;
            const int k = isqrt_floor(d2);
            const int r = d2 <= k * (k + 1) ? k : k + 1;  // r (r - 1) < d2 <= r (r + 1); r <= L / sqrt(2) + 1 < L <= 128: a byte
            bins[j >> 2] |= (unsigned int)r << (8 * (j & 3));
        }
    }
    ar_load<L, NT>(s, g.zm1 + p * g.zm1_plane_stride + origin, g.W, g.wide_in, tid);
    ar_forward<L>(s, tw, tid);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        X2[j] = e < TOTAL ? s[e] : make_float2(0.f, 0.f);
    }
    __syncthreads();  // everyone holds its part of X_-1 before the buffer is loaded again
    ar_load<L, NT>(s, g.z0 + p * g.z0_plane_stride + origin, g.W, g.wide_in, tid);
    ar_forward<L>(s, tw, tid);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        X1[j] = make_float2(0.f, 0.f);
        amp[j] = 0.f;
        if (e < TOTAL) {
            const int r = (int)((bins[j >> 2] >> (8 * (j & 3))) & 255u);
            X1[j] = s[e];
            amp[j] = s_g[r] * (sqrtf(X1[j].x * X1[j].x + X1[j].y * X1[j].y) * (1.f / (float)L));
        }
    }
    const float* wh = g.white + n * g.white_member_stride + origin;
    float* out = g.out + n * g.out_member_stride + origin;
    constexpr float INV = 1.f / ((float)L * (float)L);
    for (int t = 0; t < g.T; ++t) {
        int lt = tid;  // this step's thread index and bins: the same values, opaque (see the section's comment)
        asm volatile("" : "+v"(lt));
#pragma unroll
        for (int b = 0; b < NB; ++b) asm volatile("" : "+v"(bins[b]));
        __syncthreads();  // the reads of the step before (or of the state) are done
        ar_load<L, NT>(s, wh + (int64_t)t * g.white_step_stride, g.W, g.wide_in, lt);
        ar_forward<L>(s, tw, lt);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int e = lt + j * NT;
            if (e < TOTAL) {
                const float2 v = s[e];
                const int r = (int)((bins[j >> 2] >> (8 * (j & 3))) & 255u);
                const float p1 = s_phi1[r], p2 = s_phi2[r];
                const float2 nx = make_float2(fmaf(p1, X1[j].x, fmaf(p2, X2[j].x, amp[j] * v.x)),
                                              fmaf(p1, X1[j].y, fmaf(p2, X2[j].y, amp[j] * v.y)));
                X2[j] = X1[j];
                X1[j] = nx;
                s[e] = nx;
            }
        }
        __syncthreads();
        fft_dit_inverse<L, NH + 1, RS, 1, NT>(s, tw, lt);
        real_merge<L, L, RS, NT>(s, tw, lt);
        fft_dit_inverse<NH, L, 1, RS, NT>(s, tw, lt);
        float* o = out + (int64_t)t * g.out_step_stride;
        const bool first = g.cy == 0 && g.cx == 0;
        for (int i = lt; i < L * (L / 4); i += NT) {
            const int q = i % (L / 4), y = i / (L / 4);
            const float2 a = s[y * RS + 2 * q], b = s[y * RS + 2 * q + 1];
            const float wrow = s_wy[y];
            const float w0 = wrow * s_wx[4 * q], w1 = wrow * s_wx[4 * q + 1], w2 = wrow * s_wx[4 * q + 2], w3 = wrow * s_wx[4 * q + 3];
            float* d = o + (int64_t)y * g.W + 4 * q;
            f32x4 v;
            if (first) {
                v.x = (a.x * INV) * w0, v.y = (a.y * INV) * w1, v.z = (b.x * INV) * w2, v.w = (b.y * INV) * w3;
            } else {
                if (g.wide_out) {
                    v = *(const f32x4*)d;
                } else {
                    v.x = d[0], v.y = d[1], v.z = d[2], v.w = d[3];
                }
                v.x = fmaf(a.x * INV, w0, v.x), v.y = fmaf(a.y * INV, w1, v.y), v.z = fmaf(b.x * INV, w2, v.z), v.w = fmaf(b.y * INV, w3, v.w);
            }
            if (g.wide_out) {
                *(f32x4*)d = v;
            } else {
                d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
            }
        }
    }
}

template <int L>
int ar2_run(const Ar2Geom& g, int64_t blocks, hipStream_t st) {
    hipLaunchKernelGGL(spectral_ar2_kernel<L>, dim3((unsigned)blocks), dim3(psd_threads(L)), ar2_lds<L>(), st, g);
    return 0;
}

template <int L>
int ar2_allow_lds() {
    if (ar2_lds<L>() <= 64 * 1024) return 0;
    if (hipFuncSetAttribute((const void*)spectral_ar2_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, ar2_lds<L>()) != hipSuccess) {
        dgmr_set_error("dgmr_spectral_ar2: %d bytes of LDS per workgroup were refused: %s", ar2_lds<L>(), hipGetErrorString(hipGetLastError()));
        return -2;
    }
    return 0;
}

// ---- lag spectra (stochastic.py: lag_spectra, estimate_rho) ----------------------------------------------------------------------------
// One workgroup per (plane, window), the four window classes of the recursion in one launch.  The `b` patch is transformed first and
// its half spectrum kept in registers (ar_state(L) elements per thread, as spectral_ar_kernel holds X), the `a` patch is transformed
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
    constexpr int NT = psd_threads(L), NH = L / 2, RS = NH + 1, TOTAL = L * RS, NS = ar_state(L), P = NT / L;
    static_assert(3 * P * L * 8 <= TOTAL * 8 && 3 * L <= NT, "the partials live in the transform buffer, one thread per (q, r) adds them");
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;  // [L][RS]
    float2* tw = s + TOTAL;         // [PSD_TW]
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x / g.wins_per_plane;
    int wi = (int)(blockIdx.x - n * g.wins_per_plane);
    // the window's class: (0,0), (0,1), (1,0), (1,1), row-major inside a class
    const int ny = g.H / L, nx = g.W / L;
    int cy = 0, cx = 0;
    for (int c = 0; c < 3; ++c) {
        const int count = (ny - cy) * (nx - cx);
        if (wi < count) break;
        wi -= count;
        cy = (c + 1) >> 1, cx = (c + 1) & 1;
    }
    const int wins_x = nx - cx;  // > 0: wi is inside this class
    const int wy = wi / wins_x, wx = wi - wy * wins_x;
    const int y0 = wy * L + cy * NH, x0 = wx * L + cx * NH;  // y0 + L <= H, x0 + L <= W
    for (int i = tid; i < PSD_TW; i += NT) {
        double sn, cs;
        sincospi(-(double)i / 256.0, &sn, &cs);
        tw[i] = make_float2((float)cs, (float)sn);
    }
    __syncthreads();
    const int64_t origin = (int64_t)y0 * g.W + x0;
    float2 B[NS];
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const float* src = pass == 0 ? g.b + n * g.b_plane_stride : g.a + n * g.a_plane_stride;
        ar_load<L, NT>(s, src + origin, g.W, g.wide, tid);
        ar_forward<L>(s, tw, tid);
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
    if (lag_lds<L>() > 64 * 1024 &&
        hipFuncSetAttribute((const void*)lag_spectra_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, lag_lds<L>()) != hipSuccess) {
        dgmr_set_error("dgmr_lag_spectra: %d bytes of LDS per workgroup were refused: %s", lag_lds<L>(), hipGetErrorString(hipGetLastError()));
        return -2;
    }
    hipLaunchKernelGGL(lag_spectra_kernel<L>, dim3((unsigned)blocks), dim3(psd_threads(L)), lag_lds<L>(), st, g);
    return 0;
}

// ---- exceedance table ----------------------------------------------------------------------------------------------------------------
constexpr int EXC_MAX_M = 32, EXC_MAX_K = 8, EXC_THREADS = 256, EXC_TARGET_BLOCKS = 4096;

inline int exc_blocks_per_plane(int64_t N, int64_t quads) {
    const int64_t want = std::max<int64_t>(1, EXC_TARGET_BLOCKS / N);
    return (int)std::min<int64_t>(want, (quads + EXC_THREADS - 1) / EXC_THREADS);
}

// quads = H * W / 4 is a multiple of 64 (H and W are multiples of 16): a wave is inside the plane as a whole or not at all.
__global__ __launch_bounds__(EXC_THREADS) void exceedance_kernel(const float* __restrict__ fc, int64_t mstride, const float* __restrict__ obs,
                                                                 int M, int64_t quads, int BPP, const float* __restrict__ thr, int K,
                                                                 unsigned long long* __restrict__ table) {
    __shared__ unsigned int s_hist[EXC_MAX_K * (EXC_MAX_M + 1) * 2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_hist = K * (M + 1) * 2;
    for (int i = tid; i < n_hist; i += EXC_THREADS) s_hist[i] = 0;
    float tk[EXC_MAX_K];
#pragma unroll
    for (int k = 0; k < EXC_MAX_K; ++k) tk[k] = k < K ? thr[k] : __builtin_inff();
    __syncthreads();
    const int64_t n = blockIdx.x / BPP;
    const int b = (int)(blockIdx.x - n * BPP);
    const f32x4* __restrict__ obs_n = (const f32x4*)(obs + n * quads * 4);
    const float* __restrict__ fc_n = fc + n * quads * 4;
    for (int64_t i = (int64_t)b * EXC_THREADS + tid; i < quads; i += (int64_t)BPP * EXC_THREADS) {
        const f32x4 yv = obs_n[i];
        const float y[4] = {yv.x, yv.y, yv.z, yv.w};
        int cnt[EXC_MAX_K][4];
#pragma unroll
        for (int k = 0; k < EXC_MAX_K; ++k)
#pragma unroll
            for (int p = 0; p < 4; ++p) cnt[k][p] = 0;
#pragma unroll 4
        for (int m = 0; m < M; ++m) {
            const f32x4 xv = *(const f32x4*)(fc_n + m * mstride + i * 4);
            const float x[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int k = 0; k < EXC_MAX_K; ++k)
#pragma unroll
                for (int p = 0; p < 4; ++p) cnt[k][p] += x[p] >= tk[k] ? 1 : 0;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const bool pres = y[p] >= 0.f;
            const unsigned long long P = __ballot(pres);
            if (!P) continue;  // (wave-uniform)
            const int leader = __ffsll((long long)P) - 1;
#pragma unroll
            for (int k = 0; k < EXC_MAX_K; ++k) {
                if (k >= K) break;  // (uniform)
                const int key = (k * (M + 1) + cnt[k][p]) * 2 + (y[p] >= tk[k] ? 1 : 0);  // < n_hist: cnt <= M
                const int k0 = __builtin_amdgcn_readlane(key, leader);
                const unsigned long long same = __ballot(pres && key == k0);
                if (lane == leader) atomicAdd(&s_hist[k0], (unsigned int)__popcll(same));
                if (pres && key != k0) atomicAdd(&s_hist[key], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n_hist; i += EXC_THREADS)
        if (s_hist[i]) atomicAdd(&table[n * n_hist + i], (unsigned long long)s_hist[i]);
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

extern "C" int dgmr_spectral_ar(const float* z0, int64_t z0_plane_stride, const float* white, int64_t white_member_stride,
                                int64_t white_step_stride, const float* rho, int P, int M, int T, int H, int W, int L, float* out,
                                int64_t out_member_stride, int64_t out_step_stride, void* stream) {
    const char* fn = "dgmr_spectral_ar";
    DGMR_CHECK_ARG(L == 32 || L == 64 || L == 128, "%s: window L=%d is not one of 32, 64, 128", fn, L);
    DGMR_CHECK_ARG(T >= 1 && T <= 64, "%s: T=%d lead times, 1 ... 64 are supported", fn, T);
    DGMR_CHECK_ARG(P >= 1 && M >= 1 && (int64_t)P * M <= (1 << 24), "%s: P=%d planes of M=%d members are out of range", fn, P, M);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % L == 0 && W % L == 0, "%s: H=%d and W=%d must be positive multiples of the window L=%d", fn, H, W, L);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(z0 && white && rho && out, "%s: null pointer", fn);
    const int64_t N = (int64_t)P * M, plane = (int64_t)H * W, cap = INT64_MAX / 4 / (N * 64);
    DGMR_CHECK_ARG(z0_plane_stride >= 0 && z0_plane_stride <= cap, "%s: z0_plane_stride=%lld out of range", fn, (long long)z0_plane_stride);
    DGMR_CHECK_ARG((N == 1 || (white_member_stride >= plane && white_member_stride <= cap)) &&
                       (T == 1 || (white_step_stride >= plane && white_step_stride <= cap)),
                   "%s: white_member_stride=%lld and white_step_stride=%lld must be at least H * W = %lld", fn,
                   (long long)white_member_stride, (long long)white_step_stride, (long long)plane);
    DGMR_CHECK_ARG((N == 1 || (out_member_stride >= plane && out_member_stride <= cap)) &&
                       (T == 1 || (out_step_stride >= plane && out_step_stride <= cap)),
                   "%s: out_member_stride=%lld and out_step_stride=%lld must be at least H * W = %lld", fn, (long long)out_member_stride,
                   (long long)out_step_stride, (long long)plane);
    DGMR_CHECK_ARG(N * (H / L) * (W / L) <= (1 << 30), "%s: %lld windows are out of range", fn, (long long)(N * (H / L) * (W / L)));
    const int64_t wms = N == 1 ? 0 : white_member_stride, wss = T == 1 ? 0 : white_step_stride;
    const int64_t oms = N == 1 ? 0 : out_member_stride, oss = T == 1 ? 0 : out_step_stride;
    const int wide_in = (((uintptr_t)z0 | (uintptr_t)white) & 15) == 0 && z0_plane_stride % 4 == 0 && wms % 4 == 0 && wss % 4 == 0;
    const int wide_out = ((uintptr_t)out & 15) == 0 && oms % 4 == 0 && oss % 4 == 0;
    const int rc = L == 32 ? ar_allow_lds<32>() : L == 64 ? ar_allow_lds<64>() : ar_allow_lds<128>();
    if (rc != 0) return rc;
    hipStream_t st = ST;
    for (int c = 0; c < 4; ++c) {  // (0,0) stores; (0,1), (1,0), (1,1) add, in this order
        const int cy = c >> 1, cx = c & 1;
        const int wins_y = H / L - cy, wins_x = W / L - cx;
        if (wins_y == 0 || wins_x == 0) continue;
        const ArGeom g{z0, white, rho, out, z0_plane_stride, wms, wss, oms, oss, M, T, H, W, cy, cx, wins_y, wins_x, wide_in, wide_out};
        const int64_t blocks = N * wins_y * wins_x;
        if (L == 32)
            ar_run<32>(g, blocks, st);
        else if (L == 64)
            ar_run<64>(g, blocks, st);
        else
            ar_run<128>(g, blocks, st);
    }
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_spectral_ar2(const float* z0, int64_t z0_plane_stride, const float* zm1, int64_t zm1_plane_stride, const float* white,
                                 int64_t white_member_stride, int64_t white_step_stride, const float* coef, int64_t coef_plane_stride, int P,
                                 int M, int T, int H, int W, int L, float* out, int64_t out_member_stride, int64_t out_step_stride,
                                 void* stream) {
    const char* fn = "dgmr_spectral_ar2";
    DGMR_CHECK_ARG(L == 32 || L == 64 || L == 128, "%s: window L=%d is not one of 32, 64, 128", fn, L);
    DGMR_CHECK_ARG(T >= 1 && T <= 64, "%s: T=%d lead times, 1 ... 64 are supported", fn, T);
    DGMR_CHECK_ARG(P >= 1 && M >= 1 && (int64_t)P * M <= (1 << 24), "%s: P=%d planes of M=%d members are out of range", fn, P, M);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % L == 0 && W % L == 0, "%s: H=%d and W=%d must be positive multiples of the window L=%d", fn, H, W, L);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(z0 && zm1 && white && coef && out, "%s: null pointer", fn);
    const int64_t N = (int64_t)P * M, plane = (int64_t)H * W, cap = INT64_MAX / 4 / (N * 64);
    DGMR_CHECK_ARG(z0_plane_stride >= 0 && z0_plane_stride <= cap && zm1_plane_stride >= 0 && zm1_plane_stride <= cap,
                   "%s: z0_plane_stride=%lld or zm1_plane_stride=%lld out of range", fn, (long long)z0_plane_stride,
                   (long long)zm1_plane_stride);
    DGMR_CHECK_ARG(coef_plane_stride == 0 || (coef_plane_stride >= 3 * L && coef_plane_stride <= cap),
                   "%s: coef_plane_stride=%lld must be 0 (one set for all planes) or at least 3 L = %d", fn, (long long)coef_plane_stride, 3 * L);
    DGMR_CHECK_ARG((N == 1 || (white_member_stride >= plane && white_member_stride <= cap)) &&
                       (T == 1 || (white_step_stride >= plane && white_step_stride <= cap)),
                   "%s: white_member_stride=%lld and white_step_stride=%lld must be at least H * W = %lld", fn,
                   (long long)white_member_stride, (long long)white_step_stride, (long long)plane);
    DGMR_CHECK_ARG((N == 1 || (out_member_stride >= plane && out_member_stride <= cap)) &&
                       (T == 1 || (out_step_stride >= plane && out_step_stride <= cap)),
                   "%s: out_member_stride=%lld and out_step_stride=%lld must be at least H * W = %lld", fn, (long long)out_member_stride,
                   (long long)out_step_stride, (long long)plane);
    DGMR_CHECK_ARG(N * (H / L) * (W / L) <= (1 << 30), "%s: %lld windows are out of range", fn, (long long)(N * (H / L) * (W / L)));
    const int64_t wms = N == 1 ? 0 : white_member_stride, wss = T == 1 ? 0 : white_step_stride;
    const int64_t oms = N == 1 ? 0 : out_member_stride, oss = T == 1 ? 0 : out_step_stride;
    const int wide_in = (((uintptr_t)z0 | (uintptr_t)zm1 | (uintptr_t)white) & 15) == 0 && z0_plane_stride % 4 == 0 &&
                        zm1_plane_stride % 4 == 0 && wms % 4 == 0 && wss % 4 == 0;
    const int wide_out = ((uintptr_t)out & 15) == 0 && oms % 4 == 0 && oss % 4 == 0;
    const int rc = L == 32 ? ar2_allow_lds<32>() : L == 64 ? ar2_allow_lds<64>() : ar2_allow_lds<128>();
    if (rc != 0) return rc;
    hipStream_t st = ST;
    for (int c = 0; c < 4; ++c) {  // (0,0) stores; (0,1), (1,0), (1,1) add, in this order
        const int cy = c >> 1, cx = c & 1;
        const int wins_y = H / L - cy, wins_x = W / L - cx;
        if (wins_y == 0 || wins_x == 0) continue;
        const Ar2Geom g{z0, zm1, white, coef, out, z0_plane_stride, zm1_plane_stride, coef_plane_stride, wms, wss, oms, oss, M, T, H, W,
                        cy, cx, wins_y, wins_x, wide_in, wide_out};
        const int64_t blocks = N * wins_y * wins_x;
        if (L == 32)
            ar2_run<32>(g, blocks, st);
        else if (L == 64)
            ar2_run<64>(g, blocks, st);
        else
            ar2_run<128>(g, blocks, st);
    }
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

extern "C" int dgmr_exceedance_table(const float* forecast, int64_t member_stride, const float* observed, int M, int64_t N, int H, int W,
                                     const float* thresholds, int K, int64_t* table, void* stream) {
    const char* fn = "dgmr_exceedance_table";
    DGMR_CHECK_ARG(M >= 1 && M <= EXC_MAX_M, "%s: M=%d members, 1 ... %d are supported", fn, M, EXC_MAX_M);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "%s: H=%d and W=%d must be positive multiples of 16", fn, H, W);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(K >= 0 && K <= EXC_MAX_K, "%s: K=%d thresholds, at most %d are supported", fn, K, EXC_MAX_K);
    DGMR_CHECK_ARG(forecast && observed && ((thresholds && table) || K == 0), "%s: null pointer", fn);
    DGMR_CHECK_ARG(M == 1 || (member_stride >= 0 && member_stride % 4 == 0 && member_stride <= INT64_MAX / 4 / EXC_MAX_M),
                   "%s: member_stride=%lld must be a non-negative multiple of 4 elements", fn, (long long)member_stride);
    DGMR_CHECK_ARG((((uintptr_t)forecast | (uintptr_t)observed) & 15) == 0, "%s: forecast and observed must be 16-byte aligned", fn);
    DGMR_CHECK_ARG(((uintptr_t)table & 7) == 0, "%s: table must be 8-byte aligned", fn);
    if (K == 0) return 0;  // an empty table
    hipStream_t st = ST;
    if (hipMemsetAsync(table, 0, (size_t)N * K * (M + 1) * 2 * sizeof(int64_t), st) != hipSuccess) {
        dgmr_set_error("%s: clearing the table failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    const int64_t quads = (int64_t)H * W / 4;
    const int BPP = exc_blocks_per_plane(N, quads);
    hipLaunchKernelGGL(exceedance_kernel, dim3((unsigned)(N * BPP)), dim3(EXC_THREADS), 0, st, forecast, M == 1 ? 0 : member_stride, observed,
                       M, quads, BPP, thresholds, K, (unsigned long long*)table);
    DGMR_CHECK_LAUNCH();
    return 0;
}
