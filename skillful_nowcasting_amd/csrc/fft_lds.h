// fp32 transforms of L x L windows in LDS, shared by the spectral units (spectrum.hip: dgmr_radial_psd, dgmr_lag_spectra;
// spectral_ar.hip: dgmr_spectral_ar, dgmr_spectral_ar2).
//
// Radix-2 decimation-in-frequency transforms (two stages per pass and barrier), twiddles from a table of exp(-2 pi i k / 512)
// computed in double and rounded to fp32.  The input is real, so a row of L reals is transformed as L / 2 complex numbers
// z[m] = x[2m] + i x[2m + 1] - which is how a 16-byte load delivers them - and split afterwards:
//   X[k] = E[k] + W_L^k O[k],  E[k] = (Z[k] + conj Z[L/2 - k]) / 2,  O[k] = (Z[k] - conj Z[L/2 - k]) / 2i,  kx = 0 ... L / 2 - 1.
// Nothing is reordered: a DIF transform leaves frequency k at the bit-reversed position and its users address a mode by __brev.  The
// inverse is a DIT that starts from those positions: stage by stage the inverse butterfly (p, q) -> (p + q conj w, p - q conj w),
// which doubles the values - its users take the factor out in their store.
// LDS layout: in every batch of transforms the lanes of a wave run over the transforms, not over the butterflies of one, and the
// stride between transforms is either one element or an odd number of elements (rows are padded by one complex number), so at every
// butterfly distance the 32 lanes of an LDS lane group fall on 32 different 8-byte bank pairs.
// A whole window is [L][L / 2 + 1] complex (66 KB at L = 128); window_forward puts the Nyquist column kx = L / 2 in the padding
// element of each row, so its column passes run over L / 2 + 1 columns.
#pragma once
#include "common.h"

namespace {

constexpr int PSD_TW = 256;  // twiddle table: exp(-2 pi i k / 512), k < 256

constexpr int psd_threads(int L) { return L == 32 ? 128 : L == 64 ? 256 : 512; }
constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
// elements of a window's half spectrum [L][L / 2 + 1] per thread: element tid + j psd_threads(L) of the LDS layout belongs to thread tid
constexpr int window_state(int L) { return (L * (L / 2 + 1) + psd_threads(L) - 1) / psd_threads(L); }

// Raise a kernel's limit of dynamic LDS where `bytes` needs it; a refusal is reported under the entry's name `fn`.
template <class K>
int allow_lds(K kernel, int bytes, const char* fn) {
    if (bytes <= 64 * 1024) return 0;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        dgmr_set_error("%s: %d bytes of LDS per workgroup were refused: %s", fn, bytes, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    return 0;
}

// The overlapping windows of the stochastic ensemble (stochastic.py: window_table): class c = 0 ... 3 is (cy, cx) = (0,0), (0,1),
// (1,0), (1,1), offset by L / 2 along the axes whose index is 1; a class has (H / L - cy) (W / L - cx) windows, row-major.
__host__ __device__ __forceinline__ void window_class(int c, int& cy, int& cx) { cy = c >> 1, cx = c & 1; }

// window `wi` of a class with wins_x windows per row -> its first row and column: y0 + L <= H, x0 + L <= W
template <int L>
__device__ __forceinline__ void window_corner(int wi, int wins_x, int cy, int cx, int& y0, int& x0) {
    const int wy = wi / wins_x, wx = wi - wy * wins_x;
    y0 = wy * L + cy * (L / 2), x0 = wx * L + cx * (L / 2);
}

// The table of psd_twiddle_kernel, computed by a workgroup for itself.  No barrier.
template <int NT>
__device__ __forceinline__ void fill_twiddles(float2* __restrict__ tw, int tid) {
    for (int i = tid; i < PSD_TW; i += NT) {
        double sn, cs;
        sincospi(-(double)i / 256.0, &sn, &cs);  // -2 pi i / 512
        tw[i] = make_float2((float)cs, (float)sn);
    }
}

template <int BITS>
__device__ __forceinline__ int brev(int v) { return (int)(__brev((unsigned int)v) >> (32 - BITS)); }

__device__ __forceinline__ int isqrt_floor(int v) {  // v < 2^24
    int k = (int)sqrtf((float)v);
    while (k * k > v) --k;
    while ((k + 1) * (k + 1) <= v) ++k;
    return k;
}

// element e of a transformed window [L][L / 2 + 1] (window_forward) -> the radial bin r of its mode:
// r (r - 1) < kx^2 + ky^2 <= r (r + 1) over the signed frequencies; r <= L / sqrt(2) + 1 < L
template <int L>
__device__ __forceinline__ int radial_bin_of_element(int e) {
    constexpr int NH = L / 2, RS = NH + 1;
    const int row = e / RS, c = e - row * RS;
    int ky = brev<ilog2(L)>(row);
    ky = ky >= NH ? ky - L : ky;
    const int kx = c < NH ? brev<ilog2(NH)>(c) : NH;
    const int d2 = kx * kx + ky * ky;
    const int k = isqrt_floor(d2);
    return d2 <= k * (k + 1) ? k : k + 1;
}

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

// Rows of L reals, transformed as L / 2 complex numbers (fft_dif: Z[k] at element brev(k)) -> X[kx], kx < L / 2, at element brev(kx).
// NYQUIST: the column kx = L / 2 is formed too, X[L / 2] = Re Z[0] - Im Z[0], at element L / 2 of the row.
template <int L, int NF, int SF, int NT, bool NYQUIST>
__device__ __forceinline__ void real_split(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int NH = L / 2, BITS = ilog2(NH), TWS = 512 / L;
    for (int t = tid; t < NF * (NH / 2 + 1); t += NT) {
        const int f = t % NF, k = t / NF;  // k = 0 ... NH / 2 stands for the pair (k, NH - k)
        float2* row = s + f * SF;
        if (k == 0) {
            const float2 z = row[0];
            row[0] = make_float2(z.x + z.y, 0.f);
            if (NYQUIST) row[NH] = make_float2(z.x - z.y, 0.f);
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

// real_split<NYQUIST> undone, up to a factor 2: X[kx] at element brev(kx) (kx = L / 2 at element L / 2) -> 2 Z[k] at element brev(k),
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

// an L x L patch at `src` (row pitch W) -> s[y * RS + m] = (x[y][2m], x[y][2m + 1]), every value as it is; 16-byte loads if `wide`
template <int L, int NT>
__device__ __forceinline__ void load_patch(float2* __restrict__ s, const float* __restrict__ src, int W, int wide, int tid) {
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

// the patch at `src` -> its half spectrum in s [L][L / 2 + 1]: mode (ky, kx) at element brev(ky) * RS + brev(kx), kx = L / 2 at L / 2
template <int L>
__device__ __forceinline__ void window_forward(float2* __restrict__ s, const float2* __restrict__ tw, const float* __restrict__ src, int W,
                                               int wide, int tid) {
    constexpr int NT = psd_threads(L), NH = L / 2, RS = NH + 1;
    load_patch<L, NT>(s, src, W, wide, tid);
    fft_dif<NH, L, 1, RS, NT>(s, tw, tid);
    real_split<L, L, RS, NT, true>(s, tw, tid);
    fft_dif<L, NH + 1, RS, 1, NT>(s, tw, tid);
}

// window_forward undone, up to the factor L^2 of both axes: s[y * RS + m] = L^2 (x[y][2m], x[y][2m + 1])
template <int L>
__device__ __forceinline__ void window_inverse(float2* __restrict__ s, const float2* __restrict__ tw, int tid) {
    constexpr int NT = psd_threads(L), NH = L / 2, RS = NH + 1;
    fft_dit_inverse<L, NH + 1, RS, 1, NT>(s, tw, tid);
    real_merge<L, L, RS, NT>(s, tw, tid);
    fft_dit_inverse<NH, L, 1, RS, NT>(s, tw, tid);
}

}  // namespace
