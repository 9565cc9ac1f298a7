// The noise windows of the stochastic advection ensemble (stochastic.py) on the transforms of fft_lds.h: an AR(1) per Fourier mode
// (dgmr_spectral_ar) and the same with a second lag (dgmr_spectral_ar2).
//
// One workgroup per (plane, member, window of one class).  The window's half spectrum X [L][L / 2 + 1] and the noise amplitude
// g(r) |U| / L of every mode stay in registers through the T steps (element tid + j NT of the LDS layout belongs to thread tid:
// 17 elements at L = 128 and 512 threads); LDS holds one [L][L / 2 + 1] complex buffer (66 KB at L = 128) that every step fills with
// the white patch, transforms forward, overwrites with the updated state, transforms back and blends out - two workgroups share a
// CU.  The factor L^2 of the inverse transforms is taken out by one exact multiplication in the store.  Twiddles: the table of
// psd_twiddle_kernel, computed by every workgroup for itself (256 double sincospi against T forward and inverse transforms).
// Blend: four launches, classes (0,0), (0,1), (1,0), (1,1) in stream order; the first stores value * weight, the others read, fma and
// write.  Windows of one class are disjoint, so no two workgroups of a launch touch one element: no atomics, the same bits every call.
//
// The two kernels share everything but how a thread keeps its modes' coefficients - see spectral_ar2_kernel - and stay two bodies.
#include "fft_lds.h"

namespace {

// what both recursions take: the white field, the result and the windows of one class
struct ArCommon {
    const float* white;
    float* out;
    int64_t white_member_stride, white_step_stride, out_member_stride, out_step_stride;
    int M, T, H, W, cy, cx, wins_y, wins_x;  // wins: the windows of this class per plane
    int wide_in, wide_out;                   // 16-byte accesses allowed for the states and white / for out
};

struct ArGeom {
    static constexpr int ROWS = 4;  // LDS rows of L floats: rho, sqrt(1 - rho^2) and the two blend weight rows
    ArCommon c;
    const float* z0;
    const float* rho;
    int64_t z0_plane_stride;
};

struct Ar2Geom {
    static constexpr int ROWS = 5;  // phi1, phi2, g and the two blend weight rows
    ArCommon c;
    const float* z0;
    const float* zm1;
    const float* coef;
    int64_t z0_plane_stride, zm1_plane_stride, coef_plane_stride;
};

template <int L, class Geom>
constexpr int ar_lds() { return L * (L / 2 + 1) * 8 + PSD_TW * 8 + Geom::ROWS * L * 4; }

struct ArWindow {
    int64_t n, p, origin;  // plane * M + member, plane, the window's first element in its H x W plane
    int y0, x0;
};

template <int L>
__device__ __forceinline__ ArWindow ar_window(const ArCommon& g) {
    const int per_plane = g.wins_y * g.wins_x;
    ArWindow w;
    w.n = blockIdx.x / per_plane;
    window_corner<L>((int)(blockIdx.x - w.n * per_plane), g.wins_x, g.cy, g.cx, w.y0, w.x0);
    w.p = w.n / g.M;
    w.origin = (int64_t)w.y0 * g.W + w.x0;
    return w;
}

// The twiddles, and this window's blend weights down the rows (s_wy [L]) and along them (s_wx [L]).  Offset class:
// h(i) = sin^2(pi (i + 1/2) / L); aligned class: 1 - h of the offset window that covers the pixel, 1 in the outer L / 2 of the frame
// where there is none.  No barrier.
template <int L>
__device__ __forceinline__ void ar_tables(const ArCommon& g, const ArWindow& w, float2* __restrict__ tw, float* __restrict__ s_wy,
                                          float* __restrict__ s_wx, int tid) {
    constexpr int NT = psd_threads(L), NH = L / 2;
    fill_twiddles<NT>(tw, tid);
    for (int i = tid; i < L; i += NT) {
        const double sh = sinpi(((double)i + 0.5) / (double)L), sc = sinpi(((double)((i + NH) % L) + 0.5) / (double)L);
        const float h_own = (float)(sh * sh), h_other = (float)(sc * sc);
        const int Y = w.y0 + i, X = w.x0 + i;
        s_wy[i] = g.cy ? h_own : (Y < NH || Y >= g.H - NH) ? 1.f : 1.f - h_other;
        s_wx[i] = g.cx ? h_own : (X < NH || X >= g.W - NH) ? 1.f : 1.f - h_other;
    }
}

// s: the new state's spectrum -> the window's patch of `o` (one lead time), weighted: stored by class (0,0), added by the others
template <int L>
__device__ __forceinline__ void ar_blend_out(const ArCommon& g, float2* __restrict__ s, const float2* __restrict__ tw,
                                             const float* __restrict__ s_wy, const float* __restrict__ s_wx, float* __restrict__ o, int tid) {
    constexpr int NT = psd_threads(L), RS = L / 2 + 1;
    constexpr float INV = 1.f / ((float)L * (float)L);
    window_inverse<L>(s, tw, tid);
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

// ---- AR(1): X_t = rho X_(t-1) + sqrt(1 - rho^2) A Wh_t per mode; rho and the amplitude of every owned element in registers ------------
template <int L>
__global__ __launch_bounds__(psd_threads(L)) void spectral_ar_kernel(ArGeom g) {
    constexpr int NT = psd_threads(L), TOTAL = L * (L / 2 + 1), NS = window_state(L);
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;         // [L][L / 2 + 1]
    float2* tw = s + TOTAL;                // [PSD_TW]
    float* s_rho = (float*)(tw + PSD_TW);  // [L]
    float* s_gain = s_rho + L;             // [L]: sqrt(1 - rho^2)
    float* s_wy = s_gain + L;              // [L]
    float* s_wx = s_wy + L;                // [L]
    const int tid = threadIdx.x;
    const ArWindow w = ar_window<L>(g.c);
    ar_tables<L>(g.c, w, tw, s_wy, s_wx, tid);
    for (int i = tid; i < L; i += NT) {
        const float r = g.rho[i];
        s_rho[i] = r;
        s_gain[i] = (float)sqrt(fmax(fma(-(double)r, (double)r, 1.0), 0.0));
    }
    __syncthreads();
    window_forward<L>(s, tw, g.z0 + w.p * g.z0_plane_stride + w.origin, g.c.W, g.c.wide_in, tid);
    float2 X[NS];
    float rho[NS], amp[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        X[j] = make_float2(0.f, 0.f);
        rho[j] = 0.f, amp[j] = 0.f;
        if (e < TOTAL) {
            const int r = radial_bin_of_element<L>(e);
            X[j] = s[e];
            rho[j] = s_rho[r];
            amp[j] = s_gain[r] * (sqrtf(X[j].x * X[j].x + X[j].y * X[j].y) * (1.f / (float)L));
        }
    }
    const float* wh = g.c.white + w.n * g.c.white_member_stride + w.origin;
    float* out = g.c.out + w.n * g.c.out_member_stride + w.origin;
    for (int t = 0; t < g.c.T; ++t) {
        __syncthreads();  // the reads of the step before (or of the state) are done
        window_forward<L>(s, tw, wh + (int64_t)t * g.c.white_step_stride, g.c.W, g.c.wide_in, tid);
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
        ar_blend_out<L>(g.c, s, tw, s_wy, s_wx, out + (int64_t)t * g.c.out_step_stride, tid);
    }
}

// ---- AR(2): X_t = phi1 X_(t-1) + phi2 X_(t-2) + g A Wh_t per mode, the coefficients per radial bin as passed (coef: [3][L] per
// plane, or one set for all).  A thread holds BOTH spectra of its elements and the noise amplitude through the T steps: 5 registers
// per element, 85 at L = 128 (17 elements).  phi1 and phi2 per element would make that 119, past the 128 that two workgroups of 512
// threads on a CU may take, so they stay in two LDS tables of L floats and a thread keeps only the radial bin of each element, a
// byte (r < L <= 128), four to a register.  zm1 is transformed first, in the same buffer, and kept as X_(t-2); then z0 as X_(t-1),
// which also gives the amplitude.
// Left to itself the compiler undoes the packing: it hoists the T-loop's invariants - the 17 extracted bins, the transforms'
// addresses - into registers of their own (184 VGPRs at L = 128: one workgroup per CU, 8.1 ms against spectral_ar's 5.0 ms on the
// 1536 x 1280, M = 8, T = 18 nowcast), and capped at 128 it spills them to scratch.  So every step starts from an opaque copy of
// the thread index and of the packed bins (two empty asm statements: no instruction, only a value the optimiser cannot follow across
// the iteration) and re-derives both, a few integer operations per element and step.  Allocation (code object metadata, no scratch
// at any L): 60 VGPRs at L = 32, 81 at L = 64, 123 at L = 128 - two workgroups per CU (4 waves per SIMD), as spectral_ar_kernel.
// The parts shared with spectral_ar_kernel cost one register at L = 128 (122 with every part written out here); 128 is the limit.
template <int L>
__global__ __launch_bounds__(psd_threads(L), L == 128 ? 4 : 1) void spectral_ar2_kernel(Ar2Geom g) {  // (512 threads, 4 waves per SIMD)
    constexpr int NT = psd_threads(L), TOTAL = L * (L / 2 + 1), NS = window_state(L), NB = (NS + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char psd_smem[];
    float2* s = (float2*)psd_smem;          // [L][L / 2 + 1]
    float2* tw = s + TOTAL;                 // [PSD_TW]
    float* s_phi1 = (float*)(tw + PSD_TW);  // [L]
    float* s_phi2 = s_phi1 + L;             // [L]
    float* s_g = s_phi2 + L;                // [L]
    float* s_wy = s_g + L;                  // [L]
    float* s_wx = s_wy + L;                 // [L]
    const int tid = threadIdx.x;
    const ArWindow w = ar_window<L>(g.c);
    ar_tables<L>(g.c, w, tw, s_wy, s_wx, tid);
    const float* coef = g.coef + w.p * g.coef_plane_stride;  // [3][L]
    for (int i = tid; i < L; i += NT) {
        s_phi1[i] = coef[i];
        s_phi2[i] = coef[L + i];
        s_g[i] = coef[2 * L + i];
    }
    __syncthreads();
    float2 X1[NS], X2[NS];  // X_(t-1), X_(t-2)
    float amp[NS];
    unsigned int bins[NB];  // the radial bin of element j: byte j % 4 of bins[j / 4] (formed first: nothing else is live yet)
#pragma unroll
    for (int b = 0; b < NB; ++b) bins[b] = 0u;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        if (e < TOTAL) bins[j >> 2] |= (unsigned int)radial_bin_of_element<L>(e) << (8 * (j & 3));
    }
    window_forward<L>(s, tw, g.zm1 + w.p * g.zm1_plane_stride + w.origin, g.c.W, g.c.wide_in, tid);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int e = tid + j * NT;
        X2[j] = e < TOTAL ? s[e] : make_float2(0.f, 0.f);
    }
    __syncthreads();  // everyone holds its part of X_-1 before the buffer is loaded again
    window_forward<L>(s, tw, g.z0 + w.p * g.z0_plane_stride + w.origin, g.c.W, g.c.wide_in, tid);
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
    const float* wh = g.c.white + w.n * g.c.white_member_stride + w.origin;
    float* out = g.c.out + w.n * g.c.out_member_stride + w.origin;
    for (int t = 0; t < g.c.T; ++t) {
        int lt = tid;  // this step's thread index and bins: the same values, opaque (see the section's comment)
        asm volatile("" : "+v"(lt));
#pragma unroll
        for (int b = 0; b < NB; ++b) asm volatile("" : "+v"(bins[b]));
        __syncthreads();  // the reads of the step before (or of the state) are done
        window_forward<L>(s, tw, wh + (int64_t)t * g.c.white_step_stride, g.c.W, g.c.wide_in, lt);
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
        ar_blend_out<L>(g.c, s, tw, s_wy, s_wx, out + (int64_t)t * g.c.out_step_stride, lt);
    }
}

template <int L>
auto ar_kernel(const ArGeom&) { return spectral_ar_kernel<L>; }
template <int L>
auto ar_kernel(const Ar2Geom&) { return spectral_ar2_kernel<L>; }

// one launch per class of windows that the plane has: (0,0) stores; (0,1), (1,0), (1,1) add, in this order
template <int L, class Geom>
int ar_launch(Geom g, int64_t N, const char* fn, hipStream_t st) {
    constexpr int lds = ar_lds<L, Geom>();
    if (allow_lds(ar_kernel<L>(g), lds, fn) != 0) return -2;
    for (int c = 0; c < 4; ++c) {
        window_class(c, g.c.cy, g.c.cx);
        g.c.wins_y = g.c.H / L - g.c.cy, g.c.wins_x = g.c.W / L - g.c.cx;
        if (g.c.wins_y == 0 || g.c.wins_x == 0) continue;
        hipLaunchKernelGGL(ar_kernel<L>(g), dim3((unsigned)(N * g.c.wins_y * g.c.wins_x)), dim3(psd_threads(L)), lds, st, g);
    }
    return 0;
}

template <class Geom>
int ar_launch(const Geom& g, int64_t N, int L, const char* fn, hipStream_t st) {
    return L == 32 ? ar_launch<32>(g, N, fn, st) : L == 64 ? ar_launch<64>(g, N, fn, st) : ar_launch<128>(g, N, fn, st);
}

// The checks both entries make first.  Between the two halves each entry checks its own pointers and plane strides.
int ar_check_shape(const char* fn, int P, int M, int T, int H, int W, int L) {
    DGMR_CHECK_ARG(L == 32 || L == 64 || L == 128, "%s: window L=%d is not one of 32, 64, 128", fn, L);
    DGMR_CHECK_ARG(T >= 1 && T <= 64, "%s: T=%d lead times, 1 ... 64 are supported", fn, T);
    DGMR_CHECK_ARG(P >= 1 && M >= 1 && (int64_t)P * M <= (1 << 24), "%s: P=%d planes of M=%d members are out of range", fn, P, M);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % L == 0 && W % L == 0, "%s: H=%d and W=%d must be positive multiples of the window L=%d", fn, H, W, L);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    return 0;
}

int64_t ar_stride_cap(int P, int M) { return INT64_MAX / 4 / ((int64_t)P * M * 64); }

// The checks both entries make last -> c: strides that the shape leaves unused are 0; wide_in covers white alone, the entry adds
// its states.
int ar_check_layout(const char* fn, const float* white, int64_t white_member_stride, int64_t white_step_stride, int P, int M, int T, int H,
                    int W, int L, float* out, int64_t out_member_stride, int64_t out_step_stride, ArCommon& c) {
    const int64_t N = (int64_t)P * M, plane = (int64_t)H * W, cap = ar_stride_cap(P, M);
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
    const int wide_in = ((uintptr_t)white & 15) == 0 && wms % 4 == 0 && wss % 4 == 0;
    const int wide_out = ((uintptr_t)out & 15) == 0 && oms % 4 == 0 && oss % 4 == 0;
    c = ArCommon{white, out, wms, wss, oms, oss, M, T, H, W, 0, 0, 0, 0, wide_in, wide_out};
    return 0;
}

}  // namespace

extern "C" int dgmr_spectral_ar(const float* z0, int64_t z0_plane_stride, const float* white, int64_t white_member_stride,
                                int64_t white_step_stride, const float* rho, int P, int M, int T, int H, int W, int L, float* out,
                                int64_t out_member_stride, int64_t out_step_stride, void* stream) {
    const char* fn = "dgmr_spectral_ar";
    if (ar_check_shape(fn, P, M, T, H, W, L) != 0) return -1;
    DGMR_CHECK_ARG(z0 && white && rho && out, "%s: null pointer", fn);
    DGMR_CHECK_ARG(z0_plane_stride >= 0 && z0_plane_stride <= ar_stride_cap(P, M), "%s: z0_plane_stride=%lld out of range", fn,
                   (long long)z0_plane_stride);
    ArGeom g{{}, z0, rho, z0_plane_stride};
    if (ar_check_layout(fn, white, white_member_stride, white_step_stride, P, M, T, H, W, L, out, out_member_stride, out_step_stride, g.c) != 0)
        return -1;
    g.c.wide_in = g.c.wide_in && ((uintptr_t)z0 & 15) == 0 && z0_plane_stride % 4 == 0;
    const int rc = ar_launch(g, (int64_t)P * M, L, fn, ST);
    if (rc != 0) return rc;
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_spectral_ar2(const float* z0, int64_t z0_plane_stride, const float* zm1, int64_t zm1_plane_stride, const float* white,
                                 int64_t white_member_stride, int64_t white_step_stride, const float* coef, int64_t coef_plane_stride, int P,
                                 int M, int T, int H, int W, int L, float* out, int64_t out_member_stride, int64_t out_step_stride,
                                 void* stream) {
    const char* fn = "dgmr_spectral_ar2";
    if (ar_check_shape(fn, P, M, T, H, W, L) != 0) return -1;
    DGMR_CHECK_ARG(z0 && zm1 && white && coef && out, "%s: null pointer", fn);
    const int64_t cap = ar_stride_cap(P, M);
    DGMR_CHECK_ARG(z0_plane_stride >= 0 && z0_plane_stride <= cap && zm1_plane_stride >= 0 && zm1_plane_stride <= cap,
                   "%s: z0_plane_stride=%lld or zm1_plane_stride=%lld out of range", fn, (long long)z0_plane_stride,
                   (long long)zm1_plane_stride);
    DGMR_CHECK_ARG(coef_plane_stride == 0 || (coef_plane_stride >= 3 * L && coef_plane_stride <= cap),
                   "%s: coef_plane_stride=%lld must be 0 (one set for all planes) or at least 3 L = %d", fn, (long long)coef_plane_stride, 3 * L);
    Ar2Geom g{{}, z0, zm1, coef, z0_plane_stride, zm1_plane_stride, coef_plane_stride};
    if (ar_check_layout(fn, white, white_member_stride, white_step_stride, P, M, T, H, W, L, out, out_member_stride, out_step_stride, g.c) != 0)
        return -1;
    g.c.wide_in = g.c.wide_in && (((uintptr_t)z0 | (uintptr_t)zm1) & 15) == 0 && z0_plane_stride % 4 == 0 && zm1_plane_stride % 4 == 0;
    const int rc = ar_launch(g, (int64_t)P * M, L, fn, ST);
    if (rc != 0) return rc;
    DGMR_CHECK_LAUNCH();
    return 0;
}
