// The advection baseline on the device (advection.py): block-matching motion between two frames (dgmr_block_match) and the
// semi-Lagrangian extrapolation of a frame along a motion field for all lead times (dgmr_advect; dgmr_advect_series: the same with a
// source of its own per lead time and one field plane per group of planes - stochastic.py's ensemble members;
// dgmr_advect_series_perturbed: that with a velocity error per plane and lead time along and across the local motion).
//
// Block matching.  One workgroup per (plane, block).  The `next` block (B x B) is staged in LDS first and its wet elements are
// counted on the way; a dry block - most of a radar frame - writes its five +inf and leaves before the search window of `prev`
// ((B + 2R)^2 elements) is touched.  Otherwise the window is staged once (elements outside the frame as 0: no candidate reads them)
// and every thread takes displacements: thread index -> (wy, wx) = (R - dy, R - dx), the window position of the displaced block's
// top-left corner, wx fastest, so the lanes of a wave read consecutive LDS words of the window and the block pixel is a broadcast.
// A displacement is summed by ONE thread, fmaf(diff, diff, acc) in row-major pixel order: the order is fixed and two launches give
// the same bits.  The workgroup has as many threads (a multiple of 64, at most 512) as spread the (2R + 1)^2 displacements evenly
// over the fewest passes: 128 threads for R = 4 (81), 320 for R = 8 (289, one pass), 384 for R = 16 (1089, three passes).
// LDS at B = 32, R = 16: 4 KiB block + 16 KiB window + 4.3 KiB costs, so six workgroups share a CU.  The window pitch is B + 2R
// words: lanes that differ in wy by one are B + 2R words apart, which is 16 (mod 32) at 32/8 and 16/8 - the 2R + 1 = 17 lanes of a
// window row then overlap the next row's banks in one word only.
// The minimum is a total order - (cost, dy^2 + dx^2, dy, dx), the last three packed into one integer key - so the order of the
// reduction (lane shuffles, then the waves' results in LDS) cannot matter.
//
// Advection.  One thread owns V = 4 pixels of a row (16-byte stores; V = 1 where W, the output pointer or its strides do not allow
// them) and keeps their displacements D in registers through the T steps; the lattice of the field and the source frame are read
// through the caches.  Position arithmetic per axis and step (the `c` of the accuracy bound in include/dgmr_hip.h):
//   q = p - D                       1 rounded operation
//   g = (q - origin) / spacing      2, then clamped to [0, G - 1]; i0 = min(floor(g), G - 2), f = g - i0 (exact)
//   v = bilinear(lattice, g)        3 interpolations a + f (b - a), each one subtraction and one fma: 6
//   D = D + v                       1
// and the sample position s = p - D once per lead time (1): 10 per step + 1, on two axes - c = 22.
// A source tap is fmaf(f, b - a, a) as well: f = 0 returns a itself, so an integer displacement copies the source bit for bit, and
// the interpolation's own rounding is at most 4 * 2^-24 * max|x| (two one-axis interpolations of 2 * 2^-24 each, blended, plus the
// blend's subtraction and fma).
//
// Perturbed velocities (dgmr_advect_series_perturbed).  A second lattice of the field's geometry holds directions (uy, ux), which
// the host has normalised - the kernel has no division of its own, no square root and no transcendental - and every plane n and
// lead time t has an amplitude pair (a_par, a_perp), loaded once per step by each thread with its own n (a workgroup may straddle
// two planes).  At q = p - D, with the field's node indices i0 / i1 and weights f for both lattices, in this order:
//   (vy, vx) = bilinear(field)(q)                         as above
//   (uy, ux) = bilinear(direction)(q)                     lerp_fma, x then y, as for the field
//   vy' = fmaf(a_par, uy, fmaf(a_perp, -ux, vy))          the perpendicular of (uy, ux) is (-ux, uy)
//   vx' = fmaf(a_par, ux, fmaf(a_perp,  uy, vx))
//   D = D + v';  out[n, t][p] = s_t(p - D)
// An axis of v' takes both components of the direction: 2 x 6 rounded operations for their interpolations and 2 for the fmas, 14 on
// top of the 10 per step - (10 + 14) per step + 1, on two axes - c' = 50.  a = 0 returns v itself (fmaf(0, u, v) = v for finite u).
//
// Lucas-Kanade refinement (dgmr_lk_refine).  One workgroup of 256 threads per (plane, block), block matching's grid.  Thread 0 reads
// the block's minimum cost and displacement d0; a dry block writes its outputs and leaves before anything is staged.  Otherwise
// the `next` block (B x B) and the (B + 2)^2 window of `prev` whose corner is (y0 - d0y - 1, x0 - d0x - 1) are staged in LDS
// (8.7 KiB at B = 32; elements outside the frame and missing ones as 0).  d stays within d0 +- 1, so the sample of interior pixel
// (i, j) sits at window coordinate (i + 1 - ey, j + 1 - ex) with e = d - d0 in [-1, 1]: between i and i + 2, its four taps between
// i and i + 3 <= B + 1 - no tap leaves the window, and the position is formed from numbers below 64, not from frame coordinates.
// A thread owns the interior pixels e = tid + 256 k in row-major order (900 at B = 32: k < 4; 196 at B = 16: k < 1) and keeps their
// Q, gy, gx in registers through the iterations.  The sums (G once, b per iteration, the residual at the end): fp32 fmaf per thread
// in k order, then float64 - xor butterflies over the wave's 64 lanes (every lane ends with the same bits: a + b = b + a), the four
// waves' sums through LDS, added in wave order by every thread, which then solves the 2 x 2 system in float64 for itself from
// identical values; control flow stays uniform.  No atomics: two launches give the same bits.  The LDS slots of successive sums
// alternate between two sets, so one barrier per sum is enough.
// Window pitch B + 2 words.  The lanes of a 32-lane group read B - 2 consecutive words of one window row and continue in the next:
// at B = 32 that is 30 + 2 lanes, the two stragglers a pitch (34 = 2 mod 32) further, on banks two of the 30 hold - a two-way
// conflict on two banks, one extra LDS cycle per tap read.  Only a pitch of 30 or 62 (mod 32: the rows of a group tiling the banks)
// is free of it; 62 would nearly double the window for a cycle per read in a kernel that block matching outweighs many times over.
#include "common.h"

namespace {

constexpr int BM_MAX_R = 16, BM_MAX_THREADS = 512;

struct BmGeom {
    const float* prev;
    const float* next;
    int64_t plane_stride;
    int H, W, stride, R, By, Bx, min_wet;
    float wet_threshold;
};

__device__ __forceinline__ float present_or_zero(float v) { return v >= 0.f ? v : 0.f; }

// (cost, key) < (cost2, key2) in the total order; a NaN cost never wins
__device__ __forceinline__ bool bm_less(float c, int k, float c2, int k2) { return c < c2 || (c == c2 && k < k2); }

__device__ __forceinline__ int bm_key(int dy, int dx, int R) {
    const int D = 2 * R + 1;
    return (dy * dy + dx * dx) * 2048 + (dy + R) * D + (dx + R);  // (dy + R) D + dx + R < 1089 < 2048
}

template <int B>
__global__ __launch_bounds__(BM_MAX_THREADS) void block_match_kernel(BmGeom g, int32_t* __restrict__ disp, float* __restrict__ cost,
                                                                     int32_t* __restrict__ wet) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_smem[];
    const int R = g.R, D = 2 * R + 1, ND = D * D, WP = B + 2 * R;
    float* s_next = (float*)bm_smem;    // [B][B]
    float* s_win = s_next + B * B;      // [WP][WP]
    float* s_cost = s_win + WP * WP;    // [ND]
    __shared__ int s_wet;
    __shared__ float s_best_c[BM_MAX_THREADS / 64];
    __shared__ int s_best_k[BM_MAX_THREADS / 64];
    const int tid = threadIdx.x, NT = blockDim.x;
    const int per_plane = g.By * g.Bx;
    const int64_t id = blockIdx.x;
    const int64_t n = id / per_plane;
    const int b = (int)(id - n * per_plane);
    const int by = b / g.Bx, bx = b - by * g.Bx;
    const int y0 = by * g.stride, x0 = bx * g.stride;  // y0 + B <= H, x0 + B <= W
    if (tid == 0) s_wet = 0;
    __syncthreads();
    const float* nx = g.next + n * g.plane_stride + (int64_t)y0 * g.W + x0;
    int my_wet = 0;
    for (int e = tid; e < B * B; e += NT) {
        const int i = e / B, j = e - i * B;
        const float v = present_or_zero(nx[(int64_t)i * g.W + j]);
        my_wet += v >= g.wet_threshold ? 1 : 0;
        s_next[e] = v;
    }
    if (my_wet) atomicAdd(&s_wet, my_wet);
    __syncthreads();
    const int n_wet = s_wet;
    if (n_wet < g.min_wet) {  // dry (uniform over the workgroup): no search
        if (tid == 0) {
            wet[id] = n_wet;
            disp[id * 2] = 0;
            disp[id * 2 + 1] = 0;
        }
        if (tid < 5) cost[id * 5 + tid] = __builtin_inff();
        return;
    }
    const float* pv = g.prev + n * g.plane_stride;
    for (int e = tid; e < WP * WP; e += NT) {
        const int i = e / WP, j = e - i * WP;
        const int y = y0 - R + i, x = x0 - R + j;
        s_win[e] = (y >= 0 && y < g.H && x >= 0 && x < g.W) ? present_or_zero(pv[(int64_t)y * g.W + x]) : 0.f;
    }
    __syncthreads();
    float best_c = __builtin_inff();
    int best_k = INT32_MAX;
    for (int d = tid; d < ND; d += NT) {
        const int wy = d / D, wx = d - wy * D;
        const int dy = R - wy, dx = R - wx;
        const int py = y0 - dy, px = x0 - dx;  // the displaced block's corner in `prev`
        float acc = __builtin_inff();
        if (py >= 0 && py + B <= g.H && px >= 0 && px + B <= g.W) {
            acc = 0.f;
            const float* w = s_win + wy * WP + wx;
            for (int i = 0; i < B; ++i) {
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const float df = s_next[i * B + j] - w[i * WP + j];
                    acc = fmaf(df, df, acc);
                }
            }
        }
        s_cost[d] = acc;
        const int k = bm_key(dy, dx, R);
        if (bm_less(acc, k, best_c, best_k)) best_c = acc, best_k = k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float c2 = __shfl_xor(best_c, o, 64);
        const int k2 = __shfl_xor(best_k, o, 64);
        if (bm_less(c2, k2, best_c, best_k)) best_c = c2, best_k = k2;
    }
    if ((tid & 63) == 0) s_best_c[tid >> 6] = best_c, s_best_k[tid >> 6] = best_k;
    __syncthreads();  // (also publishes s_cost)
    if (tid < 5) {
        for (int wv = 0; wv < NT / 64; ++wv)
            if (wv == 0 || bm_less(s_best_c[wv], s_best_k[wv], best_c, best_k)) best_c = s_best_c[wv], best_k = s_best_k[wv];
        // (0, 0) is always a candidate, so for finite input the minimum is finite and best_k a real key; all-NaN costs keep (0, 0)
        const int pos = best_k == INT32_MAX ? R * D + R : best_k & 2047;
        const int wy = pos / D, wx = pos - wy * D;  // here as (dy + R, dx + R)
        const int dy = wy - R, dx = wx - R;
        if (tid == 0) {
            wet[id] = n_wet;
            disp[id * 2] = dy;
            disp[id * 2 + 1] = dx;
        }
        // entry 0: the minimum; 1 ... 4: (dy - 1, dx), (dy + 1, dx), (dy, dx - 1), (dy, dx + 1)
        const int ny = dy + (tid == 1 ? -1 : tid == 2 ? 1 : 0), nxd = dx + (tid == 3 ? -1 : tid == 4 ? 1 : 0);
        float c = __builtin_inff();
        if (ny >= -R && ny <= R && nxd >= -R && nxd <= R) c = s_cost[(R - ny) * D + (R - nxd)];
        cost[id * 5 + tid] = c;
    }
}

inline int bm_threads(int R) {
    const int nd = (2 * R + 1) * (2 * R + 1);
    const int passes = (nd + BM_MAX_THREADS - 1) / BM_MAX_THREADS;
    const int per = (nd + passes - 1) / passes;
    return std::min(BM_MAX_THREADS, (per + 63) / 64 * 64);
}

struct AdvGeom {
    const float* x;
    const float* field;
    float* out;
    int64_t x_plane_stride, field_plane_stride, out_plane_stride, out_step_stride, items;
    int H, W, Gy, Gx, T;
    float origin, spacing;
    int64_t x_step_stride;  // dgmr_advect_series: the source of lead time t is x + (t - 1) x_step_stride ...
    int field_group;        // ... and plane n reads field plane n / field_group
    // dgmr_advect_series_perturbed: the direction lattice (the field's geometry and plane mapping) and amplitude[n][t][2] = (a_par, a_perp)
    const float* direction;
    const float* amplitude;
    int64_t direction_plane_stride;
};

// lattice coordinate of pixel coordinate q on an axis of G nodes -> the lower node i0, the upper node i1 and the weight of i1
__device__ __forceinline__ void lattice_coord(float q, float origin, float spacing, int G, int& i0, int& i1, float& f) {
    float gc = (q - origin) / spacing;
    gc = fminf(fmaxf(gc, 0.f), (float)(G - 1));  // (a NaN becomes 0)
    i0 = min((int)floorf(gc), max(G - 2, 0));
    i1 = min(i0 + 1, G - 1);
    f = gc - (float)i0;
}

__device__ __forceinline__ float lerp_fma(float a, float b, float f) { return fmaf(f, b - a, a); }

__device__ __forceinline__ float source_tap(const float* __restrict__ x, int H, int W, int y, int xx) {
    return (y >= 0 && y < H && xx >= 0 && xx < W) ? present_or_zero(x[(int64_t)y * W + xx]) : 0.f;
}

__device__ __forceinline__ float source_sample(const float* __restrict__ x, int H, int W, float sy, float sx) {
    // beyond one pixel outside the frame every tap is 0: clamping there keeps the integer conversion in range (and maps a NaN to -2)
    sy = fminf(fmaxf(sy, -2.f), (float)H + 1.f);
    sx = fminf(fmaxf(sx, -2.f), (float)W + 1.f);
    const float fy0 = floorf(sy), fx0 = floorf(sx);
    const int iy = (int)fy0, ix = (int)fx0;
    const float fy = sy - fy0, fx = sx - fx0;
    const float top = lerp_fma(source_tap(x, H, W, iy, ix), source_tap(x, H, W, iy, ix + 1), fx);
    const float bot = lerp_fma(source_tap(x, H, W, iy + 1, ix), source_tap(x, H, W, iy + 1, ix + 1), fx);
    return lerp_fma(top, bot, fy);
}

// SERIES = false is dgmr_advect as it always was; SERIES = true adds the per-step source and the shared field plane, nothing else;
// PERTURBED (with SERIES) adds the direction taps and the two fmas per axis, nothing else
template <int V, bool SERIES, bool PERTURBED = false>
__global__ __launch_bounds__(256) void advect_kernel(AdvGeom g) {
    static_assert(SERIES || !PERTURBED, "the perturbed kernel is a series kernel");
    const int64_t item = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (item >= g.items) return;
    const int WV = g.W / V;
    const int64_t row = item / WV;
    const int xq = (int)(item - row * WV) * V;
    const int64_t n = row / g.H;
    const int y = (int)(row - n * g.H);
    const float* __restrict__ x = g.x + n * g.x_plane_stride;
    const float* __restrict__ fld = g.field + (SERIES ? n / g.field_group : n) * g.field_plane_stride;
    float* __restrict__ o = g.out + n * g.out_plane_stride + (int64_t)y * g.W + xq;
    const float* __restrict__ dir = nullptr;
    const float* __restrict__ amp = nullptr;
    if constexpr (PERTURBED) {
        dir = g.direction + (n / g.field_group) * g.direction_plane_stride;
        amp = g.amplitude + n * g.T * 2;  // n < 2^24, T <= 64
    }
    const float py = (float)y;
    float Dy[V], Dx[V];
#pragma unroll
    for (int k = 0; k < V; ++k) Dy[k] = 0.f, Dx[k] = 0.f;
    for (int t = 0; t < g.T; ++t) {
        float r[V];
        float a_par = 0.f, a_perp = 0.f;
        if constexpr (PERTURBED) a_par = amp[2 * t], a_perp = amp[2 * t + 1];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float px = (float)(xq + k);
            int y0, y1, x0, x1;
            float fy, fx;
            lattice_coord(py - Dy[k], g.origin, g.spacing, g.Gy, y0, y1, fy);
            lattice_coord(px - Dx[k], g.origin, g.spacing, g.Gx, x0, x1, fx);
            const float* a = fld + ((int64_t)y0 * g.Gx + x0) * 2;
            const float* b = fld + ((int64_t)y0 * g.Gx + x1) * 2;
            const float* c = fld + ((int64_t)y1 * g.Gx + x0) * 2;
            const float* d = fld + ((int64_t)y1 * g.Gx + x1) * 2;
            float vy = lerp_fma(lerp_fma(a[0], b[0], fx), lerp_fma(c[0], d[0], fx), fy);
            float vx = lerp_fma(lerp_fma(a[1], b[1], fx), lerp_fma(c[1], d[1], fx), fy);
            if constexpr (PERTURBED) {
                const float* da = dir + ((int64_t)y0 * g.Gx + x0) * 2;
                const float* db = dir + ((int64_t)y0 * g.Gx + x1) * 2;
                const float* dc = dir + ((int64_t)y1 * g.Gx + x0) * 2;
                const float* dd = dir + ((int64_t)y1 * g.Gx + x1) * 2;
                const float uy = lerp_fma(lerp_fma(da[0], db[0], fx), lerp_fma(dc[0], dd[0], fx), fy);
                const float ux = lerp_fma(lerp_fma(da[1], db[1], fx), lerp_fma(dc[1], dd[1], fx), fy);
                vy = fmaf(a_par, uy, fmaf(a_perp, -ux, vy));
                vx = fmaf(a_par, ux, fmaf(a_perp, uy, vx));
            }
            Dy[k] += vy;
            Dx[k] += vx;
            r[k] = source_sample(SERIES ? x + (int64_t)t * g.x_step_stride : x, g.H, g.W, py - Dy[k], px - Dx[k]);
        }
        float* dst = o + (int64_t)t * g.out_step_stride;
        if constexpr (V == 4) {
            f32x4 v;
            v.x = r[0], v.y = r[1], v.z = r[2], v.w = r[3];
            *(f32x4*)dst = v;
        } else {
            dst[0] = r[0];
        }
    }
}

// ---- Lucas-Kanade refinement of the block match ---------------------------------------------------------------------------------
constexpr int LK_THREADS = 256, LK_WAVES = LK_THREADS / 64, LK_MAX_ITERATIONS = 16;

struct LkGeom {
    const float* prev;
    const float* next;
    const int32_t* disp;
    const float* cost;
    int64_t plane_stride;
    int H, W, stride, By, Bx, iterations;
    float eig_ratio;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // both lanes of a pair form a + b: every lane ends with the same bits
    return v;
}

// The workgroup's sums of NV per-thread values, in every thread: lanes by butterflies, the waves' sums from LDS in wave order.
// `slot` alternates between the two sets of LDS words, so a set is rewritten only after a barrier that follows its last read.
template <int NV>
__device__ __forceinline__ void lk_sums(const float (&part)[NV], double (*s_red)[LK_WAVES][3], int& slot, int tid, double (&total)[NV]) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double s = wave_sum_f64((double)part[q]);
        if ((tid & 63) == 0) s_red[slot][tid >> 6][q] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) total[q] = ((s_red[slot][0][q] + s_red[slot][1][q]) + s_red[slot][2][q]) + s_red[slot][3][q];
    slot ^= 1;
}

// prev at window coordinate (fi - ey, fj - ex): source_sample's order of operations on the staged window.  fi, fj in [2, B - 1] and
// ey, ex in [-1, 1] keep the four taps inside rows and columns 1 ... B + 1 of the B + 2; the clamp maps a NaN to 0, also inside.
template <int B>
__device__ __forceinline__ float lk_sample(const float* s_win, float fi, float fj, float ey, float ex) {
    constexpr int WP = B + 2;
    const float sy = fminf(fmaxf(fi - ey, 0.f), (float)B), sx = fminf(fmaxf(fj - ex, 0.f), (float)B);
    const float fy0 = floorf(sy), fx0 = floorf(sx);
    const float fy = sy - fy0, fx = sx - fx0;
    const float* w = s_win + (int)fy0 * WP + (int)fx0;
    const float top = lerp_fma(w[0], w[1], fx);
    const float bot = lerp_fma(w[WP], w[WP + 1], fx);
    return lerp_fma(top, bot, fy);
}

// eig = (lambda_min, lambda_max) of G = [[gyy, gxy], [gxy, gxx]] and its determinant, float64 and uncontracted: the expressions of
// the specification, operation for operation
__device__ __forceinline__ void lk_eigen(double gyy, double gxy, double gxx, double& lmin, double& lmax, double& det) {
#pragma clang fp contract(off)
    const double tr = gyy + gxx;
    const double a = gyy * gxx, b = gxy * gxy;
    det = a - b;
    const double t2 = tr * tr, d4 = 4.0 * det;
    const double root = sqrt(fmax(t2 - d4, 0.0));
    lmin = 0.5 * (tr - root);
    lmax = 0.5 * (tr + root);
}

// delta = G^-1 b with b = -(sy, sx), the sums of g r
__device__ __forceinline__ void lk_solve(double gyy, double gxy, double gxx, double det, double sy, double sx, double& dy, double& dx) {
#pragma clang fp contract(off)
    const double by = -sy, bx = -sx;
    const double p0 = gxx * by, p1 = gxy * bx, p2 = gyy * bx, p3 = gxy * by;
    dy = (p0 - p1) / det;
    dx = (p2 - p3) / det;
}

template <int B>
__global__ __launch_bounds__(LK_THREADS) void lk_refine_kernel(LkGeom g, float* __restrict__ v, double* __restrict__ eig,
                                                               double* __restrict__ residual) {
    constexpr int M = B - 2, NI = M * M, K = (NI + LK_THREADS - 1) / LK_THREADS, WP = B + 2;
    __shared__ float s_next[B * B];
    __shared__ float s_win[WP * WP];
    __shared__ double s_red[2][LK_WAVES][3];
    __shared__ int s_head[3];  // not dry, d0y, d0x
    const int tid = threadIdx.x;
    const int per_plane = g.By * g.Bx;
    const int64_t id = blockIdx.x;
    const int64_t n = id / per_plane;
    const int b = (int)(id - n * per_plane);
    const int by = b / g.Bx, bx = b - by * g.Bx;
    const int y0 = by * g.stride, x0 = bx * g.stride;  // y0 + B <= H, x0 + B <= W
    if (tid == 0) {
        const float c0 = g.cost[id * 5];
        s_head[0] = c0 - c0 == 0.f ? 1 : 0;  // finite
        s_head[1] = g.disp[id * 2];
        s_head[2] = g.disp[id * 2 + 1];
    }
    __syncthreads();
    if (!s_head[0]) {  // dry (uniform over the workgroup): nothing is staged
        if (tid == 0) {
            v[id * 2] = 0.f;
            v[id * 2 + 1] = 0.f;
            eig[id * 2] = 0.0;
            eig[id * 2 + 1] = 0.0;
            residual[id] = (double)__builtin_inff();
        }
        return;
    }
    const int d0y = s_head[1], d0x = s_head[2];
    const float* nx = g.next + n * g.plane_stride + (int64_t)y0 * g.W + x0;
    for (int e = tid; e < B * B; e += LK_THREADS) {
        const int i = e / B, j = e - i * B;
        s_next[e] = present_or_zero(nx[(int64_t)i * g.W + j]);
    }
    const float* pv = g.prev + n * g.plane_stride;
    const int64_t wy0 = (int64_t)y0 - d0y - 1, wx0 = (int64_t)x0 - d0x - 1;  // 64-bit: any disp, whatever wrote it, only fails the test below
    for (int e = tid; e < WP * WP; e += LK_THREADS) {
        const int i = e / WP, j = e - i * WP;
        const int64_t y = wy0 + i, x = wx0 + j;
        s_win[e] = (y >= 0 && y < g.H && x >= 0 && x < g.W) ? present_or_zero(pv[y * g.W + x]) : 0.f;
    }
    __syncthreads();
    float q[K], gy[K], gx[K], fi[K], fj[K];
    float part3[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * LK_THREADS;
        q[k] = gy[k] = gx[k] = 0.f;
        fi[k] = fj[k] = 2.f;
        if (e < NI) {
            const int i = 1 + e / M, j = 1 + (e - (e / M) * M);
            const float* c = s_next + i * B + j;
            q[k] = c[0];
            gy[k] = 0.5f * (c[B] - c[-B]);
            gx[k] = 0.5f * (c[1] - c[-1]);
            fi[k] = (float)(i + 1);
            fj[k] = (float)(j + 1);
            part3[0] = fmaf(gy[k], gy[k], part3[0]);
            part3[1] = fmaf(gy[k], gx[k], part3[1]);
            part3[2] = fmaf(gx[k], gx[k], part3[2]);
        }
    }
    int slot = 0;
    double G[3];
    lk_sums<3>(part3, s_red, slot, tid, G);
    double lmin, lmax, det;
    lk_eigen(G[0], G[1], G[2], lmin, lmax, det);
    const bool conditioned = lmin > 0.0 && lmin >= (double)g.eig_ratio * lmax;  // the same bits in every thread
    const float fy0 = (float)d0y, fx0 = (float)d0x;
    float dy = fy0, dx = fx0;
    if (conditioned) {
        for (int it = 0; it < g.iterations; ++it) {
            const float ey = dy - fy0, ex = dx - fx0;  // in [-1, 1]
            float part2[2] = {0.f, 0.f};
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (tid + k * LK_THREADS < NI) {
                    const float r = q[k] - lk_sample<B>(s_win, fi[k], fj[k], ey, ex);
                    part2[0] = fmaf(gy[k], r, part2[0]);
                    part2[1] = fmaf(gx[k], r, part2[1]);
                }
            }
            double s[2], ddy, ddx;
            lk_sums<2>(part2, s_red, slot, tid, s);
            lk_solve(G[0], G[1], G[2], det, s[0], s[1], ddy, ddx);
            dy = fminf(fmaxf((float)((double)dy + ddy), fy0 - 1.f), fy0 + 1.f);
            dx = fminf(fmaxf((float)((double)dx + ddx), fx0 - 1.f), fx0 + 1.f);
        }
    }
    const float ey = dy - fy0, ex = dx - fx0;
    float part1[1] = {0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (tid + k * LK_THREADS < NI) {
            const float r = q[k] - lk_sample<B>(s_win, fi[k], fj[k], ey, ex);
            part1[0] = fmaf(r, r, part1[0]);
        }
    }
    double res[1];
    lk_sums<1>(part1, s_red, slot, tid, res);
    if (tid == 0) {
        v[id * 2] = dy;
        v[id * 2 + 1] = dx;
        eig[id * 2] = lmin;
        eig[id * 2 + 1] = lmax;
        residual[id] = res[0];
    }
}

}  // namespace

extern "C" int dgmr_lk_refine(const float* prev, const float* next, int64_t plane_stride, int64_t N, int H, int W, int block, int stride,
                              const int32_t* disp, const float* cost, int iterations, float eig_ratio, float* v, double* eig,
                              double* residual, void* stream) {
    const char* fn = "dgmr_lk_refine";
    DGMR_CHECK_ARG(prev && next && disp && cost && v && eig && residual, "%s: null pointer", fn);
    DGMR_CHECK_ARG(block == 16 || block == 32, "%s: block=%d, 16 and 32 are supported", fn, block);
    DGMR_CHECK_ARG(stride >= 1 && stride <= block, "%s: stride=%d must be 1 ... block=%d", fn, stride, block);
    DGMR_CHECK_ARG(iterations >= 1 && iterations <= LK_MAX_ITERATIONS, "%s: iterations=%d must be 1 ... %d", fn, iterations, LK_MAX_ITERATIONS);
    DGMR_CHECK_ARG(eig_ratio >= 0.f && eig_ratio <= 3.0e38f, "%s: eig_ratio=%g must be finite and not negative", fn, (double)eig_ratio);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H >= block && W >= block, "%s: H=%d and W=%d must be at least block=%d", fn, H, W, block);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(plane_stride >= 0 && plane_stride <= INT64_MAX / 4 / N, "%s: plane_stride=%lld out of range", fn, (long long)plane_stride);
    const int By = (H - block) / stride + 1, Bx = (W - block) / stride + 1;
    DGMR_CHECK_ARG(N * By * Bx <= (1ll << 30), "%s: %lld blocks are out of range", fn, (long long)(N * By * Bx));
    const LkGeom g{prev, next, disp, cost, plane_stride, H, W, stride, By, Bx, iterations, eig_ratio};
    const dim3 grid((unsigned)(N * By * Bx)), threads(LK_THREADS);
    if (block == 16)
        hipLaunchKernelGGL(lk_refine_kernel<16>, grid, threads, 0, ST, g, v, eig, residual);
    else
        hipLaunchKernelGGL(lk_refine_kernel<32>, grid, threads, 0, ST, g, v, eig, residual);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_block_match(const float* prev, const float* next, int64_t plane_stride, int64_t N, int H, int W, int block, int stride,
                                int radius, float wet_threshold, int min_wet, int32_t* disp, float* cost, int32_t* wet, void* stream) {
    const char* fn = "dgmr_block_match";
    DGMR_CHECK_ARG(prev && next && disp && cost && wet, "%s: null pointer", fn);
    DGMR_CHECK_ARG(block == 16 || block == 32, "%s: block=%d, 16 and 32 are supported", fn, block);
    DGMR_CHECK_ARG(stride >= 1 && stride <= block, "%s: stride=%d must be 1 ... block=%d", fn, stride, block);
    DGMR_CHECK_ARG(radius >= 1 && radius <= BM_MAX_R, "%s: radius=%d must be 1 ... %d", fn, radius, BM_MAX_R);
    DGMR_CHECK_ARG(min_wet >= 0, "%s: min_wet=%d must not be negative", fn, min_wet);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H >= block && W >= block, "%s: H=%d and W=%d must be at least block=%d", fn, H, W, block);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(plane_stride >= 0 && plane_stride <= INT64_MAX / 4 / N, "%s: plane_stride=%lld out of range", fn, (long long)plane_stride);
    const int By = (H - block) / stride + 1, Bx = (W - block) / stride + 1;
    DGMR_CHECK_ARG(N * By * Bx <= (1ll << 30), "%s: %lld blocks are out of range", fn, (long long)(N * By * Bx));
    const BmGeom g{prev, next, plane_stride, H, W, stride, radius, By, Bx, min_wet, wet_threshold};
    const int WP = block + 2 * radius, ND = (2 * radius + 1) * (2 * radius + 1);
    const int lds = (block * block + WP * WP + ND) * 4;  // <= 24.3 KiB
    const dim3 grid((unsigned)(N * By * Bx)), threads(bm_threads(radius));
    if (block == 16)
        hipLaunchKernelGGL(block_match_kernel<16>, grid, threads, lds, ST, g, disp, cost, wet);
    else
        hipLaunchKernelGGL(block_match_kernel<32>, grid, threads, lds, ST, g, disp, cost, wet);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_advect(const float* x, int64_t x_plane_stride, const float* field, int64_t field_plane_stride, int64_t N, int H, int W,
                           int Gy, int Gx, float origin, float spacing, int T, float* out, int64_t out_plane_stride, int64_t out_step_stride,
                           void* stream) {
    const char* fn = "dgmr_advect";
    DGMR_CHECK_ARG(x && field && out, "%s: null pointer", fn);
    DGMR_CHECK_ARG(T >= 1 && T <= 64, "%s: T=%d lead times, 1 ... 64 are supported", fn, T);
    DGMR_CHECK_ARG(spacing > 0.f && spacing <= 3.0e38f && origin == origin && origin >= -3.0e38f && origin <= 3.0e38f,
                   "%s: spacing=%g must be positive and finite, origin=%g finite", fn, (double)spacing, (double)origin);
    DGMR_CHECK_ARG(Gy >= 1 && Gx >= 1 && (int64_t)Gy * Gx <= (1 << 28), "%s: a lattice of %d x %d nodes is out of range", fn, Gy, Gx);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(x_plane_stride >= 0 && x_plane_stride <= INT64_MAX / 4 / N && field_plane_stride >= 0 &&
                       field_plane_stride <= INT64_MAX / 4 / N,
                   "%s: x_plane_stride=%lld or field_plane_stride=%lld out of range", fn, (long long)x_plane_stride,
                   (long long)field_plane_stride);
    DGMR_CHECK_ARG(out_plane_stride >= 0 && out_plane_stride <= INT64_MAX / 4 / N && (T == 1 || out_step_stride >= (int64_t)H * W) &&
                       out_step_stride >= 0 && out_step_stride <= INT64_MAX / 4 / 64,
                   "%s: out_plane_stride=%lld out of range or out_step_stride=%lld below H * W", fn, (long long)out_plane_stride,
                   (long long)out_step_stride);
    const bool wide = W % 4 == 0 && ((uintptr_t)out & 15) == 0 && out_plane_stride % 4 == 0 && out_step_stride % 4 == 0;
    const int V = wide ? 4 : 1;
    const int64_t items = N * H * (W / V);
    DGMR_CHECK_ARG(items <= (1ll << 38), "%s: %lld pixels are out of range", fn, (long long)(N * H * W));
    const AdvGeom g{x, field, out, x_plane_stride, field_plane_stride, out_plane_stride, out_step_stride, items, H, W, Gy, Gx, T, origin, spacing,
                    0, 1, nullptr, nullptr, 0};
    const dim3 grid((unsigned)((items + 255) / 256)), threads(256);
    if (wide)
        hipLaunchKernelGGL((advect_kernel<4, false>), grid, threads, 0, ST, g);
    else
        hipLaunchKernelGGL((advect_kernel<1, false>), grid, threads, 0, ST, g);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_advect_series(const float* x, int64_t x_plane_stride, int64_t x_step_stride, const float* field, int64_t field_plane_stride,
                                  int field_group, int64_t N, int H, int W, int Gy, int Gx, float origin, float spacing, int T, float* out,
                                  int64_t out_plane_stride, int64_t out_step_stride, void* stream) {
    const char* fn = "dgmr_advect_series";
    DGMR_CHECK_ARG(x && field && out, "%s: null pointer", fn);
    DGMR_CHECK_ARG(T >= 1 && T <= 64, "%s: T=%d lead times, 1 ... 64 are supported", fn, T);
    DGMR_CHECK_ARG(spacing > 0.f && spacing <= 3.0e38f && origin == origin && origin >= -3.0e38f && origin <= 3.0e38f,
                   "%s: spacing=%g must be positive and finite, origin=%g finite", fn, (double)spacing, (double)origin);
    DGMR_CHECK_ARG(Gy >= 1 && Gx >= 1 && (int64_t)Gy * Gx <= (1 << 28), "%s: a lattice of %d x %d nodes is out of range", fn, Gy, Gx);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(field_group >= 1, "%s: field_group=%d must be at least 1", fn, field_group);
    DGMR_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(x_plane_stride >= 0 && x_plane_stride <= INT64_MAX / 4 / N && field_plane_stride >= 0 &&
                       field_plane_stride <= INT64_MAX / 4 / N && x_step_stride >= 0 && x_step_stride <= INT64_MAX / 4 / 64,
                   "%s: x_plane_stride=%lld, x_step_stride=%lld or field_plane_stride=%lld out of range", fn, (long long)x_plane_stride,
                   (long long)x_step_stride, (long long)field_plane_stride);
    DGMR_CHECK_ARG(out_plane_stride >= 0 && out_plane_stride <= INT64_MAX / 4 / N && (T == 1 || out_step_stride >= (int64_t)H * W) &&
                       out_step_stride >= 0 && out_step_stride <= INT64_MAX / 4 / 64,
                   "%s: out_plane_stride=%lld out of range or out_step_stride=%lld below H * W", fn, (long long)out_plane_stride,
                   (long long)out_step_stride);
    const bool wide = W % 4 == 0 && ((uintptr_t)out & 15) == 0 && out_plane_stride % 4 == 0 && out_step_stride % 4 == 0;
    const int V = wide ? 4 : 1;
    const int64_t items = N * H * (W / V);
    DGMR_CHECK_ARG(items <= (1ll << 38), "%s: %lld pixels are out of range", fn, (long long)(N * H * W));
    const AdvGeom g{x, field, out, x_plane_stride, field_plane_stride, out_plane_stride, out_step_stride, items, H, W, Gy, Gx, T, origin, spacing,
                    x_step_stride, field_group, nullptr, nullptr, 0};
    const dim3 grid((unsigned)((items + 255) / 256)), threads(256);
    if (wide)
        hipLaunchKernelGGL((advect_kernel<4, true>), grid, threads, 0, ST, g);
    else
        hipLaunchKernelGGL((advect_kernel<1, true>), grid, threads, 0, ST, g);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_advect_series_perturbed(const float* x, int64_t x_plane_stride, int64_t x_step_stride, const float* field,
                                            int64_t field_plane_stride, const float* direction, int64_t direction_plane_stride,
                                            const float* amplitude, int field_group, int64_t N, int H, int W, int Gy, int Gx, float origin,
                                            float spacing, int T, float* out, int64_t out_plane_stride, int64_t out_step_stride, void* stream) {
    const char* fn = "dgmr_advect_series_perturbed";
    DGMR_CHECK_ARG(x && field && out, "%s: null pointer", fn);
    DGMR_CHECK_ARG(direction && amplitude, "%s: null direction or amplitude", fn);
    DGMR_CHECK_ARG(T >= 1 && T <= 64, "%s: T=%d lead times, 1 ... 64 are supported", fn, T);
    DGMR_CHECK_ARG(spacing > 0.f && spacing <= 3.0e38f && origin == origin && origin >= -3.0e38f && origin <= 3.0e38f,
                   "%s: spacing=%g must be positive and finite, origin=%g finite", fn, (double)spacing, (double)origin);
    DGMR_CHECK_ARG(Gy >= 1 && Gx >= 1 && (int64_t)Gy * Gx <= (1 << 28), "%s: a lattice of %d x %d nodes is out of range", fn, Gy, Gx);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(field_group >= 1, "%s: field_group=%d must be at least 1", fn, field_group);
    DGMR_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(x_plane_stride >= 0 && x_plane_stride <= INT64_MAX / 4 / N && field_plane_stride >= 0 &&
                       field_plane_stride <= INT64_MAX / 4 / N && x_step_stride >= 0 && x_step_stride <= INT64_MAX / 4 / 64,
                   "%s: x_plane_stride=%lld, x_step_stride=%lld or field_plane_stride=%lld out of range", fn, (long long)x_plane_stride,
                   (long long)x_step_stride, (long long)field_plane_stride);
    DGMR_CHECK_ARG(direction_plane_stride >= 0 && direction_plane_stride <= INT64_MAX / 4 / N, "%s: direction_plane_stride=%lld out of range",
                   fn, (long long)direction_plane_stride);
    DGMR_CHECK_ARG(out_plane_stride >= 0 && out_plane_stride <= INT64_MAX / 4 / N && (T == 1 || out_step_stride >= (int64_t)H * W) &&
                       out_step_stride >= 0 && out_step_stride <= INT64_MAX / 4 / 64,
                   "%s: out_plane_stride=%lld out of range or out_step_stride=%lld below H * W", fn, (long long)out_plane_stride,
                   (long long)out_step_stride);
    const bool wide = W % 4 == 0 && ((uintptr_t)out & 15) == 0 && out_plane_stride % 4 == 0 && out_step_stride % 4 == 0;
    const int V = wide ? 4 : 1;
    const int64_t items = N * H * (W / V);
    DGMR_CHECK_ARG(items <= (1ll << 38), "%s: %lld pixels are out of range", fn, (long long)(N * H * W));
    const AdvGeom g{x, field, out, x_plane_stride, field_plane_stride, out_plane_stride, out_step_stride, items, H, W, Gy, Gx, T, origin, spacing,
                    x_step_stride, field_group, direction, amplitude, direction_plane_stride};
    const dim3 grid((unsigned)((items + 255) / 256)), threads(256);
    if (wide)
        hipLaunchKernelGGL((advect_kernel<4, true, true>), grid, threads, 0, ST, g);
    else
        hipLaunchKernelGGL((advect_kernel<1, true, true>), grid, threads, 0, ST, g);
    DGMR_CHECK_LAUNCH();
    return 0;
}
