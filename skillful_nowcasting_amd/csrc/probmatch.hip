// Probability matching of the stochastic ensemble's dB fields (stochastic.py: dgmr_probability_match): every (case, member, lead time)
// plane is mapped through its own binned ranks onto the sorted values of the case's last observed frame.  The map is monotone, so no
// sort of the plane is needed: a 4096-bin integer histogram and two streaming passes give it.
//
//   clear    hipMemsetAsync of the workspace, [P M T][2][4096] int32 and one flag per case
//   flags    one workgroup per (case, chunk) of the target: does it hold a -0.0 or a NaN?  (see scan)
//   hist     one workgroup per (plane, chunk of 32768 elements): bins into a 16 KiB LDS histogram, then adds its NONZERO bins to row 0
//            of the plane's table with integer atomics - order-independent, two calls give the same bits
//   scan     one workgroup per plane: the exclusive prefix c[] of the plane's 4096 counts (thread t sums bins 16 t ... 16 t + 15, a
//            wave scan by shuffles, the four waves' totals through LDS) and, per occupied bin, the first and the last target value of
//            its span of ranks.  Row 0 becomes c[b], row 1 h[b] - or, where the two values have the same bits, row 0 gets its sign
//            bit set and row 1 holds the VALUE: every rank of the bin reads the same number, so no element of it needs the target.
//            (Equal ends of a sorted span make all of it equal in VALUE; the bits could still differ between -0.0 and 0.0 or between
//            NaNs, so a case whose target holds either - its flag - keeps the gather for every bin.)
//   apply    one workgroup per (plane, chunk): both rows into LDS (32 KiB), then its chunk again:
//            r = c[b] + min(int(f h[b]), h[b] - 1), out = target_sorted[r], or the bin's value.  An element is read and written by
//            the same lane, so out may be z.
//
// The gather is what the call costs: neighbouring pixels carry independent noise, so the 64 lanes of a load ask for 64 different
// cache lines of a sorted plane that no L1 holds, and each 4-byte value arrives as a whole line (measured, 8 x 18 planes of
// 1536 x 1280 with every element gathered: hist 0.32 ms, apply 2.7 ms).  A radar frame is mostly ONE value - 60 to 75 % exact zeros -
// and every bin whose ranks fall inside that run is constant: its elements skip the gather.
//
// The same skew is a hazard for the histogram.  Entirely dry windows come out of dgmr_spectral_ar as exact 0.0, and every masked-out
// element is put into bin 0.  LDS atomics of a wave onto one address serialise, so these two bins never go through them: their
// elements are counted per wave with a ballot and a population count (a scalar, wave-uniform counter) and added once per wave at the
// end.  Of the other elements, those that share the bin of the wave's first such lane (runs of any other constant: a clamped top
// bin, a flat field) are added by that lane alone; the rest - continuous values, few collisions - take one LDS atomic each.
//
// The bin arithmetic is the reference's, operation for operation: u = (z - lo) * scale as two separately rounded fp32 operations
// (__fsub_rn / __fmul_rn: no contraction into an fma), b = int(u) for 0 <= u < 4096, f = u - b (exact), int(f * float(h[b])).
// 16-byte loads and stores (4-byte loads of the mask) when every pointer and stride allows them, 4-byte (1-byte) ones otherwise.
#include "common.h"

namespace {

constexpr int PM_BINS = 4096, PM_THREADS = 256, PM_CHUNK = 32768, PM_PER_THREAD = PM_BINS / PM_THREADS;

struct PmGeom {
    const float* z;
    const float* target;
    const uint8_t* mask;
    float* out;
    int32_t* hist;
    int64_t z_member_stride, z_step_stride, target_stride, mask_plane_stride, mask_step_stride, out_member_stride, out_step_stride;
    int M, T, N, chunks;
    float lo, scale;
    int32_t* flags;  // [P], behind the tables
};

// -> the bin of z and, in f, its position within the bin (0 at the two clamps and for an element the mask rules out)
__device__ __forceinline__ int pm_bin(float z, float lo, float scale, bool allowed, float& f) {
    const float u = __fmul_rn(__fsub_rn(z, lo), scale);
    f = 0.f;
    if (!allowed || !(u >= 0.f)) return 0;  // below the range, NaN, masked out
    if (u >= (float)PM_BINS) return PM_BINS - 1;
    const int b = (int)u;
    f = __fsub_rn(u, (float)b);
    return b;
}

// elements i ... i + V - 1 of a plane and whether the mask allows them (no mask: all)
template <int V>
__device__ __forceinline__ void pm_load(const float* __restrict__ zp, const uint8_t* __restrict__ mp, int i, float (&v)[V], bool (&ok)[V]) {
    if constexpr (V == 4) {
        const f32x4 q = *(const f32x4*)(zp + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        const uint32_t m = mp ? *(const uint32_t*)(mp + i) : 0xffffffffu;
#pragma unroll
        for (int k = 0; k < 4; ++k) ok[k] = ((m >> (8 * k)) & 0xffu) != 0;
    } else {
        v[0] = zp[i];
        ok[0] = mp ? mp[i] != 0 : true;
    }
}

struct PmPlane {
    const float* z;
    const uint8_t* mask;
    const float* target;
    float* out;
    int64_t plane;
    int base, end;
};

__device__ __forceinline__ PmPlane pm_plane(const PmGeom& g) {
    const int64_t id = blockIdx.x;
    const int64_t plane = id / g.chunks;  // (p M + m) T + t
    const int chunk = (int)(id - plane * g.chunks);
    const int64_t pm = plane / g.T;
    const int t = (int)(plane - pm * g.T);
    const int64_t p = pm / g.M;
    PmPlane r;
    r.z = g.z + pm * g.z_member_stride + t * g.z_step_stride;
    r.mask = g.mask ? g.mask + p * g.mask_plane_stride + t * g.mask_step_stride : nullptr;
    r.target = g.target + p * g.target_stride;
    r.out = g.out + pm * g.out_member_stride + t * g.out_step_stride;
    r.plane = plane;
    r.base = chunk * PM_CHUNK;  // chunks = ceil(N / PM_CHUNK): base < N <= 2^24
    r.end = min(r.base + PM_CHUNK, g.N);
    return r;
}

template <int V>
__global__ __launch_bounds__(PM_THREADS) void pm_hist_kernel(PmGeom g) {
    __shared__ int s_h[PM_BINS];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < PM_BINS; i += PM_THREADS) s_h[i] = 0;
    __syncthreads();
    const PmPlane pl = pm_plane(g);
    float f;
    const int zero_bin = pm_bin(0.f, g.lo, g.scale, true, f);  // where exact zeros go (bin 0 itself when lo >= 0)
    int n_first = 0, n_zero = 0;                               // wave-uniform: this wave's elements of bin 0 and of zero_bin
    for (int i0 = pl.base; i0 < pl.end; i0 += PM_THREADS * V) {  // (the same trips for every lane: the ballots below see whole waves)
        const int i = i0 + tid * V;
        const bool valid = i < pl.end;  // N % V == 0 on the 16-byte path, so a valid lane holds V elements
        float v[V];
        bool ok[V];
        if (valid) pm_load<V>(pl.z, pl.mask, i, v, ok);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int b = valid ? pm_bin(v[k], g.lo, g.scale, ok[k], f) : -1;
            n_first += __popcll(__ballot(b == 0));
            n_zero += __popcll(__ballot(b == zero_bin && zero_bin != 0));
            const bool rest = b > 0 && b != zero_bin;
            const unsigned long long m = __ballot(rest);
            if (m == 0) continue;  // (wave-uniform)
            const int leader = __ffsll((long long)m) - 1;
            const int lead_bin = __shfl(b, leader, 64);
            const unsigned long long same = __ballot(rest && b == lead_bin);
            if (rest) {
                if (b != lead_bin)
                    atomicAdd(&s_h[b], 1);
                else if (lane == leader)
                    atomicAdd(&s_h[b], __popcll(same));
            }
        }
    }
    if (lane == 0) {
        if (n_first) atomicAdd(&s_h[0], n_first);
        if (n_zero) atomicAdd(&s_h[zero_bin], n_zero);
    }
    __syncthreads();
    int32_t* __restrict__ row = g.hist + pl.plane * (2 * PM_BINS);
    for (int i = tid; i < PM_BINS; i += PM_THREADS) {
        const int c = s_h[i];
        if (c) atomicAdd(&row[i], c);
    }
}

// flags[p] = 1 when case p's target holds a -0.0 or a NaN
__global__ __launch_bounds__(PM_THREADS) void pm_flag_kernel(PmGeom g) {
    const int64_t p = blockIdx.x / g.chunks;
    const int base = (int)(blockIdx.x - p * g.chunks) * PM_CHUNK, end = min(base + PM_CHUNK, g.N);
    const float* __restrict__ target = g.target + p * g.target_stride;
    bool odd = false;
    for (int i = base + threadIdx.x; i < end; i += PM_THREADS) {
        const int bits = __float_as_int(target[i]);
        odd |= bits == INT32_MIN || (bits & INT32_MAX) > 0x7f800000;
    }
    if (odd) atomicOr(&g.flags[p], 1);
}

// one workgroup per plane: row 0 of its table from counts to exclusive prefixes, row 1 the counts - or the bin's one value (see above)
__global__ __launch_bounds__(PM_THREADS) void pm_scan_kernel(PmGeom g) {
    __shared__ int s_wave[PM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t plane = blockIdx.x;
    const int64_t p = plane / g.T / g.M;
    const float* __restrict__ target = g.target + p * g.target_stride;
    const bool bits_follow_values = g.flags[p] == 0;
    int4* __restrict__ row = (int4*)(g.hist + plane * (2 * PM_BINS) + tid * PM_PER_THREAD);
    int h[PM_PER_THREAD], c[PM_PER_THREAD];
#pragma unroll
    for (int j = 0; j < PM_PER_THREAD / 4; ++j) {
        const int4 q = row[j];
        h[4 * j] = q.x, h[4 * j + 1] = q.y, h[4 * j + 2] = q.z, h[4 * j + 3] = q.w;
    }
    int mine = 0;
#pragma unroll
    for (int j = 0; j < PM_PER_THREAD; ++j) {
        c[j] = mine;
        mine += h[j];
    }
    int upto = mine;  // inclusive over the wave's lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(upto, o, 64);
        if (lane >= o) upto += y;
    }
    if (lane == 63) s_wave[wave] = upto;
    __syncthreads();
    int before = upto - mine;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
#pragma unroll
    for (int j = 0; j < PM_PER_THREAD; ++j) {
        c[j] += before;
        // the counts of a plane sum to N, so an occupied bin's span [c, c + h - 1] lies inside the target; the clamps hold whatever the
        // table held
        if (h[j] > 0 && bits_follow_values) {
            const int first = min(max(c[j], 0), g.N - 1), last = min(max(c[j] + h[j] - 1, 0), g.N - 1);
            const int lo_bits = __float_as_int(target[first]), hi_bits = __float_as_int(target[last]);
            if (lo_bits == hi_bits) c[j] |= INT32_MIN, h[j] = lo_bits;
        }
    }
#pragma unroll
    for (int j = 0; j < PM_PER_THREAD / 4; ++j) {
        row[j] = make_int4(c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3]);
        row[PM_BINS / 4 + j] = make_int4(h[4 * j], h[4 * j + 1], h[4 * j + 2], h[4 * j + 3]);
    }
}

template <int V>
__global__ __launch_bounds__(PM_THREADS) void pm_apply_kernel(PmGeom g) {
    __shared__ __attribute__((aligned(16))) int s_c[PM_BINS];  // c[b]; negative: every rank of the bin reads one value
    __shared__ __attribute__((aligned(16))) int s_h[PM_BINS];  // h[b], or that value's bits
    const int tid = threadIdx.x;
    const PmPlane pl = pm_plane(g);
    {
        const int4* __restrict__ table = (const int4*)(g.hist + pl.plane * (2 * PM_BINS));
        for (int i = tid; i < PM_BINS / 4; i += PM_THREADS) {
            ((int4*)s_c)[i] = table[i];
            ((int4*)s_h)[i] = table[PM_BINS / 4 + i];
        }
        __syncthreads();
    }
    for (int i0 = pl.base; i0 < pl.end; i0 += PM_THREADS * V) {
        const int i = i0 + tid * V;
        if (i >= pl.end) continue;
        float v[V], r[V];
        bool ok[V];
        pm_load<V>(pl.z, pl.mask, i, v, ok);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float f;
            const int b = pm_bin(v[k], g.lo, g.scale, ok[k], f);
            r[k] = 0.f;
            if (ok[k]) {
                const int cb = s_c[b], hb = s_h[b];
                if (cb < 0) {
                    r[k] = __int_as_float(hb);
                } else {  // hb >= 1: this element was counted
                    int rank = cb + min((int)__fmul_rn(f, (float)hb), hb - 1);
                    rank = min(max(rank, 0), g.N - 1);  // true of a histogram of this plane; keeps the gather inside the target whatever the table holds
                    r[k] = pl.target[rank];
                }
            }
        }
        if constexpr (V == 4) {
            f32x4 q;
            q.x = r[0], q.y = r[1], q.z = r[2], q.w = r[3];
            *(f32x4*)(pl.out + i) = q;
        } else {
            pl.out[i] = r[0];
        }
    }
}

constexpr int64_t PM_MAX_PLANES = 1 << 20;

inline int64_t pm_planes(int P, int M, int T) {
    if (P < 1 || M < 1 || T < 1 || T > 64) return -1;
    const int64_t n = (int64_t)P * M * T;
    return n <= PM_MAX_PLANES ? n : -1;
}

// the tables, then a flag per case, rounded up to 16 bytes
inline int64_t pm_bytes(int64_t planes, int P) { return planes * 2 * PM_BINS * (int64_t)sizeof(int32_t) + ((int64_t)P * 4 + 15) / 16 * 16; }

}  // namespace

extern "C" int64_t dgmr_probability_match_workspace(int P, int M, int T) {
    const int64_t n = pm_planes(P, M, T);
    return n < 0 ? -1 : pm_bytes(n, P);
}

extern "C" int dgmr_probability_match(const float* z, int64_t member_stride, int64_t step_stride, const float* target_sorted,
                                      int64_t target_stride, const uint8_t* mask, int64_t mask_plane_stride, int64_t mask_step_stride, int P,
                                      int M, int T, int H, int W, float lo, float scale, void* workspace, int64_t workspace_bytes, float* out,
                                      int64_t out_member_stride, int64_t out_step_stride, void* stream) {
    const char* fn = "dgmr_probability_match";
    DGMR_CHECK_ARG(z && target_sorted && workspace && out, "%s: null pointer", fn);
    DGMR_CHECK_ARG(T >= 1 && T <= 64, "%s: T=%d lead times, 1 ... 64 are supported", fn, T);
    const int64_t planes = pm_planes(P, M, T);
    DGMR_CHECK_ARG(planes > 0, "%s: P=%d cases and M=%d members: at least one each, at most %lld planes in all", fn, P, M,
                   (long long)PM_MAX_PLANES);
    int exponent = 0;
    DGMR_CHECK_ARG(scale > 0.f && scale <= 3.0e38f && frexpf(scale, &exponent) == 0.5f, "%s: scale=%g must be a power of two", fn, (double)scale);
    DGMR_CHECK_ARG(lo == lo && lo >= -3.0e38f && lo <= 3.0e38f, "%s: lo=%g must be finite", fn, (double)lo);
    DGMR_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24), "%s: a plane of %d x %d elements: H * W must be 1 ... 2^24", fn, H, W);
    const int64_t N = (int64_t)H * W, top = INT64_MAX / 4 / PM_MAX_PLANES;
    DGMR_CHECK_ARG(member_stride >= N && step_stride >= N && member_stride <= top && step_stride <= top,
                   "%s: member_stride=%lld or step_stride=%lld below H * W or out of range", fn, (long long)member_stride, (long long)step_stride);
    DGMR_CHECK_ARG(out_member_stride >= N && out_step_stride >= N && out_member_stride <= top && out_step_stride <= top,
                   "%s: out_member_stride=%lld or out_step_stride=%lld below H * W or out of range", fn, (long long)out_member_stride,
                   (long long)out_step_stride);
    DGMR_CHECK_ARG(target_stride >= N && target_stride <= top, "%s: target_stride=%lld below H * W or out of range", fn, (long long)target_stride);
    DGMR_CHECK_ARG(!mask || (mask_plane_stride >= N && mask_plane_stride <= top && (mask_step_stride == 0 || mask_step_stride >= N) &&
                             mask_step_stride <= top),
                   "%s: mask_plane_stride=%lld below H * W, or mask_step_stride=%lld neither 0 nor at least H * W", fn,
                   (long long)mask_plane_stride, (long long)mask_step_stride);
    const int64_t need = pm_bytes(planes, P);
    DGMR_CHECK_ARG(workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, "%s: the workspace holds %lld bytes, %lld are needed (16-byte aligned)",
                   fn, (long long)workspace_bytes, (long long)need);
    const int chunks = cdiv(N, PM_CHUNK);  // <= 512
    const bool wide = N % 4 == 0 && (((uintptr_t)z | (uintptr_t)out) & 15) == 0 && member_stride % 4 == 0 && step_stride % 4 == 0 &&
                      out_member_stride % 4 == 0 && out_step_stride % 4 == 0 &&
                      (!mask || (((uintptr_t)mask & 3) == 0 && mask_plane_stride % 4 == 0 && mask_step_stride % 4 == 0));
    const PmGeom g{z, target_sorted, mask, out, (int32_t*)workspace, member_stride, step_stride, target_stride, mask ? mask_plane_stride : 0,
                   mask ? mask_step_stride : 0, out_member_stride, out_step_stride, M, T, (int)N, chunks, lo, scale,
                   (int32_t*)workspace + planes * 2 * PM_BINS};
    if (hipMemsetAsync(workspace, 0, (size_t)need, ST) != hipSuccess) {
        dgmr_set_error("%s: clearing the workspace failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    const dim3 grid((unsigned)(planes * chunks)), threads(PM_THREADS);  // <= 2^29 workgroups
    hipLaunchKernelGGL(pm_flag_kernel, dim3((unsigned)(P * chunks)), threads, 0, ST, g);
    if (wide) {
        hipLaunchKernelGGL(pm_hist_kernel<4>, grid, threads, 0, ST, g);
        hipLaunchKernelGGL(pm_scan_kernel, dim3((unsigned)planes), threads, 0, ST, g);
        hipLaunchKernelGGL(pm_apply_kernel<4>, grid, threads, 0, ST, g);
    } else {
        hipLaunchKernelGGL(pm_hist_kernel<1>, grid, threads, 0, ST, g);
        hipLaunchKernelGGL(pm_scan_kernel, dim3((unsigned)planes), threads, 0, ST, g);
        hipLaunchKernelGGL(pm_apply_kernel<1>, grid, threads, 0, ST, g);
    }
    DGMR_CHECK_LAUNCH();
    return 0;
}
