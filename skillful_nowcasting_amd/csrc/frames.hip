// Full-frame radar in and out, for gfx950: the importance-crop sampler and the tile blend of full-frame nowcasts.  They share CROP_WAVES
// and the mapping of rows to waves.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// importance-sampled crops from full frames (data.py: ImportanceCropLoader)
// ------------------------------------------------------------------------------------------------
// Storage element -> fp32, exactly (every uint8 / int16 / float16 value is an fp32 value).
__device__ __forceinline__ float crop_raw(const uint8_t* p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ float crop_raw(const int16_t* p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ float crop_raw(const _Float16* p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ float crop_raw(const float* p, int64_t i) { return p[i]; }
// The physical value: two separately rounded fp32 operations (torch's raw.float() * scale + offset), never one fma.
__device__ __forceinline__ float crop_phys(float raw, float scale, float offset) { return __fadd_rn(__fmul_rn(raw, scale), offset); }

constexpr int CROP_WAVES = 4;   // waves per workgroup of crop_cell_sums_kernel and of crop_gather_kernel
constexpr int CROP_UNROLL = 4;  // loads a lane of crop_cell_sums_kernel issues before it consumes the first

// Pass 1.  A frame row is W * C contiguous elements and cell cx owns the run [cx * cw, (cx + 1) * cw) of it, cw = cell * C.  A workgroup
// takes the band of `cell` image rows blockIdx.y and `cpb` whole cells of it (cpb = max(1, 64 / cw)): lane l reads the elements l,
// l + 64, ... of that run, so a wave load is one contiguous run, and wave w takes the (frame, band row) pairs w, w + 4, ...  Every
// element a lane meets lies in one cell, so its running sum is a partial of that cell: the four waves' partials meet in LDS in wave
// order, then the lanes of a cell in a xor butterfly (cw a power of two, or a cell wider than a wave) or one after the other.  The
// order is a function of indices alone.  Nothing right of the last whole cell or below the last whole band is read.
template <class T>
__global__ __launch_bounds__(64 * CROP_WAVES) void crop_cell_sums_kernel(const T* __restrict__ frames, int Tn, int H, int W, int C,
                                                                       float scale, float offset, double sat_scale, int cell, int cpb,
                                                                       int CW, double* __restrict__ cell_sums,
                                                                       int32_t* __restrict__ cell_missing) {
    __shared__ double s_sum[CROP_WAVES][64];
    __shared__ int32_t s_mis[CROP_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cw = cell * C;
    const int cx0 = blockIdx.x * cpb;
    const int ncell = min(cpb, CW - cx0);  // >= 1 by the grid
    const int span = ncell * cw;           // elements of a row this workgroup reads
    const int64_t row_elems = (int64_t)W * C;
    const int64_t col0 = (int64_t)cx0 * cw;
    const int y0 = blockIdx.y * cell;
    double sum = 0.0;
    int32_t mis = 0;
    // work items of a lane: (frame, band row, 64-element chunk of the run); CROP_UNROLL loads are issued before the first is consumed
    const int nchunk = (span + 63) >> 6, items = Tn * cell * nchunk;
    for (int it0 = wave; it0 < items; it0 += CROP_UNROLL * CROP_WAVES) {
        float raw[CROP_UNROLL];
        bool ok[CROP_UNROLL];
#pragma unroll
        for (int u = 0; u < CROP_UNROLL; ++u) {
            const int it = it0 + u * CROP_WAVES;
            const int pr = it / nchunk, e = (it - pr * nchunk) * 64 + lane;
            const int t = pr / cell, r = pr - t * cell;
            ok[u] = it < items && e < span;
            raw[u] = ok[u] ? crop_raw(frames, ((int64_t)t * H + (y0 + r)) * row_elems + col0 + e) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CROP_UNROLL; ++u) {
            if (!ok[u]) continue;
            const float x = crop_phys(raw[u], scale, offset);
            if (!(x >= 0.f))
                ++mis;
            else if (x > 0.f)  // (a dry element's term is exactly 0: most of a radar frame skips the exponential)
                sum += -expm1(-(double)x / sat_scale);
        }
    }
    s_sum[wave][lane] = sum;
    s_mis[wave][lane] = mis;
    __syncthreads();
    const int lw = cw < 64 ? cw : 64;  // lanes per cell (lanes past the run hold zeros)
    const bool pow2 = (lw & (lw - 1)) == 0;
    if (wave == 0) {
        sum = s_sum[0][lane];
        mis = s_mis[0][lane];
#pragma unroll
        for (int w = 1; w < CROP_WAVES; ++w) {  // in wave order
            sum += s_sum[w][lane];
            mis += s_mis[w][lane];
        }
        if (pow2) {
            for (int o = lw >> 1; o > 0; o >>= 1) {
                sum += __shfl_xor(sum, o, 64);
                mis += __shfl_xor(mis, o, 64);
            }
            if (lane % lw == 0 && lane / lw < ncell) {
                const int64_t ci = (int64_t)blockIdx.y * CW + cx0 + lane / lw;
                cell_sums[ci] = sum;
                cell_missing[ci] = mis;
            }
        } else {
            s_sum[0][lane] = sum;
            s_mis[0][lane] = mis;
        }
    }
    if (pow2) return;  // (the same in every thread of the launch)
    __syncthreads();
    if (wave == 0 && lane < ncell) {
        double s = 0.0;
        int32_t m = 0;
        for (int k = 0; k < lw; ++k) {
            s += s_sum[0][lane * lw + k];
            m += s_mis[0][lane * lw + k];
        }
        const int64_t ci = (int64_t)blockIdx.y * CW + cx0 + lane;
        cell_sums[ci] = s;
        cell_missing[ci] = m;
    }
}

// Pass 2: candidate (gy, gx) is the k x k block of cells with top-left cell (gy, gx), added in raster order by one thread.
__global__ void crop_box_sums_kernel(const double* __restrict__ cell_sums, const int32_t* __restrict__ cell_missing, int CW, int k,
                                     int Gy, int Gx, double* __restrict__ scores, int32_t* __restrict__ missing) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= Gy * Gx) return;
    const int gy = g / Gx, gx = g - gy * Gx;
    double s = 0.0;
    int32_t m = 0;
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) {
            const int64_t ci = (int64_t)(gy + a) * CW + gx + b;
            s += cell_sums[ci];
            m += cell_missing[ci];
        }
    scores[g] = s;
    missing[g] = m;
}

// One wave per output row (n, t, c, i), lanes along j: for C == 1 a wave instruction reads one contiguous run of the frame and
// writes 256 contiguous bytes of `out`.  Every load is guarded against the frame's extent, whatever the origin.
template <class T>
__global__ __launch_bounds__(64 * CROP_WAVES) void crop_gather_kernel(const T* __restrict__ frames, int Tn, int H, int W, int C,
                                                          const int32_t* __restrict__ origins, int64_t rows, int crop, float scale,
                                                          float offset, int clamp_missing, float missing_fill, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * CROP_WAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * CROP_WAVES;
    for (int64_t row = wave0; row < rows; row += nwaves) {
        const int i = (int)(row % crop);
        int64_t q = row / crop;
        const int c = (int)(q % C);
        q /= C;
        const int t = (int)(q % Tn);
        const int n = (int)(q / Tn);
        const int64_t y = (int64_t)origins[2 * n] + i, x0 = origins[2 * n + 1];
        const bool row_in = y >= 0 && y < H;
        const int64_t base = (((int64_t)t * H + y) * W + x0) * C + c;
        float* __restrict__ o = out + row * crop;
        for (int j = lane; j < crop; j += 64) {
            float v = missing_fill;
            if (row_in && x0 + j >= 0 && x0 + j < W) {
                v = crop_phys(crop_raw(frames, base + (int64_t)j * C), scale, offset);
                if (clamp_missing && !(v >= 0.f)) v = missing_fill;
            }
            o[j] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// tiled full-frame nowcasts (tiling.py: nowcast_tiled): one tile's forecast blended into the frame
// ------------------------------------------------------------------------------------------------
// Rows to waves like crop_gather_kernel, lanes along j in 16-byte pieces: a tile row is q = tile / 4 pieces and takes lpr = min(q, 64)
// lanes, so a wave instruction covers 64 / lpr whole rows (one 1 KiB row of a 256-pixel tile; eight rows of a 32-pixel one) and every
// row segment of `pred` and of `out` is read, and `out` written, as contiguous 16-byte pieces.  A lane's column never changes from
// row to row: its piece of wx is loaded once per wave (tiles wider than 256 pixels reload the further pieces), wy[i] once per row.
// pred is read once, the covered part of out read and written once; nothing else is touched.
__global__ __launch_bounds__(64 * CROP_WAVES) void tile_blend_kernel(const f32x4* __restrict__ pred, float* __restrict__ out,
                                                                     const float* __restrict__ wy, const f32x4* __restrict__ wx,
                                                                     int rows, int tile, int H, int W, int oy, int ox) {
    const int lane = threadIdx.x & 63;
    const int q = tile >> 2, lpr = q < 64 ? q : 64, rpw = 64 / lpr;
    const int sub = lane / lpr, jl = lane - sub * lpr;
    if (sub >= rpw) return;  // (q does not divide 64: the last lanes of a wave have no row)
    const int64_t step = (int64_t)gridDim.x * CROP_WAVES * rpw;
    const f32x4 wx0 = wx[jl];
    for (int64_t row64 = (int64_t)(blockIdx.x * CROP_WAVES + (threadIdx.x >> 6)) * rpw + sub; row64 < rows; row64 += step) {
        const int row = (int)row64, p = row / tile, i = row - p * tile;
        const float wyi = wy[i];
        const f32x4* __restrict__ src = pred + (int64_t)row * q;
        f32x4* __restrict__ dst = (f32x4*)(out + ((int64_t)p * H + oy + i) * W + ox);
        f32x4 w = wx0;
        for (int j = jl;;) {
            const f32x4 v = src[j];
            f32x4 o = dst[j];
            // the weight is rounded to fp32 before the fma (dgmr_hip.h)
            o.x = fmaf(__fmul_rn(wyi, w.x), v.x, o.x);
            o.y = fmaf(__fmul_rn(wyi, w.y), v.y, o.y);
            o.z = fmaf(__fmul_rn(wyi, w.z), v.z, o.z);
            o.w = fmaf(__fmul_rn(wyi, w.w), v.w, o.w);
            dst[j] = o;
            j += lpr;
            if (j >= q) break;
            w = wx[j];
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// importance-sampled crops
// ------------------------------------------------------------------------------------------------
#define CROP_CHECK_FRAME(fn)                                                                                                        \
    DGMR_CHECK_ARG(dtype >= DGMR_DT_U8 && dtype <= DGMR_DT_F32, fn ": unknown dtype %d (DGMR_DT_U8 ... DGMR_DT_F32)", dtype);      \
    DGMR_CHECK_ARG(T > 0 && H > 0 && W > 0 && C > 0 && crop > 0, fn ": T=%d H=%d W=%d C=%d crop=%d must be positive", T, H, W, C, crop); \
    DGMR_CHECK_ARG(H >= crop && W >= crop, fn ": frame %d x %d is smaller than the crop %d", H, W, crop)

extern "C" int dgmr_crop_scores(const void* frames, int dtype, int T, int H, int W, int C, float scale, float offset, double sat_scale,
                                int cell, int crop, double* cell_sums, int32_t* cell_missing, double* scores, int32_t* missing,
                                void* stream) {
    CROP_CHECK_FRAME("dgmr_crop_scores");
    DGMR_CHECK_ARG(cell > 0 && crop % cell == 0, "dgmr_crop_scores: crop=%d is not a multiple of cell=%d", crop, cell);
    DGMR_CHECK_ARG(sat_scale > 0.0, "dgmr_crop_scores: sat_scale=%g must be positive", sat_scale);
    DGMR_CHECK_ARG(frames && cell_sums && cell_missing && scores && missing, "dgmr_crop_scores: null pointer");
    const int CH = H / cell, CW = W / cell, Gy = (H - crop) / cell + 1, Gx = (W - crop) / cell + 1;
    DGMR_CHECK_ARG((int64_t)T * cell * (((int64_t)cell * C + 63) / 64) <= INT32_MAX / 2,  // (a lane's work items are counted in int)
                   "dgmr_crop_scores: cell=%d x C=%d x T=%d out of range", cell, C, T);
    const int cw = cell * C, cpb = cw < 64 ? 64 / cw : 1;
    DGMR_CHECK_ARG(CH <= 65535, "dgmr_crop_scores: %d bands of %d rows exceed the grid", CH, cell);
    const dim3 grid(cdiv(CW, cpb), CH), block(64 * CROP_WAVES);
#define CROP_SUMS(TYPE)                                                                                                              \
    hipLaunchKernelGGL(crop_cell_sums_kernel<TYPE>, grid, block, 0, ST, (const TYPE*)frames, T, H, W, C, scale, offset, sat_scale, cell, \
                       cpb, CW, cell_sums, cell_missing)
    switch (dtype) {
        case DGMR_DT_U8: CROP_SUMS(uint8_t); break;
        case DGMR_DT_I16: CROP_SUMS(int16_t); break;
        case DGMR_DT_F16: CROP_SUMS(_Float16); break;
        default: CROP_SUMS(float); break;
    }
#undef CROP_SUMS
    hipLaunchKernelGGL(crop_box_sums_kernel, dim3(cdiv((int64_t)Gy * Gx, 256)), dim3(256), 0, ST, cell_sums, cell_missing, CW,
                       crop / cell, Gy, Gx, scores, missing);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_crop_gather(const void* frames, int dtype, int T, int H, int W, int C, const int32_t* origins, int N, int crop,
                                float scale, float offset, int clamp_missing, float missing_fill, float* out, void* stream) {
    CROP_CHECK_FRAME("dgmr_crop_gather");
    DGMR_CHECK_ARG(N >= 0, "dgmr_crop_gather: N=%d is negative", N);
    if (N == 0) return 0;
    DGMR_CHECK_ARG(frames && origins && out, "dgmr_crop_gather: null pointer");
    const int64_t rows = (int64_t)N * T * C * crop;
    const int blocks = (int)std::min<int64_t>((rows + CROP_WAVES - 1) / CROP_WAVES, 256 * 16);
#define CROP_GATHER(TYPE)                                                                                                            \
    hipLaunchKernelGGL(crop_gather_kernel<TYPE>, dim3(blocks), dim3(64 * CROP_WAVES), 0, ST, (const TYPE*)frames, T, H, W, C, origins, rows, crop, \
                       scale, offset, clamp_missing, missing_fill, out)
    switch (dtype) {
        case DGMR_DT_U8: CROP_GATHER(uint8_t); break;
        case DGMR_DT_I16: CROP_GATHER(int16_t); break;
        case DGMR_DT_F16: CROP_GATHER(_Float16); break;
        default: CROP_GATHER(float); break;
    }
#undef CROP_GATHER
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_tile_blend(const float* pred, float* out, const float* wy, const float* wx, int64_t planes, int tile, int H, int W,
                               int oy, int ox, void* stream) {
    DGMR_CHECK_ARG(pred && out && wy && wx, "dgmr_tile_blend: null pointer");
    DGMR_CHECK_ARG(planes > 0 && tile > 0 && H > 0 && W > 0, "dgmr_tile_blend: planes=%lld tile=%d H=%d W=%d must be positive",
                   (long long)planes, tile, H, W);
    DGMR_CHECK_ARG(tile % 4 == 0 && ox % 4 == 0 && W % 4 == 0, "dgmr_tile_blend: tile=%d, ox=%d and W=%d must be multiples of 4", tile,
                   ox, W);
    DGMR_CHECK_ARG(oy >= 0 && ox >= 0 && (int64_t)oy + tile <= H && (int64_t)ox + tile <= W,
                   "dgmr_tile_blend: tile %d at (oy=%d, ox=%d) is not inside the frame %d x %d", tile, oy, ox, H, W);
    DGMR_CHECK_ARG((((uintptr_t)pred | (uintptr_t)out | (uintptr_t)wx) & 15) == 0, "dgmr_tile_blend: pred, out and wx must be 16-byte aligned");
    DGMR_CHECK_ARG(planes <= INT64_MAX / ((int64_t)H * W), "dgmr_tile_blend: planes=%lld x %d x %d out of range", (long long)planes, H, W);
    DGMR_CHECK_ARG(planes <= INT32_MAX / tile, "dgmr_tile_blend: planes=%lld x tile=%d rows out of range", (long long)planes, tile);
    const int rows = (int)(planes * tile);
    const int q = tile / 4, rpw = 64 / (q < 64 ? q : 64);
    const int blocks = std::min(cdiv(cdiv(rows, rpw), CROP_WAVES), 256 * 8);
    hipLaunchKernelGGL(tile_blend_kernel, dim3(blocks), dim3(64 * CROP_WAVES), 0, ST, (const f32x4*)pred, out, wy, (const f32x4*)wx, rows,
                       tile, H, W, oy, ox);
    DGMR_CHECK_LAUNCH();
    return 0;
}
