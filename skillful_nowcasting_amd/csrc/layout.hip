// Pooling and frame layout moves for gfx950 (space-to-depth, depth-to-space, channel copies), and the window sums of the upsampling
// conv's weight gradient.  HBM-bound, 16-byte vectorised where the layout allows.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// pooling and layout
// ------------------------------------------------------------------------------------------------
__global__ void pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ addend, float* __restrict__ y, int N, int D,
                                int H, int W, int C, int pd, float scale, const float* __restrict__ mask_src,
                                const float* __restrict__ mask_a, const float* __restrict__ mask_b, int mask_group) {
    const int Do = D / pd, Ho = H / 2, Wo = W / 2, C4 = C / 4;
    const int64_t total = (int64_t)N * Do * Ho * Wo * C4;
    GRID_STRIDE(i, total) {
        const int c4 = i % C4;
        int64_t t = i / C4;
        const int wo = t % Wo;
        t /= Wo;
        const int ho = t % Ho;
        t /= Ho;
        const int d_o = t % Do;
        const int n = t / Do;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int dz = 0; dz < pd; ++dz)
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const size_t off = ((((size_t)n * D + d_o * pd + dz) * H + ho * 2 + dy) * W + wo * 2 + dx) * C + c4 * 4;
                    s += *reinterpret_cast<const f32x4*>(x + off);
                }
        s *= scale;
        const size_t o = (size_t)i * 4;
        if (addend) s += *reinterpret_cast<const f32x4*>(addend + o);
        if (mask_src) {
            f32x4 m = *reinterpret_cast<const f32x4*>(mask_src + o);
            if (mask_a) {
                const size_t gc = (size_t)(n / mask_group) * C + c4 * 4;
                const f32x4 a = *reinterpret_cast<const f32x4*>(mask_a + gc);
                const f32x4 b = *reinterpret_cast<const f32x4*>(mask_b + gc);
                m = m * a + b;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = m[j] > 0.f ? s[j] : 0.f;
        }
        *reinterpret_cast<f32x4*>(y + o) = s;
    }
}

// y[n][j] = (x[n][2j] + x[n][2j + 1]) / 2 (+ addend[n][j]): the depth half of AvgPool3d(2) over planes of `plane4` float4 (the spatial
// half already rode in the conv that produced x: dgmr_conv_args.pool2 on a 3x3x3 conv).  blockIdx.y walks the output planes.
__global__ __launch_bounds__(256) void pool_depth2_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ addend,
                                                           f32x4* __restrict__ y, int N, int D, int64_t plane4) {
    const int Do = D / 2;
    for (int op = blockIdx.y; op < N * Do; op += gridDim.y) {
        const int n = op / Do, j = op - n * Do;
        const f32x4* x0 = x + ((size_t)n * D + 2 * j) * plane4;
        const size_t ob = (size_t)op * plane4;
        GRID_STRIDE(i, plane4) {
            f32x4 v = (x0[i] + x0[plane4 + i]) * 0.5f;
            if (addend) v += addend[ob + i];
            y[ob + i] = v;
        }
    }
}

__global__ void pool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N, int D, int H, int W, int C, int pd,
                                float scale) {
    const int Do = D / pd, Ho = H / 2, Wo = W / 2, C4 = C / 4;
    const int64_t total = (int64_t)N * D * H * W * C4;
    GRID_STRIDE(i, total) {
        const int c4 = i % C4;
        int64_t t = i / C4;
        const int w = t % W;
        t /= W;
        const int h = t % H;
        t /= H;
        const int d = t % D;
        const int n = t / D;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int d_o = d / pd, ho = h >> 1, wo = w >> 1;
        if (d_o < Do && ho < Ho && wo < Wo) {
            const size_t off = ((((size_t)n * Do + d_o) * Ho + ho) * Wo + wo) * C + c4 * 4;
            v = *reinterpret_cast<const f32x4*>(dy + off) * scale;
        }
        *reinterpret_cast<f32x4*>(dx + (size_t)i * 4) = v;
    }
}

// `fol` given (dgmr_frames_s2d_pair): sample b's sequence is the Tc frames of fr[b % Bc] followed by the T - Tc frames of fol[b % Bf]
__global__ void frames_s2d_kernel(const float* __restrict__ fr, const int32_t* __restrict__ idx, float* __restrict__ out, int B,
                                  int T, int C, int H, int W, int F, int p, int frame_major, int idx_group,
                                  const float* __restrict__ fol, int Bc, int Tc, int Bf) {
    const int Ho = H / (2 * p), Wo = W / (2 * p), Co = 4 * C;
    const int64_t total = (int64_t)B * F * Ho * Wo * Co;
    const float inv = 1.f / (float)(p * p);
    GRID_STRIDE(i, total) {
        const int co = i % Co;
        int64_t t = i / Co;
        const int wo = t % Wo;
        t /= Wo;
        const int ho = t % Ho;
        t /= Ho;
        int b, f;
        if (frame_major) {
            b = t % B;
            f = t / B;
        } else {
            f = t % F;
            b = t / F;
        }
        const int c = co >> 2, dy = (co >> 1) & 1, dx = co & 1;
        const int tf = idx ? idx[(b / idx_group) * F + f] : f;
        const float* src = !fol ? fr + (((size_t)b * T + tf) * C + c) * H * W
                           : (tf < Tc ? fr + (((size_t)(b % Bc) * Tc + tf) * C + c) * H * W
                                      : fol + (((size_t)(b % Bf) * (T - Tc) + (tf - Tc)) * C + c) * H * W);
        float s = 0.f;
        for (int py = 0; py < p; ++py)
            for (int px = 0; px < p; ++px) s += src[(size_t)((2 * ho + dy) * p + py) * W + (2 * wo + dx) * p + px];
        out[i] = s * inv;
    }
}

// Gradient of frames_s2d as a GATHER over the pixels of dframes: every element sums the (at most F) selected frames that read it, in
// frame order - no atomics, no zero-fill, bit-identical from run to run (the scatter form added duplicates of a randomly drawn
// frame index in whatever order the workgroups arrived: three draws of one frame among the spatial discriminator's eight happen in
// ~10 % of the steps).  dframes is WRITTEN, every element.
// t_off > 0 (dgmr_frames_s2d_pair_bwd): dfr holds frames t_off .. t_off + T - 1 of every sequence only (the frames before get no gradient)
__global__ void frames_s2d_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ idx, float* __restrict__ dfr,
                                      int B, int T, int C, int H, int W, int F, int p, int frame_major, int idx_group, int t_off) {
    const int Ho = H / (2 * p), Wo = W / (2 * p), Co = 4 * C;
    const int64_t total = (int64_t)B * T * C * H * W;
    const float inv = 1.f / (float)(p * p);
    GRID_STRIDE(i, total) {
        const int x = i % W;
        int64_t t = i / W;
        const int y = t % H;
        t /= H;
        const int c = t % C;
        t /= C;
        const int tf = t % T + t_off;
        const int b = t / T;
        const int xo = x / p, yo = y / p;  // pixel of the (pooled) frame
        const int wo = xo >> 1, dx = xo & 1, ho = yo >> 1, dy = yo & 1;
        float g = 0.f;
        if (ho < Ho && wo < Wo) {
            const int co = (c << 2) | (dy << 1) | dx;
            const int f_lo = idx ? 0 : tf, f_hi = idx ? F : min(tf + 1, F);  // no index list: frame f reads frame f
            for (int f = f_lo; f < f_hi; ++f) {
                const int src = idx ? idx[(b / idx_group) * F + f] : f;
                if (src != tf) continue;
                const int64_t n = frame_major ? (int64_t)f * B + b : (int64_t)b * F + f;
                g += dout[((n * Ho + ho) * Wo + wo) * Co + co] * inv;
            }
        }
        dfr[i] = g;
    }
}

template <bool BWD>
__global__ void d2s_frames_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int T, int t, int C, int h, int w) {
    // forward: frames[b][t][c][2y+dy][2x+dx] = x[b][y][x][c*4+dy*2+dx]; one thread per frame pixel (coalesced frame side)
    const int H = 2 * h, W = 2 * w;
    const int64_t total = (int64_t)B * C * H * W;
    GRID_STRIDE(i, total) {
        const int X = i % W;
        int64_t r = i / W;
        const int Y = r % H;
        r /= H;
        const int c = r % C;
        const int b = r / C;
        const size_t fi = ((((size_t)b * T + t) * C + c) * H + Y) * W + X;
        const size_t xi = (((size_t)b * h + (Y >> 1)) * w + (X >> 1)) * (4 * C) + c * 4 + (Y & 1) * 2 + (X & 1);
        if (BWD) dst[xi] = src[fi];
        else dst[fi] = src[xi];
    }
}

__global__ void copy_channels_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t R, int C, int src_C, int src_off,
                                     int src_cs, int dst_C, int dst_off, int dst_cs, int accumulate) {
    const int64_t total = R * C;
    GRID_STRIDE(i, total) {
        const int c = i % C;
        const int64_t r = i / C;
        const float v = src[(size_t)r * src_C + src_off + (size_t)c * src_cs];
        float* d = dst + (size_t)r * dst_C + dst_off + (size_t)c * dst_cs;
        *d = accumulate ? *d + v : v;
    }
}

// z[n][r][c][co*9 + ky*3 + kx] = sum_{i,j in {0,1}} dy[n][2r + 1 - ky + i][2c + 1 - kx + j][co]  (zero outside the map): the window
// sums of the output gradient that meet input pixel (r, c) under tap (ky, kx) of a 3x3 conv on the nearest-2x upsampled map.  One
// block = P consecutive pixels of an input row: the 4 x (2P + 2) x C window goes through LDS once, every output is 4 LDS reads and
// one coalesced store.
__global__ void upsample_wgrad_sums_kernel(const float* __restrict__ dy, float* __restrict__ z, int H, int W, int C, int P) {
    extern __shared__ float win[];  // [4][2P + 2][C]
    const int wblocks = W / P;
    const int64_t b = blockIdx.x;
    const int c0 = (int)(b % wblocks) * P;
    const int r = (int)((b / wblocks) % H);
    const int n = (int)(b / ((int64_t)wblocks * H));
    const int H2 = 2 * H, W2 = 2 * W, cols = 2 * P + 2, C4 = C >> 2;
    for (int i = threadIdx.x; i < 4 * cols * C4; i += blockDim.x) {
        const int c4 = i % C4, col = (i / C4) % cols, row = i / (C4 * cols);
        const int R = 2 * r - 1 + row, Cc = 2 * c0 - 1 + col;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)R < (unsigned)H2 && (unsigned)Cc < (unsigned)W2)
            v = *reinterpret_cast<const f32x4*>(dy + (((size_t)n * H2 + R) * W2 + Cc) * C + c4 * 4);
        *reinterpret_cast<f32x4*>(win + ((size_t)row * cols + col) * C + c4 * 4) = v;
    }
    __syncthreads();
    const int C9 = 9 * C;
    float* zrow = z + (((size_t)n * H + r) * W + c0) * C9;
    for (int rem = threadIdx.x; rem < C9; rem += blockDim.x) {  // (divisions by constants only: the loop over pixels is inside)
        const int co = rem / 9, tap = rem - co * 9, ky = tap / 3, kx = tap - ky * 3;
        const float* w0 = win + ((size_t)(2 - ky) * cols + 2 - kx) * C + co;
        const int rs = cols * C;
        for (int j = 0; j < P; ++j, w0 += 2 * C) zrow[(size_t)j * C9 + rem] = (w0[0] + w0[C]) + (w0[rs] + w0[rs + C]);
    }
}

}  // namespace

extern "C" int dgmr_pool_fwd(const float* x, const float* addend, float* y, int N, int D, int H, int W, int C, int pd, float scale,
                             const float* mask_src, const float* mask_a, const float* mask_b, int mask_group, void* stream) {
    DGMR_CHECK_ARG(x && y, "dgmr_pool_fwd: null pointer");
    DGMR_CHECK_ARG(C % 4 == 0 && (pd == 1 || pd == 2), "dgmr_pool_fwd: C=%d pd=%d unsupported", C, pd);
    if (scale == 0.f) scale = 1.f / (4.f * pd);
    if (mask_group < 1) mask_group = 1;
    const int64_t total = (int64_t)N * (D / pd) * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(pool_fwd_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, x, addend, y, N, D, H, W, C, pd, scale,
                       mask_src, mask_a, mask_b, mask_group);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_pool_depth2(const float* x, const float* addend, float* y, int N, int D, int64_t plane, void* stream) {
    DGMR_CHECK_ARG(x && y, "dgmr_pool_depth2: null pointer");
    DGMR_CHECK_ARG(N > 0 && D >= 2 && plane > 0 && plane % 4 == 0 && al16(x) && al16(y) && al16(addend),
                   "dgmr_pool_depth2: N=%d D=%d plane=%lld (planes of whole, aligned float4)", N, D, (long long)plane);
    const int64_t plane4 = plane / 4;
    const int planes = N * (D / 2);
    hipLaunchKernelGGL(pool_depth2_kernel, dim3((unsigned)std::min<int64_t>((plane4 + 255) / 256, 1024), (unsigned)std::min(planes, 65535)),
                       dim3(256), 0, ST, (const f32x4*)x, (const f32x4*)addend, (f32x4*)y, N, D, plane4);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_pool_bwd(const float* dy, float* dx, int N, int D, int H, int W, int C, int pd, float scale, void* stream) {
    DGMR_CHECK_ARG(dy && dx, "dgmr_pool_bwd: null pointer");
    DGMR_CHECK_ARG(C % 4 == 0 && (pd == 1 || pd == 2), "dgmr_pool_bwd: C=%d pd=%d unsupported", C, pd);
    if (scale == 0.f) scale = 1.f / (4.f * pd);
    const int64_t total = (int64_t)N * D * H * W * (C / 4);
    hipLaunchKernelGGL(pool_bwd_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, dy, dx, N, D, H, W, C, pd, scale);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_frames_s2d(const float* frames, const int32_t* idx, float* out, int B, int T, int C, int H, int W, int F,
                               int pool, int frame_major, int idx_group, void* stream) {
    if (idx_group < 1) idx_group = B;
    DGMR_CHECK_ARG(frames && out, "dgmr_frames_s2d: null pointer");
    const int p = pool ? 2 : 1;
    DGMR_CHECK_ARG(H % (2 * p) == 0 && W % (2 * p) == 0, "dgmr_frames_s2d: H=%d W=%d not divisible by %d", H, W, 2 * p);
    const int64_t total = (int64_t)B * F * (H / (2 * p)) * (W / (2 * p)) * 4 * C;
    hipLaunchKernelGGL(frames_s2d_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, frames, idx, out, B, T, C, H, W, F, p,
                       frame_major, idx_group, (const float*)nullptr, 0, 0, 0);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_frames_s2d_pair(const float* context, const float* following, const int32_t* idx, float* out, int N, int Bc, int Tc,
                                    int Bf, int Tf, int C, int H, int W, int F, int pool, int frame_major, int idx_group, void* stream) {
    if (idx_group < 1) idx_group = N;
    DGMR_CHECK_ARG(context && following && out, "dgmr_frames_s2d_pair: null pointer");
    DGMR_CHECK_ARG(N > 0 && Bc > 0 && Bf > 0 && Tc > 0 && Tf > 0 && N % Bc == 0 && N % Bf == 0,
                   "dgmr_frames_s2d_pair: N=%d must be a multiple of the %d context and the %d following sequences", N, Bc, Bf);
    DGMR_CHECK_ARG(idx || F <= Tc + Tf, "dgmr_frames_s2d_pair: F=%d frames of a sequence of %d", F, Tc + Tf);
    const int p = pool ? 2 : 1;
    DGMR_CHECK_ARG(H % (2 * p) == 0 && W % (2 * p) == 0, "dgmr_frames_s2d_pair: H=%d W=%d not divisible by %d", H, W, 2 * p);
    const int64_t total = (int64_t)N * F * (H / (2 * p)) * (W / (2 * p)) * 4 * C;
    hipLaunchKernelGGL(frames_s2d_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, context, idx, out, N, Tc + Tf, C, H, W, F, p,
                       frame_major, idx_group, following, Bc, Tc, Bf);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_frames_s2d_bwd(const float* dout, const int32_t* idx, float* dframes, int B, int T, int C, int H, int W, int F,
                                   int pool, int frame_major, int idx_group, void* stream) {
    if (idx_group < 1) idx_group = B;
    DGMR_CHECK_ARG(dout && dframes, "dgmr_frames_s2d_bwd: null pointer");
    const int p = pool ? 2 : 1;
    const int64_t total = (int64_t)B * T * C * H * W;
    hipLaunchKernelGGL(frames_s2d_bwd_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, dout, idx, dframes, B, T, C, H, W, F,
                       p, frame_major, idx_group, 0);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_frames_s2d_pair_bwd(const float* dout, const int32_t* idx, float* dfollowing, int N, int Tc, int Tf, int C, int H,
                                        int W, int F, int pool, int frame_major, int idx_group, void* stream) {
    if (idx_group < 1) idx_group = N;
    DGMR_CHECK_ARG(dout && dfollowing, "dgmr_frames_s2d_pair_bwd: null pointer");
    DGMR_CHECK_ARG(N > 0 && Tc > 0 && Tf > 0, "dgmr_frames_s2d_pair_bwd: N=%d Tc=%d Tf=%d", N, Tc, Tf);
    const int p = pool ? 2 : 1;
    const int64_t total = (int64_t)N * Tf * C * H * W;
    hipLaunchKernelGGL(frames_s2d_bwd_kernel, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, dout, idx, dfollowing, N, Tf, C, H, W, F,
                       p, frame_major, idx_group, Tc);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_d2s_frames(const float* x, float* frames, int B, int T, int t, int C, int h, int w, void* stream) {
    DGMR_CHECK_ARG(x && frames && t >= 0 && t < T, "dgmr_d2s_frames: bad args");
    const int64_t total = (int64_t)B * C * 4 * h * w;
    hipLaunchKernelGGL(d2s_frames_kernel<false>, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, x, frames, B, T, t, C, h, w);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_d2s_frames_bwd(const float* dframes, float* dx, int B, int T, int t, int C, int h, int w, void* stream) {
    DGMR_CHECK_ARG(dframes && dx && t >= 0 && t < T, "dgmr_d2s_frames_bwd: bad args");
    const int64_t total = (int64_t)B * C * 4 * h * w;
    hipLaunchKernelGGL(d2s_frames_kernel<true>, dim3(ew_blocks(total)), dim3(EW_THREADS), 0, ST, dframes, dx, B, T, t, C, h, w);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_copy_channels(const float* src, float* dst, int64_t R, int C, int src_C, int src_off, int src_cstride,
                                  int dst_C, int dst_off, int dst_cstride, int accumulate, void* stream) {
    DGMR_CHECK_ARG(src && dst && R > 0 && C > 0, "dgmr_copy_channels: bad args");
    hipLaunchKernelGGL(copy_channels_kernel, dim3(ew_blocks(R * C)), dim3(EW_THREADS), 0, ST, src, dst, R, C, src_C, src_off,
                       src_cstride, dst_C, dst_off, dst_cstride, accumulate);
    DGMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int dgmr_upsample_wgrad_sums(const float* dy, float* z, int N, int H, int W, int C, void* stream) {
    DGMR_CHECK_ARG(dy && z && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "dgmr_upsample_wgrad_sums: bad args (C=%d)", C);
    int P = 8;
    while (P > 1 && (W % P != 0 || (size_t)4 * (2 * P + 2) * C * sizeof(float) > 48 * 1024)) P >>= 1;
    const size_t lds = (size_t)4 * (2 * P + 2) * C * sizeof(float);
    DGMR_CHECK_ARG(lds <= 64 * 1024, "dgmr_upsample_wgrad_sums: C=%d too wide", C);
    const int64_t blocks = (int64_t)N * H * (W / P);
    DGMR_CHECK_ARG(blocks < (1ll << 31), "dgmr_upsample_wgrad_sums: grid too large");
    hipLaunchKernelGGL(upsample_wgrad_sums_kernel, dim3((unsigned)blocks), dim3(256), lds, ST, dy, z, H, W, C, P);
    DGMR_CHECK_LAUNCH();
    return 0;
}
