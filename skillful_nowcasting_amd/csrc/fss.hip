// Fractions skill score sums (fss.py: fss_sums, FractionsVerifier): overlapping box sums of the event fields of an ensemble and of the
// observation at several thresholds and radii, and the four sums of their products over all window centres.  Integers throughout.
//
// Tiles.  A workgroup (4 waves) takes a 64 x 64 tile of window centres of one plane and one group of thresholds, and stages the tile
// plus a halo of R (the largest radius) rows above and below as BITS: a wave loads 64 consecutive columns of a row of a field (the
// observation first, then every member), and __ballot(present && x >= thr) is that row's event mask for one threshold.  A staged row
// is two 64-bit words, columns [x0 - 32, x0 + 32) and [x0 + 32, x0 + 96): with r <= 32 every window of a tile column lies inside them.
// LDS: 16 bytes per (threshold, field, row); 64 + 2 R + 1 rows (row 0 is a guard row of zeros), M + 1 fields.  The thresholds are cut
// into groups of KG so that a group fits (64 KiB where one threshold does, to keep two workgroups on a CU; else up to 160 KiB), one
// workgroup per group: with K = 3, M = 8, R = 32 all thresholds are staged from one read of the inputs.  Rows and columns outside
// the plane are zero bits (the zero padding of the specification), so are missing pixels.  All LDS is dynamic (16-byte aligned base).
//
// Box sums.  A wave takes one (threshold, radius) at a time - with fewer than four of them, one of 2 or 4 row chunks of the tile - and
// lane c owns tile column c: its window in a staged row is a 128-bit mask of 2 r + 1 bits, the horizontal count two popcounts.  All lanes
// read the same 16 bytes of a row (an LDS broadcast: no bank conflicts).  The lane walks down its rows with one running vertical sum per
// field: add row y + r, subtract row y - r - 1.  Per centre: S_f = sum_m S_m, then S_f^2 (64-bit product: 1.8e10 at M = 32, r = 32),
// S_o^2, S_f S_o and sum_m S_m^2 (each below 2^32) are added to 64-bit lane accumulators.  The wave adds its lanes by xor butterflies and
// adds the four totals to the output with one 64-bit integer atomic per non-zero value: exact in any order, no workspace, two launches
// give the same bits.  The event counts come from the staging ballots (the tile's own rows and columns only), per wave and threshold.
// No floating-point arithmetic after the comparisons.
//
// Cost.  The box sums are VALU work: per (threshold, radius, field, centre) two 128-bit row reads and sixteen and / popcount
// instructions, whatever the radius (profiles/fss_timing.json: 30 x the time of one read of the inputs at the product shape).  The
// member loops carry no branch on m < M and the rows of eight members are read together behind a compiler fence: with the LDS
// allowing two waves per SIMD, a wait per read cost a quarter of the time.
#include "common.h"

namespace {

constexpr int FSS_MAX_M = 32, FSS_MAX_K = 8, FSS_MAX_S = 8, FSS_MAX_R = 32;
constexpr int FSS_TILE = 64, FSS_WAVES = 4, FSS_THREADS = 64 * FSS_WAVES;
constexpr int FSS_MB = 8;               // box sums: members whose rows are read together
constexpr int FSS_UNR = 4, FSS_FB = 5;  // staging: rows x segments and fields loaded together
constexpr int FSS_LDS_SMALL = 64 * 1024, FSS_LDS_LARGE = 160 * 1024;
constexpr int64_t FSS_MAX_BLOCKS = 1 << 18;  // a workgroup strides over (plane, tile, threshold group) items beyond that

struct FssRadii {
    int r[FSS_MAX_S];
};

__host__ __device__ inline int fss_rows(int R) { return FSS_TILE + 2 * R + 1; }
// bytes of LDS per staged threshold
inline int64_t fss_lds_per_threshold(int M, int R) { return (int64_t)(M + 1) * fss_rows(R) * 16; }

__device__ __forceinline__ unsigned long long bits_below(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1ull; }

__device__ __forceinline__ int hcount(const ulonglong2 v, unsigned long long mlo, unsigned long long mhi) {
    return __popcll(v.x & mlo) + __popcll(v.y & mhi);
}

template <int MCAP>
__global__ __launch_bounds__(FSS_THREADS) void fss_kernel(const float* __restrict__ fc, int64_t mstride, const float* __restrict__ obs, int M,
                                                          int H, int W, int tiles_x, int tiles, int64_t items,
                                                          const float* __restrict__ thr, int K, int KG, int groups, FssRadii radii, int S,
                                                          int R, int RC, unsigned long long* __restrict__ sums,
                                                          unsigned long long* __restrict__ events) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_bits[];  // [KG][M + 1][ROWS][2]; field 0 is the observation
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ROWS = fss_rows(R), F = M + 1;
    const int64_t HW = (int64_t)H * W;

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int g = (int)(item % groups);
        const int64_t pt = item / groups;
        const int tile = (int)(pt % tiles);
        const int64_t n = pt / tiles;
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int y0 = ty * FSS_TILE, x0 = tx * FSS_TILE;
        const int k0 = g * KG, KGc = min(KG, K - k0);
        const float* __restrict__ obs_n = obs + n * HW;
        const float* __restrict__ fc_n = fc + n * HW;
        float tk[FSS_MAX_K];
#pragma unroll
        for (int k = 0; k < FSS_MAX_K; ++k) tk[k] = k < KGc ? thr[k0 + k] : __builtin_inff();

        // ---- stage the event bits: item = (staged row j, 64-column segment); lane k keeps the mask of threshold k0 + k ----
        unsigned int evf = 0, evo = 0;
        for (int it0 = wave * FSS_UNR; it0 < ROWS * 2; it0 += FSS_WAVES * FSS_UNR) {
            // FSS_UNR items at a time, FSS_FB fields of each: FSS_UNR * FSS_FB independent loads are in flight before the first is used
            int64_t off[FSS_UNR];
            bool valid[FSS_UNR], pres[FSS_UNR];
#pragma unroll
            for (int u = 0; u < FSS_UNR; ++u) {
                const int it = it0 + u, j = it >> 1, seg = it & 1;
                const int gy = y0 - R - 1 + j, gx = x0 - 32 + seg * 64 + lane;
                // the guard row, the rows and the columns outside the plane: no load, zero bits
                valid[u] = it < ROWS * 2 && j >= 1 && gy >= 0 && gy < H && gx >= 0 && gx < W;
                off[u] = (int64_t)gy * W + gx;  // < H * W where valid
                pres[u] = false;
            }
            for (int f0 = 0; f0 < F; f0 += FSS_FB) {
                float x[FSS_UNR][FSS_FB];
#pragma unroll
                for (int u = 0; u < FSS_UNR; ++u)
#pragma unroll
                    for (int v = 0; v < FSS_FB; ++v) {
                        const int f = f0 + v;  // field 0 is the observation
                        const float* __restrict__ src = f == 0 ? obs_n : fc_n + (int64_t)(f - 1) * mstride;
                        x[u][v] = (valid[u] && f < F) ? src[off[u]] : -1.f;
                    }
                if (f0 == 0) {
#pragma unroll
                    for (int u = 0; u < FSS_UNR; ++u) pres[u] = x[u][0] >= 0.f;
                }
#pragma unroll
                for (int u = 0; u < FSS_UNR; ++u) {
                    const int it = it0 + u, j = it >> 1, seg = it & 1;
                    if (it >= ROWS * 2) break;  // (uniform)
                    const bool own_row = j >= R + 1 && j < R + 1 + FSS_TILE;
                    const unsigned long long cmask = !own_row ? 0ull : seg ? 0x00000000FFFFFFFFull : 0xFFFFFFFF00000000ull;  // the tile's own columns
#pragma unroll
                    for (int v = 0; v < FSS_FB; ++v) {
                        const int f = f0 + v;
                        if (f >= F) break;  // (uniform)
                        unsigned long long w = 0ull;
                        // (thresholds beyond the group's are +inf: their ballots land in lanes that store nothing)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const unsigned long long b = __ballot(pres[u] && x[u][v] >= tk[k]);
                            if (lane == k) w = b;
                        }
                        if (KGc > 4) {  // (uniform)
#pragma unroll
                            for (int k = 4; k < FSS_MAX_K; ++k) {
                                const unsigned long long b = __ballot(pres[u] && x[u][v] >= tk[k]);
                                if (lane == k) w = b;
                            }
                        }
                        if (lane < KGc) {
                            s_bits[(((int64_t)lane * F + f) * ROWS + j) * 2 + seg] = w;
                            const unsigned int c = __popcll(w & cmask);
                            if (f == 0) evo += c;
                            else evf += c;
                        }
                    }
                }
            }
        }
        if (lane < KGc) {
            if (evf) atomicAdd(&events[(n * K + k0 + lane) * 2 + 0], (unsigned long long)evf);
            if (evo) atomicAdd(&events[(n * K + k0 + lane) * 2 + 1], (unsigned long long)evo);
        }
        __syncthreads();

        // ---- box sums and products: item = (threshold of the group, radius, row chunk), lane = tile column ----
        const int rows_in_tile = min(FSS_TILE, H - y0), rpc = FSS_TILE / RC;
        const bool colok = x0 + lane < W;
        const ulonglong2* __restrict__ rows = (const ulonglong2*)s_bits;
        for (int it = wave; it < KGc * S * RC; it += FSS_WAVES) {
            const int chunk = it % RC, combo = it / RC;
            const int s = combo % S, kl = combo / S;
            const int r = radii.r[s];
            const int ys = chunk * rpc, ye = min(ys + rpc, rows_in_tile);
            if (ys >= ye) continue;
            // the window of tile column `lane`: bits lane + 32 - r ... lane + 32 + r of the 128 staged columns
            const int b0 = lane + 32 - r, b1 = lane + 32 + r + 1;
            const unsigned long long mlo = bits_below(b1) & ~bits_below(b0), mhi = bits_below(b1 - 64) & ~bits_below(b0 - 64);
            const ulonglong2* __restrict__ base = rows + (int64_t)kl * F * ROWS;  // field f, staged row j: base[f * ROWS + j]
            int V[MCAP], Vo = 0;
#pragma unroll
            for (int m = 0; m < MCAP; ++m) V[m] = 0;
            // the window of tile row ys - 1: staged rows ys + R - r ... ys + R + r (tile row y is staged row y + R + 1)
            // No branch on m < M anywhere below: a member beyond M reads field M's rows and its counts are dropped by a select, so the
            // LDS reads of all fields of a row are issued together.
            // The reads of FSS_MB members' rows are issued together and fenced off from their uses (the compiler would otherwise
            // wait for every read before it issues the next: two waves per SIMD cannot hide that).
            for (int j = ys + R - r; j <= ys + R + r; ++j) {
                const ulonglong2 ao = base[j];
#pragma unroll
                for (int m0 = 0; m0 < MCAP; m0 += FSS_MB) {
                    ulonglong2 a[FSS_MB];
#pragma unroll
                    for (int i = 0; i < FSS_MB; ++i)
                        if (m0 + i < MCAP) a[i] = base[min(m0 + i + 1, M) * ROWS + j];
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int i = 0; i < FSS_MB; ++i)
                        if (m0 + i < MCAP) {
                            const int h = hcount(a[i], mlo, mhi);
                            V[m0 + i] += m0 + i < M ? h : 0;
                        }
                }
                Vo += hcount(ao, mlo, mhi);
            }
            const unsigned int keep = colok ? ~0u : 0u;  // a tile column outside the plane is no window centre
            unsigned long long a_ff = 0, a_oo = 0, a_fo = 0, a_mm = 0;
            for (int y = ys; y < ye; ++y) {
                const int ja = y + R + r + 1, js = y + R - r;  // 0 <= js, ja <= ROWS - 1
                const ulonglong2 ao = base[ja], bo = base[js];
                unsigned int sf = 0, mm = 0;
#pragma unroll
                for (int m0 = 0; m0 < MCAP; m0 += FSS_MB) {
                    ulonglong2 a[FSS_MB], b[FSS_MB];
#pragma unroll
                    for (int i = 0; i < FSS_MB; ++i)
                        if (m0 + i < MCAP) {
                            const int fm = min(m0 + i + 1, M) * ROWS;
                            a[i] = base[fm + ja];
                            b[i] = base[fm + js];
                        }
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int i = 0; i < FSS_MB; ++i)
                        if (m0 + i < MCAP) {
                            const int d = hcount(a[i], mlo, mhi) - hcount(b[i], mlo, mhi);
                            V[m0 + i] += m0 + i < M ? d : 0;  // (stays 0 beyond M)
                            sf += (unsigned int)V[m0 + i];
                            mm += (unsigned int)V[m0 + i] * (unsigned int)V[m0 + i];  // sum <= 32 * 4225^2 < 2^32
                        }
                }
                Vo += hcount(ao, mlo, mhi) - hcount(bo, mlo, mhi);
                sf &= keep;
                const unsigned int so = (unsigned int)Vo & keep;
                a_ff += (unsigned long long)sf * sf;
                a_oo += so * so;
                a_fo += sf * so;  // <= 32 * 4225 * 4225 < 2^32
                a_mm += mm & keep;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                a_ff += __shfl_xor(a_ff, o, 64);
                a_oo += __shfl_xor(a_oo, o, 64);
                a_fo += __shfl_xor(a_fo, o, 64);
                a_mm += __shfl_xor(a_mm, o, 64);
            }
            const unsigned long long v = lane == 0 ? a_ff : lane == 1 ? a_oo : lane == 2 ? a_fo : a_mm;
            if (lane < 4 && v) atomicAdd(&sums[((n * K + k0 + kl) * S + s) * 4 + lane], v);
        }
        __syncthreads();  // the next item stages over these bits
    }
}

template <int MCAP>
int fss_launch(const char* fn, int blocks, int lds, hipStream_t st, const float* fc, int64_t mstride, const float* obs, int M, int H, int W,
               int tiles_x, int tiles, int64_t items, const float* thr, int K, int KG, int groups, const FssRadii& radii, int S, int R, int RC,
               void* sums, void* events) {
    if (lds > FSS_LDS_SMALL &&
        hipFuncSetAttribute((const void*)fss_kernel<MCAP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        dgmr_set_error("%s: %d bytes of LDS per workgroup were refused: %s", fn, lds, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    hipLaunchKernelGGL((fss_kernel<MCAP>), dim3(blocks), dim3(FSS_THREADS), lds, st, fc, mstride, obs, M, H, W, tiles_x, tiles, items, thr, K,
                       KG, groups, radii, S, R, RC, (unsigned long long*)sums, (unsigned long long*)events);
    return 0;
}

}  // namespace

extern "C" int dgmr_fss_sums(const float* forecast, int64_t member_stride, const float* observed, int M, int64_t N, int H, int W,
                             const float* thresholds, int K, const int* radii, int S, void* sums, void* events, void* stream) {
    const char* fn = "dgmr_fss_sums";
    DGMR_CHECK_ARG(M >= 1 && M <= FSS_MAX_M, "%s: M=%d members, 1 ... %d are supported", fn, M, FSS_MAX_M);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "%s: H=%d and W=%d must be positive multiples of 16", fn, H, W);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
    DGMR_CHECK_ARG(K >= 1 && K <= FSS_MAX_K, "%s: K=%d thresholds, 1 ... %d are supported", fn, K, FSS_MAX_K);
    DGMR_CHECK_ARG(S >= 1 && S <= FSS_MAX_S, "%s: S=%d radii, 1 ... %d are supported", fn, S, FSS_MAX_S);
    DGMR_CHECK_ARG(forecast && observed && thresholds && radii && sums && events, "%s: null pointer", fn);
    FssRadii rad = {};
    int R = 0;
    for (int s = 0; s < S; ++s) {
        DGMR_CHECK_ARG(radii[s] >= 0 && radii[s] <= FSS_MAX_R, "%s: radius %d is outside 0 ... %d", fn, radii[s], FSS_MAX_R);
        for (int q = 0; q < s; ++q) DGMR_CHECK_ARG(radii[q] != radii[s], "%s: radius %d is given twice", fn, radii[s]);
        rad.r[s] = radii[s];
        R = std::max(R, radii[s]);
    }
    DGMR_CHECK_ARG(M == 1 || (member_stride >= 0 && member_stride % 4 == 0 && member_stride <= INT64_MAX / 4 / FSS_MAX_M),
                   "%s: member_stride=%lld must be a non-negative multiple of 4 elements", fn, (long long)member_stride);
    DGMR_CHECK_ARG((((uintptr_t)forecast | (uintptr_t)observed) & 15) == 0, "%s: forecast and observed must be 16-byte aligned", fn);
    DGMR_CHECK_ARG((((uintptr_t)sums | (uintptr_t)events) & 7) == 0, "%s: sums and events must be 8-byte aligned", fn);
    {   // every sum is at most M^2 (2 R + 1)^4 H W
        const unsigned __int128 side = 2 * R + 1, bound = (unsigned __int128)(M * M) * side * side * side * side * (uint64_t)H * (uint64_t)W;
        DGMR_CHECK_ARG(bound < ((unsigned __int128)1 << 63), "%s: M^2 (2 R + 1)^4 H W with M=%d, R=%d, H=%d, W=%d reaches 2^63: the sums could overflow",
                       fn, M, R, H, W);
    }
    const int64_t per = fss_lds_per_threshold(M, R);  // <= 33 * 129 * 16 = 68112
    const int budget = per <= FSS_LDS_SMALL ? FSS_LDS_SMALL : FSS_LDS_LARGE;
    const int KG = (int)std::min<int64_t>(K, budget / per), groups = (K + KG - 1) / KG;
    const int lds = (int)(per * KG);
    const int RC = KG * S >= 4 ? 1 : KG * S >= 2 ? 2 : 4;
    const int tiles_x = (W + FSS_TILE - 1) / FSS_TILE, tiles = ((H + FSS_TILE - 1) / FSS_TILE) * tiles_x;
    const int64_t items = N * tiles * groups;
    const int blocks = (int)std::min<int64_t>(items, FSS_MAX_BLOCKS);
    hipStream_t st = ST;
    if (hipMemsetAsync(sums, 0, (size_t)N * K * S * 4 * sizeof(int64_t), st) != hipSuccess ||
        hipMemsetAsync(events, 0, (size_t)N * K * 2 * sizeof(int64_t), st) != hipSuccess) {
        dgmr_set_error("%s: clearing the outputs failed: %s", fn, hipGetErrorString(hipGetLastError()));
        return -2;
    }
#define FSS_GO(MCAP)                                                                                                                       \
    fss_launch<MCAP>(fn, blocks, lds, st, forecast, M == 1 ? 0 : member_stride, observed, M, H, W, tiles_x, tiles, items, thresholds, K, KG, \
                     groups, rad, S, R, RC, sums, events)
    const int rc = M == 1 ? FSS_GO(1) : M <= 6 ? FSS_GO(6) : M <= 8 ? FSS_GO(8) : M <= 16 ? FSS_GO(16) : FSS_GO(32);
#undef FSS_GO
    if (rc != 0) return rc;
    DGMR_CHECK_LAUNCH();
    return 0;
}
