// Ensemble verification on the device (verification.py: ensemble_scores, NowcastVerifier): pooled CRPS terms, contingency counts and
// the rank table of an ensemble forecast against an observation, in one streaming read of both.
//
// Layout.  A plane [H][W] is cut into 16 x 16 tiles and a wave takes one tile at a time: lane l holds the four pixels (row l >> 2,
// columns 4 * (l & 3) ... + 3) of every member and of the observation, one 16-byte load each.  Every pooling cell of every scale
// (2, 4, 8, 16) then lies inside the wave, and its pooled values come from xor butterflies:
//     level 2:  (p0 + p1), (p2 + p3) in the lane, then + the lane 4 away (the row below / above)
//     level 4:  the lane's two level-2 cells, then + the lane 8 away
//     level 8:  + the lane 1 away, then + the lane 16 away
//     level 16: + the lane 2 away, then + the lane 32 away
// i.e. at every level a cell is (top-left + top-right) + (bottom-left + bottom-right) of the level below - the order
// verification.py's reference uses, so the float64 pooled sums are the same bits on both sides (a + b is commutative: both lanes of
// an exchange hold the same value).  Maxima follow the same tree.
//
// Sums.  The float64 terms of a workgroup are added per lane in tile order, across the lanes of a wave by a xor butterfly, across
// the four waves in wave order, and stored as one row of partials in the workspace; ens_finalize_kernel adds the rows of a plane in
// index order.  No floating-point atomics anywhere: two launches give the same bits.  The integer counts (cells, contingency, ranks)
// are exact in any order: waves count with ballots (the rank table: the key of the wave's first present lane by ballot, every
// other key lane by lane), add to LDS counters and the workgroup adds its non-zero counters to the outputs
// with integer atomics.
//
// Exceedance table (value.py: dgmr_exceedance_table), from which reliability, Brier score, ROC points and economic value are derived.
// One streaming read (16-byte loads) of the ensemble and the observation; per pixel and threshold the number of members that reach the
// threshold is the row, the observation's own exceedance the column of a per-workgroup histogram in LDS (at most 8 x 33 x 2
// counters).  A wave adds the key of its first present lane once by ballot - in a radar field that is nearly everybody's key - and the other keys lane by lane; the workgroup adds its non-zero counters to the table with integer atomics.
#include "common.h"

namespace {

constexpr int ENS_WAVES = 4;       // waves per workgroup, one 16 x 16 tile each per round
constexpr int ENS_LEVELS = 5;      // scales 1, 2, 4, 8, 16
constexpr int ENS_Q = ENS_LEVELS * 4;  // doubles per partial row: [level][avg, max][abs_err, pair]
constexpr int ENS_MAX_M = 32, ENS_MAX_K = 8;
constexpr int ENS_TARGET_BLOCKS = 4096;  // about 16 workgroups of 4 waves per CU

// NaN-propagating maximum (numpy's maximum): a NaN operand gives NaN; of +0 and -0 either (only |differences| are formed from it)
__device__ __forceinline__ float pmax(float a, float b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ int popc64(unsigned long long v) { return __popcll(v); }

// The two terms of one cell: a = sum_m |v_m - y|, p = sum_{m<k} |v_m - v_k|, members in index order, pairs in (m, k) lexicographic order.
template <int MCAP, bool EXACT>
__device__ __forceinline__ void cell_terms(const double (&v)[MCAP], double y, int M, double& a, double& p) {
    a = 0.0;
    p = 0.0;
#pragma unroll
    for (int m = 0; m < MCAP; ++m) {
        if (EXACT || m < M) {
            a += fabs(v[m] - y);
#pragma unroll
            for (int k = m + 1; k < MCAP; ++k)
                if (EXACT || k < M) p += fabs(v[m] - v[k]);
        }
    }
}

// Workgroups of a plane: enough of them to fill the chip over all planes, never more than the plane has rounds of four tiles.
inline int ens_blocks_per_plane(int64_t N, int tiles) {
    const int64_t want = std::max<int64_t>(1, ENS_TARGET_BLOCKS / N);
    return (int)std::min<int64_t>(want, (tiles + ENS_WAVES - 1) / ENS_WAVES);
}

// lvl_slot: 4 bits per level, the output slot of that scale or 0xF when the scale is not asked for.
__device__ __forceinline__ int slot_of(uint32_t lvl_slot, int lvl) { return (lvl_slot >> (4 * lvl)) & 0xF; }

template <int MCAP, bool EXACT>
__global__ __launch_bounds__(64 * ENS_WAVES) void ens_scores_kernel(
    const float* __restrict__ fc, int64_t mstride, const float* __restrict__ obs, int M, int W, int tiles_x, int tiles, int BPP,
    uint32_t lvl_slot, int max_lvl, int S, const float* __restrict__ thr, int K, double* __restrict__ ws,
    unsigned long long* __restrict__ cells, unsigned long long* __restrict__ cont, unsigned long long* __restrict__ ranks, int64_t HW) {
    __shared__ unsigned int s_cont[ENS_MAX_K * ENS_MAX_M * 3];
    __shared__ unsigned int s_rank[(ENS_MAX_M + 1) * (ENS_MAX_M + 1)];
    __shared__ unsigned int s_cells[ENS_LEVELS];
    __shared__ double s_part[ENS_WAVES][ENS_Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_cont = K * M * 3, n_rank = (M + 1) * (M + 1);
    for (int i = tid; i < n_cont; i += 64 * ENS_WAVES) s_cont[i] = 0;
    for (int i = tid; i < n_rank; i += 64 * ENS_WAVES) s_rank[i] = 0;
    if (tid < ENS_LEVELS) s_cells[tid] = 0;
    __syncthreads();

    const int64_t n = blockIdx.x / BPP;
    const int b = blockIdx.x - (int)n * BPP;
    const int row = lane >> 2, c4 = lane & 3;
    const float* __restrict__ obs_n = obs + n * HW;
    const float* __restrict__ fc_n = fc + n * HW;
    const bool want0 = slot_of(lvl_slot, 0) != 0xF, want1 = slot_of(lvl_slot, 1) != 0xF, want2 = slot_of(lvl_slot, 2) != 0xF,
               want3 = slot_of(lvl_slot, 3) != 0xF, want4 = slot_of(lvl_slot, 4) != 0xF;
    const bool own1 = (lane & 4) == 0, own2 = (lane & 12) == 0, own3 = (lane & 29) == 0, own4 = lane == 0;

    double acc[ENS_Q];
#pragma unroll
    for (int q = 0; q < ENS_Q; ++q) acc[q] = 0.0;
    unsigned int ncell[ENS_LEVELS] = {0, 0, 0, 0, 0};  // (the same in every lane of the wave)

    for (int t = b * ENS_WAVES + wave; t < tiles; t += BPP * ENS_WAVES) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int64_t off = (int64_t)(ty * 16 + row) * W + tx * 16 + c4 * 4;  // < H * W: tiles = (H / 16) * (W / 16)
        const f32x4 yv = *(const f32x4*)(obs_n + off);
        f32x4 xv[MCAP];
#pragma unroll
        for (int m = 0; m < MCAP; ++m)
            xv[m] = (EXACT || m < M) ? *(const f32x4*)(fc_n + m * mstride + off) : f32x4{0.f, 0.f, 0.f, 0.f};
        const float y[4] = {yv.x, yv.y, yv.z, yv.w};
        float x[MCAP][4];
#pragma unroll
        for (int m = 0; m < MCAP; ++m) {
            const bool on = EXACT || m < M;
            x[m][0] = on ? xv[m].x : 0.f;
            x[m][1] = on ? xv[m].y : 0.f;
            x[m][2] = on ? xv[m].z : 0.f;
            x[m][3] = on ? xv[m].w : 0.f;
        }
        bool pres[4];
        unsigned long long P[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pres[j] = y[j] >= 0.f;
            P[j] = __ballot(pres[j]);
        }

        // ---- contingency counts at the grid scale: one compare per (threshold, member, pixel), counted by ballot.  misses = wet - hits
        // - (NaN members over wet pixels): x < thr is !(x >= thr) unless x is NaN, which is neither (and rare: a scalar branch) ----
        unsigned long long nan_any[MCAP];
#pragma unroll
        for (int m = 0; m < MCAP; ++m)
            nan_any[m] = (EXACT || m < M) ? __ballot(x[m][0] != x[m][0] || x[m][1] != x[m][1] || x[m][2] != x[m][2] || x[m][3] != x[m][3]) : 0ull;
        for (int k = 0; k < K; ++k) {
            const float tk = thr[k];
            unsigned long long O[4];
            unsigned int wet = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                O[j] = __ballot(pres[j] && y[j] >= tk);
                wet += popc64(O[j]);
            }
#pragma unroll
            for (int m = 0; m < MCAP; ++m) {
                if (EXACT || m < M) {
                    unsigned int hits = 0, reach = 0, nan_wet = 0;  // reach: present pixels where the member reaches the threshold
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned long long ge = __ballot(x[m][j] >= tk);
                        hits += popc64(ge & O[j]);
                        reach += popc64(ge & P[j]);
                    }
                    if (nan_any[m]) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) nan_wet += popc64(__ballot(x[m][j] != x[m][j]) & O[j]);
                    }
                    if (lane < 3)
                        atomicAdd(&s_cont[(k * M + m) * 3 + lane], lane == 0 ? hits : lane == 1 ? wet - hits - nan_wet : reach - hits);
                }
            }
        }

        // ---- rank table: (members below, members tied) per present pixel ----
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int below = 0, tied = 0;
#pragma unroll
            for (int m = 0; m < MCAP; ++m)
                if (EXACT || m < M) {
                    below += x[m][j] < y[j] ? 1 : 0;
                    tied += x[m][j] == y[j] ? 1 : 0;
                }
            const int key = below * (M + 1) + tied;  // < (M + 1)^2: below + tied <= M
            // the key of the first present lane (in a radar field usually everybody's: all dry, all tied) is added once for the wave,
            // the lanes with another key add theirs one by one
            if (P[j]) {
                const int leader = __ffsll((long long)P[j]) - 1;
                const int k0 = __builtin_amdgcn_readlane(key, leader);
                const unsigned long long same = __ballot(pres[j] && key == k0);
                if (lane == leader) atomicAdd(&s_rank[k0], (unsigned int)popc64(same));
                if (pres[j] && key != k0) atomicAdd(&s_rank[key], 1u);
            }
        }

        // ---- level 0: the grid scale ----
        if (want0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v[MCAP];
#pragma unroll
                for (int m = 0; m < MCAP; ++m) v[m] = (double)x[m][j];
                double a, p;
                cell_terms<MCAP, EXACT>(v, (double)y[j], M, a, p);
                acc[0] += pres[j] ? a : 0.0;
                acc[1] += pres[j] ? p : 0.0;
                ncell[0] += popc64(P[j]);
            }
        }
        if (max_lvl < 1) continue;

        // ---- level 1: 2 x 2 cells, two per lane ----
        double sa1[MCAP + 1][2];  // [M] is the observation
        float sm1[MCAP + 1][2];
        int mis1[2];
#pragma unroll
        for (int m = 0; m <= MCAP; ++m) {
            const bool is_obs = m == MCAP;
            if (!(EXACT || m < M || is_obs)) {  // a member that is switched off: zeros, never used by cell_terms
                sa1[m][0] = sa1[m][1] = 0.0;
                sm1[m][0] = sm1[m][1] = 0.f;
                continue;
            }
            const float v0 = is_obs ? y[0] : x[m][0], v1 = is_obs ? y[1] : x[m][1], v2 = is_obs ? y[2] : x[m][2],
                        v3 = is_obs ? y[3] : x[m][3];
            const double c0 = (double)v0 + (double)v1, c1 = (double)v2 + (double)v3;
            sa1[m][0] = c0 + __shfl_xor(c0, 4, 64);
            sa1[m][1] = c1 + __shfl_xor(c1, 4, 64);
            const float m0 = pmax(v0, v1), m1 = pmax(v2, v3);
            sm1[m][0] = pmax(m0, __shfl_xor(m0, 4, 64));
            sm1[m][1] = pmax(m1, __shfl_xor(m1, 4, 64));
        }
        {
            const int a0 = (pres[0] ? 0 : 1) + (pres[1] ? 0 : 1), a1 = (pres[2] ? 0 : 1) + (pres[3] ? 0 : 1);
            mis1[0] = a0 + __shfl_xor(a0, 4, 64);
            mis1[1] = a1 + __shfl_xor(a1, 4, 64);
        }
        if (want1) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bool ok = own1 && mis1[c] == 0;
                double v[MCAP], a, p;
#pragma unroll
                for (int m = 0; m < MCAP; ++m) v[m] = sa1[m][c] * 0.25;
                cell_terms<MCAP, EXACT>(v, sa1[MCAP][c] * 0.25, M, a, p);
                acc[4] += ok ? a : 0.0;
                acc[5] += ok ? p : 0.0;
#pragma unroll
                for (int m = 0; m < MCAP; ++m) v[m] = (double)sm1[m][c];
                cell_terms<MCAP, EXACT>(v, (double)sm1[MCAP][c], M, a, p);
                acc[6] += ok ? a : 0.0;
                acc[7] += ok ? p : 0.0;
                ncell[1] += popc64(__ballot(ok));
            }
        }
        if (max_lvl < 2) continue;

        // ---- levels 2, 3, 4: one cell per lane, shared by 4, 16 and 64 lanes ----
        double sa[MCAP + 1];
        float sm[MCAP + 1];
        int mis;
#pragma unroll
        for (int m = 0; m <= MCAP; ++m) {
            if (!(EXACT || m < M || m == MCAP)) {
                sa[m] = 0.0;
                sm[m] = 0.f;
                continue;
            }
            const double c = sa1[m][0] + sa1[m][1];
            sa[m] = c + __shfl_xor(c, 8, 64);
            const float f = pmax(sm1[m][0], sm1[m][1]);
            sm[m] = pmax(f, __shfl_xor(f, 8, 64));
        }
        mis = mis1[0] + mis1[1];
        mis += __shfl_xor(mis, 8, 64);
#define ENS_LEVEL_TERMS(LVL, OWN, INV)                                   \
    {                                                                    \
        const bool ok = (OWN) && mis == 0;                               \
        double v[MCAP], a, p;                                            \
        _Pragma("unroll") for (int m = 0; m < MCAP; ++m) v[m] = sa[m] * (INV); \
        cell_terms<MCAP, EXACT>(v, sa[MCAP] * (INV), M, a, p);           \
        acc[(LVL) * 4 + 0] += ok ? a : 0.0;                              \
        acc[(LVL) * 4 + 1] += ok ? p : 0.0;                              \
        _Pragma("unroll") for (int m = 0; m < MCAP; ++m) v[m] = (double)sm[m]; \
        cell_terms<MCAP, EXACT>(v, (double)sm[MCAP], M, a, p);           \
        acc[(LVL) * 4 + 2] += ok ? a : 0.0;                              \
        acc[(LVL) * 4 + 3] += ok ? p : 0.0;                              \
        ncell[LVL] += popc64(__ballot(ok));                              \
    }
#define ENS_LEVEL_UP(D_COL, D_ROW)                                       \
    {                                                                    \
        _Pragma("unroll") for (int m = 0; m <= MCAP; ++m) {              \
            if (!(EXACT || m < M || m == MCAP)) continue;                \
            const double c = sa[m] + __shfl_xor(sa[m], D_COL, 64);       \
            sa[m] = c + __shfl_xor(c, D_ROW, 64);                        \
            const float f = pmax(sm[m], __shfl_xor(sm[m], D_COL, 64));   \
            sm[m] = pmax(f, __shfl_xor(f, D_ROW, 64));                   \
        }                                                                \
        mis += __shfl_xor(mis, D_COL, 64);                               \
        mis += __shfl_xor(mis, D_ROW, 64);                               \
    }
        if (want2) ENS_LEVEL_TERMS(2, own2, 0.0625)
        if (max_lvl < 3) continue;
        ENS_LEVEL_UP(1, 16)
        if (want3) ENS_LEVEL_TERMS(3, own3, 0.015625)
        if (max_lvl < 4) continue;
        ENS_LEVEL_UP(2, 32)
        if (want4) ENS_LEVEL_TERMS(4, own4, 0.00390625)
#undef ENS_LEVEL_TERMS
#undef ENS_LEVEL_UP
    }

    // ---- the workgroup's partial row: lanes by butterfly, waves in order ----
#pragma unroll
    for (int q = 0; q < ENS_Q; ++q) {
        double v = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s_part[wave][q] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int l = 0; l < ENS_LEVELS; ++l)
            if (ncell[l]) atomicAdd(&s_cells[l], ncell[l]);
    }
    __syncthreads();
    if (tid < ENS_Q) {
        double v = s_part[0][tid];
#pragma unroll
        for (int w = 1; w < ENS_WAVES; ++w) v += s_part[w][tid];
        ws[(int64_t)blockIdx.x * ENS_Q + tid] = v;
    }
    for (int i = tid; i < n_cont; i += 64 * ENS_WAVES)
        if (s_cont[i]) atomicAdd(&cont[n * n_cont + i], (unsigned long long)s_cont[i]);
    for (int i = tid; i < n_rank; i += 64 * ENS_WAVES)
        if (s_rank[i]) atomicAdd(&ranks[n * n_rank + i], (unsigned long long)s_rank[i]);
    if (tid < ENS_LEVELS && slot_of(lvl_slot, tid) != 0xF && s_cells[tid])
        atomicAdd(&cells[n * S + slot_of(lvl_slot, tid)], (unsigned long long)s_cells[tid]);
}

// One wave per (plane, entry of the partial row): lane l adds the rows l, l + 64, ... of the plane in that order, the lanes meet in a
// xor butterfly.  abs_err is divided by M here, once per plane; at the grid scale the max row is a copy of the avg row.
__global__ __launch_bounds__(64 * ENS_WAVES) void ens_finalize_kernel(const double* __restrict__ ws, int64_t N, int BPP, int M,
                                                                     uint32_t lvl_slot, int S, double* __restrict__ abs_err,
                                                                     double* __restrict__ pair) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * ENS_WAVES + (threadIdx.x >> 6);
    if (item >= N * ENS_Q) return;  // (wave-uniform)
    const int64_t n = item / ENS_Q;
    const int q = (int)(item - n * ENS_Q);
    const int lvl = q >> 2, pool = (q >> 1) & 1, kind = q & 1;
    const int slot = slot_of(lvl_slot, lvl);
    if (slot == 0xF || (lvl == 0 && pool == 1)) return;
    double v = 0.0;
    for (int r = lane; r < BPP; r += 64) v += ws[(n * BPP + r) * ENS_Q + q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane != 0) return;
    double* out = kind == 0 ? abs_err : pair;
    if (kind == 0) v /= (double)M;
    out[(n * 2 + pool) * S + slot] = v;
    if (lvl == 0) out[(n * 2 + 1) * S + slot] = v;
}

template <int MCAP, bool EXACT>
void ens_launch(int blocks, hipStream_t st, const float* fc, int64_t mstride, const float* obs, int M, int W, int tiles_x, int tiles,
                int BPP, uint32_t lvl_slot, int max_lvl, int S, const float* thr, int K, double* ws, int64_t* cells, int64_t* cont,
                int64_t* ranks, int64_t HW) {
    hipLaunchKernelGGL((ens_scores_kernel<MCAP, EXACT>), dim3(blocks), dim3(64 * ENS_WAVES), 0, st, fc, mstride, obs, M, W, tiles_x, tiles,
                       BPP, lvl_slot, max_lvl, S, thr, K, ws, (unsigned long long*)cells, (unsigned long long*)cont,
                       (unsigned long long*)ranks, HW);
}

int ens_check_shape(const char* fn, int M, int64_t N, int H, int W) {
    DGMR_CHECK_ARG(M >= 1 && M <= ENS_MAX_M, "%s: M=%d members, 1 ... %d are supported", fn, M, ENS_MAX_M);
    DGMR_CHECK_ARG(N >= 1 && N <= (1 << 24), "%s: N=%lld planes out of range", fn, (long long)N);
    DGMR_CHECK_ARG(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "%s: H=%d and W=%d must be positive multiples of 16", fn, H, W);
    DGMR_CHECK_ARG((int64_t)H * W <= INT32_MAX, "%s: a plane of %d x %d elements is out of range", fn, H, W);
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

extern "C" int64_t dgmr_ensemble_scores_workspace(int M, int64_t N, int H, int W) {
    if (ens_check_shape("dgmr_ensemble_scores_workspace", M, N, H, W) != 0) return -1;
    return N * ens_blocks_per_plane(N, (H / 16) * (W / 16)) * ENS_Q * (int64_t)sizeof(double);
}

extern "C" int dgmr_ensemble_scores(const float* forecast, int64_t member_stride, const float* observed, int M, int64_t N, int H, int W,
                                    const int* scales, int S, const float* thresholds, int K, void* workspace, int64_t workspace_bytes,
                                    int64_t* cells, double* abs_err, double* pair, int64_t* contingency, int64_t* ranks,
                                    void* stream) {
    if (ens_check_shape("dgmr_ensemble_scores", M, N, H, W) != 0) return -1;
    DGMR_CHECK_ARG(scales && S >= 1 && S <= ENS_LEVELS, "dgmr_ensemble_scores: %d scales, 1 ... %d out of {1, 2, 4, 8, 16} are supported", S,
                   ENS_LEVELS);
    DGMR_CHECK_ARG(K >= 0 && K <= ENS_MAX_K, "dgmr_ensemble_scores: K=%d thresholds, at most %d are supported", K, ENS_MAX_K);
    uint32_t lvl_slot = 0xFFFFF;
    int max_lvl = 0;
    for (int s = 0; s < S; ++s) {
        int lvl = -1;
        for (int l = 0; l < ENS_LEVELS; ++l)
            if (scales[s] == (1 << l)) lvl = l;
        DGMR_CHECK_ARG(lvl >= 0, "dgmr_ensemble_scores: scale %d is not one of 1, 2, 4, 8, 16", scales[s]);
        DGMR_CHECK_ARG(((lvl_slot >> (4 * lvl)) & 0xF) == 0xF, "dgmr_ensemble_scores: scale %d is given twice", scales[s]);
        lvl_slot = (lvl_slot & ~(0xFu << (4 * lvl))) | ((uint32_t)s << (4 * lvl));
        max_lvl = std::max(max_lvl, lvl);
    }
    DGMR_CHECK_ARG(forecast && observed && workspace && cells && abs_err && pair && ranks && ((thresholds && contingency) || K == 0),
                   "dgmr_ensemble_scores: null pointer");
    const int64_t HW = (int64_t)H * W;
    DGMR_CHECK_ARG(M == 1 || (member_stride >= 0 && member_stride % 4 == 0 && member_stride <= INT64_MAX / 4 / ENS_MAX_M),
                   "dgmr_ensemble_scores: member_stride=%lld must be a non-negative multiple of 4 elements", (long long)member_stride);
    DGMR_CHECK_ARG((((uintptr_t)forecast | (uintptr_t)observed) & 15) == 0, "dgmr_ensemble_scores: forecast and observed must be 16-byte aligned");
    DGMR_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "dgmr_ensemble_scores: workspace must be 8-byte aligned");
    const int tiles_x = W / 16, tiles = (H / 16) * tiles_x;
    const int BPP = ens_blocks_per_plane(N, tiles);
    const int64_t need = N * BPP * ENS_Q * (int64_t)sizeof(double);
    DGMR_CHECK_ARG(workspace_bytes >= need, "dgmr_ensemble_scores: workspace of %lld bytes, %lld are needed (dgmr_ensemble_scores_workspace)",
                   (long long)workspace_bytes, (long long)need);
    const int blocks = (int)(N * BPP);  // <= max(N, ENS_TARGET_BLOCKS)
    hipStream_t st = ST;
    if (hipMemsetAsync(cells, 0, (size_t)N * S * sizeof(int64_t), st) != hipSuccess ||
        (K > 0 && hipMemsetAsync(contingency, 0, (size_t)N * K * M * 3 * sizeof(int64_t), st) != hipSuccess) ||
        hipMemsetAsync(ranks, 0, (size_t)N * (M + 1) * (M + 1) * sizeof(int64_t), st) != hipSuccess) {
        dgmr_set_error("dgmr_ensemble_scores: clearing the count outputs failed: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
#define ENS_GO(MCAP, EXACT)                                                                                                           \
    ens_launch<MCAP, EXACT>(blocks, st, forecast, M == 1 ? 0 : member_stride, observed, M, W, tiles_x, tiles, BPP, lvl_slot, max_lvl, S, \
                            thresholds, K, (double*)workspace, cells, contingency, ranks, HW)
    switch (M) {  // the member loops are unrolled: exact instantiations for small ensembles, guarded ones above
        case 1: ENS_GO(1, true); break;
        case 2: ENS_GO(2, true); break;
        case 3: ENS_GO(3, true); break;
        case 4: ENS_GO(4, true); break;
        case 5: ENS_GO(5, true); break;
        case 6: ENS_GO(6, true); break;
        case 7: ENS_GO(7, true); break;
        case 8: ENS_GO(8, true); break;
        default:
            if (M <= 12) ENS_GO(12, false);
            else if (M <= 16) ENS_GO(16, false);
            else if (M <= 24) ENS_GO(24, false);
            else ENS_GO(32, false);
    }
#undef ENS_GO
    hipLaunchKernelGGL(ens_finalize_kernel, dim3(cdiv(N * ENS_Q, ENS_WAVES)), dim3(64 * ENS_WAVES), 0, st, (const double*)workspace, N, BPP, M,
                       lvl_slot, S, abs_err, pair);
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
