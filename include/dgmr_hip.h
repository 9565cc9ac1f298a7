/*
 * dgmr_hip.h — C ABI of libdgmr_hip.so: the MI355X (gfx950) kernels behind the DGMR training step.
 *
 * The reference (openclimatefix/skillful_nowcasting) has NO native code and no FFI: every FLOP of
 * `DGMR.training_step` (dgmr/dgmr.py:137-218) runs inside stock torch ops.  The boundary this library
 * replaces is therefore "the torch op call sites on the hot path" (SURVEY.md §8a); each entry point
 * below names the reference call sites it stands in for.  The Python host side
 * (skillful_nowcasting_amd/_lib.py) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - Activations are fp32, channels-last: NHWC for 2-D, NDHWC for 3-D ("N D H W C"; 2-D == D 1).
 *   - Conv weights are fp32 [Cout][KD][KH][KW][Cin] (a torch OIHW / OIDHW parameter held in
 *     channels_last memory format has exactly this physical layout).
 *   - Cin % 4 == 0 and Cout % 4 == 0 for every conv (true for every conv on the DGMR path; the single
 *     Linear(768 -> 1) heads use dgmr_linear1_*).
 *   - Every buffer (incl. workspaces) is allocated by the caller.  Kernels never allocate, free or
 *     synchronise; every launch goes to the `stream` argument (a hipStream_t passed as void*), so the
 *     calls are graph-capture safe.
 *   - Return value: 0 on success, negative on error; dgmr_last_error() returns a thread-local message.
 */
#ifndef DGMR_HIP_H
#define DGMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGMR_ABI_VERSION 13

int dgmr_abi_version(void);
const char* dgmr_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on v_mfma_f32_32x32x2_f32).
 * Replaces torch.nn.Conv2d / Conv3d forward+backward at every `conv2d(` / `get_conv_layer` call site:
 * dgmr/common.py:43-66,113-137,192-215,266-286,350-384,451-455; dgmr/generators.py:52-56,67-73,84-90,
 * 101-107,115-121; dgmr/layers/ConvGRU.py:29-55; dgmr/layers/Attention.py:38-66 — together with the
 * ops the reference applies around them, fused into the operand load / epilogue:
 *   relu on load            F.relu / nn.ReLU before a conv (common.py:77,80,146,151,230,232,296,298)
 *   affine+relu on load     BatchNorm2d(train) + ReLU before a conv (common.py:76-80,145-151; generators.py:176)
 *   nearest 2x on load      nn.Upsample(scale_factor=2) before a conv (common.py:142,148)
 *   1/sigma epilogue scale  spectral_norm's W/sigma (torch/nn/utils/parametrizations.py:506-521)
 *   residual add            `x2 + sc` (common.py:83,154,237,300)
 * ---------------------------------------------------------------------------------------------- */
typedef struct dgmr_conv_args {
    const float* x;        /* input [N][D][Hin][Win][Cin]; Hin,Win = H,W  (or H/2,W/2 when upsample) */
    const float* w;        /* [Cout][KD][KH][KW][Cin] */
    const float* bias;     /* [Cout] or NULL */
    const float* scale;    /* per-group multiplier (1/sigma): scale[n / scale_group]; NULL = 1 */
    const float* pre_a;    /* NULL, or per-(group,channel) a: x' = relu(x*a+b), [N/pre_group][Cin] */
    const float* pre_b;
    const float* addend;   /* NULL or [M][Cout]: added to the accumulator BEFORE scale */
    const float* residual; /* NULL or [M][Cout]: added after scale+bias */
    const float* mask_src; /* NULL or [M][Cout]: y = (mask_src*mask_a+mask_b > 0) ? y : 0  (relu backward) */
    const float* mask_a;   /* NULL (plain mask_src > 0) or [N/mask_group][Cout] */
    const float* mask_b;
    float* y;              /* output [N][D][H][W][Cout] */
    int32_t N, D, H, W;    /* output extent (== input extent after the optional upsample) */
    int32_t Cin, Cout;
    int32_t KD, KH, KW;    /* each 1 or 3; 'same' zero padding K/2, stride 1 */
    int32_t upsample;      /* 1: x is [N][D][H/2][W/2][Cin], nearest-upsampled on the fly */
    int32_t pre_relu;      /* 1: relu on the input (ignored when pre_a != NULL, which implies relu) */
    int32_t scale_group;   /* samples per scale group (>=1) */
    int32_t pre_group;     /* samples per pre_a/pre_b group */
    int32_t mask_group;
    int32_t act_relu;      /* 1: relu after scale+bias, before the residual add (F.relu(conv(..)), common.py:424) */
    /* -- ABI 3 -- */
    int32_t w_cin;         /* weights are the input-channel slice [w_coff, w_coff+Cin) of a [Cout][KD][KH][KW][w_cin] tensor
                              (the x / h halves of a ConvGRU conv applied to torch.cat([x, h], 1): ConvGRU.py:69,79); 0: dense */
    int32_t w_coff;
    int32_t epi_mode;      /* DGMR_EPI_*: fused tail after scale+bias (replaces act_relu / residual / mask when != PLAIN) */
    int32_t ksplit;        /* out: ignored on input; the library splits K itself when splitk_ws is given and the grid is small */
    const float* gru_h;    /* [M][Cout] previous hidden state (GRU modes) */
    const float* gru_pu;   /* [M][Cout] update-gate pre-activation (DGMR_EPI_GRU_BLEND) */
    float* pre_out;        /* [M][Cout] receives the pre-activation (scale+bias applied) in the GRU modes (needed by the backward);
                              NULL: not stored (forwards without a graph: a fifth of the recurrent step's HBM traffic) */
    float* splitk_ws;      /* NULL, or scratch for split-K partial sums */
    int64_t splitk_ws_bytes;
    const uint16_t* w_split; /* NULL, or the SAME weights (of the slice, if w_cin/w_coff select one) pre-split into dense bf16
                                planes [P][Cout][KH*KW][Cin] by dgmr_split_weights (P = 2 in the modes bf16x3 / bf16, 3 in bf16x6 - the
                                library reads as many planes as the mode set when the launch is issued): lets the bf16 modes run 3x3
                                convs of the big feature maps through the LDS-window kernel */
    int32_t residual_up;     /* 1: residual is [N][H/2][W/2][Cout], added with nearest-2x upsampling (the 1x1 shortcut of an upsampling
                                G-block evaluated before the upsample: conv1x1(up(x)) == up(conv1x1(x)), common.py:142-143,154) */
    int32_t reserved0;       /* must be 0 (library-internal) */
    /* -- ABI 6 -- */
    float* stats_out;        /* NULL, or [dgmr_conv_stats_rows(args)][2][Cout]: per-workgroup-tile partial sums (sum y, sum y^2) of the
                                OUTPUT, one row per pixel tile - the BatchNorm batch statistics of the next layer taken in this conv's
                                epilogue instead of by a second pass over y (GBlock: bn2(first_conv(..)), common.py:76-80,145-151).
                                Rows are ordered like the samples; dgmr_bn_partial_reduce folds them per statistics group.
                                With mask_src (data gradient through relu(BatchNorm(x))) the second sum is sum y * mask_src instead:
                                with dgmr_bn_bwd_center the two sums BatchNorm's backward needs (common.py:76,145 backwards). */
    /* -- ABI 7 -- */
    const uint16_t* w_phase; /* NULL, or (with `upsample`, 3x3, bf16 modes) the tap sums of the four output-pixel parities as bf16 planes
                                [2][4*Cout][2*2][Cin]: dgmr_upsample_phase_weights then dgmr_split_weights.  The upsampling conv of
                                UpsampleGBlock (common.py:142,148) then runs as four 2x2 convs on the low-resolution input - 16 instead of
                                36 multiply steps per input pixel, same sums up to the fp32 rounding of the tap sums. */
    int32_t pool2;           /* 1: y = 2x2 sum pool of the conv, [N][H/2][W/2][Cout] (H, W stay the conv's map; mask_src / stats_out refer to
                                the pooled output) - the data gradient of an upsampling conv (common.py:142,148 backwards) without
                                writing the full-resolution gradient.  Needs w_phase = dgmr_pool2_phase_weights + dgmr_split_weights
                                ([2][Cout][16][Cin]) and a conv the window kernel takes: ask dgmr_conv_pool2_supported.
                                ABI 10: also the FORWARD of a DBlock's last conv + AvgPool (common.py:233-237; tap sums x 0.25): `residual`
                                is then [N][H/2][W/2][Cout]; and 3x3x3 convs (KD = 3, D > 1), plane by plane, w_phase =
                                [2][Cout][3 * 16][Cin] (dgmr_pool2_phase_weights per depth tap): y = [N][D][H/2][W/2][Cout], the 2 x 2
                                spatial half of AvgPool3d - dgmr_pool_depth2 finishes it. */
    int32_t reserved1;
    /* -- ABI 8 -- DGMR_EPI_GRU_GATES2: the ConvGRU's read AND update gate convs in one launch (ConvGRU.py:69-76: both convolve the same
       cat[x, h]); see the define below */
    const float* scale2;     /* 1/sigma of the second (update) gate conv, indexed like `scale` */
    const float* bias2;      /* [gru_split] */
    const float* addend2;    /* [M][gru_split], or NULL */
    float* y2;               /* [M][gru_split]: the update gate's pre-activation */
    int32_t gru_split;       /* C: output columns [0, C) are the read gate's, [C, 2C) the update gate's; Cout == 2 C, C % 4 == 0 */
    /* -- ABI 12 -- */
    int32_t plan_n;          /* 0, or a multiple of N: choose the kernel as for a batch of plan_n samples (groups scaled alike).  A launch
                                on part of a batch then runs the tile variant, window plan and split-K factor - hence the summation order
                                of every output element - that the same samples get inside the whole batch.  Every chip-fill heuristic
                                (window kernel or implicit GEMM, tile width, 256-pixel tiles, streaming 1x1, split-K factor and its
                                workspace cap) reads plan_n; structural requirements (two-image tiles of 8x8 maps: even N and even
                                scale / pre / mask groups) keep reading N, and where one holds for plan_n but not for N the call fails
                                with an argument error naming it - no other kernel is picked. */
} dgmr_conv_args;

/* ---- the sampler's output layer: relu(BatchNorm(x)) -> 1x1 conv to 4 channels (generators.py:159-166), streaming fp32 kernels ----
 * x: [M][C] (C <= 64, % 4); a, b: BatchNorm affine per call group [G][C]; w: [4][C]; scale: 1/sigma per call group [G] or NULL;
 * a call group = pixels_per_group consecutive pixels (M = G * pixels_per_group).  Exact fp32 in every precision mode.
 * dgmr_head_blocks: number of per-block partial rows the backward writes (0: shape unsupported, use the conv entry points). */
int dgmr_head_blocks(int64_t M, int64_t pixels_per_group, int C);
int dgmr_head_fwd(const float* x, const float* a, const float* b, const float* w, const float* bias, const float* scale, float* y,
                  int64_t M, int64_t pixels_per_group, int C, void* stream);
/* Backward pass 1 - the data gradient g = [a x + b > 0] (1/sigma) W^T dy is formed in registers and NOT written: per block
 * bn_partials[blk][2][C] = (sum g, sum g x)  (-> dgmr_bn_partial_reduce, dgmr_bn_bwd_center), w_partials[blk][4][C] = sum dy (x) relu(a x + b)
 * (the raw weight gradient; blocks of a call group are consecutive: dgmr_wgrad_reduce with nsplit = blocks), bias_partials[blk][4]. */
int dgmr_head_bwd_sums(const float* x, const float* a, const float* b, const float* w, const float* scale, const float* dy,
                       float* bn_partials, float* w_partials, float* bias_partials, int64_t M, int64_t pixels_per_group, int C,
                       void* stream);
/* Backward pass 2 - g recomputed, BatchNorm's backward applied (dgmr_bn_bwd_apply's arithmetic), dx written; dgamma / dbeta
 * accumulated from `sums` when given. */
int dgmr_head_bwd_apply(const float* x, const float* a, const float* b, const float* w, const float* scale, const float* dy,
                        const float* mean, const float* rstd, const float* gamma, const double* sums, float* dx, float* dgamma,
                        float* dbeta, int64_t M, int64_t pixels_per_group, int C, int train, void* stream);

/* Weight gradient of an upsampling conv (common.py:142,148 backwards) as a 1x1 problem: z[n][r][c][co*9 + ky*3 + kx] = the sum of the
 * 2x2 pixels of dy ([N][2H][2W][C]) that meet input pixel (r, c) under tap (ky, kx), so that dW[co][ky][kx][ci] = sum over the INPUT
 * pixels of z * pre(x) - dgmr_conv_wgrad with KH = KW = 1, Cout = 9 C, dy = z: a quarter of the multiply steps of the gradient taken
 * on the upsampled map, and its partial[..][co*9 + tap][ci] is the layout dgmr_wgrad_reduce expects.  z: [N][H][W][9 C] floats. */
int dgmr_upsample_wgrad_sums(const float* dy, float* z, int N, int H, int W, int C, void* stream);
/* 1 when dgmr_conv_fwd accepts these arguments with pool2 = 1 (host arithmetic, no launch). */
int dgmr_conv_pool2_supported(const dgmr_conv_args* a);
/* ABI 12: what dgmr_conv_fwd would dispatch for these arguments in the current arithmetic mode - host arithmetic, nothing is launched
 * and no pointer is dereferenced (pointers count as given / NULL and by their 16-byte alignment).  *detail = the dispatch word of the
 * profiler records (dgmr_profile_collect_detail: kernel class, tile, 256-pixel tiles, phase / pooled mode, 3-D, split-K ...), *ksplit =
 * the split-K factor (1: none).  Two argument sets with equal answers run the same kernel with the same reduction order per output
 * element; with plan_n the answer is that of the whole batch.  < 0 on the argument errors dgmr_conv_fwd would report. */
int dgmr_conv_plan(const dgmr_conv_args* a, uint32_t* detail, int32_t* ksplit);
/* out[co][(p*2+q)*4 + a*2+b][ci]: the 4x4 stride-2 kernel of "3x3 conv then 2x2 sum pool" (row u = 2a + 1 - p sums the taps ky with
 * ky + i = u, i in {0,1}), grouped by the parity (p, q) of the input pixel.  w: [Cout][3][3][Cin] fp32; out: [Cout][16][Cin] fp32. */
int dgmr_pool2_phase_weights(const float* w, float* out, int Cout, int Cin, void* stream);

/* out[(py*2+px)*Cout + co][a][b][ci] = sum of w[co][ky][kx][ci] over the taps (ky, kx) that read input pixel (h + py - 1 + a,
 * w + px - 1 + b) when the conv runs on the nearest-2x upsampled map at output pixel (2h + py, 2w + px): ky in {0} | {1,2} for py = 0,
 * a = 0 | 1; {0,1} | {2} for py = 1; kx likewise.  w: [Cout][3][3][Cin] fp32 (channels-last OIHW); out: [4*Cout][2][2][Cin] fp32. */
int dgmr_upsample_phase_weights(const float* w, float* out, int Cout, int Cin, void* stream);
/* 1 when dgmr_conv_fwd accepts these arguments with epi_mode = DGMR_EPI_GRU_GATES2 in the current arithmetic mode (host arithmetic only) */
int dgmr_conv_gates2_supported(const dgmr_conv_args* a);

/* Number of partial-sum rows dgmr_conv_fwd writes to stats_out for these arguments (host arithmetic, no launch): 0 when the kernel
 * the library would dispatch has no fused statistics (only the LDS-window 3x3 kernels of the bf16 modes do), then stats_out must
 * be NULL and the caller takes the statistics with dgmr_bn_stats. */
int dgmr_conv_stats_rows(const dgmr_conv_args* a);

#define DGMR_EPI_PLAIN 0
#define DGMR_EPI_GRU_GATE 1  /* pre_out = v ; y = sigmoid(v) * gru_h                              (ConvGRU.py:69-71,78) */
#define DGMR_EPI_GRU_BLEND 2 /* pre_out = v ; y = s*gru_h + (1-s)*relu(v), s = sigmoid(gru_pu)     (ConvGRU.py:80-84) */
/* Read and update gate of one ConvGRU step fused (ConvGRU.py:69-76): ONE conv with Cout = 2 C output columns whose weights (w_split
 * rows) are the read gate's [0, C) followed by the update gate's [C, 2C) - the input halo (h, or cat[x, h]) is staged once for both.
 * Every tensor of the epilogue has C channels per pixel:
 *   column c <  C:  v = (acc + addend[m][c]) * scale[g] + bias[c];        pre_out[m][c] = v (if given);  y[m][c] = sigmoid(v) * gru_h[m][c]
 *   column c >= C:  v = (acc + addend2[m][c-C]) * scale2[g] + bias2[c-C];  y2[m][c-C] = v
 * Only for convs the LDS-DMA window kernel takes, with 16-byte aligned tensors: ask dgmr_conv_gates2_supported first. */
#define DGMR_EPI_GRU_GATES2 3

/* out[k][i] = bf16(w_i - out[0][i] - ... - out[k-1][i]), k < planes, for the [rows][Cin] slice [w_coff, w_coff+Cin) of a
 * [rows][w_cin] weight matrix (rows = Cout * taps; w_cin == 0: dense).  Cin must be even.  planes: 2 for DGMR_PREC_BF16X3 /
 * DGMR_PREC_BF16, 3 for DGMR_PREC_BF16X6 (three bf16 hold all 24 mantissa bits: the planes sum to w exactly).  Valid until the
 * weights change.  plane_stride: elements between two planes of `out` (0: dense, rows * Cin) - lets several weight tensors share one
 * plane set (the fused ConvGRU gates: the read gate's rows followed by the update gate's).  (ABI 8: `planes`, `plane_stride` added.) */
int dgmr_split_weights(const float* w, uint16_t* out, int64_t rows, int Cin, int w_cin, int w_coff, int planes, int64_t plane_stride,
                       void* stream);

/* Arithmetic of the forward / data-gradient contraction (process-wide; tensors in HBM stay fp32, accumulation is fp32):
 *   DGMR_PREC_F32     exact fp32 on v_mfma_f32_32x32x2_f32 (157 TF peak) -- the parity mode
 *   DGMR_PREC_BF16X3  each operand split into two bf16 terms, 3 x v_mfma_f32_32x32x16_bf16 per product: products carry 16
 *                     significant bits (~2^-16 relative error per product - NOT fp32 arithmetic), 833 TF effective peak
 *   DGMR_PREC_BF16    operands rounded to bf16 (BASELINE.json configs[1]): 2.5 PF peak, ~3 significant digits
 *   DGMR_PREC_BF16X6  (ABI 8) three bf16 terms per operand (exact: 3 x 8 bits = the fp32 mantissa), the six products a_i * b_j with
 *                     i + j <= 2 on six MFMAs: the dropped terms are <= 2^-25 |ab|, below the rounding of an fp32 product -
 *                     fp32-faithful contractions at 417 TF effective peak (2.6 x the exact-f32 MFMA's)
 * A caller may switch the mode between launches (it is read when a launch is issued): the module layer runs the discriminator
 * forward in BF16X6 inside a BF16X3 step (skillful_nowcasting_amd.ops.set_precision). */
#define DGMR_PREC_F32 0
#define DGMR_PREC_BF16X3 1
#define DGMR_PREC_BF16 2
#define DGMR_PREC_BF16X6 3
int dgmr_set_precision(int mode);
int dgmr_get_precision(void);

/* y = act(conv(pre(x), w) (+addend) *scale + bias) (+residual), masked.  Forward AND data-gradient (the
 * latter with dgmr_conv_flip_weights()'ed weights and dy as x). */
int dgmr_conv_fwd(const dgmr_conv_args* a, void* stream);

/* w_t[Cin][KD][KH][KW][Cout] = w[Cout][KD-1-kd][KH-1-kh][KW-1-kw][w_coff + ci]: weights of the transposed
 * (data-gradient) convolution, for the input-channel slice [w_coff, w_coff+Cin) of a tensor with w_cin input channels
 * (w_cin == 0: dense, w_cin = Cin). */
int dgmr_conv_flip_weights(const float* w, float* w_t, int Cout, int Cin, int KD, int KH, int KW, int w_cin, int w_coff,
                           void* stream);

typedef struct dgmr_wgrad_args {
    const float* x;      /* forward input, as in dgmr_conv_args (pre_* / upsample applied on load) */
    const float* dy;     /* [M][Cout] gradient of the conv output (before scale: caller folds scale later) */
    const float* pre_a;
    const float* pre_b;
    float* partial;      /* workspace [nsplit][Cout][K] (K = KD*KH*KW*Cin), written, not accumulated */
    int32_t N, D, H, W, Cin, Cout, KD, KH, KW;
    int32_t upsample, pre_relu, pre_group;
    int32_t nsplit;      /* >= 1: the M = N*D*H*W reduction is cut into nsplit contiguous slabs */
    int32_t groups;      /* >= 1, divides N and nsplit: consecutive N/groups samples form a group (one spectral-norm call:
                            forecast step / frame); a slab never straddles two groups */
    float* bias_grad;    /* NULL, or [Cout]: += column sums of dy (the conv's bias gradient) in the same pass */
    /* -- ABI 11 -- deterministic bias gradient: a workspace of `bias_rows` rows of Cout floats (bias_rows as filled in by
       dgmr_conv_wgrad_plan).  With it every slab's column sums land in a row of their own (or, for the kernels whose workgroups meet
       in a channel, a fixed-order column-sum pass over dy fills the rows) and ONE thread per channel adds the rows up in order:
       bias_grad is bit-identical from run to run.  NULL: the slabs' sums meet in float atomics (any order), whatever
       dgmr_set_deterministic says - the rows are the caller's to provide. */
    float* bias_partial;
    int32_t bias_rows;
    int32_t bias_stride; /* set by the library (0 / Cout); ignored on input */
} dgmr_wgrad_args;

/* Weight-gradient partial sums: partial[s] = dy[slab s]^T * im2col(pre(x))[slab s]. */
int dgmr_conv_wgrad(const dgmr_wgrad_args* a, void* stream);
/* Suggested nsplit (a multiple of groups) for a problem (pure host arithmetic). */
int dgmr_conv_wgrad_nsplit(int M, int Cout, int K, int groups);
/* Same with the whole geometry in view (the kernel choice depends on it): fills a->nsplit from the other fields; the caller then
 * sizes `partial` and calls dgmr_conv_wgrad with the same struct. */
int dgmr_conv_wgrad_plan(dgmr_wgrad_args* a);

/* With P_q = sum of group q's slabs:  g[Cout*K] = sum_q scale[q] * P_q  (scale == NULL: 1);  dot[q] += <P_q, w>  (dot == NULL:
 * skipped; otherwise [groups], zeroed by the caller / the previous finalize).  groups <= 128.
 * ABI 11: `dot` holds dgmr_wgrad_dot_floats(groups) floats - `groups` normally; in deterministic mode groups * (1 + 1024): the
 * workgroups leave their partial dots in rows of their own behind the first `groups` floats and one thread per group adds them up in
 * order (otherwise they meet in float atomics).
 * The slabs are CONSUMED: for narrow weights (numel <= 8192 with at least four slabs per group) a first launch over (group, element
 * block) sums each group's slabs - in the order of the single launch, so the results are the same bits - in place into the group's
 * first slab, and the reduce then reads one slab per group; `partial` must be writable and holds no usable values afterwards. */
int dgmr_wgrad_dot_floats(int groups);
int dgmr_wgrad_reduce(const float* partial, int nsplit, int groups, int64_t numel, const float* w, const float* scale, float* g,
                      float* dot, void* stream);
/* Same for a weight gradient computed on an input-channel slice: partial is [nsplit][Cout][taps][cin_slice]; element
 * (co, tap, ci) is written to / dotted with index (co*taps + tap)*cin_total + coff + ci of g / w.  Two calls (x and h halves)
 * fill one g and accumulate one set of dots. */
int dgmr_wgrad_reduce_slice(const float* partial, int nsplit, int groups, int Cout, int taps, int cin_slice, int cin_total, int coff,
                            const float* w, const float* scale, float* g, float* dot, void* stream);
/* Spectral-norm chain rule (torch/nn/utils/parametrizations.py:515-521), summed over the `groups` calls of the module that
 * one batched launch covered (g already carries the 1/sigma_q factors, see dgmr_wgrad_reduce):
 *   gw[i][k] (+)= g[i][k] - sum_q dot[q]*inv_sigma[q]^2 * u[q][i]*v[q][perm(k)],  then dot[0..groups) = 0.
 * u: [groups][Cout], v: [groups][K] in torch's logical (ci, kd, kh, kw) order; w/g in physical (kd,kh,kw,ci) order.
 * accumulate != 0 adds into gw instead of overwriting.  u == v == NULL: no rank-1 term (plain or scalar-gain conv). */
int dgmr_sn_wgrad_finalize(const float* g, float* gw, float* dot, const float* inv_sigma, const float* u, const float* v,
                           int Cout, int Cin, int taps, int groups, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Spectral-norm power iteration — torch/nn/utils/parametrizations.py:454-521, called on every
 * `spectral_norm(` module forward (list in SURVEY.md §8a row a14).
 * train != 0: u <- normalize(W v), v <- normalize(W^T u) in place (eps-clamped), inv_sigma = 1/(u^T W v).
 * train == 0: inv_sigma = 1/(u^T W v) with the stored u, v.
 * u_save/v_save (may be NULL) receive copies of the u, v used for sigma (needed by the backward).
 * scratch: 4 floats, zero on entry, left zero on exit.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_spectral_sigma(const float* w, float* u, float* v, float* u_save, float* v_save, float* inv_sigma,
                        float* scratch, float* tmp /* [Cout + K] */, int Cout, int Cin, int taps, float eps, int train,
                        void* stream);

/* The T consecutive train-mode calls of a module (a sampler conv is called once per forecast step, a discriminator conv once
 * per frame: generators.py:153-178, discriminators.py:119-133,201-226) in one go, for many modules at once: every spectral-norm
 * call sequence of one generator / discriminator forward (the iterations do not depend on activations).  gram = W W^T
 * [Cout][Cout] (computed by the caller with dgmr_conv_fwd on the [Cout][K] weight matrix, valid until W changes): the T dependent
 * power iterations then run on gram alone and W is read twice instead of 2T times.  Outputs per call t: inv_sigma[t],
 * u_hist[t][Cout], v_hist[t][K] (the vectors sigma_t was computed with); u, v are left at their values after call T.
 * descs: DEVICE array of n descriptors.  Outputs live in one caller-allocated float arena (offsets in floats):
 * inv_sigma[T], u_hist[T][Cout], v_hist[T][K], tmp[3*Cout + T].  row_block0 / col_block0 / iter_block0: exclusive prefix sums of
 * Cout, of ceil(K/64) and of ceil(Cout/32) over the descriptors; the totals are passed alongside.  max_cout: largest Cout (sizes
 * the iteration kernel's LDS), max_T: largest T (the chain runs as max_T + 1 launches, one power iteration of every module each). */
typedef struct dgmr_sn_desc {
    const float* w;
    const float* gram;
    float* u;
    float* v;
    int64_t inv_sigma_off;
    int64_t u_hist_off;
    int64_t v_hist_off;
    int64_t tmp_off;
    int32_t Cout, Cin, taps, T;
    float eps;
    int32_t row_block0, col_block0, iter_block0;
    /* perm[t] (DEVICE array of T ints, or NULL = identity): the group ("slot") of the batched launch that the t-th call of the
     * sequence belongs to.  inv_sigma / u_hist / v_hist are written at slot perm[t]; the module's u, v end at the LAST call's.
     * Batched generator draws run the calls (draw d, step t) as groups [t][d] of one batch while the reference's call order is
     * draw-major (and draw-reversed in the activation-checkpoint recompute, dgmr/dgmr.py:176). */
    const int32_t* perm;
} dgmr_sn_desc;
int dgmr_spectral_sigma_seq_multi(const dgmr_sn_desc* descs_dev, int n, int total_row_blocks, int total_col_blocks,
                                  int total_iter_blocks, int max_cout, int max_T, float* arena, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-channel reductions / BatchNorm — torch.nn.BatchNorm2d (common.py:38-39,108-109; generators.py:113)
 * and BatchNorm1d (discriminators.py:102,194) in train and eval mode.
 * x is [G][R][C] (G groups of R rows); everything is per (group, channel).
 * ---------------------------------------------------------------------------------------------- */
/* sums[g][0][c] += sum_r x ; sums[g][1][c] += sum_r x^2   (double accumulators, zeroed by the caller). */
int dgmr_bn_stats(const float* x, double* sums, int G, int64_t R, int C, void* stream);
/* train: mean/var from sums -> a = gamma*rstd, b = beta - mean*a ; updates running stats once per group (momentum, unbiased
 * var) and num_batches_tracked += G.  The updates are applied in the order order[0], order[1], ... (DEVICE array of G group
 * indices; NULL = 0..G-1): the order in which the reference called the module on those groups.
 * eval (sums == NULL): a,b from running stats (G == 1).  save_mean/save_rstd: [G][C] for the backward. */
int dgmr_bn_finalize(const double* sums, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float* a, float* b, float* save_mean, float* save_rstd, int G,
                     int64_t R, int C, float eps, float momentum, const int32_t* order, void* stream);
/* sums[g][0][c] += sum over the group's rows of partials[row][0][c], sums[g][1][c] likewise: `partials` is what dgmr_conv_fwd wrote to
 * stats_out ([G * rows_per_group][2][C] floats, fp32 sums over one pixel tile each); double accumulation from here on. */
int dgmr_bn_partial_reduce(const float* partials, double* sums, int G, int64_t rows_per_group, int C, void* stream);
/* In place: sums[g][1][c] = rstd[g][c] * (sums[g][1][c] - mean[g][c] * sums[g][0][c]): turns (sum g, sum g * x) - folded by
 * dgmr_bn_partial_reduce from the stats_out rows of a data-gradient conv - into dgmr_bn_bwd_reduce's (sum g, sum g * xhat). */
int dgmr_bn_bwd_center(double* sums, const float* mean, const float* rstd, int G, int C, void* stream);
/* sums[g][0][c] = sum_r g ; sums[g][1][c] = sum_r g * xhat   with xhat = (x-mean)*rstd  (sums zeroed by caller). */
int dgmr_bn_bwd_reduce(const float* gy, const float* x, const float* mean, const float* rstd, double* sums, int G,
                       int64_t R, int C, void* stream);
/* dx = a*(gy - sums0/R - xhat*sums1/R) (+ dx_add); dgamma[c] += sum_g sums1, dbeta[c] += sum_g sums0 (if non-NULL). */
int dgmr_bn_bwd_apply(const float* gy, const float* x, const float* mean, const float* rstd, const float* gamma,
                      const double* sums, const float* dx_add, float* dx, float* dgamma, float* dbeta, int G, int64_t R,
                      int C, int train, void* stream);
/* out[c] (+)= sum_r x[r][c]  (conv / linear bias gradient).  tmp: dgmr_colsum_tmp_doubles(R, C) doubles of scratch, cleared by the
 * call itself. */
int dgmr_colsum(const float* x, float* out, double* tmp, int64_t R, int C, int accumulate, void* stream);
/* The doubles dgmr_colsum(.., R, C, ..) needs behind `tmp`, in the mode that is set when both are called.  Few rows x many columns
 * (R <= 4096 && C >= 4096 && C % 4 == 0) go through a column-parallel kernel, one thread per column quad, that never touches tmp:
 * 2 there (any non-NULL pointer will do).  Otherwise dgmr_reduce_doubles(1, R, C): 2*C, or the deterministic mode's rows.  Both
 * functions decide the path by the same predicate, so a caller that sizes tmp from here never repeats the condition. */
int64_t dgmr_colsum_tmp_doubles(int64_t R, int C);
/* y = x*a[g][c]+b[g][c]  (BatchNorm1d apply; no relu) */
int dgmr_affine(const float* x, const float* a, const float* b, float* y, int G, int64_t R, int C, int relu, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling / resampling / layout — nn.AvgPool2d/3d (common.py:189-191; discriminators.py:68,165),
 * PixelUnshuffle / PixelShuffle (common.py:326; discriminators.py:69,166; generators.py:123),
 * nn.Upsample backward (common.py:121), einops rearrange (common.py:423).
 * ---------------------------------------------------------------------------------------------- */
/* y[N][D/pd][H/2][W/2][C] = mean over pd x 2 x 2 window (pd in {1,2}) (+ addend).  scale overrides 1/window when != 0
 * (scale = 1 gives the sum-pool that is the backward of a nearest upsample).  Optional relu-backward mask on the
 * output: y = (mask_src*mask_a+mask_b > 0) ? y : 0. */
int dgmr_pool_fwd(const float* x, const float* addend, float* y, int N, int D, int H, int W, int C, int pd, float scale,
                  const float* mask_src, const float* mask_a, const float* mask_b, int mask_group, void* stream);
/* dx[N][D][H][W][C] = dy[n][d/pd][h/2][w/2][c] * scale  (scale = 1/window for avg-pool backward). */
int dgmr_pool_bwd(const float* dy, float* dx, int N, int D, int H, int W, int C, int pd, float scale, void* stream);
/* y[N][D/2][plane] = (x[n][2j] + x[n][2j+1]) / 2 (+ addend): the depth half of nn.AvgPool3d(2) (common.py:189) over planes of `plane`
 * floats (H/2 * W/2 * C), when the 2 x 2 spatial half already rode in the 3x3x3 conv that produced x (dgmr_conv_args.pool2).  A last
 * odd plane of x is dropped, like AvgPool3d does. */
int dgmr_pool_depth2(const float* x, const float* addend, float* y, int N, int D, int64_t plane, void* stream);
/* frames [B][T][C][H][W] (reference layout) -> channels-last space-to-depth tiles.
 * out[(b*F+f)][H/(2p)][W/(2p)][4C] with channel (c*4 + dy*2 + dx) (PixelUnshuffle(2) order), frame = idx[f],
 * p = pool ? 2 : 1 (AvgPool2d(2) first).  idx == NULL -> frames 0..F-1.  out_frame_major: 1 -> row (f*B+b).
 * idx is [B / idx_group][F]: samples b .. b + idx_group - 1 share one row of frame indices (idx_group <= 0: one row for all) -
 * several discriminator calls, each with its own random frame draw (discriminators.py:199), batched into one. */
int dgmr_frames_s2d(const float* frames, const int32_t* idx, float* out, int B, int T, int C, int H, int W, int F, int pool,
                    int frame_major, int idx_group, void* stream);
int dgmr_frames_s2d_bwd(const float* dout, const int32_t* idx, float* dframes /* written, every element (ABI 11: gather form, no atomics) */, int B, int T, int C, int H,
                        int W, int F, int pool, int frame_major, int idx_group, void* stream);
/* ABI 12: the same gather from TWO tensors - output sample n reads the sequence made of the Tc frames of context[n % Bc] ([Bc][Tc][C][H][W])
 * followed by the Tf frames of following[n % Bf] ([Bf][Tf][C][H][W]); N % Bc == 0, N % Bf == 0; idx selects among the Tc + Tf frames.
 * torch.cat([images, predictions], dim=1) of dgmr/dgmr.py:186-189 for every generator draw (Bf = N) and the real sequence of every
 * discriminator call (Bf = Bc) without materialising either; per-element arithmetic is dgmr_frames_s2d's.
 * _bwd: the gradient of the following frames alone, dfollowing [N][Tf][C][H][W] (Bf == N), written, every element; the context
 * frames get none. */
int dgmr_frames_s2d_pair(const float* context, const float* following, const int32_t* idx, float* out, int N, int Bc, int Tc, int Bf,
                         int Tf, int C, int H, int W, int F, int pool, int frame_major, int idx_group, void* stream);
int dgmr_frames_s2d_pair_bwd(const float* dout, const int32_t* idx, float* dfollowing, int N, int Tc, int Tf, int C, int H, int W, int F,
                             int pool, int frame_major, int idx_group, void* stream);
/* channels-last [B][h][w][4C] -> frames[b][t][c][2h][2w] (PixelShuffle(2)) and its backward. */
int dgmr_d2s_frames(const float* x, float* frames, int B, int T, int t, int C, int h, int w, void* stream);
int dgmr_d2s_frames_bwd(const float* dframes, float* dx, int B, int T, int t, int C, int h, int w, void* stream);
/* dst[t][n][i] = src[n][t][i], i < inner (inner % 4 == 0): frames of a [N][T][H][W][C] tensor to a frame-major batch
 * (discriminators.py:119-120 `x[:, :, idx]` for every idx at once) and back. */
int dgmr_permute_nt(const float* src, float* dst, int N, int T, int64_t inner, void* stream);
/* Strided channel copy: dst[r][dst_off + c*dst_cstride] (+)= src[r][src_off + c*src_cstride], c < C.
 * Implements torch.cat(dim=1) / channel slicing / "b t c h w -> b (c t) h w" on channels-last tensors. */
int dgmr_copy_channels(const float* src, float* dst, int64_t R, int C, int src_C, int src_off, int src_cstride, int dst_C,
                       int dst_off, int dst_cstride, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ConvGRU gating — dgmr/layers/ConvGRU.py:69-85.
 * ---------------------------------------------------------------------------------------------- */
/* rh = sigmoid(pr) * h */
int dgmr_gru_gate_fwd(const float* pr, const float* h, float* rh, int64_t n, void* stream);
/* dpr = d_rh * h * s*(1-s), dh = d_rh * s  (s = sigmoid(pr)) */
int dgmr_gru_gate_bwd(const float* d_rh, const float* pr, const float* h, float* dpr, float* dh, int64_t n, void* stream);
/* out = s(pu)*h + (1-s(pu))*relu(pc) */
int dgmr_gru_blend_fwd(const float* pu, const float* h, const float* pc, float* out, int64_t n, void* stream);
int dgmr_gru_blend_bwd(const float* dout, const float* pu, const float* h, const float* pc, float* dpu, float* dh, float* dpc,
                       int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Elementwise helpers.
 * ---------------------------------------------------------------------------------------------- */
/* y = x * s[0] * host_scale   (s is a device scalar: an upstream gradient) */
int dgmr_scale_by_dev(const float* x, const float* s, float host_scale, float* y, int64_t n, void* stream);
/* y = alpha*a + beta*b (b may be NULL) */
/* ------------------------------------------------------------------------------------------------
 * (ABI 11) Deterministic mode.  on != 0: every cross-workgroup sum of the step is formed in a fixed order - bias gradients through
 * dgmr_wgrad_args.bias_partial, <P_q, W> through the rows behind `dot`, per-channel statistics (dgmr_bn_stats, dgmr_bn_bwd_reduce,
 * dgmr_colsum, dgmr_bn_partial_reduce, dgmr_grid_cell_loss) through per-workgroup partial rows in the caller's `sums` / `tmp` / `acc`
 * buffer, which then holds dgmr_reduce_doubles(G, R, C) doubles instead of G*2*C.  Two identical runs then give bit-identical
 * parameters and buffers (tests/test_gpu_determinism.py).  Off: those sums meet in float / double atomics. */
int dgmr_set_deterministic(int on);
int dgmr_get_deterministic(void);
/* doubles the caller provides (zeroed) as `sums` / `tmp` / `acc` of a [G][R][C] per-channel reduction: G*2*C, or, in deterministic
 * mode, (1 + nb) * G*2*C with nb = the number of row blocks the library will launch (<= 512, capped so that the buffer stays below 32 MB) */
int64_t dgmr_reduce_doubles(int G, int64_t R, int C);
/* (ABI 11) count += number of non-finite values (NaN, +-Inf) among x[0..n): the opt-in stand-in for the reference's
 * torch.autograd.set_detect_anomaly(True) (dgmr/dgmr.py:130) - parameter gradients are written by kernels here, so autograd's anomaly
 * mode cannot see them.  count: one int32 on the device, accumulated (zero it first). */
int dgmr_nonfinite_count(const float* x, int64_t n, int32_t* count, void* stream);

int dgmr_axpby(const float* a, const float* b, float* y, float alpha, float beta, int64_t n, void* stream);
/* dst[i][:] = src[:] for i < repeat, rows of n floats (n % 4 == 0): einops 'b c h w -> (repeat b) c h w' at b == 1
 * (generators.py:146-148) */
int dgmr_repeat_rows(const float* src, float* dst, int64_t n, int repeat, void* stream);
/* x is [groups][rows][n] (n % 4 == 0): out[g][:] = sum_r w[((g*rows + r) / rows_per_w) * w_stride + col_block] * x[g][r][:] where
 * col_block = column / (n / w_stride) (w_stride 1: one weight per row); w == NULL: plain sums.
 * Sums the per-sample gradients of a ConvGRU whose input is the same latent for every sample and step (generators.py:146-149). */
int dgmr_group_rowsum(const float* x, const float* w, float* out, int groups, int rows, int64_t n, int rows_per_w, int w_stride,
                      void* stream);
/* dst[(k*repeat + r)][:] = src[k][:] for k < nblocks, r < repeat, rows of `block` floats (block % 4 == 0):
 * einops 'k c h w -> (k repeat) c h w' - one latent map per generator draw handed to the `repeat` samples of that draw. */
int dgmr_repeat_interleave(const float* src, float* dst, int64_t nblocks, int64_t block, int repeat, void* stream);
/* dx = (x > 0) ? dy : 0 */
int dgmr_relu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);
int dgmr_fill(float* p, float value, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Latent attention — dgmr/layers/Attention.py:9-20 (attention_einsum).  q, k, v, out are ONE sample,
 * channels-last [H][W][Cq].  The reference hands the NCHW view [Cq][H][W] to an einsum written for
 * "[h w c]": position p = cq*H + y (L = Cq*H of them), feature index = x (length W).  beta: [L][L] saved
 * softmax.  tmp: [L][L] scratch.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_attention_fwd(const float* q, const float* k, const float* v, float* beta, float* out, int Cq, int H, int W,
                       void* stream);
int dgmr_attention_bwd(const float* dout, const float* q, const float* k, const float* v, const float* beta, float* dq,
                       float* dk, float* dv, float* tmp, int Cq, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Discriminator heads — discriminators.py:127-131,217-219: sum_hw(relu(x)), Linear(C -> 1).
 * ---------------------------------------------------------------------------------------------- */
int dgmr_relu_sum_hw_fwd(const float* x, float* y, int N, int HW, int C, void* stream);
int dgmr_relu_sum_hw_bwd(const float* dy, const float* x, float* dx, int N, int HW, int C, void* stream);
/* y[n] = scale[n / scale_group] * <x[n], w> + bias   (scale_group rows per spectral-norm call; <= 0: all N rows) */
int dgmr_linear1_fwd(const float* x, const float* w, const float* bias, const float* scale, float* y, int N, int C,
                     int scale_group, void* stream);
/* dx[n][c] = dy[n]*scale[q]*w[c]; gw_raw[q][c] = sum_{n in group q} dy[n]*x[n][c]; gb = sum_n dy[n]   (q = n / scale_group) */
int dgmr_linear1_bwd(const float* dy, const float* x, const float* w, const float* scale, float* dx, float* gw_raw, float* gb,
                     int N, int C, int scale_group, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Losses — dgmr/losses.py:172-192,307-319; dgmr/dgmr.py:20-33.
 * ---------------------------------------------------------------------------------------------- */
/* loss = mean(relu(1 - real)) + mean(relu(1 + gen)); d_real/d_gen = gradient * gscale */
int dgmr_hinge_disc(const float* s_real, const float* s_gen, float* loss, float* d_real, float* d_gen, int n_real, int n_gen,
                    void* stream);
/* loss = mult * sum_i |mean_k pred_k[i] - y[i]| * w[i];  pred_k = preds + k*pred_stride;  w = weights (explicit, [n]) or, when
 * weights == NULL, the reference's default weight_fn max(y[i]+1, cap) (dgmr/dgmr.py:20-33) evaluated in the kernel.
 * acc: one double, zero on entry, left zero.  dweight[i] (optional) = sign(.)*w/K, the per-prediction gradient / mult. */
/* (ABI 11) doubles behind `acc` (zeroed by the caller): 1, or in deterministic mode 1 + the number of workgroups of the launch */
int64_t dgmr_grid_cell_acc_doubles(int64_t n);
int dgmr_grid_cell_loss(const float* preds, int K, int64_t pred_stride, const float* target, const float* weights, float cap,
                        double* acc, float* loss, float mult, float* dweight, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adam — torch.optim.Adam as constructed at dgmr/dgmr.py:292-300 (eps 1e-8, no weight decay, no amsgrad).
 * ---------------------------------------------------------------------------------------------- */
/* Hyper-parameters travel as doubles: torch forms 1 - beta, lr / (1 - beta1^step) and sqrt(1 - beta2^step) in double and rounds
 * each to float once; the kernel does the same (lerp for the first moment, as torch's foreach implementation). */
int dgmr_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
              int step, void* stream);
/* (ABI 9) All tensors of one optimiser (dgmr/dgmr.py:292-300: one Adam per network) in ONE launch.  descs: device array, one entry per
 * tensor in ascending block0 order; block0 = first workgroup of the tensor when every tensor gets ceil(n / dgmr_adam_chunk())
 * workgroups; step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) rounded from double by the caller, as dgmr_adam
 * forms them (torch keeps one step counter per parameter: they travel per tensor).  Same arithmetic per element as dgmr_adam.
 * descs may point INTO a larger table (one parameter group's slice), as for dgmr_adam_multi_guarded: workgroup 0 of the launch is
 * block descs[0].block0; total_blocks counts this slice's only. */
typedef struct dgmr_adam_desc {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    int32_t block0;
    float step_size;
    float bc2_sqrt;
    int32_t reserved;
} dgmr_adam_desc;
int dgmr_adam_chunk(void);
int dgmr_adam_multi(const dgmr_adam_desc* descs, int n_tensors, int total_blocks, double beta1, double beta2, double eps, void* stream);

/* (ABI 13) Gradient guard: the global L2 norm of one optimiser's gradients, torch.nn.utils.clip_grad_norm_'s coefficient and a
 * "skip this update on NaN / Inf" flag, all formed on the device (no host synchronisation) from ONE extra read of the gradients.
 * The record lives in device memory; dgmr_grad_norm_multi fills it and dgmr_adam_multi_guarded reads it. */
typedef struct dgmr_grad_guard {
    float total_norm;      /* sqrt(sum over tensors of sum g^2): squares and sums in double, rounded to float once */
    float clip_coef;       /* min(1, max_norm / (total_norm + 1e-6f)) formed in float as torch does (NaN stays NaN); 1 when clipping is off */
    int32_t skipped;       /* 1 if skip_nonfinite and total_norm is not finite, else 0 */
    int32_t skipped_total; /* running count: every call adds `skipped` to it (the caller zeroes it once) */
} dgmr_grad_guard;
/* Replaces torch.nn.utils.clip_grad_norm_'s norm (torch/nn/utils/clip_grad.py: vector_norm per tensor, vector_norm of the stack,
 * max_norm / (total_norm + 1e-6) clamped to 1).  descs / n_tensors / total_blocks: the table of the Adam launch(es) of the same step,
 * over EVERY tensor the norm runs over (block0 ascending from 0); only g, n and block0 are read.  g needs 4-byte alignment only
 * (views into a flat gradient buffer).  partials (total_blocks doubles) receives one sum of squares per workgroup, tensor_sq
 * (n_tensors doubles) the per-tensor sums of squares; both are overwritten.  Three launches: per workgroup, per tensor, total.
 * Deterministic: no atomics and no arrival-order ticket - the association order of every sum depends on the tensor lengths and the
 * element index only, not on pointer alignment, so separate gradient tensors and views into a flat buffer give the same bits.
 * The sum of squares (fp32 squares are exact in double and cannot overflow it) is non-finite exactly when a gradient element is:
 * the pass is also the NaN / Inf detector.  max_norm <= 0: no clipping (clip_coef = 1). */
int dgmr_grad_norm_multi(const dgmr_adam_desc* descs, int n_tensors, int total_blocks, double* partials, double* tensor_sq,
                         double max_norm, int skip_nonfinite, dgmr_grad_guard* guard, void* stream);
/* dgmr_adam_multi (torch.optim.Adam as constructed at dgmr/dgmr.py:292-300) on the gradient g * guard->clip_coef (one float product
 * per element, what clip_grad_norm_'s g.mul_(coef) stores); g itself is not rewritten.  guard->skipped != 0: nothing is stored.
 * clip_coef == 1 reproduces dgmr_adam_multi bit for bit.  descs may point INTO a larger table (one parameter group's slice of the
 * table dgmr_grad_norm_multi read): workgroup 0 of the launch is block descs[0].block0; total_blocks counts this slice's only. */
int dgmr_adam_multi_guarded(const dgmr_adam_desc* descs, int n_tensors, int total_blocks, double beta1, double beta2, double eps,
                            const dgmr_grad_guard* guard, void* stream);

/* (added under ABI 13: new symbols only) Exponential moving average of the weights inside the Adam launch.  Stands for
 * torch.optim.swa_utils.get_ema_multi_avg_fn(decay), i.e. Tensor.lerp_(param, 1 - decay) on every shadow after the optimiser step:
 * e = w < 0.5f ? fmaf(w, p_new - e, e) : p_new - (p_new - e) * (1.f - w) (at::lerp), with p_new the float this launch has just stored
 * to p and w = (float)ema_weight = 1 - decay, formed in double by the caller and rounded once here.  ema: device array of n_tensors
 * pointers parallel to descs (a shadow has its parameter's length and element order); a NULL entry leaves that tensor without an
 * average.  guard == NULL: p, m, v come out as from dgmr_adam_multi; otherwise as from dgmr_adam_multi_guarded (g * clip_coef; a
 * skipped step stores nothing, to the shadows either) - bit for bit in both cases.  descs / ema may be the matching slices of larger
 * tables, as for dgmr_adam_multi_guarded.  ema_weight outside [0, 1] (or NaN) is refused. */
int dgmr_adam_multi_ema(const dgmr_adam_desc* descs, float* const* ema, int n_tensors, int total_blocks, double beta1, double beta2,
                        double eps, double ema_weight, const dgmr_grad_guard* guard, void* stream);
/* The evaluation swap: exchanges the contents of descs[i].p and ema[i] for every i in one launch (what evaluating
 * swa_utils.AveragedModel.module instead of the model does, in place: the parameters keep their addresses).  Reads only p, n and
 * block0 of each descriptor; NULL entries of ema are skipped.  Twice is the identity.  The caller invalidates whatever it caches
 * from the parameters. */
int dgmr_swap_multi(const dgmr_adam_desc* descs, float* const* ema, int n_tensors, int total_blocks, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Importance-sampled training crops from full frames (data.py: ImportanceCropLoader).  New symbols, same ABI version.
 * Both entry points read `frames` as ONE sequence [T][H][W][C], channels last as rows arrive, in its storage dtype; only element
 * alignment of `frames` is assumed.  The physical value of an element is x = fadd_rn(fmul_rn((float)raw, scale), offset): two
 * separately rounded fp32 operations, never an fma (torch's raw.float() * scale + offset, bit for bit).  An element is MISSING when
 * !(x >= 0.f): negative, -inf or NaN.  Argument errors (unknown dtype, crop % cell != 0, H < crop, W < crop, non-positive extents or
 * sat_scale, null pointers) return < 0 and set dgmr_last_error() before any launch.
 * ---------------------------------------------------------------------------------------------- */
#define DGMR_DT_U8 0
#define DGMR_DT_I16 1
#define DGMR_DT_F16 2
#define DGMR_DT_F32 3
/* scores[gy][gx] = sum over t, c and the crop x crop pixels with top-left (gy*cell, gx*cell) of  -expm1(-(double)x / sat_scale)
 * (missing elements contribute 0);  missing[gy][gx] = number of missing elements in the same box.
 * Gy = (H - crop)/cell + 1, Gx = (W - crop)/cell + 1; crop % cell == 0; H, W >= crop; a remainder of H or W beyond the last full cell is
 * never covered.  cell_sums [H/cell][W/cell] doubles and cell_missing [H/cell][W/cell] int32: caller's workspace, overwritten.
 * Terms and sums are doubles added in an order that depends on indices only: two launches give the same bits, and a host evaluation
 * of the same formula agrees to summation order (~1e-13), so that an accept decision u < q falls the same way on both. */
int dgmr_crop_scores(const void* frames, int dtype, int T, int H, int W, int C, float scale, float offset, double sat_scale,
                     int cell, int crop, double* cell_sums, int32_t* cell_missing, double* scores, int32_t* missing, void* stream);
/* out[n][t][c][i][j] = x(frames[t][y_n + i][x_n + j][c]) for the N origins (y_n, x_n) in `origins` (device, [N][2] int32), fp32, the
 * model's layout.  clamp_missing != 0: missing elements are written as missing_fill.  N == 0: no launch, returns 0.  Every load is
 * guarded: an element outside the frame (an origin outside [0, H - crop] x [0, W - crop]) is written as missing_fill. */
int dgmr_crop_gather(const void* frames, int dtype, int T, int H, int W, int C, const int32_t* origins, int N, int crop,
                     float scale, float offset, int clamp_missing, float missing_fill, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tiled full-frame nowcasts (tiling.py: nowcast_tiled, DGMR.nowcast_full_frame).  New symbol, same ABI version.
 * One tile's forecast pred [planes][tile][tile] is added, weighted, into the frame out [planes][H][W] (planes = K * T * C) at the
 * tile's top-left corner (oy, ox).  For every (p, i, j):
 *     out[p][oy + i][ox + j] = fmaf(wy[i] * wx[j], pred[p][i][j], out[p][oy + i][ox + j])
 * with the product wy[i] * wx[j] rounded to fp32 FIRST (one fmul_rn, then one fma).  wy, wx: `tile` floats each, the separable
 * blending weights of this tile (tiling.py: blend_weights; over the tiles that cover a pixel they sum to one).  Nothing outside
 * the tile's rectangle is read or written, and there are no atomics: the launches of one nowcast go to one stream in raster order,
 * so the sum at a pixel is formed in that order and two runs give the same bits.  Rows are moved in 16-byte pieces: tile, ox and W
 * are multiples of 4 and pred, out, wx are 16-byte aligned.  Argument errors (null pointers, non-positive extents, tile / ox / W not
 * multiples of 4, a misaligned pointer, a tile that is not inside the frame: oy < 0, oy + tile > H, ox < 0, ox + tile > W) return
 * < 0 and set dgmr_last_error() before any launch.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_tile_blend(const float* pred, float* out, const float* wy, const float* wx, int64_t planes, int tile, int H, int W,
                    int oy, int ox, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ensemble verification (verification.py: ensemble_scores, NowcastVerifier).  New symbols, same ABI version.
 * forecast: M members of N planes [H][W], fp32; member m starts at forecast + m * member_stride (elements), its planes are
 * contiguous ([N][H][W]).  observed: [N][H][W] fp32 in the same unit; an observed element is MISSING when !(y >= 0.f) (negative,
 * -inf, NaN: the loader's rule); forecast values are taken as they are.  scales: S distinct values out of {1, 2, 4, 8, 16} (HOST
 * array, read during the call); thresholds: K <= 8 floats on the DEVICE.  Per plane n, with a cell of scale s being one of the
 * non-overlapping s x s blocks (stride s) whose s * s observed elements are all present, x_m / y its pooled member / observation
 * (pool 0: the float64 sum of the s * s fp32 values / (s * s), formed as (top-left + top-right) + (bottom-left + bottom-right) level by
 * level; pool 1: the maximum):
 *   cells[n][si]              int64   number of cells of scales[si]
 *   abs_err[n][pool][si]      double  sum over cells of (1 / M) sum_m |x_m - y|
 *   pair[n][pool][si]         double  sum over cells of sum_{m<k} |x_m - x_k|      (at scale 1 the two pool rows are the same bits)
 *   contingency[n][k][m][3]   int64   over present pixels: hits (x >= thr_k, y >= thr_k), misses (x < thr_k, y >= thr_k), false
 *                                     alarms (x >= thr_k, y < thr_k); fp32 comparisons
 *   ranks[n][b][e]            int64   present pixels with b = #{m: x_m < y} and e = #{m: x_m == y}; [M + 1][M + 1]
 * Every element of forecast and observed is read once (16-byte loads: both pointers 16-byte aligned, member_stride % 4 == 0, H and W
 * multiples of 16); besides the outputs only `workspace` is written: dgmr_ensemble_scores_workspace(M, N, H, W) bytes (8-byte aligned;
 * < 0 for a shape the call would refuse) of per-workgroup float64 partials, which a second small launch adds in index order - no
 * floating-point atomics, two calls give the same bits; the integer counts are added with integer atomics onto outputs the call
 * clears first.  Runs on `stream`, does not synchronise.  Argument errors (null pointers, M outside 1 ... 32, H or W not a multiple of
 * 16, a scale outside the set or given twice, K > 8, misaligned pointers or stride, a workspace that is too small) return < 0 and set
 * dgmr_last_error() before anything is enqueued.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgmr_ensemble_scores_workspace(int M, int64_t N, int H, int W);
int dgmr_ensemble_scores(const float* forecast, int64_t member_stride, const float* observed, int M, int64_t N, int H, int W,
                         const int* scales, int S, const float* thresholds, int K, void* workspace, int64_t workspace_bytes,
                         int64_t* cells, double* abs_err, double* pair, int64_t* contingency, int64_t* ranks, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Radially averaged power spectral density (spectra.py: radial_psd, SpectrumVerifier).  New symbols, same ABI version.
 * x: N planes [H][W] of fp32, plane n at x + n * plane_stride (elements; >= H * W, a multiple of 4), rows contiguous, x 16-byte
 * aligned.  A plane is cut into (H / L) x (W / L) non-overlapping L x L windows, L one of 32, 64, 128, 256, 512; windows are numbered
 * row-major over [N][H / L][W / L].  Per window: an element is MISSING when !(x >= 0.f) (the loader's rule), is read as 0 and counted
 * in missing[window]; F = fft2(window), unnormalised, NO window function and NO detrending; with integer frequencies kx, ky in
 * {-L/2 ... L/2 - 1} a mode belongs to bin r = round(sqrt(kx^2 + ky^2)), found in integers (r (r - 1) < kx^2 + ky^2 <= r (r + 1));
 *   power[window][r]  double  sum of |F|^2 over the modes of bin r, r = 0 ... L / 2 - 1 (modes with r >= L / 2 - the corners, the
 *                             Nyquist row and column - are dropped).  Sums, not means: the mode counts depend on L alone.
 * fp32 transforms (radix 2, twiddles from a table computed in double), |F|^2 formed in fp32 and added in float64; the input's
 * Hermitian symmetry is used (half spectrum, kx > 0 counted twice).  L <= 128: one workgroup per window, everything in LDS.  L >= 256:
 * a row pass writes the transposed half spectrum of a round of windows to the workspace, a column pass transforms and bins it, a
 * small launch adds the column workgroups' bin partials in index order.  workspace (16-byte aligned): a 2 KiB twiddle table plus,
 * for L >= 256, 4 L^2 + 8 (L / 2) (L / 2 / c) bytes per window of a round (c = 32 columns per workgroup at 256, 16 at 512).
 * dgmr_radial_psd_workspace returns what the whole call would use, capped at 64 MiB (+ the table; < 0 for a shape the call would
 * refuse); any workspace of at least dgmr_radial_psd_workspace(1, L, L, L) bytes is accepted and only sets how many windows a round
 * takes - the results are the same bits for every workspace size, and two calls give the same bits (no floating-point atomics).
 * Runs on `stream`, does not synchronise.  Argument errors (null pointers, L outside the set, H or W not a multiple of L, N < 1,
 * misaligned pointer or stride, a workspace below the one-window need) return < 0 and set dgmr_last_error() before anything is
 * enqueued.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgmr_radial_psd_workspace(int64_t N, int H, int W, int L);
int dgmr_radial_psd(const float* x, int64_t plane_stride, int64_t N, int H, int W, int L, void* workspace, int64_t workspace_bytes,
                    double* power, int64_t* missing, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exceedance table (value.py: exceedance_table, ValueVerifier).  New symbol, same ABI version.
 * forecast, member_stride, observed, M, N, H, W, thresholds, K: as in dgmr_ensemble_scores, with the same missing rule, fp32
 * comparisons, alignment rules and refusals (1 <= M <= 32, H and W multiples of 16, K <= 8 thresholds on the DEVICE).
 *   table[n][k][j][o]  int64  present pixels of plane n at which exactly j of the M members are >= thr_k and the observation is
 *                             (o = 1) or is not (o = 0) >= thr_k; [N][K][M + 1][2]
 * One streaming read of the ensemble and the observation (16-byte loads), a per-workgroup integer histogram in LDS, integer atomics
 * onto a table the call clears first: exact, independent of the order, no workspace.  K = 0 enqueues nothing.  Runs on `stream`,
 * does not synchronise.  Argument errors return < 0 and set dgmr_last_error() before anything is enqueued.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_exceedance_table(const float* forecast, int64_t member_stride, const float* observed, int M, int64_t N, int H, int W,
                          const float* thresholds, int K, int64_t* table, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fractions skill score sums (fss.py: fss_sums, FractionsVerifier; csrc/fss.hip).  New symbol, same ABI version.
 * forecast, member_stride, observed, M, N, H, W, thresholds, K: as in dgmr_exceedance_table, with the same missing rule (an observed
 * element is missing when !(y >= 0); at a missing pixel neither the observation nor any member is an event; NaN reaches no threshold),
 * fp32 comparisons, alignment rules and refusals, but 1 <= K <= 8.  radii: S host integers, 1 <= S <= 8, distinct, 0 <= r <= 32, in
 * any order; the neighbourhood of a pixel is the (2 r + 1)^2 square centred on it, the plane zero-padded outside, and every pixel of
 * the plane is a window centre.  With I_m = present & (x_m >= thr_k), I_o = present & (y >= thr_k), S_m = box_r(I_m), S_o = box_r(I_o)
 * and S_f = sum_m S_m (integers; the (2 r + 1)^2 normalisation is never applied):
 *   sums[n][k][s][4]  int64  sum over the centres of plane n of  S_f^2,  S_o^2,  S_f S_o,  sum_m S_m^2
 *   events[n][k][2]   int64  sum_m sum_pixels I_m,  sum_pixels I_o
 * One workgroup per 64 x 64 tile of centres and group of thresholds: the tile and a halo of the largest radius are staged in LDS as
 * one bit per (threshold, field, pixel) by wave ballots, box sums are popcounts of row windows and a running vertical sum, products and
 * sums are integers (64-bit accumulators), added to outputs the call clears first with 64-bit integer atomics: exact, independent of
 * the order, no workspace, two calls give the same bits.  Runs on `stream`, does not synchronise.  Argument errors (null pointers, M
 * outside 1 ... 32, H or W not a multiple of 16, K or S outside 1 ... 8, a radius outside 0 ... 32 or given twice, misaligned pointers
 * or stride, M^2 (2 R + 1)^4 H W >= 2^63 with R the largest radius: a conservative bound of every sum) return < 0 and set
 * dgmr_last_error() before anything is enqueued.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_fss_sums(const float* forecast, int64_t member_stride, const float* observed, int M, int64_t N, int H, int W,
                  const float* thresholds, int K, const int* radii, int S, void* sums, void* events, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The advection baseline (advection.py; csrc/advect.hip).  New symbols, same ABI version.
 *
 * Block matching (TREC) between two frames.  prev, next: N fp32 planes of H x W, plane_stride elements apart; an element with
 * !(x >= 0) is missing and read as 0.  Blocks of block x block pixels with their top-left corners at (by stride, bx stride) on the
 * lattice By = (H - block) / stride + 1 by Bx = (W - block) / stride + 1; what of `next` lies beyond the last block is never read.
 *   wet[n][by][bx]      int32  elements of the `next` block (missing ones as 0) that are >= wet_threshold, compared in fp32
 *   disp[n][by][bx][2]  int32  (dy, dx), |dy|, |dx| <= radius: the candidate of least cost.  d is a candidate when the displaced block
 *                              prev[y0 - dy ...][x0 - dx ...] lies wholly inside the H x W frame; its cost is the sum over the block
 *                              of (next[y0 + i][x0 + j] - prev[y0 - dy + i][x0 - dx + j])^2, fp32, fmaf in row-major pixel order by
 *                              one thread.  Ties: the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx.
 *   cost[n][by][bx][5]  fp32   the minimum, then the costs at (dy - 1, dx), (dy + 1, dx), (dy, dx - 1), (dy, dx + 1); +inf where that
 *                              neighbour is no candidate
 * A block with wet < min_wet is dry: no search, disp = (0, 0), all five costs +inf.  One workgroup per (plane, block), the block and
 * the (block + 2 radius)^2 window of `prev` staged in LDS once; two launches give the same bits.  Supported: block 16 or 32,
 * 1 <= stride <= block, 1 <= radius <= 16, H, W >= block, N >= 1, min_wet >= 0; everything else and null pointers return < 0 and set
 * the error message before anything is enqueued.  No alignment demands.  Runs on `stream`, does not synchronise.
 *
 * Semi-Lagrangian extrapolation of x (N planes of H x W, x_plane_stride apart; missing elements read as 0) along a motion field for
 * T lead times in one launch.  field[n][gy][gx][2] = (vy, vx) in pixels per step at pixel (origin + gy spacing, origin + gx spacing),
 * field_plane_stride elements per plane (0: one field for all planes).  v(p): bilinear interpolation of the lattice, positions
 * clamped to its extent (Gy = Gx = 1: a uniform field).  s(p): bilinear interpolation of x, a tap outside the frame is 0.
 *   D_0 = 0;  D_t(p) = D_(t-1)(p) + v(p - D_(t-1)(p));  out[n][t - 1][p] = s(p - D_t(p)),  t = 1 ... T,
 * written to out + n out_plane_stride + (t - 1) out_step_stride + y W + x: every lead time interpolates the source once.  Every
 * interpolation is a + f (b - a) with one fma, so an integer displacement copies the source bit for bit.  Against exact arithmetic
 * the result is within  c T max(H, W) 2^-24 A + 4 * 2^-24 max|x|,  A the largest difference of adjacent elements of x, c = 22 the
 * rounded fp32 operations per step in the position arithmetic of both axes (advect.hip lists them), for fields that change by less
 * than 1 / (4 T) pixels per pixel and displacements that stay below max(H, W).  1 <= T <= 64, spacing > 0, Gy, Gx >= 1; 16-byte
 * stores are used when W, out and its two strides allow them and 4-byte stores otherwise: no alignment demands.  Argument errors
 * return < 0 and set the error message before anything is enqueued.  Runs on `stream`, does not synchronise.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_block_match(const float* prev, const float* next, int64_t plane_stride, int64_t N, int H, int W, int block, int stride, int radius,
                     float wet_threshold, int min_wet, int32_t* disp, float* cost, int32_t* wet, void* stream);
int dgmr_advect(const float* x, int64_t x_plane_stride, const float* field, int64_t field_plane_stride, int64_t N, int H, int W, int Gy,
                int Gx, float origin, float spacing, int T, float* out, int64_t out_plane_stride, int64_t out_step_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lucas-Kanade refinement of a block match (advection.py: lk_refine, motion_field(subpixel="lk"); csrc/advect.hip).  A new symbol,
 * same ABI version.
 *
 * prev, next, plane_stride, N, H, W, block, stride: dgmr_block_match's, and disp[n][by][bx][2], cost[n][by][bx][5] its results for
 * them.  Per plane and block with corner (y0, x0) = (by stride, bx stride), integer match d0 = disp and Q = next (missing as 0), over
 * the block's interior I = {(y0 + i, x0 + j): 1 <= i, j <= block - 2}:
 *   g = (gy, gx)   central differences of Q, 0.5 (Q[y + 1][x] - Q[y - 1][x]) and the same along x (fp32; every tap inside the block)
 *   G = sum_I g g^T, (lambda_min, lambda_max) = (tr -+ sqrt(max(tr^2 - 4 det, 0))) / 2 in float64
 *   the block is conditioned when lambda_min > 0 and lambda_min >= eig_ratio lambda_max
 *   d = d0; `iterations` times, for a conditioned block:  r(p) = Q(p) - s(p - d), s the bilinear interpolation of prev (a + f (b - a)
 *     with one fma, x then y, as dgmr_advect; elements outside the frame and missing ones are 0);  b = -sum_I g r;
 *     delta = G^-1 b (float64, closed form);  d <- clip(d + delta, d0 - 1, d0 + 1) per axis, kept as fp32
 *   v[n][by][bx][2]      fp32     d (d0 for a block that is not conditioned)
 *   eig[n][by][bx][2]    float64  (lambda_min, lambda_max)
 *   residual[n][by][bx]  float64  sum_I r^2 at the final d
 * A block whose cost[...][0] is not finite is dry: v = (0, 0), eig = (0, 0), residual = +inf, nothing staged.  One workgroup of 256
 * threads per (plane, block); the block and the (block + 2)^2 window of prev around the match staged in LDS once (d never leaves
 * d0 +- 1, so no tap leaves the window; any int32 in disp is safe, a window outside the frame reads as 0); every sum is fp32 fmaf
 * per thread over its at most four pixels, then float64 in a fixed order over lanes and waves - no atomics, two launches give the
 * same bits.  A match that is exact at an integer (r = 0 on I) returns v = d0 bit for bit and residual = 0.  Supported: block 16 or
 * 32, 1 <= stride <= block, H, W >= block, N >= 1, 1 <= iterations <= 16, eig_ratio >= 0 and finite; everything else and null
 * pointers return < 0 and set the error message before anything is enqueued.  No alignment demands.  Runs on `stream`, does not
 * synchronise.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_lk_refine(const float* prev, const float* next, int64_t plane_stride, int64_t N, int H, int W, int block, int stride,
                   const int32_t* disp, const float* cost, int iterations, float eig_ratio, float* v, double* eig, double* residual,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * The stochastic advection ensemble (stochastic.py; csrc/spectral_ar.hip, csrc/advect.hip).  New symbols, same ABI version.
 *
 * dgmr_spectral_ar: an AR(1) process per Fourier mode of overlapping L x L windows, L one of 32, 64, 128, blended to full planes.
 * z0: P fp32 planes [H][W], z0_plane_stride apart, any real values (no missing-value rule).  white: plane n = p M + m of lead time t
 * at white + n white_member_stride + (t - 1) white_step_stride; out likewise with its two strides.  rho: L fp32 values in [-1, 1].
 * H and W multiples of L, 1 <= T <= 64.  Windows in four classes (cy, cx), cy, cx in {0, 1}: the origins of a class are
 * (i L + cy L / 2, j L + cx L / 2), i < H / L - cy, j < W / L - cx.  Per window and member, with U = fft2(z0 patch), A = |U| / L,
 * X_0 = U and Wh_t = fft2(white patch of lead t):
 *   X_t(k) = rho[r(k)] X_(t-1)(k) + sqrt(1 - rho[r(k)]^2) A(k) Wh_t(k),   x_t = real(ifft2(X_t)),   t = 1 ... T,
 * r(k) the radial bin of dgmr_radial_psd (r (r - 1) < kx^2 + ky^2 <= r (r + 1) over the signed frequencies in [-L/2, L/2); r < L).
 * Blend weights per axis, multiplied: an offset window (class index 1 on the axis) has h(i) = sin^2(pi (i + 1/2) / L) at local
 * index i, computed in double and rounded to fp32; an aligned window has 1 - h(i') (fp32), i' the pixel's index in the offset
 * window that covers it on that axis, and 1 in the outer L / 2 of the frame where there is none.  out[n][t - 1] = the weighted sum
 * of the at most four windows over a pixel.  fp32 radix-2 transforms in LDS (the PSD's forward DIF with the Nyquist column carried,
 * a DIT from the bit-reversed positions back), the window's spectrum and noise amplitudes in registers through the T steps,
 * sqrt(1 - rho^2) formed in double.  One workgroup per (plane, member, window); four launches, one per class in the order (0,0),
 * (0,1), (1,0), (1,1): the first stores, the others read, add (one fma) and write, and windows of a class are disjoint - no atomics,
 * two calls give the same bits.  16-byte accesses when pointers and strides allow them (z0 and white together, out on its own),
 * 4-byte accesses otherwise.  Argument errors (null pointers, L outside the set, H or W not a multiple of L, T outside 1 ... 64, a
 * white or out stride below H * W) return < 0 and set dgmr_last_error() before anything is enqueued.  Runs on `stream`, does not
 * synchronise.
 *
 * dgmr_advect_series: dgmr_advect with a source of its own per lead time - lead t of plane n samples
 * x + n x_plane_stride + (t - 1) x_step_stride - and with plane n reading field plane n / field_group (the members of an ensemble
 * share their case's motion).  Every source value below 0 (or NaN) reads as 0.  Everything else - the D_t recursion, the arithmetic,
 * the store widths, the bound with A and max|x| taken over all steps' sources, the refusals - is dgmr_advect's;
 * x_step_stride = 0 with field_group = 1 gives dgmr_advect's bits.
 *
 * dgmr_advect_series_perturbed (a new symbol, same ABI version): dgmr_advect_series with a velocity error per plane and lead time, along and across the
 * local motion (STEPS' perturbed motion vectors; stochastic.py).  direction[n / field_group][gy][gx][2] = (uy, ux): a second fp32
 * lattice of the field's geometry (Gy, Gx, origin, spacing) and plane mapping, direction_plane_stride elements per plane (0: one for
 * all planes), which the CALLER has normalised (advection.unit_directions: v / |v|, (0, 0) at calm nodes) - the kernel divides by
 * nothing and takes no root.  amplitude[n][t - 1][2] = (a_par, a_perp) in pixels per step, contiguous, N T pairs.  At q = p - D_(t-1)(p),
 * with u(q) the bilinear interpolation of the direction lattice through the field's node indices and weights:
 *   vy' = fma(a_par, uy, fma(a_perp, -ux, vy)),  vx' = fma(a_par, ux, fma(a_perp, uy, vx))      (the perpendicular of u is (-ux, uy))
 *   D_t(p) = D_(t-1)(p) + v'(q);  out[n][t - 1][p] = s_t(p - D_t(p)).
 * a = 0 gives dgmr_advect_series' bits for finite directions.  Against exact arithmetic the result is within
 *   c' T max(H, W) 2^-24 A + 4 * 2^-24 max|x|,  c' = 50:  per step and axis the 10 operations of dgmr_advect, 2 x 6 for the
 * interpolations of the two direction components an axis of v' takes and 2 for its fmas, + 1 for the sample position, on two axes
 * (advect.hip lists them) - for a TOTAL velocity v' that changes by less than 1 / (4 T) pixels per pixel and displacements that stay
 * below max(H, W).  Layouts, store widths and refusals are dgmr_advect_series'; in addition direction and amplitude must not be null
 * and direction_plane_stride has field_plane_stride's range.  Argument errors return < 0 and set dgmr_last_error() before anything
 * is enqueued.  Runs on `stream`, does not synchronise.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_spectral_ar(const float* z0, int64_t z0_plane_stride, const float* white, int64_t white_member_stride, int64_t white_step_stride,
                     const float* rho, int P, int M, int T, int H, int W, int L, float* out, int64_t out_member_stride,
                     int64_t out_step_stride, void* stream);
int dgmr_advect_series(const float* x, int64_t x_plane_stride, int64_t x_step_stride, const float* field, int64_t field_plane_stride,
                       int field_group, int64_t N, int H, int W, int Gy, int Gx, float origin, float spacing, int T, float* out,
                       int64_t out_plane_stride, int64_t out_step_stride, void* stream);
int dgmr_advect_series_perturbed(const float* x, int64_t x_plane_stride, int64_t x_step_stride, const float* field,
                                 int64_t field_plane_stride, const float* direction, int64_t direction_plane_stride, const float* amplitude,
                                 int field_group, int64_t N, int H, int W, int Gy, int Gx, float origin, float spacing, int T, float* out,
                                 int64_t out_plane_stride, int64_t out_step_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lag spectra: the radially binned cross-spectrum of two planes over the windows and bins dgmr_spectral_ar evolves (stochastic.py:
 * lag_spectra, estimate_rho; csrc/spectrum.hip).  New symbol, same ABI version.
 * a, b: N fp32 planes [H][W] each, plane n at a + n a_plane_stride and b + n b_plane_stride (elements, >= H * W), any finite real
 * values (no missing-value rule, as for z0 of dgmr_spectral_ar).  L one of 32, 64, 128; H and W multiples of L.  The windows are the
 * four classes of dgmr_spectral_ar, origins (i L + cy L / 2, j L + cx L / 2), i < H / L - cy, j < W / L - cx, numbered per plane class
 * by class in the order (0,0), (0,1), (1,0), (1,1) and row-major inside a class; Wn = the sum over the classes of
 * (H / L - cy) (W / L - cx).  With A = fft2(a patch), B = fft2(b patch), unnormalised, over ALL L^2 modes of radial bin r:
 *   sums[n][window][q][r]  double  q = 0: sum |A|^2;  q = 1: sum |B|^2;  q = 2: sum Re(A conj B);   [N][Wn][3][L]
 * r is dgmr_spectral_ar's bin (r (r - 1) < kx^2 + ky^2 <= r (r + 1) over the signed frequencies in [-L/2, L/2); r < L): unlike
 * dgmr_radial_psd the corner modes with r >= L / 2 and the Nyquist row and column are kept.  Bins that hold no mode (all above
 * round(L / sqrt 2)) are written as 0.  fp32 radix-2 transforms on the half spectrum with the Nyquist column carried (the forward
 * transform of dgmr_spectral_ar); a mode with 0 < kx < L / 2 counts twice, one with kx = 0 or kx = L / 2 once.  The three terms of a
 * mode are formed in fp32 by one expression shape, fma(re, re', im im'), by one copy of the transform code, so b == a gives three
 * bit-equal rows and b == -a gives q = 2 equal to -(q = 0); they are added in float64 in a fixed order (ascending kx and |ky|, +ky
 * before -ky, four column partials per bin in index order).  One workgroup per (plane, window), one launch, no workspace, no
 * floating-point atomics: two calls give the same bits and the result for plane n does not depend on N.  16-byte loads when both
 * pointers and both strides allow them, 4-byte loads otherwise: no alignment demands on a and b (sums: 8 bytes).  Argument errors
 * (null pointers, L outside the set, H or W not a multiple of L, N < 1, a plane stride below H * W) return < 0 and set
 * dgmr_last_error() before anything is enqueued.  Runs on `stream`, does not synchronise.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_lag_spectra(const float* a, int64_t a_plane_stride, const float* b, int64_t b_plane_stride, int64_t N, int H, int W, int L,
                     double* sums, void* stream);

/* ------------------------------------------------------------------------------------------------
 * dgmr_spectral_ar2: dgmr_spectral_ar with a second lag (stochastic.py: spectral_ar2, ar2_coefficients, estimate_ar2;
 * csrc/spectral_ar.hip).  New symbol, same ABI version.
 * z0, white, out, P, M, T, H, W, L, the windows, their classes, the radial bin r(k), the blend and the four launches are
 * dgmr_spectral_ar's.  zm1: the frame before z0 in z0's coordinates, P fp32 planes [H][W], zm1_plane_stride apart.  coef: per plane
 * three rows of L fp32 values (phi1[r], phi2[r], g[r]), plane p at coef + p coef_plane_stride; coef_plane_stride = 0 is one set for
 * all planes, otherwise it is at least 3 L.  Per window and member, with X_0 = fft2(z0 patch), X_-1 = fft2(zm1 patch),
 * A = |X_0| / L and Wh_t = fft2(white patch of lead t):
 *   X_t(k) = (phi1[r(k)] X_(t-1)(k) + phi2[r(k)] X_(t-2)(k)) + g[r(k)] A(k) Wh_t(k),   x_t = real(ifft2(X_t)),   t = 1 ... T.
 * The coefficients are used as passed, never recomputed: per component X_t = fma(phi1, X_(t-1), fma(phi2, X_(t-2), amp v)) with
 * amp = g[r] (|X_0| (1 / L)), so coef = (rho, 0, fp32(sqrt(1 - rho^2))) is dgmr_spectral_ar's recursion term for term.  Both spectra
 * of a thread's elements stay in registers through the T steps; phi1 and phi2 are read from LDS tables by the element's radial bin,
 * kept as packed bytes; zm1 is transformed once, before the loop, in the one LDS buffer.  No atomics, no workspace, two calls give
 * the same bits.  16-byte accesses when pointers and strides allow them (z0, zm1 and white together, out on its own).  Argument
 * errors (null pointers, L outside the set, H or W not a multiple of L, T outside 1 ... 64, P or M below 1, a negative stride, a
 * white or out stride below H * W, a coef stride between 1 and 3 L - 1) return < 0 and set dgmr_last_error() before anything is
 * enqueued.  Runs on `stream`, does not synchronise.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_spectral_ar2(const float* z0, int64_t z0_plane_stride, const float* zm1, int64_t zm1_plane_stride, const float* white,
                      int64_t white_member_stride, int64_t white_step_stride, const float* coef, int64_t coef_plane_stride, int P, int M,
                      int T, int H, int W, int L, float* out, int64_t out_member_stride, int64_t out_step_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Probability matching for the stochastic ensemble (stochastic.py: probability_match; csrc/probmatch.hip).  New symbols, same ABI
 * version.
 * z: the dB fields of dgmr_spectral_ar with its plane addressing - plane n = p M + m of lead time t at z + n member_stride +
 * (t - 1) step_stride, H W contiguous fp32 values; out likewise with its two strides.  target_sorted: per case p the N = H W values of
 * the frame to match, sorted ascending, at target_sorted + p target_stride.  mask: null, or uint8 planes at mask + p mask_plane_stride
 * + (t - 1) mask_step_stride (0: one plane for all lead times); nonzero = rain is allowed here.  4096 bins of 1 / scale dB from lo;
 * scale must be a power of two.  Per plane, every fp32 operation rounded once and none contracted:
 *   u = (z - lo) * scale;  !(u >= 0) (below the range, NaN): b = 0, f = 0;  u >= 4096: b = 4095, f = 0;  else b = floor(u), f = u - b;
 *   a masked-out element: b = 0, f = 0;
 *   h[b] = the number of the plane's N elements in bin b;  c[b] = sum of h[b'] over b' < b;
 *   r = c[b] + min(int(f * float(h[b])), h[b] - 1);  out = target_sorted[r], and 0.0 for a masked-out element.
 * r lies in [c[b], c[b] + h[b] - 1], inside [0, N): the map is monotone in z, every output is a value of the target, and a rank is off
 * from the exact one by less than its bin's occupancy.  All counts are integers (an LDS histogram per workgroup, its nonzero bins added
 * with integer atomics onto the workspace, which the call clears first), so the result is the reference's bit for bit and two calls
 * give the same bits.  A bin whose span of ranks reads one and the same target value - most of a radar frame is exact zeros - takes
 * that value without reading the target per element (not where the case's target holds a -0.0 or a NaN, whose bits equal values do
 * not fix).  out may be z itself (each element is read and written by the same lane); any other overlap is undefined.
 * workspace: dgmr_probability_match_workspace(P, M, T) bytes - two rows of 4096 int32 per plane and a flag per case, 32768 P M T +
 * 4 P rounded up to 16 -, 16-byte aligned (< 0 for P, M < 1, T outside 1 ... 64 or more than 2^20 planes).  16-byte accesses when z, out, the mask and all their strides allow them, 4-byte ones otherwise: no
 * alignment demands.  Argument errors (null z, target_sorted, workspace or out, scale no power of two, lo not finite, H W > 2^24, a
 * stride below H W - mask_step_stride may be 0 -, T outside 1 ... 64, a workspace that is too small) return < 0 and set
 * dgmr_last_error() before anything is enqueued.  Runs on `stream`, does not synchronise.
 * ---------------------------------------------------------------------------------------------- */
int64_t dgmr_probability_match_workspace(int P, int M, int T);
int dgmr_probability_match(const float* z, int64_t member_stride, int64_t step_stride, const float* target_sorted, int64_t target_stride,
                           const uint8_t* mask, int64_t mask_plane_stride, int64_t mask_step_stride, int P, int M, int T, int H, int W,
                           float lo, float scale, void* workspace, int64_t workspace_bytes, float* out, int64_t out_member_stride,
                           int64_t out_step_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py's roofline leg; not part of the reference's surface).  When enabled, every conv /
 * wgrad launch is bracketed by HIP events on its launch stream; collect() returns, per tile variant, the summed
 * kernel time, the summed algorithmic FLOPs (2*M*K*Cout) and the launch count, then clears the records.
 * ---------------------------------------------------------------------------------------------- */
int dgmr_profile_enable(int on);
int dgmr_profile_variants(void);
const char* dgmr_profile_variant_name(int variant);
int dgmr_profile_collect(double* total_ms, double* total_flops, int64_t* launches, int n);
/* The same plus executed_flops[v]: the flops the matrix pipe really issued - 16/36 of the algorithmic figure for upsampling convs run
 * as phase convs / pooled data gradients (w_phase), times the MFMAs per product of the mode the launch was issued in (3 in
 * DGMR_PREC_BF16X3, 6 in DGMR_PREC_BF16X6; ABI 8: this factor used to be the caller's to apply). */
int dgmr_profile_collect2(double* total_ms, double* total_flops, double* executed_flops, int64_t* launches, int n);
/* (ABI 9) The same records grouped by INSTANTIATED kernel instead of by class: tile (output-channel block, 128- / 256-pixel), mode
 * (plain / phase / pooled 3x3, 3-D, ConvGRU epilogue, split-K, 1x1), launch size (fewer than 1024 workgroups = "small": such a launch
 * cannot fill 256 CUs four times over) and arithmetic.  Writes "name\tlaunches\ttotal_ms\talgorithmic_flops\texecuted_flops\n" lines
 * (NUL-terminated, truncated to cap) and returns the bytes needed.  Does not clear the records: call it BEFORE dgmr_profile_collect*. */
int dgmr_profile_collect_detail(char* buf, int cap);
/* Dispatch override for tools/conv_bench.py's tile / split-K sweeps (process-wide; -1 = the library's own choice, which is
 * also the state at load): variant = index of a conv_fwd_dgrad<..> tile as listed by dgmr_profile_variant_name, ksplit = number
 * of K slabs (needs a workspace in the args), window = 0 never / 1 the register-staged LDS-window 3x3 kernel whenever the geometry allows / 2 likewise, with the experimental
 * 256-pixel tiles / 3 the LDS-DMA window kernel where eligible (what -1 picks, but also below the automatic size threshold) /
 * 4 its private-weight-slice variant / 5 its 16-column-block variant for <= 48 output channels / 6 (ABI 9) the LDS-DMA kernel with
 * the block shapes of the wave-specialised kernel (the bit-for-bit reference of 7) / 7 (ABI 9) the wave-specialised persistent
 * kernel (conv_win_ws.h: matrix waves + loader / epilogue waves in one workgroup per CU) wherever it applies, at any size;
 * wgrad_window = 0 never an LDS-window weight-gradient kernel / 1 the one-role kernel of round 2 (wgrad_win.h) wherever the geometry
 * allows / 2 the wave-specialised one (wgrad_ws.h: loader waves + matrix waves, ds_read_b64_tr_b16 fragments) with three matrix
 * waves (32x32x16 MFMAs, one filter row each) / 3 (= automatic) with four (16x16x32 MFMAs, one per SIMD; bf16x6: three) / 4 like 3,
 * and upsampling convs by output-pixel parity on the low-resolution map (wgrad_ws.h PHASE) even under DGMR_WGRAD_PHASES=0 (by default
 * that is the library's own choice where the four-wave kernel applies) / 5 (round 6) like 3, but layers with <= 48 output channels on
 * the 64-column tile of rounds 3 - 5 instead of the pixel-split 48-column one (wgrad_ws.h PSPLIT; the A/B reference) and no phase launches. */
int dgmr_conv_tune(int variant, int ksplit, int window, int wgrad_window);
/* Kernel-phase timing switches for tools/conv_bench.py (process-wide, 0 at load and in every product launch): bit 0 = the LDS-window
 * conv kernels return before their epilogue, bit 1 = they stage only their first input halo.  Outputs are then garbage by design;
 * only the launch duration is meaningful (how much of a launch is operand staging / matrix work / epilogue).  Bit 3 (8) = the
 * window kernels use their lane-per-channel epilogue instead of the 16-byte one (A/B: results are bit-identical); 64 / 128 = every
 * wave sleeps ~3.4 / ~6.8 us after issuing its last store (how long does a finished wave wait for its stores anyway?); 16 = the
 * wave-specialised weight-gradient kernel without its matrix work (the loaders' time alone); 256 (round 5) = phase launches of the
 * upsampling convs with one workgroup per ROW parity that computes both column parities from one staged halo, instead of one
 * workgroup per output-pixel parity (conv_win_glds.h PAIR; same results bit for bit - tests/test_gpu_kernels.py; measured no faster,
 * so it is not the default: DGMR_PHASE_PAIR=1 switches it on for a whole process).  512 = the streaming 1x1 kernel writes BatchNorm
 * partial sums from its epilogue (stats_out) and dgmr_conv_stats_rows answers for it (DGMR_CONV1X1_STATS=1 for a whole process; off by
 * default); 1024 = dgmr_wgrad_reduce[_slice] never take their two-stage path (DGMR_WGRAD_NARROW=0; same bits either way); 2048 =
 * dgmr_sn_wgrad_finalize uses its one-thread-per-element kernel (DGMR_SN_FINALIZE_TILED=0; same bits either way); 4096 = dispatch probe:
 * the LDS-tiled finalize kernel, where dgmr_sn_wgrad_finalize launches it, returns at once and gw keeps its values (garbage by design).
 * 8192 = BatchNorm's stream passes (dgmr_bn_stats / _bwd_reduce / _bwd_apply, dgmr_colsum and the two serial walks behind them) keep
 * one row in flight per lane on their former grids instead of several (same bits either way; the tests' reference and the A/B). */
int dgmr_debug_flags(int flags);

#ifdef __cplusplus
}
#endif
#endif /* DGMR_HIP_H */
