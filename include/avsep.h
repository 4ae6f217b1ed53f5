/*
 * avsep.h — C ABI of libavsep_gfx950.so: the MI355X (gfx950) kernels behind the
 * mix-and-separate train step of abcqmars/audio-visual-sepatation-in-visual-agnostic-situtation.
 *
 * The reference has no native layer: every entry point below
 * replaces a group of stock PyTorch operators at the cited reference call site,
 * and is what a binding for the reference's Python would load with ctypes
 * (INTEGRATION.md shows the stub).  Conventions:
 *   - extern "C", plain pointers and sizes; no C++/torch types cross the boundary;
 *   - every pointer is a DEVICE pointer unless the name says host; tensors are
 *     dense fp32 NCHW unless stated; the caller owns all buffers incl. workspaces;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous;
 *   - return value: 0 = ok, negative = error (avsep_strerror()).
 *   - the library keeps no mutable global state, reads no environment variable and is re-entrant per stream; what steers
 *     the dispatch of a convolution call (A/B and tuning overrides) travels in its descriptor (avsep_conv_desc.algo / .tune).
 */
#ifndef AVSEP_H
#define AVSEP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVSEP_OK 0
#define AVSEP_ERR_ARG (-1)     /* bad shape / null pointer / unsupported geometry */
#define AVSEP_ERR_LAUNCH (-2)  /* hipGetLastError() after a launch */
#define AVSEP_ERR_WORKSPACE (-3)

#define AVSEP_ACT_NONE 0
#define AVSEP_ACT_RELU 1
#define AVSEP_ACT_LRELU02 2    /* LeakyReLU(0.2): models/audio_net.py:64 */
#define AVSEP_ACT_SIGMOID 3
#define AVSEP_ACT_TANH 4
#define AVSEP_ACT_SOFTMAX2 5   /* softmax over a 2-channel dim (models/__init__.py:19-20) */

#define AVSEP_PREC_F32 0
#define AVSEP_PREC_BF16 1

/* Storage format of an activation / gradient tensor [N,C,H,W]:
 *   AVSEP_FMT_F32: dense fp32 NCHW (the reference's tensors);
 *   AVSEP_FMT_B16: bf16, channel-blocked  [N][C/16][H][W][16]  (C % 16 == 0): the 16 channels of a block at one position
 *                  are 32 contiguous bytes — exactly one position of the bf16 kernels' LDS patch, so an operand is staged
 *                  with one 16-byte load per (position, 8-channel half) and no conversion.  Used between the bf16 kernels
 *                  (BASELINE.json configs[2]: half the HBM bytes of fp32 activations). */
#define AVSEP_FMT_F32 0
#define AVSEP_FMT_B16 1

typedef void* avsep_stream_t;

int avsep_version(void);
const char* avsep_arch(void);          /* "gfx950" */
const char* avsep_strerror(int code);
/* The launch plan of a glue kernel (csrc/ops.hip, csrc/b16.hip): the kernel form and the grid (256-thread workgroups) its
 * launcher chooses for a shape, from the very function the launcher calls.  Host only: no device is touched, no pointer
 * but `op`, `form` and `grid` is read.  `op` and the meaning of (N, C, H, W, aux), HW = H * W wherever the entry point takes HW:
 *   channel_stats, bn_bwd_apply, affine_act, affine_act_bwd, maxpool_bn_relu_bwd_stats, maxpool_bn_relu_bwd_apply,
 *   f32_to_b16, b16_to_f32, bn_bwd_apply_to_b16, b16_affine_act, b16_affine_act_bwd, b16_bn_bwd_apply, b16_channel_sum,
 *   b16_maxpool_fwd, b16_maxpool_bwd_stats, b16_maxpool_bwd_apply, b16_space_to_depth2      [N, C, H, W] as the entry point's
 *   maxpool_fwd, maxpool_bwd        NC = N * C planes of H x W
 *   space_to_depth2                 aux = Cp
 *   temporal_mean_fwd, temporal_mean_bwd    B = N, T = aux, CHW = C * H * W
 *   sgd                             n = N * C * H * W
 *   relu_up2x_fwd, relu_up2x_bwd    the descriptor's low-resolution [N, C0 + C1, H, W]; aux = 1 when a source is a broadcast
 *                                   vector (bcast0 or bcast1), else 0
 *   b16_relu_up2x_fwd, b16_relu_up2x_bwd    low-resolution [N, C0 + C1, H, W] with C0 = aux
 * `form` (cap >= 32 bytes) receives the form's name, grid[3] the grid.  AVSEP_ERR_ARG for an unknown op or a shape the
 * launcher refuses: a launcher accepts or refuses a shape, and picks form and grid, in that one function and nowhere else.
 * (avsep_b16_grid_pack and avsep_grid_unpack plan the same way but are no op here: their geometry is nine integers.) */
int avsep_glue_plan(const char* op, int32_t N, int32_t C, int32_t H, int32_t W, int32_t aux, char* form, size_t cap,
                    int32_t grid[3]);

/* ---------------------------------------------------------------------------
 * Convolution as implicit GEMM on the f32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces nn.Conv2d forward/backward at models/audio_net.py:72-98,177-182 and the
 * torchvision ResNet-18 convs wrapped by models/vision_net.py:84-92.
 *
 * The conv input is a virtual tensor: channel-concat of up to two sources (the U-Net
 * skip concat, audio_net.py:122,203), each passed through an optional per-channel
 * affine (a folded BatchNorm, audio_net.py:65-67) and activation (LeakyReLU / ReLU,
 * audio_net.py:64,66) while it is gathered — none of those is materialised.
 * With up2x != 0 the virtual input is additionally the bilinear x2 upsample
 * (align_corners=True, audio_net.py:68-69) of that tensor; H,W are then the
 * UPSAMPLED sizes and the sources are [N,C,H/2,W/2].
 * ------------------------------------------------------------------------- */
/* avsep_conv_desc.algo */
#define AVSEP_ALGO_NO_WINOGRAD        1   /* 3x3/s1 forward + data gradient: direct form instead of Winograd F(2x2,3x3) / F(4x4,3x3) */
#define AVSEP_ALGO_NO_WINOGRAD_WGRAD  2   /* weight gradients: direct form instead of the Winograd-domain kernels */
#define AVSEP_ALGO_NO_FLAT            4   /* no flat-pixel tiles on the 14x14 / 7x7 maps */
#define AVSEP_ALGO_NO_MISC_PATCH      8   /* 3x3/s2, 1x1, stem: im2col kernel instead of the halo-patch kernel */
#define AVSEP_ALGO_NO_BF16_KERNELS   16   /* prec = bf16 ignored: every call runs its exact f32 kernel */
#define AVSEP_ALGO_NO_SMALLCI_WGRAD  32   /* stem / first U-Net conv weight gradient on the im2col kernel */
#define AVSEP_ALGO_NO_WINOGRAD4      64   /* Winograd layers stay on F(2x2,3x3): no F(4x4,3x3) kernel */

typedef struct avsep_conv_desc {
  int32_t N, Cin, H, W;        /* virtual input  [N,Cin,H,W]   */
  int32_t Cout, Ho, Wo;        /* output         [N,Cout,Ho,Wo] */
  int32_t KH, KW, stride, pad, dil;
  int32_t C0;                  /* channels from x0; Cin-C0 from x1 (0 => x1 unused) */
  int32_t act0, act1;          /* AVSEP_ACT_NONE/RELU/LRELU02, applied after the affine */
  int32_t up2x;
  int32_t prec;                /* AVSEP_PREC_F32 (0): exact f32 MFMA; AVSEP_PREC_BF16 (1): operands rounded to bf16 while they are
                                  staged, fp32 accumulation / statistics / outputs (BASELINE.json configs[2]); geometries without a
                                  bf16 kernel run in f32 */
  int32_t plan_n;              /* batch the launch heuristics are PLANNED for (0 = N).  Tile sizes, split-K and the kernel family
                                  of a call depend on how many workgroups its grid has, i.e. on N; with plan_n = 64 a batch-8
                                  call takes the decisions of the batch-64 call (grids and workspaces stay those of N).  The
                                  parity tests use it to run the benched dispatch at an oracle-sized batch; results never
                                  depend on it beyond the summation order of the chosen kernel. */
  int32_t xfmt, yfmt;          /* AVSEP_FMT_* of x0 (forward / weight gradient) and of y as avsep_conv2d_fwd writes it */
  int32_t dyfmt, dxfmt;        /* AVSEP_FMT_* of dy (data / weight gradient) and of dx as avsep_conv2d_dgrad writes it.
                                  avsep_conv_io_formats tells which formats a call takes; B16 pointers are passed as float* */
  int32_t algo;                /* bit set of AVSEP_ALGO_NO_*: kernel families this call must NOT use (0 = the library's choice).
                                  This is the ONLY way to steer the dispatch: the library reads no environment variable and keeps
                                  no process-wide switch, so pack / workspace / launch calls of one descriptor cannot disagree. */
  int32_t tune;                /* measurement tools only (tools/conv_bench.py), 0 = the library's heuristics: bits 0-3 group shape
                                  of the Winograd forward / data gradient + 1, bits 4-7 of the Winograd weight gradient + 1,
                                  bits 8-23 target workgroup count of its K-split */
  const float* x0;
  const float* x1;
  const float* scale0;         /* [C0] or NULL */
  const float* shift0;
  const float* scale1;         /* [Cin-C0] or NULL */
  const float* shift1;
} avsep_conv_desc;

/* Weight repack, once per optimizer step.  w: OIHW [Cout,Cin,KH,KW].
 * mode 0 -> forward operand  [Kpad][Mpad], k=(ci,kh,kw), Mpad=roundup(Cout,128), Kpad=roundup(K,32)
 * mode 1 -> dgrad operand    [KH*KW*Cout (padded to 32)][roundup(Cin,128)]            */
size_t avsep_conv_packed_floats(const avsep_conv_desc* d, int mode);
int avsep_conv_pack_weights(const avsep_conv_desc* d, const float* w, float* packed, int mode,
                            avsep_stream_t stream);

/* y = conv(virtual input) (+bias).  stats (optional, double[2*Cout], pre-zeroed):
 * per-channel sum and sum of squares of y, for the following BatchNorm.
 * workspace (avsep_conv2d_fwd_workspace_bytes; may be 0/NULL): split-K partial slabs for layers whose
 * output grid cannot fill the chip; without it the call falls back to an unsplit launch.        */
/* Formats of a call (mode 0 forward, 1 data gradient, 2 weight gradient) under d->prec and the geometry:
 * *in_fmt = the AVSEP_FMT_* its input tensors MUST have (x0 for mode 0; dy for mode 1; x0 and dy for mode 2),
 * *out_b16 = 1 when the output (y / dx) may be requested as AVSEP_FMT_B16 through d->yfmt / d->dxfmt (fp32 always may).
 * A call whose descriptor disagrees returns AVSEP_ERR_ARG. */
int avsep_conv_io_formats(const avsep_conv_desc* d, int32_t mode, int32_t* in_fmt, int32_t* out_b16);
size_t avsep_conv2d_fwd_workspace_bytes(const avsep_conv_desc* d);
int avsep_conv2d_fwd(const avsep_conv_desc* d, const float* w_packed, const float* bias, float* y,
                     double* stats, void* workspace, size_t workspace_bytes, avsep_stream_t stream);
/* dx = gradient w.r.t. the VIRTUAL input [N,Cin,H,W] (after affine/activation/upsample). */
size_t avsep_conv2d_dgrad_workspace_bytes(const avsep_conv_desc* d);
int avsep_conv2d_dgrad(const avsep_conv_desc* d, const float* w_packed_dgrad, const float* dy,
                       float* dx, void* workspace, size_t workspace_bytes, avsep_stream_t stream);
/* The data gradient taken THROUGH the activation (and BatchNorm / residual add) in front of the convolution's input, in the
 * producing kernel's epilogue: the backward of `relu(bn1(y1))` between the two convs of a ResNet BasicBlock and of the block
 * tail `relu(bn2(y2) + residual)` (vision_net.py:84-109 through torchvision's BasicBlock; main.py:557-569 runs it as
 * autograd's ReluBackward + NativeBatchNormBackward between the two ConvolutionBackward nodes).  The operands are those of
 * avsep_affine_act_bwd below with dz = the data gradient:
 *     dx = act'(scale*y + shift [+ res_scale*residual + res_shift]) * (dgrad(dy) [+ dz2]) [+ add]
 *     bstats += (sum dx, sum dx * (y - mean) * invstd)                                  per channel of dx, fp64
 * y, residual, dz2, add: [N,Cin,H,W] fp32 like dx; the per-channel rows [Cin].  Exactly avsep_conv2d_dgrad followed by
 * avsep_affine_act_bwd in place on dx — which is what the call runs for the kernel families without the epilogue
 * (avsep_conv2d_dgrad_act_fused(d) == 0); with it the gradient is never written unmasked and never re-read.
 * fp32 dx only (d->dxfmt == AVSEP_FMT_F32).  workspace as avsep_conv2d_dgrad.
 * Measured (MI355X, tools/conv_bench.py dgrad --act-epilogue): with y alone (the bn1 form) the call costs what the data
 * gradient alone did on the 14x14 ... 56x56 trunk maps and saves the pass (the host layer uses it there); every further
 * operand (residual, dz2, add) is a read the epilogue cannot hide: slower than the two launches below 32x32 maps,
 * 5-15 % faster on 64x64 and 128x128 ones. */
typedef struct avsep_act_bwd {
  const float* y;              /* the BatchNorm input whose activation the gradient passes            (required) */
  const float* scale;          /* folded BatchNorm rows of y (NULL: identity)                                     */
  const float* shift;
  const float* residual;       /* added to scale*y + shift before the activation (NULL: none)                     */
  const float* res_scale;      /* folded BatchNorm rows of the residual (NULL: plain add)                         */
  const float* res_shift;
  const float* dz2;            /* a second gradient branch reaching the same activation output (NULL: none)       */
  const float* add;            /* added after the activation gradient (NULL: none)                                */
  const float* mean;           /* batch statistics of y: required with bstats                                     */
  const float* invstd;
  double* bstats;              /* [2*Cin], accumulated (NULL: no sums)                                            */
  int32_t act;                 /* AVSEP_ACT_*                                                                     */
} avsep_act_bwd;
int32_t avsep_conv2d_dgrad_act_fused(const avsep_conv_desc* d);   /* 1: one kernel; 0: the two launches */
int avsep_conv2d_dgrad_act(const avsep_conv_desc* d, const float* w_packed_dgrad, const float* dy,
                           const avsep_act_bwd* e, float* dx, void* workspace, size_t workspace_bytes,
                           avsep_stream_t stream);
/* dw OIHW; dbias optional ([Cout]).  workspace from avsep_conv2d_wgrad_workspace_bytes(). */
size_t avsep_conv2d_wgrad_workspace_bytes(const avsep_conv_desc* d);
int avsep_conv2d_wgrad(const avsep_conv_desc* d, const float* dy, float* dw, float* dbias,
                       void* workspace, size_t workspace_bytes, avsep_stream_t stream);

/* Fused decoder head (audio_net.py:72-76, the outermost up path: ReLU -> Upsample x2 -> Conv3x3 -> num_mix logits).
 * When avsep_conv2d_head_applicable(d) is 1 (up2x=1, 3x3/s1/p1, Cout <= 4, ReLU on both sources, both channel counts
 * multiples of 8, Cin <= 256), avsep_conv2d_fwd / _wgrad contract the channels at LOW resolution (interpolation and
 * channel mix commute) instead of reading a materialised hi-res copy, and avsep_conv2d_dgrad_up2x takes the gradient
 * straight to the two low-res sources: the same results as avsep_conv2d_dgrad followed by avsep_relu_up2x_bwd
 * (g0 [N,C0,H/2,W/2] accumulated in place when acc0, g1 [N,C1,H/2,W/2], bstats1[2*C1] += BatchNorm-backward sums of
 * source 1).  w is OIHW.  All three need their workspace (9*Cout low-res planes per image). */
size_t avsep_conv2d_dgrad_up2x_workspace_bytes(const avsep_conv_desc* d);
int32_t avsep_conv2d_head_applicable(const avsep_conv_desc* d);
/* Name of the kernel family avsep_conv2d_fwd (mode 0, `with_stats` as it will be called), _dgrad (mode 1) or _wgrad
 * (mode 2) dispatches this descriptor to ("convbf_kernel", "wgradbf_kernel", "conv3x3_kernel", "wgrad3x3_kernel",
 * "igemm_kernel<fwd|dgrad|wgrad>", "head_*_kernel", "smallco_*", "smallci_dgrad"): measurement bookkeeping
 * (bench.py groups its HIP-event timings by it), static strings, never freed. */
const char* avsep_conv_kernel_name(const avsep_conv_desc* d, int32_t mode, int32_t with_stats);
/* The same plus every launch decision that depends on the size of the grid (tile shape, 64- / 128-row tiles, 256- / 512-
 * thread workgroups, split-K), e.g. "convbf_kernel:8x32,128x256", "conv3x3_kernel:4x32,BM64", "igemm_kernel<fwd>:BM64,split6":
 * two descriptors with equal variants run the same kernel instantiation.  An "igemm_kernel<...>" variant ends in "ld64"
 * ("...,ld64"; the weight gradient's is "igemm_kernel<wgrad>:ld64") when a tensor the call gathers (a source of x; dY) has
 * 4 * elements + 16 >= 0xfffffff0 bytes, which keeps it on the 64-bit loader.  The parity tests assert that a batch-8 step
 * planned for the bench batch (desc.plan_n) has, layer by layer, the variants of the batch-64 step bench.py times. */
int avsep_conv_kernel_variant(const avsep_conv_desc* d, int32_t mode, int32_t with_stats, char* buf, size_t cap);
int avsep_conv2d_dgrad_up2x(const avsep_conv_desc* d, const float* w, const float* dy, float* g0,
                            float* g1, const float* mean1, const float* invstd1, double* bstats1,
                            int32_t acc0, void* workspace, size_t workspace_bytes, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * SoP++ attention module core (SoP++/attention_net.py:24-58: `att` + `av_infer_forward`, shared by AttModel / MatchAtt):
 * a [B,S,K] pooled audio queries (S <= 4, K <= 128), mix [B,K,HW] mixed visual map (HW <= 4096), att 0 = cos, 1 = sig.
 *   maps_raw [B,S,HW] similarity maps BEFORE the clamp; ctx [B,S,K] = mean_hw(mix * clamp(maps,0,1));
 *   match [B] = -sum_s mean_hw maps_raw (the module's match term is its batch mean).
 * Backward: dctx [B,S,K], dmaps [B,S,HW] (wrt the clamped maps; may be NULL), dmatch [B] (may be NULL) -> da, dmix.
 * ------------------------------------------------------------------------- */
int avsep_attmodel_infer_fwd(const float* a, const float* mix, int32_t B, int32_t S, int32_t K, int32_t HW, int32_t att,
                             float* maps_raw, float* ctx, float* match, avsep_stream_t stream);
int avsep_attmodel_infer_bwd(const float* a, const float* mix, const float* maps_raw, const float* dctx,
                             const float* dmaps, const float* dmatch, int32_t B, int32_t S, int32_t K, int32_t HW,
                             int32_t att, float* da, float* dmix, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * BatchNorm2d pieces (train-mode batch statistics; nn.BatchNorm2d at audio_net.py:37,65,67).
 * ------------------------------------------------------------------------- */
/* stats[2*C] += per-channel (sum, sumsq) of x [N,C,HW]. */
int avsep_channel_stats(const float* x, int32_t N, int32_t C, int32_t HW, double* stats,
                        avsep_stream_t stream);
/* From (sum,sumsq) -> scale=gamma*invstd, shift=beta-mean*scale, mean, invstd; updates the
 * running buffers (momentum, unbiased var) when training!=0; with training==0 uses them.
 * `updates` >= 1: the running buffers receive that many momentum updates and num_batches_tracked
 * (nn.BatchNorm2d's int64 counter, may be NULL) is incremented by it — a shared encoder stands for
 * several identical forward passes of the reference (main.py:128-141). */
int avsep_bn_finalize(const double* stats, double count, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps,
                      int32_t C, int32_t training, float* scale, float* shift, float* mean,
                      float* invstd, int64_t* num_batches_tracked, int32_t updates, avsep_stream_t stream);
/* Backward of train-mode BN given dz (grad wrt BN output) sums: bstats[2*C] = (sum dz, sum dz*xhat).
 * Writes dgamma,dbeta and the coefficients of dy = p*dz + q*y + r (p,q,r: [C] each).     */
int avsep_bn_bwd_coeffs(const double* bstats, double count, const float* gamma, const float* mean,
                        const float* invstd, int32_t C, float* dgamma, float* dbeta, float* pqr,
                        avsep_stream_t stream);
/* dy = p[c]*dz + q[c]*y + r[c]  (in place on dz allowed). */
int avsep_bn_bwd_apply(const float* dz, const float* y, const float* pqr, int32_t N, int32_t C,
                       int32_t HW, float* dy, avsep_stream_t stream);
/* z = act(scale[c]*y + shift[c] [+ res_scale[c]*residual + res_shift[c]]): BatchNorm + residual + ReLU of a
 * ResNet BasicBlock in one pass (the residual carries its own folded BN when it comes from a downsample conv;
 * res_scale/res_shift NULL -> plain residual add). */
int avsep_affine_act(const float* y, const float* scale, const float* shift, const float* residual,
                     const float* res_scale, const float* res_shift, int32_t act, int32_t N, int32_t C,
                     int32_t HW, float* z, avsep_stream_t stream);
/* Gradient through that z:  dz_pre = act'(pre)*(dz [+ dz2]) (+ add);  also accumulates
 * bstats (sum dz_pre, sum dz_pre*xhat(y)) when bstats != NULL.  dz2 (may be NULL): a second gradient
 * branch reaching z (a BasicBlock output feeds the next block's conv1 AND its residual add), summed on the fly. */
int avsep_affine_act_bwd(const float* dz, const float* dz2, const float* y, const float* scale, const float* shift,
                         const float* residual, const float* res_scale, const float* res_shift,
                         const float* add, const float* mean, const float* invstd, int32_t act,
                         int32_t N, int32_t C, int32_t HW, float* dz_pre, double* bstats,
                         avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * U-Net decoder glue: ReLU + bilinear x2 (align_corners=True) of the concat
 * (audio_net.py:66-69,122,203) and its transpose.
 * Sources as in avsep_conv_desc; a source with bcast!=0 is a [N,C] vector tiled over HxW
 * (the fusion output, fusion_net.py:70-72).
 * ------------------------------------------------------------------------- */
typedef struct avsep_cat_desc {
  int32_t N, C0, C1, H, W;     /* low-res sizes; output is [N,C0+C1,2H,2W] */
  int32_t bcast0, bcast1;
  const float* x0;
  const float* x1;
  const float* scale0;
  const float* shift0;
  const float* scale1;
  const float* shift1;
} avsep_cat_desc;
int avsep_relu_up2x_fwd(const avsep_cat_desc* d, float* out, avsep_stream_t stream);
/* g0/g1: gradient wrt the pre-ReLU (post-affine) value of each source, masked by (value>0);
 * for a bcast source the gradient is summed over HxW into [N,C].  bstats1 (optional):
 * (sum g1, sum g1*xhat1) for the BN that produced source 1 (needs mean1/invstd1).
 * acc0 != 0: g0 += instead of =.                                                         */
int avsep_relu_up2x_bwd(const avsep_cat_desc* d, const float* dout, float* g0, float* g1,
                        const float* mean1, const float* invstd1, double* bstats1, int32_t acc0,
                        avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * prepare: +1e-10, log-frequency warp (grid_sample bilinear/zeros/align_corners=False on the
 * utils.py:12-26 grid), loss weight, ground-truth masks, log  (main.py:51-95).
 * mags: [S][B,1,Fin,T] contiguous as one buffer [S,B,Fin,T].  warp==0 -> Fout==Fin, no resample.
 * Outputs [B,1,Fout,T]: mag_mix_w, log_mag_mix, weight; [S,B,Fout,T]: mags_w, gt.
 * ------------------------------------------------------------------------- */
int avsep_prepare(const float* mag_mix, const float* mags, int32_t S, int32_t B, int32_t Fin,
                  int32_t T, int32_t Fout, int32_t warp, int32_t weighted, int32_t binary,
                  float* mag_mix_w, float* mags_w, float* log_mag_mix, float* weight, float* gt,
                  avsep_stream_t stream);
/* grid_sample of [B,C,Hin,Win] on warpgrid(B,Hout,Wout,warp) — the un-warp of main.py:216-220
 * (warp=0) and the generic resample. */
int avsep_warp(const float* x, int32_t BC, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
               int32_t warp, float* y, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Bottleneck fusion (models/fusion_net.py).  x: [B,2*Dc,F,T] bottleneck; v: [C=2][B,Dc,H,W].
 * kind: 0 hidsep/CoLoc, 1 CoLoc_Sel, 2 MixVis (v is then ONE map [B,Dc,H,W]);  att: 0 cos, 1 sig.
 * Outputs: feat [B,2*Dc] (the two broadcast vectors), att_maps [B,2,H,W], match_part [B]
 * (per-sample match-loss terms; the caller averages), best [B] (winning permutation),
 * pool_idx [B,2*Dc] argmax of the global max-pool, sel_idx [B,2*Dc] argmax used for feat.
 * bwd: dfeat [B,2*Dc]; dmaps optional [B,2,H,W]; the match-loss cotangent is the DEVICE scalar
 * *dmatch (NULL = 1) times the host factor dmatch_scale (1/B for the batch mean); the gradient
 * wrt x is ADDED into dx_accum [B,2*Dc,F,T]; dv0/dv1 [B,Dc,H,W] are overwritten.
 * ------------------------------------------------------------------------- */
int avsep_fusion_av_fwd(const float* x, const float* v0, const float* v1, int32_t B, int32_t Dc,
                        int32_t FT, int32_t HW, int32_t kind, int32_t att, float* a_pool,
                        int32_t* pool_idx, float* feat, int32_t* sel_idx, float* att_maps,
                        float* match_part, int32_t* best, avsep_stream_t stream);
int avsep_fusion_av_bwd(const float* x, const float* v0, const float* v1, int32_t B, int32_t Dc,
                        int32_t FT, int32_t HW, int32_t kind, int32_t att, const float* a_pool,
                        const int32_t* pool_idx, const int32_t* sel_idx, const float* att_maps,
                        const int32_t* best, const float* dfeat, const float* dmaps,
                        const float* dmatch, float dmatch_scale, float* dx_accum, float* dv0,
                        float* dv1, avsep_stream_t stream);
/* AO branch (fusion_net.py:93-104): feat = swapped global-max-pooled blocks. draws: uint8[B]. */
/* CoLoc (kind 0) for C = 2..4 sources — BUILD-DEFINED generalisation of fusion_net.py:35-72,93-104 (the reference
 * hard-codes C = 2; rules in csrc/fusion_n.hip and DESIGN.md §9): x [B,D,F,T], v[c] [B,Dc,H,W] with Dc = D / C, the
 * audio blocks are the first C*Dc pooled channels, all C! permutations in itertools order, first maximum wins;
 * feat [B,D] (remainder channels zero), att_maps [B,C,H,W], match_part [B], best [B] (permutation index).
 * v / dv: HOST arrays of C device pointers.  Audio-only: draws[b] = permutation index (itertools order) of sample b. */
int avsep_fusion_n_av_fwd(const float* x, const float* const* v, int32_t B, int32_t C, int32_t D, int32_t FT,
                          int32_t HW, int32_t att, float* a_pool, int32_t* pool_idx, float* feat, int32_t* sel_idx,
                          float* att_maps, float* match_part, int32_t* best, avsep_stream_t stream);
int avsep_fusion_n_av_bwd(const float* x, const float* const* v, int32_t B, int32_t C, int32_t D, int32_t FT,
                          int32_t HW, int32_t att, const float* a_pool, const int32_t* pool_idx,
                          const int32_t* sel_idx, const int32_t* best, const float* dfeat, const float* dmatch,
                          float dmatch_scale, float* dx_accum, float* const* dv, avsep_stream_t stream);
int avsep_fusion_n_ao_fwd(const float* x, const int32_t* draws, int32_t B, int32_t C, int32_t D, int32_t FT,
                          float* feat, int32_t* pool_idx, avsep_stream_t stream);
int avsep_fusion_n_ao_bwd(const int32_t* draws, int32_t B, int32_t C, int32_t D, int32_t FT,
                          const int32_t* pool_idx, const float* dfeat, float* dx_accum, avsep_stream_t stream);
int avsep_fusion_ao_fwd(const float* x, const uint8_t* draws, int32_t all_zero, int32_t B,
                        int32_t Dc, int32_t FT, float* feat, int32_t* pool_idx,
                        avsep_stream_t stream);
int avsep_fusion_ao_bwd(const uint8_t* draws, int32_t all_zero, int32_t B, int32_t Dc, int32_t FT,
                        const int32_t* pool_idx, const float* dfeat, float* dx_accum,
                        avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Mask loss: activation + weighted BCE/L1/L2 (models/criterion.py:10-49) and the PIT loss
 * matrix (criterion.py:138-178) in one pass.  logits [B,S,FT]; gt [S,B,FT]; weight [B,FT] shared by
 * all targets (w_target_stride 0) or one map per target i at weight + i*w_target_stride.
 * pred [B,S,FT] = activation(logits).  sums: double[B*S*S], sums[b,i,j] = sum_ft w*l(pred_j, gt_i).
 * loss: 0 bce, 1 l1, 2 l2.
 * bwd: dlogits[b,j,ft] = sum_i coef[b,i,j] * w * dl/dlogit(pred_j, gt_i).
 * ------------------------------------------------------------------------- */
int avsep_mask_loss_fwd(const float* logits, const float* gt, const float* weight,
                        int64_t w_target_stride, int32_t B, int32_t S, int32_t FT, int32_t act,
                        int32_t loss, float* pred, double* sums, avsep_stream_t stream);
int avsep_mask_loss_bwd(const float* logits, const float* gt, const float* weight,
                        int64_t w_target_stride, const float* coef, int32_t B, int32_t S, int32_t FT,
                        int32_t act, int32_t loss, float* dlogits, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * STFT / iSTFT (librosa semantics, dataset/base.py:142-147, utils.py:101-104): periodic Hann,
 * center=True, DFT as GEMM on the f32 MFMA.  wav [R,L]; mag/phase [R,n_fft/2+1,frames].
 * The bases (window folded in, cos then -sin) are conv operands built once by avsep_stft_basis
 * into caller buffers of avsep_stft_basis_floats() floats; reflect=1 -> librosa<0.10 pad mode,
 * 0 -> zeros (librosa>=0.10).  phase may be NULL.
 * ------------------------------------------------------------------------- */
size_t avsep_stft_basis_floats(int32_t n_fft, int32_t inverse);
int avsep_stft_basis(int32_t n_fft, float* fwd_basis, float* inv_basis, avsep_stream_t stream);
size_t avsep_stft_workspace_bytes(int32_t R, int32_t L, int32_t n_fft, int32_t hop);
int avsep_stft_mag(const float* wav, int32_t R, int32_t L, int32_t n_fft, int32_t hop,
                   int32_t reflect, const float* basis, float* mag, float* phase, void* workspace,
                   size_t workspace_bytes, avsep_stream_t stream);
size_t avsep_istft_workspace_bytes(int32_t R, int32_t n_fft, int32_t frames);
int avsep_istft(const float* mag, const float* phase, int32_t R, int32_t n_fft, int32_t hop,
                int32_t frames, const float* inv_basis, float* wav, int32_t out_len, void* workspace,
                size_t workspace_bytes, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Misc per-frame visual ops and the optimizer.
 * ------------------------------------------------------------------------- */
/* nn.MaxPool2d(3,2,1) of act(scale[c]*x + shift[c]) (the ResNet stem's BN + ReLU folded in; scale NULL = plain). */
int avsep_maxpool3x3s2_fwd(const float* x, const float* scale, const float* shift, int32_t act, int32_t C,
                           int32_t NC, int32_t H, int32_t W, float* y, int32_t* idx, avsep_stream_t stream);
int avsep_maxpool3x3s2_bwd(const float* dy, const int32_t* idx, int32_t NC, int32_t H, int32_t W,
                           float* dx, avsep_stream_t stream);
/* Space-to-depth of the frames for the stem (vision_net.py:111, resnet conv1 7x7/s2/p3 == a 4x4/s1/p0 conv over it):
 * xs [N, Cp, H/2+3, W/2+3], xs[n][(dy*2+dx)*C + c][i+2][j+2] = x[n][c][2i+dy][2j+dx], zero elsewhere; H, W even, Cp >= 4*C. */
int avsep_space_to_depth2(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Cp, float* xs,
                          avsep_stream_t stream);
/* Stem tail backward, fused (vision_net.py:111-117: conv1 -> bn1 -> relu -> maxpool): from g = dL/d(pooled), the forward's
 * arg-max positions idx and the RAW conv output y with its BatchNorm rows (scale, shift, mean, invstd):
 *   _stats: bstats[2*C] (pre-zeroed) += (sum dz, sum dz*xhat), dz = relu'(scale*y+shift) * maxpool_backward(g);
 *   avsep_bn_bwd_coeffs turns them into (p,q,r);  _apply: dy = p*dz + q*y + r.  dz is never materialised. */
int avsep_maxpool_bn_relu_bwd_stats(const float* g, const int32_t* idx, const float* y, const float* scale,
                                    const float* shift, const float* mean, const float* invstd, int32_t N, int32_t C,
                                    int32_t H, int32_t W, double* bstats, avsep_stream_t stream);
int avsep_maxpool_bn_relu_bwd_apply(const float* g, const int32_t* idx, const float* y, const float* scale,
                                    const float* shift, const float* pqr, int32_t N, int32_t C, int32_t H, int32_t W,
                                    float* dy, avsep_stream_t stream);
/* y[b,c,hw] = mean_t x[b*T+t,c,hw]  (vision_net.py:134-135) and its transpose. */
int avsep_temporal_mean_fwd(const float* x, int32_t B, int32_t T, int32_t CHW, float* y,
                            avsep_stream_t stream);
int avsep_temporal_mean_bwd(const float* dy, int32_t B, int32_t T, int32_t CHW, float* dx,
                            avsep_stream_t stream);
/* SGD with momentum + weight decay (torch.optim.SGD semantics, main.py:547):
 * g += wd*p; buf = first ? g : mom*buf + g; p -= lr*buf.  grad_scale multiplies g first
 * (1/world after the RCCL sum). */
int avsep_sgd_momentum(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                       float weight_decay, float grad_scale, int32_t first, avsep_stream_t stream);
/* InnerProd / Bias synthesizer (models/synthesizer_net.py:12-19): z[b,hw] = sum_k img[b,k]*scale[k]*snd[b,k,hw] + bias */
int avsep_innerprod_fwd(const float* img, const float* snd, const float* scale, const float* bias,
                        int32_t B, int32_t K, int32_t HW, float* z, avsep_stream_t stream);
/* The synthesizer's inference helpers (models/synthesizer_net.py:21-38; scale NULL for `Bias`):
 * forward_nosum     z[b,k,hw] = img[b,k]*scale[k]*snd[b,k,hw] + bias                         z [B,K,HW]
 * forward_pixelwise z[b,p,hw] = sum_k imgs[b,k,p]*scale[k]*snd[b,k,hw] + bias  (imgs [B,K,P]) z [B,P,HW], K even:
 *                   the per-sample [P x K] x [K x HW] contraction on the f32 MFMA. */
int avsep_innerprod_nosum(const float* img, const float* snd, const float* scale, const float* bias,
                          int32_t B, int32_t K, int32_t HW, float* z, avsep_stream_t stream);
int avsep_innerprod_pixelwise(const float* imgs, const float* snd, const float* scale, const float* bias,
                              int32_t B, int32_t K, int32_t P, int32_t HW, float* z, avsep_stream_t stream);
/* backward: dsnd[b,k,hw] = img[b,k]*scale[k]*dz[b,hw] (optional) and r[b,k] = sum_hw snd[b,k,hw]*dz[b,hw],
 * from which the caller forms dimg = scale*r, dscale = sum_b img*r, dbias = sum dz. */
int avsep_innerprod_bwd(const float* img, const float* snd, const float* scale, const float* dz,
                        int32_t B, int32_t K, int32_t HW, float* dsnd, float* r, avsep_stream_t stream);

/* Separation metrics (main.py:260-266): per row r the fp64 inner products
 * sums[3r..] += (<est,ref>, <ref,ref>, <est,est>) over L samples; SI-SDR and SDR are ratios of them. */
int avsep_sdr_sums(const float* est, const float* ref, int32_t R, int32_t L, int64_t est_stride,
                   int64_t ref_stride, double* sums, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Long-form separation (csrc/longform.hip): one recording of F STFT frames is cut into K windows of W frames whose start
 * frames `starts` [K] (int32, strictly ascending, >= 0) overlap; the windows go through the network as one batch and their
 * masks are blended back on the recording's linear-frequency grid.  The reference only ever processes one W = 256 tile.
 * mag: [Fin, F] whole-recording magnitude; masks: [K, N, Fout, W] warped per-window masks.  K, Fin, N <= 65535.
 * ------------------------------------------------------------------------- */
/* The network input of every window without materialising the [Fin, W] slices: per window k what inference.py:433-475
 * (+1e-10, grid_sample on warpgrid(.., Fout, W, warp=True) of utils.py:12-26, log) computes from mag[:, s_k : s_k + W];
 * frames past F read as 0 (then +1e-10).  mag_w, log_mag_w: [K, 1, Fout, W]. */
int avsep_window_prepare(const float* mag, int32_t Fin, int32_t F, const int32_t* starts, int32_t K, int32_t Fout,
                         int32_t W, float* mag_w, float* log_mag_w, avsep_stream_t stream);
/* How well the sources of consecutive windows agree where the windows overlap (the audio-only branch has no fixed source
 * order): D[k,i,j] = sum_f sum_c |m[k,i,f,c+d_k] - m[k+1,j,f,c]|, d_k = s[k+1] - s[k], c in [0, W - d_k); 0 when they
 * do not overlap.  D: float64 [K-1, N, N], K >= 2.  One workgroup per entry, fixed summation order, no atomics: the
 * result is bit-identical from run to run (the host takes an argmin over it). */
int avsep_window_agreement(const float* masks, const int32_t* starts, int32_t K, int32_t N, int32_t Fout, int32_t W,
                           double* D, avsep_stream_t stream);
/* Cross-faded masks x mixture magnitude (main.py:205-246 for a recording of any length):
 *   M[n,f,t] = sum_k w(t-s_k) * unwarp(m[k, perm[k,n]])(f, t-s_k) / sum_k w(t-s_k)   over windows with 0 <= t-s_k < W,
 *   w(j) = min(j+1, W-j);   out[n,c,f,t] = mag[c,f,t] * (binary ? (M > thres) : M)      (threshold after blending).
 * unwarp = grid_sample on warpgrid(.., Fin, W, warp=False) (utils.py:12-26), per window, time axis resampled too, as
 * avsep_warp(.., warp=0) does.  A frame covered by ONE window gets that window's un-warped mask unchanged, so a one-tile
 * recording reproduces avsep_warp + threshold + multiply bit for bit.  perm: int32 [K, N], entries in [0, N) (others
 * contribute nothing).
 * mag: [C, Fin, F], one magnitude per channel the recording keeps (C = 1: the down-mix alone).  The model hears the down-mix
 * and its masks are functions of (source, bin, frame) only: M is blended once per (n, f, t) and multiplied into the C
 * magnitudes, so out[:, c] does not depend on the other channels.  out: [N, C, Fin, F], the layout avsep_istft takes as N*C
 * rows ([N, Fin, F] at C = 1); mask_out (optional, may be null): the blended M, [N, Fin, F].  C <= 65535; offsets are formed
 * in 64 bits ([N, C, Fin, F] passes 2^31 elements on a multi-hour recording). */
int avsep_mask_stitch(const float* masks, const int32_t* starts, const int32_t* perm, const float* mag, int32_t K,
                      int32_t N, int32_t Fout, int32_t W, int32_t C, int32_t Fin, int32_t F, int32_t binary, float thres,
                      float* out, float* mask_out, avsep_stream_t stream);
/* The visual feature of every window from the per-frame features of a clip (vision_net.py:126-147, forward_multiframe, for
 * frame ranges that overlap as the windows do).  f: [T, P] fp32, one row per video frame (P = Dc*h*w for feature maps, Dc for
 * pooled vectors); ranges: int32 [K, 2] on the device, row k = (first, count), the frames of window k; out: [K, P].  One
 * launch serves all windows.
 *   op 0, mean: out[k,p] = (f[first,p] + f[first+1,p] + ... + f[first+count-1,p]) / (float)count.  The sum starts from
 *         f[first,p] and adds one frame at a time in ascending frame order, in fp32, without a tree and without atomics; one
 *         IEEE (correctly rounded) division follows.  The result is a pure function of the inputs: a NumPy float32 loop in
 *         this order reproduces it bit for bit, and count = 1 returns the frame unchanged.  What forward_multiframe(pool=False)
 *         gives for a window's frames, and avgpool over them for pooled vectors.
 *   op 1, max:  out[k,p] = max over the range (inputs free of NaN); with pool_type maxpool the 3-D max pool is the max over
 *         frames of the per-frame pooled vectors.
 * Inside the kernel first is clamped to [0, T-1] and count to [1, T-first]: a bad table never becomes an out-of-range read.
 * Rows are read with 16-byte loads when P % 4 == 0 and f and out are 16-byte aligned, one element at a time otherwise.
 * Every offset is formed in 64 bits (T*P passes 2^31 for half an hour of 30 fps video at 256 x 14 x 14).  T, K, P >= 1,
 * K <= 65535, op in {0, 1}, no null pointer: anything else is AVSEP_ERR_ARG before any launch. */
int avsep_window_reduce(const float* f, const int32_t* ranges, int32_t T, int32_t K, int64_t P, int32_t op, float* out,
                        avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Multichannel Wiener filter over the stitched source images (csrc/mwf.hip): what turns N masked copies of a C-channel
 * recording into N sources with their own place in the spatial image.  X[c,f,t] = xmag * exp(i xph) is the channels' STFT
 * [C, Fin, F]; Y_n[c,f,t] = ymag * exp(i yph) the current source images [N, C, Fin, F].  One pass, all in fp32:
 *   1. v_n[f,t] = (1/C) sum_c ymag[n,c,f,t]^2
 *   2. R_n[f]   = (sum_t Y_n[:,f,t] Y_n[:,f,t]^H) / max(sum_t v_n[f,t], FLT_MIN)     C x C Hermitian; a silent source: R_n = 0
 *   3. S[f,t]   = sum_n v_n[f,t] R_n[f] + (reg * tr(sum_n v_n R_n) / C + FLT_MIN) I
 *   4. S z = X[:,f,t]                                  one Cholesky solve per bin, shared by the sources
 *   5. Y_n'[:,f,t] = v_n[f,t] R_n[f] z                 (exactly 0 where v_n = 0), stored as magnitude and atan2 phase (0 at 0)
 * The regulariser is relative to the bin's own power (a dual-mono file gives a rank-1 S at every level): the sources of a
 * pass sum to X / (1 + about reg), not to X.  1 <= N <= 8, 1 <= C <= 8, Fin <= 65535, F <= 2^31 - 1 - 4096; every offset into
 * [N, C, Fin, F] is formed in 64 bits.  No atomics: every sum has a fixed order that depends on F alone (threads walk chunks of
 * 2048 frames), so a second call gives the same bits.
 * avsep_mwf_cov:   steps 1-2.  yph is [N, C, Fin, F] when phase_per_source != 0, else [C, Fin, F] shared by the sources (the
 *   first pass: masked magnitudes on the mixture's phase).  cov: f32 [N, Fin, C, C, 2], the full R_n as (re, im), diagonal
 *   imaginary parts exactly 0, upper triangle the exact conjugate of the lower.  ws: avsep_mwf_workspace_bytes(N, C, Fin, F).
 * avsep_mwf_apply: steps 3-5 from cov; out_mag / out_phase [N, C, Fin, F], the layout avsep_istft takes as N*C rows; they must
 *   not alias ymag.  reg >= 0 (0 is only safe where S has full rank).
 * Anything outside these limits, a null pointer or a workspace that is too small is AVSEP_ERR_ARG before any launch (the
 * workspace query returns 0). */
size_t avsep_mwf_workspace_bytes(int32_t N, int32_t C, int32_t Fin, int32_t F);
int avsep_mwf_cov(const float* ymag, const float* yph, int32_t phase_per_source, int32_t N, int32_t C, int32_t Fin, int32_t F,
                  float* cov, float* ws, size_t ws_bytes, avsep_stream_t stream);
int avsep_mwf_apply(const float* xmag, const float* xph, const float* ymag, const float* cov, int32_t N, int32_t C, int32_t Fin,
                    int32_t F, float reg, float* out_mag, float* out_phase, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * The same filter with time-varying spatial covariances, for sources that move through the image (csrc/mwf.hip, DESIGN.md
 * §24 beside §16).  H is the span in frames: a multiple of 64 with 64 <= H <= 4096.  Centres sit at frames k H,
 * k = 0 ... K - 1, K = ceil((F - 1) / H) + 1 (K = 1 for F = 1); frame t lies in segment s = t / H at u = (t - s H) / H, and
 * centre s weighs it with 1 - u, centre s + 1 with u: the hat w_k(t) = max(0, 1 - |t - k H| / H).  Steps 1, 4 and 5 are those
 * above; in their place steps 2 and 3 read
 *   2'. R_n[k,f] = (sum_t w_k(t) Y_n Y_n^H) / max(sum_t w_k(t) v_n[f,t], FLT_MIN)     a source silent over the support: R = 0
 *   3'. R_n[f,t] = (1 - u) R_n[s,f] + u R_n[s + 1,f], used for R_n[f] in S and in Y_n' = v_n R_n[f,t] z
 * The limits on N, C, Fin and F, the 64-bit offsets and the no-atomics rule are those above; every sum has a fixed order that
 * depends on (F, H) alone (a wave walks one segment of H frames), so a second call gives the same bits.
 * avsep_mwf_cov_tv:   steps 1-2'.  ymag, yph and phase_per_source as avsep_mwf_cov.  cov: f32 [N, K, Fin, C, C, 2], every
 *   R_n[k,f] in full as (re, im), diagonal imaginary parts exactly 0, upper triangle the exact conjugate of the lower.
 *   ws: avsep_mwf_tv_workspace_bytes(N, C, Fin, F, H) bytes, two slabs of C (C + 1) + 1 floats per (segment, source, bin row).
 * avsep_mwf_apply_tv: steps 3'-5 from that cov with the same H; out_mag / out_phase [N, C, Fin, F], not aliasing ymag; reg >= 0.
 * An H that is no multiple of 64 or outside 64 ... 4096, anything outside the limits above, a null pointer or a workspace that
 * is too small is AVSEP_ERR_ARG before any launch (the workspace query returns 0). */
size_t avsep_mwf_tv_workspace_bytes(int32_t N, int32_t C, int32_t Fin, int32_t F, int32_t H);
int avsep_mwf_cov_tv(const float* ymag, const float* yph, int32_t phase_per_source, int32_t N, int32_t C, int32_t Fin, int32_t F,
                     int32_t H, float* cov, float* ws, size_t ws_bytes, avsep_stream_t stream);
int avsep_mwf_apply_tv(const float* xmag, const float* xph, const float* ymag, const float* cov, int32_t N, int32_t C, int32_t Fin,
                       int32_t F, int32_t H, float reg, float* out_mag, float* out_phase, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Mixture-consistent phase iterations (csrc/misi.hip; MISI, Gunawan & Sen 2010): give every stem of a mixture a phase of its
 * own.  R = N * G rows: N sources, G groups; a group is the set of N rows that sum to one mixture (G = 1 for mono stems,
 * G = C for channel stems).  mix [G, out_len] with out_len = hop * (frames - 1); mag [N, G, bins, frames] the target
 * magnitudes A; phase the start phase, [G, bins, frames] shared by the sources or, with phase_per_source != 0,
 * [N, G, bins, frames].  iSTFT / STFT below are avsep_istft (synthesis window in the basis, window-sum-square normalisation,
 * centre trim, length out_len) and avsep_stft_mag's transform (reflect or zero padding, `frames` frames).  In fp32:
 *   1. s_n = iSTFT(A_n * exp(i phase))
 *   2. for k = 1 ... iterations:
 *        e  = mix - sum_n s_n                  (n ascending)
 *        Z_n = STFT(s_n + e / N)
 *        s_n = iSTFT(A_n * Z_n / |Z_n|)        (A_n * 1 where Z_n = 0, as atan2f(0, 0) = 0 gives)
 *   3. wav_out [N, G, out_len] = s_n after the last pass: the plain iSTFT of the last spectrum (the stems are not forced to
 *      sum to the mixture); phase_out (optional, may be null) [N, G, bins, frames] = atan2f of the last Z_n.
 * fwd_basis / inv_basis: avsep_stft_basis(n_fft).  1 <= N <= 8, 1 <= G <= 8, iterations >= 1, out_len > n_fft / 2.  One call
 * enqueues every pass on the stream: no host synchronisation, no allocation, no atomics; every sum has a fixed order, so a second
 * call gives the same bits, and the groups are processed one by one, so a call with G groups gives the bits of G calls with
 * one.  Every offset is formed in 64 bits.  A null pointer, a zero size or anything outside these limits is AVSEP_ERR_ARG
 * before any launch (the workspace query returns 0); ws: avsep_misi_workspace_bytes bytes, else AVSEP_ERR_WORKSPACE. */
size_t avsep_misi_workspace_bytes(int32_t N, int32_t G, int32_t n_fft, int32_t hop, int32_t frames);
int avsep_misi(const float* mix, const float* mag, const float* phase, int32_t phase_per_source, int32_t N, int32_t G,
               int32_t n_fft, int32_t hop, int32_t frames, int32_t reflect, int32_t iterations, const float* fwd_basis,
               const float* inv_basis, float* wav_out, float* phase_out_or_null, void* ws, size_t ws_bytes,
               avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Sound-source localisation over a clip (csrc/localise.hip): T video frames against the K windows of one recording.
 * ------------------------------------------------------------------------- */
/* The CoLoc similarity maps of every frame in one launch (replaces one whole forward pass per video frame,
 * inference.py:537-578 calling inference.py:29-160; the maps themselves are fusion_net.py:35-64).
 * x: [K, D, FT] fp32 bottleneck of the K windows; win: int32 [T], the window of frame t (values outside [0, K) are clamped);
 * v: C pointers to [T, Dc, HW] fp32 visual feature maps, Dc = D / C (duet: the same pointer twice); att: 0 cos / 1 sig.
 * Per frame, with k = win[t]: a_i = max over FT of x[k, i*Dc : (i+1)*Dc] (the first C*Dc channels), m[i][c] = att(a_i, v_c[t])
 * exactly as avsep_fusion_n_av_fwd, score_p = sum_c max_hw m[perm_p[c]][c] over the C! permutations in itertools order,
 * best = the FIRST maximum.  maps: [T, C, HW], maps[t, c] = m[perm_best[c]][c]; best: int32 [T]; scores: [T, C!].
 * C in {2, 3}.  The C*C maps of a frame live in LDS: an HW that does not fit is AVSEP_ERR_ARG. */
int avsep_localise_maps(const float* x, const int32_t* win, const float* const* v, int32_t T, int32_t K, int32_t C, int32_t D,
                        int32_t FT, int32_t HW, int32_t att, float* maps, int32_t* best, float* scores, avsep_stream_t stream);
/* Heat maps blended over the frames on the device (replaces the per-frame host round trip inference.py:509-534:
 * normalise, cv2.resize, cv2.applyColorMap, weighted add).  maps: [T*C, h, w] fp32, map m belongs to frame m / C and source
 * m % C; frames: C pointers to [T, 3, H, W] fp32 ImageNet-normalised RGB (duet: the same pointer); table: 256 x 3 uint8 RGB
 * colours on the device; alpha256 in [0, 256].  out: uint8 [C, T, H, W, 3] RGB.  Defined so that integer and fp32 arithmetic
 * in this exact order reproduces it bit for bit:
 *   1. q = (uint8) trunc((255.0f * (m - mn)) / (mx - mn)) per cell, mn / mx = the map's min / max, fp32 round-to-nearest with
 *      IEEE division and no fused multiply-add; mx == mn: q = 0.
 *   2. resize h x w -> H x W, half-pixel centres, replicated border: num = (2X+1)*w - W, x0 = floor(num / 2W),
 *      cx1 = ((num - x0*2W)*2048 + W) / (2W), cx0 = 2048 - cx1, x0 and x0 + 1 clamped to [0, w-1]; the same in y;
 *      level = (q00*cx0*cy0 + q01*cx1*cy0 + q10*cx0*cy1 + q11*cx1*cy1 + 2^21) >> 22.
 *   3. colour = table[level].
 *   4. frame pixel p = clamp(floor((x*std + mean)*255 + 0.5), 0, 255), mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225).
 *   5. out = (colour*alpha256 + p*(256 - alpha256) + 128) >> 8.
 * h, w, H, W <= 65535; the map, the table and H + W resize entries live in LDS (64 KiB), else AVSEP_ERR_ARG. */
int avsep_heatmap_overlay(const float* maps, const float* const* frames, const uint8_t* table, int32_t T, int32_t C, int32_t h,
                          int32_t w, int32_t H, int32_t W, int32_t alpha256, uint8_t* out, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Evaluation visuals (csrc/visuals.hip): the spectrogram, weight and mask images of a whole batch as image bytes.
 * ------------------------------------------------------------------------- */
/* One launch for R images (replaces, per image, utils.py:90-98 magnitude2heatmap, the mask product of main.py:367-369, the
 * clip of main.py:375-376 and the [::-1] row flips of main.py:358-386, all NumPy / OpenCV on the host).
 * mag: [R, F, T] fp32; mask_or_null: [R, F, T] fp32; thres: a NaN means "no threshold"; cell >= 1 frames per image column;
 * reduce: 0 max / 1 mean; log: 0 / 1; table_or_null: 256 x 3 uint8 RGB colours on the device.
 * out: uint8 [R, F, W, ch], W = ceil(T / cell), ch = 3 with a table and 1 (the level itself) without.  Per pixel (r, f, w):
 *   1. the source row is F - 1 - f: low frequencies end up at the bottom of the picture.
 *   2. over the frames t in [w*cell, min((w+1)*cell, T)): p = mag[t] * m(t), ONE fp32 multiply, with m = 1 without a mask,
 *      (mask > thres ? 1 : 0) with a threshold, the mask value without one.
 *   3. c = max of p (a NaN stays, as in numpy.max), or the mean: an fp32 sum in a fixed order divided by the number of frames
 *      actually in the cell.  The order is the frame order for cell <= 32; beyond that lane l of a wave sums frames l, l + 64,
 *      ... in that order and the 64 lane sums meet in a butterfly (xor 32, 16, ... 1).
 *   4. v = log ? log10f(c + 1) * scale : c * scale;  level = v > 255 ? 255 : trunc(v); a negative v and a NaN give level 0
 *      (the reference's astype(uint8) would wrap them).
 *   5. the pixel is table[level], or level.
 * cell = 1, log = 1, scale = 200 with the JET table is magnitude2heatmap followed by the BGR->RGB and row flips; log = 0,
 * scale = 100 the weight image; log = 0, scale = 255 without a table is clip(mask, 0, 1) * 255 truncated.
 * No atomics; a second call gives the same bytes.  Every offset is formed in 64 bits; the work is strided over a bounded
 * grid.  A null mag / out, R, F or T <= 0, cell < 1, reduce or log outside {0, 1} and R * F > 2^31 - 1 are AVSEP_ERR_ARG
 * before any launch. */
int avsep_spec_image(const float* mag, const float* mask_or_null, float thres, int32_t R, int32_t F, int32_t T, int32_t cell,
                     int32_t reduce, int32_t log, float scale, const uint8_t* table_or_null, uint8_t* out,
                     avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Sample-rate conversion (csrc/resample.hip): a rational polyphase FIR resampler, so that a WAV file at any rate goes in
 * and the separated sources come out at the file's own rate.  up = rate_out / g, down = rate_in / g, g = gcd; both in
 * [1, 1280] (8 ... 96 kHz to and from 11 025 Hz; the worst cases are 441/1280 and 147/1280).
 * Filter (the caller builds it in float64 and rounds it ONCE to f32): m = max(up, down), half = 10*m, M = 2*half + 1,
 *   h[i] = up * w[i] / sum(w),  w[i] = (1/m) * sinc((i - half) / m) * kaiser(M, beta = 5.0)[i],   sinc(t) = sin(pi t)/(pi t),
 * which is up * scipy.signal.firwin(M, 1/m, window=('kaiser', 5.0)): scipy.signal.resample_poly's default filter.
 * It is passed as the polyphase table ho: f32 [T, up], T = ceil(M / up), with its columns in OUTPUT order, so that the
 * threads of consecutive outputs read consecutive floats: column t holds the phase of every output j = t (mod up),
 *   p(t) = (t*down + half) mod up,   ho[i][t] = h[p(t) + i*up] where p(t) + i*up < M, else 0.
 * Result, per row r (rows never see each other; samples outside a row are zero: resample_poly's padtype='constant'):
 *   Lout = ceil(L * up / down),   y[r, j] = sum_n x[r, n] * h[j*down - n*up + half]   over 0 <= n < L, filter index in [0, M).
 * Arithmetic: with pos = j*down + half (64-bit), p = pos mod up, n0 = pos div up:
 *   acc = 0;  for i = 0 .. T-1 (in this order):  acc = fma(x[r, n0 - i], f32(h[p + i*up]), acc)   (one f32 rounding per tap),
 * a sample outside [0, L) is 0 and the last tap takes no sample when p + (T-1)*up >= M.  The order depends on (up, down, j)
 * only: not on B, the launch geometry or the run; there are no atomics.  A row gives the same bits alone, inside a batch
 * and on a second call.
 * Frames (x of avsep_resample_poly with in_ch >= 1 and of avsep_resample_split, y of avsep_resample_join and of
 * avsep_resample_poly) are a file's packed little-endian samples at ANY byte address: a data chunk rarely starts on a dword
 * and a three-byte frame never stays on one.  One sample as f32:
 *   AVSEP_SAMPLE_S16  2 bytes, WAVE tag 1           v / 2^15 (exact)
 *   AVSEP_SAMPLE_S24  3 bytes packed, WAVE tag 1    sign-extended v / 2^23 (exact)
 *   AVSEP_SAMPLE_S32  4 bytes, WAVE tag 1           the integer rounded to f32 once (nearest-even), times 2^-31
 *   AVSEP_SAMPLE_F32  IEEE binary32, WAVE tag 3     the bits as they are (no range or NaN check)
 * Down-mix (the mono row of avsep_resample_poly with in_ch = C and row 0 of avsep_resample_split), integer formats: the exact
 *   64-bit sum of the C channels over C * 2^(bits-1), rounded to f32 ONCE.  It is computed as
 *   (float)((double)sum / (double)(C << (bits-1))): sum and divisor are exact in f64 and the f64 -> f32 double rounding of a
 *   quotient is innocuous at 53 >= 2*24 + 2 bits.  F32: the channels added in f64 in the order c = 0 ... C-1, divided by C in
 *   f64, rounded to f32 once.  One channel (C = 1) is the sample itself.  The conversion happens while the tile is staged: no
 *   f32 copy of the file exists.
 * Output formats, of exactly the f32 value v of the chain: S16 = clip(rintf(v * 2^15), -2^15, 2^15 - 1), S24 =
 *   clip(rintf(v * 2^23), -2^23, 2^23 - 1), ties to even (the products are exact), little-endian; F32 the accumulator's bits,
 *   not clipped.  There is no S32 output (an f32 value has 24 significant bits) and no dither.
 * A format changes only what is staged and how a result is stored, never the chain.  No alignment is ever required of frames; S16
 *   frames on a 2-byte boundary (and f32 rows, S16 / F32 outputs on their own boundary) are moved with typed loads and stores
 *   in place of byte assembly: the same values, chosen by the entry point from the formats and addresses it is handed.
 * avsep_resample_poly: in_ch = 0: x is f32 [B, L] on a 4-byte boundary and in_fmt must be AVSEP_SAMPLE_F32; in_ch = C in
 *   [1, 256]: x is frames [L, C] of in_fmt (B must be 1), down-mixed.  y: [B, Lout] samples of out_fmt, packed.
 * 1 <= L, Lout < 2^31, B <= 65535; anything else, a format code outside the table or a null pointer is AVSEP_ERR_ARG before
 * any launch.
 * ------------------------------------------------------------------------- */
#define AVSEP_SAMPLE_S16 1
#define AVSEP_SAMPLE_S24 2
#define AVSEP_SAMPLE_S32 3
#define AVSEP_SAMPLE_F32 4
int avsep_resample_poly(const void* x, const float* ho, int32_t B, int32_t L, int32_t up, int32_t down, int32_t in_ch,
                        int32_t in_fmt, int32_t out_fmt, void* y, avsep_stream_t stream);
/* The two ends of a pipeline that keeps a file's channels apart, 1 <= C <= 8 (up to 7.1); filter table, formats, limits and
 * the per-output arithmetic are avsep_resample_poly's (one chain per output, its order a function of (up, down, j) only), so
 * every value below is bit for bit the value avsep_resample_poly gives for the same row.
 * avsep_resample_split: x is frames [L, C] of in_fmt; y is f32 [1 + C, Lout].  Row 0 is the down-mix, what
 *   avsep_resample_poly(in_ch = C) gives; row 1 + c is channel c, what avsep_resample_poly(in_ch = 0) gives for that channel
 *   as an f32 row.  One pass over the file: no de-interleaved copy of it exists.
 * avsep_resample_join: x is f32 [C, L]; y is frames [Lout, C] of out_fmt, y[j, c] the out_fmt form of the value
 *   avsep_resample_poly gives row c.  A workgroup makes all C channels of its frames and stores them as whole frames: whole
 *   dwords between a head and a tail of up to three bytes, whatever the address. */
int avsep_resample_split(const void* x, const float* ho, int32_t L, int32_t C, int32_t up, int32_t down, int32_t in_fmt,
                         float* y, avsep_stream_t stream);
int avsep_resample_join(const float* x, const float* ho, int32_t C, int32_t L, int32_t up, int32_t down, int32_t out_fmt,
                        void* y, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Full-band stems (csrc/fullband.hip; avsep_amd/resample.py band_extend): the model hears a file at its own rate, so a stem
 * ends at that rate's Nyquist; what the file holds above it, high = file - up(down(file)), is handed to the sources under a
 * time-varying gain.  N sources, G rows per source (1 for mono stems, C for channel stems); 1 <= N, G <= 8.
 * avsep_band_gains: stem_mag f32 [N, G, bins, F], mix_mag f32 [G, bins, F], 1 <= lo_bin < bins, F >= 1 -> gains f32 [N, G, F],
 *   the share of the mixture's RMS amplitude source n holds over the bins [lo_bin, bins) of frame t.  With B = bins - lo_bin:
 *     num = 0;  for f = lo_bin .. bins-1 (in this order):  num = fma(stem_mag[n,g,f,t], stem_mag[n,g,f,t], num)
 *     den = 0;  for f = lo_bin .. bins-1 (in this order):  den = fma(mix_mag[g,f,t], mix_mag[g,f,t], den)
 *     gains[n,g,t] = min(1, sqrt(num / (den + 1e-20f * (float)B)))        (f32, division and root correctly rounded)
 *   A frame whose sums are zero gets exactly 0, a source at or above the mixture exactly 1.  The order depends on
 *   (bins, lo_bin) only; there are no atomics: a second call gives the same bits and a (n, g) row gives the same bits alone
 *   as inside a batch.  One thread per (g, t) walks the bins (F is the contiguous axis: coalesced) with den formed once.
 * avsep_band_extend: stems f32 [N, G, Lm] at the model's rate; low f32 [G, Ll], Ll >= Lm, the model-rate mixture rows the
 *   stems were made from (not trimmed to Lm: the filter sees real samples past the stems' end); file f32 [G, Lf] the same
 *   rows at the file's rate; gains f32 [N, G, F]; hop the STFT hop of the gains' frames (frame t is centred on model sample
 *   t * hop); ho the polyphase table of (up, down) above, up / down = file rate / model rate > 1 -> out f32 [N, G, Lout],
 *   Lout = ceil(Lm * up / down).  With chain(row, L)[j] exactly the per-output arithmetic of avsep_resample_poly above (same
 *   tap order, one fma per tap, samples outside [0, L) zero), per output j:
 *     s   = chain(stems[n,g], Lm)[j]          the bits avsep_resample_poly gives that row
 *     l   = chain(low[g], Ll)[j]              once per (g, j), shared by the N sources
 *     h   = j < Lf ? file[g,j] - l : 0
 *     num = j * down (64-bit),  den = up * hop           output j sits at model sample j * down / up
 *     t0  = min(num div den, F-1),  t1 = min(t0 + 1, F-1)
 *     fr  = (float)(num - t0 * den) / (float)den         both exact in f32 while t0 < F-1: den < 2^24
 *     gi  = fma(fr, gains[n,g,t1] - gains[n,g,t0], gains[n,g,t0])
 *     out[n,g,j] = fma(gi, h, s)
 *   Past the last frame t1 = t0, so gi = gains[n,g,F-1] whatever fr is.  Gains of 0 give avsep_resample_poly's bits; with
 *   N = 1, gains of 1 and stems = low the file comes back to one rounding.  The order depends on (up, down, j) only; there
 *   are no atomics: a row gives the same bits alone, inside a batch and on a second call.  A workgroup stages its tile of
 *   low[g] and of the N stem rows of that g in LDS and produces its outputs for every n.
 *   up > down, both in [1, 1280]; 1 <= hop <= 4096; F >= 1; Lm, Lf >= 1; Lout < 2^31.  Every offset is formed in 64 bits.
 * Anything outside these limits or a null pointer is AVSEP_ERR_ARG before any launch.
 * ------------------------------------------------------------------------- */
int avsep_band_gains(const float* stem_mag, const float* mix_mag, int32_t N, int32_t G, int32_t bins, int32_t F, int32_t lo_bin,
                     float* gains, avsep_stream_t stream);
int avsep_band_extend(const float* stems, const float* low, const float* file, const float* gains, const float* ho, int32_t N,
                      int32_t G, int32_t Lm, int32_t Ll, int32_t Lf, int32_t F, int32_t hop, int32_t up, int32_t down, float* out,
                      avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Stem levels (csrc/levels.hip; avsep_amd/levels.py): what ITU-R BS.1770-4 loudness and true peak need from every sample of
 * R rows x f32 [R, L] in device memory.  float64 throughout (a sample is converted once), no atomics, no waveform written;
 * every sum has a fixed order, so a row gives the same bits alone, inside a batch and on a second call.
 * avsep_loudness_energies: sos is 12 doubles in HOST memory, read before the call returns: two biquads b0 b1 b2 1 a1 a2
 *   (scipy's sos rows; every value finite, a0 = 1), applied in cascade from rest at sample 0 of every row (transposed
 *   direct form II).  E f64 [R, S], S = L div h: E[r, s] = sum of y^2 over the samples [s*h, (s+1)*h) of the filtered row
 *   y; the tail L mod h counts nowhere.  The row is cut into pieces by a plan that depends on h only (a sub-block is
 *   ceil(h / 128) pieces of floor or ceil of their mean length; none straddles a sub-block edge): the pieces run from rest,
 *   their start states follow from v' = M v + e with the 4x4 transition M of a piece (built in float64 inside the call),
 *   then they run again from their true state and their sums are added per sub-block in ascending order.  Hence the first
 *   S' energies of a row do not change when L grows.  1 <= R <= 65535, 1 <= h <= L < 2^31.
 * avsep_true_peak: taps f64 [21, os] in DEVICE memory, the polyphase table of an interpolation filter g of 20*os + 1 taps,
 *   taps[i][p] = g[p + i*os] (0 past the filter's end), os in {1, 2, 4}.  peaks f64 [R, 2]: peaks[r, 0] = max_n |x[r, n]|,
 *   peaks[r, 1] = the maximum of that and of |u[m]| over m in [0, os*L), where with pos = m + 10*os, p = pos mod os,
 *   n0 = pos div os:  u[m] = sum_{i = 0 .. 20, in this order} fma(x[r, n0 - i], taps[i][p], .), samples outside [0, L) being 0:
 *   avsep_resample_poly's indexing at down = 1.  A NaN or infinite sample makes both peaks of its row +inf.  The maxima are
 *   taken per workgroup and then over the workgroups' partials: exact, whatever the order.  1 <= R <= 65535, 1 <= L,
 *   os*L < 2^31.
 * Anything outside these limits or a null pointer is AVSEP_ERR_ARG before any launch (the workspace query returns 0); ws:
 * the query's bytes, else AVSEP_ERR_WORKSPACE. */
size_t avsep_loudness_energies_workspace_bytes(int32_t R, int32_t L, int32_t h);
int avsep_loudness_energies(const float* x, const double* sos, int32_t R, int32_t L, int32_t h, double* E, void* ws,
                            size_t ws_bytes, avsep_stream_t stream);
size_t avsep_true_peak_workspace_bytes(int32_t R, int32_t L);
int avsep_true_peak(const float* x, const double* taps, int32_t R, int32_t L, int32_t os, double* peaks, void* ws, size_t ws_bytes,
                    avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * Linked look-ahead true-peak limiter (csrc/levels.hip; avsep_amd/levels.py limit): x f32 [P][C][L] in device memory, P
 * programmes of C rows; ONE gain curve per programme, applied to all of its rows, so that stems keep their balance and sum
 * to the limited mixture as well as they summed to the mixture.  taps and os are avsep_true_peak's; w f64 [2A + 1] in DEVICE
 * memory, w[k + A] = (1 + cos(pi k / (A + 1))) / sum for k = -A .. A (symmetric, sum 1, built by the caller); G = pre_gain,
 * c = ceiling (linear).  Per programme, float64 throughout:
 *   1 detector  p[n] = max over the C rows of max(|x[n]|, |u[os*n + q]|, q = 0 .. os-1), u avsep_true_peak's oversampled row
 *               (one device function serves both: max_n p[n] is bit for bit the programme's largest true peak).
 *   2 required  r[n] = min(1, c / (G * p[n])) for 0 <= n < L, 1 outside; p = 0 gives 1.
 *   3 hold      h[j] = min of r over |i - j| <= A, for -A <= j < L + A: the envelope reaches A samples past both ends.
 *   4 smooth    g[n] = 1 - sum_{k = -A .. A, ascending} w[k + A] * (1 - h[n + k]): an untouched stretch gives exactly 1.
 *   5 apply     y[row][n] = the f32 nearest to the float64 product x[row][n] * (G * g[n]).
 * Every h[n + k] is a minimum over a window that holds n, so in exact arithmetic g[n] <= r[n] and |y[n]| <= c: the gain never
 * rises above what the oversampled detector asks for at n.  (The TRUE peak of y may still pass c a little, because the
 * modulation moves the inter-sample peaks: the caller measures y and trims.)
 * y may be x itself.  gain: f64 [P][L] or NULL.  stats f64 [P][3]: max_n p[n] (not scaled by G; +inf when a sample of the
 * programme is NaN or infinite), min_n g[n], the number of n with g[n] < 1.  No atomics; the reductions are a maximum, a
 * minimum and a count of integers (order-free) and the sum of step 4 runs in ascending k: a programme gives the same bits
 * alone, inside a batch and on a second call.  1 <= P <= 65535, 1 <= C <= 64, 1 <= L, os*L < 2^31, os in {1, 2, 4},
 * 1 <= A <= 2048, pre_gain finite and > 0, 0 < ceiling <= 1.  Anything outside these limits or a null pointer (but gain) is
 * AVSEP_ERR_ARG before any launch (the workspace query returns 0); ws: the query's bytes, else AVSEP_ERR_WORKSPACE. */
size_t avsep_limiter_workspace_bytes(int32_t P, int32_t C, int32_t L);
int avsep_limiter(const float* x, const double* taps, const double* w, int32_t P, int32_t C, int32_t L, int32_t os, int32_t A,
                  double pre_gain, double ceiling, float* y, double* gain, double* stats, void* ws, size_t ws_bytes,
                  avsep_stream_t stream);

/* ---- Frames as shot (csrc/frames.hip; avsep_amd/frames.py): uint8 RGB frames [T][H][W][3] -> out f32 [T][3][S][S], bit for bit
 * dataset.VideoTransform: Pillow's 8-bit bicubic resize to (w, h), the crop of S x S at (crop_i, crop_j) of the resized image
 * (rows, columns; either may be negative or reach past the image: pixels outside it are 0), the left-right flip, and
 * (v / 255 - mean) / std.  All floating-point arithmetic is the host's: the kernel is handed, in DEVICE memory,
 *   hcoef int32 [w][kh], hbound int32 [w][2]: per column of the resized image its kh fixed-point weights (22 fractional bits,
 *     those past the count are 0) and (first input column, count); vcoef [h][kv], vbound [h][2] likewise for the rows.
 *     kh = 2 * ceil(2 * max(W / w, 1)) + 1 and kv = 2 * ceil(2 * max(H / h, 1)) + 1, Pillow's, each at most 81 (a downscale of
 *     up to 20); an axis that keeps its size has the identity table.  first and count are clamped to the input, so a wrong
 *     table gives wrong pixels and never an access outside `frames`.
 *   lut f32 [256][3]: the normalised value of every byte value per channel.
 * Horizontal pass: mid = clip((2^21 + sum_k hcoef[x][k] * frames[.., first + k, c]) >> 22, 0, 255) in int32 with an arithmetic
 * shift, rounded to uint8; vertical pass: the same rule over mid.  out[t][c][y][x'] = lut[v][c] with v the cropped pixel and
 * x' = S - 1 - x under flip.  out_u8 (or NULL): uint8 [T][S][S][3], the pixels v themselves, after crop and flip.
 * 1 <= T <= 65535, 1 <= H, W, h, w <= 4096, 8 <= S <= 1024, |crop_i|, |crop_j| <= 4096, flip 0 | 1; `frames` may start at any
 * byte.  Anything else, or a null pointer other than out_u8, is AVSEP_ERR_ARG before any launch. */
int avsep_frames_prepare(const uint8_t* frames, int32_t T, int32_t H, int32_t W, const int32_t* hcoef, const int32_t* hbound, int32_t w,
                         int32_t kh, const int32_t* vcoef, const int32_t* vbound, int32_t h, int32_t kv, int32_t S, int32_t crop_i,
                         int32_t crop_j, int32_t flip, const float* lut, float* out, uint8_t* out_u8, avsep_stream_t stream);

/* Frames of many sizes in one launch (the training loader: B x N clips, each with its own size, crop and flip).  `pixels` is one
 * uint8 DEVICE buffer of pixel_bytes bytes that holds the n RGB frames back to back, each [H][W][3] and starting at any byte;
 * `tables` one int32 DEVICE buffer of table_words words that holds the coefficient and bound tables of every axis pair the
 * batch has, in the layout above (frames of one axis pair share them).  One row per frame says where everything is: */
typedef struct avsep_frames_row {
  int64_t pix_off;                          /* the frame's first byte in `pixels` */
  int64_t out_off;                          /* the first float of its channel 0 in `out` */
  int32_t H, W, w, h, kh, kv;               /* as for avsep_frames_prepare */
  int32_t hcoef, hbound, vcoef, vbound;     /* word offsets of the four tables in `tables` */
  int32_t crop_i, crop_j, flip;
  int32_t TR, max_cols, in_bytes, mid_rows; /* launch sizing: written by avsep_frames_batch_plan, never by the caller */
  int32_t reserved;
} avsep_frames_row;
/* Frame r writes out[out_off + c * plane + y * S + x'], c = 0 .. 2: plane = S*S and out_off = r*3*S*S give [n][3][S][S];
 * plane = T*S*S and out_off = (b*3*T + t)*S*S give the loader's [B][3][T][S][S].
 * avsep_frames_batch_plan (host only, nothing is launched): checks n HOST rows against the limits of avsep_frames_prepare
 * (sides, S, kh / kv as the sizes imply and <= 81, crop, flip), every pixel range inside pixel_bytes, every table range inside
 * table_words and every output range out_off + 2*plane + S*S inside out_floats (plane >= S*S); fills in the rows' launch
 * sizing and returns launch[0] = grid y (S over the smallest tile height of the batch), launch[1] = dynamic LDS bytes (the
 * largest any frame needs), launch[2] = that smallest tile height.  1 <= n <= 65535.  On AVSEP_ERR_ARG the rows' sizing fields
 * are unspecified.
 * avsep_frames_prepare_batch: rows = the planned rows in DEVICE memory, grid_y and lds_bytes = the plan's answer.  The kernel
 * does not trust the device rows with addresses: every offset, count and size it reads is clamped or checked against
 * pixel_bytes, table_words, out_floats and lds_bytes, so a wrong row gives wrong pixels or an untouched output, never an
 * access outside a buffer.  A null pointer, n outside 1 .. 65535, S outside 8 .. 1024, plane < S*S, out_floats < 2*plane + S*S,
 * grid_y outside ceil(S/32) .. S or lds_bytes outside 3072 .. 54400 is AVSEP_ERR_ARG before any launch. */
int avsep_frames_batch_plan(avsep_frames_row* rows, int32_t n, int32_t S, int64_t pixel_bytes, int64_t table_words,
                            int64_t out_floats, int64_t plane, int32_t* launch);
int avsep_frames_prepare_batch(const uint8_t* pixels, int64_t pixel_bytes, const avsep_frames_row* rows, int32_t n,
                               const int32_t* tables, int64_t table_words, int32_t S, const float* lut, float* out,
                               int64_t out_floats, int64_t plane, int32_t grid_y, int32_t lds_bytes, avsep_stream_t stream);

/* ---- Baseline JPEG frames (csrc/jpeg.hip, csrc/jpeg_parts.h; avsep_amd/jpeg.py): SOF0, 8 bit, Huffman, one interleaved scan,
 * grey or YCbCr with luma sampling 1x1, 2x1 or 2x2 -> uint8 RGB [H][W][3], bit for bit libjpeg-turbo's default decoder (islow
 * inverse DCT, fancy upsampling), which is what Pillow gives.  The host reads the markers and hands over, in DEVICE memory,
 *   bytes  uint8 [nbytes]: the entropy-coded bytes of the images back to back (stuffed FF 00 still in them);
 *   tables int32 [table_words]: quantisation tables (64 words, NATURAL order) and Huffman tables (546 words: look[256] =
 *     (length << 8) | value by the next 8 bits, 0 = a longer code; maxcode[17] by length, -1 = none; valoff[17], a code's value
 *     is values[valoff[length] + code]; values[256]) anywhere in it, shared by the images that have them;
 *   one row per image and one per entropy-coded segment (a file without restart intervals is one segment).  The image row is
 *   the one the encoder below takes too.  Decoding, block0 is anywhere inside the workspace and interval0 is the index of the
 *   image's first segment row (the planner fills it; no decoding kernel reads it).  Encoding, the rows' block0 and interval0 run
 *   on from 0: every row starts where the row before it ends. */
typedef struct avsep_jpeg_image {
  int64_t pix_off;                          /* the image's first byte in `pixels`: H*W*3 bytes decoded; encoded, H*W*ncomp */
  int64_t block0;                           /* its first block in the coefficient workspace (64 int16 per block) */
  int64_t interval0;                        /* its first restart interval (1 per image without restarts), counted over the rows */
  int32_t H, W, ncomp;                      /* 1 <= H, W <= 16384; ncomp 1 | 3 */
  int32_t hs, vs;                           /* luma sampling: (1,1), (2,1) or (2,2); (1,1) with one component */
  int32_t mcux, mcuy;                       /* MCUs across and down: ceil(W / (8 hs)), ceil(H / (8 vs)) */
  int32_t quant[3], dc[3], ac[3];           /* word offsets in `tables`, per component */
  int32_t restart;                          /* MCUs per restart interval, 0 = none (one interval) */
  int32_t reserved;
} avsep_jpeg_image;                         /* 96 bytes.  pix_off, block0, interval0 >= 0 */
typedef struct avsep_jpeg_segment {
  int64_t begin, end;                       /* its bytes: bytes[begin .. end) */
  int32_t image;                            /* row of `images` */
  int32_t mcu0, mcus;                       /* first MCU and MCU count */
  int32_t reserved;
} avsep_jpeg_segment;
/* An image's blocks lie component after component, each [blocks down][blocks across], the luma plane mcuy*vs x mcux*hs blocks
 * and each chroma plane mcuy x mcux; a block is 64 coefficients in natural order.
 * avsep_jpeg_plan_check (host only, nothing is launched): every HOST row against the limits above and against the buffer
 *   sizes: pixel range inside pixel_bytes, blocks inside ws_blocks, tables inside table_words, segment bytes inside nbytes,
 *   segment MCUs inside the image and matching its restart interval.  AVSEP_ERR_ARG on the first row that fails.
 * avsep_jpeg_entropy: zeroes coef[0 .. 64 ws_blocks) and decodes one segment per lane into it.  A lane trusts neither the
 *   rows nor the stream: a read outside [begin, end) (status bit 1), no code within 16 bits (2), a DC size above 11 (4), a
 *   coefficient index past 63 (8), a marker inside the segment (16), a block outside the segment's blocks (32), a table outside
 *   `tables` (64), |coefficient x quantiser| above AVSEP_JPEG_MAX_COEF (128), a row outside its limits (256) or bytes left over
 *   after the last block (512) stops the lane and ORs the bit into status[image]; no check reads or writes out of range.
 *   status: int32 [n_images], zeroed by the caller.  Every segment gets a wavefront of its own: lanes of one wavefront that
 *   walk different streams pay for each other's branches (DESIGN §32 has the measurement).
 * avsep_jpeg_pixels: coefficients -> planes (uint8, 64 per block, the workspace's block order) -> pixels.  Images whose status
 *   is not 0 are skipped: their pixels are left as they were.  max_blocks, max_pixels: the most any one image has (the grids).
 * AVSEP_JPEG_MAX_COEF: below it no value of either inverse DCT pass can leave int32; equality with the int64
 *   recipe is claimed up to it, and with libjpeg-turbo for what an encoder makes of 8-bit pixels.
 * A null pointer, a count < 1, a size < 1, or coef or planes off a 16-byte boundary in avsep_jpeg_pixels (its lanes move whole
 * rows of a block) is AVSEP_ERR_ARG before any launch. */
#define AVSEP_JPEG_MAX_COEF 1173
int avsep_jpeg_plan_check(const avsep_jpeg_image* images, int32_t n_images, const avsep_jpeg_segment* segments, int32_t n_segments,
                          int64_t nbytes, int64_t table_words, int64_t pixel_bytes, int64_t ws_blocks);
int avsep_jpeg_entropy(const uint8_t* bytes, int64_t nbytes, const avsep_jpeg_image* images, int32_t n_images,
                       const avsep_jpeg_segment* segments, int32_t n_segments, const int32_t* tables, int64_t table_words,
                       int16_t* coef, int64_t ws_blocks, int32_t* status, avsep_stream_t stream);
int avsep_jpeg_pixels(const int16_t* coef, uint8_t* planes, int64_t ws_blocks, const avsep_jpeg_image* images, int32_t n_images,
                      int32_t max_blocks, int32_t max_pixels, const int32_t* tables, int64_t table_words, const int32_t* status,
                      uint8_t* pixels, int64_t pixel_bytes, avsep_stream_t stream);

/* ---- Progressive JPEG frames (SOF2; csrc/jpeg.hip, csrc/jpeg_parts.h: jp_decode_scan; avsep_amd/jpeg.py: probe_scans).
 * A progressive file fills the same coefficient workspace through several scans, and avsep_jpeg_pixels turns it into pixels as it
 * does for a baseline file.  Its image row is the baseline one (dc / ac point at any valid table, restart = 0); what differs per
 * scan travels in one row per (scan, restart interval): */
#define AVSEP_JPEG_MAX_SCANS 64             /* scans per file the host accepts (jpeg.MAX_SCANS) */
typedef struct avsep_jpeg_scan {
  int64_t begin, end;                       /* its bytes: bytes[begin .. end) */
  int32_t image;                            /* row of `images` */
  int32_t comps;                            /* mask of the frame's components in the scan: bit c = component c; 1 .. 7 */
  int32_t ss, se, ah, al;                   /* the band of zig-zag positions and the bit positions, as in the SOS header */
  int32_t table[3];                         /* per frame component in the scan: word offset of its DC (ss = 0) or AC Huffman table;
                                               not read by a DC refinement scan */
  int32_t unit0, units;                     /* first unit and unit count */
  int32_t level;                            /* scans of one level of an image touch disjoint (component, coefficient) sets */
  int32_t reserved[2];
} avsep_jpeg_scan;                          /* 72 bytes */
/* Units: with more than one component in the mask, the image's MCUs in raster order (each the blocks of the masked components
 * in frame order, padding blocks included); with one component c, that component's own blocks in raster order over its REAL
 * block grid, ceil(ceil(W h / hmax) / 8) across and ceil(ceil(H v / vmax) / 8) down, so padding blocks are never visited.
 * Rules of a row: 0 <= ss <= se <= 63; ss = 0 implies se = 0; ss > 0 implies one component; ah, al <= 13; ah = 0 or al = ah - 1.
 *   ss = 0, ah = 0  DC first: per block a size symbol (<= 11), receive-and-extend, a predictor per component (0 at a row's
 *                   start); stores predictor << al.
 *   ss = 0, ah > 0  DC refinement: one bit per block, ORs 1 << al into the stored value.  No table.
 *   ss > 0, ah = 0  AC first: run/size symbols over [ss, se], value << al stored; ZRL; size 0 with run r < 15 starts an
 *                   end-of-band run of (1 << r) + r further bits - 1 more blocks, carried across the row's blocks.
 *   ss > 0, ah > 0  AC refinement (T.81 G.1.2.3): a size of 0 or 1; non-zero coefficients passed take one correction bit each,
 *                   applied away from zero where bit al is clear; the new +-(1 << al) lands where the run of zeros ends.
 * avsep_jpeg_scan_check (host only): every HOST image row as avsep_jpeg_plan_check checks it, and every scan row: the rules
 *   above, bytes inside nbytes, image inside n_images, mask inside the image's components, units inside the units of its
 *   image and mask, every table it reads inside table_words, 0 <= level < AVSEP_JPEG_MAX_SCANS.  AVSEP_ERR_ARG on the first
 *   row that fails.
 * avsep_jpeg_scans: one lane (a wavefront of its own, as avsep_jpeg_entropy's) per row of `scans`, all of ONE level; the caller
 *   launches the levels of a chunk in rising order on one stream.  zero != 0 first zeroes coef[0 .. 64 ws_blocks) (a chunk
 *   without baseline segments, whose workspace avsep_jpeg_entropy has not zeroed).  A lane trusts neither rows nor stream and
 *   sets the status bits of avsep_jpeg_entropy, with: a band, mask, level (a row whose level is not `level`) or bit position
 *   outside the rules (256), a coefficient index past its band (8), a value that leaves int16 after its shift (128), a
 *   refinement symbol whose size is neither 0 nor 1 (1024), an end-of-band run longer than the row's remaining blocks (2048).
 *   A lane of level > 0 does nothing for an image whose status word is already set.
 * avsep_jpeg_coef_bound: after the last level, one lane per block of every image of the chunk (max_blocks: the most any
 *   one has): |coefficient x quantiser| above AVSEP_JPEG_MAX_COEF sets bit 128 (a progressive coefficient is only whole then;
 *   a baseline image's lanes have checked theirs already).  coef off a 16-byte boundary is AVSEP_ERR_ARG.
 * A null pointer, a count < 1 or a size < 1 is AVSEP_ERR_ARG before any launch. */
int avsep_jpeg_scan_check(const avsep_jpeg_image* images, int32_t n_images, const avsep_jpeg_scan* scans, int32_t n_scans,
                          int64_t nbytes, int64_t table_words, int64_t pixel_bytes, int64_t ws_blocks);
int avsep_jpeg_scans(const uint8_t* bytes, int64_t nbytes, const avsep_jpeg_image* images, int32_t n_images,
                     const avsep_jpeg_scan* scans, int32_t n_scans, int32_t level, int32_t zero, const int32_t* tables,
                     int64_t table_words, int16_t* coef, int64_t ws_blocks, int32_t* status, avsep_stream_t stream);
int avsep_jpeg_coef_bound(const int16_t* coef, int64_t ws_blocks, const avsep_jpeg_image* images, int32_t n_images,
                          int32_t max_blocks, const int32_t* tables, int64_t table_words, int32_t* status, avsep_stream_t stream);

/* ---- Baseline JPEG files written (csrc/jpeg_enc.hip, csrc/jpeg_parts.h; avsep_amd/jpeg.py: encode): uint8 [H][W] (grey, one
 * component) or [H][W][3] (RGB -> YCbCr, three components) -> the entropy-coded bytes of a file, byte for byte what libjpeg-turbo's
 * default encoder (Pillow's `save(f, "JPEG", quality=, subsampling=, restart_marker_blocks=)`) puts after its SOS segment, EOI
 * included.  The markers before it are the host's (jpeg.encode_header).  THE RULE:
 *   scope    luma sampling 1x1, 2x1 or 2x2, chroma 1x1; grey is 1x1.  quality 1 .. 100.  restart = MCUs per interval, 0 = none.
 *   header   SOI, APP0 JFIF 1.01 (density 1:1, no units), one DQT per table (luma; chroma with three components), SOF0, the
 *            DHTs (DC0, AC0 and with three components DC1, AC1: the Annex K tables), DRI only with restarts, SOS.
 *            Quantisers: scale = 5000 / q for q < 50, else 200 - 2q; entry = clamp((std * scale + 50) / 100, 1, 255), zig-zag.
 *   colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *            Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *   edges    a plane is replicated to the right to width_in_blocks * 8 * (hmax / h) columns and at the bottom to a multiple of
 *            vmax rows, THEN downsampled (2x1: (a + b + bias) >> 1, bias 0,1,0,1.. along the output columns; 2x2:
 *            (a + b + c + d + bias) >> 2, bias 1,2,1,2..), and only then replicated at the bottom to the MCU rows' height: a
 *            sample is the downsampled value of source coordinates clamped to the picture, and below the downsampled plane's
 *            ceil(H v / vmax) rows its last row again.  Blocks of
 *            an MCU beyond the component's width_in_blocks = ceil(ceil(W h / hmax) / 8) or height_in_blocks are DUMMY blocks: all
 *            AC zero, DC the quantised DC of the block before them in MCU order.
 *   DCT      libjpeg's islow forward DCT of sample - 128, 13-bit constants: rows first, scaled up by 4; then columns with
 *            rounded descales by 2 and 15; the result is 8 times the true DCT.
 *   quantise (|d| + ((8 q) >> 1)) / (8 q), the sign restored.
 *   entropy  one interleaved scan, MCUs in raster order, the luma blocks of an MCU in raster order inside it.  A DC difference
 *            (to the component's previous block in the interval, 0 at its start) is its category's code and the extra bits; AC
 *            values are run/size symbols with ZRL (0xF0) for runs above 15 and EOB (0x00) when zeros trail; a negative v of
 *            size s is written as v + 2^s - 1.  Every 0xFF byte is followed by 0x00.  The last byte of every restart interval
 *            and of the scan is padded with 1-bits; RSTn (n = 0 .. 7 in turn) stands between intervals, EOI at the end.
 * In DEVICE memory: pixels (the images back to back, anywhere in it), tables int32 [table_words] (quantisers: 64 words, NATURAL
 * order, 1 .. 255; Huffman codes: 256 words by symbol, (length << 16) | code, length <= 16, 0 = no such symbol), one avsep_jpeg_image row
 * per image (above), its pixels H*W bytes (one component) or H*W*3.
 * An image's blocks lie in SCAN order: MCU after MCU, in an MCU hs*vs luma blocks, then Cb, then Cr; a block is 64 int16 in
 * ZIG-ZAG order; dummy blocks are there like any other.  Four stages on the caller's stream, none of which reads anything back
 * (the caller copies the two totals it sizes the next buffer by):
 * avsep_jpeg_enc_plan_check (host only): every HOST row against the limits, block0 and interval0 running on from 0 to ws_blocks
 *   and n_intervals, pixel and table ranges inside their buffers.
 * avsep_jpeg_enc_coef: pixels -> coef int16 [64 ws_blocks], one lane per block (16-byte aligned).
 * avsep_jpeg_enc_count: bits int32 [ws_blocks] = every block's Huffman bits; pos int64 [ws_blocks + 1] = their running sum;
 *   ivl_bytes int32 [n_intervals] = an interval's bytes before stuffing, ivl_off int64 [n_intervals + 1] their running sum:
 *   ivl_off[n_intervals] is the size of the unstuffed stream.
 * avsep_jpeg_enc_pack: zeroes stream_buf[0 .. stream_bytes) and every block writes its bits at its place, the last block of an
 *   interval the 1-bit padding too; whole words are stored, the words a block shares with its neighbours are ORed in with an
 *   integer atomicOr (the order does not show in the result).  stream_bytes: ivl_off[n_intervals] rounded up to a multiple of 4
 *   (4-byte aligned).  Then groups int32 [ceil(stream_bytes / 64)] = the 0xFF bytes of every 64 bytes, ffpos int64 [groups + 1]
 *   their running sum, ff0 int64 [n_intervals] = the 0xFF bytes before an interval, ivl_out int32 [n_intervals] = an interval's
 *   bytes after stuffing plus its 2-byte marker, out_off int64 [n_intervals + 1] their running sum: out_off[n_intervals] is the
 *   size of all output.
 * avsep_jpeg_enc_stuff: out uint8 [out_bytes] = image after image the stuffed intervals with RSTn between them and EOI at the
 *   end; sizes int64 [2 n_images] = (first byte, byte count) of every image in `out`.
 * tiles int64 [tile_words]: scratch of the running sums, tile_words >= ceil(max(ws_blocks, n_intervals, groups) / 256).
 * Grids are bounded and strided, offsets 64 bit.  Rows in device memory are checked again by every lane that reads one and
 * every store is checked against its buffer's size: a wrong row gives wrong bytes, not an access outside a buffer.  A null
 * pointer, a count or size < 1, ws_blocks above 2^32, n_images above 2^24, a misaligned coef or stream_buf, or scratch too
 * small is AVSEP_ERR_ARG before any launch. */
int avsep_jpeg_enc_plan_check(const avsep_jpeg_image* images, int32_t n_images, int64_t pixel_bytes, int64_t table_words,
                              int64_t ws_blocks, int64_t n_intervals);
int avsep_jpeg_enc_coef(const uint8_t* pixels, int64_t pixel_bytes, const avsep_jpeg_image* images, int32_t n_images,
                        const int32_t* tables, int64_t table_words, int16_t* coef, int64_t ws_blocks, avsep_stream_t stream);
int avsep_jpeg_enc_count(const int16_t* coef, int64_t ws_blocks, const avsep_jpeg_image* images, int32_t n_images,
                         int64_t n_intervals, const int32_t* tables, int64_t table_words, int32_t* bits, int64_t* pos,
                         int32_t* ivl_bytes, int64_t* ivl_off, int64_t* tiles, int64_t tile_words, avsep_stream_t stream);
int avsep_jpeg_enc_pack(const int16_t* coef, int64_t ws_blocks, const avsep_jpeg_image* images, int32_t n_images,
                        int64_t n_intervals, const int32_t* tables, int64_t table_words, const int64_t* pos, const int64_t* ivl_off,
                        uint8_t* stream_buf, int64_t stream_bytes, int32_t* groups, int64_t* ffpos, int64_t* ff0, int32_t* ivl_out,
                        int64_t* out_off, int64_t* tiles, int64_t tile_words, avsep_stream_t stream);
int avsep_jpeg_enc_stuff(const uint8_t* stream_buf, int64_t stream_bytes, const avsep_jpeg_image* images, int32_t n_images,
                         int64_t n_intervals, const int64_t* ivl_off, const int64_t* ffpos, const int64_t* ff0,
                         const int64_t* out_off, uint8_t* out, int64_t out_bytes, int64_t* sizes, avsep_stream_t stream);

/* ---- PNG frames (csrc/png.hip, csrc/png_parts.h; avsep_amd/png.py): bit depth 8, colour type 0 (grey), 2 (RGB),
 * 3 (palette), 4 (grey + alpha) or 6 (RGBA), not interlaced -> uint8 RGB [H][W][3], the pixels of Pillow's
 * `Image.open(p).convert("RGB")`.  The host walks the chunks, checks their CRCs and hands over, in DEVICE memory,
 *   bytes  uint8 [nbytes]: the zlib streams (the IDAT payloads of a file joined) of the images back to back;
 *   tables uint8 [table_bytes]: the palettes, 3 bytes (R, G, B) per entry, anywhere in it, equal palettes shared;
 *   one row per image.  THE RULE:
 *   inflate   RFC 1950 / 1951, at least as strict as zlib 1.2.11's inflate(): the stream must fill exactly the image's
 *             H * (1 + W * channels) filtered bytes, end with the Adler-32 of those bytes and have nothing after it;
 *   unfilter  per scanline its filter byte 0 .. 4: None, Sub, Up, Average = floor((a + b) / 2) on the 9-bit sum, Paeth with
 *             p = a + b - c and the first of a, b, c nearest to p; a = the byte `channels` to the left, b the one above,
 *             c the one above a; zero outside the image; sums modulo 256;
 *   colour    grey -> (g, g, g); RGB as it is; grey + alpha and RGBA lose their alpha (no compositing); palette -> the
 *             entry's three bytes, an index at or past `entries` being an error. */
typedef struct avsep_png_image {
  int64_t pix_off;                          /* the image's first byte in `pixels`: H*W*3 bytes */
  int64_t begin, end;                       /* its zlib stream: bytes[begin .. end) */
  int64_t ws_off;                           /* its filtered scanlines in the workspace: H * (1 + W * channels) bytes */
  int32_t H, W;                             /* 1 <= H, W <= 16384, H * W <= 2^26 */
  int32_t colour, channels;                 /* colour type 0 | 2 | 3 | 4 | 6 and its bytes per pixel 1 | 3 | 1 | 2 | 4 */
  int32_t palette, entries;                 /* colour type 3: byte offset in `tables` and entry count 1 .. 256; else 0, 0 */
  int32_t reserved[2];
} avsep_png_image;                          /* 64 bytes.  pix_off, begin, ws_off >= 0; end >= begin */
/* avsep_png_plan_check (host only, nothing is launched): every HOST row against the limits above and against the buffer
 *   sizes: stream inside nbytes, scanlines inside ws_bytes, pixels inside pixel_bytes, palette inside table_bytes, channels
 *   matching the colour type.  AVSEP_ERR_ARG on the first row that fails.
 * avsep_png_inflate: one lane (a wavefront of its own: one stream is serial, and lanes that walk different streams pay for
 *   each other's branches) per image inflates its stream straight into its scanlines in `ws`, which are also the
 *   LZ77 window; the block's Huffman tables are built by the lane in LDS.  A lane trusts neither its row nor the stream.  Each
 *   of these stops it and ORs the bit into status[image]: a read outside the stream (1); a zlib header with CM != 8,
 *   CINFO > 7, a failing FCHECK or FDICT (2); block type 3 (4); a stored block whose LEN is not the complement of NLEN (8);
 *   HLIT > 286 or HDIST > 30 (16); a length repeat with no previous length or past HLIT + HDIST (32); an over-subscribed code
 *   set (64); an incomplete one, but for zlib's exception, a literal/length or distance set whose longest code is 1 bit
 *   (128); no end-of-block code (256); no code within 15 bits or a code the set leaves unused (512); literal/length symbol
 *   286 / 287 or distance symbol 30 / 31 (1024); a distance beyond the bytes written (2048); output past the image's
 *   scanlines (4096); a final block that ends short of them (8192); bytes left after the Adler-32 (16384); an Adler-32 that
 *   does not match (32768); the loop bound, output bytes + stream bits, exceeded (65536); a row outside its limits or its
 *   buffers (524288).  No check reads or writes out of range.  status: int32 [n_images], zeroed by the caller.
 * avsep_png_pixels: the scanlines of every image whose status is 0 are unfiltered in place (one wavefront per image, lane k
 *   = row k of a group of 64 rows, one pixel behind lane k - 1; a filter byte above 4 sets bit 131072) and then turned into
 *   pixels, one lane per pixel (max_pixels: the most any one image has; a palette index at or past `entries` sets bit 262144).
 *   Images whose status is not 0 are skipped: their pixels are left as they were.  stages: 3 = both; 1 = unfilter only, 2 =
 *   colour only (for a caller that times them apart; colour alone takes scanlines that are already unfiltered).
 * A null pointer, a count < 1 (or n_images above 65535), a size < 1 or stages outside 1 .. 3 is AVSEP_ERR_ARG before any launch. */
int avsep_png_plan_check(const avsep_png_image* images, int32_t n_images, int64_t nbytes, int64_t table_bytes, int64_t pixel_bytes,
                         int64_t ws_bytes);
int avsep_png_inflate(const uint8_t* bytes, int64_t nbytes, const avsep_png_image* images, int32_t n_images, uint8_t* ws,
                      int64_t ws_bytes, int32_t* status, avsep_stream_t stream);
int avsep_png_pixels(uint8_t* ws, int64_t ws_bytes, const avsep_png_image* images, int32_t n_images, int32_t max_pixels,
                     const uint8_t* tables, int64_t table_bytes, int32_t* status, uint8_t* pixels, int64_t pixel_bytes,
                     int32_t stages, avsep_stream_t stream);

/* ---------------------------------------------------------------------------
 * AVSEP_FMT_B16 images (bf16, [N][C/16][H][W][16]; csrc/b16.hip): what travels between the bf16 convolution kernels.
 * HW = H*W positions; every entry point is one HBM pass with 16-byte accesses.  Statistics buffers are pre-zeroed doubles
 * that are accumulated into, exactly as for the fp32 NCHW entry points of the same names below.
 * ------------------------------------------------------------------------- */
int avsep_f32_to_b16(const float* x, int32_t N, int32_t C, int32_t HW, void* out, avsep_stream_t stream);
int avsep_b16_to_f32(const void* x, int32_t N, int32_t C, int32_t HW, float* out, avsep_stream_t stream);
/* z = act(scale*y + shift [+ res_scale*residual + res_shift | + residual])   (BasicBlock tail; act NONE/RELU/LRELU02) */
int avsep_b16_affine_act(const void* y, const float* scale, const float* shift, const void* residual,
                         const float* res_scale, const float* res_shift, int32_t act, int32_t N, int32_t C, int32_t HW,
                         void* z, avsep_stream_t stream);
/* out = act'(scale*y + shift [+ residual term]) * (dz [+ dz2]) [+ add]  (out may alias dz; NULL = statistics only);
 * bstats[2*C] += (sum out, sum out * (y - mean) * invstd) */
int avsep_b16_affine_act_bwd(const void* dz, const void* dz2, const void* y, const float* scale, const float* shift,
                             const void* residual, const float* res_scale, const float* res_shift, const void* add,
                             const float* mean, const float* invstd, int32_t act, int32_t N, int32_t C, int32_t HW,
                             void* out, double* bstats, avsep_stream_t stream);
/* out = p*dz + q*y + r with pqr[3*C] from avsep_bn_bwd_coeffs (out may alias dz) */
int avsep_b16_bn_bwd_apply(const void* dz, const void* y, const float* pqr, int32_t N, int32_t C, int32_t HW, void* out,
                           avsep_stream_t stream);
/* Grid image of a batch of small maps — the 2x2 ... 8x8 maps of the deep U-Net levels, models/audio_net.py:64-69,75-76 —
 * (B16 out [1][C/16][HG][WG][16]): image n of x (fp32 NCHW or B16, `xfmt`) goes to rows
 * (n / GX) * PY .., columns (n % GX) * PX .. after the folded affine (scale / shift per channel, or NULL) and activation `act`
 * (AVSEP_ACT_NONE / RELU / LRELU02); every other position is zero.  HG = rows (a multiple of PY), WG = GX * PX.  With pitch
 * H + 1 (3x3 / pad 1; X and dY) or H + 2 for X and H/2 + 1 for dY (4x4 / stride 2 / pad 1) the separators are every image's zero
 * padding, and avsep_conv2d_wgrad over the two grid images (N = 1) returns the weight gradient of the batch. */
int avsep_b16_grid_pack(const void* x, int32_t xfmt, int32_t N, int32_t C, int32_t H, int32_t W, int32_t GX, int32_t PY, int32_t PX,
                        int32_t HG, int32_t WG, const float* scale, const float* shift, int32_t act, void* out, avsep_stream_t stream);
/* The inverse for a convolution RESULT computed over grid images: out (B16 image or fp32 NCHW, `ofmt`) [N][C][H][W] = the real
 * positions of the fp32 grid image [1][C][HG][WG] (image n at rows (n / GX) * PY, columns (n % GX) * PX); stats (or NULL) +=
 * (sum y, sum y^2) per channel of those fp32 values, as avsep_conv2d_fwd accumulates them. */
int avsep_grid_unpack(const float* grid, int32_t N, int32_t C, int32_t H, int32_t W, int32_t GX, int32_t PY, int32_t PX, int32_t HG,
                      int32_t WG, void* out, int32_t ofmt, double* stats, avsep_stream_t stream);
/* out (B16) = p*dz + q*y + r with dz, y fp32 NCHW: avsep_bn_bwd_apply + avsep_f32_to_b16 in one pass (the fp32 -> B16 boundary
 * below the fused decoder head) */
int avsep_bn_bwd_apply_to_b16(const float* dz, const float* y, const float* pqr, int32_t N, int32_t C, int32_t HW, void* out,
                              avsep_stream_t stream);
/* out [N][(C0+C1)/16][2H][2W][16] = bilinear x2 (align_corners) of relu(affine(cat(x0, x1)))   (audio_net.py:66-69,122) */
int avsep_b16_relu_up2x_fwd(const void* x0, const void* x1, const float* sc0, const float* sh0, const float* sc1,
                            const float* sh1, int32_t N, int32_t C0, int32_t C1, int32_t H, int32_t W, void* out,
                            avsep_stream_t stream);
/* its adjoint: g0 / g1 = gradient wrt the pre-ReLU affine values of the two low-res sources (acc0: add into g0);
 * bstats1[2*C1] += BatchNorm-backward sums of source 1 (needs mean1 / invstd1) */
int avsep_b16_relu_up2x_bwd(const void* x0, const void* x1, const float* sc0, const float* sh0, const float* sc1,
                            const float* sh1, int32_t N, int32_t C0, int32_t C1, int32_t H, int32_t W, const void* dout,
                            void* g0, void* g1, const float* mean1, const float* invstd1, double* bstats1, int32_t acc0,
                            avsep_stream_t stream);
/* z = MaxPool2d(3,2,1)(act(scale*y + shift)); idx: one byte per element (winning tap kh*3+kw), blocked like z */
int avsep_b16_maxpool3x3s2_fwd(const void* y, const float* scale, const float* shift, int32_t act, int32_t N, int32_t C,
                               int32_t H, int32_t W, void* z, void* idx, avsep_stream_t stream);
/* fused stem-tail backward (avsep_maxpool_bn_relu_bwd_stats / _apply on B16 images): dy == NULL -> pass 1 (bstats),
 * else pass 2 (dy = p*dz + q*y + r; dy_f32 != 0: dy is written as fp32 NCHW for the fp32 stem weight gradient);
 * g2 (may be NULL) is added to g on the fly */
int avsep_b16_maxpool_bn_relu_bwd(const void* g, const void* g2, const void* idx, const void* y, const float* scale,
                                  const float* shift, const float* mean, const float* invstd, const float* pqr,
                                  int32_t N, int32_t C, int32_t H, int32_t W, double* bstats, void* dy, int32_t dy_f32,
                                  avsep_stream_t stream);
/* avsep_space_to_depth2 written as a one-block B16 image [N][1][H/2+3][W/2+3][16] (4*C <= 16) */
int avsep_b16_space_to_depth2(const float* x, int32_t N, int32_t C, int32_t H, int32_t W, void* xs, avsep_stream_t stream);

/* ---- BSS-eval (csrc/bss_windows.hip; avsep_amd/bss_eval.py, avsep_amd/score.py): SDR / SIR / SAR of 6 s mono training batches (eval
 * path; replaces asteroid -> mir_eval.separation.bss_eval_sources, main.py:260-266) and the image form of the same decomposition
 * (Vincent et al. 2006, bss_decomp_mtifilt) for whole recordings: SDR / ISR / SIR / SAR over all channels of a source, in short
 * windows.  A batch [B][S][L] is the rows [S][B*L], C = 1, sample b the segment [b*L, b*L + L).
 * float64 throughout.  refs, ests: [P][L], row p = source * C + channel, P = S * C <= 8.  A segment is the samples
 * [seg_starts[s], seg_starts[s] + n) of every row, treated as zero outside itself; seg_starts [nseg] (int64, device memory), all
 * segments of a call have the same length n; flen <= 512.
 * avsep_bss_seg_corr:  R [nseg][P][P][2*flen-1]: R[..][tau + flen - 1] = sum_t r_p[t + tau] * r_q[t],
 *                      D [nseg][P(estimate e)][P(reference p)][flen]: D[..][k] = sum_t r_p[t - k] * e_e[t]; the rows are read in
 *                      place, no atomics: per-block partial sums in `workspace` are added in ascending order, so a segment's result
 *                      is the same bits in every call that holds it.
 * avsep_bss_solve_groups: the least-squares filters of the row groups g*G .. g*G+G-1 (G divides P; G = C: a source on its own
 *                      channels, G = P: all sources), G*flen <= 2048 unknowns and G right-hand sides (the estimate rows of the
 *                      group) per (segment, group), by LU with partial pivoting (numpy.linalg.solve's algorithm), one workgroup
 *                      per system: C [nseg * P/G][G*flen][G]; info [nseg * P/G] = 0, or k + 1 when pivot k is exactly zero (a silent
 *                      row): C is zero there and the caller solves that system by minimum-norm least squares, as mir_eval does.
 * avsep_bss_window_energies: range i = samples [range_off[i], range_off[i] + rlen) of segment range_seg[i], relative to the
 *                      segment's start (range_seg int32 [nrange], range_off int64 [nrange], device memory; the projections live on
 *                      [0, n + flen - 1)).  With C_all [nseg][P*flen][P] (G = P) and C_own [nseg * S][C*flen][C] (G = C) from
 *                      avsep_bss_solve_groups, p_all / p_own the two FIR projections of row q, s = r_q, e = e_q:
 *                      sums [nrange][S][8] = sum over the range and the source's channels of
 *                      s^2, (e-s)^2, (p_own-s)^2, p_own^2, (p_all-p_own)^2, p_all^2, (e-p_all)^2, (e-p_own)^2 (the last is the
 *                      distortion of mir_eval's SDR).  No waveform is written; block partials in `workspace`, then an ordered sum. */
size_t avsep_bss_seg_corr_workspace_bytes(int32_t nseg, int32_t P, int64_t n, int32_t flen);
int avsep_bss_seg_corr(const double* refs, const double* ests, int32_t P, int64_t L, int32_t flen, const int64_t* seg_starts,
                       int32_t nseg, int64_t n, double* workspace, size_t workspace_bytes, double* R, double* D, avsep_stream_t stream);
size_t avsep_bss_solve_groups_workspace_bytes(int32_t nseg, int32_t P, int32_t G, int32_t flen);
int avsep_bss_solve_groups(const double* R, const double* D, int32_t nseg, int32_t P, int32_t G, int32_t flen, double* workspace,
                           size_t workspace_bytes, double* C, int32_t* info, avsep_stream_t stream);
size_t avsep_bss_window_energies_workspace_bytes(int32_t nrange, int32_t P, int64_t rlen);
int avsep_bss_window_energies(const double* refs, const double* ests, int32_t P, int32_t C, int64_t L, int32_t flen,
                              const int64_t* seg_starts, int32_t nseg, int64_t n, const double* C_all, const double* C_own,
                              const int32_t* range_seg, const int64_t* range_off, int32_t nrange, int64_t rlen, double* workspace,
                              size_t workspace_bytes, double* sums, avsep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AVSEP_H */
