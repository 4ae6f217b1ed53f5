// Every host function of the conv code that crosses a .hip boundary, grouped by the file that defines it.  Both the
// defining file and every caller include this header; no .hip file carries a prototype of another file's function.
//
// A kernel family `p` serves conv calls through slots of ONE signature each (the typedefs below); a callee ignores the
// arguments it has no use for.  conv.hip's route tables take a family's slots by prefix, so a family that joins needs its
// block here and one table entry there.  `mode` is 0 forward, 1 data gradient, 2 weight gradient throughout.
#pragma once
#include "common.h"

typedef bool conv_applicable_fn(const avsep_conv_desc* d, int mode);
typedef size_t conv_packed_floats_fn(const avsep_conv_desc* d, int mode);
typedef int conv_pack_fn(const avsep_conv_desc* d, const float* w, float* packed, int mode, hipStream_t st);
typedef size_t conv_workspace_fn(const avsep_conv_desc* d, int mode);   // bytes
typedef void conv_variant_fn(const avsep_conv_desc* d, int mode, char* buf, size_t cap);
typedef int conv_fwd_fn(const avsep_conv_desc* d, const float* wp, const float* bias, float* y, double* stats, void* ws,
                        size_t ws_bytes, hipStream_t st);
typedef int conv_dgrad_fn(const avsep_conv_desc* d, const float* wp, const float* dy, float* dx, const avsep_act_bwd* e,
                          void* ws, size_t ws_bytes, hipStream_t st);   // e: only the family avsep_conv2d_dgrad_act fuses reads it
typedef int conv_wgrad_fn(const avsep_conv_desc* d, const float* dy, float* dw, float* dbias, float* ws, hipStream_t st);

// Leading dimension of the im2col family's packed weight image ([k][Cout] forward, [k][Cin] data gradient): the image the
// few-output-channel forward kernels (smallco, head) read as well.
static inline int igemm_packed_ld(const avsep_conv_desc* d, int mode) { return roundup(mode == 0 ? d->Cout : d->Cin, 128); }

// conv.hip: split-K combines
int splitk_combine(const float* ws, long long slab, int S, const avsep_conv_desc* d, const float* bias, float* y, double* stats,
                   hipStream_t st);
int reduce_slabs(const float* ws, float* out, long long n, int S, hipStream_t st);
int reduce_slabs_strided(const float* ws, float* out, long long n, int S, long long stride, hipStream_t st);

// direct.hip: VALU kernels for convolutions with <= 4 output channels (3x3, stride 1) or <= 4 input channels
conv_applicable_fn smallco_applicable;  conv_workspace_fn smallco_workspace_bytes;  conv_fwd_fn smallco_fwd;  conv_wgrad_fn smallco_wgrad;
conv_applicable_fn smallci_applicable;  conv_packed_floats_fn smallci_packed_floats;  conv_pack_fn smallci_pack;  conv_dgrad_fn smallci_dgrad;

// head_gemm.hip: the fused decoder head over the virtual up2x(relu(affine(cat))) input
conv_applicable_fn head_applicable;  conv_workspace_fn head_workspace_bytes;  conv_fwd_fn head_fwd;  conv_wgrad_fn head_wgrad;
size_t head_dgrad_workspace_floats(const avsep_conv_desc* d);
int head_dgrad(const avsep_conv_desc* d, const float* w, const float* dy, float* g0, float* g1, const float* mean1,
               const float* invstd1, double* bstats1, int acc0, float* ws, hipStream_t st);

// conv_bf16.hip: bf16-operand halo-patch kernels (desc.prec == AVSEP_PREC_BF16)
conv_applicable_fn bf_applicable;  conv_packed_floats_fn bf_packed_floats;  conv_pack_fn bf_pack;  conv_workspace_fn bf_workspace_bytes;
conv_fwd_fn bf_fwd;  conv_dgrad_fn bf_dgrad;  conv_variant_fn bf_variant;
bool bf_out_b16(const avsep_conv_desc* d, int mode);

// conv_wino4.hip: Winograd F(4x4, 3x3) for the maps that tile by 4 (asked before F(2x2, 3x3))
conv_applicable_fn w4_applicable;  conv_packed_floats_fn w4_packed_floats;  conv_pack_fn w4_pack;
conv_fwd_fn w4_fwd;  conv_dgrad_fn w4_dgrad;  conv_variant_fn w4_variant;

// conv_wino.hip: Winograd F(2x2, 3x3) form of the 3x3 / stride 1 / 'same' convs (forward and dgrad), fp32
conv_applicable_fn wn_applicable;  conv_packed_floats_fn wn_packed_floats;  conv_pack_fn wn_pack;  conv_fwd_fn wn_fwd;  conv_dgrad_fn wn_dgrad;

// conv3x3.hip: LDS-halo-patch kernel for 3x3 / stride 1 / pad 1 (c3), 4x4 / stride 2 (c4) and their weight gradient (w3)
conv_applicable_fn c3_applicable;  conv_packed_floats_fn c3_packed_floats;  conv_pack_fn c3_pack;
conv_fwd_fn c3_fwd;  conv_dgrad_fn c3_dgrad;  conv_variant_fn c3_variant;
conv_applicable_fn c4_applicable;  conv_packed_floats_fn c4_packed_floats;  conv_pack_fn c4_pack;
conv_fwd_fn c4_fwd;  conv_dgrad_fn c4_dgrad;  conv_variant_fn c4_variant;
conv_applicable_fn w3_applicable;  conv_workspace_fn w3_workspace_bytes;  conv_wgrad_fn w3_wgrad;
void c3_variant_text(int M, int Ho, int Wo, long long planN, bool flat, bool quantise, char* buf, size_t cap);
int w3_reduce(const float* ws, float* dw, long long P, int splits, hipStream_t st);
int c1x4_stft_fwd(const float* xt, const float* wp, float* out, int R, int NH, int hop, int cout, int frames, hipStream_t st);

// conv_flat.hip: the flat (whole small map per tile) form of the halo-patch launch
struct C3Args;
int c3_flat_width(int H, int W, int dil);
int c3_flat_launch(C3Args& a, int dil, hipStream_t st);

// conv_misc.hip: 3x3/s2 and 1x1 convolutions of the visual trunk on the halo-patch kernel (fp32)
conv_applicable_fn cm_applicable;  conv_packed_floats_fn cm_packed_floats;  conv_pack_fn cm_pack;
conv_fwd_fn cm_fwd;  conv_dgrad_fn cm_dgrad;  conv_variant_fn cm_variant;

// wgrad_b16.hip: bf16 weight gradient over B16 images; its workspace ends with 2 * Cout doubles for b16_channel_sum (b16.hip)
conv_applicable_fn wbn_applicable;  conv_workspace_fn wbn_workspace_bytes;  conv_wgrad_fn wbn_wgrad;  conv_variant_fn wbn_variant;
int b16_channel_sum(const void* x, int N, int C, int HW, double* acc, float* out, hipStream_t st);

// wgrad_wino4.hip: Winograd F(4x4, 3x3) weight gradient (asked before the F(2x2) form)
conv_applicable_fn x4_applicable;  conv_workspace_fn x4_workspace_bytes;  conv_wgrad_fn x4_wgrad;  conv_variant_fn x4_variant;

// wgrad_wino.hip: Winograd F(2x2, 3x3) weight gradient (ww) and the 4x4 / stride 2 direct form on the same skeleton (w4d)
conv_applicable_fn ww_applicable;  conv_workspace_fn ww_workspace_bytes;  conv_wgrad_fn ww_wgrad;
conv_applicable_fn w4d_applicable;  conv_workspace_fn w4d_workspace_bytes;  conv_wgrad_fn w4d_wgrad;

// wgrad_smallci.hip: weight gradient of convs with few input channels
conv_applicable_fn scw_applicable;  conv_workspace_fn scw_workspace_bytes;  conv_wgrad_fn scw_wgrad;
