// stft.hip's host functions that misi.hip calls as well: the two DFT GEMMs of the transform pair with what stages their
// operands.  Both files include this header.
#pragma once
#include "common.h"

// whether (R rows of L samples, n_fft, hop) takes the hop-transposed 1x4-conv form
bool stft_fast_path(int R, int L, int n_fft, int hop);
// forward basis -> the operand of that form, [hop * 4][roundup(2 * bins, 128)]
int stft_repack_basis(const float* basis, int n_fft, int hop, float* wp, hipStream_t st);
// Pad (reflect / zero) and multiply with the forward basis.  Fast path: `basis` is the repacked one, stage holds
// [hop][R][frames + 3] and spec comes out co-major, [2*bins][R][frames].  Otherwise `basis` is the plan's, stage holds
// [R][L + n_fft] and spec is [R][2*bins][frames].  frames = 1 + L / hop.
int stft_pad_gemm(const float* wav, int R, int L, int n_fft, int hop, int reflect, const float* basis, float* stage, float* spec,
                  hipStream_t st);
// td [R][n_fft][frames] = inverse basis x spec [R][2*bins][frames]
int istft_gemm(const float* spec, int R, int n_fft, int frames, const float* inv_basis, float* td, hipStream_t st);
