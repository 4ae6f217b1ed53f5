// Implicit-GEMM convolution (forward / data-gradient / weight-gradient) on the exact-f32
// MFMA (v_mfma_f32_32x32x2_f32) for gfx950.  NCHW fp32.  See include/avsep.h.
//
// GEMM view (D[M][N], N on the lanes so global stores are coalesced):
//   fwd   : D[co][pix]   = sum_k  Wp[k][co]      * X(k, pix)        k = (ci,kh,kw)
//   dgrad : D[ci][pixin] = sum_k' Wd[k'][ci]     * dY(k', pixin)    k' = (tap,co), one launch
//           slice (blockIdx.y) per input-pixel parity class so strided convs waste no MFMA work
//   wgrad : D[co][k]     = sum_pix dY[co][pix]   * X(k, pix)        split over pixel chunks
// X(k,pix) is the *virtual* conv input: two-source channel concat, per-channel affine (folded
// BatchNorm), activation and optional bilinear x2 upsample are applied while gathering.
// Both operands are staged global -> registers -> LDS (K-major, double buffered, one barrier
// per K-tile); each wave owns a (BM/WM)x(BN/WN) block of 32x32 MFMA tiles.
#include "common.h"
#include "conv_families.h"
#include <stdio.h>
#include <string.h>
#include <type_traits>

enum { M_FWD = 0, M_DGRAD = 1, M_WGRAD = 2 };

struct CArgs {
  int N, Cin, H, W, Cout, Ho, Wo, KH, KW, stride, pad, dil;
  int C0, C1, act0, act1, up2x;
  int Hs, Ws;  // source spatial size (H/2, W/2 when up2x)
  float rh, rw;
  const float *x0, *x1, *sc0, *sh0, *sc1, *sh1;
  const float* wp;
  int wp_ld;
  const float* dy;
  float* out;
  const float* bias;
  double* stats;
  int M, Ncols, K;
  int gridM;
  int chunk, P;  // wgrad: pixels per split, total pixels
  int kts;       // fwd/dgrad split-K: K-tiles per split (0 = no split)
  long long slab;  // fwd/dgrad split-K: elements of one partial output slab
  int lstride;   // log2(stride) (dgrad)
};

__device__ __forceinline__ float load_src(const CArgs& a, long long nb0, long long nb1, int ci, int off) {
  float v;
  if (ci < a.C0) {
    v = a.x0[nb0 + (long long)ci * (a.Hs * a.Ws) + off];
    if (a.sc0) v = fmaf(v, a.sc0[ci], a.sh0[ci]);
    v = act_apply(v, a.act0);
  } else {
    int c1 = ci - a.C0;
    v = a.x1[nb1 + (long long)c1 * (a.Hs * a.Ws) + off];
    if (a.sc1) v = fmaf(v, a.sc1[c1], a.sh1[c1]);
    v = act_apply(v, a.act1);
  }
  return v;
}

// value of the virtual input at (ci, hi, wi), 0<=hi<H, 0<=wi<W
__device__ __forceinline__ float load_virtual(const CArgs& a, long long nb0, long long nb1, int ci, int hi,
                                              int wi) {
  if (!a.up2x) return load_src(a, nb0, nb1, ci, hi * a.Ws + wi);
  // nn.Upsample(scale_factor=2, bilinear, align_corners=True): src = dst*(in-1)/(out-1)
  float fh = a.rh * (float)hi, fw = a.rw * (float)wi;
  int h0 = (int)fh, w0 = (int)fw;
  int h1 = h0 + (h0 < a.Hs - 1), w1 = w0 + (w0 < a.Ws - 1);
  float lh = fh - (float)h0, lw = fw - (float)w0;
  float v00 = load_src(a, nb0, nb1, ci, h0 * a.Ws + w0), v01 = load_src(a, nb0, nb1, ci, h0 * a.Ws + w1);
  float v10 = load_src(a, nb0, nb1, ci, h1 * a.Ws + w0), v11 = load_src(a, nb0, nb1, ci, h1 * a.Ws + w1);
  return (1.f - lh) * ((1.f - lw) * v00 + lw * v01) + lh * ((1.f - lw) * v10 + lw * v11);
}

// UP2X: the fused bilinear x2 gather is compiled in only where it is used (as a run-time flag it put four corner loads,
// their interpolation and a scalar branch per element into every instantiation's K loop).
// BUF (fwd, dgrad): the gathered operand comes through raw buffer loads with 32-bit byte offsets (igemm_buf32 decides on the
// host).  What depends on the column alone is computed once per workgroup: a bit mask of the taps that fall outside the image
// and the lane's byte offset.  What depends on the row k alone -- its byte offset (channel + tap), its tap index and its folded
// BatchNorm pair -- is decoded by ONE thread per row into an LDS table two K-tiles ahead, instead of by every wave on its
// scalar unit for every element.  Per element the loader then pays one LDS read, one add, one bit-field extract and one or: an
// element outside the image (or past K) gets the offset 0xffffffff, which is out of the resource's range and loads as 0.
// The weight gradient's form of it is described at its loader state below.  BUF = false is the 64-bit global_load loader, for
// sources too large for 32-bit offsets and for the UP2X gather.
template <int MODE, int BM, int BN, int BK, int WM, int WN, bool UP2X = false, bool BUF = false>
__global__ __launch_bounds__(256) void igemm_kernel(CArgs a) {
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int LDA = BM + ((MODE == M_WGRAD) ? 1 : 4);
  constexpr int LDB = BN + ((MODE == M_WGRAD) ? 1 : 0);
  __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];
  __shared__ float Bs[2][BK][LDB];
  __shared__ int s_tab[(MODE == M_WGRAD) ? BN : 24];
  __shared__ float s_sc[(MODE == M_WGRAD) ? BN : 1], s_sh[(MODE == M_WGRAD) ? BN : 1];
  __shared__ int s_code[(MODE == M_WGRAD) ? BN : 1];
  // BUF: rows of the K-tiles in flight.  fwd {byte offset, tap, scale, shift}, dgrad {byte offset, tap, packed weight row, -}.
  // Slot kt & 1 is read by issue(kt) / finish(kt), both in iteration kt - 1, and rewritten for tile kt + 2 at the end of
  // iteration kt: the K loop's one barrier (end of iteration kt - 1) lies between the last read and the write, and the barrier
  // at the end of iteration kt between the write and the reads of issue(kt + 2).
  constexpr bool DEC = BUF && MODE != M_WGRAD;
  __shared__ __attribute__((aligned(16))) unsigned s_dec[DEC ? 2 : 1][DEC ? BK : 1][4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int HoWo = a.Ho * a.Wo, KHW = a.KH * a.KW, HW = a.H * a.W;
  const long long srcHW = (long long)a.Hs * a.Ws;

  int M = a.M, Ncols = a.Ncols, K = a.K;
  int ph = 0, pw = 0, Hc = 0, Wc = 0, ntw = 1;
  if (MODE == M_DGRAD) {
    const int s = a.stride;
    ph = blockIdx.y / s;
    pw = blockIdx.y % s;
    Hc = (a.H > ph) ? (a.H - ph + s - 1) / s : 0;
    Wc = (a.W > pw) ? (a.W - pw + s - 1) / s : 0;
    if (tid == 0) {
      int nh = 0, nw = 0;
      for (int kh = 0; kh < a.KH; ++kh) {
        int t = ph + a.pad - kh * a.dil;
        if (((t % s) + s) % s == 0) s_tab[2 + nh++] = kh;
      }
      for (int kw = 0; kw < a.KW; ++kw) {
        int t = pw + a.pad - kw * a.dil;
        if (((t % s) + s) % s == 0) s_tab[12 + nw++] = kw;
      }
      s_tab[0] = nh;
      s_tab[1] = nw;
    }
    __syncthreads();
    ntw = s_tab[1];
    Ncols = a.N * Hc * Wc;
    K = s_tab[0] * ntw * a.Cout;
  }
  const int t_lin = xcd_remap(blockIdx.x, gridDim.x);
  const int n0 = (t_lin / a.gridM) * BN, m0 = (t_lin % a.gridM) * BM;
  if (MODE == M_DGRAD && n0 >= Ncols) return;  // block-uniform

  int p_begin = 0, p_end = 0, nK;
  if (MODE == M_WGRAD) {
    p_begin = blockIdx.y * a.chunk;
    p_end = min(a.P, p_begin + a.chunk);
    nK = (p_end - p_begin + BK - 1) / BK;
    // per-column (k) decode table: ci | dh<<16 | dw<<24
    for (int c = tid; c < BN; c += 256) {
      int k = n0 + c, v = -1, code = 0;
      float sc = 1.f, sh = 0.f;
      if (k < Ncols) {
        int ci = k / KHW, r = k % KHW;
        v = ci | ((r / a.KW) * a.dil << 16) | ((r % a.KW) * a.dil << 24);
        bool first = ci < a.C0;
        int cs = first ? ci : ci - a.C0;
        const float* sp = first ? a.sc0 : a.sc1;
        const float* hp = first ? a.sh0 : a.sh1;
        if (sp) { sc = sp[cs]; sh = hp[cs]; code = 1; }
        code |= (first ? a.act0 : a.act1) << 1;
        if constexpr (BUF) code = __float_as_int(act_slope(first ? a.act0 : a.act1));   // BUF: the slope itself (sc = 1, sh = 0: no flag)
      }
      s_tab[c] = v;
      s_sc[c] = sc;
      s_sh[c] = sh;
      s_code[c] = code;
    }
    __syncthreads();
  } else {
    nK = (K + BK - 1) / BK;
  }
  // split-K (fwd: blockIdx.y, dgrad: blockIdx.z): this block reduces K-tiles [kt0, nK) of its slice
  int kt0 = 0, ksplit = 0;
  if (MODE != M_WGRAD && a.kts > 0) {
    ksplit = (MODE == M_FWD) ? blockIdx.y : blockIdx.z;
    kt0 = ksplit * a.kts;
    nK = min(nK, kt0 + a.kts);
  }

  // ---------------- per-thread loader state ----------------
  // fwd/dgrad: thread owns one column (bcol) and BROWS consecutive k rows.
  // Loads are split in two phases so that their latency hides behind the MFMA loop:
  //   issue(kt+1): address math + UNCONDITIONAL global loads (clamped addresses) into raw registers
  //   finish():    affine + activation + zero-masking, then the LDS stores, after the MFMA loop.
  constexpr int BGROUPS = 256 / BN, BROWS = (MODE == M_WGRAD) ? 1 : BK / BGROUPS;
  constexpr int A4 = BM / 4, AV = (MODE == M_WGRAD) ? 1 : (BK * A4) / 256;
  constexpr int PG = 256 / BK, AE = BM / PG, BE = BN / PG;  // wgrad
  constexpr int NBR = (MODE == M_WGRAD) ? BE : BROWS;
  constexpr int NSC = (MODE == M_FWD) ? BROWS : 1;
  // BN >= 64, so all lanes of a wave own the same k rows: keep everything k-dependent on the scalar unit
  const int bcol = tid % BN, brow0 = __builtin_amdgcn_readfirstlane((tid / BN) * BROWS);
  bool cvalid = false;
  long long nb0 = 0, nb1 = 0, nbdy = 0;
  int hi0 = 0, wi0 = 0;
  if (MODE == M_FWD) {
    int j = n0 + bcol;
    cvalid = j < Ncols;
    int jj = cvalid ? j : 0;
    int n = jj / HoWo, hw = jj % HoWo;
    hi0 = (hw / a.Wo) * a.stride - a.pad;
    wi0 = (hw % a.Wo) * a.stride - a.pad;
    nb0 = (long long)n * a.C0 * srcHW;
    nb1 = (long long)n * a.C1 * srcHW;
  } else if (MODE == M_DGRAD) {
    int q = n0 + bcol;
    cvalid = q < Ncols;
    int qq = cvalid ? q : 0;
    int n = qq / (Hc * Wc), r = qq % (Hc * Wc);
    hi0 = (r / Wc) * a.stride + ph + a.pad;  // hi + pad
    wi0 = (r % Wc) * a.stride + pw + a.pad;
    nbdy = (long long)n * a.Cout * HoWo;
  }
  const bool has0 = a.sc0 != nullptr, has1 = a.sc1 != nullptr;
  const float slope0 = act_slope(a.act0), slope1 = act_slope(a.act1);   // branch-free activation (common.h)
  const int pixoff = hi0 * a.Ws + wi0;   // fwd: offset of the (possibly out-of-range) window origin
  static_assert(!(BUF && UP2X), "the bilinear gather keeps the 64-bit loader");
  // BUF loader state.  tinv: bit t set = tap t of this column lies outside the image (bit 31 is always set: the tap index
  // an element past K is given).  voff0/voff1: byte offset of the lane's window origin in source 0/1 (fwd, modulo 2^32: it is
  // negative where the window starts in the padding, and a valid tap's offset brings the sum back in range) or of its
  // (hi / stride, wi / stride) pixel in dY (dgrad).
  unsigned tinv = 0xffffffffu, voff0 = 0, voff1 = 0;
  int dbh = 0, dbw = 0;   // dgrad: (hi + pad) % stride, (wi + pad) % stride: uniform over a parity class
  __amdgpu_buffer_rsrc_t rs0, rs1;
  if constexpr (BUF && MODE == M_FWD) {
    for (int t = 0; t < KHW; ++t) {   // t, kh, kw uniform
      const int hi = hi0 + (t / a.KW) * a.dil, wi = wi0 + (t % a.KW) * a.dil;
      const bool ok = cvalid && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
      tinv &= ~((unsigned)ok << t);
    }
    voff0 = 4u * (unsigned)(nb0 + pixoff);
    voff1 = 4u * (unsigned)(nb1 + pixoff);
    rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x0, 0, (int)(4u * (unsigned)((long long)a.N * a.C0 * srcHW)), 0x00020000);
    rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.C1 ? a.x1 : a.x0), 0,
                                            (int)(4u * (unsigned)((long long)a.N * (a.C1 ? a.C1 : a.C0) * srcHW)), 0x00020000);
  } else if constexpr (BUF && MODE == M_DGRAD) {
    const int sm = a.stride - 1;   // stride is 1, 2 or 4
    dbh = (ph + a.pad) & sm;
    dbw = (pw + a.pad) & sm;
    const int ah = hi0 >> a.lstride, aw = wi0 >> a.lstride;
    const int nth = s_tab[0];
    for (int ih = 0; ih < nth; ++ih)
      for (int iw = 0; iw < ntw; ++iw) {   // a class tap's (db - k * dil) is a multiple of the stride: the shift is exact
        const int ho = ah + ((dbh - s_tab[2 + ih] * a.dil) >> a.lstride), wo = aw + ((dbw - s_tab[12 + iw] * a.dil) >> a.lstride);
        const bool ok = cvalid && (unsigned)ho < (unsigned)a.Ho && (unsigned)wo < (unsigned)a.Wo;
        tinv &= ~((unsigned)ok << (ih * ntw + iw));
      }
    voff0 = 4u * (unsigned)(nbdy + ah * a.Wo + aw);
    rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, (int)(4u * (unsigned)((long long)a.N * a.Cout * HoWo)), 0x00020000);
  }
  // BUF wgrad: a thread's columns (k) and dY rows (co) never change, so their byte offsets and tap indices are registers; per
  // K-tile it decodes its pixel once, builds the pixel's mask of taps outside the image (tinv) from a row and a column mask,
  // and an element is again one add, one bit-field extract and one or.  A workgroup whose columns straddle the two sources
  // loads every element from both resources, one of them out of range.
  constexpr int WBE = (BUF && MODE == M_WGRAD) ? BN / (256 / BK) : 1, WAE = (BUF && MODE == M_WGRAD) ? BM / (256 / BK) : 1;
  unsigned wcoff[WBE], wrow[WAE], wfirst = 0, voffa = 0;
  int wtap[WBE];
  __amdgpu_buffer_rsrc_t rsd;
  if constexpr (BUF && MODE == M_WGRAD) {
    const int grp = tid / BK;
#pragma unroll
    for (int e = 0; e < WBE; ++e) {
      const int tab = s_tab[grp + (256 / BK) * e], k = n0 + grp + (256 / BK) * e;
      const int ci = tab & 0xffff;
      const bool first = tab < 0 || ci < a.C0;
      wcoff[e] = 4u * ((unsigned)(first ? ci : ci - a.C0) * (unsigned)srcHW + (unsigned)(((tab >> 16) & 0xff) * a.Ws + ((tab >> 24) & 0xff)));
      wtap[e] = tab < 0 ? 31 : k % KHW;                     // a column past Ncols: the always-invalid tap
      wfirst |= (unsigned)first << e;
    }
#pragma unroll
    for (int e = 0; e < WAE; ++e) wrow[e] = 4u * (unsigned)min(m0 + grp + (256 / BK) * e, M - 1) * (unsigned)HoWo;
    rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)a.x0, 0, (int)(4u * (unsigned)((long long)a.N * a.C0 * srcHW)), 0x00020000);
    rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.C1 ? a.x1 : a.x0), 0,
                                            (int)(4u * (unsigned)((long long)a.N * (a.C1 ? a.C1 : a.C0) * srcHW)), 0x00020000);
    rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, (int)(4u * (unsigned)((long long)a.N * a.Cout * HoWo)), 0x00020000);
  }

  float braw[NBR], bsc[NSC], bsh[NSC];
  f32x4 areg4[AV];   // native vector type (a float4 struct array would live in scratch memory)
  float areg[(MODE == M_WGRAD) ? AE : 1];
  unsigned bmask = 0, bfirst = 0, amask = 0;

  // ---- BUF: decode of the rows of K-tile kt by threads 0 .. BK-1 (dec_issue: arithmetic and the BatchNorm loads, before the
  // MFMA loop; dec_finish: the LDS store, after it) ----
  unsigned dk_off = 0, dk_tap = 31, dk_c = 0, dk_d = 0;
  auto dec_issue = [&](int kt) __attribute__((always_inline)) {
    if constexpr (DEC) {
      if (tid < BK) {
        const int k = kt * BK + tid;
        const bool kok = k < K;
        if (MODE == M_FWD) {
          const int ci = k / KHW, r = k - ci * KHW, kh = r / a.KW, kw = r - kh * a.KW;
          const int cc = min(ci, a.Cin - 1);
          const bool first = cc < a.C0;
          const int c = first ? cc : cc - a.C0;
          dk_off = 4u * ((unsigned)c * (unsigned)srcHW + (unsigned)((kh * a.Ws + kw) * a.dil));
          dk_tap = kok ? r : 31;
          const float* sp = first ? a.sc0 : a.sc1;
          const float* hp = first ? a.sh0 : a.sh1;
          dk_c = __float_as_uint(sp ? sp[c] : 1.f);
          dk_d = __float_as_uint(sp ? hp[c] : 0.f);
        } else {
          const int kk = kok ? k : 0, t = kk / a.Cout, co = kk - t * a.Cout, ih = t / ntw, iw = t - ih * ntw;
          const int kh = s_tab[2 + ih], kw = s_tab[12 + iw];
          const int tapoff = ((dbh - kh * a.dil) >> a.lstride) * a.Wo + ((dbw - kw * a.dil) >> a.lstride);
          dk_off = 4u * (unsigned)(co * HoWo + tapoff);   // modulo 2^32: a valid lane's sum is in range
          dk_tap = kok ? t : 31;
          dk_c = kok ? (unsigned)((kh * a.KW + kw) * a.Cout + co) : 0xffffffffu;
        }
      }
    }
  };
  auto dec_finish = [&](int buf) __attribute__((always_inline)) {
    if constexpr (DEC) {
      if (tid < BK) *reinterpret_cast<uint4*>(&s_dec[buf][tid][0]) = make_uint4(dk_off, dk_tap, dk_c, dk_d);
    }
  };
  // the K-tile's rows of this wave against the switch from source 0 to source 1 (fwd): 0 / 1 = all in that source, 2 = mixed
  const int S0 = a.C0 * KHW;
  int cls = 0, kf = 0;
  if constexpr (BUF && MODE == M_WGRAD) cls = (a.C1 == 0 || n0 + BN <= S0) ? 0 : (n0 >= S0 ? 1 : 2);   // the workgroup's columns
  int binv[(BUF && MODE == M_FWD) ? BROWS : 1];   // 0 or -1 (outside the image / past K), kept for finish()
  auto src_first = [&](auto tag, int e) __attribute__((always_inline)) {
    constexpr int SRC = decltype(tag)::value;
    return SRC == 0 || (SRC == 2 && kf + e < S0);
  };
  auto with_cls = [&](auto&& body) __attribute__((always_inline)) {
    if (cls == 0) body(std::integral_constant<int, 0>{});
    else if (cls == 1) body(std::integral_constant<int, 1>{});
    else body(std::integral_constant<int, 2>{});
  };
  auto issue_buf = [&](int kt) __attribute__((always_inline)) {
    const int db = kt & 1;
    if constexpr (MODE == M_FWD) {
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        int idx = tid + 256 * e, row = idx / A4, c4 = idx % A4;
        areg4[e] = *reinterpret_cast<const f32x4*>(a.wp + (long long)(kt * BK + row) * a.wp_ld + m0 + c4 * 4);
      }
      kf = kt * BK + brow0;                                // wave-uniform
      cls = (a.C1 == 0 || kf + BROWS <= S0) ? 0 : (kf >= S0 ? 1 : 2);
      with_cls([&](auto tag) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < BROWS; ++e) {
          const uint2 d = *reinterpret_cast<const uint2*>(&s_dec[db][brow0 + e][0]);   // uniform address: a broadcast read
          const bool first = src_first(tag, e);
          binv[e] = __builtin_amdgcn_sbfe((int)tinv, d.y, 1u);
          const unsigned off = ((first ? voff0 : voff1) + d.x) | (unsigned)binv[e];
          braw[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(first ? rs0 : rs1, (int)off, 0, 0));
        }
      });
    } else if constexpr (MODE == M_DGRAD) {
      amask = 0;
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        int idx = tid + 256 * e, row = idx / A4, c4 = idx % A4;
        const int wrow = (int)s_dec[db][row][2];
        const bool ok = wrow >= 0;
        areg4[e] = *reinterpret_cast<const f32x4*>(a.wp + (long long)(ok ? wrow : 0) * a.wp_ld + m0 + c4 * 4);
        amask |= (unsigned)ok << e;
      }
#pragma unroll
      for (int e = 0; e < BROWS; ++e) {
        const uint2 d = *reinterpret_cast<const uint2*>(&s_dec[db][brow0 + e][0]);
        const unsigned off = (voff0 + d.x) | (unsigned)__builtin_amdgcn_sbfe((int)tinv, d.y, 1u);
        braw[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs0, (int)off, 0, 0));
      }
    } else {
      const int p = p_begin + kt * BK + (tid % BK);
      const bool pv = p < p_end;
      const int pp = pv ? p : 0;
      const int n = pp / HoWo, hw = pp - n * HoWo, ho = hw / a.Wo, wo = hw - ho * a.Wo;
      const int hb = ho * a.stride - a.pad, wb = wo * a.stride - a.pad;
      unsigned rinv = 0, cinv = 0;
      for (int kh = 0; kh < a.KH; ++kh) rinv |= (unsigned)((unsigned)(hb + kh * a.dil) >= (unsigned)a.H) << kh;
      for (int kw = 0; kw < a.KW; ++kw) cinv |= (unsigned)((unsigned)(wb + kw * a.dil) >= (unsigned)a.W) << kw;
      const unsigned full = (1u << a.KW) - 1u;
      tinv = 0x80000000u;
      for (int kh = 0; kh < a.KH; ++kh) tinv |= (((rinv >> kh) & 1u) ? full : cinv) << (kh * a.KW);
      if (!pv) tinv = 0xffffffffu;
      const int pix = hb * a.Ws + wb;
      voff0 = 4u * (unsigned)((long long)n * a.C0 * srcHW + pix);
      voff1 = 4u * (unsigned)((long long)n * a.C1 * srcHW + pix);
      voffa = 4u * (unsigned)((long long)n * a.Cout * HoWo + hw);
      amask = pv ? 0xffffffffu : 0u;
#pragma unroll
      for (int e = 0; e < WAE; ++e)   // rows >= M are never stored by the epilogue
        areg[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsd, (int)(voffa + wrow[e]), 0, 0));
      with_cls([&](auto tag) __attribute__((always_inline)) {
        constexpr int SRC = decltype(tag)::value;
#pragma unroll
        for (int e = 0; e < WBE; ++e) {
          const unsigned inv = (unsigned)__builtin_amdgcn_sbfe((int)tinv, (unsigned)wtap[e], 1u);
          if constexpr (SRC != 2) {
            const unsigned off = ((SRC == 0 ? voff0 : voff1) + wcoff[e]) | inv;
            braw[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(SRC == 0 ? rs0 : rs1, (int)off, 0, 0));
          } else {
            const unsigned f = 0u - ((wfirst >> e) & 1u);   // all ones: the column is in source 0
            const int l0 = __builtin_amdgcn_raw_buffer_load_b32(rs0, (int)((voff0 + wcoff[e]) | inv | ~f), 0, 0);
            const int l1 = __builtin_amdgcn_raw_buffer_load_b32(rs1, (int)((voff1 + wcoff[e]) | inv | f), 0, 0);
            braw[e] = __builtin_bit_cast(float, l0 | l1);
          }
        }
      });
    }
  };
  auto finish_buf = [&](int buf) __attribute__((always_inline)) {
    if constexpr (MODE == M_WGRAD) {
      const int pl = tid % BK, grp = tid / BK;
#pragma unroll
      for (int e = 0; e < WAE; ++e) As[buf][pl][grp + (256 / BK) * e] = amask ? areg[e] : 0.f;
#pragma unroll
      for (int e = 0; e < WBE; ++e) {
        const int col = grp + (256 / BK) * e;
        const float v = act_by_slope(fmaf(braw[e], s_sc[col], s_sh[col]), __int_as_float(s_code[col]));
        // the padding of an affine operand (and a pixel past the chunk) is zeroed here
        Bs[buf][pl][col] = __uint_as_float(__float_as_uint(v) & ~(unsigned)__builtin_amdgcn_sbfe((int)tinv, (unsigned)wtap[e], 1u));
      }
      return;
    }
#pragma unroll
    for (int e = 0; e < AV; ++e) {
      int idx = tid + 256 * e, row = idx / A4, c4 = idx % A4;
      f32x4 v = areg4[e];
      if (MODE == M_DGRAD && !((amask >> e) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(&As[buf][row][c4 * 4]) = v;
    }
    if constexpr (MODE == M_FWD) {
      with_cls([&](auto tag) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < BROWS; ++e) {
          const float2 ss = *reinterpret_cast<const float2*>(&s_dec[buf][brow0 + e][2]);   // identity where there is no affine
          float v = act_by_slope(fmaf(braw[e], ss.x, ss.y), src_first(tag, e) ? slope0 : slope1);
          // act(affine(0)) != 0: the padding of an affine operand is zeroed here (a raw operand's already loaded as 0)
          Bs[buf][brow0 + e][bcol] = __uint_as_float(__float_as_uint(v) & ~(unsigned)binv[e]);
        }
      });
    } else {
#pragma unroll
      for (int e = 0; e < BROWS; ++e) Bs[buf][brow0 + e][bcol] = braw[e];   // outside the image: loaded as 0
    }
  };

  auto issue = [&](int kt) __attribute__((always_inline)) {
    if constexpr (BUF) {
      issue_buf(kt);
      return;
    }
    if (MODE == M_FWD) {
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        int idx = tid + 256 * e, row = idx / A4, c4 = idx % A4;
        areg4[e] = *reinterpret_cast<const f32x4*>(a.wp + (long long)(kt * BK + row) * a.wp_ld + m0 + c4 * 4);
      }
      const int k = kt * BK + brow0;                       // wave-uniform
      int ci = k / KHW, r = k % KHW, kh = r / a.KW, kw = r % a.KW;
      bmask = 0;
      bfirst = 0;
#pragma unroll
      for (int e = 0; e < BROWS; ++e) {
        const int dh = kh * a.dil, dw = kw * a.dil;          // uniform
        const int hi = hi0 + dh, wi = wi0 + dw;
        const bool ok = cvalid && (k + e < K) && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
        const int cc = min(ci, a.Cin - 1);
        if constexpr (UP2X) {  // the bilinear gather finishes here (raw value is final)
          braw[e] = ok ? load_virtual(a, nb0, nb1, cc, hi, wi) : 0.f;
          bsc[e] = 1.f;
          bsh[e] = 0.f;
        } else {
          const bool first = cc < a.C0;                      // uniform
          const int c = first ? cc : cc - a.C0;
          const float* xc = (first ? a.x0 : a.x1) + (long long)c * srcHW + (dh * a.Ws + dw);   // uniform pointer
          const long long lane_off = (first ? nb0 : nb1) + (ok ? pixoff : -(dh * a.Ws + dw));
          braw[e] = xc[lane_off];
          const bool has = first ? has0 : has1;
          bsc[e] = has ? (first ? a.sc0 : a.sc1)[c] : 1.f;   // uniform -> scalar loads
          bsh[e] = has ? (first ? a.sh0 : a.sh1)[c] : 0.f;
          bfirst |= (unsigned)first << e;
        }
        bmask |= (unsigned)ok << e;
        if (++kw == a.KW) {
          kw = 0;
          if (++kh == a.KH) { kh = 0; ++ci; }
        }
      }
    } else if (MODE == M_DGRAD) {
      amask = 0;
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        int idx = tid + 256 * e, row = idx / A4, c4 = idx % A4;
        int k = kt * BK + row;
        bool ok = k < K;
        int kk = ok ? k : 0;
        int co = kk % a.Cout, t = kk / a.Cout;
        int kh = s_tab[2 + t / ntw], kw = s_tab[12 + t % ntw];
        areg4[e] = *reinterpret_cast<const f32x4*>(a.wp + (long long)((kh * a.KW + kw) * a.Cout + co) * a.wp_ld + m0 +
                                                   c4 * 4);
        amask |= (unsigned)ok << e;
      }
      const int k = kt * BK + brow0;                       // wave-uniform
      int co = k % a.Cout, t = k / a.Cout;
      bmask = 0;
#pragma unroll
      for (int e = 0; e < BROWS; ++e) {
        const bool kok = k + e < K;
        const int tt = kok ? t : 0;
        const int kh = __builtin_amdgcn_readfirstlane(s_tab[2 + tt / ntw]);
        const int kw = __builtin_amdgcn_readfirstlane(s_tab[12 + tt % ntw]);
        const int th = hi0 - kh * a.dil, tw = wi0 - kw * a.dil;
        const int ho = th >> a.lstride, wo = tw >> a.lstride;   // exact: the parity class makes th,tw multiples of stride
        const bool ok = cvalid && kok && th >= 0 && tw >= 0 && ho < a.Ho && wo < a.Wo;
        const float* yc = a.dy + (long long)co * HoWo;       // uniform pointer
        braw[e] = yc[nbdy + (ok ? ho * a.Wo + wo : 0)];
        bmask |= (unsigned)ok << e;
        if (++co == a.Cout) { co = 0; ++t; }
      }
    } else {  // WGRAD: thread owns one pixel row (p_local) and AE/BE strided columns
      int p = p_begin + kt * BK + (tid % BK);
      bool pv = p < p_end;
      int pp = pv ? p : 0;
      int n = pp / HoWo, hw = pp % HoWo;
      int hb = (hw / a.Wo) * a.stride - a.pad, wb = (hw % a.Wo) * a.stride - a.pad;
      long long b0 = (long long)n * a.C0 * srcHW, b1 = (long long)n * a.C1 * srcHW;
      long long bdy = (long long)n * a.Cout * HoWo + hw;
      const int grp = tid / BK;
      amask = pv ? 0xffffffffu : 0u;
#pragma unroll
      for (int e = 0; e < AE; ++e) {
        int co = min(m0 + grp + PG * e, M - 1);   // rows >= M are never stored by the epilogue
        areg[e] = a.dy[bdy + (long long)co * HoWo];
      }
      bmask = 0;
#pragma unroll
      for (int e = 0; e < BE; ++e) {
        int tab = s_tab[grp + PG * e];
        int tt = tab >= 0 ? tab : 0;
        int ci = tt & 0xffff, hi = hb + ((tt >> 16) & 0xff), wi = wb + ((tt >> 24) & 0xff);
        bool ok = pv && tab >= 0 && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
        if constexpr (UP2X) {
          braw[e] = ok ? load_virtual(a, b0, b1, ci, hi, wi) : 0.f;
        } else {
          bool first = ci < a.C0;
          int c = first ? ci : ci - a.C0;
          const float* xb = first ? a.x0 + b0 : a.x1 + b1;
          int off = ok ? hi * a.Ws + wi : 0;
          braw[e] = xb[(long long)c * srcHW + off];
        }
        bmask |= (unsigned)ok << e;
      }
    }
  };

  auto finish = [&](int buf) __attribute__((always_inline)) {
    if constexpr (BUF) {
      finish_buf(buf);
      return;
    }
    if (MODE == M_FWD) {
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        int idx = tid + 256 * e, row = idx / A4, c4 = idx % A4;
        *reinterpret_cast<f32x4*>(&As[buf][row][c4 * 4]) = areg4[e];
      }
#pragma unroll
      for (int e = 0; e < BROWS; ++e) {
        float v = braw[e];
        if constexpr (!UP2X) {
          bool first = (bfirst >> e) & 1u;
          if (first ? has0 : has1) v = fmaf(v, bsc[e], bsh[e]);
          v = act_by_slope(v, first ? slope0 : slope1);
        }
        Bs[buf][brow0 + e][bcol] = ((bmask >> e) & 1u) ? v : 0.f;
      }
    } else if (MODE == M_DGRAD) {
#pragma unroll
      for (int e = 0; e < AV; ++e) {
        int idx = tid + 256 * e, row = idx / A4, c4 = idx % A4;
        f32x4 v = areg4[e];
        if (!((amask >> e) & 1u)) v = f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(&As[buf][row][c4 * 4]) = v;
      }
#pragma unroll
      for (int e = 0; e < BROWS; ++e) Bs[buf][brow0 + e][bcol] = ((bmask >> e) & 1u) ? braw[e] : 0.f;
    } else {
      const int pl = tid % BK, grp = tid / BK;
#pragma unroll
      for (int e = 0; e < AE; ++e) As[buf][pl][grp + PG * e] = amask ? areg[e] : 0.f;
#pragma unroll
      for (int e = 0; e < BE; ++e) {
        float v = braw[e];
        if constexpr (!UP2X) {
          int col = grp + PG * e;
          int code = s_code[col];   // bit0: affine present, bits1-2: activation
          if (code & 1) v = fmaf(v, s_sc[col], s_sh[col]);
          v = act_by_slope(v, act_slope(code >> 1));
        }
        Bs[buf][pl][grp + PG * e] = ((bmask >> e) & 1u) ? v : 0.f;
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if constexpr (DEC) {   // the tables of the first two K-tiles
    if (nK > kt0) { dec_issue(kt0); dec_finish(kt0 & 1); }
    if (nK > kt0 + 1) { dec_issue(kt0 + 1); dec_finish((kt0 + 1) & 1); }
    __syncthreads();
  }
  if (nK > kt0) {
    issue(kt0);
    finish(kt0 & 1);
  }
  __syncthreads();
  const int li = lane & 31, lk = lane >> 5;
  for (int kt = kt0; kt < nK; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nK) issue(kt + 1);
    if (kt + 2 < nK) dec_issue(kt + 2);
    // operands of k-step k2+1 are read before the MFMAs of k-step k2 issue (order pinned with sched_barrier):
    // the LDS latency hides behind TM*TN*64 MFMA cycles instead of stalling the wave every step
    float av[2][TM], bv[2][TN];
    auto read_ops = [&](int k2, int slot) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < TM; ++i) av[slot][i] = As[buf][2 * k2 + lk][wm * WTM + i * 32 + li];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[slot][j] = Bs[buf][2 * k2 + lk][wn * WTN + j * 32 + li];
    };
    read_ops(0, 0);
#pragma unroll
    for (int k2 = 0; k2 < BK / 2; ++k2) {
      const int cur = k2 & 1;
      if (k2 + 1 < BK / 2) read_ops(k2 + 1, cur ^ 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i], bv[cur][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kt + 1 < nK) finish(buf ^ 1);
    if (kt + 2 < nK) dec_finish(buf);   // tile kt's table was last read before the previous barrier
    __syncthreads();
  }

  // ---------------- epilogue ----------------
  // C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  long long cbase[TN];
  bool cok[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    int col = n0 + wn * WTN + j * 32 + li;
    cok[j] = col < Ncols;
    int cc = cok[j] ? col : 0;
    if (MODE == M_FWD) {
      int n = cc / HoWo, hw = cc % HoWo;
      cbase[j] = (long long)ksplit * a.slab + (long long)n * a.Cout * HoWo + hw;
    } else if (MODE == M_DGRAD) {
      int n = cc / (Hc * Wc), r = cc % (Hc * Wc);
      cbase[j] = (long long)ksplit * a.slab + (long long)n * a.Cin * HW + ((r / Wc) * a.stride + ph) * a.W +
                 (r % Wc) * a.stride + pw;
    } else {
      cbase[j] = (long long)blockIdx.y * M * Ncols + cc;
    }
  }
  const long long rstride = (MODE == M_FWD) ? HoWo : (MODE == M_DGRAD ? HW : Ncols);
  const bool want_stats = (MODE == M_FWD) && a.stats != nullptr && a.kts == 0;
  // per-row partial sums of this wave go to LDS (the operand tiles are dead after the last barrier),
  // so each workgroup issues ONE pair of double atomics per output channel
  float* s_sum = &As[0][0][0];   // [WN][BM]
  float* s_sq = &Bs[0][0][0];    // [WN][BM]
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int lrow = wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
      int row = m0 + lrow;
      bool rok = row < M;
      float bias = (MODE == M_FWD && a.bias && rok && a.kts == 0) ? a.bias[row] : 0.f;
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        float v = acc[i][j][r] + bias;
        if (rok && cok[j]) {
          a.out[cbase[j] + (long long)row * rstride] = v;
          s += v;
          q += v * v;
        }
      }
      if (want_stats) {
        s = half_sum(s);
        q = half_sum(q);
        if (li == 0) {
          s_sum[wn * BM + lrow] = s;
          s_sq[wn * BM + lrow] = q;
        }
      }
    }
  }
  if (want_stats) {
    __syncthreads();
    for (int rr = tid; rr < BM; rr += 256) {
      int row = m0 + rr;
      if (row < M) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int w = 0; w < WN; ++w) { s += s_sum[w * BM + rr]; q += s_sq[w * BM + rr]; }
        atomicAdd(&a.stats[row], (double)s);
        atomicAdd(&a.stats[M + row], (double)q);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// small helper kernels
// ---------------------------------------------------------------------------
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ out, int Cout, int Cin, int KH,
                                    int KW, int rows, int ld, int mode) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)rows * ld;
  if (i >= total) return;
  int row = (int)(i / ld), col = (int)(i % ld);
  int KHW = KH * KW;
  float v = 0.f;
  if (mode == 0) {  // row = k = (ci,kh,kw), col = co
    if (row < Cin * KHW && col < Cout) v = w[(long long)col * Cin * KHW + row];
  } else {  // row = tap*Cout + co, col = ci
    if (row < KHW * Cout && col < Cin) {
      int tap = row / Cout, co = row % Cout;
      v = w[((long long)co * Cin + col) * KHW + tap];
    }
  }
  out[i] = v;
}

// out[i] = sum over S slabs (`stride` elements apart) of ws[z][i], i < n.  Block = 64 consecutive elements x 4 slab groups:
// thread (e, q) sums slabs z = q, q + 4, ... with four independent loads in flight, the four partials are added in a fixed
// order through LDS (deterministic).  The one-thread-per-element form walked its S slabs as one dependent chain: 0.15 TB/s
// on a [256 x 1152] gradient with 32 slabs.
// E elements x G = 256 / E slab groups per block: 64 x 4 for large gradients; 16 x 16 when n is small and S large (the decoder
// head's [2 x 128 x 9] gradient has 512 slabs: 36 blocks of the 64-element form left 220 CUs idle, 106 us).
template <int E>
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ ws, float* __restrict__ out, long long n,
                                                           int S, long long stride) {
  constexpr int G = 256 / E;
  __shared__ float part[G][E];
  const int e = threadIdx.x % E, q = threadIdx.x / E;
  const long long i = (long long)blockIdx.x * E + e;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < n) {
    int z = q;
    for (; z + 3 * G < S; z += 4 * G) {
      s0 += ws[(long long)z * stride + i];
      s1 += ws[(long long)(z + G) * stride + i];
      s2 += ws[(long long)(z + 2 * G) * stride + i];
      s3 += ws[(long long)(z + 3 * G) * stride + i];
    }
    for (; z < S; z += G) s0 += ws[(long long)z * stride + i];
  }
  part[q][e] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (q == 0 && i < n) {
    float v[G];
#pragma unroll
    for (int g = 0; g < G; ++g) v[g] = part[g][e];
#pragma unroll
    for (int w = G / 2; w > 0; w >>= 1)        // fixed pairwise order: deterministic
#pragma unroll
      for (int g = 0; g < w; ++g) v[g] = v[2 * g] + v[2 * g + 1];
    out[i] = v[0];
  }
}
static int launch_reduce_slabs(const float* ws, float* out, long long n, int S, long long stride, hipStream_t st) {
  if (n <= 16384 && S >= 64) hipLaunchKernelGGL(reduce_slabs_kernel<16>, dim3(cdiv(n, 16)), dim3(256), 0, st, ws, out, n, S, stride);
  else hipLaunchKernelGGL(reduce_slabs_kernel<64>, dim3(cdiv(n, 64)), dim3(256), 0, st, ws, out, n, S, stride);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// split-K forward combine: y = sum of slabs (+ bias); per-channel (sum, sumsq) for the following BatchNorm.
// grid (C, chunks); a block owns one channel over a slice of (n, hw)
__global__ __launch_bounds__(256) void splitk_combine_kernel(const float* __restrict__ ws, long long slab, int S, int N, int C,
                                                             int HW, const float* __restrict__ bias,
                                                             float* __restrict__ y, double* stats) {
  const int c = blockIdx.x;
  const float b = bias ? bias[c] : 0.f;
  const int n_per = (N + gridDim.y - 1) / gridDim.y, n_beg = blockIdx.y * n_per, n_end = min(N, n_beg + n_per);
  float s1 = 0.f, s2 = 0.f;
  // the block's (image, pixel) pairs as ONE index range: the maps that need split-K are 2x2 ... 8x8, and a loop over the
  // pixels of one image left 75-98 % of the threads idle; two slab chains in flight per element
  const int total = (n_end - n_beg) * HW;
  for (int e = threadIdx.x; e < total; e += 256) {
    const int n = n_beg + e / HW, i = e - (e / HW) * HW;
    const long long base = ((long long)n * C + c) * HW + i;
    float v0 = b, v1 = 0.f;
    int z = 0;
    for (; z + 1 < S; z += 2) {
      v0 += ws[(long long)z * slab + base];
      v1 += ws[(long long)(z + 1) * slab + base];
    }
    if (z < S) v0 += ws[(long long)z * slab + base];
    const float v = v0 + v1;
    y[base] = v;
    s1 += v;
    s2 += v * v;
  }
  if (stats) {
    double d1 = wave_sum_d((double)s1), d2 = wave_sum_d((double)s2);
    __shared__ double sh[8];
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = d1; sh[4 + (threadIdx.x >> 6)] = d2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      atomicAdd(&stats[c], sh[0] + sh[1] + sh[2] + sh[3]);
      atomicAdd(&stats[C + c], sh[4] + sh[5] + sh[6] + sh[7]);
    }
  }
}

// dbias[c] = sum over n,hw of dy[n,c,hw]; one block per channel
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ x, int N, int C, int HW,
                                                          float* __restrict__ out) {
  int c = blockIdx.x;
  double s = 0.0;
  for (int n = 0; n < N; ++n) {
    const float* p = x + ((long long)n * C + c) * HW;
    float t = 0.f;
    for (int i = threadIdx.x; i < HW; i += 256) t += p[i];
    s += (double)t;
  }
  __shared__ double sh[4];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[c] = (float)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int check_desc(const avsep_conv_desc* d, bool fwd_only = false) {
  if (!d || !d->x0) return AVSEP_ERR_ARG;
  if (d->N <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->H <= 0 || d->W <= 0) return AVSEP_ERR_ARG;
  if (d->KH <= 0 || d->KW <= 0 || d->stride <= 0 || d->dil <= 0) return AVSEP_ERR_ARG;
  // the dgrad tap tables and the wgrad column table hold at most 8 taps per axis / 8-bit offsets
  if (!fwd_only && (d->KH > 8 || d->KW > 8 || (d->KH - 1) * d->dil > 255 || (d->KW - 1) * d->dil > 255 ||
                    d->Cin > 65535))
    return AVSEP_ERR_ARG;
  if (d->C0 <= 0 || d->C0 > d->Cin || (d->C0 < d->Cin && !d->x1)) return AVSEP_ERR_ARG;
  int ho = (d->H + 2 * d->pad - d->dil * (d->KH - 1) - 1) / d->stride + 1;
  int wo = (d->W + 2 * d->pad - d->dil * (d->KW - 1) - 1) / d->stride + 1;
  if (ho != d->Ho || wo != d->Wo) return AVSEP_ERR_ARG;
  if (d->up2x && ((d->H & 1) || (d->W & 1))) return AVSEP_ERR_ARG;
  if ((d->scale0 == nullptr) != (d->shift0 == nullptr)) return AVSEP_ERR_ARG;
  if ((d->scale1 == nullptr) != (d->shift1 == nullptr)) return AVSEP_ERR_ARG;
  if (d->prec != AVSEP_PREC_F32 && d->prec != AVSEP_PREC_BF16) return AVSEP_ERR_ARG;
  return AVSEP_OK;
}

static CArgs make_args(const avsep_conv_desc* d) {
  CArgs a{};
  a.N = d->N; a.Cin = d->Cin; a.H = d->H; a.W = d->W; a.Cout = d->Cout; a.Ho = d->Ho; a.Wo = d->Wo;
  a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad; a.dil = d->dil;
  a.C0 = d->C0; a.C1 = d->Cin - d->C0; a.act0 = d->act0; a.act1 = d->act1; a.up2x = d->up2x;
  a.Hs = d->up2x ? d->H / 2 : d->H;
  a.Ws = d->up2x ? d->W / 2 : d->W;
  a.rh = (d->up2x && d->H > 1) ? (float)(a.Hs - 1) / (float)(d->H - 1) : 0.f;
  a.rw = (d->up2x && d->W > 1) ? (float)(a.Ws - 1) / (float)(d->W - 1) : 0.f;
  a.x0 = d->x0; a.x1 = d->x1; a.sc0 = d->scale0; a.sh0 = d->shift0; a.sc1 = d->scale1; a.sh1 = d->shift1;
  return a;
}

// split-K combines, shared with the other conv files
int splitk_combine(const float* ws, long long slab, int S, const avsep_conv_desc* d, const float* bias, float* y, double* stats,
                   hipStream_t st) {
  int chunks = min(cdiv(1024, d->Cout), d->N);
  if (chunks < 1) chunks = 1;
  hipLaunchKernelGGL(splitk_combine_kernel, dim3(d->Cout, chunks), dim3(256), 0, st, ws, slab, S, d->N, d->Cout, d->Ho * d->Wo,
                     bias, y, stats);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
int reduce_slabs_strided(const float* ws, float* out, long long n, int S, long long stride, hipStream_t st) {
  return launch_reduce_slabs(ws, out, n, S, stride, st);
}
int reduce_slabs(const float* ws, float* out, long long n, int S, hipStream_t st) { return launch_reduce_slabs(ws, out, n, S, n, st); }

// ---------------------------------------------------------------------------
// the im2col family (igemm): serves every descriptor, so it closes each route table
// ---------------------------------------------------------------------------
static inline int packed_rows(const avsep_conv_desc* d, int mode) {
  return mode == 0 ? roundup(d->Cin * d->KH * d->KW, 32) : roundup(d->KH * d->KW * d->Cout, 32);
}
static bool igemm_applicable(const avsep_conv_desc*, int) { return true; }
static size_t igemm_packed_floats(const avsep_conv_desc* d, int mode) { return (size_t)packed_rows(d, mode) * igemm_packed_ld(d, mode); }
static int igemm_pack(const avsep_conv_desc* d, const float* w, float* packed, int mode, hipStream_t st) {
  int rows = packed_rows(d, mode), ld = igemm_packed_ld(d, mode);
  long long total = (long long)rows * ld;
  hipLaunchKernelGGL(pack_weights_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, w, packed, d->Cout, d->Cin, d->KH, d->KW,
                     rows, ld, mode);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// big tiles when they still fill the chip, else 64x64
static inline bool use_big(int M, long long ncols) {
  return M > 64 && (long long)cdiv(M, 128) * cdiv(ncols, 128) >= 64;   // few big tiles are topped up by split-K
}

// split-K plan for layers whose output grid cannot fill the chip (deep U-Net levels: 2x2 .. 8x8 maps, K ~ 8-9k)
struct SplitPlan { int splits, kts; };
static SplitPlan splitk_plan(long long tiles, int K) {
  SplitPlan p{1, 0};
  int nK = cdiv(K, 16);
  if (tiles >= 640 || nK < 64) return p;
  int want = cdiv(768, tiles), maxs = nK / 32;
  int s = want < maxs ? want : maxs;
  if (s > 32) s = 32;
  if (s < 2) return p;
  p.kts = cdiv(nK, s);
  p.splits = cdiv(nK, p.kts);
  if (p.splits < 2) { p.splits = 1; p.kts = 0; }
  return p;
}
// the im2col kernel's tile size and split-K are decided on the planned batch (plan_desc), like every launch heuristic
static bool fwd_big(const avsep_conv_desc* d) { return use_big(d->Cout, (long long)plan_batch(d) * d->Ho * d->Wo); }
static bool dgrad_big(const avsep_conv_desc* d) {
  const int s = d->stride;
  return use_big(d->Cin, (long long)plan_batch(d) * cdiv(d->H, s) * cdiv(d->W, s) * s * s);
}
static SplitPlan fwd_split(const avsep_conv_desc* d) {
  long long ncols = (long long)plan_batch(d) * d->Ho * d->Wo;
  bool big = use_big(d->Cout, ncols);
  long long tiles = big ? (long long)cdiv(d->Cout, 128) * cdiv(ncols, 128) : (long long)cdiv(d->Cout, 64) * cdiv(ncols, 64);
  return splitk_plan(tiles, d->Cin * d->KH * d->KW);
}
static SplitPlan dgrad_split(const avsep_conv_desc* d) {
  const int s = d->stride;
  long long ncols = (long long)plan_batch(d) * cdiv(d->H, s) * cdiv(d->W, s);
  bool big = use_big(d->Cin, ncols * s * s);
  long long tiles = (big ? (long long)cdiv(d->Cin, 128) * cdiv(ncols, 128) : (long long)cdiv(d->Cin, 64) * cdiv(ncols, 64)) * s * s;
  int taps = cdiv(d->KH, s) * cdiv(d->KW, s);               // taps of the fullest parity class
  return splitk_plan(tiles, taps * d->Cout);
}
struct WgradPlan {
  bool big;
  int splits, chunk, tiles;
};
static WgradPlan wgrad_plan(const avsep_conv_desc* d) {
  WgradPlan p;
  int M = d->Cout, Kc = d->Cin * d->KH * d->KW;
  long long P = (long long)d->N * d->Ho * d->Wo;
  p.big = M > 64 && Kc > 64;
  int bm = p.big ? 128 : 64;
  p.tiles = cdiv(M, bm) * cdiv(Kc, bm);
  int want = cdiv(1024, p.tiles);                       // aim for ~1024 workgroups
  long long maxs = (P + 255) / 256;                      // at least 256 pixels per split
  int splits = (int)((want < maxs) ? want : maxs);
  if (splits < 1) splits = 1;
  long long chunk = (P + splits - 1) / splits;
  chunk = (chunk + 31) / 32 * 32;
  p.chunk = (int)chunk;
  p.splits = (int)((P + chunk - 1) / chunk);
  return p;
}

// The buffer-load loader (igemm_kernel<..., BUF = true>) reaches a gathered tensor through 32-bit byte offsets: it serves a call
// whose gathered tensors (both sources of x; dY for the data gradient; all three for the weight gradient) each stay below the
// range with 16 bytes to spare, whose taps fit the loader's 31-bit tap mask and whose K is at least four tiles.  Everything
// else keeps the 64-bit global_load loader.
static inline bool igemm_src32(long long elems) { return 4 * elems + 16 < 0xfffffff0LL; }
static bool igemm_range32(const avsep_conv_desc* d, int mode) {
  const long long hw = (long long)d->H * d->W;
  const bool dy_fits = igemm_src32((long long)d->N * d->Cout * d->Ho * d->Wo);
  if (mode == 1) return dy_fits;
  return (mode == 0 || dy_fits) && igemm_src32((long long)d->N * d->C0 * hw) && igemm_src32((long long)d->N * (d->Cin - d->C0) * hw);
}
static bool igemm_buf32(const avsep_conv_desc* d, int mode) {
  if (d->up2x || d->KH * d->KW > 31) return false;
  // the loader's per-workgroup prologue (tap mask, the tables of two K-tiles, one more barrier) is paid back over the K-tiles:
  // with fewer than four of them (the Cin = 1 first conv has one) the call keeps the 64-bit loader
  const int s = d->stride;
  if (mode == 0 && d->Cin * d->KH * d->KW < 64) return false;
  if (mode == 1 && d->Cout * cdiv(d->KH, s) * cdiv(d->KW, s) < 64) return false;
  return igemm_range32(d, mode);
}

static size_t igemm_workspace_bytes(const avsep_conv_desc* d, int mode) {   // the split-K slabs
  const int S = mode == 0 ? fwd_split(d).splits : mode == 1 ? dgrad_split(d).splits : wgrad_plan(d).splits;
  if (S <= 1) return 0;
  if (mode == 0) return (size_t)S * d->N * d->Cout * d->Ho * d->Wo * sizeof(float);
  if (mode == 1) return (size_t)S * d->N * d->Cin * d->H * d->W * sizeof(float);
  return (size_t)S * d->Cout * d->Cin * d->KH * d->KW * sizeof(float);
}
static void igemm_variant(const avsep_conv_desc* d, int mode, char* buf, size_t cap) {
  if (mode == 0) snprintf(buf, cap, "BM%d,split%d", fwd_big(d) ? 128 : 64, fwd_split(d).splits);
  else if (mode == 1) snprintf(buf, cap, "BM%d,split%d", dgrad_big(d) ? 128 : 64, dgrad_split(d).splits);
  // "ld64": a gathered tensor is beyond the buffer-load loader's 32-bit range (no benched geometry comes near it).  The suffix
  // names the SIZE case only: a call with the fused upsample, more than 31 taps or fewer than four K-tiles also runs the 64-bit
  // loader, as it always did, and says nothing.  (`buf` arrives as an empty string: avsep_conv_kernel_variant.)
  if (!igemm_range32(d, mode)) {
    size_t n = strlen(buf);
    snprintf(buf + n, cap - n, "%sld64", n ? "," : "");
  }
}

static int igemm_fwd(const avsep_conv_desc* d, const float* w_packed, const float* bias, float* y, double* stats, void* workspace,
                     size_t workspace_bytes, hipStream_t st) {
  CArgs a = make_args(d);
  a.wp = w_packed; a.wp_ld = igemm_packed_ld(d, 0); a.out = y; a.bias = bias; a.stats = stats;
  a.M = d->Cout; a.K = d->Cin * d->KH * d->KW;
  long long ncols = (long long)d->N * d->Ho * d->Wo;
  if (ncols > 0x7fffffffLL) return AVSEP_ERR_ARG;
  a.Ncols = (int)ncols;
  SplitPlan sp = fwd_split(d);
  // too little workspace: unsplit.  Asked of the size the caller was told (both routes of the descriptor), not of this family's
  if (sp.splits > 1 && (!workspace || workspace_bytes < avsep_conv2d_fwd_workspace_bytes(d))) sp = SplitPlan{1, 0};
  if (sp.splits > 1) {
    a.kts = sp.kts;
    a.slab = (long long)d->N * d->Cout * d->Ho * d->Wo;
    a.out = (float*)workspace;
  }
  if (fwd_big(d)) {
    a.gridM = cdiv(a.M, 128);
    if (d->up2x) hipLaunchKernelGGL((igemm_kernel<M_FWD, 128, 128, 16, 2, 2, true>), dim3(a.gridM * cdiv(ncols, 128), sp.splits), dim3(256), 0, st, a);
    else if (igemm_buf32(d, 0)) hipLaunchKernelGGL((igemm_kernel<M_FWD, 128, 128, 16, 2, 2, false, true>), dim3(a.gridM * cdiv(ncols, 128), sp.splits), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_kernel<M_FWD, 128, 128, 16, 2, 2, false>), dim3(a.gridM * cdiv(ncols, 128), sp.splits), dim3(256), 0, st, a);
  } else {
    a.gridM = cdiv(a.M, 64);
    if (d->up2x) hipLaunchKernelGGL((igemm_kernel<M_FWD, 64, 64, 16, 2, 2, true>), dim3(a.gridM * cdiv(ncols, 64), sp.splits), dim3(256), 0, st, a);
    else if (igemm_buf32(d, 0)) hipLaunchKernelGGL((igemm_kernel<M_FWD, 64, 64, 16, 2, 2, false, true>), dim3(a.gridM * cdiv(ncols, 64), sp.splits), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_kernel<M_FWD, 64, 64, 16, 2, 2, false>), dim3(a.gridM * cdiv(ncols, 64), sp.splits), dim3(256), 0, st, a);
  }
  AVSEP_LAUNCH_CHECK();
  return sp.splits > 1 ? splitk_combine((const float*)workspace, a.slab, sp.splits, d, bias, y, stats, st) : AVSEP_OK;
}

static int igemm_dgrad(const avsep_conv_desc* d, const float* w_packed_dgrad, const float* dy, float* dx, const avsep_act_bwd*,
                       void* workspace, size_t workspace_bytes, hipStream_t st) {
  CArgs a = make_args(d);
  a.wp = w_packed_dgrad; a.wp_ld = igemm_packed_ld(d, 1); a.dy = dy; a.out = dx;
  a.M = d->Cin;
  const int s = d->stride;
  if (s != 1 && s != 2 && s != 4) return AVSEP_ERR_ARG;
  a.lstride = s == 1 ? 0 : (s == 2 ? 1 : 2);
  long long ncols = (long long)d->N * cdiv(d->H, s) * cdiv(d->W, s);  // largest parity class
  if ((long long)d->N * d->H * d->W > 0x7fffffffLL) return AVSEP_ERR_ARG;
  SplitPlan sp = dgrad_split(d);
  if (sp.splits > 1 && (!workspace || workspace_bytes < igemm_workspace_bytes(d, 1))) sp = SplitPlan{1, 0};
  if (sp.splits > 1) {
    a.kts = sp.kts;
    a.slab = (long long)d->N * d->Cin * d->H * d->W;
    a.out = (float*)workspace;
  }
  if (dgrad_big(d)) {
    a.gridM = cdiv(a.M, 128);
    const dim3 grid(a.gridM * cdiv(ncols, 128), s * s, sp.splits);
    if (igemm_buf32(d, 1)) hipLaunchKernelGGL((igemm_kernel<M_DGRAD, 128, 128, 16, 2, 2, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_kernel<M_DGRAD, 128, 128, 16, 2, 2>), grid, dim3(256), 0, st, a);
  } else {
    a.gridM = cdiv(a.M, 64);
    const dim3 grid(a.gridM * cdiv(ncols, 64), s * s, sp.splits);
    if (igemm_buf32(d, 1)) hipLaunchKernelGGL((igemm_kernel<M_DGRAD, 64, 64, 16, 2, 2, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_kernel<M_DGRAD, 64, 64, 16, 2, 2>), grid, dim3(256), 0, st, a);
  }
  AVSEP_LAUNCH_CHECK();
  if (sp.splits > 1) {
    hipLaunchKernelGGL(reduce_slabs_kernel<64>, dim3(cdiv(a.slab, 64)), dim3(256), 0, st, (const float*)workspace, dx, a.slab,
                       sp.splits, a.slab);
    AVSEP_LAUNCH_CHECK();
  }
  return AVSEP_OK;
}

static int igemm_wgrad(const avsep_conv_desc* d, const float* dy, float* dw, float*, float* ws, hipStream_t st) {
  WgradPlan p = wgrad_plan(d);
  CArgs a = make_args(d);
  a.dy = dy;
  a.M = d->Cout; a.Ncols = d->Cin * d->KH * d->KW; a.K = 0;
  long long P = (long long)d->N * d->Ho * d->Wo;
  if (P > 0x7fffffffLL) return AVSEP_ERR_ARG;
  a.P = (int)P; a.chunk = p.chunk;
  a.out = (p.splits > 1) ? ws : dw;
  if (p.big) {
    a.gridM = cdiv(a.M, 128);
    if (d->up2x) hipLaunchKernelGGL((igemm_kernel<M_WGRAD, 128, 128, 32, 2, 2, true>), dim3(a.gridM * cdiv(a.Ncols, 128), p.splits), dim3(256), 0, st, a);
    else if (igemm_buf32(d, 2)) hipLaunchKernelGGL((igemm_kernel<M_WGRAD, 128, 128, 32, 2, 2, false, true>), dim3(a.gridM * cdiv(a.Ncols, 128), p.splits), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_kernel<M_WGRAD, 128, 128, 32, 2, 2, false>), dim3(a.gridM * cdiv(a.Ncols, 128), p.splits), dim3(256), 0, st, a);
  } else {
    a.gridM = cdiv(a.M, 64);
    if (d->up2x) hipLaunchKernelGGL((igemm_kernel<M_WGRAD, 64, 64, 32, 2, 2, true>), dim3(a.gridM * cdiv(a.Ncols, 64), p.splits), dim3(256), 0, st, a);
    else if (igemm_buf32(d, 2)) hipLaunchKernelGGL((igemm_kernel<M_WGRAD, 64, 64, 32, 2, 2, false, true>), dim3(a.gridM * cdiv(a.Ncols, 64), p.splits), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((igemm_kernel<M_WGRAD, 64, 64, 32, 2, 2, false>), dim3(a.gridM * cdiv(a.Ncols, 64), p.splits), dim3(256), 0, st, a);
  }
  AVSEP_LAUNCH_CHECK();
  if (p.splits > 1) {
    long long n = (long long)a.M * a.Ncols;
    hipLaunchKernelGGL(reduce_slabs_kernel<64>, dim3(cdiv(n, 64)), dim3(256), 0, st, (const float*)ws, dw, n, p.splits, n);
    AVSEP_LAUNCH_CHECK();
  }
  return AVSEP_OK;
}

// ---------------------------------------------------------------------------
// routes: which family serves a call.  The three tables below are the ONLY place where the order of the families exists:
// the first applicable entry of the mode's table launches the call, and every query about the call (formats, packed image,
// workspace, name, variant) reads the slots of that same entry.
// ---------------------------------------------------------------------------
enum ConvFamily { /* forward, data gradient: */ SMALLCO, HEAD, SMALLCI, BF, W4, WN, C3, C4, CM, IGEMM,
                  /* weight gradient:        */ G_SMALLCO, G_HEAD, G_WBN, G_X4, G_WW, G_W4D, G_W3, G_SCW, G_IGEMM };
struct ConvEntry {
  ConvFamily fam, image;     // image: the family whose packed weight image the launch reads
  bool stats_free;           // serves forward calls without BatchNorm statistics only
  const char* name;
  conv_applicable_fn* applicable;
  conv_workspace_fn* workspace;
  conv_variant_fn* variant;
  conv_packed_floats_fn* packed_floats;
  conv_pack_fn* pack;
  conv_fwd_fn* fwd;          // the launch slot: the one of the table's mode is set
  conv_dgrad_fn* dgrad;
  conv_wgrad_fn* wgrad;
};
// slots a family leaves empty
#define NO_WORKSPACE(p) static size_t p##_workspace_bytes(const avsep_conv_desc*, int) { return 0; }
#define NO_VARIANT(p) static void p##_variant(const avsep_conv_desc*, int, char*, size_t) {}
NO_WORKSPACE(smallci) NO_WORKSPACE(w4) NO_WORKSPACE(wn) NO_WORKSPACE(c3) NO_WORKSPACE(c4) NO_WORKSPACE(cm)
NO_VARIANT(smallco) NO_VARIANT(head) NO_VARIANT(smallci) NO_VARIANT(wn) NO_VARIANT(ww) NO_VARIANT(w4d) NO_VARIANT(w3) NO_VARIANT(scw)
// an entry takes every slot from ONE prefix
#define SLOTS(p) p##_applicable, p##_workspace_bytes, p##_variant
#define FWD(F, p, name) {F, F, false, name, SLOTS(p), p##_packed_floats, p##_pack, p##_fwd, nullptr, nullptr}
// the few-output-channel forward kernels read the im2col family's [k][Cout] image and leave statistics to the other route
#define FWD_STATS_FREE(F, p, name) {F, IGEMM, true, name, SLOTS(p), nullptr, nullptr, p##_fwd, nullptr, nullptr}
#define DGRAD(F, p, name) {F, F, false, name, SLOTS(p), p##_packed_floats, p##_pack, nullptr, p##_dgrad, nullptr}
#define WGRAD(F, p, name) {F, F, false, name, SLOTS(p), nullptr, nullptr, nullptr, nullptr, p##_wgrad}
static const ConvEntry FWD_TABLE[] = {
    FWD_STATS_FREE(SMALLCO, smallco, "smallco_fwd"), FWD_STATS_FREE(HEAD, head, "head_fwd_kernel"),
    FWD(BF, bf, "convbf_kernel"), FWD(W4, w4, "wino4_kernel"), FWD(WN, wn, "wino_kernel"), FWD(C3, c3, "conv3x3_kernel"),
    FWD(C4, c4, "conv3x3_kernel"), FWD(CM, cm, "conv3x3_kernel"), FWD(IGEMM, igemm, "igemm_kernel<fwd>")};
static const ConvEntry DGRAD_TABLE[] = {
    DGRAD(SMALLCI, smallci, "smallci_dgrad"), DGRAD(BF, bf, "convbf_kernel"), DGRAD(W4, w4, "wino4_kernel"),
    DGRAD(WN, wn, "wino_kernel"), DGRAD(C3, c3, "conv3x3_kernel"), DGRAD(C4, c4, "conv3x3_kernel"),
    DGRAD(CM, cm, "conv3x3_kernel"), DGRAD(IGEMM, igemm, "igemm_kernel<dgrad>")};
static const ConvEntry WGRAD_TABLE[] = {
    WGRAD(G_SMALLCO, smallco, "smallco_wgrad"), WGRAD(G_HEAD, head, "head_wgrad_kernel"), WGRAD(G_WBN, wbn, "wgradb_kernel"),
    WGRAD(G_X4, x4, "winow4_kernel"), WGRAD(G_WW, ww, "winow_kernel"), WGRAD(G_W4D, w4d, "wgrad4d_kernel"),
    WGRAD(G_W3, w3, "wgrad3x3_kernel"), WGRAD(G_SCW, scw, "smallci_wgrad_kernel"), WGRAD(G_IGEMM, igemm, "igemm_kernel<wgrad>")};

struct ConvRoute { const ConvEntry* run; const ConvEntry* pack; };   // the entry that launches; the entry whose weight image it reads
// The route of a call of `mode` over a valid descriptor.  A forward descriptor has two routes, with and without statistics,
// and ONE packed weight image: AVSEP_ERR_ARG if the two would not read the same image.
static int conv_route(const avsep_conv_desc* d, int mode, bool with_stats, ConvRoute* r) {
  const ConvEntry* table = mode == 0 ? FWD_TABLE : mode == 1 ? DGRAD_TABLE : WGRAD_TABLE;
  const ConvEntry* e = table;
  while (!e->applicable(d, mode)) ++e;          // ends at the im2col entry at the latest
  const ConvEntry* s = e;                        // the same walk past the entries that take no statistics
  while (s->stats_free) do ++s; while (!s->applicable(d, mode));
  if (s->image != e->image) return AVSEP_ERR_ARG;
  r->run = with_stats ? s : e;
  for (r->pack = table; r->pack->fam != r->run->image;) ++r->pack;
  return AVSEP_OK;
}

extern "C" int avsep_conv_io_formats(const avsep_conv_desc* d, int32_t mode, int32_t* in_fmt, int32_t* out_b16) {
  if (!in_fmt || !out_b16 || mode < 0 || mode > 2) return AVSEP_ERR_ARG;
  int rc = check_desc(d, mode == 0);
  ConvRoute r;
  if (rc || (rc = conv_route(d, mode, false, &r))) return rc;
  *in_fmt = (r.run->fam == BF || r.run->fam == G_WBN) ? AVSEP_FMT_B16 : AVSEP_FMT_F32;
  *out_b16 = r.run->fam == BF ? bf_out_b16(d, mode) : 0;
  return AVSEP_OK;
}

extern "C" size_t avsep_conv_packed_floats(const avsep_conv_desc* d, int mode) {
  ConvRoute r;
  if (!d || (mode != 0 && mode != 1) || conv_route(d, mode, true, &r)) return 0;
  return r.pack->packed_floats(d, mode);
}

extern "C" int avsep_conv_pack_weights(const avsep_conv_desc* d, const float* w, float* packed, int mode,
                                       avsep_stream_t stream) {
  if (!d || !w || !packed || (mode != 0 && mode != 1)) return AVSEP_ERR_ARG;
  ConvRoute r;
  int rc = conv_route(d, mode, true, &r);
  return rc ? rc : r.pack->pack(d, w, packed, mode, (hipStream_t)stream);
}

// the workspace of the run entry of a call; 0 for a descriptor no call accepts
static size_t route_workspace(const avsep_conv_desc* d, int mode, bool with_stats) {
  ConvRoute r;
  return (check_desc(d, mode == 0) || conv_route(d, mode, with_stats, &r)) ? 0 : r.run->workspace(d, mode);
}
extern "C" size_t avsep_conv2d_fwd_workspace_bytes(const avsep_conv_desc* d) {   // covers both routes of the descriptor
  return max(route_workspace(d, 0, true), route_workspace(d, 0, false));
}
extern "C" size_t avsep_conv2d_dgrad_workspace_bytes(const avsep_conv_desc* d) { return route_workspace(d, 1, false); }
extern "C" size_t avsep_conv2d_wgrad_workspace_bytes(const avsep_conv_desc* d) { return route_workspace(d, 2, false); }

extern "C" int avsep_conv2d_fwd(const avsep_conv_desc* d, const float* w_packed, const float* bias, float* y,
                                double* stats, void* workspace, size_t workspace_bytes, avsep_stream_t stream) {
  int rc = check_desc(d, true);
  if (rc) return rc;
  if (!w_packed || !y) return AVSEP_ERR_ARG;
  ConvRoute r;
  if ((rc = conv_route(d, 0, stats != nullptr, &r))) return rc;
  return r.run->fwd(d, w_packed, bias, y, stats, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int avsep_conv2d_dgrad(const avsep_conv_desc* d, const float* w_packed_dgrad, const float* dy, float* dx,
                                  void* workspace, size_t workspace_bytes, avsep_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!w_packed_dgrad || !dy || !dx) return AVSEP_ERR_ARG;
  ConvRoute r;
  if ((rc = conv_route(d, 1, false, &r))) return rc;
  return r.run->dgrad(d, w_packed_dgrad, dy, dx, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

// the data gradient through the activation in front of the conv's input (include/avsep.h): in the F(4x4) Winograd kernel's
// epilogue, else as the two launches it stands for
extern "C" int32_t avsep_conv2d_dgrad_act_fused(const avsep_conv_desc* d) {
  ConvRoute r;
  return (!check_desc(d) && !conv_route(d, 1, false, &r) && r.run->fam == W4) ? 1 : 0;
}
extern "C" int avsep_conv2d_dgrad_act(const avsep_conv_desc* d, const float* w_packed_dgrad, const float* dy,
                                      const avsep_act_bwd* e, float* dx, void* workspace, size_t workspace_bytes,
                                      avsep_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!w_packed_dgrad || !dy || !dx || !e || !e->y) return AVSEP_ERR_ARG;
  if (d->dxfmt != AVSEP_FMT_F32) return AVSEP_ERR_ARG;
  if ((e->scale == nullptr) != (e->shift == nullptr) || (e->res_scale == nullptr) != (e->res_shift == nullptr) ||
      (e->res_scale && !e->residual) || (e->bstats && (!e->mean || !e->invstd)))
    return AVSEP_ERR_ARG;
  if (e->act != AVSEP_ACT_NONE && e->act != AVSEP_ACT_RELU && e->act != AVSEP_ACT_LRELU02) return AVSEP_ERR_ARG;
  ConvRoute r;
  if ((rc = conv_route(d, 1, false, &r))) return rc;
  if (r.run->fam == W4) return r.run->dgrad(d, w_packed_dgrad, dy, dx, e, workspace, workspace_bytes, (hipStream_t)stream);
  rc = avsep_conv2d_dgrad(d, w_packed_dgrad, dy, dx, workspace, workspace_bytes, stream);
  if (rc) return rc;
  return avsep_affine_act_bwd(dx, e->dz2, e->y, e->scale, e->shift, e->residual, e->res_scale, e->res_shift, e->add, e->mean,
                              e->invstd, e->act, d->N, d->Cin, d->H * d->W, dx, e->bstats, stream);
}

extern "C" int avsep_conv2d_wgrad(const avsep_conv_desc* d, const float* dy, float* dw, float* dbias, void* workspace,
                                  size_t workspace_bytes, avsep_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!dy || !dw) return AVSEP_ERR_ARG;
  ConvRoute r;
  if ((rc = conv_route(d, 2, false, &r))) return rc;
  const ConvFamily fam = r.run->fam;
  const size_t need = r.run->workspace(d, 2);
  if (need > workspace_bytes || (need && !workspace)) return AVSEP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  rc = r.run->wgrad(d, dy, dw, dbias, (float*)workspace, st);
  if (rc || !dbias || fam == G_SMALLCO || fam == G_HEAD) return rc;   // those two sum dbias themselves
  if (fam == G_WBN)   // dy is a B16 image; the accumulators are the last 2 * Cout doubles of the family's workspace
    return b16_channel_sum(dy, d->N, d->Cout, d->Ho * d->Wo, (double*)((char*)workspace + need) - 2 * d->Cout, dbias, st);
  hipLaunchKernelGGL(channel_sum_kernel, dim3(d->Cout), dim3(256), 0, st, dy, d->N, d->Cout, d->Ho * d->Wo, dbias);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// the name a call is reported under, and its entry (null where no slot of the tables stands behind the name)
static const char* reported_name(const avsep_conv_desc* d, int mode, bool with_stats, const ConvEntry** run) {
  ConvRoute r;
  *run = nullptr;
  if (check_desc(d, mode == 0) || conv_route(d, mode, with_stats, &r)) return "invalid";
  // a head descriptor's data gradient is the separate entry point avsep_conv2d_dgrad_up2x; callers read its kernel's name here
  if (mode == 1 && head_applicable(d, mode)) return "head_dgrad_kernel";
  *run = r.run;
  return r.run->name;
}
extern "C" const char* avsep_conv_kernel_name(const avsep_conv_desc* d, int32_t mode, int32_t with_stats) {
  const ConvEntry* run;
  return reported_name(d, mode, with_stats != 0, &run);
}
extern "C" int avsep_conv_kernel_variant(const avsep_conv_desc* d, int32_t mode, int32_t with_stats, char* buf, size_t cap) {
  if (!buf || cap < 8) return AVSEP_ERR_ARG;
  const ConvEntry* run;
  const char* fam = reported_name(d, mode, with_stats != 0, &run);
  char tail[64] = "";
  if (run) run->variant(d, mode, tail, sizeof(tail));
  snprintf(buf, cap, tail[0] ? "%s:%s" : "%s", fam, tail);
  return AVSEP_OK;
}

// ---------------------------------------------------------------------------
// fused decoder head (head_gemm.hip): dgrad of a conv over the virtual up2x(relu(affine(cat))) input, taken straight to
// the two low-res sources
// ---------------------------------------------------------------------------
extern "C" int32_t avsep_conv2d_head_applicable(const avsep_conv_desc* d) {
  return (check_desc(d) == AVSEP_OK && head_applicable(d, 1)) ? 1 : 0;
}
extern "C" size_t avsep_conv2d_dgrad_up2x_workspace_bytes(const avsep_conv_desc* d) {
  return (check_desc(d) == AVSEP_OK && head_applicable(d, 1)) ? head_dgrad_workspace_floats(d) * sizeof(float) : 0;
}
extern "C" int avsep_conv2d_dgrad_up2x(const avsep_conv_desc* d, const float* w, const float* dy, float* g0, float* g1,
                                       const float* mean1, const float* invstd1, double* bstats1, int32_t acc0,
                                       void* workspace, size_t workspace_bytes, avsep_stream_t stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (!w || !dy || (!g0 && !g1)) return AVSEP_ERR_ARG;
  if (bstats1 && (!mean1 || !invstd1 || !g1)) return AVSEP_ERR_ARG;
  if (!head_applicable(d, 1)) return AVSEP_ERR_ARG;   // unsupported geometry: use avsep_conv2d_dgrad + avsep_relu_up2x_bwd
  if (!workspace || workspace_bytes < head_dgrad_workspace_floats(d) * sizeof(float)) return AVSEP_ERR_WORKSPACE;
  return head_dgrad(d, w, dy, g0, g1, mean1, invstd1, bstats1, acc0, (float*)workspace, (hipStream_t)stream);
}
