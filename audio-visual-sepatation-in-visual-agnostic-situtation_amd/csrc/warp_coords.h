// Coordinates of the reference's log-frequency warp (utils.py:12-26 warpgrid) and of
// F.grid_sample(bilinear, zeros, align_corners=False) on it: shared by ops.hip (prepare / warp) and longform.hip
// (window prepare / mask stitch), which must agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// numpy.linspace(-1, 1, n)[i] in float64
__device__ __forceinline__ double linspace_pm1(int i, int n) {
  if (n == 1) return -1.0;
  if (i == n - 1) return 1.0;
  return -1.0 + (double)i * (2.0 / (double)(n - 1));
}
// y coordinate of utils.py:warpgrid in float64, cast to fp32 like grid.astype(np.float32)
__device__ __forceinline__ float warp_gy(int f, int Fout, int warp) {
  double yv = linspace_pm1(f, Fout);
  double gy = warp ? (pow(21.0, (yv + 1.0) / 2.0) - 11.0) / 10.0 : log(yv * 10.0 + 11.0) / log(21.0) * 2.0 - 1.0;
  return (float)gy;
}

struct Bilin {
  int y0, x0;
  float wnw, wne, wsw, wse;
};
// F.grid_sample(bilinear, zeros, align_corners=False) coordinates for one output location
__device__ __forceinline__ Bilin grid_bilin(float gx, float gy, int Hin, int Win) {
  float ix = ((gx + 1.f) * (float)Win - 1.f) / 2.f;
  float iy = ((gy + 1.f) * (float)Hin - 1.f) / 2.f;
  float fx = floorf(ix), fy = floorf(iy);
  Bilin b;
  b.x0 = (int)fx;
  b.y0 = (int)fy;
  float ex = fx + 1.f - ix, ey = fy + 1.f - iy;  // distance to the east / south neighbour
  float wx = ix - fx, wy = iy - fy;
  b.wnw = ex * ey;
  b.wne = wx * ey;
  b.wsw = ex * wy;
  b.wse = wx * wy;
  return b;
}
__device__ __forceinline__ float sample_bilin(const float* __restrict__ p, const Bilin& b, int Hin, int Win,
                                              float eps) {
  float v = 0.f;
  bool y0 = (unsigned)b.y0 < (unsigned)Hin, y1 = (unsigned)(b.y0 + 1) < (unsigned)Hin;
  bool x0 = (unsigned)b.x0 < (unsigned)Win, x1 = (unsigned)(b.x0 + 1) < (unsigned)Win;
  if (y0 && x0) v += (p[b.y0 * Win + b.x0] + eps) * b.wnw;
  if (y0 && x1) v += (p[b.y0 * Win + b.x0 + 1] + eps) * b.wne;
  if (y1 && x0) v += (p[(b.y0 + 1) * Win + b.x0] + eps) * b.wsw;
  if (y1 && x1) v += (p[(b.y0 + 1) * Win + b.x0 + 1] + eps) * b.wse;
  return v;
}
