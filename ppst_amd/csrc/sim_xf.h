// The similarity transform of a crop inside a photograph, in integers (include/ppst_hip.h: ppst_extract_similarity).  Shared by
// the crop kernel (imageio.hip) and the paste kernel (guided_filter.hip), host and device.
//   U =  a (2X + 1) + b (2Y + 1) + cu,   V = -b (2X + 1) + a (2Y + 1) + cv     units of 2^-24 crop pixel
// and back, with D = a^2 + b^2 and (px, py) = (2X + 1, 2Y + 1):  px = (a (U - cu) - b (V - cv)) / D,  py = (b (U - cu) + a (V - cv)) / D.
#pragma once
#include <stdint.h>

#define SX_ONE ((int64_t)1 << 24)        // one crop pixel
#define SX_HALF ((int64_t)1 << 23)
#define SX_NMAX 4096
#define SX_MAXPIX ((int64_t)1 << 28)
#define SX_CMAX ((int64_t)1 << 56)

__host__ __device__ inline int64_t sx_min(int64_t x, int64_t y) { return x < y ? x : y; }
__host__ __device__ inline int64_t sx_max(int64_t x, int64_t y) { return x > y ? x : y; }

struct SimXf { int64_t a, b, cu, cv; };

// 1 <= s <= 8, offsets that cannot overflow: a^2 + b^2 in [2^40, 2^46] (so |a|, |b| <= 2^23)
__host__ __device__ inline bool sx_rule(const SimXf& t) {
  const int64_t m = (int64_t)1 << 23;
  if (t.a < -m || t.a > m || t.b < -m || t.b > m) return false;
  const int64_t D = t.a * t.a + t.b * t.b;
  if (D < ((int64_t)1 << 40) || D > ((int64_t)1 << 46)) return false;
  return t.cu >= -SX_CMAX && t.cu <= SX_CMAX && t.cv >= -SX_CMAX && t.cv <= SX_CMAX;
}

// Pixel box [x0, x1] x [y0, y1] (not clipped to any image) that holds every integer pixel whose centre maps into the crop-frame
// rectangle [Ulo, Uhi] x [Vlo, Vhi], grown by ``margin`` pixels a side.  The corners are mapped back in double, through one
// reciprocal of D (error far below a
// pixel at every accepted transform); margin >= 1 covers it.  Results are limited to +-2^30.
__host__ __device__ inline void sx_box(const SimXf& t, int64_t Ulo, int64_t Uhi, int64_t Vlo, int64_t Vhi, int margin,
                                       int& x0, int& y0, int& x1, int& y1) {
  const double inv = 1.0 / (double)(t.a * t.a + t.b * t.b), a = (double)t.a, b = (double)t.b;
  double pxl = 1e300, pxh = -1e300, pyl = 1e300, pyh = -1e300;
  for (int k = 0; k < 4; ++k) {
    const double dU = (double)(((k & 1) ? Uhi : Ulo) - t.cu), dV = (double)(((k & 2) ? Vhi : Vlo) - t.cv);
    const double px = (a * dU - b * dV) * inv, py = (b * dU + a * dV) * inv;
    pxl = px < pxl ? px : pxl; pxh = px > pxh ? px : pxh;
    pyl = py < pyl ? py : pyl; pyh = py > pyh ? py : pyh;
  }
  const double lim = 1073741824.0;
  auto lo = [&](double p) { double v = floor((p - 1.0) * 0.5) - margin; return (int)(v < -lim ? -lim : (v > lim ? lim : v)); };
  auto hi = [&](double p) { double v = ceil((p - 1.0) * 0.5) + margin; return (int)(v < -lim ? -lim : (v > lim ? lim : v)); };
  x0 = lo(pxl); x1 = hi(pxh); y0 = lo(pyl); y1 = hi(pyh);
}
