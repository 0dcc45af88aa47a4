// sRGB bytes <-> CIELAB in fp32, stated once for colour_stats.hip (forward) and colour_transfer.hip (forward and inverse); the
// definition is in include/ppst_hip.h ("colour statistics", "colour transfer").
//   forward   channel c -> lin(c) by a 256-entry table built in float64 and rounded once; (X/Xn, Y/Yn, Z/Zn) = M lin with M the
//             sRGB (D65) rows divided by the white point in float64, rounded once; f = cbrt above (6/29)^3, else the linear
//             branch; L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z))
//   inverse   fy = (L + 16) / 116, fx = fy + a / 500, fz = fy - b / 200; t = f^3 above 6/29, else (f - 4/29) * 108/841; linear
//             RGB = Minv t with Minv the float64 inverse of the float64 M, rounded once; clamp to [0, 1]; the sRGB transfer curve
//             (12.92 c up to 0.0031308, else 1.055 c^(1/2.4) - 0.055); rint(255 s)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

struct CsMat { float m[3][3]; };
struct CsLab { float L, a, b; };

__device__ __forceinline__ float cs_f(float t) {
  return t > 0.008856451679035631f ? cbrtf(t) : fmaf(t, 7.787037037037037f, 0.13793103448275862f);
}
// (every multiply-add is an explicit fma: the pivot and the pixels go through the same arithmetic wherever this is inlined)
__device__ __forceinline__ CsLab cs_lab(const float* __restrict__ tab, const CsMat& M, unsigned r, unsigned g, unsigned b) {
  const float lr = tab[r], lg = tab[g], lb = tab[b];
  const float fx = cs_f(fmaf(M.m[0][0], lr, fmaf(M.m[0][1], lg, M.m[0][2] * lb)));
  const float fy = cs_f(fmaf(M.m[1][0], lr, fmaf(M.m[1][1], lg, M.m[1][2] * lb)));
  const float fz = cs_f(fmaf(M.m[2][0], lr, fmaf(M.m[2][1], lg, M.m[2][2] * lb)));
  CsLab o;
  o.L = fmaf(116.f, fy, -16.f);
  o.a = 500.f * (fx - fy);
  o.b = 200.f * (fy - fz);
  return o;
}

__device__ __forceinline__ float cs_finv(float f) {
  return f > 0.20689655172413793f ? f * f * f : (f - 0.13793103448275862f) * 0.12841854934601665f;
}
__device__ __forceinline__ unsigned cs_srgb_byte(float c) {
  c = fminf(fmaxf(c, 0.f), 1.f);
  const float s = c <= 0.0031308f ? 12.92f * c : fmaf(1.055f, powf(c, 0.4166666666666667f), -0.055f);
  return (unsigned)rintf(255.f * s);
}
// -> r | g << 8 | b << 16
__device__ __forceinline__ unsigned cs_lab_to_rgb(const CsMat& Mi, float L, float a, float b) {
  const float fy = (L + 16.f) / 116.f;
  const float tx = cs_finv(fy + a / 500.f), ty = cs_finv(fy), tz = cs_finv(fy - b / 200.f);
  const float r = fmaf(Mi.m[0][0], tx, fmaf(Mi.m[0][1], ty, Mi.m[0][2] * tz));
  const float g = fmaf(Mi.m[1][0], tx, fmaf(Mi.m[1][1], ty, Mi.m[1][2] * tz));
  const float bl = fmaf(Mi.m[2][0], tx, fmaf(Mi.m[2][1], ty, Mi.m[2][2] * tz));
  return cs_srgb_byte(r) | (cs_srgb_byte(g) << 8) | (cs_srgb_byte(bl) << 16);
}

// ---- the constants, on the host
inline void cs_srgb_table(float* tab) {
  for (int i = 0; i < 256; ++i) {
    const double c = i / 255.0;
    tab[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
  }
}
inline void cs_lab_matrix64(double m[3][3]) {
  static const double XYZ[3][3] = {{0.4124564, 0.3575761, 0.1804375}, {0.2126729, 0.7151522, 0.0721750}, {0.0193339, 0.1191920, 0.9503041}};
  static const double WHITE[3] = {0.95047, 1.0, 1.08883};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m[r][c] = XYZ[r][c] / WHITE[r];
}
inline CsMat cs_lab_matrix() {
  double m[3][3];
  cs_lab_matrix64(m);
  CsMat M;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M.m[r][c] = (float)m[r][c];
  return M;
}
inline CsMat cs_lab_inverse_matrix() {                       // the adjugate over the determinant, float64
  double m[3][3];
  cs_lab_matrix64(m);
  const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                     m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
  CsMat I;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
      I.m[r][c] = (float)((m[r1][c1] * m[r2][c2] - m[r1][c2] * m[r2][c1]) / det);
    }
  return I;
}
