// A feathered matte from a label map (include/ppst_hip.h: ppst_label_matte): the exact, clipped, signed Euclidean distance
// transform of "label kept", then a smoothstep.  Everything that decides something is an integer; only the last step is fp32.
//
// A pixel is INSIDE iff its label L < 32 and bit L of ``keep`` is set.  D2(p) = min(R^2, min |p - q|^2) over the pixels q of the
// plane whose inside-ness differs from p's; sd2 = + D2 inside, - D2 outside.  The squared distance separates:
// |p - q|^2 = dx^2 + dy^2, so min over q = min over columns x + dx of dx^2 + g(x + dx)^2 with g the VERTICAL distance to the nearest
// pixel of the opposite class in that column.
//   columns   for every pixel the vertical distance, clipped to R, to the nearest outside pixel and to the nearest inside pixel
//             of its column (0 for the class the pixel itself has), packed as two 16-bit halves of the sd2 word (outside: low,
//             inside: high; R <= 256 fits).  One thread per column segment of MT_SEG rows: a sweep down from R rows above the
//             segment that writes the segment's words, a sweep up from R rows below it that takes the minimum with the thread's
//             own words; neighbouring threads read neighbouring columns.  A pixel farther than R is as good as none: its word says R either way.
//   rows      a block stages one whole row of packed words in LDS (w <= 4096: 16 KB) and only then writes the row in place.  A
//             thread takes min(dx^2 + g(x +- dx)^2) outwards from dx = 0 over the halves of the class OPPOSITE to its own pixel's,
//             and stops once dx^2 >= best: no farther column can improve it.  best starts at R^2, so at most R steps.  MT_ROW
//             threads a block loop over wider rows.
// Clipping never changes the matte.  With R = max(grow, max(feather - grow, 0)) + 1 and sd = +-(sqrt(D2) - 1/2): an inside pixel
// with D2 >= R^2 has sd + grow >= R - 1/2 + grow >= feather + 1/2, so t = clamp((sd + grow) / feather, 0, 1) = 1 at any true
// distance (feather == 0: sd + grow > 0, m = 1); an outside pixel with D2 >= R^2 has sd + grow <= -(R - 1/2) + grow <= -1/2, so
// t = 0 and m = 0 (feather == 0: not > 0, m = 0).
#include "common.h"
#include <math.h>

#define MT_SEG 32
#define MT_ROW 256
#define MT_COLS 64                                  // threads (columns) of a block of the column launch
#define MT_MAX 4096

namespace {

__device__ __forceinline__ bool mt_inside(unsigned L, unsigned keep) { return L < 32u && ((keep >> L) & 1u); }

__global__ __launch_bounds__(MT_COLS) void mt_cols_kernel(const unsigned char* __restrict__ lab, int B, int h, int w, unsigned keep,
                                                          int R, unsigned* __restrict__ pk2) {
  const int x = blockIdx.x * MT_COLS + threadIdx.x, y0 = blockIdx.y * MT_SEG;
  if (x >= w) return;                                                           // (no barrier in this kernel)
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    const unsigned char* L = lab + (int64_t)b * h * w + x;
    unsigned* o = pk2 + (int64_t)b * h * w + x;
    int dO = R, dI = R;                                                         // to the nearest outside / inside pixel at or above
    auto step = [&](unsigned l) {
      const bool in = mt_inside(l, keep);
      dO = in ? min(dO + 1, R) : 0;
      dI = in ? 0 : min(dI + 1, R);
    };
    const int ya = max(y0 - R, 0), yb = min(y0 + MT_SEG - 1 + R, h - 1), ye = min(y0 + MT_SEG - 1, h - 1);
    const unsigned char* p = L + (int64_t)ya * w;                               // (running pointers: one 64-bit add a row)
    for (int y = ya; y < y0; ++y, p += w) step(*p);
    unsigned* q = o + (int64_t)y0 * w;
    for (int y = y0; y <= ye; ++y, p += w, q += w) { step(*p); *q = (unsigned)dO | ((unsigned)dI << 16); }
    dO = R; dI = R;                                                             // ... at or below
    p = L + (int64_t)yb * w;
    for (int y = yb; y > ye; --y, p -= w) step(*p);
    q = o + (int64_t)ye * w;                                                    // (p is at row ye: yb == ye, or the sweep ended there)
    for (int y = ye; y >= y0; --y, p -= w, q -= w) {
      step(*p);
      const unsigned dn = *q;                                                   // this thread's own word of the sweep down
      *q = min(dn & 0xffffu, (unsigned)dO) | (min(dn >> 16, (unsigned)dI) << 16);
    }
  }
}

__global__ __launch_bounds__(MT_ROW) void mt_rows_kernel(int64_t rows, int w, int R, int feather, int grow, int* sd2,
                                                         float* __restrict__ matte) {
  __shared__ unsigned row[MT_MAX];
  const int t = threadIdx.x;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    int* g = sd2 + r * w;
    for (int x = t; x < w; x += MT_ROW) row[x] = (unsigned)g[x];
    __syncthreads();
    for (int x = t; x < w; x += MT_ROW) {
      const bool in = (row[x] & 0xffffu) != 0;                                  // not at distance 0 from an outside pixel
      const int sh = in ? 0 : 16;                                               // the half of the opposite class
      int best = R * R;
      for (int dx = 0; dx * dx < best; ++dx) {
        if (x + dx < w) { const int d = (int)((row[x + dx] >> sh) & 0xffffu); best = min(best, dx * dx + d * d); }
        if (x - dx >= 0) { const int d = (int)((row[x - dx] >> sh) & 0xffffu); best = min(best, dx * dx + d * d); }
      }
      g[x] = in ? best : -best;
      if (matte) {
        const float s = sqrtf((float)best) - 0.5f, u = (in ? s : -s) + (float)grow;
        float m;
        if (feather > 0) {
          const float tt = fminf(fmaxf(u / (float)feather, 0.f), 1.f);
          m = tt * tt * (3.f - 2.f * tt);
        } else {
          m = u > 0.f ? 1.f : 0.f;
        }
        matte[r * w + x] = m;
      }
    }
    __syncthreads();                                                            // (the next row's staging overwrites row)
  }
}

}  // namespace

extern "C" int ppst_label_matte(const void* labels_u8, int B, int h, int w, unsigned int keep, int feather, int grow, void* sd2_i32,
                                void* matte_f32, void* stream) {
  if (B < 0 || h < 1 || h > MT_MAX || w < 1 || w > MT_MAX || feather < 0 || feather > 255 || grow < 0 || grow > 255) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!labels_u8 || !sd2_i32) return PPST_ENULL;
  const int fg = feather - grow, R = (grow > fg ? grow : (fg > 0 ? fg : 0)) + 1;
  PPST_LAUNCH(mt_cols_kernel, dim3((unsigned)cdiv(w, MT_COLS), (unsigned)cdiv(h, MT_SEG), (unsigned)(B > 65535 ? 65535 : B)), dim3(MT_COLS),
              0, as_stream(stream), (const unsigned char*)labels_u8, B, h, w, keep, R, (unsigned*)sd2_i32);
  int rc = PPST_LAUNCH_CHECK();
  if (rc) return rc;
  const int64_t rows = (int64_t)B * h;
  PPST_LAUNCH(mt_rows_kernel, dim3((unsigned)(rows > (1 << 20) ? (1 << 20) : rows)), dim3(MT_ROW), 0, as_stream(stream), rows, w, R,
              feather, grow, (int*)sd2_i32, (float*)matte_f32);
  return PPST_LAUNCH_CHECK();
}
