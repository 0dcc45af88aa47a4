// SSIM / MS-SSIM / PSNR of two image batches and the SSIM gradient to the first one (include/ppst_hip.h, "image-quality
// metrics").
//
// Scheme.  Everything works at data range 1 on inputs times 1 / L (SSIM is invariant under a common scale of a, b and L).
//   forward     a block owns a 32 x 32 tile of the VALID grid of one (image, channel) plane.  It stages the 42 x 42 pixels of a and
//               b under the tile into LDS and subtracts their MEAN over the staged pixels from each (the variances are
//               shift-invariant, mu = m + g*(a - m) up to what the fp32 window's sum misses of 1 (SsWin), the tile mean minimises
//               sum (a - m)^2, and a flat tile then cancels exactly in g*(a^2) - mu^2), filters the five moment planes (a, b, a^2,
//               b^2, ab) horizontally into LDS (42 rows x 32 columns), then vertically out of LDS (a thread = one column, four consecutive rows: 14 LDS rows feed 4 x 11
//               taps), forms ssim and cs in registers and reduces them: wave butterfly, the four waves in order, one
//               (sum ssim, sum cs) pair per block.  The moment planes never reach HBM.  A finishing launch adds a plane's pairs in
//               a fixed order in float64.
//   backward    ONE launch; a block owns a 16 x 32 tile of the IMAGE and recomputes what reaches it: it stages the 36 x 52 pixels
//               of a and b around the tile, filters the five moment planes to the 26 x 42 map pixels p in [q - 10, q] (36 x 42
//               half-filtered rows in LDS), forms there A = d ssim / d mu_a, Bm = d ssim / d (g*a^2), Cm = d ssim / d (g*ab)
//               (zero outside the valid grid: the "full" correlation of the zero-extended maps) into the LDS the staged pixels no
//               longer need, filters the three maps with the transposed window through the LDS the half-filtered rows no longer
//               need, and writes grad = (g^T*A + 2 a g^T*Bm + b g^T*Cm) * gout[n] / (L C (H - 10)(W - 10)).  No map reaches HBM.
//   (The backward works on the UNSHIFTED pixels, the contract's formula as it stands.  Tried there and dropped: the shift by the
//   tile's first pixel, and by its mean.  The gradient's last step, g^T*A + 2 a g^T*Bm + b g^T*Cm, cancels terms of the size
//   |a| Bm, and on images whose brightness moves by O(1) across a tile a shift makes |a - m| larger than |a| somewhere: the
//   error against float64 went from 1.7e-6 of max |grad| to 2.3e-5 (first pixel) and 8.9e-6 (mean) at 64 x 64, over the bar.)
//   pool        2 x 2 mean, stride 2, any strides -> contiguous fp32 (the step between two MS-SSIM scales: a launch of its own)
//   sqerr       per image sum (a - b)^2 and sum |a - b|: 4096 elements per block, fixed-order block sums, float64 finish
// No floating-point atomics: two calls with the same inputs give the same bits.
#include "common.h"
#include <math.h>

namespace {

#define SS_K 11
#define SS_T 32                    // tile edge
#define SS_S (SS_T + SS_K - 1)     // staged edge: 42
#define SS_BT 16                   // rows of a backward tile (SS_T columns)
#define SS_BS (SS_BT + 2 * (SS_K - 1))   // staged rows of the backward pass: 36
#define SS_BW (SS_T + 2 * (SS_K - 1))    // staged columns: 52
#define SS_BMH (SS_BT + SS_K - 1)        // map rows: 26
#define SS_BMW (SS_T + SS_K - 1)         // map columns: 42
#define SS_SQ_CHUNK 4096           // elements per block of the squared-error pass

// the taps, and what their rounding to fp32 leaves of "the window sums to 1": sw = (sum g)^2, the 2-D sum, and dw = 1 - sw
// (about 3e-9).  The forward's shifted form is exact only with them: g*a = sw m + g*(a - m), and the variances pick up dw terms
struct SsWin { float g[SS_K]; float sw, dw; };
SsWin ss_window() {
  double e[SS_K], s = 0.0, t = 0.0;
  for (int i = 0; i < SS_K; ++i) { e[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); s += e[i]; }
  SsWin w;
  for (int i = 0; i < SS_K; ++i) { w.g[i] = (float)(e[i] / s); t += (double)w.g[i]; }
  w.sw = (float)(t * t); w.dw = (float)(1.0 - t * t);
  return w;
}
struct SsStr { int64_t n, c, y, x; };
inline SsStr ss_str(const int64_t* s) { return SsStr{s[0], s[1], s[2], s[3]}; }

template <int U8> __device__ __forceinline__ float ss_ld(const void* p, int64_t i) {
  if (U8) return (float)((const unsigned char*)p)[i];
  return ((const float*)p)[i];
}

// ssim, cs and what the gradient needs of them at one pixel, from the means, variances and covariance of the range-1 inputs
struct SsPoint { float s, cs, l, D1, D2; };
__device__ __forceinline__ SsPoint ss_point(float mua, float mub, float va, float vb, float vab) {
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  SsPoint p;
  p.D1 = mua * mua + mub * mub + C1; p.D2 = va + vb + C2;
  p.l = (2.f * mua * mub + C1) / p.D1;
  p.cs = (2.f * vab + C2) / p.D2;
  p.s = p.l * p.cs;
  return p;
}

// part[(plane * tiles + tile) * 2 + {0, 1}] = the tile's (sum ssim, sum cs)
template <int U8>
__global__ __launch_bounds__(256) void ss_moments_kernel(const void* __restrict__ a, SsStr sa, const void* __restrict__ b, SsStr sb, int C,
                                                         int H, int W, FastDiv d_tx, FastDiv d_tiles, float inv_L, SsWin win,
                                                         float* __restrict__ part) {
  __shared__ float sA[SS_S * SS_S], sB[SS_S * SS_S];
  __shared__ float sH[5][SS_S * SS_T];
  __shared__ float sRed[2][4];
  const int tid = threadIdx.x;
  unsigned tile, tx;
  const unsigned plane = fd_divmod(blockIdx.x, d_tiles, tile);
  const unsigned ty = fd_divmod(tile, d_tx, tx);
  const int n = (int)plane / C, c = (int)plane % C;
  const int vh = H - (SS_K - 1), vw = W - (SS_K - 1);
  const int y0 = (int)ty * SS_T, x0 = (int)tx * SS_T;          // < vh, < vw: inside the image
  const int64_t base_a = n * sa.n + c * sa.c, base_b = n * sb.n + c * sb.c;
  float tot_a = 0.f, tot_b = 0.f;
  for (int i = tid; i < SS_S * SS_S; i += 256) {
    const int r = i / SS_S, cx = i - r * SS_S;
    const int y = y0 + r, x = x0 + cx;
    float va = 0.f, vb = 0.f;                                 // beyond the image: feeds no valid output
    if (y < H && x < W) {
      va = ss_ld<U8>(a, base_a + y * sa.y + x * sa.x) * inv_L;
      vb = ss_ld<U8>(b, base_b + y * sb.y + x * sb.x) * inv_L;
    }
    sA[i] = va; sB[i] = vb;
    tot_a += va; tot_b += vb;
  }
  // the shift of this block: the mean of its staged pixels (fixed order: thread, wave butterfly, the four waves).  The variances
  // do not change under a shift, the mean of the tile minimises sum (a - m)^2, and a flat tile then cancels exactly
  tot_a = wave_sum(tot_a); tot_b = wave_sum(tot_b);
  if ((tid & 63) == 0) { sRed[0][tid >> 6] = tot_a; sRed[1][tid >> 6] = tot_b; }
  __syncthreads();
  const float inv_cnt = 1.f / (float)(min(SS_S, H - y0) * min(SS_S, W - x0));
  const float ma = (((sRed[0][0] + sRed[0][1]) + sRed[0][2]) + sRed[0][3]) * inv_cnt;
  const float mb = (((sRed[1][0] + sRed[1][1]) + sRed[1][2]) + sRed[1][3]) * inv_cnt;
  for (int i = tid; i < SS_S * SS_T; i += 256) {
    const int r = i / SS_T, x = i % SS_T;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
      const float va = sA[r * SS_S + x + k] - ma, vb = sB[r * SS_S + x + k] - mb, g = win.g[k];
      m0 = fmaf(g, va, m0); m1 = fmaf(g, vb, m1);
      m2 = fmaf(g, va * va, m2); m3 = fmaf(g, vb * vb, m3); m4 = fmaf(g, va * vb, m4);
    }
    sH[0][i] = m0; sH[1][i] = m1; sH[2][i] = m2; sH[3][i] = m3; sH[4][i] = m4;
  }
  __syncthreads();
  const int lx = tid % SS_T, rg = tid / SS_T;                 // column, group of four rows
  float acc[5][4];
#pragma unroll
  for (int p = 0; p < 5; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[p][j] = 0.f;
#pragma unroll
  for (int rr = 0; rr < 4 + SS_K - 1; ++rr) {
    float v[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) v[p] = sH[p][(rg * 4 + rr) * SS_T + lx];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (rr - j >= 0 && rr - j < SS_K) {
#pragma unroll
        for (int p = 0; p < 5; ++p) acc[p][j] = fmaf(win.g[rr - j], v[p], acc[p][j]);
      }
    }
  }
  const int x = x0 + lx;
  float sum_s = 0.f, sum_cs = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool valid = y0 + rg * 4 + j < vh && x < vw;
    // from the moments of the shifted pixels (da = g*(a - ma), ...): mu = sw ma + da, and the variances with their dw terms
    const float da = acc[0][j], db = acc[1][j], sw = win.sw, dw = win.dw;
    const float va = acc[2][j] - da * da + dw * (2.f * ma * da + sw * ma * ma), vb = acc[3][j] - db * db + dw * (2.f * mb * db + sw * mb * mb);
    const float vab = acc[4][j] - da * db + dw * (ma * db + mb * da + sw * ma * mb);
    const SsPoint p = ss_point(sw * ma + da, sw * mb + db, va, vb, vab);
    sum_s += valid ? p.s : 0.f;
    sum_cs += valid ? p.cs : 0.f;
  }
  sum_s = wave_sum(sum_s); sum_cs = wave_sum(sum_cs);
  if ((tid & 63) == 0) { sRed[0][tid >> 6] = sum_s; sRed[1][tid >> 6] = sum_cs; }
  __syncthreads();
  if (tid == 0) {
    part[(int64_t)blockIdx.x * 2] = ((sRed[0][0] + sRed[0][1]) + sRed[0][2]) + sRed[0][3];
    part[(int64_t)blockIdx.x * 2 + 1] = ((sRed[1][0] + sRed[1][1]) + sRed[1][2]) + sRed[1][3];
  }
}

// one block of 64 lanes per image: a plane's pairs are added lane-strided, then across the lanes, in float64
__global__ __launch_bounds__(64) void ss_finish_kernel(const float* __restrict__ part, int C, int tiles, double inv_cnt, float* __restrict__ out,
                                                       float* __restrict__ ssim_bc, float* __restrict__ cs_bc) {
  const int n = blockIdx.x, lane = threadIdx.x;
  double img = 0.0;
  for (int c = 0; c < C; ++c) {
    const int64_t plane = (int64_t)n * C + c;
    const float* p = part + plane * tiles * 2;
    double s = 0.0, q = 0.0;
    for (int t = lane; t < tiles; t += 64) { s += (double)p[2 * t]; q += (double)p[2 * t + 1]; }
    s = wave_sum_f64(s) * inv_cnt; q = wave_sum_f64(q) * inv_cnt;
    if (lane == 0) { ssim_bc[plane] = (float)s; cs_bc[plane] = (float)q; }
    img += s;
  }
  if (lane == 0 && out) out[n] = (float)(img / C);
}

// the backward pass: a 16 x 32 tile of one (image, channel) plane of the IMAGE (scheme: the head of this file)
__global__ __launch_bounds__(256) void ss_grad_kernel(const float* __restrict__ a, SsStr sa, const float* __restrict__ b, SsStr sb,
                                                      const float* __restrict__ gout, int C, int H, int W, FastDiv d_tx, FastDiv d_tiles,
                                                      float inv_L, float scale, SsWin win, float* __restrict__ grad) {
  __shared__ float sAB[2 * SS_BS * SS_BW];       // staged a, b [36][52]; then the maps A, Bm, Cm [26][42]
  __shared__ float sH[5 * SS_BS * SS_BMW];       // half-filtered moment rows [5][36][42]; then the half-filtered maps [3][26][32]
  static_assert(3 * SS_BMH * SS_BMW <= 2 * SS_BS * SS_BW && 3 * SS_BMH * SS_T <= 5 * SS_BS * SS_BMW, "the LDS reuse");
  float* sA = sAB;
  float* sB = sAB + SS_BS * SS_BW;
  const int tid = threadIdx.x;
  unsigned tile, tx;
  const unsigned plane = fd_divmod(blockIdx.x, d_tiles, tile);
  const unsigned ty = fd_divmod(tile, d_tx, tx);
  const int n = (int)plane / C, c = (int)plane % C;
  const int vh = H - (SS_K - 1), vw = W - (SS_K - 1);
  const int y0 = (int)ty * SS_BT, x0 = (int)tx * SS_T;         // < H, < W
  const int64_t base_a = n * sa.n + c * sa.c, base_b = n * sb.n + c * sb.c;
  // staged (r, cx) = image pixel (y0 - 10 + r, x0 - 10 + cx), zero outside the image (feeds no valid map pixel)
  for (int i = tid; i < SS_BS * SS_BW; i += 256) {
    const int r = i / SS_BW, cx = i - r * SS_BW;
    const int y = y0 - (SS_K - 1) + r, x = x0 - (SS_K - 1) + cx;
    float va = 0.f, vb = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      va = a[base_a + y * sa.y + x * sa.x] * inv_L;
      vb = b[base_b + y * sb.y + x * sb.x] * inv_L;
    }
    sA[i] = va; sB[i] = vb;
  }
  __syncthreads();
  // map pixel (r, cx) = valid-grid pixel (y0 - 10 + r, x0 - 10 + cx): its window starts at staged (r, cx)
  for (int i = tid; i < SS_BS * SS_BMW; i += 256) {
    const int r = i / SS_BMW, cx = i - r * SS_BMW;
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
      const float va = sA[r * SS_BW + cx + k], vb = sB[r * SS_BW + cx + k], g = win.g[k];
      m0 = fmaf(g, va, m0); m1 = fmaf(g, vb, m1);
      m2 = fmaf(g, va * va, m2); m3 = fmaf(g, vb * vb, m3); m4 = fmaf(g, va * vb, m4);
    }
    sH[i] = m0; sH[SS_BS * SS_BMW + i] = m1; sH[2 * SS_BS * SS_BMW + i] = m2; sH[3 * SS_BS * SS_BMW + i] = m3; sH[4 * SS_BS * SS_BMW + i] = m4;
  }
  // this thread's two output pixels (column lx, rows 2 rg, 2 rg + 1 of the tile): their a, b before the maps overwrite them
  const int lx = tid % SS_T, rg = tid / SS_T;
  float pa[2], pb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    pa[j] = sA[(rg * 2 + j + SS_K - 1) * SS_BW + lx + SS_K - 1];
    pb[j] = sB[(rg * 2 + j + SS_K - 1) * SS_BW + lx + SS_K - 1];
  }
  __syncthreads();
  // vertical pass + the maps: an item = one map column, two consecutive map rows (12 LDS rows feed 2 x 11 taps); 13 x 42 items
  float mP[3][2], mQ[3][2], mR[3][2];                          // at most ceil(546 / 256) = 3 items per thread
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int item = tid + it * 256;
    if (item < (SS_BMH / 2) * SS_BMW) {
      const int r2 = item / SS_BMW, cx = item - r2 * SS_BMW;
      float acc[5][2];
#pragma unroll
      for (int p = 0; p < 5; ++p) { acc[p][0] = 0.f; acc[p][1] = 0.f; }
#pragma unroll
      for (int rr = 0; rr < 2 + SS_K - 1; ++rr) {
        float v[5];
#pragma unroll
        for (int p = 0; p < 5; ++p) v[p] = sH[p * SS_BS * SS_BMW + (r2 * 2 + rr) * SS_BMW + cx];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (rr - j >= 0 && rr - j < SS_K) {
#pragma unroll
            for (int p = 0; p < 5; ++p) acc[p][j] = fmaf(win.g[rr - j], v[p], acc[p][j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int py = y0 - (SS_K - 1) + r2 * 2 + j, px = x0 - (SS_K - 1) + cx;
        const SsPoint p = ss_point(acc[0][j], acc[1][j], acc[2][j] - acc[0][j] * acc[0][j], acc[3][j] - acc[1][j] * acc[1][j],
                                   acc[4][j] - acc[0][j] * acc[1][j]);
        const bool valid = py >= 0 && py < vh && px >= 0 && px < vw;
        const float Smu = p.cs * 2.f * (acc[1][j] - acc[0][j] * p.l) / p.D1;   // d ssim / d mu_a at fixed variances
        const float Q = -p.s / p.D2, R = 2.f * p.l / p.D2;                // d ssim / d var_a, d ssim / d cov
        mP[it][j] = valid ? Smu - 2.f * Q * acc[0][j] - R * acc[1][j] : 0.f;      // A of the contract
        mQ[it][j] = valid ? Q : 0.f;
        mR[it][j] = valid ? R : 0.f;
      }
    }
  }
  // (every thread read its a, b before the barrier above: the staged pixels may go)
  float* sM = sAB;                                             // [3][26][42]
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int item = tid + it * 256;
    if (item < (SS_BMH / 2) * SS_BMW) {
      const int r2 = item / SS_BMW, cx = item - r2 * SS_BMW;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int o = (r2 * 2 + j) * SS_BMW + cx;
        sM[o] = mP[it][j]; sM[SS_BMH * SS_BMW + o] = mQ[it][j]; sM[2 * SS_BMH * SS_BMW + o] = mR[it][j];
      }
    }
  }
  __syncthreads();                                             // the maps are written, the half-filtered moment rows are read
  // T(r, x) = sum_i g[i] M(r, x0 + x - i): map column x + 10 - i
  float* sT = sH;                                              // [3][26][32]
  for (int i = tid; i < SS_BMH * SS_T; i += 256) {
    const int r = i / SS_T, x = i % SS_T;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int k = 0; k < SS_K; ++k) {
      const int o = r * SS_BMW + x + (SS_K - 1) - k;
      const float g = win.g[k];
      t0 = fmaf(g, sM[o], t0); t1 = fmaf(g, sM[SS_BMH * SS_BMW + o], t1); t2 = fmaf(g, sM[2 * SS_BMH * SS_BMW + o], t2);
    }
    sT[i] = t0; sT[SS_BMH * SS_T + i] = t1; sT[2 * SS_BMH * SS_T + i] = t2;
  }
  __syncthreads();
  // out(y0 + yl) = sum_i g[i] T(map row yl + 10 - i); yl = 2 rg + j, map row 2 rg + rr: i = j + 10 - rr
  float acc[3][2];
#pragma unroll
  for (int p = 0; p < 3; ++p) { acc[p][0] = 0.f; acc[p][1] = 0.f; }
#pragma unroll
  for (int rr = 0; rr < 2 + SS_K - 1; ++rr) {
    float v[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) v[p] = sT[p * SS_BMH * SS_T + (rg * 2 + rr) * SS_T + lx];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j + (SS_K - 1) - rr >= 0 && j + (SS_K - 1) - rr < SS_K) {
#pragma unroll
        for (int p = 0; p < 3; ++p) acc[p][j] = fmaf(win.g[j + (SS_K - 1) - rr], v[p], acc[p][j]);
      }
    }
  }
  const int x = x0 + lx;
  if (x >= W) return;
  const float w = gout[n] * scale;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + rg * 2 + j;
    if (y < H) grad[((int64_t)plane * H + y) * W + x] = (acc[0][j] + 2.f * pa[j] * acc[1][j] + pb[j] * acc[2][j]) * w;
  }
}

template <int U8>
__global__ __launch_bounds__(256) void ss_pool_kernel(const void* __restrict__ x, SsStr sx, int C, FastDiv d_ow, FastDiv d_oh, FastDiv d_c,
                                                      unsigned total, float* __restrict__ out) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
    unsigned ox, oy, c;
    const unsigned n = fd_divmod(fd_divmod(fd_divmod((unsigned)t, d_ow, ox), d_oh, oy), d_c, c);
    const int64_t o = n * sx.n + c * sx.c + 2 * (int64_t)oy * sx.y + 2 * (int64_t)ox * sx.x;
    out[t] = 0.25f * (((ss_ld<U8>(x, o) + ss_ld<U8>(x, o + sx.x)) + ss_ld<U8>(x, o + sx.y)) + ss_ld<U8>(x, o + sx.y + sx.x));
  }
}

struct SsW5 { double w[5]; };
__global__ void ss_msssim_kernel(const float* __restrict__ vals, int B, int C, SsW5 w, float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= B) return;
  double acc = 0.0;
  for (int c = 0; c < C; ++c) {
    double p = 1.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) p *= pow(fmax((double)vals[((int64_t)j * B + n) * C + c], 0.0), w.w[j]);
    acc += p;
  }
  out[n] = (float)(acc / C);
}

// element e of an image = (r1, r2, q) by d1 then d2, at offset r1 * s1 + r2 * s2 + q * s3 (the host puts the smaller of the
// channel and the column stride first)
template <int U8>
__global__ __launch_bounds__(256) void ss_sqerr_kernel(const void* __restrict__ a, const void* __restrict__ b, int64_t an, int64_t a1, int64_t a2,
                                                       int64_t a3, int64_t bn, int64_t b1, int64_t b2, int64_t b3, FastDiv d1, FastDiv d2,
                                                       FastDiv d_blk, unsigned per, float* __restrict__ part) {
  __shared__ float sRed[2][4];
  const int tid = threadIdx.x;
  unsigned blk;
  const unsigned n = fd_divmod(blockIdx.x, d_blk, blk);
  float s2 = 0.f, s1 = 0.f;
#pragma unroll 4
  for (int k = 0; k < SS_SQ_CHUNK / 256; ++k) {
    const uint64_t e = (uint64_t)blk * SS_SQ_CHUNK + k * 256 + tid;
    if (e < per) {
      unsigned r1, r2;
      const unsigned q = fd_divmod(fd_divmod((unsigned)e, d1, r1), d2, r2);
      const float d = ss_ld<U8>(a, n * an + r1 * a1 + r2 * a2 + q * a3) - ss_ld<U8>(b, n * bn + r1 * b1 + r2 * b2 + q * b3);
      s2 = fmaf(d, d, s2); s1 += fabsf(d);
    }
  }
  s2 = wave_sum(s2); s1 = wave_sum(s1);
  if ((tid & 63) == 0) { sRed[0][tid >> 6] = s2; sRed[1][tid >> 6] = s1; }
  __syncthreads();
  if (tid == 0) {
    part[(int64_t)blockIdx.x * 2] = ((sRed[0][0] + sRed[0][1]) + sRed[0][2]) + sRed[0][3];
    part[(int64_t)blockIdx.x * 2 + 1] = ((sRed[1][0] + sRed[1][1]) + sRed[1][2]) + sRed[1][3];
  }
}
__global__ __launch_bounds__(64) void ss_sqerr_finish_kernel(const float* __restrict__ part, int nblk, double inv_per, double L, float* __restrict__ out) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* p = part + (int64_t)n * nblk * 2;
  double s2 = 0.0, s1 = 0.0;
  for (int t = lane; t < nblk; t += 64) { s2 += (double)p[2 * t]; s1 += (double)p[2 * t + 1]; }
  s2 = wave_sum_f64(s2) * inv_per; s1 = wave_sum_f64(s1) * inv_per;
  if (lane == 0) {
    out[n * 3] = (float)s2;
    out[n * 3 + 1] = (float)s1;
    out[n * 3 + 2] = s2 > 0.0 ? (float)(10.0 * log10(L * L / s2)) : __builtin_inff();
  }
}

// sizes: PPST_EINVAL or PPST_OK
int ss_check(int B, int C, int H, int W, int min_hw) {
  if (B < 0 || C < 1 || H < min_hw || W < min_hw) return PPST_EINVAL;
  const int64_t hw = (int64_t)H * W;
  if (hw > PPST_IDX32_MAX || hw * C > PPST_IDX32_MAX || hw * C * (B > 0 ? B : 1) > PPST_IDX32_MAX) return PPST_EINVAL;
  return PPST_OK;
}
inline int64_t ss_tiles(int h, int w) { return (int64_t)cdiv(h, SS_T) * cdiv(w, SS_T); }

}  // namespace

extern "C" {

int64_t ppst_ssim_ws(int B, int C, int H, int W) {
  if (ss_check(B, C, H, W, SS_K)) return PPST_EINVAL;
  return (int64_t)B * C * ss_tiles(H - (SS_K - 1), W - (SS_K - 1)) * 2 * sizeof(float) + 16;
}

int ppst_ssim_forward(const void* a, const int64_t* a_strides, const void* b, const int64_t* b_strides, int u8, int B, int C, int H,
                      int W, float data_range, void* out, void* ssim_bc, void* cs_bc, void* ws, void* stream) {
  if (ss_check(B, C, H, W, SS_K) || !(data_range > 0.f) || u8 < 0 || u8 > 1) return PPST_EINVAL;
  const int vh = H - (SS_K - 1), vw = W - (SS_K - 1);
  const int64_t tiles = ss_tiles(vh, vw), planes = (int64_t)B * C, blocks = planes * tiles;
  if (blocks > 0x7FFFFFFFll) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!a || !a_strides || !b || !b_strides || !ssim_bc || !cs_bc || !ws) return PPST_ENULL;
  hipStream_t st = as_stream(stream);
  const FastDiv d_tx = make_fastdiv((unsigned)cdiv(vw, SS_T)), d_tiles = make_fastdiv((unsigned)tiles);
  const float inv_L = 1.f / data_range;
  if (u8)
    PPST_LAUNCH(ss_moments_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a, ss_str(a_strides), b, ss_str(b_strides), C, H, W, d_tx,
                d_tiles, inv_L, ss_window(), (float*)ws);
  else
    PPST_LAUNCH(ss_moments_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, a, ss_str(a_strides), b, ss_str(b_strides), C, H, W, d_tx,
                d_tiles, inv_L, ss_window(), (float*)ws);
  int rc = PPST_LAUNCH_CHECK();
  if (rc) return rc;
  PPST_LAUNCH(ss_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)ws, C, (int)tiles, 1.0 / ((double)vh * vw), (float*)out,
              (float*)ssim_bc, (float*)cs_bc);
  return PPST_LAUNCH_CHECK();
}

int ppst_ssim_backward(const void* a, const int64_t* a_strides, const void* b, const int64_t* b_strides, const void* gout, int B,
                       int C, int H, int W, float data_range, void* grad, void* stream) {
  if (ss_check(B, C, H, W, SS_K) || !(data_range > 0.f)) return PPST_EINVAL;
  const int vh = H - (SS_K - 1), vw = W - (SS_K - 1);
  const int64_t planes = (int64_t)B * C, tiles = (int64_t)cdiv(H, SS_BT) * cdiv(W, SS_T);
  if (planes * tiles > 0x7FFFFFFFll) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!a || !a_strides || !b || !b_strides || !gout || !grad) return PPST_ENULL;
  const float inv_L = 1.f / data_range;
  const float scale = (float)((double)inv_L / ((double)C * vh * vw));
  PPST_LAUNCH(ss_grad_kernel, dim3((unsigned)(planes * tiles)), dim3(256), 0, as_stream(stream), (const float*)a, ss_str(a_strides),
              (const float*)b, ss_str(b_strides), (const float*)gout, C, H, W, make_fastdiv((unsigned)cdiv(W, SS_T)),
              make_fastdiv((unsigned)tiles), inv_L, scale, ss_window(), (float*)grad);
  return PPST_LAUNCH_CHECK();
}

int ppst_pool2x2(const void* x, const int64_t* strides, int u8, int B, int C, int H, int W, void* out, void* stream) {
  if (ss_check(B, C, H, W, 2) || u8 < 0 || u8 > 1) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!x || !strides || !out) return PPST_ENULL;
  const int oh = H / 2, ow = W / 2;
  const int64_t total = (int64_t)B * C * oh * ow;
  const FastDiv d_ow = make_fastdiv(ow), d_oh = make_fastdiv(oh), d_c = make_fastdiv(C);
  if (u8)
    PPST_LAUNCH(ss_pool_kernel<1>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), x, ss_str(strides), C, d_ow, d_oh, d_c, (unsigned)total,
                (float*)out);
  else
    PPST_LAUNCH(ss_pool_kernel<0>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), x, ss_str(strides), C, d_ow, d_oh, d_c, (unsigned)total,
                (float*)out);
  return PPST_LAUNCH_CHECK();
}

int ppst_msssim_combine(const void* vals, int B, int C, void* out, void* stream) {
  if (B < 0 || C < 1 || (int64_t)B * C > 0x7FFFFFFFll / 5) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!vals || !out) return PPST_ENULL;
  const SsW5 w = {{0.0448, 0.2856, 0.3001, 0.2363, 0.1333}};
  PPST_LAUNCH(ss_msssim_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, as_stream(stream), (const float*)vals, B, C, w, (float*)out);
  return PPST_LAUNCH_CHECK();
}

int64_t ppst_sqerr_ws(int B, int C, int H, int W) {
  if (ss_check(B, C, H, W, 1)) return PPST_EINVAL;
  return (int64_t)B * cdiv64((int64_t)C * H * W, SS_SQ_CHUNK) * 2 * sizeof(float) + 16;
}

int ppst_sqerr(const void* a, const int64_t* a_strides, const void* b, const int64_t* b_strides, int u8, int B, int C, int H, int W,
               float data_range, void* out, void* ws, void* stream) {
  if (ss_check(B, C, H, W, 1) || !(data_range > 0.f) || u8 < 0 || u8 > 1) return PPST_EINVAL;
  const int64_t per = (int64_t)C * H * W, nblk = cdiv64(per, SS_SQ_CHUNK);
  if ((int64_t)B * nblk > 0x7FFFFFFFll) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!a || !a_strides || !b || !b_strides || !out || !ws) return PPST_ENULL;
  hipStream_t st = as_stream(stream);
  // walk order: the channel first where it is the closest in memory (channels-last), else the column
  const bool cfast = a_strides[1] < a_strides[3];
  const int i1 = cfast ? 1 : 3, i2 = cfast ? 3 : 2, i3 = cfast ? 2 : 1;
  const FastDiv d1 = make_fastdiv(cfast ? C : W), d2 = make_fastdiv(cfast ? W : H), d_blk = make_fastdiv((unsigned)nblk);
  if (u8)
    PPST_LAUNCH(ss_sqerr_kernel<1>, dim3((unsigned)(B * nblk)), dim3(256), 0, st, a, b, a_strides[0], a_strides[i1], a_strides[i2], a_strides[i3],
                b_strides[0], b_strides[i1], b_strides[i2], b_strides[i3], d1, d2, d_blk, (unsigned)per, (float*)ws);
  else
    PPST_LAUNCH(ss_sqerr_kernel<0>, dim3((unsigned)(B * nblk)), dim3(256), 0, st, a, b, a_strides[0], a_strides[i1], a_strides[i2], a_strides[i3],
                b_strides[0], b_strides[i1], b_strides[i2], b_strides[i3], d1, d2, d_blk, (unsigned)per, (float*)ws);
  int rc = PPST_LAUNCH_CHECK();
  if (rc) return rc;
  PPST_LAUNCH(ss_sqerr_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)ws, (int)nblk, 1.0 / (double)per, (double)data_range,
              (float*)out);
  return PPST_LAUNCH_CHECK();
}

}  // extern "C"
