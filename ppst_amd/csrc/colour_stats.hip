// Per-region colour statistics of uint8 RGB images and exact 1-Wasserstein distances between their histograms
// (include/ppst_hip.h, "colour statistics").
//
// Scheme.
//   setup       writes the launch's constants -- the 256-entry sRGB table and the P directions with their offsets, validated
//               and built on the host -- from its kernel arguments to the head of the workspace (the caller's memory: no host
//               buffer has to outlive the call, no symbol per device)
//   stats       a block owns up to 64 KB of LDS histograms [R][P][256] of ONE image and at most 1/64 of its pixels; each of
//               its four waves walks wave chunks of 1024 consecutive pixels (lane l: pixels k * 64 + l, k < 16, kept packed in
//               16 registers).  First walk: the LDS histogram adds and the integer sums (count, r, g, b) per region.  Where
//               every lane of a wave that has a pixel to add hits the SAME word -- a flat image, a flat background -- one lane adds
//               the population count instead (the adds of a wave to one LDS word serialise: 64 passes become 1); otherwise
//               the lanes add one by one.  Then the wave's pivot per region, the Lab value of its rounded mean colour, and the
//               second walk over the registers: sums of d = lab - pivot (3) and of the products of d (6) per region, wave
//               butterfly, one 64-byte record per (wave chunk, region) in the workspace.  A flat region has d == 0 in every
//               pixel.  At the end the block adds its non-zero LDS bins to the image's histogram (integer atomics).
//   finish      one wave per (image, region): N = sum n_k and mu = sum (n_k pivot_k + sum d) / N, then with e_k = pivot_k - mu
//               C = sum_k (sum dd + e sum d^T + sum d e^T + n_k e e^T), lane-strided and butterflied in float64, cov = C / N.
//               For a flat region every term is exact: mu is the pixel's value and the covariance is 0.
//   w1          one wave per (pair, region, projection): four bins per lane, a wave scan of the lane totals, the numerator in
//               int64.
// Nothing depends on the batch: the wave chunks and the blocks per image follow from H * W alone.
#include "common.h"
#include "colour_lab.h"                   // sRGB -> Lab: the table, the matrix, cs_lab
#include <math.h>

namespace {

#define CS_MAX_R 4
#define CS_MAX_P 16
#define CS_MAX_HW (1 << 22)
#define CS_WCHUNK 1024                // pixels of a wave chunk: 64 lanes x CS_PIX
#define CS_PIX 16
#define CS_MAX_BLOCKS 64              // per image
#define CS_REC 16                     // floats of a record: (pivot L a b, n) (sum d L a b, -) (LL La Lb aa) (ab bb - -)
#define CS_CONST_FLOATS (256 + 4 * CS_MAX_P)

struct CsConst { float tab[256]; int dir[CS_MAX_P][4]; };   // (d0, d1, d2, 255 * sum of the negative |d_c|)

__global__ __launch_bounds__(64) void cs_setup_kernel(CsConst c, float* __restrict__ out) {
  for (int i = threadIdx.x; i < CS_CONST_FLOATS; i += 64)
    out[i] = i < 256 ? c.tab[i] : __int_as_float(c.dir[(i - 256) >> 2][(i - 256) & 3]);
}

__device__ __forceinline__ int cs_wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void cs_stats_kernel(const unsigned char* __restrict__ img, int64_t sn, int64_t sy,
                                                       const unsigned char* __restrict__ labels, int64_t ln, int64_t ly, int HW,
                                                       FastDiv d_w, int R, int P, int nb, int nwc, CsMat M,
                                                       const float* __restrict__ cst, unsigned* __restrict__ hist,
                                                       float* __restrict__ part) {
  extern __shared__ unsigned cs_h[];                           // [R][P][256]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = (int)blockIdx.x / nb, j = (int)blockIdx.x - n * nb;
  const int words = R * P * 256;
  for (int i = tid; i < words; i += 256) cs_h[i] = 0u;
  __syncthreads();
  const float* tab = cst;
  const int4* dir = (const int4*)(cst + 256);
  const unsigned char* im = img + n * sn;
  const unsigned char* lb = labels ? labels + n * ln : nullptr;
  for (int c = j * 4 + wv; c < nwc; c += nb * 4) {             // (uniform in a wave)
    unsigned px[CS_PIX];                                       // r | g << 8 | b << 16 | label << 24
    int cnt[CS_MAX_R], sr[CS_MAX_R], sg[CS_MAX_R], sb[CS_MAX_R];
#pragma unroll
    for (int r = 0; r < CS_MAX_R; ++r) cnt[r] = sr[r] = sg[r] = sb[r] = 0;
#pragma unroll
    for (int k = 0; k < CS_PIX; ++k) {
      const unsigned e = (unsigned)c * CS_WCHUNK + k * 64 + lane;
      unsigned v = 0xFF000000u;                                // beyond the image: no region
      if (e < (unsigned)HW) {
        unsigned x;
        const unsigned y = fd_divmod(e, d_w, x);
        const unsigned char* p = im + y * sy + x * 3;
        v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((lb ? (unsigned)lb[y * ly + x] : 0u) << 24);
      }
      px[k] = v;
      const int cr = v & 255, cg = (v >> 8) & 255, cb = (v >> 16) & 255, lab = v >> 24;
      const bool valid = lab < R;
#pragma unroll
      for (int r = 0; r < CS_MAX_R; ++r) {
        const bool m = lab == r;                               // (lab < R: regions >= R stay empty)
        cnt[r] += m ? 1 : 0; sr[r] += m ? cr : 0; sg[r] += m ? cg : 0; sb[r] += m ? cb : 0;
      }
      const unsigned long long act = __ballot(valid);
      if (act == 0ull) continue;
      const int lead = __ffsll((long long)act) - 1;
      for (int p = 0; p < P; ++p) {
        const int4 d = dir[p];
        const int t = ((d.x * cr + d.y * cg + d.z * cb + d.w) >> 12) & 255;     // (0 .. 255 already: the host checked the row)
        const int key = valid ? (lab * P + p) * 256 + t : -1;
        const int k0 = __builtin_amdgcn_readlane(key, lead);
        if (__ballot(key == k0) == act) {                      // one word for the whole wave: one add of the count
          if (lane == lead) atomicAdd(&cs_h[k0], (unsigned)__popcll(act));
        } else if (valid) {
          atomicAdd(&cs_h[key], 1u);
        }
      }
    }
    // the pivots: the Lab value of the region's mean colour in this wave chunk, rounded to integers
    CsLab piv[CS_MAX_R];
    int nr[CS_MAX_R];
#pragma unroll
    for (int r = 0; r < CS_MAX_R; ++r) {
      piv[r].L = piv[r].a = piv[r].b = 0.f;
      nr[r] = 0;
      if (r < R) {
        const int q = cs_wave_sum_i(cnt[r]), tr = cs_wave_sum_i(sr[r]), tg = cs_wave_sum_i(sg[r]), tb = cs_wave_sum_i(sb[r]);
        nr[r] = q;
        if (q > 0) piv[r] = cs_lab(tab, M, (unsigned)((tr + q / 2) / q), (unsigned)((tg + q / 2) / q), (unsigned)((tb + q / 2) / q));
      }
    }
    float acc[CS_MAX_R][9];
#pragma unroll
    for (int r = 0; r < CS_MAX_R; ++r)
#pragma unroll
      for (int i = 0; i < 9; ++i) acc[r][i] = 0.f;
#pragma unroll
    for (int k = 0; k < CS_PIX; ++k) {
      const unsigned v = px[k];
      const int lab = v >> 24;
      const CsLab q = cs_lab(tab, M, v & 255, (v >> 8) & 255, (v >> 16) & 255);
#pragma unroll
      for (int r = 0; r < CS_MAX_R; ++r) {
        if (r < R) {
          const bool m = lab == r;
          const float dL = m ? q.L - piv[r].L : 0.f, da = m ? q.a - piv[r].a : 0.f, db = m ? q.b - piv[r].b : 0.f;
          acc[r][0] += dL; acc[r][1] += da; acc[r][2] += db;
          acc[r][3] = fmaf(dL, dL, acc[r][3]); acc[r][4] = fmaf(dL, da, acc[r][4]); acc[r][5] = fmaf(dL, db, acc[r][5]);
          acc[r][6] = fmaf(da, da, acc[r][6]); acc[r][7] = fmaf(da, db, acc[r][7]); acc[r][8] = fmaf(db, db, acc[r][8]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < CS_MAX_R; ++r) {
      if (r < R) {
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[r][i] = wave_sum(acc[r][i]);
        if (lane == 0) {
          float4* o = (float4*)(part + (((int64_t)n * nwc + c) * CS_MAX_R + r) * CS_REC);
          o[0] = make_float4(piv[r].L, piv[r].a, piv[r].b, (float)nr[r]);
          o[1] = make_float4(acc[r][0], acc[r][1], acc[r][2], 0.f);
          o[2] = make_float4(acc[r][3], acc[r][4], acc[r][5], acc[r][6]);
          o[3] = make_float4(acc[r][7], acc[r][8], 0.f, 0.f);
        }
      }
    }
  }
  __syncthreads();
  unsigned* h = hist + (int64_t)n * words;
  for (int i = tid; i < words; i += 256) {
    const unsigned v = cs_h[i];
    if (v) atomicAdd(&h[i], v);
  }
}

__global__ __launch_bounds__(64) void cs_finish_kernel(const float* __restrict__ part, int R, int nwc, unsigned* __restrict__ count,
                                                       double* __restrict__ mean, double* __restrict__ cov) {
  const int n = (int)blockIdx.x / R, r = (int)blockIdx.x - n * R, lane = threadIdx.x;
  const float* p = part + ((int64_t)n * nwc * CS_MAX_R + r) * CS_REC;
  const int64_t step = CS_MAX_R * CS_REC;
  double N = 0.0, S[3] = {0.0, 0.0, 0.0};
  for (int c = lane; c < nwc; c += 64) {
    const float4 a = *(const float4*)(p + c * step), d = *(const float4*)(p + c * step + 4);
    if (a.w > 0.f) {
      const double nk = (double)a.w;
      N += nk;
      S[0] += nk * (double)a.x + (double)d.x; S[1] += nk * (double)a.y + (double)d.y; S[2] += nk * (double)a.z + (double)d.z;
    }
  }
  N = wave_sum_f64(N);
#pragma unroll
  for (int i = 0; i < 3; ++i) S[i] = wave_sum_f64(S[i]);
  double mu[3] = {0.0, 0.0, 0.0}, C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (N > 0.0) {                                               // (uniform)
#pragma unroll
    for (int i = 0; i < 3; ++i) mu[i] = S[i] / N;
    for (int c = lane; c < nwc; c += 64) {
      const float4 a = *(const float4*)(p + c * step), d = *(const float4*)(p + c * step + 4);
      const float4 u = *(const float4*)(p + c * step + 8), w = *(const float4*)(p + c * step + 12);
      if (a.w > 0.f) {
        const double nk = (double)a.w, e0 = (double)a.x - mu[0], e1 = (double)a.y - mu[1], e2 = (double)a.z - mu[2];
        const double d0 = (double)d.x, d1 = (double)d.y, d2 = (double)d.z;
        C[0] += (double)u.x + 2.0 * e0 * d0 + nk * e0 * e0;
        C[1] += (double)u.y + e0 * d1 + e1 * d0 + nk * e0 * e1;
        C[2] += (double)u.z + e0 * d2 + e2 * d0 + nk * e0 * e2;
        C[3] += (double)u.w + 2.0 * e1 * d1 + nk * e1 * e1;
        C[4] += (double)w.x + e1 * d2 + e2 * d1 + nk * e1 * e2;
        C[5] += (double)w.y + 2.0 * e2 * d2 + nk * e2 * e2;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) C[i] = wave_sum_f64(C[i]) / N;
  }
  if (lane == 0) {
    count[blockIdx.x] = (unsigned)N;
    for (int i = 0; i < 3; ++i) mean[(int64_t)blockIdx.x * 3 + i] = mu[i];
    for (int i = 0; i < 6; ++i) cov[(int64_t)blockIdx.x * 6 + i] = C[i];
  }
}

// block = (pair k, region * P + projection): lane l holds bins 4 l .. 4 l + 3 of both histograms
__global__ __launch_bounds__(64) void cs_w1_kernel(const unsigned* __restrict__ ha, int Ba, const unsigned* __restrict__ hb, int Bb,
                                                   const int* __restrict__ pairs, int RP, long long* __restrict__ num) {
  const int k = (int)blockIdx.x / RP, rp = (int)blockIdx.x - k * RP, lane = threadIdx.x;
  const int i = pairs[2 * k], j = pairs[2 * k + 1];
  if (i < 0 || i >= Ba || j < 0 || j >= Bb) {                  // (uniform) nothing is read
    if (lane == 0) num[blockIdx.x] = -1;
    return;
  }
  const uint4 a = ((const uint4*)(ha + ((int64_t)i * RP + rp) * 256))[lane];
  const uint4 b = ((const uint4*)(hb + ((int64_t)j * RP + rp) * 256))[lane];
  unsigned ca[4] = {a.x, a.x + a.y, a.x + a.y + a.z, a.x + a.y + a.z + a.w};
  unsigned cb[4] = {b.x, b.x + b.y, b.x + b.y + b.z, b.x + b.y + b.z + b.w};
  unsigned ta = ca[3], tb = cb[3];                             // inclusive scan of the lane totals (n <= 2^22 fits)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned ua = __shfl_up(ta, o, 64), ub = __shfl_up(tb, o, 64);
    if (lane >= o) { ta += ua; tb += ub; }
  }
  const long long nA = (long long)__shfl(ta, 63, 64), nB = (long long)__shfl(tb, 63, 64);
  const unsigned xa = ta - ca[3], xb = tb - cb[3];             // bins before this lane's
  long long s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long v = (long long)(xa + ca[q]) * nB - (long long)(xb + cb[q]) * nA;
    s += v < 0 ? -v : v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) num[blockIdx.x] = s;
}

// sizes: PPST_EINVAL or PPST_OK
int cs_check(int B, int H, int W) {
  if (B < 0 || H < 1 || W < 1 || (int64_t)H * W > CS_MAX_HW) return PPST_EINVAL;
  return PPST_OK;
}
inline int cs_wave_chunks(int H, int W) { return cdiv(H * W, CS_WCHUNK); }

}  // namespace

extern "C" {

int64_t ppst_colour_stats_ws(int B, int H, int W) {
  if (cs_check(B, H, W)) return PPST_EINVAL;
  return (int64_t)CS_CONST_FLOATS * sizeof(float) + (int64_t)B * cs_wave_chunks(H, W) * CS_MAX_R * CS_REC * sizeof(float) + 16;
}

int ppst_colour_stats(const void* img, int64_t img_sn, int64_t img_sy, int64_t img_sx, const void* labels, int64_t lab_sn,
                      int64_t lab_sy, int B, int H, int W, int R, const int16_t* dirs, int P, void* hist, void* count, void* lab_mean,
                      void* lab_cov, void* ws, void* stream) {
  if (cs_check(B, H, W) || R < 1 || R > CS_MAX_R || P < 1 || P > CS_MAX_P || img_sx != 3) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!img || !dirs || !hist || !count || !lab_mean || !lab_cov || !ws) return PPST_ENULL;
  static CsConst base;                                         // the table: built once (the same values every time)
  static const bool built = [] {
    cs_srgb_table(base.tab);
    return true;
  }();
  (void)built;
  CsConst cst = base;
  for (int p = 0; p < CS_MAX_P; ++p) {
    int d[3] = {0, 0, 0}, mag = 0, neg = 0;
    if (p < P)
      for (int c = 0; c < 3; ++c) {
        d[c] = dirs[p * 3 + c];
        mag += d[c] < 0 ? -d[c] : d[c];
        neg += d[c] < 0 ? -d[c] : 0;
      }
    if (mag > 4096) return PPST_EINVAL;
    cst.dir[p][0] = d[0]; cst.dir[p][1] = d[1]; cst.dir[p][2] = d[2]; cst.dir[p][3] = 255 * neg;
  }
  const CsMat M = cs_lab_matrix();
  hipStream_t st = as_stream(stream);
  const int nwc = cs_wave_chunks(H, W), nb = cdiv(nwc, 4) < CS_MAX_BLOCKS ? cdiv(nwc, 4) : CS_MAX_BLOCKS;
  const size_t hist_bytes = (size_t)B * R * P * 256 * sizeof(unsigned);
  if (hipMemsetAsync(hist, 0, hist_bytes, st) != hipSuccess) return (int)hipGetLastError();
  float* consts = (float*)ws;
  float* part = consts + CS_CONST_FLOATS;
  PPST_LAUNCH(cs_setup_kernel, dim3(1), dim3(64), 0, st, cst, consts);
  int rc = PPST_LAUNCH_CHECK();
  if (rc) return rc;
  PPST_LAUNCH(cs_stats_kernel, dim3((unsigned)(B * nb)), dim3(256), (size_t)R * P * 1024, st, (const unsigned char*)img, img_sn, img_sy,
              (const unsigned char*)labels, lab_sn, lab_sy, H * W, make_fastdiv((unsigned)W), R, P, nb, nwc, M, (const float*)consts,
              (unsigned*)hist, part);
  rc = PPST_LAUNCH_CHECK();
  if (rc) return rc;
  PPST_LAUNCH(cs_finish_kernel, dim3((unsigned)(B * R)), dim3(64), 0, st, (const float*)part, R, nwc, (unsigned*)count, (double*)lab_mean,
              (double*)lab_cov);
  return PPST_LAUNCH_CHECK();
}

int ppst_hist_w1(const void* hist_a, int Ba, const void* hist_b, int Bb, const void* pairs, int K, int R, int P, void* num,
                 void* stream) {
  if (Ba < 0 || Bb < 0 || K < 0 || R < 1 || R > CS_MAX_R || P < 1 || P > CS_MAX_P || (int64_t)K * R * P > 0x7FFFFFFFll) return PPST_EINVAL;
  if (K == 0) return PPST_OK;
  if (!hist_a || !hist_b || !pairs || !num) return PPST_ENULL;
  PPST_LAUNCH(cs_w1_kernel, dim3((unsigned)(K * R * P)), dim3(64), 0, as_stream(stream), (const unsigned*)hist_a, Ba, (const unsigned*)hist_b, Bb,
              (const int*)pairs, R * P, (long long*)num);
  return PPST_LAUNCH_CHECK();
}

}  // extern "C"
