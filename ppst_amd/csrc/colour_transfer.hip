// Classical per-region colour transfer of uint8 RGB images (include/ppst_hip.h, "colour transfer"): the baselines the
// style-fidelity metrics are read against.
//
// Scheme.
//   lut      one wave per (pair, region, channel), as cs_w1_kernel: lane l holds bins 4 l .. 4 l + 3 of the content's and the
//            style's histogram, a wave scan of the lane totals gives both inclusive cumulative sums; the style's go to LDS
//            (256 words) and every lane bisects them (8 steps) for each of its four levels:
//            LUT[v] = min{u : 2 cumS(u) nC >= (cumC(v - 1) + cumC(v)) nS}, the products in int64; one dword of four levels
//            per lane.
//   apply    blocks of 4096 consecutive pixels of ONE image; a thread owns quads of four consecutive pixels: three dwords of
//            RGB and one dword of labels in, three dwords out (the dwords sit at any byte address: a crop view starts its rows
//            anywhere, and H * W * 3 need not be a multiple of four).  A quad that crosses a row end of a view, or the end of
//            the image, is read pixel by pixel (and the image's last, partial quad is written so).  The maps of the image are
//            staged in LDS first: the LUTs (R * 768 bytes), or the affine rows (R * 12 floats) and the 256-entry sRGB table.
//            Every pixel is computed alone, in a fixed order of operations: no atomics, nothing depends on the batch.
#include "common.h"
#include "colour_lab.h"

namespace {

#define CT_MAX_R 4
#define CT_MAX_HW (1 << 22)
#define CT_QUADS 4                               // quads of a thread
#define CT_BLOCK_PIX (256 * 4 * CT_QUADS)        // pixels of a block

typedef unsigned __attribute__((aligned(1))) ct_u32;          // a dword at any byte address

struct CtTab { float tab[256]; };

// block = (pair k, region, channel)
__global__ __launch_bounds__(64) void ct_lut_kernel(const unsigned* __restrict__ hc, int Bc, const unsigned* __restrict__ hs, int Bs,
                                                    const int* __restrict__ pairs, int R, int P, unsigned* __restrict__ out) {
  __shared__ unsigned cum_s[256];
  const int k = (int)blockIdx.x / (R * 3), rc = (int)blockIdx.x - k * (R * 3), r = rc / 3, c = rc - r * 3, lane = threadIdx.x;
  const int i = pairs[2 * k], j = pairs[2 * k + 1];
  uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
  if (i >= 0 && i < Bc && j >= 0 && j < Bs) {                  // (uniform) an index outside reads nothing: the identity table
    a = ((const uint4*)(hc + (((int64_t)i * R + r) * P + c) * 256))[lane];
    b = ((const uint4*)(hs + (((int64_t)j * R + r) * P + c) * 256))[lane];
  }
  const unsigned ca[4] = {a.x, a.x + a.y, a.x + a.y + a.z, a.x + a.y + a.z + a.w};
  const unsigned cb[4] = {b.x, b.x + b.y, b.x + b.y + b.z, b.x + b.y + b.z + b.w};
  unsigned ta = ca[3], tb = cb[3];                             // inclusive scan of the lane totals (n <= 2^22 fits)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned ua = __shfl_up(ta, o, 64), ub = __shfl_up(tb, o, 64);
    if (lane >= o) { ta += ua; tb += ub; }
  }
  const long long nC = (long long)__shfl(ta, 63, 64), nS = (long long)__shfl(tb, 63, 64);
  const unsigned xa = ta - ca[3], xb = tb - cb[3];             // bins before this lane's
#pragma unroll
  for (int q = 0; q < 4; ++q) cum_s[4 * lane + q] = xb + cb[q];
  __syncthreads();
  unsigned word = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long below = (long long)(xa + (q ? ca[q - 1] : 0u)), upto = (long long)(xa + ca[q]);
    const long long rhs = (below + upto) * nS;
    int lo = 0, hi = 255;                                      // cumS(255) = nS and rhs <= 2 nC nS: the set is never empty
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int mid = (lo + hi) >> 1;
      if (2ll * (long long)cum_s[mid] * nC >= rhs) hi = mid; else lo = mid + 1;
    }
    const unsigned u = (nC == 0 || nS == 0) ? (unsigned)(4 * lane + q) : (unsigned)lo;
    word |= u << (8 * q);
  }
  out[(int64_t)blockIdx.x * 64 + lane] = word;
}

// one pixel v = r | g << 8 | b << 16 | label << 24 -> its three new bytes
template <int MODE, bool WT>
__device__ __forceinline__ unsigned ct_pixel(unsigned v, const float (&w)[CT_MAX_R], int R, const unsigned char* __restrict__ lut,
                                             const float* __restrict__ aff, const float* __restrict__ tab, const CsMat& M,
                                             const CsMat& Mi) {
  const unsigned lab = v >> 24, cr = v & 255u, cg = (v >> 8) & 255u, cb = (v >> 16) & 255u;
  if (lab >= (unsigned)R) return v & 0xFFFFFFu;                // no region: the pixel keeps its bytes
  float den = 0.f;
  if (WT) {
#pragma unroll
    for (int r = 0; r < CT_MAX_R; ++r)
      if (r < R) den += w[r];
  }
  const bool blend = WT && den > 0.f;                          // all weights zero: the hard label
  if (MODE == PPST_CT_LUT) {
    const unsigned ch[3] = {cr, cg, cb};
    unsigned o = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      unsigned u;
      if (blend) {
        float num = 0.f;
#pragma unroll
        for (int r = 0; r < CT_MAX_R; ++r)
          if (r < R) num = fmaf(w[r], (float)lut[(r * 3 + c) * 256 + ch[c]], num);
        u = (unsigned)fminf(rintf(num / den), 255.f);
      } else {
        u = lut[(lab * 3 + c) * 256 + ch[c]];
      }
      o |= u << (8 * c);
    }
    return o;
  }
  float k[12];
  if (blend) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      float num = 0.f;
#pragma unroll
      for (int r = 0; r < CT_MAX_R; ++r)
        if (r < R) num = fmaf(w[r], aff[r * 12 + i], num);
      k[i] = num / den;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) k[i] = aff[lab * 12 + i];
  }
  const CsLab q = cs_lab(tab, M, cr, cg, cb);
  const float L = fmaf(k[0], q.L, fmaf(k[1], q.a, fmaf(k[2], q.b, k[9])));
  const float A = fmaf(k[3], q.L, fmaf(k[4], q.a, fmaf(k[5], q.b, k[10])));
  const float Bv = fmaf(k[6], q.L, fmaf(k[7], q.a, fmaf(k[8], q.b, k[11])));
  return cs_lab_to_rgb(Mi, L, A, Bv);
}

template <int MODE, bool WT>
__global__ __launch_bounds__(256) void ct_apply_kernel(const unsigned char* __restrict__ img, int64_t sn, int64_t sy,
                                                       const unsigned char* __restrict__ labels, int64_t ln, int64_t ly, int HW, int W,
                                                       FastDiv d_w, int R, int nb, const void* __restrict__ maps,
                                                       const float* __restrict__ wts, unsigned char* __restrict__ out, CsMat M, CsMat Mi,
                                                       CtTab T) {
  __shared__ __attribute__((aligned(16))) unsigned char s_lut[MODE == PPST_CT_LUT ? CT_MAX_R * 768 : 16];
  __shared__ float s_aff[MODE == PPST_CT_LUT ? 4 : CT_MAX_R * 12];
  __shared__ float s_tab[MODE == PPST_CT_LUT ? 4 : 256];
  const int tid = threadIdx.x;
  const int n = (int)blockIdx.x / nb, j = (int)blockIdx.x - n * nb;
  if (MODE == PPST_CT_LUT) {
    const unsigned* src = (const unsigned*)maps + (int64_t)n * R * 192;       // (B, R, 3, 256) bytes: 192 dwords a region
    for (int i = tid; i < R * 192; i += 256) ((unsigned*)s_lut)[i] = src[i];
  } else {
    const float* src = (const float*)maps + (int64_t)n * R * 12;
    if (tid < R * 12) s_aff[tid] = src[tid];
    s_tab[tid] = T.tab[tid];
  }
  __syncthreads();
  const unsigned char* im = img + n * sn;
  const unsigned char* lb = labels ? labels + n * ln : nullptr;
  unsigned char* po = out + (int64_t)n * HW * 3;
  const float* pw = WT ? wts + (int64_t)n * R * HW : nullptr;
#pragma unroll 1
  for (int t = 0; t < CT_QUADS; ++t) {
    const unsigned e0 = ((unsigned)(j * CT_QUADS + t) * 256u + (unsigned)tid) * 4u;
    if (e0 >= (unsigned)HW) break;
    unsigned x0;
    const unsigned y0 = fd_divmod(e0, d_w, x0);
    const bool whole = e0 + 3u < (unsigned)HW;
    unsigned px[4];
    if (whole && x0 + 3u < (unsigned)W) {                      // four pixels of one row: three dwords and one
      const ct_u32* p = (const ct_u32*)(im + y0 * sy + x0 * 3);
      const unsigned d0 = p[0], d1 = p[1], d2 = p[2];
      const unsigned l4 = lb ? *(const ct_u32*)(lb + y0 * ly + x0) : 0u;
      px[0] = (d0 & 0xFFFFFFu) | (l4 << 24);
      px[1] = (((d0 >> 24) | (d1 << 8)) & 0xFFFFFFu) | ((l4 >> 8) << 24);
      px[2] = (((d1 >> 16) | (d2 << 16)) & 0xFFFFFFu) | ((l4 >> 16) << 24);
      px[3] = (d2 >> 8) | ((l4 >> 24) << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned e = e0 + i;
        unsigned v = 0xFF000000u;                              // beyond the image: no region
        if (e < (unsigned)HW) {
          unsigned x;
          const unsigned y = fd_divmod(e, d_w, x);
          const unsigned char* p = im + y * sy + x * 3;
          v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((lb ? (unsigned)lb[y * ly + x] : 0u) << 24);
        }
        px[i] = v;
      }
    }
    unsigned o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float w[CT_MAX_R] = {0.f, 0.f, 0.f, 0.f};
      if (WT && e0 + i < (unsigned)HW) {
#pragma unroll
        for (int r = 0; r < CT_MAX_R; ++r)
          if (r < R) w[r] = pw[(int64_t)r * HW + e0 + i];
      }
      o[i] = ct_pixel<MODE, WT>(px[i], w, R, s_lut, s_aff, s_tab, M, Mi);
    }
    unsigned char* q = po + (int64_t)e0 * 3;
    if (whole) {
      ct_u32* qd = (ct_u32*)q;
      qd[0] = o[0] | (o[1] << 24);
      qd[1] = (o[1] >> 8) | (o[2] << 16);
      qd[2] = (o[2] >> 16) | (o[3] << 8);
    } else {
      for (int i = 0; i < 4 && e0 + i < (unsigned)HW; ++i) {
        q[3 * i] = (unsigned char)o[i]; q[3 * i + 1] = (unsigned char)(o[i] >> 8); q[3 * i + 2] = (unsigned char)(o[i] >> 16);
      }
    }
  }
}

}  // namespace

extern "C" {

int ppst_hist_match_lut(const void* hist_c, int Bc, const void* hist_s, int Bs, const void* pairs, int K, int R, int P, void* luts,
                        void* stream) {
  if (Bc < 0 || Bs < 0 || K < 0 || R < 1 || R > CT_MAX_R || P < 3 || P > 16 || (int64_t)K * R * 3 > 0x7FFFFFFFll) return PPST_EINVAL;
  if (K == 0) return PPST_OK;
  if (!hist_c || !hist_s || !pairs || !luts) return PPST_ENULL;
  PPST_LAUNCH(ct_lut_kernel, dim3((unsigned)(K * R * 3)), dim3(64), 0, as_stream(stream), (const unsigned*)hist_c, Bc,
              (const unsigned*)hist_s, Bs, (const int*)pairs, R, P, (unsigned*)luts);
  return PPST_LAUNCH_CHECK();
}

int ppst_colour_transfer_apply(const void* img, int64_t img_sn, int64_t img_sy, int64_t img_sx, const void* labels, int64_t lab_sn,
                               int64_t lab_sy, int B, int H, int W, int R, int mode, const void* maps, const void* weights, void* out,
                               void* stream) {
  if (B < 0 || H < 1 || W < 1 || (int64_t)H * W > CT_MAX_HW || R < 1 || R > CT_MAX_R || img_sx != 3 ||
      (mode != PPST_CT_LUT && mode != PPST_CT_AFFINE))
    return PPST_EINVAL;
  const int HW = H * W, nb = cdiv(HW, CT_BLOCK_PIX);
  if ((int64_t)B * nb > 0x7FFFFFFFll) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!img || !maps || !out) return PPST_ENULL;
  static CtTab tab;                                            // built once (the same values every time)
  static const bool built = [] { cs_srgb_table(tab.tab); return true; }();
  (void)built;
  const CsMat M = cs_lab_matrix(), Mi = cs_lab_inverse_matrix();
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(B * nb));
#define CT_GO(MODE_, WT_)                                                                                                       \
  PPST_LAUNCH((ct_apply_kernel<MODE_, WT_>), grid, dim3(256), 0, st, (const unsigned char*)img, img_sn, img_sy,                 \
              (const unsigned char*)labels, lab_sn, lab_sy, HW, W, make_fastdiv((unsigned)W), R, nb, maps, (const float*)weights, \
              (unsigned char*)out, M, Mi, tab)
  if (mode == PPST_CT_LUT) { if (weights) CT_GO(PPST_CT_LUT, true); else CT_GO(PPST_CT_LUT, false); }
  else { if (weights) CT_GO(PPST_CT_AFFINE, true); else CT_GO(PPST_CT_AFFINE, false); }
#undef CT_GO
  return PPST_LAUNCH_CHECK();
}

}  // extern "C"
