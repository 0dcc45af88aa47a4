// Colour-guided filter post-process of PPSTModel.decode (models/ppst_model.py:288-306 ->
// photo_gif.py:25-46 -> cv2.ximgproc.guidedFilter(guide=content, src=output, radius, eps)).
// The arithmetic lives in opencv-contrib 4.8.1.78, which is not vendored by the reference:
// this restates the published algorithm (He et al., as OpenCV implements it: fp32 work type,
// normalised (2r+1)^2 box mean with BORDER_REFLECT, eps on the covariance diagonal, 3x3
// symmetric inverse by cofactors, cvRound + saturate to uint8).  PARITY UNPINNED against
// OpenCV itself; pinned against oracle/ppst_oracle.py:guided_filter_color.
//
// Two pipelines, chosen by the radius (ppst_guided_filter at the end of the file):
//   r == 30 (the path's radius, photo_gif.py:43), r == 60 and r == 90 (30 * side / 512 for 1024^2 and 1536^2 images,
//     ppst_model.guided_filter_radius): TWO fused launches that keep every box sum on the chip --
//     gf_s1_fused (uint8 -> exact uint32 moment sums -> 3x3 solve -> 12 half planes (a, b)), gf_s2_fused (means of (a, b),
//     q = sum a_k I_k + b, round; uint8 + fp32 NCHW (q/255-0.5)*2).  Described at the kernels; each radius has its own strip geometry.
//   every other radius up to GF_MAXR: the PLANE ROUTE (gf_plane_route) and gf_v_final (means of a, b; q; round; the two outputs).
// The plane route: four launches of separable direct sums (no running sums: order-independent fp32 error) over [B][plane][H][W]
// fp32 planes in the caller's workspace, which leave the h-summed coefficient planes for the caller's last V pass --
//     gf_h<source> (NM h-sums of the moments; one block per image row, row staged in LDS, reflected)
//     gf_v         (NM means; lanes along x (coalesced), 2r+1 row reads per output served by L1/L2)
//     solve        (-> 4 NC planes a_c[3], b_c)
//     gf_h<planes> (4 NC h-sums)
// It serves three entries.  ppst_guided_filter: a colour source (NM = 21 moments: I(3), p(3), I_i*I_j(6), I_i*p_c(9); NC = 3), the
// V pass with a float accumulator and the contracting gf_solve_kernel, which keep this entry's bytes.  ppst_guided_filter_coeffs
// (native-size output, below) and ppst_guided_matte_coeffs (a ONE-channel source, He et al.'s guided feathering -- the refined alpha
// is a . I + b: NM = 13, NC = 1) run the EXACT forms and end in an exact V pass into the caller's buffer.  Their planes are judged
// ALONE against float64 (twice the error of a float32 run whose window means are float64 means rounded once,
// tests/gf_native_cases.py:plane_ref), and the first forms do not meet that: the float V pass sums 2r + 1 row sums in fp32 (exact only
// up to r = 7: 255^2 (2r + 1)^2 < 2^24) and multiplies by a ROUNDED 1 / (2r + 1)^2, gf_solve_kernel compiles with contraction, and an
// ill-conditioned covariance amplifies both (measured with them: 3.39e-3 against a bar of 2.47e-3 at r = 7, 2.65e-4 against 2.50e-4
// at r = 30).  Exact: gf_v<double> accumulates in double and divides once, rounded once -- on the integer moment sums of stage 1
// (every stage-1 value is an integer <= 255^2 and a row sum <= 255^2 (2 GF_MAXR + 1) < 2^24: exact in fp32 in any order) the mean is
// the correctly rounded one; gf_solve_exact_kernel is gf_solve_kernel's text (the shared GF_SOLVE_* macros, six divisions) with
// contraction off: every operation rounds once, in the order written.
// The matte source is the fp32 matte quantised on load, p = rint(255 clamp(m, 0, 1)) (fmaxf drops a NaN: 0), an integer in 0..255,
// and its 13 moments are those of the colour source (p, p, p) with P1, P2 and their products left out (GFM_PLANE).  Every operation
// is the one the 21-plane entry performs on channel 0, in its order, so the result is BIT-EQUAL to planes 0..3 of
// ppst_guided_filter_coeffs on the source (p, p, p): a matte does not depend on the entry that computed it.
// The round-4 sliding-window forms of the radius-30 path (three and four launches through fp32 planes) were removed from the source;
// bc82816 is the last commit that holds them, their measurements are in DESIGN.md section 4.
#include "common.h"

#define GF_MAXW 2048
#define GF_MAXR 64

__device__ __forceinline__ int reflect_idx(int i, int n) {  // cv2.BORDER_REFLECT (edge pixel repeated)
  if (i < 0) i = -i - 1;
  if (i >= n) i = 2 * n - 1 - i;
  return i;
}

// plane value for stage 1 from the guide (I) and source (P) bytes of one pixel: THE table of the 21 moments
__device__ __forceinline__ float gf_plane_value(int pl, float I0, float I1, float I2, float P0, float P1, float P2) {
  switch (pl) {
    case 0: return I0; case 1: return I1; case 2: return I2;
    case 3: return P0; case 4: return P1; case 5: return P2;
    case 6: return I0 * I0; case 7: return I0 * I1; case 8: return I0 * I2;
    case 9: return I1 * I1; case 10: return I1 * I2; case 11: return I2 * I2;
    default: {
      int k = pl - 12, c = k / 3, i = k - c * 3;  // 12 + c*3 + i = I_i * p_c
      float Iv = i == 0 ? I0 : (i == 1 ? I1 : I2);
      float Pv = c == 0 ? P0 : (c == 1 ? P1 : P2);
      return Iv * Pv;
    }
  }
}
// A one-channel source needs 13 of them -- plane 0..2 I, 3 p, 4..9 I_i I_j, 10..12 I_i p: the 21-plane order with P1, P2 and their
// products left out.  GFM_PLANE: moment i of the 21 -> its plane among the 13 (i < 4 or i >= 6); GFM_MOMENT: the inverse.
#define GFM_PLANE(i) ((i) < 4 ? (i) : (i) - 2)
#define GFM_MOMENT(j) ((j) < 4 ? (j) : (j) + 2)

// the same 21 planes of one pixel as exact integers (plane order as above), from its six bytes
__device__ __forceinline__ void gf_moments(unsigned I0, unsigned I1, unsigned I2, unsigned P0, unsigned P1, unsigned P2, unsigned (&m)[21]) {
  m[0] = I0; m[1] = I1; m[2] = I2; m[3] = P0; m[4] = P1; m[5] = P2;
  m[6] = __umul24(I0, I0); m[7] = __umul24(I0, I1); m[8] = __umul24(I0, I2);
  m[9] = __umul24(I1, I1); m[10] = __umul24(I1, I2); m[11] = __umul24(I2, I2);
  m[12] = __umul24(I0, P0); m[13] = __umul24(I1, P0); m[14] = __umul24(I2, P0);
  m[15] = __umul24(I0, P1); m[16] = __umul24(I1, P1); m[17] = __umul24(I2, P1);
  m[18] = __umul24(I0, P2); m[19] = __umul24(I1, P2); m[20] = __umul24(I2, P2);
}

// The per-pixel 3x3 solve, stated once.  M(i) names the i-th of the 21 window means.  GF_SOLVE_DET declares the means of the guide,
// the covariance (+ eps on its diagonal), its cofactors c.. and the determinant det; the caller then forms the inverse i.. from them
// in ITS way -- gf_solve_kernel by six divisions, gf_s1_fused_kernel by one reciprocal: the two differ in the last bit and each path
// keeps its bytes; GF_SOLVE_AB(M, c) declares (A0, A1, A2, bb) = (a_c0, a_c1, a_c2, b_c) of output channel c.
// (Macros, not force-inlined functions: with hipcc 7.x such a function -- taking the means as an array or through a loader -- changes
//  the register count of gf_solve_kernel (49 VGPRs / 46 SGPRs) or the instruction stream of gf_s1_fused_kernel; as text both kernels
//  compile to the streams they had.)
#define GF_SOLVE_DET(M, eps)                                                                                                     \
  const float mI0 = M(0), mI1 = M(1), mI2 = M(2);                                                                                \
  const float a00 = M(6) - mI0 * mI0 + eps, a01 = M(7) - mI0 * mI1, a02 = M(8) - mI0 * mI2;                                      \
  const float a11 = M(9) - mI1 * mI1 + eps, a12 = M(10) - mI1 * mI2, a22 = M(11) - mI2 * mI2 + eps;                              \
  const float c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;                             \
  const float c11 = a00 * a22 - a02 * a02, c12 = a02 * a01 - a00 * a12, c22 = a00 * a11 - a01 * a01;                             \
  const float det = a00 * c00 + a01 * c01 + a02 * c02
#define GF_SOLVE_AB(M, c)                                                                                                        \
  const float mp_c = M(3 + (c));                                                                                                 \
  const float cp0 = M(12 + (c) * 3 + 0) - mI0 * mp_c, cp1 = M(12 + (c) * 3 + 1) - mI1 * mp_c, cp2 = M(12 + (c) * 3 + 2) - mI2 * mp_c; \
  const float A0 = i00 * cp0 + i01 * cp1 + i02 * cp2;                                                                            \
  const float A1 = i01 * cp0 + i11 * cp1 + i12 * cp2;                                                                            \
  const float A2 = i02 * cp0 + i12 * cp1 + i22 * cp2;                                                                            \
  const float bb = mp_c - A0 * mI0 - A1 * mI1 - A2 * mI2

// channel c of the output pixel (b, y, x): round like cv2 (saturate_cast<uchar>(cvRound)); either output may be absent
__device__ __forceinline__ void gf_store(float qv, float* out, unsigned char* out_u8, int64_t b, int c, int y, int x, int H, int W, int64_t P) {
  const float rq = fminf(fmaxf(rintf(qv), 0.f), 255.f);
  if (out_u8) out_u8[((b * H + y) * W + x) * 3 + c] = (unsigned char)rq;
  if (out) out[(b * 3 + c) * P + (int64_t)y * W + x] = (rq / 255.0f - 0.5f) * 2.f;  // ToTensor, (x-0.5)*2 (ppst_model.py:301-303)
}

// H pass.  grid = (H, nplanes, B).  ``src`` by SRC: [B][nplanes][H][W] fp32 planes (the guide is not read); a uint8 colour source
// [B][H][W][3] beside the guide; an fp32 matte [B][H][W] beside the guide.
#define GF_SRC_PLANES 0
#define GF_SRC_COLOUR 1
#define GF_SRC_MATTE 2
template <int SRC>
__global__ __launch_bounds__(256) void gf_h_kernel(const unsigned char* __restrict__ guide, const void* __restrict__ src,
                                                   float* __restrict__ out, int H, int W, int r, int nplanes) {
  __shared__ float row[GF_MAXW + 2 * GF_MAXR];
  const int y = blockIdx.x, pl = blockIdx.y, b = blockIdx.z;
  const int64_t P = (int64_t)H * W;
  for (int i = threadIdx.x; i < W + 2 * r; i += 256) {
    const int x = reflect_idx(i - r, W);
    const int64_t o = ((int64_t)b * H + y) * W + x;
    float v;
    if (SRC == GF_SRC_PLANES) {
      v = ((const float*)src)[((int64_t)b * nplanes + pl) * P + (int64_t)y * W + x];
    } else {
      const unsigned char* g = guide + o * 3;
      if (SRC == GF_SRC_COLOUR) {
        const unsigned char* s = (const unsigned char*)src + o * 3;
        v = gf_plane_value(pl, g[0], g[1], g[2], s[0], s[1], s[2]);
      } else {
        const float p = rintf(255.f * fminf(fmaxf(((const float*)src)[o], 0.f), 1.f));
        v = gf_plane_value(GFM_MOMENT(pl), g[0], g[1], g[2], p, p, p);
      }
    }
    row[i] = v;
  }
  __syncthreads();
  float* o = out + ((int64_t)b * nplanes + pl) * P + (int64_t)y * W;
  for (int x = threadIdx.x; x < W; x += 256) {
    float s = 0.f;
    for (int k = 0; k <= 2 * r; ++k) s += row[x + k];
    o[x] = s;
  }
}

// V pass: out = (sum over 2r+1 rows of in) / (2r+1)^2.  grid-stride over (b, plane, y, x).  ACC is the arithmetic: a float
// accumulator times the rounded reciprocal, or a double accumulator and a true division, rounded once (the exact form).
__device__ __forceinline__ float gf_mean(float s, int n2) { return s * (1.f / (float)n2); }
__device__ __forceinline__ float gf_mean(double s, int n2) { return (float)(s / (double)n2); }
template <typename ACC>
__global__ __launch_bounds__(256) void gf_v_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int r,
                                                   int64_t total) {
  const int n2 = (2 * r + 1) * (2 * r + 1);
  const int64_t P = (int64_t)H * W;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int x = (int)(t % W);
    int64_t q = t / W;
    int y = (int)(q % H);
    int64_t bp = q / H;
    const float* col = in + bp * P + x;
    ACC s = 0;
    for (int k = -r; k <= r; ++k) s += (ACC)col[(int64_t)reflect_idx(y + k, H) * W];
    out[t] = gf_mean(s, n2);
  }
}

// per-pixel 3x3 solve.  means: [B][21][P] -> ab: [B][12][P] (a_c0,a_c1,a_c2,b_c for c=0..2)
__global__ __launch_bounds__(256) void gf_solve_kernel(const float* __restrict__ m, float* __restrict__ ab, int64_t P, float eps,
                                                       int64_t total) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int64_t b = t / P, p = t - b * P;
    const float* mp = m + b * 21 * P + p;
#define GF_M(i) mp[(i) * P]
    GF_SOLVE_DET(GF_M, eps);
    const float i00 = c00 / det, i01 = c01 / det, i02 = c02 / det, i11 = c11 / det, i12 = c12 / det, i22 = c22 / det;
    float* o = ab + b * 12 * P + p;
    for (int c = 0; c < 3; ++c) {
      GF_SOLVE_AB(GF_M, c);
      o[(c * 4 + 0) * P] = A0; o[(c * 4 + 1) * P] = A1; o[(c * 4 + 2) * P] = A2; o[(c * 4 + 3) * P] = bb;
#undef GF_M
    }
  }
}

// The same solve with contraction off (the pragma is lexical, which is why gf_solve_kernel is not an instance of this template:
// it keeps its contracted bytes).  means: [B][NM][P], the 21 moments (NM = 21) or the 13 of a one-channel source (GFM_PLANE)
// -> ab: [B][4 NC][P] for the NC = 3 or 1 channels of the source.
template <int NM, int NC>
__global__ __launch_bounds__(256) void gf_solve_exact_kernel(const float* __restrict__ m, float* __restrict__ ab, int64_t P, float eps,
                                                             int64_t total) {
#pragma clang fp contract(off)
  static_assert((NM == 21 && NC == 3) || (NM == 13 && NC == 1), "moment planes of a colour or a one-channel source");
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int64_t b = t / P, p = t - b * P;
    const float* mp = m + b * NM * P + p;
#define GF_M(i) mp[(NM == 21 ? (i) : GFM_PLANE(i)) * P]
    GF_SOLVE_DET(GF_M, eps);
    const float i00 = c00 / det, i01 = c01 / det, i02 = c02 / det, i11 = c11 / det, i12 = c12 / det, i22 = c22 / det;
    float* o = ab + b * 4 * NC * P + p;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      GF_SOLVE_AB(GF_M, c);
      o[(c * 4 + 0) * P] = A0; o[(c * 4 + 1) * P] = A1; o[(c * 4 + 2) * P] = A2; o[(c * 4 + 3) * P] = bb;
    }
#undef GF_M
  }
}

// The plane route, H1 -> V -> solve -> H2, for a source of kind SRC with NM moment planes and NC channels; EXACT chooses the V pass
// and the solve (the header comment).  It owns the argument rule the three entries share (``dst`` stands for the caller's output
// and is only tested), the split of the workspace ([B][NM][P] twice) and the launches.  On PPST_OK *hs is the h-summed
// coefficient planes [B][4 NC][P] for the caller's last V pass -- or null when B == 0 and nothing was launched.
static unsigned gf_blocks_for(int64_t total) { int64_t b = cdiv64(total, 256); return (unsigned)(b > 256 * 32 ? 256 * 32 : b); }

template <int SRC, int NM, int NC, bool EXACT>
static int gf_plane_route(hipStream_t st, const void* guide_u8, const void* src, const void* dst, void* work, int B, int H, int W, int r,
                          float eps, const float** hs) {
  static_assert(EXACT || (NM == 21 && NC == 3), "gf_solve_kernel solves the colour source");
  *hs = nullptr;
  if (B < 0 || H <= 0 || W <= 0 || W > GF_MAXW || r <= 0 || r > GF_MAXR || r >= H || r >= W) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!guide_u8 || !src || !dst || !work) return PPST_ENULL;
  const int64_t P = (int64_t)H * W, tm = (int64_t)B * NM * P;
  const unsigned char* g = (const unsigned char*)guide_u8;
  float* bufA = (float*)work;  // [B][NM][P]
  float* bufB = bufA + tm;     // [B][NM][P]
  int e;
  PPST_LAUNCH(gf_h_kernel<SRC>, dim3(H, NM, B), dim3(256), 0, st, g, src, bufA, H, W, r, NM);
  if ((e = PPST_LAUNCH_CHECK())) return e;
  PPST_LAUNCH((gf_v_kernel<std::conditional_t<EXACT, double, float>>), dim3(gf_blocks_for(tm)), dim3(256), 0, st, (const float*)bufA, bufB,
              H, W, r, tm);
  if ((e = PPST_LAUNCH_CHECK())) return e;
  if constexpr (EXACT) PPST_LAUNCH((gf_solve_exact_kernel<NM, NC>), dim3(gf_blocks_for(B * P)), dim3(256), 0, st, (const float*)bufB, bufA, P, eps, (int64_t)B * P);
  else PPST_LAUNCH(gf_solve_kernel, dim3(gf_blocks_for(B * P)), dim3(256), 0, st, (const float*)bufB, bufA, P, eps, (int64_t)B * P);
  if ((e = PPST_LAUNCH_CHECK())) return e;
  PPST_LAUNCH(gf_h_kernel<GF_SRC_PLANES>, dim3(H, 4 * NC, B), dim3(256), 0, st, g, (const void*)bufA, bufB, H, W, r, 4 * NC);
  if ((e = PPST_LAUNCH_CHECK())) return e;
  *hs = bufB;
  return PPST_OK;
}

// final V pass over the 12 h-summed (a,b) planes + combination with the guide.
__global__ __launch_bounds__(256) void gf_v_final_kernel(const float* __restrict__ hs, const unsigned char* __restrict__ guide,
                                                         float* __restrict__ out, unsigned char* __restrict__ out_u8, int H, int W,
                                                         int r, int64_t total) {
  const float inv = 1.f / (float)((2 * r + 1) * (2 * r + 1));
  const int64_t P = (int64_t)H * W;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int x = (int)(t % W);
    int64_t q = t / W;
    int y = (int)(q % H);
    int64_t b = q / H;
    float m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = 0.f;
    const float* base = hs + b * 12 * P + x;
    for (int k = -r; k <= r; ++k) {
      int64_t ro = (int64_t)reflect_idx(y + k, H) * W;
#pragma unroll
      for (int i = 0; i < 12; ++i) m[i] += base[i * P + ro];
    }
    const unsigned char* g = guide + ((b * H + y) * W + x) * 3;
    float I0 = g[0], I1 = g[1], I2 = g[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float qv = (m[c * 4] * inv) * I0 + (m[c * 4 + 1] * inv) * I1 + (m[c * 4 + 2] * inv) * I2 + m[c * 4 + 3] * inv;
      gf_store(qv, out, out_u8, b, c, y, x, H, W, P);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// The filter at the radii RR = 30, 60 and 90 in TWO launches that keep every box sum on the chip (round 5; round-4 verdict: 439 B /
// pixel of HBM traffic by counter against 9 B / pixel algorithmic -- the three-launch form handed 21 + 12 fp32 planes through HBM and
// re-read them).  The kernels are templates on RR; the strip geometry of each radius is GfGeom<RR> below (figures in this comment are
// radius 30's where they name one).
// The windows SLIDE: after a first direct sum of 2 RR + 1 values the next window adds the entering and subtracts the leaving one.
//   * the 21 moment planes of stage 1 are INTEGERS: row and column sums run in uint32 -- a window sum is at most 255^2 (2 RR + 1)^2
//     (< 2^28 at RR = 30, 2.13e9 < 2^32 at RR = 90; exact up to RR = 127, which the kernel asserts) -- exact whatever the order, and the
//     mean is formed from the exact sum (the direct fp32 sums of the generic path, and of the oracle, carry ~1e-7 relative rounding there);
//   * the (a, b) planes of stage 2 are floats: a horizontal window slides over at most SEG - 1 = 15 steps (every geometry below has
//     SEG = 16) before the next thread starts from a direct sum again, a vertical one over at most VS - 1 rows: the drift is bounded
//     by that many roundings of a sum of 2 RR + 1 terms.
// Bar: <= 1 uint8 LSB against the oracle (tests/gpu_diag.py:t_guided); against float64: tests/test_gpu_guided_filter*.py.
//   gf_s1_fused_kernel: a block owns WC output columns (+ RR on both sides: 192 + 60 = 252 of its 256 threads at RR = 30) and VS rows.
//     Thread = column: its 21 vertical window sums live in REGISTERS and slide down the rows (the entering / leaving row's moments formed
//     from the 6 uint8 bytes of the pixel, exact uint32); per row the column sums go to LDS, 21 x WC / SEG threads slide the horizontal
//     window over SEG-output segments (exact uint32), the window sums go back to LDS and thread = pixel solves its 3x3 system.
//     Only (a, b) leave the kernel -- as 12 IEEE-half planes (24 B / pixel; they feed a (2 RR + 1)^2 mean): each thread carries the
//     rounding residual of every value down its column (error diffusion), so a vertical window sum of the stored halves differs from
//     the fp32 sum by at most the two end residuals of every run of VS rows it spans -- not 2 RR + 1 correlated roundings (a flat
//     image region rounds every b alike).
//   gf_s2_fused_kernel: the same structure over the 12 half planes (fp32 sums, sliding with the bounded drift above), ending in
//     q = mean(a) . I + mean(b), rounded to uint8 like cv2 (saturate_cast<uchar>(cvRound)).
// Borders: reflect_idx reflects ONCE, which is enough because the entry point requires r < H and r < W, for every radius.
// Half overflow of b at small eps applies to RR = 60 and 90 exactly as to RR = 30: the stored half of a |b| > 65504 is
// infinite.  The clamp is not part of these kernels at any radius.
// HBM traffic per pixel: 6 B x halo factors in, 24 out; 24 x ((WC + 2 RR) / WC columns x (VS2 + 2 RR) / VS2 rows) in, 3 guide,
// 12 (+ 3) out -- at RR = 30: 1.31 columns x (VS2 + 60) / VS2 rows.
// Strip geometry per radius: NT threads per block (= columns a block reads: WC outputs + RR on both sides, the rest idle), WC
// output columns per strip, SEG outputs per sliding segment.  WC + 2 RR <= NT, WC a multiple of SEG, one horizontal item per
// (plane, segment) and thread: 21 WC / SEG <= NT.  UNR: unroll count of a segment's first direct sum, 0 = the compiler's choice.
// Radius 30 keeps the compiler's choice (it unrolls all 61 reads; 168 VGPRs, three blocks of 256 per CU); left alone at RR = 60 it
// unrolls all 121 and needs 219 / 223 VGPRs -- two waves per SIMD, ONE block of 384 per CU -- where UNR = 16 needs 145 / 100.
// (How each geometry was chosen: the table at ppst_guided_filter.)
template <int RR> struct GfGeom;
template <> struct GfGeom<30> { static constexpr int NT = 256, WC = 192, SEG = 16, UNR = 0; };
template <> struct GfGeom<60> { static constexpr int NT = 384, WC = 256, SEG = 16, UNR = 16; };
template <> struct GfGeom<90> { static constexpr int NT = 512, WC = 320, SEG = 16, UNR = 16; };
// LDS row index with one pad slot per 16 entries: lanes are 16 entries apart (one segment each) -- unpadded, all of a wave's
// reads fall on two banks
#define GF_ROW(i) ((i) + ((i) >> 4))

// The horizontal pass of both fused kernels, stated once: thread (plane ipl, segment iseg) forms the window sums of the GF_SEG outputs
// j0 .. j0 + 15 of its plane over the padded LDS rows col[ipl] -> win[ipl] (output j covers entries j .. j + 2 RR): the first is a
// direct sum, each next one adds the entering and subtracts the leaving entry.  T is the element type: unsigned in stage 1 (exact),
// float in stage 2 (same summation order in both).
// (A macro, not a force-inlined function template: with hipcc 7.x such a function -- taking pointers, the LDS arrays by reference,
//  or (col, win, ipl, iseg) -- compiles gf_s1_fused_kernel to 172 and gf_s2_fused_kernel to 170 VGPRs against 168, which costs the
//  third resident block per CU; as text both kernels compile to the streams they had.)
#define GF_SLIDE_SEGMENT(T, RR, SEG, col, win, ipl, iseg)                              \
  do {                                                                                 \
    const T* r = col[ipl];                                                             \
    T* wv = win[ipl];                                                                  \
    const int j0 = (iseg) * SEG;                                                       \
    T sum = 0;                                                                         \
    if constexpr (GfGeom<RR>::UNR == 0) {                                              \
      for (int k = 0; k <= 2 * RR; ++k) sum += r[GF_ROW(j0 + k)];                      \
    } else {                                                                           \
      _Pragma("unroll (GfGeom<RR>::UNR)") for (int k = 0; k <= 2 * RR; ++k) sum += r[GF_ROW(j0 + k)]; \
    }                                                                                  \
    wv[GF_ROW(j0)] = sum;                                                              \
    _Pragma("unroll") for (int j = 1; j < SEG; ++j) {                                  \
      sum += r[GF_ROW(j0 + j + 2 * RR)] - r[GF_ROW(j0 + j - 1)];                       \
      wv[GF_ROW(j0 + j)] = sum;                                                        \
    }                                                                                  \
  } while (0)

template <int RR, int VS>
__global__ __launch_bounds__(GfGeom<RR>::NT) void gf_s1_fused_kernel(const unsigned char* __restrict__ guide, const unsigned char* __restrict__ src,
                                                          unsigned short* __restrict__ ab, int H, int W, float eps) {
  constexpr int GS_NT = GfGeom<RR>::NT, GS_WC = GfGeom<RR>::WC, GF_SEG = GfGeom<RR>::SEG, GS_NSEG = GS_WC / GF_SEG;
  static_assert(GS_WC + 2 * RR <= GS_NT && GS_WC % GF_SEG == 0 && 21 * GS_NSEG <= GS_NT, "strip geometry");
  static_assert(RR <= 127, "a uint32 window sum holds 255^2 (2 RR + 1)^2 up to RR = 127");
  __shared__ unsigned col[21][GF_ROW(GS_NT) + 1];
  __shared__ unsigned win[21][GF_ROW(GS_WC) + 1];
  const int t = threadIdx.x, x0 = blockIdx.x * GS_WC, y0 = blockIdx.y * VS, b = blockIdx.z;
  const int64_t P = (int64_t)H * W;
  const int xc = reflect_idx(min(x0 - RR + t, W - 1 + RR), W);          // (columns past the image's reflected margin are never used)
  const unsigned char* gp = guide + ((int64_t)b * P + xc) * 3;
  const unsigned char* sp = src + ((int64_t)b * P + xc) * 3;
  unsigned cs[21];
#pragma unroll
  for (int pl = 0; pl < 21; ++pl) cs[pl] = 0;
  struct Px { unsigned I0, I1, I2, P0, P1, P2; };
  auto fetch = [&](int y) __attribute__((always_inline)) -> Px {
    const int64_t o = (int64_t)reflect_idx(y, H) * W * 3;
    return Px{gp[o], gp[o + 1], gp[o + 2], sp[o], sp[o + 1], sp[o + 2]};
  };
  auto apply = [&](const Px& q, bool add) __attribute__((always_inline)) {
    unsigned m[21];
    gf_moments(q.I0, q.I1, q.I2, q.P0, q.P1, q.P2, m);
#pragma unroll
    for (int pl = 0; pl < 21; ++pl) cs[pl] = add ? cs[pl] + m[pl] : cs[pl] - m[pl];
  };
  for (int k = -RR; k <= RR; ++k) apply(fetch(y0 + k), true);
  const int y1 = min(y0 + VS, H);
  const int ipl = t % 21, iseg = t / 21;                                 // horizontal item of this thread: (plane, 16-output segment)
  const bool pix_ok = t < GS_WC && x0 + t < W;
  const float inv = 1.f / (float)((2 * RR + 1) * (2 * RR + 1));
  float res[12];                                                         // rounding residuals carried down the column
#pragma unroll
  for (int i = 0; i < 12; ++i) res[i] = 0.f;
  unsigned short* op = ab + (int64_t)b * 12 * P + x0 + t;
  for (int y = y0; y < y1; ++y) {
    // the bytes of the entering / leaving rows are requested here, ahead of the two LDS phases (a barrier is a fence: hipcc does not
    // move the loads up by itself), and used at the bottom of the iteration.  (Requested a whole iteration earlier still -- two sets in
    // flight -- the kernel was SLOWER, 0.36 -> 0.44 ms per batch: the extra registers cost a resident block per CU, and three co-resident
    // blocks hide the latency better than a deeper prefetch in two.)
    const Px pin = fetch(min(y + 1 + RR, H - 1 + RR)), pout = fetch(y - RR);
#pragma unroll
    for (int pl = 0; pl < 21; ++pl) col[pl][GF_ROW(t)] = cs[pl];
    __syncthreads();
    if (iseg < GS_NSEG) GF_SLIDE_SEGMENT(unsigned, RR, GF_SEG, col, win, ipl, iseg);
    __syncthreads();
    if (pix_ok) {
      float m[21];
#pragma unroll
      for (int pl = 0; pl < 21; ++pl) m[pl] = (float)win[pl][GF_ROW(t)] * inv;
#define GF_M(i) m[i]
      GF_SOLVE_DET(GF_M, eps);
      const float rdet = 1.f / det;          // (one division: gf_solve_kernel's six differ from it in the last bit)
      const float i00 = c00 * rdet, i01 = c01 * rdet, i02 = c02 * rdet, i11 = c11 * rdet, i12 = c12 * rdet, i22 = c22 * rdet;
      float v[12];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        GF_SOLVE_AB(GF_M, c);
        v[c * 4 + 0] = A0; v[c * 4 + 1] = A1; v[c * 4 + 2] = A2; v[c * 4 + 3] = bb;
      }
#undef GF_M
      const int64_t po = (int64_t)y * W;
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        const float want = v[i] + res[i];
        const _Float16 h = (_Float16)want;
        res[i] = want - (float)h;
        op[i * P + po] = __builtin_bit_cast(unsigned short, h);
      }
    }
    if (y + 1 < y1) {
      apply(pin, true);
      apply(pout, false);
    }
  }
}

template <int RR, int VS>
__global__ __launch_bounds__(GfGeom<RR>::NT) void gf_s2_fused_kernel(const unsigned short* __restrict__ ab, const unsigned char* __restrict__ guide,
                                                          float* __restrict__ out, unsigned char* __restrict__ out_u8, int H, int W) {
  constexpr int GS_NT = GfGeom<RR>::NT, GS_WC = GfGeom<RR>::WC, GF_SEG = GfGeom<RR>::SEG, GS_NSEG = GS_WC / GF_SEG;
  static_assert(GS_WC + 2 * RR <= GS_NT && GS_WC % GF_SEG == 0 && 12 * GS_NSEG <= GS_NT, "strip geometry");
  __shared__ float col[12][GF_ROW(GS_NT) + 1];
  __shared__ float win[12][GF_ROW(GS_WC) + 1];
  const int t = threadIdx.x, x0 = blockIdx.x * GS_WC, y0 = blockIdx.y * VS, b = blockIdx.z;
  const int64_t P = (int64_t)H * W;
  const int xc = reflect_idx(min(x0 - RR + t, W - 1 + RR), W);
  const unsigned short* in = ab + (int64_t)b * 12 * P + xc;
  auto ld = [&](int i, int64_t ro) -> float { return (float)__builtin_bit_cast(_Float16, in[i * P + ro]); };
  float s[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = 0.f;
  for (int k = -RR; k <= RR; ++k) {
    const int64_t ro = (int64_t)reflect_idx(y0 + k, H) * W;
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] += ld(i, ro);
  }
  const int y1 = min(y0 + VS, H);
  const int ipl = t % 12, iseg = t / 12;
  const bool pix_ok = t < GS_WC && x0 + t < W;
  const float inv = 1.f / (float)((2 * RR + 1) * (2 * RR + 1));
  for (int y = y0; y < y1; ++y) {
    unsigned short din[12], dout[12];      // entering / leaving row (raw halves), requested ahead of the two LDS phases
    {
      const int64_t rin = (int64_t)reflect_idx(min(y + 1 + RR, H - 1 + RR), H) * W, rout = (int64_t)reflect_idx(y - RR, H) * W;
#pragma unroll
      for (int i = 0; i < 12; ++i) { din[i] = in[i * P + rin]; dout[i] = in[i * P + rout]; }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) col[i][GF_ROW(t)] = s[i];
    __syncthreads();
    if (iseg < GS_NSEG) GF_SLIDE_SEGMENT(float, RR, GF_SEG, col, win, ipl, iseg);
    __syncthreads();
    if (pix_ok) {
      const int x = x0 + t;
      const unsigned char* g = guide + (((int64_t)b * H + y) * W + x) * 3;
      const float I0 = g[0], I1 = g[1], I2 = g[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float qv = (win[c * 4][GF_ROW(t)] * inv) * I0 + (win[c * 4 + 1][GF_ROW(t)] * inv) * I1 + (win[c * 4 + 2][GF_ROW(t)] * inv) * I2 +
                         win[c * 4 + 3][GF_ROW(t)] * inv;
        gf_store(qv, out, out_u8, b, c, y, x, H, W, P);
      }
    }
    if (y + 1 < y1) {
#pragma unroll
      for (int i = 0; i < 12; ++i) s[i] += (float)__builtin_bit_cast(_Float16, din[i]) - (float)__builtin_bit_cast(_Float16, dout[i]);
    }
  }
}

// one launch of each fused kernel with VS rows per block
template <int RR, int VS>
static void gf_s1_launch(hipStream_t st, const unsigned char* g, const unsigned char* s, unsigned short* abh, int B, int H, int W, float eps) {
  PPST_LAUNCH((gf_s1_fused_kernel<RR, VS>), dim3(cdiv(W, GfGeom<RR>::WC), cdiv(H, VS), B), dim3(GfGeom<RR>::NT), 0, st, g, s, abh, H, W, eps);
}
template <int RR, int VS>
static void gf_s2_launch(hipStream_t st, const unsigned short* abh, const unsigned char* g, void* out, void* out_u8, int B, int H, int W) {
  PPST_LAUNCH((gf_s2_fused_kernel<RR, VS>), dim3(cdiv(W, GfGeom<RR>::WC), cdiv(H, VS), B), dim3(GfGeom<RR>::NT), 0, st, abh, g, (float*)out, (unsigned char*)out_u8, H, W);
}

// tuning aid: rows per block of the two fused launches, for all three fused radii (0 = the default of that radius, from the table
// below; 32 / 64 / 128 = forced).  Process-wide; after (0, 0) the defaults reproduce their bytes.
static int g_gf_vs1 = 0, g_gf_vs2 = 0;
extern "C" int ppst_guided_filter_tune(int vs1, int vs2) { g_gf_vs1 = vs1; g_gf_vs2 = vs2; return PPST_OK; }

// (42 planes: the generic radius hands 21 + 21 fp32 planes through the workspace; the fused radii use 12 half planes of it)
extern "C" int64_t ppst_guided_filter_ws(int B, int H, int W) { return (int64_t)B * 42 * H * W * (int64_t)sizeof(float); }

// the two fused launches of radius RR; DVS1 / DVS2 are that radius's default rows per block
template <int RR, int DVS1, int DVS2>
static int gf_fused(hipStream_t st, const unsigned char* g, const unsigned char* s, unsigned short* abh, void* out, void* out_u8, int B, int H,
                    int W, float eps) {
  int e;
  const int vs1 = g_gf_vs1 ? g_gf_vs1 : DVS1;
  if (vs1 == 32) gf_s1_launch<RR, 32>(st, g, s, abh, B, H, W, eps);
  else if (vs1 == 128) gf_s1_launch<RR, 128>(st, g, s, abh, B, H, W, eps);
  else gf_s1_launch<RR, 64>(st, g, s, abh, B, H, W, eps);
  if ((e = PPST_LAUNCH_CHECK())) return e;
  const int vs2 = g_gf_vs2 ? g_gf_vs2 : DVS2;
  if (vs2 == 128) gf_s2_launch<RR, 128>(st, abh, g, out, out_u8, B, H, W);
  else if (vs2 == 32) gf_s2_launch<RR, 32>(st, abh, g, out, out_u8, B, H, W);
  else gf_s2_launch<RR, 64>(st, abh, g, out, out_u8, B, H, W);
  return PPST_LAUNCH_CHECK();
}

extern "C" int ppst_guided_filter(const void* guide_u8, const void* src_u8, void* out, void* out_u8, int B, int H, int W, int r,
                                  float eps, void* work, void* stream) {
  // (r == 90 is the one radius above GF_MAXR: it has a fused form and never reaches the generic kernels, whose LDS row is GF_MAXR wide)
  if (B < 0 || H <= 0 || W <= 0 || W > GF_MAXW || r <= 0 || (r > GF_MAXR && r != 90) || r >= H || r >= W) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!guide_u8 || !src_u8 || !work || (!out && !out_u8)) return PPST_ENULL;
  hipStream_t st = as_stream(stream);
  const int64_t P = (int64_t)H * W;
  const unsigned char* g = (const unsigned char*)guide_u8;
  const unsigned char* s = (const unsigned char*)src_u8;
  int e;
  // The fused radii: 30 (the path's radius at 512^2, photo_gif.py:43) and its multiples for 1024^2 and 1536^2 images
  // (ppst_model.guided_filter_radius): two fused launches, box sums kept on the chip.  abh = [B][12][P] IEEE half.
  // r == 30, rows per block: 32 in the first launch (its halo re-reads are uint8 rows: 6 B / pixel each), 64 in the second (24 B / pixel each).
  // Measured, batch of four 1024^2 images (tests/gf_prof.sh): (64, 64) 0.36 ms, (32, 64) 0.33 ms, (32, 32) 0.30 ms with 1.25x the traffic,
  // (64, 128) 0.44 ms -- three co-resident blocks per CU (768 blocks) are what hides the per-row latency.
  // r == 60 and r == 90, geometry and rows per block.  Measured on one MI355X (tests/gf_radius_time.py, ms per call, median of five
  // groups of ten calls, groups within 1 %); (NT, WC, SEG, UNR): resident blocks per CU by registers and LDS (first, second launch):
  // best rows per block -- also (32, 64) / (64, 64):
  //   r = 60, four 1024^2 images (the five-launch generic path of this radius: 8.00 ms)
  //     (256, 128, 16, 16): 3, 4 blocks:  0.56 at (32, 64) -- 0.56 / 0.56
  //     (384, 256, 16, 16): 2, 2 blocks:  0.54 at (32, 32) -- 0.61 / 0.58                      <- adopted, with (32, 32)
  //     (384, 256, 16,  8): 2, 2 blocks:  0.56 at (32, 32) -- 0.65 / 0.62
  //     (384, 256, 32,  8): 2, 2 blocks:  0.52 at (32, 32) -- 0.62 / 0.58
  //     (512, 384, 16, 16): 1, 2 blocks:  0.61 at (32, 32) -- 0.68 / 0.64   (three strips for 1024 columns: a quarter of them idle)
  //     (768, 640, 32, 16): 1, 1 block:   0.45 at (32, 32) -- 0.56 / 0.75   (100 B / lane of scratch in the first launch)
  //   r = 90, four 1536^2 images (the parent refuses this radius)
  //     (256,  64, 16, 16): 3, 4 blocks:  2.79 at (64, 64) -- 2.96 / 2.79
  //     (384, 192, 16, 16): 2, 2 blocks:  1.53 at (64, 128) -- 1.79 / 1.63
  //     (384, 192, 16,  8): 2, 2 blocks:  1.80 at (64, 128) -- 2.02 / 1.87
  //     (384, 192, 32,  8): 2, 2 blocks:  1.95 at (64, 128) -- 2.13 / 1.97
  //     (512, 320, 16, 16): 1, 2 blocks:  1.39 at (64, 64) -- 1.51 / 1.39                      <- adopted, with (64, 64)
  //     (768, 576, 32, 16): 1, 1 block:   1.78 at (32, 32) -- 1.82 / 1.97   (100 B / lane of scratch in the first launch)
  // Not adopted at r = 60 although fastest at that batch: 768 threads.  Its 0.45 ms is the case of 2 strips x 32 row blocks x 4 images
  // = 256 blocks on 256 CUs, one resident block each; a single 1024^2 image (what a swap decodes) is 64 such blocks on a quarter of
  // the chip and takes 0.44 ms, where 384 threads give 128 blocks of half the waves and 0.33 ms; and its first launch spills.  The longer segment (SEG = 32: 7.6
  // LDS reads per output and plane at r = 90 in place of 13) did not pay for the threads it idles during the horizontal pass.
  if (r == 30) return gf_fused<30, 32, 64>(st, g, s, (unsigned short*)work, out, out_u8, B, H, W, eps);
  if (r == 60) return gf_fused<60, 32, 32>(st, g, s, (unsigned short*)work, out, out_u8, B, H, W, eps);
  if (r == 90) return gf_fused<90, 64, 64>(st, g, s, (unsigned short*)work, out, out_u8, B, H, W, eps);
  const float* hs;
  if ((e = gf_plane_route<GF_SRC_COLOUR, 21, 3, false>(st, g, s, out ? out : out_u8, work, B, H, W, r, eps, &hs))) return e;
  // (register blocking of this pass -- 12 planes x 8 rows per thread -- measured 3.5x SLOWER: 262 k threads with
  //  ~200 live registers each leave the chip empty; the plain form keeps one thread per pixel)
  PPST_LAUNCH(gf_v_final_kernel, dim3(gf_blocks_for(B * P)), dim3(256), 0, st, hs, g, (float*)out, (unsigned char*)out_u8, H, W, r,
              (int64_t)B * P);
  return PPST_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------------------
// Native-size output (He and Sun, "Fast Guided Filter", arXiv:1505.00996): the mean planes (mean a, mean b) of a filter solved at
// (h, w) are smooth by construction, so they are upsampled bilinearly and applied to the guide at ITS size (H, W) >= (h, w).
//   ppst_guided_filter_coeffs: the 12 mean planes [B][12][h][w] fp32 (plane 4c + k: k = 0..2 mean a_ck, k = 3 mean b_c), by the
//     plane route (exact forms, the header comment) at EVERY accepted radius (30 and 60 included: the fused launches never store
//     the means) and a last exact V pass into the caller's buffer (gf_coeffs).
//   ppst_guided_filter_apply -> gf_apply_up_kernel: q_c = A_c0 I0 + A_c1 I1 + A_c2 I2 + B_c per native pixel, (A, B) the bilinear
//     interpolation of the mean planes (half-pixel centres, edge replication: F.interpolate(mode="bilinear", align_corners=False)),
//     horizontally first, then vertically; rounded and stored like gf_store.  The 12 upsampled planes never exist in memory.
// Tap positions are INTEGERS: along an axis of n coefficient and N output samples, output Y has num = (2Y + 1) n - N,
// i0 = floor(num / 2N) (>= -1 since num > -2N), f = (num - 2N i0) / 2N, taps clamp(i0, 0, n - 1) and clamp(i0 + 1, 0, n - 1): no
// float position is ever floored, so a tap index cannot differ from a float64 judge's at any size.
// Geometry: a block of 256 threads owns a tile of GA_TW = 64 output columns x GA_TH = 16 rows, looping over the images of the
// batch that its blockIdx.y owns.  n <= N makes i0 grow by 0 or 1 per output sample, so the tile's taps lie in at most
// (GA_TH + 1) x (GA_TW + 1) coefficient samples -- the footprint, largest at scale 1: 17 x 65 x 12 floats = 53,040 B of LDS
// (60,080 B with the row buffers and tables: two blocks per CU).  At scale >= 2 on both axes it is at most 10 x 34 samples, and a
// second instance of the same body declares only that (23,360 B: five blocks per CU by registers, 92 VGPRs; measured 62 -> 45 us
// at 512^2 -> 1024^2 and 194 -> 102 us at -> 2048^2, B = 4).  Both instances compute the same bytes.  The footprint is staged
// PIXEL-MAJOR ([row][column][12 planes], edge replication resolved while staging: the compute phase never clamps) so that one
// thread's 2 taps x 12 planes are 24 consecutive floats = six 16-byte LDS reads (lane stride 12 dwords at scale 1: 16 lanes cover
// the 64 banks once; at scale >= 2 neighbours share a column and the read broadcasts).
// Thread = output column; a wave walks 4 consecutive rows and keeps the horizontally interpolated coefficient rows i0 and i0 + 1
// in registers: a row is read from LDS only when i0 advances (wave-uniform).  LDS words read per output pixel: 24 (1 + rows
// advanced) / 4 -- 30 at scale 1, 18 to 24 at scale 2, 12 at scale >= 4, against 48 of the form that reads four taps per pixel.
// Guide and output bytes move as ALIGNED DWORDS over each tile row's byte span through two small LDS row buffers (the bytes of a
// span that do not fill a dword -- at most 3 at either end -- move as bytes), whatever the alignment of the tensors.
// Every staged index is clamped to the plane and every local index to the footprint in the kernel itself.
#define GA_TW 64
#define GA_TH 16
#define GA_FC (GA_TW + 1)       // footprint of a tile at any scale >= 1 ...
#define GA_FR (GA_TH + 1)
#define GA_FC2 (GA_TW / 2 + 2)  // ... and at scale >= 2 on both axes: i0 advances at most every other sample (10 x 34 at exactly 2)
#define GA_FR2 (GA_TH / 2 + 2)
#define GA_NT 256
#define GA_RDW ((GA_TW * 3 + 3 + 3) / 4 + 1)   // dwords of one staged byte row: 192 B + up to 3 B of misalignment, rounded up: 50
#define GA_MAXPIX ((int64_t)1 << 28)

// tap of output sample Y along an axis of n coefficient and N >= n output samples
__device__ __forceinline__ void ga_tap(int Y, int n, int N, int& i0, float& f) {
  const int64_t num = (2 * (int64_t)Y + 1) * n - N, den = 2 * (int64_t)N;
  const int64_t q = num < 0 ? -1 : num / den;                          // floor: num > -den
  i0 = (int)q;
  f = (float)(num - q * den) / (float)den;
}

// the horizontally interpolated 12 coefficients of footprint row lr at the column pair (lc, lc + 1)
template <int FC>
__device__ __forceinline__ void ga_hrow(const float* fp, int lr, int lc, float fx, float (&v)[12]) {
  const float4* p = (const float4*)(fp + (lr * FC + lc) * 12);
  float4 q[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) q[i] = p[i];
  const float* a = (const float*)q;
  const float gx = 1.f - fx;
#pragma unroll
  for (int i = 0; i < 12; ++i) v[i] = gx * a[i] + fx * a[12 + i];
}

// FR x FC: the footprint the instance has LDS for (its local indices are clamped to it: a launch with the wrong instance would
// give wrong values, never an access outside)
template <int FR, int FC>
__global__ __launch_bounds__(GA_NT) void gf_apply_up_kernel(const float* __restrict__ coef, int h, int w,
                                                            const unsigned char* __restrict__ guide, unsigned char* __restrict__ out_u8,
                                                            float* __restrict__ out, int B, int H, int W, int tiles_x) {
  __shared__ __attribute__((aligned(16))) float fp[FR * FC * 12];
  __shared__ unsigned gsh[GA_TH][GA_RDW], osh[GA_TH][GA_RDW];
  __shared__ int rowi[GA_TH], coli[GA_TW];
  __shared__ float rowf[GA_TH], colf[GA_TW];
  const int t = threadIdx.x;
  const int X0 = (int)(blockIdx.x % tiles_x) * GA_TW, Y0 = (int)(blockIdx.x / tiles_x) * GA_TH;
  const int ncols = min(GA_TW, W - X0), nrows = min(GA_TH, H - Y0);
  // the tile's tap tables, once (absolute i0; samples past the image repeat its last one and are never stored)
  if (t < GA_TH) ga_tap(min(Y0 + t, H - 1), h, H, rowi[t], rowf[t]);
  else if (t >= 64 && t < 64 + GA_TW) ga_tap(min(X0 + t - 64, W - 1), w, W, coli[t - 64], colf[t - 64]);
  __syncthreads();
  const int ilo = rowi[0], jlo = coli[0];
  const int fr = min(rowi[nrows - 1] - ilo + 2, FR), fc = min(coli[ncols - 1] - jlo + 2, FC);
  const int64_t p = (int64_t)h * w, P = (int64_t)H * W;
  const int lane = t & 63, wv = t >> 6;
  const int xc = min(lane, ncols - 1);
  const int lc = min(coli[xc] - jlo, FC - 2);
  const float fx = colf[xc];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    // ---- stage the footprint: thread = (column, row mod 4), 12 plane reads in flight; column 64 (scale 1 only) by a second loop
    const float* cb = coef + (int64_t)b * 12 * p;
    if (lane < fc) {
      const int gx = min(max(jlo + lane, 0), w - 1);
      for (int lr = wv; lr < fr; lr += GA_NT / 64) {
        const float* s = cb + (int64_t)min(max(ilo + lr, 0), h - 1) * w + gx;
        float v[12];
#pragma unroll
        for (int pl = 0; pl < 12; ++pl) v[pl] = s[pl * p];
        float4* d = (float4*)(fp + (lr * FC + lane) * 12);
        d[0] = make_float4(v[0], v[1], v[2], v[3]);
        d[1] = make_float4(v[4], v[5], v[6], v[7]);
        d[2] = make_float4(v[8], v[9], v[10], v[11]);
      }
    }
    if (FC > 64 && fc > 64) {
      const int gx = min(max(jlo + 64, 0), w - 1);
      for (int i = t; i < fr * 12; i += GA_NT) {
        const int lr = i / 12, pl = i - lr * 12;
        fp[(lr * FC + 64) * 12 + pl] = cb[pl * p + (int64_t)min(max(ilo + lr, 0), h - 1) * w + gx];
      }
    }
    // ---- stage the guide bytes of the tile's rows: dword k of row y is the ALIGNED dword k of the row span's address range
    for (int i = t; i < nrows * 64; i += GA_NT) {
      const int y = i >> 6, k = i & 63;
      const unsigned char* a = guide + (((int64_t)b * H + Y0 + y) * W + X0) * 3;
      const int mis = (int)((uintptr_t)a & 3), n = ncols * 3, lo = 4 * k - mis;      // span bytes lo .. lo + 3
      if (k < GA_RDW && lo < n && lo + 4 > 0) {
        if (lo >= 0 && lo + 4 <= n) gsh[y][k] = *(const unsigned*)(a + lo);
        else
          for (int j = max(lo, 0); j < min(lo + 4, n); ++j) ((unsigned char*)gsh[y])[mis + j] = a[j];
      }
    }
    __syncthreads();
    // ---- compute: lane = column, the wave's 4 rows top to bottom
    {
      float top[12], bot[12];
      int cur = -2;
      for (int yy = 0; yy < GA_TH / 4; ++yy) {
        const int y = wv * (GA_TH / 4) + yy;
        if (y >= nrows) break;
        const int lr = __builtin_amdgcn_readfirstlane(min(rowi[y] - ilo, FR - 2));
        const float fy = rowf[y], gy = 1.f - fy;
        if (lr != cur) {
          if (lr == cur + 1) {
#pragma unroll
            for (int i = 0; i < 12; ++i) top[i] = bot[i];
          } else {
            ga_hrow<FC>(fp, lr, lc, fx, top);
          }
          ga_hrow<FC>(fp, lr + 1, lc, fx, bot);
          cur = lr;
        }
        const int64_t row = ((int64_t)b * H + Y0 + y) * W + X0;
        const unsigned char* g = (const unsigned char*)gsh[y] + (int)((uintptr_t)(guide + row * 3) & 3) + xc * 3;
        const float I0 = g[0], I1 = g[1], I2 = g[2];
        unsigned char* o = out_u8 ? (unsigned char*)osh[y] + (int)((uintptr_t)(out_u8 + row * 3) & 3) + xc * 3 : nullptr;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float A0 = gy * top[c * 4] + fy * bot[c * 4], A1 = gy * top[c * 4 + 1] + fy * bot[c * 4 + 1];
          const float A2 = gy * top[c * 4 + 2] + fy * bot[c * 4 + 2], Bc = gy * top[c * 4 + 3] + fy * bot[c * 4 + 3];
          const float qv = A0 * I0 + A1 * I1 + A2 * I2 + Bc;
          const float rq = fminf(fmaxf(rintf(qv), 0.f), 255.f);          // as gf_store
          if (lane < ncols) {
            if (o) o[c] = (unsigned char)rq;
            if (out) out[((int64_t)b * 3 + c) * P + (int64_t)(Y0 + y) * W + X0 + lane] = (rq / 255.0f - 0.5f) * 2.f;
          }
        }
      }
    }
    __syncthreads();
    // ---- store the output bytes: aligned dwords over each row's span, bytes where the span does not fill one
    if (out_u8) {
      for (int i = t; i < nrows * 64; i += GA_NT) {
        const int y = i >> 6, k = i & 63;
        unsigned char* a = out_u8 + (((int64_t)b * H + Y0 + y) * W + X0) * 3;
        const int mis = (int)((uintptr_t)a & 3), n = ncols * 3, lo = 4 * k - mis;
        if (k < GA_RDW && lo < n && lo + 4 > 0) {
          if (lo >= 0 && lo + 4 <= n) *(unsigned*)(a + lo) = osh[y][k];
          else
            for (int j = max(lo, 0); j < min(lo + 4, n); ++j) a[j] = ((const unsigned char*)osh[y])[mis + j];
        }
      }
    }
    // (the next image's staging writes fp and gsh, which nobody reads after the barrier above; osh is written again only
    //  behind the next barrier)
  }
}

// The two coefficient entries: the exact plane route and its last V pass into the caller's buffer ([B][4 NC][h][w]).
template <int SRC, int NM, int NC>
static int gf_coeffs(const void* guide_u8, const void* src, void* coeffs, int B, int h, int w, int r, float eps, void* work, void* stream) {
  hipStream_t st = as_stream(stream);
  const float* hs;
  const int e = gf_plane_route<SRC, NM, NC, true>(st, guide_u8, src, coeffs, work, B, h, w, r, eps, &hs);
  if (e || !hs) return e;
  const int64_t tc = (int64_t)B * 4 * NC * h * w;
  PPST_LAUNCH(gf_v_kernel<double>, dim3(gf_blocks_for(tc)), dim3(256), 0, st, hs, (float*)coeffs, h, w, r, tc);
  return PPST_LAUNCH_CHECK();
}

// (the route's radius rule: r = 90, the fused radius above GF_MAXR, has no fp32-plane form)
extern "C" int ppst_guided_filter_coeffs(const void* guide_u8, const void* src_u8, void* coeffs, int B, int h, int w, int r, float eps,
                                         void* work, void* stream) {
  return gf_coeffs<GF_SRC_COLOUR, 21, 3>(guide_u8, src_u8, coeffs, B, h, w, r, eps, work, stream);
}

// (26 planes: 13 + 13 fp32 planes handed through the workspace)
extern "C" int64_t ppst_guided_matte_ws(int B, int h, int w) { return (int64_t)B * 26 * h * w * (int64_t)sizeof(float); }

extern "C" int ppst_guided_matte_coeffs(const void* guide_u8, const void* matte_f32, void* mcoeffs, int B, int h, int w, int r, float eps,
                                        void* work, void* stream) {
  return gf_coeffs<GF_SRC_MATTE, 13, 1>(guide_u8, matte_f32, mcoeffs, B, h, w, r, eps, work, stream);
}

extern "C" int ppst_guided_filter_apply(const void* coeffs, int h, int w, const void* guide_u8, void* out_u8, void* out_f32, int B, int H,
                                        int W, void* stream) {
  if (B < 0 || h <= 0 || w <= 0 || H < h || W < w || (int64_t)H * W > GA_MAXPIX) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!coeffs || !guide_u8 || (!out_u8 && !out_f32)) return PPST_ENULL;
  const int tiles_x = cdiv(W, GA_TW);
  const int64_t tiles = (int64_t)tiles_x * cdiv(H, GA_TH);     // <= 2^28: H W <= 2^28
  const dim3 grid((unsigned)tiles, (unsigned)(B > 65535 ? 65535 : B));
  // two instances of one body: at scale >= 2 on both axes the footprint is a quarter and three times the blocks fit a CU
  if (2 * (int64_t)h <= H && 2 * (int64_t)w <= W)
    PPST_LAUNCH((gf_apply_up_kernel<GA_FR2, GA_FC2>), grid, dim3(GA_NT), 0, as_stream(stream), (const float*)coeffs, h, w,
                (const unsigned char*)guide_u8, (unsigned char*)out_u8, (float*)out_f32, B, H, W, tiles_x);
  else
    PPST_LAUNCH((gf_apply_up_kernel<GA_FR, GA_FC>), grid, dim3(GA_NT), 0, as_stream(stream), (const float*)coeffs, h, w,
                (const unsigned char*)guide_u8, (unsigned char*)out_u8, (float*)out_f32, B, H, W, tiles_x);
  return PPST_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------------------
// The coefficients applied INSIDE a photograph (ppst_guided_filter_paste; the transform and its integer units are in sim_xf.h):
// gf_apply_up_kernel's arithmetic along a similarity map instead of an axis-aligned one, plus a feathered edge.  For the photo
// pixel (X, Y): U, V in int64; inside iff 0 <= U, V < n 2^24; taps from Ui = U - 2^23: i0 = Ui >> 24 (>= -1), fraction
// (Ui & (2^24 - 1)) / 2^24 (exact in fp32), clamped to [0, n - 1]; horizontally, then vertically; q = A I + B on the photo's own
// pixel; out = rint(g q + (1 - g) I), g the smoothstep of the distance to the crop's edge over ``feather`` crop pixels.  Pixels
// outside the crop are not written.
// Geometry: photo tiles of GP_T x GP_T pixels on the photo's own grid (multiples of GP_T), one thread per pixel, over the box of
// the quad only: a block derives the box of its image from the transform (sx_box, margin 1; the entry point sizes the grid with
// margin 2, so it never has fewer tiles than a block counts) and leaves if its index is past it.  A tile's taps lie between the
// floors of Ui, Vi at its four corner pixels (both are linear in X, Y): 15 (|cos| + |sin|) / s <= 21.3 coefficient samples apart,
// so at most GP_FS = 24 a side with the + 1 tap.  That footprint is staged pixel-major in LDS (24 x 24 x 12 floats = 27,648 B;
// rows and columns limited to the plane, so fewer near the crop's edge), a thread reads its 4 taps x 12 planes as 12 16-byte
// reads.  A 32 x 16 tile would need up to 37 x 37 samples at 45 degrees and s = 1 -- 65.7 KB, more than a block may declare.
// Every staged index is clamped to the plane and every local index to the footprint.
// Through a matte (ppst_guided_filter_paste_matte; MATTE = GP_PLANE, the same body): the matte plane [B][n][n] is a 13th plane with
// the same footprint, staged in an array of its own (24 x 24 floats = 2,304 B: the 12-plane array keeps its 48-byte pixels and
// 16-byte reads) and sampled by the same taps and fractions; g = g_edge m^, and a pixel with g == 0 is left unwritten.
// Through guided-matte coefficients (ppst_guided_filter_paste_gmatte; MATTE = GP_COEFFS): the four planes [B][4][n][n] of
// ppst_guided_matte_coeffs are staged pixel-major in a third array (24 x 24 x 4 floats = 9,216 B, one 16-byte read per tap),
// sampled like the 12 and evaluated on the photo's pixel: m^ = clamp((M . I + Mb) / 255, 0, 1); the optional weight plane gets
// rint(255 g) for every pixel inside the square, written or not.  The kernel's ``matte`` pointer is the form's one extra input.
#include "sim_xf.h"
#define GP_T 16
#define GP_FS 24

#define GP_NONE 0       // the three forms of the one body: no matte,
#define GP_PLANE 1      // a matte plane [B][n][n],
#define GP_COEFFS 2     // guided-matte coefficients [B][4][n][n]

template <int MATTE>
__global__ __launch_bounds__(GP_T * GP_T) void gf_paste_kernel(const float* __restrict__ coef, const float* __restrict__ matte, int n,
                                                               const unsigned char* photo, unsigned char* out,
                                                               unsigned char* __restrict__ weight, int B, int H, int W,
                                                               const int64_t* __restrict__ xf, int feather) {
  __shared__ __attribute__((aligned(16))) float fp[GP_FS * GP_FS * 12];
  __shared__ float fm[MATTE == GP_PLANE ? GP_FS * GP_FS : 1];
  __shared__ float4 fg[MATTE == GP_COEFFS ? GP_FS * GP_FS : 1];
  const int t = threadIdx.x;
  const int64_t p = (int64_t)n * n, side = (int64_t)n * SX_ONE;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const SimXf f = {xf[4 * b], xf[4 * b + 1], xf[4 * b + 2], xf[4 * b + 3]};
    int bx0, by0, bx1, by1;
    sx_box(f, 0, side, 0, side, 1, bx0, by0, bx1, by1);
    bx0 = max(bx0, 0); by0 = max(by0, 0); bx1 = min(bx1, W - 1); by1 = min(by1, H - 1);
    if (bx0 > bx1 || by0 > by1) continue;                                      // (block-uniform, like every exit below)
    const int tx0 = bx0 / GP_T, ty0 = by0 / GP_T, ntx = bx1 / GP_T - tx0 + 1, nty = by1 / GP_T - ty0 + 1;
    if ((int64_t)blockIdx.x >= (int64_t)ntx * nty) continue;
    const int X0 = (tx0 + (int)(blockIdx.x % ntx)) * GP_T, Y0 = (ty0 + (int)(blockIdx.x / ntx)) * GP_T;
    const int XL = min(X0 + GP_T - 1, W - 1), YL = min(Y0 + GP_T - 1, H - 1);
    // ---- the tile's footprint: extremes of Ui, Vi over the corner pixels
    int64_t ulo = INT64_MAX, uhi = INT64_MIN, vlo = INT64_MAX, vhi = INT64_MIN;
    for (int k = 0; k < 4; ++k) {
      const int64_t px = 2 * (int64_t)((k & 1) ? XL : X0) + 1, py = 2 * (int64_t)((k & 2) ? YL : Y0) + 1;
      const int64_t Ui = f.a * px + f.b * py + f.cu - SX_HALF, Vi = -f.b * px + f.a * py + f.cv - SX_HALF;
      ulo = sx_min(ulo, Ui); uhi = sx_max(uhi, Ui); vlo = sx_min(vlo, Vi); vhi = sx_max(vhi, Vi);
    }
    // U and V are linear in (X, Y): a tile whose corners all lie on the outer side of one edge of the square has no pixel in it
    // (the box of a turned square is up to twice its area)
    if (uhi + SX_HALF < 0 || ulo + SX_HALF >= side || vhi + SX_HALF < 0 || vlo + SX_HALF >= side) continue;
    const int64_t nm1 = n - 1;
    const int ilo = (int)sx_min(sx_max(ulo >> 24, 0), nm1), ihi = (int)sx_min(sx_max((uhi >> 24) + 1, 0), nm1);
    const int jlo = (int)sx_min(sx_max(vlo >> 24, 0), nm1), jhi = (int)sx_min(sx_max((vhi >> 24) + 1, 0), nm1);
    const int fc = min(ihi - ilo + 1, GP_FS), fr = min(jhi - jlo + 1, GP_FS);
    const float* cb = coef + (int64_t)b * 12 * p;
    for (int k = t; k < fr * fc; k += GP_T * GP_T) {
      const int lr = k / fc, lc = k - lr * fc;
      const float* s = cb + (int64_t)min(jlo + lr, n - 1) * n + min(ilo + lc, n - 1);
      float v[12];
#pragma unroll
      for (int pl = 0; pl < 12; ++pl) v[pl] = s[pl * p];
      float4* d = (float4*)(fp + (lr * GP_FS + lc) * 12);
      d[0] = make_float4(v[0], v[1], v[2], v[3]);
      d[1] = make_float4(v[4], v[5], v[6], v[7]);
      d[2] = make_float4(v[8], v[9], v[10], v[11]);
      if (MATTE == GP_PLANE) fm[lr * GP_FS + lc] = matte[(int64_t)b * p + (s - cb)];
      if (MATTE == GP_COEFFS) {
        const float* ms = matte + (int64_t)b * 4 * p + (s - cb);
        fg[lr * GP_FS + lc] = make_float4(ms[0], ms[p], ms[2 * p], ms[3 * p]);
      }
    }
    __syncthreads();
    const int X = X0 + (t % GP_T), Y = Y0 + (t / GP_T);
    if (X < W && Y < H) {
      const int64_t U = f.a * (2 * (int64_t)X + 1) + f.b * (2 * (int64_t)Y + 1) + f.cu;
      const int64_t V = -f.b * (2 * (int64_t)X + 1) + f.a * (2 * (int64_t)Y + 1) + f.cv;
      if (U >= 0 && U < side && V >= 0 && V < side) {
        const int64_t Ui = U - SX_HALF, Vi = V - SX_HALF;
        const int i0 = (int)(Ui >> 24), j0 = (int)(Vi >> 24);
        const float fx = (float)(int)(Ui & (SX_ONE - 1)) * (1.f / 16777216.f), fy = (float)(int)(Vi & (SX_ONE - 1)) * (1.f / 16777216.f);
        const float gx = 1.f - fx, gy = 1.f - fy;
        const int c0 = min(max(min(max(i0, 0), n - 1) - ilo, 0), fc - 1), c1 = min(max(min(max(i0 + 1, 0), n - 1) - ilo, 0), fc - 1);
        const int r0 = min(max(min(max(j0, 0), n - 1) - jlo, 0), fr - 1), r1 = min(max(min(max(j0 + 1, 0), n - 1) - jlo, 0), fr - 1);
        float top[12], bot[12];
        {
          const float4* a0 = (const float4*)(fp + (r0 * GP_FS + c0) * 12);
          const float4* a1 = (const float4*)(fp + (r0 * GP_FS + c1) * 12);
          const float4* b0 = (const float4*)(fp + (r1 * GP_FS + c0) * 12);
          const float4* b1 = (const float4*)(fp + (r1 * GP_FS + c1) * 12);
          float4 q[12];
#pragma unroll
          for (int k = 0; k < 3; ++k) { q[k] = a0[k]; q[3 + k] = a1[k]; q[6 + k] = b0[k]; q[9 + k] = b1[k]; }
          const float* a = (const float*)q;
#pragma unroll
          for (int k = 0; k < 12; ++k) { top[k] = gx * a[k] + fx * a[12 + k]; bot[k] = gx * a[24 + k] + fx * a[36 + k]; }
        }
        const int64_t at = (((int64_t)b * H + Y) * W + X) * 3;
        const float I0 = photo[at], I1 = photo[at + 1], I2 = photo[at + 2];
        float g = 1.f;
        if (feather > 0) {
          const int64_t d = sx_min(sx_min(U, side - U), sx_min(V, side - V));
          const float tt = fminf(fmaxf((float)d * (1.f / 16777216.f) / (float)feather, 0.f), 1.f);
          g = tt * tt * (3.f - 2.f * tt);
        }
        if (MATTE == GP_PLANE) {
          const float mt = gx * fm[r0 * GP_FS + c0] + fx * fm[r0 * GP_FS + c1], mb = gx * fm[r1 * GP_FS + c0] + fx * fm[r1 * GP_FS + c1];
          g *= gy * mt + fy * mb;
        }
        if (MATTE == GP_COEFFS) {
          const float4 t0 = fg[r0 * GP_FS + c0], t1 = fg[r0 * GP_FS + c1], u0 = fg[r1 * GP_FS + c0], u1 = fg[r1 * GP_FS + c1];
          const float M0 = gy * (gx * t0.x + fx * t1.x) + fy * (gx * u0.x + fx * u1.x);
          const float M1 = gy * (gx * t0.y + fx * t1.y) + fy * (gx * u0.y + fx * u1.y);
          const float M2 = gy * (gx * t0.z + fx * t1.z) + fy * (gx * u0.z + fx * u1.z);
          const float Mb = gy * (gx * t0.w + fx * t1.w) + fy * (gx * u0.w + fx * u1.w);
          g *= fminf(fmaxf((M0 * I0 + M1 * I1 + M2 * I2 + Mb) * (1.f / 255.f), 0.f), 1.f);     // (fmaxf drops a NaN: 0)
          if (weight) weight[((int64_t)b * H + Y) * W + X] = (unsigned char)rintf(255.f * g);
        }
        const float I[3] = {I0, I1, I2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (MATTE && g == 0.f) break;                                          // (unwritten: the byte stays the caller's)
          const float A0 = gy * top[c * 4] + fy * bot[c * 4], A1 = gy * top[c * 4 + 1] + fy * bot[c * 4 + 1];
          const float A2 = gy * top[c * 4 + 2] + fy * bot[c * 4 + 2], Bc = gy * top[c * 4 + 3] + fy * bot[c * 4 + 3];
          const float qv = A0 * I0 + A1 * I1 + A2 * I2 + Bc;
          out[at + c] = (unsigned char)fminf(fmaxf(rintf(g * qv + (1.f - g) * I[c]), 0.f), 255.f);
        }
      }
    }
    __syncthreads();                                                          // (the next image's staging overwrites fp)
  }
}

template <int MATTE>
static int gf_paste(const void* coeffs, const void* matte, int n, const void* photo_u8, void* out_u8, void* weight_u8, int B, int H, int W,
                    const void* xf_host, const void* xf_dev, int feather, void* stream) {
  if (B < 0 || n <= 0 || n > SX_NMAX || H <= 0 || W <= 0 || (int64_t)H * W > SX_MAXPIX || feather < 0 || 2 * feather > n) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!coeffs || (MATTE && !matte) || !photo_u8 || !out_u8 || !xf_host || !xf_dev) return PPST_ENULL;
  const SimXf* f = (const SimXf*)xf_host;
  int64_t tiles = 0;
  for (int b = 0; b < B; ++b) {
    if (!sx_rule(f[b])) return PPST_EINVAL;
    int x0, y0, x1, y1;
    sx_box(f[b], 0, (int64_t)n * SX_ONE, 0, (int64_t)n * SX_ONE, 2, x0, y0, x1, y1);
    x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0; x1 = x1 > W - 1 ? W - 1 : x1; y1 = y1 > H - 1 ? H - 1 : y1;
    if (x0 > x1 || y0 > y1) continue;
    const int64_t nt = (int64_t)(x1 / GP_T - x0 / GP_T + 1) * (y1 / GP_T - y0 / GP_T + 1);
    tiles = nt > tiles ? nt : tiles;
  }
  if (tiles == 0) return PPST_OK;                                             // no quad meets its photo
  PPST_LAUNCH((gf_paste_kernel<MATTE>), dim3((unsigned)tiles, (unsigned)(B > 65535 ? 65535 : B)), dim3(GP_T * GP_T), 0, as_stream(stream),
              (const float*)coeffs, (const float*)matte, n, (const unsigned char*)photo_u8, (unsigned char*)out_u8,
              (unsigned char*)weight_u8, B, H, W, (const int64_t*)xf_dev, feather);
  return PPST_LAUNCH_CHECK();
}

extern "C" int ppst_guided_filter_paste(const void* coeffs, int n, const void* photo_u8, void* out_u8, int B, int H, int W,
                                        const void* xf_host, const void* xf_dev, int feather, void* stream) {
  return gf_paste<GP_NONE>(coeffs, nullptr, n, photo_u8, out_u8, nullptr, B, H, W, xf_host, xf_dev, feather, stream);
}

extern "C" int ppst_guided_filter_paste_matte(const void* coeffs, const void* matte_f32, int n, const void* photo_u8, void* out_u8,
                                              int B, int H, int W, const void* xf_host, const void* xf_dev, int feather, void* stream) {
  return gf_paste<GP_PLANE>(coeffs, matte_f32, n, photo_u8, out_u8, nullptr, B, H, W, xf_host, xf_dev, feather, stream);
}

extern "C" int ppst_guided_filter_paste_gmatte(const void* coeffs, const void* mcoeffs, int n, const void* photo_u8, void* out_u8,
                                               void* weight_u8, int B, int H, int W, const void* xf_host, const void* xf_dev, int feather,
                                               void* stream) {
  return gf_paste<GP_COEFFS>(coeffs, mcoeffs, n, photo_u8, out_u8, weight_u8, B, H, W, xf_host, xf_dev, feather, stream);
}

// (the revision history is at PPST_ABI_VERSION in include/ppst_hip.h; callers built against another revision must rebuild)
extern "C" int ppst_version(void) { return PPST_ABI_VERSION; }
