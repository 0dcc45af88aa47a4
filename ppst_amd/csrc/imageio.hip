// Image preprocessing in front of the swap path, on the device:
// Pillow's 8-bit bicubic resample (Image.resize(..., BICUBIC) of data/base_dataset.py:141-168) as two
// integer passes over interleaved uint8 HWC images, and ToTensor + Normalize(0.5, 0.5).
// The 22-bit fixed-point coefficient tables are host logic (ppst_amd/imageio.py mirrors Pillow's
// precompute_coeffs / normalize_coeffs_8bpc); the kernels are pure integer: bit-exact by construction.
#include "common.h"

// One thread = one output sample (pixel, channel).  HORIZ: out[b][y][xx][c] = clip8((2^21 + sum_k in[b][y][xmin+k][c] *
// coef[xx][k]) >> 22); vertical: the same along y.  bounds[i] = (first, count), coef [n_out][ksize].
template <bool HORIZ>
__global__ __launch_bounds__(256) void resample_u8_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y,
                                                          const int* __restrict__ bounds, const int* __restrict__ coef, int ksize,
                                                          int in_h, int in_w, int out_h, int out_w, int C, unsigned total,
                                                          FastDiv d_c, FastDiv d_w, FastDiv d_h) {
  for (uint64_t t64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; t64 < total; t64 += (uint64_t)gridDim.x * 256) {
    unsigned cu, xu, yu;
    unsigned r = fd_divmod((unsigned)t64, d_c, cu);
    r = fd_divmod(r, d_w, xu);
    const int b = (int)fd_divmod(r, d_h, yu);
    const int c = (int)cu, ox = (int)xu, oy = (int)yu;
    const int i = HORIZ ? ox : oy;
    const int first = bounds[2 * i], n = bounds[2 * i + 1];
    const int* k = coef + (int64_t)i * ksize;
    int ss = 1 << 21;
    if (HORIZ) {
      const unsigned char* p = x + (((int64_t)b * in_h + oy) * in_w + first) * C + c;
      for (int j = 0; j < n; ++j) ss += (int)p[(int64_t)j * C] * k[j];
    } else {
      const unsigned char* p = x + (((int64_t)b * in_h + first) * in_w + ox) * C + c;
      for (int j = 0; j < n; ++j) ss += (int)p[(int64_t)j * in_w * C] * k[j];
    }
    ss >>= 22;  // arithmetic shift (Pillow's clip8 table is indexed by the shifted value)
    y[t64] = (unsigned char)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
  }
}

extern "C" int ppst_resample_u8(const void* x, void* y, int B, int in_h, int in_w, int C, int out_size, int horizontal,
                                const void* bounds, const void* coef, int ksize, void* stream) {
  if (B < 0 || in_h <= 0 || in_w <= 0 || C <= 0 || out_size <= 0 || ksize <= 0) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!x || !y || !bounds || !coef) return PPST_ENULL;
  const int out_h = horizontal ? in_h : out_size, out_w = horizontal ? out_size : in_w;
  int64_t total = (int64_t)B * out_h * out_w * C;
  if (total > PPST_IDX32_MAX) return PPST_EINVAL;
  int64_t blocks = cdiv64(total, 256);
  if (blocks > 256 * 32) blocks = 256 * 32;
  const FastDiv d_c = make_fastdiv(C), d_w = make_fastdiv(out_w), d_h = make_fastdiv(out_h);
  if (horizontal)
    PPST_LAUNCH(resample_u8_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const unsigned char*)x,
                (unsigned char*)y, (const int*)bounds, (const int*)coef, ksize, in_h, in_w, out_h, out_w, C, (unsigned)total, d_c, d_w, d_h);
  else
    PPST_LAUNCH(resample_u8_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const unsigned char*)x,
                (unsigned char*)y, (const int*)bounds, (const int*)coef, ksize, in_h, in_w, out_h, out_w, C, (unsigned)total, d_c, d_w, d_h);
  return PPST_LAUNCH_CHECK();
}

// transforms.ToTensor (uint8 HWC -> float CHW, .div(255)) + Normalize(mean, std) per channel: (v/255 - mean)/std in fp32,
// the same operation order as torchvision.
__global__ __launch_bounds__(256) void u8_to_tensor_kernel(const unsigned char* __restrict__ x, float* __restrict__ y, int C, unsigned P,
                                                           unsigned total, float mean, float stdv, FastDiv d_p, FastDiv d_c) {
  for (uint64_t t64 = (uint64_t)blockIdx.x * 256 + threadIdx.x; t64 < total; t64 += (uint64_t)gridDim.x * 256) {
    unsigned pu, cu;
    unsigned r = fd_divmod((unsigned)t64, d_p, pu);   // output index = ((b*C + c)*P + p)
    const unsigned b = fd_divmod(r, d_c, cu);
    float v = (float)x[((int64_t)b * P + pu) * C + cu] / 255.0f;
    y[t64] = (v - mean) / stdv;
  }
}
extern "C" int ppst_u8_to_tensor(const void* x, void* y, int B, int H, int W, int C, float mean, float stdv, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || C <= 0 || stdv == 0.f) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!x || !y) return PPST_ENULL;
  int64_t P = (int64_t)H * W, total = (int64_t)B * C * P;
  if (total > PPST_IDX32_MAX) return PPST_EINVAL;
  int64_t blocks = cdiv64(total, 256);
  if (blocks > 256 * 32) blocks = 256 * 32;
  PPST_LAUNCH(u8_to_tensor_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const unsigned char*)x, (float*)y, C,
              (unsigned)P, (unsigned)total, mean, stdv, make_fastdiv((unsigned)P), make_fastdiv(C));
  return PPST_LAUNCH_CHECK();
}

// The same filter on fp32 planes, both axes in one launch (ppst_resample_f32).  A block owns an RS_TH x RS_TW tile of one output
// plane.  Pass 1: each of the input rows [y0, y0 + nrows) under the tile's vertical windows is filtered horizontally at the tile's
// RS_TW output columns into LDS (a wave = one row: lane l reads x[row][first(ox0 + l) + j]).  Pass 2: every output sample is the
// vertical filter over its column of the LDS tile (lanes = consecutive columns: conflict-free).  A null bounds table = that axis is
// copied.  Windows are clipped to the image and to the LDS tile, whatever the tables say: a bad table gives wrong values, never an
// access outside x or the tile.
#define RS_TH 16
#define RS_TW 64
#define RS_ROWS_MAX 192
__global__ __launch_bounds__(256) void resample_f32_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const int* __restrict__ bnd_h, const float* __restrict__ coef_h, int ksize_h,
                                                           const int* __restrict__ bnd_v, const float* __restrict__ coef_v, int ksize_v,
                                                           int in_h, int in_w, int out_h, int out_w, int rows_cap, int clamp, float lo,
                                                           float hi, FastDiv d_tx, FastDiv d_ty) {
  extern __shared__ __attribute__((aligned(16))) float rs_tile[];  // [rows_cap][RS_TW]
  unsigned tx, ty;
  const unsigned plane = fd_divmod(fd_divmod(blockIdx.x, d_tx, tx), d_ty, ty);
  const int lx = threadIdx.x & (RS_TW - 1), wy = threadIdx.x / RS_TW;
  const int ox = (int)tx * RS_TW + lx, oy0 = (int)ty * RS_TH;
  const int oy_last = min(oy0 + RS_TH, out_h) - 1;
  int y0 = oy0, y1 = oy_last + 1;
  if (bnd_v) { y0 = bnd_v[2 * oy0]; y1 = bnd_v[2 * oy_last] + bnd_v[2 * oy_last + 1]; }
  y0 = min(max(y0, 0), in_h);
  const int nrows = min(max(min(y1, in_h) - y0, 0), rows_cap);
  if (ox < out_w) {
    int first = ox, n = 1;
    const float* k = coef_h;
    if (bnd_h) {
      first = min(max(bnd_h[2 * ox], 0), in_w);
      n = min(bnd_h[2 * ox + 1], min(ksize_h, in_w - first));
      k += (int64_t)ox * ksize_h;
    }
    const float* p = x + ((int64_t)plane * in_h + y0) * in_w + first;
    for (int r = wy; r < nrows; r += 256 / RS_TW) {
      const float* q = p + (int64_t)r * in_w;
      float s;
      if (bnd_h) {
        s = 0.f;
        for (int j = 0; j < n; ++j) s = fmaf(q[j], k[j], s);
      } else {
        s = q[0];
      }
      rs_tile[r * RS_TW + lx] = s;
    }
  }
  __syncthreads();
  if (ox >= out_w) return;
  for (int oy = oy0 + wy; oy <= oy_last; oy += 256 / RS_TW) {
    int r0 = oy - y0, n = 1;
    const float* k = coef_v;
    if (bnd_v) {
      r0 = bnd_v[2 * oy] - y0;
      n = min(bnd_v[2 * oy + 1], ksize_v);
      k += (int64_t)oy * ksize_v;
    }
    if (r0 < 0) n = 0;
    n = min(n, nrows - r0);
    const float* t = rs_tile + r0 * RS_TW + lx;
    float s;
    if (bnd_v) {
      s = 0.f;
      for (int j = 0; j < n; ++j) s = fmaf(t[j * RS_TW], k[j], s);
    } else {
      s = n > 0 ? t[0] : 0.f;
    }
    if (clamp) s = fminf(fmaxf(s, lo), hi);
    y[((int64_t)plane * out_h + oy) * out_w + ox] = s;
  }
}

extern "C" int ppst_resample_f32(const void* x, void* y, int B, int in_h, int in_w, int out_h, int out_w, const void* bounds_h,
                                 const void* coef_h, int ksize_h, const void* bounds_v, const void* coef_v, int ksize_v, int clamp,
                                 float lo, float hi, void* stream) {
  if (B < 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return PPST_EINVAL;
  const bool copy_h = in_w == out_w, copy_v = in_h == out_h;
  if ((!copy_h && ksize_h <= 0) || (!copy_v && ksize_v <= 0)) return PPST_EINVAL;
  if (clamp && !(lo <= hi)) return PPST_EINVAL;
  if ((int64_t)B * in_h * in_w > PPST_IDX32_MAX || (int64_t)B * out_h * out_w > PPST_IDX32_MAX) return PPST_EINVAL;
  // rows under the vertical windows of RS_TH consecutive outputs: the window starts move by at most (RS_TH - 1) * in / out, the
  // last window is at most ksize_v long
  int64_t rows = (int64_t)(RS_TH - 1) * in_h / out_h + (copy_v ? 1 : ksize_v) + 1;
  if (rows > in_h) rows = in_h;
  if (rows > RS_ROWS_MAX) return PPST_EINVAL;
  const int64_t tiles_x = cdiv64(out_w, RS_TW), tiles_y = cdiv64(out_h, RS_TH), blocks = (int64_t)B * tiles_x * tiles_y;
  if (blocks > 0x7FFFFFFFll) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!x || !y || (!copy_h && (!bounds_h || !coef_h)) || (!copy_v && (!bounds_v || !coef_v))) return PPST_ENULL;
  PPST_LAUNCH(resample_f32_kernel, dim3((unsigned)blocks), dim3(256), (size_t)rows * RS_TW * sizeof(float), as_stream(stream),
              (const float*)x, (float*)y, copy_h ? nullptr : (const int*)bounds_h, (const float*)coef_h, ksize_h,
              copy_v ? nullptr : (const int*)bounds_v, (const float*)coef_v, ksize_v, in_h, in_w, out_h, out_w, (int)rows, clamp, lo, hi,
              make_fastdiv((unsigned)tiles_x), make_fastdiv((unsigned)tiles_y));
  return PPST_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------------------
// An aligned crop of a photograph under a similarity transform (ppst_extract_similarity; the transform and its integer units are
// in sim_xf.h): Pillow's antialiased bicubic stated in the CROP's frame.  Crop pixel (i, j) has its centre at
// (Uc, Vc) = ((2i + 1) 2^23, (2j + 1) 2^23); every photo pixel (X, Y) with |U - Uc| < 2^25 and |V - Vc| < 2^25 -- decided on the
// int64 values, never on a float -- contributes w = k((U - Uc) / 2^24) k((V - Vc) / 2^24); the output is sum w p / sum w.  The
// arguments are converted to fp32 from integers below 2^25 and the weights are fp32; a row of taps is summed on its own and the
// row sums are added up (at s = 8 a pixel has 1024 taps: one running sum would carry their roundings).
// Geometry: a block owns T x T crop pixels, one per thread.  The taps of the tile lie in the box of the rotated square of
// (T + 3) crop pixels a side: at most (T + 3) s sqrt(2) + 3 photo pixels a side with the margin of sx_box -- 111 at T = 16, s <= 4
// and 128 at T = 8, s <= 8, which is what the rule s <= 8 is for.  Its bytes are staged in LDS (EX_FS16^2 x 3 = 37,632 B,
// EX_FS8^2 x 3 = 49,152 B) with the edge replication resolved while staging; a thread then walks the box of its own support
// (limited to the staged box: a tap outside it -- there is none -- would be dropped, never read) with U, V advanced by
// additions.
#include "sim_xf.h"
#define EX_FS16 112
#define EX_FS8 128

__device__ __forceinline__ float ex_bicubic(float x) {
  x = fabsf(x);
  const float a = -0.5f;
  return x < 1.f ? ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f : (x < 2.f ? (((x - 5.f) * x + 8.f) * x - 4.f) * a : 0.f);
}

template <int T, int FS>
__global__ __launch_bounds__(T * T) void extract_similarity_kernel(const unsigned char* __restrict__ photo, const int64_t* __restrict__ xf,
                                                                   unsigned char* __restrict__ out, int B, int H, int W, int n, int tiles_x) {
  __shared__ unsigned char sh[FS * FS * 3];
  const int t = threadIdx.x;
  const int i0 = (int)(blockIdx.x % tiles_x) * T, j0 = (int)(blockIdx.x / tiles_x) * T;
  const int i = i0 + (t % T), j = j0 + (t / T);
  const int64_t R = (int64_t)1 << 25;                                         // the filter's support: 2 crop pixels
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const SimXf f = {xf[4 * b], xf[4 * b + 1], xf[4 * b + 2], xf[4 * b + 3]};
    // ---- the tile's box and its bytes
    const int il = min(i0 + T - 1, n - 1), jl = min(j0 + T - 1, n - 1);
    int X0, Y0, X1, Y1;
    sx_box(f, (2 * (int64_t)i0 + 1) * SX_HALF - R, (2 * (int64_t)il + 1) * SX_HALF + R, (2 * (int64_t)j0 + 1) * SX_HALF - R,
           (2 * (int64_t)jl + 1) * SX_HALF + R, 1, X0, Y0, X1, Y1);
    const int bw = min(X1 - X0 + 1, FS), bh = min(Y1 - Y0 + 1, FS);
    const unsigned char* pb = photo + (int64_t)b * H * W * 3;
    for (int k = t; k < bw * bh; k += T * T) {
      const int ly = k / bw, lx = k - ly * bw;
      const unsigned char* p = pb + ((int64_t)min(max(Y0 + ly, 0), H - 1) * W + min(max(X0 + lx, 0), W - 1)) * 3;
      sh[k * 3] = p[0]; sh[k * 3 + 1] = p[1]; sh[k * 3 + 2] = p[2];
    }
    __syncthreads();
    if (i < n && j < n) {
      const int64_t Uc = (2 * (int64_t)i + 1) * SX_HALF, Vc = (2 * (int64_t)j + 1) * SX_HALF;
      int x0, y0, x1, y1;
      sx_box(f, Uc - R, Uc + R, Vc - R, Vc + R, 1, x0, y0, x1, y1);
      x0 = max(x0, X0); y0 = max(y0, Y0); x1 = min(x1, X0 + bw - 1); y1 = min(y1, Y0 + bh - 1);
      float n0 = 0.f, n1 = 0.f, n2 = 0.f, den = 0.f;
      for (int Y = y0; Y <= y1; ++Y) {
        int64_t dU = f.a * (2 * (int64_t)x0 + 1) + f.b * (2 * (int64_t)Y + 1) + f.cu - Uc;
        int64_t dV = -f.b * (2 * (int64_t)x0 + 1) + f.a * (2 * (int64_t)Y + 1) + f.cv - Vc;
        const unsigned char* row = sh + ((Y - Y0) * bw + (x0 - X0)) * 3;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f, rw = 0.f;
        for (int X = x0; X <= x1; ++X, dU += 2 * f.a, dV -= 2 * f.b, row += 3) {
          if (dU > -R && dU < R && dV > -R && dV < R) {
            const float w = ex_bicubic((float)(int)dU * (1.f / 16777216.f)) * ex_bicubic((float)(int)dV * (1.f / 16777216.f));
            r0 += w * (float)row[0]; r1 += w * (float)row[1]; r2 += w * (float)row[2]; rw += w;
          }
        }
        n0 += r0; n1 += r1; n2 += r2; den += rw;
      }
      unsigned char* o = out + (((int64_t)b * n + j) * n + i) * 3;
      o[0] = (unsigned char)fminf(fmaxf(rintf(n0 / den), 0.f), 255.f);
      o[1] = (unsigned char)fminf(fmaxf(rintf(n1 / den), 0.f), 255.f);
      o[2] = (unsigned char)fminf(fmaxf(rintf(n2 / den), 0.f), 255.f);
    }
    __syncthreads();                                                          // (the next image's staging overwrites sh)
  }
}

extern "C" int ppst_extract_similarity(const void* photo_u8, int B, int H, int W, const void* xf_host, const void* xf_dev, int n,
                                       void* out_u8, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || n <= 0 || n > SX_NMAX || (int64_t)H * W > SX_MAXPIX) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!photo_u8 || !xf_host || !xf_dev || !out_u8) return PPST_ENULL;
  const SimXf* f = (const SimXf*)xf_host;
  int64_t dmin = (int64_t)1 << 46;
  for (int b = 0; b < B; ++b) {
    if (!sx_rule(f[b])) return PPST_EINVAL;
    const int64_t D = f[b].a * f[b].a + f[b].b * f[b].b;
    dmin = D < dmin ? D : dmin;
  }
  const unsigned gy = (unsigned)(B > 65535 ? 65535 : B);
  // s <= 4 for every image (a^2 + b^2 >= 2^42): 16 x 16 tiles; else 8 x 8, whose box fits up to s = 8.  Same bytes either way.
  if (dmin >= ((int64_t)1 << 42)) {
    const int tx = cdiv(n, 16);
    PPST_LAUNCH((extract_similarity_kernel<16, EX_FS16>), dim3((unsigned)(tx * tx), gy), dim3(256), 0, as_stream(stream),
                (const unsigned char*)photo_u8, (const int64_t*)xf_dev, (unsigned char*)out_u8, B, H, W, n, tx);
  } else {
    const int tx = cdiv(n, 8);
    PPST_LAUNCH((extract_similarity_kernel<8, EX_FS8>), dim3((unsigned)(tx * tx), gy), dim3(64), 0, as_stream(stream),
                (const unsigned char*)photo_u8, (const int64_t*)xf_dev, (unsigned char*)out_u8, B, H, W, n, tx);
  }
  return PPST_LAUNCH_CHECK();
}
