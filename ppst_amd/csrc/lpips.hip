// LPIPS v0.1, net = 'alex' (lpips = True, spatial = False, normalize = False, eval mode): forward over two image batches and
// the input gradient (include/ppst_hip.h, "LPIPS-AlexNet metric").  The weights are frozen: no weight gradient exists here.
//
// Scheme.  Both batches run through the trunk as ONE batch of 2B images, channels-last, fp32 storage and plain fp32 FMA
// arithmetic (one rounding per product and per add: the error class of torch's own fp32 run, so ReLU / arg-max decisions differ
// from a float64 run at the 1e-6 level).
//   repack      NCHW (any strides) -> space-to-depth by 4 of the SCALED image, offset by the conv's pad of 2:
//               Z[j][i][(dy, dx, c)] = ((x - shift) / scale)(4j + dy - 2, 4i + dx - 2, c), zero outside.  conv1 (11x11, stride 4,
//               pad 2) is then a 3x3 stride-1 valid conv over 48 channels (11 <= 3 * 4; the taps 4t + d >= 11 carry zero weights)
//   conv        one implicit-GEMM kernel for every layer and every input gradient: 64 pixels x 64 output channels per block,
//               4 x 4 outputs per thread, K walked tap by tap in 16-channel chunks through a double-buffered LDS tile;
//               bias + ReLU in the epilogue.  The input gradient of a stride-1 conv is the same kernel on the flipped, transposed
//               weights (packed once, beside the forward ones) with pad' = K - 1 - pad; conv1's runs on the space-to-depth form
//               and ends in the inverse repack (* 1 / scale)
//   pool        3x3 stride 2, first maximum in row-major window order; the forward stores the arg-max (0..8) as a byte, the
//               backward is a GATHER over the at most four windows that cover an input pixel (no atomics), folded into the
//               tail's backward pass
//   tail        per layer one pass forward -- one wave per pixel: both channel norms, the difference, the lin dot product;
//               fixed-order sums per wave, per block and (one finishing launch) per image -- and one pass backward: the
//               gradient to fa and / or fb, plus what arrives from the layer above, times the layer's ReLU gate
// Where sqrt(sum_c f^2) == 0 (every channel of a post-ReLU pixel is 0) the gradient to that pixel's features is DEFINED as 0
// (torch's autograd gives NaN there: the derivative of sqrt at 0).
// Every reduction has a fixed order: two calls with the same inputs give the same bits.
#include "common.h"

namespace {

struct LpLayer { int K, pad, cin, cout, coutp; };
// forward convs (conv1 in its space-to-depth form) and their input gradients
const LpLayer LP_FWD[5] = {{3, 0, 48, 64, 64}, {5, 2, 64, 192, 192}, {3, 1, 192, 384, 384}, {3, 1, 384, 256, 256}, {3, 1, 256, 256, 256}};
const LpLayer LP_BWD[5] = {{3, 2, 64, 48, 64}, {5, 2, 192, 64, 64}, {3, 1, 384, 192, 192}, {3, 1, 256, 384, 384}, {3, 1, 256, 256, 256}};
const int LP_C[5] = {64, 192, 384, 256, 256};

inline int64_t lp_wfloats(const LpLayer& l) { return (int64_t)l.K * l.K * l.cin * l.coutp; }

struct LpPack { int64_t wf[5], wb[5], bias[5], lin[5], shift, scale, total; };
LpPack lp_pack_layout() {
  LpPack p;
  int64_t o = 0;
  for (int l = 0; l < 5; ++l) { p.wf[l] = o; o += lp_wfloats(LP_FWD[l]); }
  for (int l = 0; l < 5; ++l) { p.wb[l] = o; o += lp_wfloats(LP_BWD[l]); }
  for (int l = 0; l < 5; ++l) { p.bias[l] = o; o += LP_C[l]; }
  for (int l = 0; l < 5; ++l) { p.lin[l] = o; o += LP_C[l]; }
  p.shift = o; o += 4;
  p.scale = o; o += 4;
  p.total = o;
  return p;
}

struct LpDims {
  int H, W, ZH, ZW;
  int h[5], w[5];        // the five feature maps
  int ph[2], pw[2];      // the two pooled maps (== h[1], h[2])
};
int lp_dims(int H, int W, LpDims* d) {
  if (H < 31 || W < 31 || H > 16384 || W > 16384) return PPST_EINVAL;    // below 31 the second pool has no full window
  d->H = H; d->W = W;
  d->h[0] = (H + 4 - 11) / 4 + 1; d->w[0] = (W + 4 - 11) / 4 + 1;
  d->ZH = d->h[0] + 2; d->ZW = d->w[0] + 2;
  d->ph[0] = (d->h[0] - 3) / 2 + 1; d->pw[0] = (d->w[0] - 3) / 2 + 1;
  d->h[1] = d->ph[0]; d->w[1] = d->pw[0];
  d->ph[1] = (d->h[1] - 3) / 2 + 1; d->pw[1] = (d->w[1] - 3) / 2 + 1;
  for (int l = 2; l < 5; ++l) { d->h[l] = d->ph[1]; d->w[l] = d->pw[1]; }
  return PPST_OK;
}

inline int64_t up4(int64_t v) { return (v + 3) & ~(int64_t)3; }
#define LP_TAIL_PIX 64       // pixels per block of the tail's forward pass (4 waves x 16 pixels)

// forward workspace, float offsets (idx: byte offsets from the workspace's start)
struct LpWs { int64_t z, f[5], p[2], part, idx[2], bytes; int nblk[5], part_per_img; };
LpWs lp_ws_layout(const LpDims& d, int n) {
  LpWs w;
  int64_t o = 0;
  w.z = o; o += up4((int64_t)n * d.ZH * d.ZW * 48);
  for (int l = 0; l < 5; ++l) { w.f[l] = o; o += up4((int64_t)n * d.h[l] * d.w[l] * LP_C[l]); }
  for (int l = 0; l < 2; ++l) { w.p[l] = o; o += up4((int64_t)n * d.ph[l] * d.pw[l] * LP_C[l]); }
  w.part_per_img = 0;
  for (int l = 0; l < 5; ++l) { w.nblk[l] = cdiv(d.h[l] * d.w[l], LP_TAIL_PIX); w.part_per_img += w.nblk[l]; }
  w.part = o; o += up4((int64_t)(n / 2 + 1) * w.part_per_img);
  int64_t b = o * 4;
  for (int l = 0; l < 2; ++l) { w.idx[l] = b; b += up4((int64_t)n * d.ph[l] * d.pw[l] * LP_C[l]); }
  w.bytes = b;
  return w;
}

// ------------------------------------------------------------------ weight packing ----
// conv1's weight in the space-to-depth form: tap (ty, tx) in 0..2, channel ch = (dy * 4 + dx) * 3 + c
__device__ __forceinline__ float lp_w0(const float* w, int co, int ch, int ty, int tx) {
  if (ch >= 48) return 0.f;
  const int c = ch % 3, dx = (ch / 3) % 4, dy = ch / 12;
  const int ky = 4 * ty + dy, kx = 4 * tx + dx;
  return (ky < 11 && kx < 11) ? w[((co * 3 + c) * 11 + ky) * 11 + kx] : 0.f;
}
// out[tap][ci][co] (co padded to coutp).  mode 0: forward layer >= 1, 1: forward conv1, 2: gradient layer >= 1, 3: gradient conv1
__global__ void lp_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int K, int cin, int cout, int coutp, int mode, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int co = (int)(i % coutp);
  const int ci = (int)((i / coutp) % cin);
  const int tap = (int)(i / ((int64_t)coutp * cin));
  const int ky = tap / K, kx = tap % K;
  float v = 0.f;
  if (co < cout) {
    if (mode == 0) v = w[(((int64_t)co * cin + ci) * K + ky) * K + kx];
    else if (mode == 1) v = lp_w0(w, co, ci, ky, kx);
    else if (mode == 2) v = w[(((int64_t)ci * cout + co) * K + (K - 1 - ky)) * K + (K - 1 - kx)];   // torch weight [ci][co]: roles swapped
    else v = lp_w0(w, ci, co, 2 - ky, 2 - kx);
  }
  out[i] = v;
}
__global__ void lp_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// ------------------------------------------------------------------ repack ----
struct LpStr { int64_t n, c, y, x; };
__global__ void lp_repack_kernel(const float* __restrict__ a, LpStr sa, int na, const float* __restrict__ b, LpStr sb, int H, int W, int ZH, int ZW,
                                 const float* __restrict__ shift, const float* __restrict__ scale, float* __restrict__ z, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % 48);
  int64_t r = i / 48;
  const int zx = (int)(r % ZW); r /= ZW;
  const int zy = (int)(r % ZH);
  const int n = (int)(r / ZH);
  const int c = ch % 3, dx = (ch / 3) % 4, dy = ch / 12;
  const int y = 4 * zy + dy - 2, x = 4 * zx + dx - 2;
  float v = 0.f;
  if (y >= 0 && y < H && x >= 0 && x < W) {
    const float s = n < na ? a[n * sa.n + c * sa.c + y * sa.y + x * sa.x] : b[(n - na) * sb.n + c * sb.c + y * sb.y + x * sb.x];
    v = (s - shift[c]) / scale[c];
  }
  z[i] = v;
}
// gradient of the repack: every image pixel sits in exactly one cell of Z -- a gather; contiguous NCHW out
__global__ void lp_unrepack_kernel(const float* __restrict__ gz, float* __restrict__ gx, int H, int W, int ZH, int ZW,
                                   const float* __restrict__ scale, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % W);
  int64_t r = i / W;
  const int y = (int)(r % H); r /= H;
  const int c = (int)(r % 3);
  const int64_t n = r / 3;
  const int zy = (y + 2) >> 2, dy = (y + 2) & 3, zx = (x + 2) >> 2, dx = (x + 2) & 3;
  float v = 0.f;
  if (zy < ZH && zx < ZW) v = gz[((n * ZH + zy) * ZW + zx) * 48 + (dy * 4 + dx) * 3 + c] / scale[c];
  gx[i] = v;
}

// ------------------------------------------------------------------ conv ----
// out[p][co] = act(bias[co] + sum_{ky, kx, ci} in[n][oy + ky - pad][ox + kx - pad][ci] * wp[ky * K + kx][ci][co]), zero padding.
// cin % 16 == 0, coutp % 64 == 0, cout % 4 == 0.  256 threads: a 64-pixel x 64-channel tile, 4 x 4 per thread.
#define LP_BM 64
#define LP_BN 64
#define LP_BK 16
template <bool RELU>
__global__ __launch_bounds__(256) void lp_conv_kernel(const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
                                                      float* __restrict__ out, int npix, int IH, int IW, int OH, int OW, int cin, int cout,
                                                      int coutp, int K, int pad) {
  __shared__ __attribute__((aligned(16))) float As[2][LP_BK][LP_BM + 4];
  __shared__ __attribute__((aligned(16))) float Bs[2][LP_BK][LP_BN];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * LP_BN;
  // staging roles
  const int a_pix = tid >> 2, a_cq = tid & 3;
  const int b_k = tid >> 4, b_c = (tid & 15) * 4;
  const int p = m0 + a_pix;
  const bool valid = p < npix;
  int oy = 0, ox = 0;
  int64_t img = 0;
  if (valid) {
    ox = p % OW;
    const int r = p / OW;
    oy = r % OH;
    img = (int64_t)(r / OH) * IH * IW;
  }
  const int nck = cin / LP_BK;
  const int steps = K * K * nck;
  int ky = 0, kx = 0, ck = 0;                      // the step being LOADED
  float4 ra, rb;
  auto load = [&]() {
    const int iy = oy + ky - pad, ix = ox + kx - pad;
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid && iy >= 0 && iy < IH && ix >= 0 && ix < IW)
      ra = *(const float4*)(in + (img + (int64_t)iy * IW + ix) * cin + ck * LP_BK + a_cq * 4);
    rb = *(const float4*)(wp + ((int64_t)((ky * K + kx) * cin + ck * LP_BK + b_k)) * coutp + n0 + b_c);
    if (++ck == nck) { ck = 0; if (++kx == K) { kx = 0; ++ky; } }
  };
  auto stage = [&](int buf) {
    As[buf][a_cq * 4 + 0][a_pix] = ra.x;
    As[buf][a_cq * 4 + 1][a_pix] = ra.y;
    As[buf][a_cq * 4 + 2][a_pix] = ra.z;
    As[buf][a_cq * 4 + 3][a_pix] = ra.w;
    *(float4*)&Bs[buf][b_k][b_c] = rb;
  };
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  load();
  stage(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) load();
#pragma unroll
    for (int k = 0; k < LP_BK; ++k) {
      const float4 a4 = *(const float4*)&As[buf][k][ty * 4];
      const float4 b4 = *(const float4*)&Bs[buf][k][tx * 4];
      const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    if (s + 1 < steps) stage(buf ^ 1);
    __syncthreads();
  }
  const int co = n0 + tx * 4;
  if (co >= cout) return;
  float4 bz = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) bz = *(const float4*)(bias + co);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = m0 + ty * 4 + i;
    if (q >= npix) continue;
    float4 o = make_float4(acc[i][0] + bz.x, acc[i][1] + bz.y, acc[i][2] + bz.z, acc[i][3] + bz.w);
    if (RELU) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    *(float4*)(out + (int64_t)q * cout + co) = o;
  }
}

int lp_conv(const LpLayer& l, const float* in, const float* wp, const float* bias, float* out, int n, int IH, int IW, int OH, int OW,
            bool relu, hipStream_t st) {
  const int64_t npix = (int64_t)n * OH * OW;
  if (npix == 0) return PPST_OK;
  if (npix > 0x7fffffffll / 4 || l.cin % LP_BK || l.coutp % LP_BN || l.cout % 4) return PPST_EINVAL;
  dim3 grid((unsigned)cdiv64(npix, LP_BM), (unsigned)(l.coutp / LP_BN));
  if (relu)
    PPST_LAUNCH(lp_conv_kernel<true>, grid, dim3(256), 0, st, in, wp, bias, out, (int)npix, IH, IW, OH, OW, l.cin, l.cout, l.coutp, l.K, l.pad);
  else
    PPST_LAUNCH(lp_conv_kernel<false>, grid, dim3(256), 0, st, in, wp, bias, out, (int)npix, IH, IW, OH, OW, l.cin, l.cout, l.coutp, l.K, l.pad);
  return PPST_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ pool ----
// 3x3 stride 2, no padding; C % 4 == 0.  idx: position 0..8 (row-major in the window) of the FIRST maximum
__global__ void lp_pool_kernel(const float* __restrict__ f, float* __restrict__ p, unsigned char* __restrict__ idx, int IH, int IW, int PH, int PW,
                               int C4, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  int64_t r = i / C4;
  const int ox = (int)(r % PW); r /= PW;
  const int oy = (int)(r % PH);
  const int64_t n = r / PH;
  const float4* src = (const float4*)f + ((n * IH + 2 * oy) * IW + 2 * ox) * C4 + c4;
  float4 best = src[0];
  uchar4 bi = make_uchar4(0, 0, 0, 0);
#pragma unroll
  for (int k = 1; k < 9; ++k) {
    const float4 v = src[((int64_t)(k / 3) * IW + (k % 3)) * C4];
    if (v.x > best.x) { best.x = v.x; bi.x = k; }
    if (v.y > best.y) { best.y = v.y; bi.y = k; }
    if (v.z > best.z) { best.z = v.z; bi.z = k; }
    if (v.w > best.w) { best.w = v.w; bi.w = k; }
  }
  ((float4*)p)[i] = best;
  ((uchar4*)idx)[i] = bi;
}

// gradient of the pool at input pixel (y, x), channel c of image n: the windows that cover it and chose it
__device__ __forceinline__ float lp_pool_gather(const float* __restrict__ gp, const unsigned char* __restrict__ idx, int64_t n, int y, int x, int c,
                                                int PH, int PW, int C) {
  const int oy0 = y >= 2 ? (y - 1) >> 1 : 0, oy1 = min(PH - 1, y >> 1);
  const int ox0 = x >= 2 ? (x - 1) >> 1 : 0, ox1 = min(PW - 1, x >> 1);
  float g = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      const int64_t o = ((n * PH + oy) * PW + ox) * C + c;
      if (idx[o] == (y - 2 * oy) * 3 + (x - 2 * ox)) g += gp[o];
    }
  return g;
}

// ------------------------------------------------------------------ tail ----
// n(fa) - n(fb) of one channel.  No contraction: fused into fma(va, ia, -(vb * ib)) one product is rounded and the other is not,
// and equal inputs no longer give exactly 0.
__device__ __forceinline__ float lp_diff(float va, float ia, float vb, float ib) {
#pragma clang fp contract(off)
  const float x = va * ia, y = vb * ib;
  return x - y;
}

// forward: block (blk, b) takes pixels [blk * 64, +64) of image pair b; wave v the pixels v, v + 4, ...; CPL = C / 64
template <int CPL>
__global__ __launch_bounds__(256) void lp_tail_fwd_kernel(const float* __restrict__ f, const float* __restrict__ lin, float* __restrict__ part,
                                                          int B, int HW) {
  constexpr int C = CPL * 64;
  __shared__ float ws[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  float w[CPL];
#pragma unroll
  for (int t = 0; t < CPL; ++t) w[t] = lin[lane + 64 * t];
  float sum = 0.f;
  for (int k = 0; k < LP_TAIL_PIX / 4; ++k) {
    const int p = blockIdx.x * LP_TAIL_PIX + wave + 4 * k;
    if (p >= HW) break;                                     // (wave-uniform)
    const float* fa = f + ((int64_t)b * HW + p) * C;
    const float* fb = f + ((int64_t)(B + b) * HW + p) * C;
    float va[CPL], vb[CPL], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      va[t] = fa[lane + 64 * t];
      vb[t] = fb[lane + 64 * t];
      sa = fmaf(va[t], va[t], sa);
      sb = fmaf(vb[t], vb[t], sb);
    }
    const float ia = 1.f / (sqrtf(wave_sum(sa)) + 1e-10f), ib = 1.f / (sqrtf(wave_sum(sb)) + 1e-10f);
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const float d = lp_diff(va[t], ia, vb[t], ib);
      s = fmaf(w[t] * d, d, s);
    }
    sum += wave_sum(s);
  }
  if (lane == 0) ws[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

struct LpFin { int64_t off[5]; int nblk[5]; float inv_hw[5]; };
// one wave per image pair: the block partials of the five layers in a fixed order
__global__ __launch_bounds__(64) void lp_tail_finish_kernel(const float* __restrict__ part, LpFin fin, float* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float total = 0.f;
#pragma unroll
  for (int l = 0; l < 5; ++l) {
    const float* p = part + fin.off[l] + (int64_t)b * fin.nblk[l];
    float s = 0.f;
    for (int i = lane; i < fin.nblk[l]; i += 64) s += p[i];
    total += wave_sum(s) * fin.inv_hw[l];
  }
  if (lane == 0) out[b] = total;
}

// backward: one wave per pixel of image pair b.  ga / gb: [B][HW][C] gradients of the layer's PRE-activation (ReLU gate applied),
// either may be null.  What arrives from above: gin_* (same layout) or, through a pool, gp_* [B][PH][PW][C] with idx_*.
struct LpSide { float* g; const float* gin; const float* gp; const unsigned char* idx; };
template <int CPL>
__global__ __launch_bounds__(256) void lp_tail_bwd_kernel(const float* __restrict__ f, const float* __restrict__ lin, const float* __restrict__ gout,
                                                          LpSide A, LpSide Bd, int B, int H, int W, int PH, int PW) {
  constexpr int C = CPL * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y, HW = H * W;
  const int p = blockIdx.x * 4 + wave;
  if (p >= HW) return;
  const float* fa = f + ((int64_t)b * HW + p) * C;
  const float* fb = f + ((int64_t)(B + b) * HW + p) * C;
  const float go2 = 2.f * gout[b] / (float)HW;
  float va[CPL], vb[CPL], sa = 0.f, sb = 0.f;
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    va[t] = fa[lane + 64 * t];
    vb[t] = fb[lane + 64 * t];
    sa = fmaf(va[t], va[t], sa);
    sb = fmaf(vb[t], vb[t], sb);
  }
  const float ra = sqrtf(wave_sum(sa)), rb = sqrtf(wave_sum(sb));
  const float ia = 1.f / (ra + 1e-10f), ib = 1.f / (rb + 1e-10f);
  float q[CPL], da = 0.f, db = 0.f;
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    q[t] = go2 * lin[lane + 64 * t] * lp_diff(va[t], ia, vb[t], ib);
    da = fmaf(q[t], va[t], da);
    db = fmaf(q[t], vb[t], db);
  }
  // d/df of f / (|f| + eps): q / n - (q . f) f / (n^2 |f|); zero-norm pixel: defined as 0
  const float ka = ra > 0.f ? wave_sum(da) * ia * ia / ra : 0.f, kb = rb > 0.f ? wave_sum(db) * ib * ib / rb : 0.f;
  const float ma = ra > 0.f ? ia : 0.f, mb = rb > 0.f ? ib : 0.f;
  const int y = p / W, x = p - y * W;
  const int64_t o = ((int64_t)b * HW + p) * C;
  if (A.g) {
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int c = lane + 64 * t;
      float g = q[t] * ma - ka * va[t];
      if (A.gin) g += A.gin[o + c];
      if (A.gp) g += lp_pool_gather(A.gp, A.idx, b, y, x, c, PH, PW, C);
      A.g[o + c] = va[t] > 0.f ? g : 0.f;
    }
  }
  if (Bd.g) {
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int c = lane + 64 * t;
      float g = kb * vb[t] - q[t] * mb;
      if (Bd.gin) g += Bd.gin[o + c];
      if (Bd.gp) g += lp_pool_gather(Bd.gp, Bd.idx, b, y, x, c, PH, PW, C);
      Bd.g[o + c] = vb[t] > 0.f ? g : 0.f;
    }
  }
}

// NHWC feature map of the workspace -> contiguous NCHW
__global__ void lp_feature_kernel(const float* __restrict__ f, float* __restrict__ out, int C, int HW, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int p = (int)(i % HW);
  const int64_t r = i / HW;
  const int c = (int)(r % C);
  const int64_t n = r / C;
  out[i] = f[(n * HW + p) * C + c];
}

inline unsigned lp_blocks(int64_t total) { return (unsigned)cdiv64(total, 256); }

}  // namespace

extern "C" {

int64_t ppst_lpips_pack_floats(void) { return lp_pack_layout().total; }

int ppst_lpips_pack(const void* const* weight, const void* const* bias, const void* const* lin, const void* shift, const void* scale,
                    void* pack, void* stream) {
  if (!weight || !bias || !lin || !shift || !scale || !pack) return PPST_ENULL;
  for (int l = 0; l < 5; ++l)
    if (!weight[l] || !bias[l] || !lin[l]) return PPST_ENULL;
  const LpPack P = lp_pack_layout();
  float* out = (float*)pack;
  hipStream_t st = as_stream(stream);
  for (int l = 0; l < 5; ++l) {
    const LpLayer &lf = LP_FWD[l], &lb = LP_BWD[l];
    int64_t tot = lp_wfloats(lf);
    PPST_LAUNCH(lp_pack_kernel, dim3(lp_blocks(tot)), dim3(256), 0, st, (const float*)weight[l], out + P.wf[l], lf.K, lf.cin, lf.cout, lf.coutp,
                l == 0 ? 1 : 0, tot);
    tot = lp_wfloats(lb);
    PPST_LAUNCH(lp_pack_kernel, dim3(lp_blocks(tot)), dim3(256), 0, st, (const float*)weight[l], out + P.wb[l], lb.K, lb.cin, lb.cout, lb.coutp,
                l == 0 ? 3 : 2, tot);
    PPST_LAUNCH(lp_copy_kernel, dim3(cdiv(LP_C[l], 256)), dim3(256), 0, st, (const float*)bias[l], out + P.bias[l], LP_C[l]);
    PPST_LAUNCH(lp_copy_kernel, dim3(cdiv(LP_C[l], 256)), dim3(256), 0, st, (const float*)lin[l], out + P.lin[l], LP_C[l]);
  }
  PPST_LAUNCH(lp_copy_kernel, dim3(1), dim3(256), 0, st, (const float*)shift, out + P.shift, 3);
  PPST_LAUNCH(lp_copy_kernel, dim3(1), dim3(256), 0, st, (const float*)scale, out + P.scale, 3);
  return PPST_LAUNCH_CHECK();
}

int ppst_lpips_dims(int H, int W, int* hw) {
  if (!hw) return PPST_ENULL;
  LpDims d;
  if (lp_dims(H, W, &d)) return PPST_EINVAL;
  for (int l = 0; l < 5; ++l) { hw[2 * l] = d.h[l]; hw[2 * l + 1] = d.w[l]; }
  return PPST_OK;
}

int64_t ppst_lpips_ws(int n, int H, int W) {
  LpDims d;
  if (n < 0 || n > 65536 || lp_dims(H, W, &d)) return PPST_EINVAL;
  return lp_ws_layout(d, n).bytes + 16;
}

int ppst_lpips_trunk(const void* pack, const void* a, const int64_t* a_strides, int na, const void* b, const int64_t* b_strides, int nb,
                     int H, int W, void* ws, void* stream) {
  LpDims d;
  if (na < 0 || nb < 0 || na + nb > 65536 || lp_dims(H, W, &d)) return PPST_EINVAL;
  const int n = na + nb;
  if (n == 0) return PPST_OK;
  if (!pack || !ws || (na && (!a || !a_strides)) || (nb && (!b || !b_strides))) return PPST_ENULL;
  if ((int64_t)n * d.ZH * d.ZW * 64 > 0x7fffffffll / 4) return PPST_EINVAL;
  const LpPack P = lp_pack_layout();
  const LpWs L = lp_ws_layout(d, n);
  const float* pk = (const float*)pack;
  float* w = (float*)ws;
  hipStream_t st = as_stream(stream);
  LpStr sa = {0, 0, 0, 0}, sb = {0, 0, 0, 0};
  if (na) sa = {a_strides[0], a_strides[1], a_strides[2], a_strides[3]};
  if (nb) sb = {b_strides[0], b_strides[1], b_strides[2], b_strides[3]};
  const int64_t zt = (int64_t)n * d.ZH * d.ZW * 48;
  PPST_LAUNCH(lp_repack_kernel, dim3(lp_blocks(zt)), dim3(256), 0, st, (const float*)a, sa, na, (const float*)b, sb, H, W, d.ZH, d.ZW,
              pk + P.shift, pk + P.scale, w + L.z, zt);
  int rc = PPST_LAUNCH_CHECK();
  if (rc) return rc;
  const float* in = w + L.z;
  int ih = d.ZH, iw = d.ZW;
  for (int l = 0; l < 5; ++l) {
    rc = lp_conv(LP_FWD[l], in, pk + P.wf[l], pk + P.bias[l], w + L.f[l], n, ih, iw, d.h[l], d.w[l], true, st);
    if (rc) return rc;
    in = w + L.f[l]; ih = d.h[l]; iw = d.w[l];
    if (l < 2) {
      const int64_t tot = (int64_t)n * d.ph[l] * d.pw[l] * (LP_C[l] / 4);
      PPST_LAUNCH(lp_pool_kernel, dim3(lp_blocks(tot)), dim3(256), 0, st, w + L.f[l], w + L.p[l], (unsigned char*)ws + L.idx[l], d.h[l], d.w[l],
                  d.ph[l], d.pw[l], LP_C[l] / 4, tot);
      rc = PPST_LAUNCH_CHECK();
      if (rc) return rc;
      in = w + L.p[l]; ih = d.ph[l]; iw = d.pw[l];
    }
  }
  return PPST_OK;
}

int ppst_lpips_feature(const void* ws, int n, int H, int W, int layer, void* out_nchw, void* stream) {
  LpDims d;
  if (n < 0 || n > 65536 || layer < 0 || layer > 4 || lp_dims(H, W, &d)) return PPST_EINVAL;
  if (n == 0) return PPST_OK;
  if (!ws || !out_nchw) return PPST_ENULL;
  const LpWs L = lp_ws_layout(d, n);
  const int64_t tot = (int64_t)n * d.h[layer] * d.w[layer] * LP_C[layer];
  PPST_LAUNCH(lp_feature_kernel, dim3(lp_blocks(tot)), dim3(256), 0, as_stream(stream), (const float*)ws + L.f[layer], (float*)out_nchw,
              LP_C[layer], d.h[layer] * d.w[layer], tot);
  return PPST_LAUNCH_CHECK();
}

int ppst_lpips_tail(const void* pack, void* ws, int B, int H, int W, void* out, void* stream) {
  LpDims d;
  if (B < 0 || B > 32768 || lp_dims(H, W, &d)) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!pack || !ws || !out) return PPST_ENULL;
  const LpPack P = lp_pack_layout();
  const LpWs L = lp_ws_layout(d, 2 * B);
  const float* pk = (const float*)pack;
  float* w = (float*)ws;
  hipStream_t st = as_stream(stream);
  LpFin fin;
  int64_t off = L.part;
  for (int l = 0; l < 5; ++l) {
    const int HW = d.h[l] * d.w[l];
    fin.off[l] = off; fin.nblk[l] = L.nblk[l]; fin.inv_hw[l] = 1.f / (float)HW;
    dim3 grid((unsigned)L.nblk[l], (unsigned)B);
    const float* f = w + L.f[l];
    const float* lin = pk + P.lin[l];
    switch (LP_C[l] / 64) {
      case 1: PPST_LAUNCH(lp_tail_fwd_kernel<1>, grid, dim3(256), 0, st, f, lin, w + off, B, HW); break;
      case 3: PPST_LAUNCH(lp_tail_fwd_kernel<3>, grid, dim3(256), 0, st, f, lin, w + off, B, HW); break;
      case 6: PPST_LAUNCH(lp_tail_fwd_kernel<6>, grid, dim3(256), 0, st, f, lin, w + off, B, HW); break;
      default: PPST_LAUNCH(lp_tail_fwd_kernel<4>, grid, dim3(256), 0, st, f, lin, w + off, B, HW); break;
    }
    const int rc = PPST_LAUNCH_CHECK();
    if (rc) return rc;
    off += (int64_t)B * L.nblk[l];
  }
  PPST_LAUNCH(lp_tail_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)w, fin, (float*)out);
  return PPST_LAUNCH_CHECK();
}

// two buffers, each large enough for any gradient map of `sides * B` images
static int64_t lp_bwd_buf_floats(const LpDims& d, int n) {
  int64_t m = (int64_t)d.ZH * d.ZW * 48;
  for (int l = 0; l < 5; ++l) m = m > (int64_t)d.h[l] * d.w[l] * LP_C[l] ? m : (int64_t)d.h[l] * d.w[l] * LP_C[l];
  return up4(m * n);
}

int64_t ppst_lpips_bwd_ws(int B, int H, int W, int which) {
  LpDims d;
  if (B < 0 || B > 32768 || which < 1 || which > 3 || lp_dims(H, W, &d)) return PPST_EINVAL;
  return 2 * lp_bwd_buf_floats(d, (which == 3 ? 2 : 1) * B) * 4 + 16;
}

int ppst_lpips_backward(const void* pack, const void* ws, const void* gout, int B, int H, int W, int which, void* ga, void* gb, void* bws,
                        void* stream) {
  LpDims d;
  if (B < 0 || B > 32768 || which < 1 || which > 3 || lp_dims(H, W, &d)) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!pack || !ws || !gout || !bws || ((which & 1) && !ga) || ((which & 2) && !gb)) return PPST_ENULL;
  const int sides = which == 3 ? 2 : 1, n = sides * B;
  if ((int64_t)n * d.ZH * d.ZW * 64 > 0x7fffffffll / 4) return PPST_EINVAL;
  const LpPack P = lp_pack_layout();
  const LpWs L = lp_ws_layout(d, 2 * B);
  const float* pk = (const float*)pack;
  const float* w = (const float*)ws;
  hipStream_t st = as_stream(stream);
  const int64_t bufsz = lp_bwd_buf_floats(d, n);
  float* G = (float*)bws;            // gradients of the pre-activations (tail output)
  float* U = G + bufsz;              // what the layer below receives (conv output)
  int rc;
  for (int l = 4; l >= 0; --l) {
    const int HW = d.h[l] * d.w[l], C = LP_C[l];
    const int64_t side = (int64_t)B * HW * C;                 // one side's gradient map
    const bool pooled = l < 2;                                // the layer above reads this one through a pool
    const int PH = pooled ? d.ph[l] : 0, PW = pooled ? d.pw[l] : 0;
    const int64_t pside = (int64_t)B * PH * PW * C;
    LpSide A = {nullptr, nullptr, nullptr, nullptr}, Bd = A;
    if (which & 1) {
      A.g = G;
      if (l < 4) { if (pooled) { A.gp = U; A.idx = (const unsigned char*)ws + L.idx[l]; } else A.gin = U; }
    }
    if (which & 2) {
      const int64_t so = which == 3 ? 1 : 0;
      Bd.g = G + so * side;
      if (l < 4) { if (pooled) { Bd.gp = U + so * pside; Bd.idx = (const unsigned char*)ws + L.idx[l] + pside; } else Bd.gin = U + so * side; }
    }
    dim3 grid((unsigned)cdiv(HW, 4), (unsigned)B);
    const float* f = w + L.f[l];
    const float* lin = pk + P.lin[l];
    const float* go = (const float*)gout;
    switch (C / 64) {
      case 1: PPST_LAUNCH(lp_tail_bwd_kernel<1>, grid, dim3(256), 0, st, f, lin, go, A, Bd, B, d.h[l], d.w[l], PH, PW); break;
      case 3: PPST_LAUNCH(lp_tail_bwd_kernel<3>, grid, dim3(256), 0, st, f, lin, go, A, Bd, B, d.h[l], d.w[l], PH, PW); break;
      case 6: PPST_LAUNCH(lp_tail_bwd_kernel<6>, grid, dim3(256), 0, st, f, lin, go, A, Bd, B, d.h[l], d.w[l], PH, PW); break;
      default: PPST_LAUNCH(lp_tail_bwd_kernel<4>, grid, dim3(256), 0, st, f, lin, go, A, Bd, B, d.h[l], d.w[l], PH, PW); break;
    }
    rc = PPST_LAUNCH_CHECK();
    if (rc) return rc;
    // the conv's input gradient: to the pooled map / feature map below, or (conv1) to the space-to-depth image
    int oh, ow;
    if (l == 0) { oh = d.ZH; ow = d.ZW; }
    else if (l <= 2) { oh = d.ph[l - 1]; ow = d.pw[l - 1]; }
    else { oh = d.h[l - 1]; ow = d.w[l - 1]; }
    rc = lp_conv(LP_BWD[l], G, pk + P.wb[l], nullptr, U, n, d.h[l], d.w[l], oh, ow, false, st);
    if (rc) return rc;
  }
  const int64_t zside = (int64_t)B * d.ZH * d.ZW * 48, tot = (int64_t)B * 3 * H * W;
  if (which & 1) {
    PPST_LAUNCH(lp_unrepack_kernel, dim3(lp_blocks(tot)), dim3(256), 0, st, (const float*)U, (float*)ga, H, W, d.ZH, d.ZW, pk + P.scale, tot);
    rc = PPST_LAUNCH_CHECK();
    if (rc) return rc;
  }
  if (which & 2) {
    PPST_LAUNCH(lp_unrepack_kernel, dim3(lp_blocks(tot)), dim3(256), 0, st, (const float*)U + (which == 3 ? zside : 0), (float*)gb, H, W, d.ZH,
                d.ZW, pk + P.scale, tot);
    rc = PPST_LAUNCH_CHECK();
    if (rc) return rc;
  }
  return PPST_OK;
}

}  // extern "C"
