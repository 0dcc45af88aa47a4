// The encoders' first ResBlock (stylegan2_layers.py:552-579, no norm: E2) as ONE kernel whose intermediates stay in LDS:
//     out = (lrelu(conv2_s2(blur(lrelu(conv1(x) + b1))) + b2) + skip1x1(blur_down2(x))) / sqrt 2,     32 -> 32 -> 64 channels.
// The unfused path runs five HBM passes (skip blur, conv1, skip 1x1, blur to space-to-depth, conv2) that move about nine times
// the input tensor; the result needs x read once and the output written once.
//
// A tile is TOH x TOW outputs (8 x 8) of one image.  Its receptive field: 3x3 stride-2 conv over the blurred extent (2 TOH + 1)^2
// <- [1,2,1]^2 blur, reflect pad (2, 1) <- y1 on (2 TOH + 3)^2 <- 3x3 conv, reflect pad 1 <- x on (2 TOH + 5)^2.  Blocks are
// persistent (one 512-thread block per CU, two waves per SIMD): every weight fragment a wave needs -- one 16-channel tile each of
// conv1, conv2 and the skip, 152 registers -- is loaded once per launch, and the x patch of the NEXT tile is in flight (28
// registers per thread) while this one computes.  Per tile:
//   1. the x patch from registers to LDS: split to bf16 hi / lo ONCE (image coordinates went through conv1's reflect map, then
//      a clamp: positions further out feed only y1 positions no output reads); its interior also as fp32 for the skip;
//   2. the skip's blur (zero pad (1, 0), every second sample) on the VALU from the fp32 copy; conv1 by MFMA from LDS over every
//      pixel of the y1 region (halo recomputed: 19^2 for 16^2), weights as the A operand as in conv1x1.hip -- a lane's accumulator
//      is 4 consecutive channels of one pixel -- bias + leaky ReLU, y1 kept in LDS as fp32;
//   3. blur of y1 on the VALU, taps in upfirdn2d_chan's order, rows / columns through the blur's reflect map into the y1 region
//      (a reflected index of the image always lies inside the region of the tile that needs it), split to bf16 hi / lo into the
//      image conv2 reads -- it takes the x patch's place;
//   4. conv2 (stride 2) and the skip's 1x1 by MFMA into separate accumulators; epilogue (lrelu(conv2 + b2) + skip) / sqrt 2 with
//      conv_epi_value4 (residual after the activation), 16-B stores.
// bf16 images in LDS: [hi | lo][k-group g of 8 channels][pixel][16 B], planes a multiple of 256 B apart: the 16 lanes that one
// ds_read_b128 cycle serves read consecutive pixels of one or two planes, each run on its own banks.  The blurred image numbers a
// row's pixels [even columns | odd columns] (20 per row), so the stride-2 taps of eight outputs are consecutive too and the
// second output row of an m-tile lands eight slots further.
// Per output element the MFMA order is al*bh, ah*bl, ah*bh per tap, taps ky-major: conv1 and the skip equal the direct kernels
// bit for bit; conv2 sums its nine taps in ky-major order where the space-to-depth form groups them by phase (fp32 reassociation).
// Weights: the ppst_conv_pack blobs (N tile 64, 'conv' step table) of the three layers.
#include "conv_common.h"

namespace {

constexpr int EB_NT = 512;
constexpr int EB_SLOTS = EB_NT / 8;   // pixels the block's threads cover at four channels each
constexpr int EB_BLOB = 8192;       // bytes per tap of a packed weight (bn = 64: [hi | lo][g 4][n 64][8] bf16)
constexpr int EB_YS = 36;           // floats per pixel of the y1 image (32 + 4: the 8 lanes of a ds_write_b128 cycle on 8 bank quads)

template <int TOH, int TOW>
struct EbGeom {
  static constexpr int Y1H = 2 * TOH + 3, Y1W = 2 * TOW + 3;     // y1 region
  static constexpr int XH = Y1H + 2, XW = Y1W + 2;               // x patch
  static constexpr int BH = 2 * TOH + 1, BW = 2 * TOW + 1;       // blurred extent
  static constexpr int BROW = 2 * TOW + 4, BHALF = TOW + 2;      // blurred image: pixels per row, start of the odd columns
  static constexpr int NPX = TOH * TOW;
  static constexpr int XPL = (XH * XW + 15) / 16 * 16;           // pixels per plane
  static constexpr int BPL = (BH * BROW + 15) / 16 * 16;
  static constexpr int X_BYTES = 8 * XPL * 16, B_BYTES = 8 * BPL * 16, S_BYTES = 8 * NPX * 16;
  static constexpr int Y1_BYTES = Y1H * Y1W * EB_YS * 4;
  static constexpr int XF_BYTES = BH * BW * 128;                 // fp32 x on the skip's extent: rows / columns 2 o - 1 .. 2 o + 1
  static constexpr int LDS = X_BYTES + Y1_BYTES + XF_BYTES + S_BYTES;
  static constexpr int NX = XH * XW * 8, NIT = (NX + EB_NT - 1) / EB_NT;
  static_assert(B_BYTES <= X_BYTES, "the blurred image takes the x patch's place");
  static_assert(NPX % 16 == 0 && TOW + 1 <= BHALF && LDS <= 160 * 1024, "16-pixel m-tiles; one block per CU");
};

struct EbArgs {
  const float* x;
  const unsigned char* w1;
  const unsigned char* w2;
  const unsigned char* ws;
  const float* b1;
  const float* b2;
  const float* blur;
  float* y;
  int H, W, OH, OW, tiles_y, tiles_x, nblocks;
};

__device__ __forceinline__ bf16x8 eb_wfrag(const unsigned char* w, int tap, int hl, int nt16, int lane) {
  return *(const bf16x8*)(w + tap * EB_BLOB + hl * (EB_BLOB / 2) + (((lane >> 4) * 64 + nt16 * 16 + (lane & 15)) << 4));
}
__device__ __forceinline__ f32x4 eb_mfma3(bf16x8 wh, bf16x8 wl, bf16x8 xh, bf16x8 xl, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc, 0, 0, 0);
}
// four channels (quad cq of a pixel's 32) of pixel px into a bf16 image of `plane` pixels per plane
__device__ __forceinline__ void eb_put_split(unsigned char* img, int plane, int px, int cq, float4 v) {
  uint2 hi, lo;
  split_bf16x4(v, hi, lo);
  unsigned char* const d = img + (((cq >> 1) * plane + px) << 4) + (cq & 1) * 8;
  *(uint2*)d = hi;
  *(uint2*)(d + plane * 64) = lo;
}
__device__ __forceinline__ void eb_fir(float4& acc, float4 v, float f) {
  acc.x = fmaf(v.x, f, acc.x); acc.y = fmaf(v.y, f, acc.y); acc.z = fmaf(v.z, f, acc.z); acc.w = fmaf(v.w, f, acc.w);
}
__device__ __forceinline__ float4 eb_bias4(const float* b, int n0) { return make_float4(b[n0], b[n0 + 1], b[n0 + 2], b[n0 + 3]); }

struct EbTile { int b, oy0, ox0; };
template <int TOH, int TOW>
__device__ __forceinline__ EbTile eb_tile(const EbArgs& a, int v) {
  int id = xcd_block_id(v, a.nblocks);
  EbTile t;
  t.ox0 = (id % a.tiles_x) * TOW;
  id /= a.tiles_x;
  t.oy0 = (id % a.tiles_y) * TOH;
  t.b = id / a.tiles_y;
  return t;
}
// Items of a P-pixel-wide image walked EB_SLOTS pixels at a time: thread (pixel slot r = tid >> 3, channel quad cq = tid & 7) takes
// pixels r, r + EB_SLOTS, ..: (row, column) advance by (EB_SLOTS / P, EB_SLOTS % P) with one carry -- no division in the tile loop.
template <int P>
__device__ __forceinline__ void eb_step(int& row, int& col) {
  row += EB_SLOTS / P;
  col += EB_SLOTS % P;
  if (col >= P) { col -= P; ++row; }
}
// the x patch of a tile, item by item (item = four channels of a patch pixel; the items past the end repeat the last one: every
// request is unconditional and in bounds).  A patch inside the image needs no index map.
template <int TOH, int TOW>
__device__ __forceinline__ void eb_fetch(const EbArgs& a, const EbTile& t, int pr, int cq, float4 (&v)[EbGeom<TOH, TOW>::NIT]) {
  using G = EbGeom<TOH, TOW>;
  const float* const xb = a.x + (int64_t)t.b * a.H * a.W * 32 + cq * 4;
  const int y0 = 2 * t.oy0 - 3, x0 = 2 * t.ox0 - 3;
  const bool inside = y0 >= 0 && x0 >= 0 && y0 + G::XH <= a.H && x0 + G::XW <= a.W;
  auto go = [&](auto in_c) {
    int j = pr / G::XW, i = pr % G::XW;
#pragma unroll
    for (int it = 0; it < G::NIT; ++it) {
      const bool past = (it + 1) * EB_SLOTS > G::XH * G::XW && it * EB_SLOTS + pr >= G::XH * G::XW;
      const int jj = past ? G::XH - 1 : j, ii = past ? G::XW - 1 : i;
      const int ry = in_c.value ? y0 + jj : conv_pad_index(y0 + jj, a.H, PPST_PAD_REFLECT), rx = in_c.value ? x0 + ii : conv_pad_index(x0 + ii, a.W, PPST_PAD_REFLECT);
      v[it] = *(const float4*)(xb + (ry * a.W + rx) * 32);
      eb_step<G::XW>(j, i);
    }
  };
  if (inside) go(EpiC<1>{}); else go(EpiC<0>{});
}

template <int TOH, int TOW>
__global__ __launch_bounds__(EB_NT) void encoder_resblock_kernel(EbArgs a) {
  using G = EbGeom<TOH, TOW>;
  __shared__ __attribute__((aligned(256))) unsigned char lds[G::LDS];
  unsigned char* const xs = lds;                         // phases 1-2: x patch; 3-4: blurred image
  unsigned char* const bs = lds;
  float* const y1s = (float*)(lds + G::X_BYTES);
  float* const xf = (float*)(lds + G::X_BYTES + G::Y1_BYTES);
  unsigned char* const ss = lds + G::X_BYTES + G::Y1_BYTES + G::XF_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cq = tid & 7;                                // the VALU phases: channel quad; pixel slot tid >> 3 (eb_step)
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // the wave's weights, for the whole launch: conv1 n-tile nt1 (m-tiles mg1, mg1 + 4, ..), conv2 / skip n-tile nt2 (m-tile group mg2)
  const int nt1 = wave & 1, mg1 = wave >> 1, nt2 = wave & 3, mg2 = wave >> 2;
  bf16x8 w1h[9], w1l[9], w2h[9], w2l[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    w1h[t] = eb_wfrag(a.w1, t, 0, nt1, lane);
    w1l[t] = eb_wfrag(a.w1, t, 1, nt1, lane);
    w2h[t] = eb_wfrag(a.w2, t, 0, nt2, lane);
    w2l[t] = eb_wfrag(a.w2, t, 1, nt2, lane);
  }
  const bf16x8 sh = eb_wfrag(a.ws, 0, 0, nt2, lane), sl = eb_wfrag(a.ws, 0, 1, nt2, lane);
  const float4 b1v = eb_bias4(a.b1, nt1 * 16 + (lane >> 4) * 4);
  const float4 b2v = eb_bias4(a.b2, nt2 * 16 + (lane >> 4) * 4);
  float kf[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) kf[i] = a.blur[8 - i];

  float4 v[G::NIT];
  if ((int)blockIdx.x < a.nblocks) eb_fetch<TOH, TOW>(a, eb_tile<TOH, TOW>(a, blockIdx.x), tid >> 3, cq, v);
  for (int work = blockIdx.x; work < a.nblocks; work += gridDim.x) {
    const EbTile tl = eb_tile<TOH, TOW>(a, work);
    const int oy0 = tl.oy0, ox0 = tl.ox0;
    const int y1r0 = 2 * oy0 - 2, y1c0 = 2 * ox0 - 2;    // image position of the y1 region's corner; the x patch starts one further out
    // the pixel slot, opaque per tile: the per-item (row, column) values derived from it are then recomputed here (a few integer
    // operations each) and not carried across the tile loop in registers the resident weights do not leave
    int pr = tid >> 3, r16 = lane & 15, g = lane >> 4;
    asm volatile("" : "+v"(pr), "+v"(r16), "+v"(g));

    // ---- 1. x patch -> LDS; the next tile's requests go out
    {
      int j = pr / G::XW, i = pr % G::XW;
#pragma unroll
      for (int it = 0; it < G::NIT; ++it) {
        eb_put_split(xs, G::XPL, min(pr + it * EB_SLOTS, G::XH * G::XW - 1), cq, v[it]);     // (a repeated last item stores the same bytes)
        if ((unsigned)(j - 2) < (unsigned)G::BH && (unsigned)(i - 2) < (unsigned)G::BW) *(float4*)(xf + ((j - 2) * G::BW + (i - 2)) * 32 + cq * 4) = v[it];
        eb_step<G::XW>(j, i);
      }
    }
    if (work + (int)gridDim.x < a.nblocks) eb_fetch<TOH, TOW>(a, eb_tile<TOH, TOW>(a, work + gridDim.x), pr, cq, v);
    __syncthreads();

    // ---- 2a. the skip's blur: zero pad (1, 0), samples 2 o - 1 .. 2 o + 1 (row / column -1 of the image: zero)
    for (int pix = pr; pix < G::NPX; pix += EB_SLOTS) {
      const int ly = pix / TOW, lx = pix - ly * TOW;
      float4 acc = zero4;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          float4 t = *(const float4*)(xf + ((2 * ly + ky) * G::BW + 2 * lx + kx) * 32 + cq * 4);
          if (2 * (oy0 + ly) - 1 + ky < 0 || 2 * (ox0 + lx) - 1 + kx < 0) t = zero4;
          eb_fir(acc, t, kf[ky * 3 + kx]);
        }
      eb_put_split(ss, G::NPX, pix, cq, acc);
    }
    // ---- 2b. conv1 over the y1 region: m-tiles of 16 consecutive region pixels, three per pass
    {
      constexpr int NP1 = G::Y1H * G::Y1W, NM1 = (NP1 + 15) / 16, PASSES = (NM1 + 11) / 12;
      for (int pass = 0; pass < PASSES; ++pass) {
        int p[3];
        const unsigned char* src[3];
        f32x4 acc[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          p[u] = (mg1 + 4 * (pass * 3 + u)) * 16 + r16;
          const int pc = min(p[u], NP1 - 1), qy = pc / G::Y1W, qx = pc - qy * G::Y1W;
          src[u] = xs + ((g * G::XPL + qy * G::XW + qx) << 4);
          acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int off = ((t / 3) * G::XW + (t % 3)) * 16;
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            const bf16x8 xh = *(const bf16x8*)(src[u] + off), xl = *(const bf16x8*)(src[u] + off + G::XPL * 64);
            acc[u] = eb_mfma3(w1h[t], w1l[t], xh, xl, acc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          float o[4];
          conv_epi_value4(o, make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]), b1v, 0.f, zero4, 0.f, 1.f, EpiC<PPST_ACT_LRELU>{}, EpiC<0>{});
          if (p[u] < NP1) *(float4*)(y1s + p[u] * EB_YS + nt1 * 16 + g * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
      }
    }
    __syncthreads();                                     // y1 and the skip image complete; the x patch is dead

    // ---- 3. blur of y1, reflect pad (2, 1): blurred (i, j) of the tile = rows 2 oy0 + i - 2 .. 2 oy0 + i of y1
    // (a region inside the image needs no index map: the nine taps are constant offsets from the item's first one)
    {
      const bool inside = y1r0 >= 0 && y1c0 >= 0 && y1r0 + G::Y1H <= a.H && y1c0 + G::Y1W <= a.W;
      auto go = [&](auto in_c) {
        int i = pr / G::BW, j = pr % G::BW;
#pragma unroll 1                                         // (the resident weights leave room for one item's reads)
        for (int it = 0; it < (G::BH * G::BW + EB_SLOTS - 1) / EB_SLOTS; ++it) {
          if ((it + 1) * EB_SLOTS <= G::BH * G::BW || it * EB_SLOTS + pr < G::BH * G::BW) {
            int ro[3], co[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              if (in_c.value) { ro[k] = (i + k) * G::Y1W; co[k] = j + k; }
              else {
                const int r = conv_pad_index(y1r0 + i + k, a.H, PPST_PAD_REFLECT) - y1r0, c = conv_pad_index(y1c0 + j + k, a.W, PPST_PAD_REFLECT) - y1c0;
                ro[k] = min(max(r, 0), G::Y1H - 1) * G::Y1W;
                co[k] = min(max(c, 0), G::Y1W - 1);
              }
            }
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
              for (int kx = 0; kx < 3; ++kx) eb_fir(acc, *(const float4*)(y1s + (ro[ky] + co[kx]) * EB_YS + cq * 4), kf[ky * 3 + kx]);
            eb_put_split(bs, G::BPL, i * G::BROW + (j & 1) * G::BHALF + (j >> 1), cq, acc);
          }
          eb_step<G::BW>(i, j);
        }
      };
      if (inside) go(EpiC<1>{}); else go(EpiC<0>{});
    }
    __syncthreads();

    // ---- 4. conv2 (stride 2) + skip 1x1: m-tiles of 16 consecutive tile pixels, group mg2 takes its half of them
    {
      constexpr int MT = G::NPX / 32;
      int ly[MT], lx[MT];
      const unsigned char* src[MT];
      f32x4 acc[MT], accs[MT];
#pragma unroll
      for (int u = 0; u < MT; ++u) {
        const int pl = (mg2 * MT + u) * 16 + r16;
        ly[u] = pl / TOW;
        lx[u] = pl - ly[u] * TOW;
        src[u] = bs + ((g * G::BPL + 2 * ly[u] * G::BROW + lx[u]) << 4);
        const unsigned char* sp = ss + ((g * G::NPX + pl) << 4);
        accs[u] = eb_mfma3(sh, sl, *(const bf16x8*)sp, *(const bf16x8*)(sp + G::NPX * 64), (f32x4){0.f, 0.f, 0.f, 0.f});
        acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int kx = t % 3, off = ((t / 3) * G::BROW + (kx & 1) * G::BHALF + (kx >> 1)) * 16;
#pragma unroll
        for (int u = 0; u < MT; ++u) {
          const bf16x8 xh = *(const bf16x8*)(src[u] + off), xl = *(const bf16x8*)(src[u] + off + G::BPL * 64);
          acc[u] = eb_mfma3(w2h[t], w2l[t], xh, xl, acc[u]);
        }
      }
      float* const yb = a.y + (int64_t)tl.b * a.OH * a.OW * 64;
#pragma unroll
      for (int u = 0; u < MT; ++u) {
        const int oy = oy0 + ly[u], ox = ox0 + lx[u];
        float o[4];
        conv_epi_value4(o, make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]), b2v, 0.f,
                        make_float4(accs[u][0], accs[u][1], accs[u][2], accs[u][3]), 0.f, 0.70710678118654752f, EpiC<PPST_ACT_LRELU>{}, EpiC<2>{});
        if (oy < a.OH && ox < a.OW) PPST_EPI_STORE(yb + (oy * a.OW + ox) * 64 + nt2 * 16 + g * 4, o);
      }
    }
    __syncthreads();                                     // the blurred image is read: the next patch may take its place
  }
}

// blocks of the persistent launch: one per CU, a multiple of 8 so that block & 7 stays the XCD of xcd_block_id's ranges
int eb_grid(int64_t tiles) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8) cus = 256;
  cus &= ~7;
  return (int)(tiles < cus ? tiles : cus);
}

}  // namespace

extern "C" int ppst_encoder_resblock(const void* x, int x_st, int B, int H, int W, int cin, int cmid, int cout, int x_ld, const void* w1,
                                     const void* w2, const void* ws, const void* b1, const void* b2, const void* blur, void* y, void* stream) {
  constexpr int TOH = 8, TOW = 8;
  if (x_st != PPST_ST_F32 || cin != 32 || cmid != 32 || cout != 64 || x_ld != 32 || B < 1 || H < 4 || W < 4 || (H & 1) || (W & 1)) return PPST_EINVAL;
  if (!x || !w1 || !w2 || !ws || !b1 || !b2 || !blur || !y) return PPST_ENULL;
  if ((int64_t)H * W * 32 >= (1ll << 31)) return PPST_EINVAL;                 // 32-bit element offsets inside an image
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)ws) % 16 || ((uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)blur) % 4)
    return PPST_EINVAL;
  EbArgs a;
  a.x = (const float*)x; a.w1 = (const unsigned char*)w1; a.w2 = (const unsigned char*)w2; a.ws = (const unsigned char*)ws;
  a.b1 = (const float*)b1; a.b2 = (const float*)b2; a.blur = (const float*)blur; a.y = (float*)y;
  a.H = H; a.W = W; a.OH = H / 2; a.OW = W / 2;
  a.tiles_y = cdiv(a.OH, TOH); a.tiles_x = cdiv(a.OW, TOW);
  const int64_t tiles = (int64_t)B * a.tiles_y * a.tiles_x;
  if (tiles >= (1ll << 31)) return PPST_EINVAL;
  a.nblocks = (int)tiles;
  PPST_LAUNCH((encoder_resblock_kernel<TOH, TOW>), dim3((unsigned)eb_grid(tiles)), dim3(EB_NT), 0, as_stream(stream), a);
  return PPST_LAUNCH_CHECK();
}
