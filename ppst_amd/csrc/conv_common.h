// What the forward conv kernel families share (conv_mfma.hip, conv_mfma2.hip, conv1x1.hip, conv_wino.hip, conv_f32.hip; train.hip
// takes the block map): block map, padding index, normalise-on-load activation, the output arithmetic and its dispatch, the
// argument block of the two tile kernels and their transposition epilogue.  The families must agree to the bit wherever they
// compute the same sum (tests/gpu_diag.py t_conv_variants, t_conv1x1_stream; tests/test_gpu_conv_epilogue.py): each of these is
// stated here once.  Device / host helpers only -- no translation unit of its own.
#pragma once
#include "common.h"

// ---- block map: the 8 XCDs take blocks round-robin (block id & 7); this bijective remap gives each XCD a CONTIGUOUS range of work
// ids, so that co-resident blocks of one XCD stream the same weight blobs / neighbouring tiles from its L2
__device__ __forceinline__ int xcd_block_id(int id, int nblocks) {
  const int q = nblocks >> 3, r = nblocks & 7, xcd = id & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}

// ---- padding: index i of an extent n under reflect / replicate padding (zero padding is the caller's: it tests the bounds first);
// the clamp is replicate, and the safety net for reflect on far-out (masked) tile pixels
__device__ __forceinline__ int conv_pad_index(int i, int n, int mode) {
  if (mode == PPST_PAD_REFLECT) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
  }
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// ---- normalise-on-load: the activation of the producer layer, applied to t = a * x + s while the tile is staged
__device__ __forceinline__ float conv_in_act(float t, int in_act, float in_slope) {
  if (in_act == PPST_ACT_LRELU) return (t > 0.f ? t : t * 0.2f) * 1.41421356237309515f;
  if (in_act == PPST_ACT_PRELU) return t >= 0.f ? t : t * in_slope;
  return t;
}

// ---- output arithmetic.  Tags for (activation, residual mode: 0 none, 1 joins before the activation, 2 after): EpiC = compile-time,
// EpiR = run-time.  The fp32-class kernels instantiate their pass loops per combination -- as run-time values hipcc evaluated the
// leaky-ReLU AND the PReLU branch of every element and selected: ~30 VALU instructions per element (27.7 k cycles per tile, 9 % of a
// 72-step tile, profiles/r02_conv_trace_v2.txt) against ~10 when specialised; the reduced-precision kernels
// take the one generic instance (shorter build).
template <int V> struct EpiC { static constexpr int value = V; };
struct EpiR { int value; };

// ((acc + bias) + nz) [+ res] -> lrelu * sqrt 2 | prelu -> [+ res] -> * out_scale; nz = noise_weight * noise.  No fused
// multiply-add: every kernel family rounds every step alike.
template <class ActT, class ResT>
__device__ __forceinline__ float conv_epi_value(float acc, float bias, float nz, float res, float slope, float out_scale, ActT act_c,
                                                ResT res_c) {
#pragma clang fp contract(off)
  const int ACT = act_c.value, RES = res_c.value;
  float t = acc + bias + nz;
  if (RES == 1) t += res;
  if (ACT == PPST_ACT_LRELU) t = (t > 0.f ? t : t * 0.2f) * 1.41421356237309515f;
  else if (ACT == PPST_ACT_PRELU) t = t >= 0.f ? t : t * slope;
  if (RES == 2) t += res;
  return t * out_scale;
}
// four consecutive channels of one pixel
template <class ActT, class ResT>
__device__ __forceinline__ void conv_epi_value4(float (&o)[4], float4 v, float4 bv, float nz, float4 rv, float slope, float out_scale,
                                                ActT act_c, ResT res_c) {
  o[0] = conv_epi_value(v.x, bv.x, nz, rv.x, slope, out_scale, act_c, res_c);
  o[1] = conv_epi_value(v.y, bv.y, nz, rv.y, slope, out_scale, act_c, res_c);
  o[2] = conv_epi_value(v.z, bv.z, nz, rv.z, slope, out_scale, act_c, res_c);
  o[3] = conv_epi_value(v.w, bv.w, nz, rv.w, slope, out_scale, act_c, res_c);
}
// ... and their share of the tile statistics (sum, sum of squares; products rounded before they are added, as above)
__device__ __forceinline__ void conv_epi_accum(float4& s1, float4& s2, const float (&o)[4]) {
#pragma clang fp contract(off)
  s1.x += o[0]; s1.y += o[1]; s1.z += o[2]; s1.w += o[3];
  s2.x += o[0] * o[0]; s2.y += o[1] * o[1]; s2.z += o[2] * o[2]; s2.w += o[3] * o[3];
}
// sum of (s1, s2) over lanes lane ^ o, o = FROM, 2 FROM, .. 32
template <int FROM>
__device__ __forceinline__ void conv_epi_xor_sum(float4& s1, float4& s2) {
#pragma unroll
  for (int o = FROM; o < 64; o <<= 1) {
    s1.x += __shfl_xor(s1.x, o, 64); s1.y += __shfl_xor(s1.y, o, 64); s1.z += __shfl_xor(s1.z, o, 64); s1.w += __shfl_xor(s1.w, o, 64);
    s2.x += __shfl_xor(s2.x, o, 64); s2.y += __shfl_xor(s2.y, o, 64); s2.z += __shfl_xor(s2.z, o, 64); s2.w += __shfl_xor(s2.w, o, 64);
  }
}
// (sum, sum of squares) of four channels as the partial-sum rows hold them: interleaved per channel
__device__ __forceinline__ void conv_epi_put_sums(float* r, float4 s1, float4 s2) {
  r[0] = s1.x; r[1] = s2.x; r[2] = s1.y; r[3] = s2.y; r[4] = s1.z; r[5] = s2.z; r[6] = s1.w; r[7] = s2.w;
}

// run FN(act tag, res tag) for a launch's (act, resm): compile-time tags per combination when SPEC, else the one run-time instance
#define CONV_EPI_GO_(FN, A_, resm)                                                                    \
  do {                                                                                                \
    if ((resm) == 0) FN(EpiC<A_>{}, EpiC<0>{});                                                       \
    else if ((resm) == 1) FN(EpiC<A_>{}, EpiC<1>{});                                                  \
    else FN(EpiC<A_>{}, EpiC<2>{});                                                                   \
  } while (0)
#define CONV_EPI_DISPATCH(SPEC, FN, act, resm)                                                        \
  do {                                                                                                \
    if (!(SPEC)) FN(EpiR{act}, EpiR{resm});                                                           \
    else if ((act) == PPST_ACT_LRELU) CONV_EPI_GO_(FN, PPST_ACT_LRELU, resm);                         \
    else if ((act) == PPST_ACT_PRELU) CONV_EPI_GO_(FN, PPST_ACT_PRELU, resm);                         \
    else CONV_EPI_GO_(FN, PPST_ACT_NONE, resm);                                                       \
  } while (0)

// ---- bias and noise of an epilogue.  Fetched for the whole wave tile BEFORE the first store: vmcnt counts stores too and retires in
// order, so a load issued behind a pass's stores made its s_waitcnt sit out their acknowledgements (one HBM round trip per pass).
// Buffer loads, every request unconditional -- a pixel outside the tile / image, channels beyond cout and a launch without bias /
// noise read out of range and get zeros: as conditional global loads hipcc issued them one by one, each with its own wait (found in
// the nine-product upscale, where 32 of them cost 0.3 ms of a 2.6-ms launch).  `any`: a valid address for the empty descriptor.
#define CONV_OOB ((int)0x80000000)      // offset of a request that must read zero: out of range of every image (< 2^31 bytes)
__device__ __forceinline__ float4 conv_epi_bias4(const float* bias, const void* any, int cout, int n0) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
      __builtin_amdgcn_make_buffer_rsrc((void*)(bias ? (const void*)bias : any), 0, bias ? cout * 4 : 0, 0x00020000), n0 * 4, 0, 0));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_epi_noise_rsrc(const float* noise_img, const void* any, int npix) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(noise_img ? (const void*)noise_img : any), 0, noise_img ? npix * 4 : 0, 0x00020000);
}
__device__ __forceinline__ float conv_epi_noise(__amdgpu_buffer_rsrc_t nrs, bool ok, int pix) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(nrs, ok ? pix * 4 : CONV_OOB, 0, 0));
}

// ---- argument block of conv_mfma_kernel and conv_mfma2_kernel
struct ConvKArgs {
  const float* x;
  const unsigned short* wpack;
  const int4* steps;
  float* y;
  const float* bias;
  const float* noise;
  const float* prelu;
  float* stats;
  const float* residual;
  float noise_weight, out_scale;
  int B, in_h, in_w, in_ld, out_h, out_w, out_ld, cout;
  int nsteps, n_groups, pad_mode, in_off_y, in_off_x, out_sy, out_sx, act, res_ld, tile_h, tile_w;
  int tiles_y, tiles_x, n_tiles;
  const float* in_ss;     // optional [B][in_c][2] (scale, shift) applied to the input while staging
  const float* in_prelu;  // slope for in_act == PRELU
  int in_c, in_act;
  int early_a;              // step table guarantees chunks of >= 2 steps: a chunk's global loads go out one step early
  unsigned long long* dbg;  // -DPPST_CONV_TRACE builds: the debug buffer (else unused)
  KSplitDev ks;             // ks.S > 1: grid row y runs steps [ks.start[y], ks.start[y + 1]) of every group (common.h)
  int prefetch_w;           // conv_mfma_kernel, small grid (<= 512 blocks): a block requests its weight blobs up front
};
// (the storage type of x / residual / y -- ppst_conv_args.io_st, single-pass precision modes only -- is a template parameter IOS of
// the kernels, not a field: the pointers above are then half / bfloat16 tensors behind their `float*` type)
static inline ConvKArgs conv_kargs_fill(const ppst_conv_args* a, int n_tiles, int tiles_y, int tiles_x) {
  ConvKArgs k;
  k.x = (const float*)a->x; k.wpack = (const unsigned short*)a->wpack; k.steps = (const int4*)a->steps; k.y = (float*)a->y;
  k.bias = (const float*)a->bias; k.noise = (const float*)a->noise; k.prelu = (const float*)a->prelu;
  k.stats = (float*)a->stats; k.residual = (const float*)a->residual;
  k.noise_weight = a->noise_weight; k.out_scale = a->out_scale;
  k.B = a->B; k.in_h = a->in_h; k.in_w = a->in_w; k.in_ld = a->in_ld; k.out_h = a->out_h; k.out_w = a->out_w;
  k.out_ld = a->out_ld; k.cout = a->cout; k.nsteps = a->nsteps; k.n_groups = a->n_groups; k.pad_mode = a->pad_mode;
  k.in_off_y = a->in_off_y; k.in_off_x = a->in_off_x; k.out_sy = a->out_sy; k.out_sx = a->out_sx; k.act = a->act;
  k.res_ld = a->res_ld; k.tile_h = a->tile_h; k.tile_w = a->tile_w;
  k.tiles_y = tiles_y; k.tiles_x = tiles_x; k.n_tiles = n_tiles;
  k.in_ss = (const float*)a->in_scale_shift; k.in_prelu = (const float*)a->in_prelu;
  k.in_c = a->in_c; k.in_act = a->in_act;
  k.early_a = a->early_a ? 1 : 0;
  k.dbg = nullptr;
  k.ks.scratch = nullptr; k.ks.flags = nullptr; k.ks.epoch = 0; k.ks.S = 1;
  k.prefetch_w = 0;
#ifdef PPST_CONV_TRACE
  k.dbg = (unsigned long long*)a->prelu;  // diagnostic builds: the (unused) prelu slot carries the debug buffer
  k.prelu = nullptr;
#endif
  return k;
}

// ---- transposition epilogue of conv_mfma_kernel (conv_mfma2_kernel keeps a copy of its own for its register budget: see there;
// any change here goes there too -- tests/test_gpu_conv_epilogue.py holds the two to the bit): + bias + noise [+ residual]
// -> act -> * out_scale -> store, tile statistics.  A wave holds MT m-tiles (16-pixel tile rows) x 2 NP n-tiles (16 channels) of
// accumulators, lane = channel, registers = pixels; they are transposed through the wave's LDS tile `tw` (64 px x (32 ch + 4 pad)
// floats) so that every lane stores 16 contiguous bytes of one pixel (128-B segments per pixel per wave-instruction instead of 64-B
// ones, 4x fewer store instructions, and the pixel address arithmetic runs once per float4): per group of four m-tiles, NP passes
// of 32 channels.
//   tyb, tx0: the wave's first tile row and the tile's first column;  nch0: the wave's first output channel;  egy, egx: output
//   phase of the transposed conv (0 for one group);  s1a, s2a: the lane's sums per pass, for conv_epi_transpose_sums (whose `redw`
//   is the wave's [32 NP][2] row of the block's partial sums; the caller adds the rows of its M-waves behind a barrier).
// Output addressing: 32-bit element offsets inside image b (the entry point rejects images of >= 2^31 elements); the tile row and the
// column half of a store are wave-uniform, so their strides are scalar.  (With the pixel offset as a 64-bit product per store the
// epilogue was bound by v_mul_lo_u32 / v_mad_u64_u32: ~45 vector instructions per store, a third of them quarter-rate.)
template <int MT, int NP, int IOS, bool SPEC>
__device__ __forceinline__ void conv_epi_transpose(const ConvKArgs& a, const f32x4 (&acc)[MT][2 * NP], int b, int tyb, int tx0, int nch0,
                                                   int egy, int egx, float* tw, float4 (&s1a)[NP], float4 (&s2a)[NP], int lane) {
  constexpr int ES = IOS == PPST_ST_F32 ? 4 : 2;         // bytes per stored element
  const int r16 = lane & 15, g = lane >> 4, f8 = lane & 7, prow = lane >> 3;
  const int act = a.act & 0xff;
  const int resm = a.residual ? (((a.act >> 8) & 1) ? 2 : 1) : 0;   // (bit 8: the residual joins after the activation -- resnet skip)
  const float slope = (act == PPST_ACT_PRELU && a.prelu) ? a.prelu[0] : 0.f;
  const int oyb = tyb * a.out_sy + egy;                                   // first output row of this wave (uniform)
  const int txl = tx0 + prow, oxl = txl * a.out_sx + egx;                 // this lane's column for even `it` (odd: 8 further)
  const bool okx0 = txl < a.tile_w && oxl < a.out_w, okx1 = txl + 8 < a.tile_w && oxl + 8 * a.out_sx < a.out_w;
  const int pix0 = oyb * a.out_w + oxl, rs_pix = a.out_sy * a.out_w;
  const int64_t img = (int64_t)b * a.out_h * a.out_w;
  unsigned char* const yb = (unsigned char*)a.y + img * a.out_ld * ES;
  const unsigned char* const rb = a.residual ? (const unsigned char*)a.residual + img * a.res_ld * ES : nullptr;
  float nzv[2 * MT];
  float4 bva[NP];
  const __amdgpu_buffer_rsrc_t nrs = conv_epi_noise_rsrc(a.noise ? a.noise + img : nullptr, yb, a.out_h * a.out_w);
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i) {
    const int r = i >> 1, c8 = i & 1;
    // (oy / ox bounds: odd scattered extents -- the input gradient of a stride-2 conv)
    const bool ok = tyb + r < a.tile_h && oyb + r * a.out_sy < a.out_h && (c8 ? okx1 : okx0);
    nzv[i] = a.noise_weight * conv_epi_noise(nrs, ok, pix0 + r * rs_pix + c8 * 8 * a.out_sx);
  }
#pragma unroll
  for (int pass = 0; pass < NP; ++pass) bva[pass] = conv_epi_bias4(a.bias, a.y, a.cout, nch0 + pass * 32 + f8 * 4);
#pragma unroll
  for (int i = 0; i < NP; ++i) { s1a[i] = make_float4(0.f, 0.f, 0.f, 0.f); s2a[i] = s1a[i]; }
  auto epi_passes = [&](auto act_c, auto res_c) {
#pragma unroll
    for (int mh = 0; mh < (MT + 3) / 4; ++mh) {
      const int MG = MT - mh * 4 < 4 ? MT - mh * 4 : 4;     // m-tiles of this group (MT = 6: 4 + 2)
#pragma unroll
      for (int pass = 0; pass < NP; ++pass) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int ntl = 0; ntl < 2; ++ntl)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (mt < MG) tw[(mt * 16 + g * 4 + j) * 36 + ntl * 16 + r16] = acc[mh * 4 + mt < MT ? mh * 4 + mt : 0][pass * 2 + ntl][j];
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): only this wave touches its tile
        __builtin_amdgcn_wave_barrier();
        const int n0 = nch0 + pass * 32 + f8 * 4;
        const bool nok = n0 < a.cout;
        const float4 bv = bva[pass];
        const int yo0 = pix0 * a.out_ld + n0, ro0 = pix0 * a.res_ld + n0;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          if (it >= 2 * MG) continue;
          const int p = it * 8 + prow;
          const int r = mh * 4 + (it >> 1), c8 = it & 1;   // tile row of the wave and column half of this store
          float4 v = *(const float4*)(tw + p * 36 + f8 * 4);
          const bool rowok = tyb + r < a.tile_h && oyb + r * a.out_sy < a.out_h;
          if (nok && rowok && (c8 ? okx1 : okx0)) {
            const int d = r * rs_pix + c8 * 8 * a.out_sx;  // uniform pixel step from (row 0, even column half)
            float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (res_c.value) rv = st_ld4<IOS>(rb, ro0 + d * a.res_ld);
            float o[4];
            conv_epi_value4(o, v, bv, nzv[mh * 8 + it], rv, slope, a.out_scale, act_c, res_c);
            if (IOS == PPST_ST_F32) PPST_EPI_STORE((float*)yb + (yo0 + d * a.out_ld), o);
            else st_st4<IOS>(yb, yo0 + d * a.out_ld, make_float4(o[0], o[1], o[2], o[3]));
            conv_epi_accum(s1a[pass], s2a[pass], o);
          }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();  // tile reads done before the next pass overwrites it
      }
    }
  };
  CONV_EPI_DISPATCH(SPEC, epi_passes, act, resm);
}
// ... and the wave-level reduction of its sums (a lane: 4 channels of 8 of the wave's 64 pixel columns) into the wave's row of `red`
template <int NP>
__device__ __forceinline__ void conv_epi_transpose_sums(float4 (&s1a)[NP], float4 (&s2a)[NP], float* redw, int lane) {
#pragma unroll
  for (int pass = 0; pass < NP; ++pass) {
    conv_epi_xor_sum<8>(s1a[pass], s2a[pass]);           // over the 8 pixel rows of the wave (lanes with equal lane & 7)
    if ((lane >> 3) == 0) conv_epi_put_sums(redw + (pass * 32 + (lane & 7) * 4) * 2, s1a[pass], s2a[pass]);
  }
}
