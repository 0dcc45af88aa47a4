// Backward / optimiser kernels of the GAN train step (reference:
// optimizers/ppst_optimizer.py:96-130 discriminator update, torch autograd of F.conv2d /
// F.linear inside models/networks/stylegan2_layers.py).
//
//  * conv weight gradient: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) with the reduction over
//    pixels.  NHWC makes both operands lane-contiguous for that instruction (A = dY[p][n0+i],
//    B = X[p+tap][c0+j], k = 2 consecutive pixels), so fragments come straight from L1/L2
//    with 128-B coalesced loads: no LDS, no transposition.  It shares the forward's step
//    table, so plain, 1x1 and space-to-depth (stride-2) convs are one code path.
//  * conv input gradient: not here -- it is the forward kernel (ppst_conv2d_mfma) run on a
//    transposed / flipped pack of the same weights.
//  * small glue: scatter of the per-step gradients into the (Cout,Cin,k,k) parameter layout,
//    FromRGB weight gradient, column sums (bias gradients), linear layer gradients, LSGAN
//    loss/gradient, Adam.
#include "conv_common.h"   // the XCD block map

// ------------------------------------------------------------ conv wgrad ----
// partial[split][step][n][32] = sum over this split's pixels of dY[p][n] * X[p + tap(step)][chan(step) + k]
// grid = (cout/128 n-tiles, chunks, splits); block = 4 waves, wave w owns n = n0 + 32w .. +31;
// one block handles ONE chunk = up to 9 consecutive steps that share chan_off (registers: 9 x 16).
// Four kernels take this sum -- conv_wgrad_kernel (fp32, operands from L1 / L2), conv_wgrad_lds_kernel (fp32, LDS-staged),
// conv_wgrad_tr2_kernel (bf16 hi / lo split of fp32 tiles: production) and conv_wgrad_tr2b_kernel (bf16-stored operands) -- and
// differ in how a tile reaches the matrix pipe.  What surrounds that is stated once, here:
//   WgChunk, wg_chunk_load, wg_chan_of    a chunk of the step table: first step, length, channel offset, the taps' (dy, dx)
//   wg_zero                               the accumulators
//   wg_range, wg_tile                     the pixel split's range of tiles (conv_wgrad_kernel: of rows); a tile's image and origin
//   wg_block_xcd                          the XCD-aware block map to (x = n tile, y = chunk group, z = pixel split)
//   wg_units, wg_csum_finish              the (pixel, channel quad) units of the live 32-channel slabs of dY dealt to the threads,
//                                         and the block's column sums of dY (the bias gradient) from the threads' sums over them
//   WG_STORE_TILE                         one accumulator (the MFMA's 32 x 32 D tile) into partial
// The tap loops stay apart: conv_wgrad_tr2_kernel's and conv_wgrad_tr2b_kernel's differ in the fragment reader and the pass count, the
// two fp32 kernels' pixel loops in where an operand comes from.
#define WG_MAXT 9
#define WG_TR 2                     // the tile of the three staged kernels: 2 x 32 pixels of dY
#define WG_TC 32
template <int TM> struct WgChunk { int s0, T, chan; int tdy[TM], tdx[TM]; };
// (taps beyond the chunk's length T repeat tap 0: their offsets are loaded, never used.  I: the caller's index type -- blockIdx.y is
// unsigned, and widening it as an int gives other address arithmetic)
template <int TM, typename I>
__device__ __forceinline__ void wg_chunk_load(WgChunk<TM>& c, const int4* steps, const int* chunk_start, I chunk) {
  c.s0 = chunk_start[chunk];
  c.T = chunk_start[chunk + 1] - c.s0;
  c.chan = steps[c.s0].x;
#pragma unroll
  for (int t = 0; t < TM; ++t) {
    int4 d = steps[c.s0 + (t < c.T ? t : 0)];
    c.tdy[t] = d.y; c.tdx[t] = d.z;
  }
}
// channel offset of chunk ci, a wave-uniform RUNTIME index, written as selects.  ``chan`` is a copy of the chunks' offsets in an
// array of its own: at NCH = 4 hipcc turns the selects back into an indexed read and keeps that array in memory (16 bytes per thread,
// which it places in LDS) -- indexed inside the chunks, all of them would go to scratch
template <int NCH>
__device__ __forceinline__ int wg_chan_of(const int (&chan)[NCH], int ci) {
  int c = chan[0];
#pragma unroll
  for (int j = 1; j < NCH; ++j) c = ci == j ? chan[j] : c;
  return c;
}
template <int N>
__device__ __forceinline__ void wg_zero(f32x16 (&acc)[N]) {
#pragma unroll
  for (int t = 0; t < N; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
}
template <int M, int N>
__device__ __forceinline__ void wg_zero(f32x16 (&acc)[M][N]) {
#pragma unroll
  for (int ci = 0; ci < M; ++ci) wg_zero(acc[ci]);
}
struct WgRange { int begin, end; };
__device__ __forceinline__ WgRange wg_range(int split, int per_split, int total) {
  const int begin = split * per_split;
  return {begin, min(begin + per_split, total)};
}
struct WgTile { int b, ty0, tx0; };
__device__ __forceinline__ WgTile wg_tile(int tile, int tiles_per_image, int tiles_x) {
  const int b = tile / tiles_per_image;
  const int r = tile - b * tiles_per_image;
  return {b, (r / tiles_x) * WG_TR, (r - (r / tiles_x) * tiles_x) * WG_TC};
}
struct WgBlock { int x, y, z; };
__device__ __forceinline__ WgBlock wg_block_xcd() {      // (conv_common.h; why: the comment in front of conv_wgrad_tr2_kernel)
  const int nb = gridDim.x * gridDim.y * gridDim.z;
  const int id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  int v = xcd_block_id(id, nb);
  WgBlock k;
  k.x = v % (int)gridDim.x; v /= (int)gridDim.x;
  k.y = v % (int)gridDim.y; k.z = v / (int)gridDim.y;
  return k;
}
// The 64 pixels x NQ = 8 nslab channel quads of a dY tile's live slabs, dealt to the block's 256 threads: thread tid < stride takes
// the units i = tid, tid + stride, .. < 64 NQ; unit i is (pixel i / NQ, quad i % NQ).  stride is 256 rounded down to a multiple of
// NQ (8, 16, 32: 256; 24: 240), so a thread keeps ONE quad, tid % NQ, in every pass -- its column sums need no index.
struct WgUnits { int NQ, stride; };
__device__ __forceinline__ WgUnits wg_units(int nslab) {
  const int NQ = 8 * nslab;
  return {NQ, (256 / NQ) * NQ};
}
// csum[split][n0 ..] = the block's column sums of dY: cs = this thread's sums of its quad; the threads with equal tid % NQ share a
// quad and are added in thread order.  red: 4 KB of LDS that no wave reads any more (barrier inside)
__device__ __forceinline__ void wg_csum_finish(float4 cs, float4* red, int nslab, int tid, float* csum, int split, int n0, int cout) {
  const WgUnits u = wg_units(nslab);
  __syncthreads();
  red[tid] = tid < u.stride ? cs : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  if (tid < u.NQ) {
    float4 a = red[tid];
    for (int r = tid + u.NQ; r < u.stride; r += u.NQ) { const float4 v = red[r]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    const int n = n0 + tid * 4;
    float* o = csum + (int64_t)split * cout + n;
    if (n < cout) { o[0] = a.x; if (n + 1 < cout) o[1] = a.y; if (n + 2 < cout) o[2] = a.z; if (n + 3 < cout) o[3] = a.w; }
  }
}
// D tile of a wave whose first output channel is nw0: col = lane & 31 (k within the 32-channel chunk),
// row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (n).  Reads the kernel's partial, nsteps, cout and lane.  (Expanded as text:
// the same lines as a __forceinline__ function gave every kernel another instruction stream, and conv_wgrad_lds_kernel 40 more
// bytes of scratch -- profiles/wgrad_shared_isa.txt.)
#define WG_STORE_TILE(acc, split, step, nw0)                                                  \
  do {                                                                                          \
    float* o = partial + (((int64_t)(split) * nsteps + step) * cout) * 32;                      \
    _Pragma("unroll") for (int rg = 0; rg < 16; ++rg) {                                         \
      int nn = nw0 + (rg & 3) + 8 * (rg >> 2) + 4 * (lane >> 5);                                \
      if (nn < cout) o[(int64_t)nn * 32 + (lane & 31)] = (acc)[rg];                             \
    }                                                                                           \
  } while (0)

__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const int4* __restrict__ steps, const int* __restrict__ chunk_start,
                                                         float* __restrict__ partial, int B, int in_h, int in_w, int in_ld,
                                                         int oh, int ow, int dy_ld, int cout, int nsteps, int rows_per_split) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const int n = blockIdx.x * 128 + wave * 32 + li;
  WgChunk<WG_MAXT> ck;
  wg_chunk_load(ck, steps, chunk_start, blockIdx.y);
  const int T = ck.T;
  if (blockIdx.x * 128 + wave * 32 >= cout) return;   // waves beyond the last output channel (no barrier in this kernel)
  f32x16 acc[WG_MAXT];
  wg_zero(acc);
  const WgRange rows = wg_range(blockIdx.z, rows_per_split, B * oh);
  const bool nok = n < cout;
  const int nc = nok ? n : 0;
  for (int r = rows.begin; r < rows.end; ++r) {
    const int b = r / oh, y = r - b * oh;
    const float* dyr = dy + ((int64_t)(b * oh + y) * ow) * dy_ld + nc;
    const float* xb = x + (int64_t)b * in_h * in_w * in_ld + ck.chan + li;
    // per-row tap state: row pointer (clamped) and validity, so the pixel loop issues unconditional loads
    // (select afterwards): the compiler can then hoist the loads of the next pixel pair above this pair's MFMAs
    const float* rowp[WG_MAXT];
    bool rowok[WG_MAXT];
#pragma unroll
    for (int t = 0; t < WG_MAXT; ++t) {
      const int iy = y + ck.tdy[t];
      rowok[t] = t < T && iy >= 0 && iy < in_h;
      rowp[t] = xb + (int64_t)(rowok[t] ? iy : 0) * in_w * in_ld;
    }
#pragma unroll 2
    for (int x0 = 0; x0 < ow; x0 += 2) {
      const int xx = x0 + lk;
      const bool xok = xx < ow;
      float av = dyr[(int64_t)(xok ? xx : 0) * dy_ld];
      av = (nok && xok) ? av : 0.f;
      float bv[WG_MAXT];
#pragma unroll
      for (int t = 0; t < WG_MAXT; ++t) {
        const int ix = xx + ck.tdx[t];
        const bool ok = rowok[t] && xok && ix >= 0 && ix < in_w;
        const float v = rowp[t][(int64_t)(ok ? ix : 0) * in_ld];
        bv[t] = ok ? v : 0.f;
      }
#pragma unroll
      for (int t = 0; t < WG_MAXT; ++t)
        if (t < T) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[t], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < WG_MAXT; ++t)
    if (t < T) WG_STORE_TILE(acc[t], blockIdx.z, ck.s0 + t, blockIdx.x * 128 + wave * 32);
}

// LDS-staged variant (round 2): the block stages a 2 x 32-pixel tile of dY (64 px x 128 n, 32 KB) and the matching
// (2+2) x (32+2)-pixel halo tile of the 32-channel input chunk (17 KB) with 16-B loads, then every k-pair costs one
// conflict-free ds_read_b32 per operand instead of an L1/L2 round trip per lane.  Same arithmetic (exact fp32 MFMA), same
// step tables; the round-1 kernel above was latency bound (26 TFLOP/s = 17 % of the fp32 MFMA peak: two waves per SIMD
// each waiting ~500 cycles per operand fetch).  49 KB of LDS, 3 blocks per CU: one block's staging overlaps the
// others' MFMAs.
__global__ __launch_bounds__(256, 3) void conv_wgrad_lds_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const int4* __restrict__ steps, const int* __restrict__ chunk_start,
                                                              float* __restrict__ partial, int B, int in_h, int in_w, int in_ld,
                                                              int oh, int ow, int dy_ld, int cout, int nsteps, int tiles_x,
                                                              int tiles_per_image, int tiles_total, int tiles_per_split) {
  constexpr int XH = WG_TR + 2, XW = WG_TC + 2;
  __shared__ __attribute__((aligned(16))) float sdy[WG_TR * WG_TC][128];
  __shared__ __attribute__((aligned(16))) float sx[XH * XW][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const int n0 = blockIdx.x * 128;
  WgChunk<WG_MAXT> ck;
  wg_chunk_load(ck, steps, chunk_start, blockIdx.y);
  const int T = ck.T, chan = ck.chan;
  f32x16 acc[WG_MAXT];
  wg_zero(acc);
  const WgRange tiles = wg_range(blockIdx.z, tiles_per_split, tiles_total);
  const bool wave_live = n0 + wave * 32 < cout;          // waves beyond the last output channel only help staging
  for (int tile = tiles.begin; tile < tiles.end; ++tile) {
    const auto [b, ty0, tx0] = wg_tile(tile, tiles_per_image, tiles_x);
    __syncthreads();                                       // previous tile's reads are done
    // dY tile: 64 px x 128 n (zeros outside the image / beyond cout)
    for (int i = tid; i < WG_TR * WG_TC * 32; i += 256) {
      const int q = i & 31, p = i >> 5;                    // float4 index within the pixel, pixel
      const int y = ty0 + p / WG_TC, xx = tx0 + p % WG_TC;
      const int n = n0 + q * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y < oh && xx < ow && n < cout) {                 // cout % 4 == 0 (host check)
        v = *(const float4*)(dy + (((int64_t)b * oh + y) * ow + xx) * dy_ld + n);
      }
      *(float4*)&sdy[p][q * 4] = v;
    }
    // input halo tile: (TR + 2) x (TC + 2) px x 32 channels, zero outside the image
    for (int i = tid; i < XH * XW * 8; i += 256) {
      const int q = i & 7, p = i >> 3;
      const int iy = ty0 - 1 + p / XW, ix = tx0 - 1 + p % XW;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (iy >= 0 && iy < in_h && ix >= 0 && ix < in_w)
        v = *(const float4*)(x + (((int64_t)b * in_h + iy) * in_w + ix) * in_ld + chan + q * 4);
      *(float4*)&sx[p][q * 4] = v;
    }
    __syncthreads();
    if (wave_live) {
#pragma unroll 4
      for (int kp = 0; kp < WG_TR * WG_TC; kp += 2) {
        const int p = kp + lk;
        const int py = p / WG_TC, px = p % WG_TC;
        const float av = sdy[p][wave * 32 + li];
        float bv[WG_MAXT];
#pragma unroll
        for (int t = 0; t < WG_MAXT; ++t) bv[t] = sx[(py + 1 + ck.tdy[t]) * XW + px + 1 + ck.tdx[t]][li];
#pragma unroll
        for (int t = 0; t < WG_MAXT; ++t)
          if (t < T) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[t], acc[t], 0, 0, 0);
      }
    }
  }
  if (!wave_live) return;
#pragma unroll
  for (int t = 0; t < WG_MAXT; ++t)
    if (t < T) WG_STORE_TILE(acc[t], blockIdx.z, ck.s0 + t, n0 + wave * 32);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The production weight gradient (every precision but 2, 16-byte aligned operands): the same partial layout, step tables and
// 2 x 32-pixel tiles as conv_wgrad_lds_kernel, on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16) with the fp32 operands split
// into bf16 hi / lo halves: three passes (lo x hi, hi x lo, hi x hi -- 5.3x the fp32 MFMA's rate after the three passes; every
// product carries the 2^-17 relative error of the split, the sums are the MFMA's fp32 accumulation as before: the discriminator /
// generator gradient bars of tests/ are 5e-3), or ONE pass over the hi halves (X1, below).
//   * Feed: LDS-DMA.  The raw fp32 tile (dY 64 px x 128 n = 32 KB, input halo 4 x 34 px x 32 ch = 17 KB) goes global -> LDS by
//     global_load_lds_dwordx4: no registers, one 1-KB piece (64 lanes x 16 B) per wave instruction.  A lane whose pixel lies outside
//     the image or whose channels lie beyond cout reads the 16-byte ZERO WORD g_wg_zero instead of its own address: the image needs
//     no zero fill and the request no branch.  hipcc adds no wait for LDS-DMA: s_waitcnt vmcnt(0) in front of the barrier.
//   * Conversion IN PLACE, one pass of all threads per tile: a 16-byte unit (one pixel, four channels) becomes [hi x 4 | lo x 4]
//     bf16 in the same 16 bytes -- no second image -- and, in the blocks of chunk 0, the fp32 column sums of dY are taken on the way
//     (the bias gradient: the 304 colsum launches per train step re-read every dY the weight gradient had just read).  Units of
//     pixels p and p + 2 alias the same banks, so every other pixel PAIR stores [lo | hi] instead: the 32 eight-byte reads of a
//     half-wave (4 pixels x 8 channel quads) then hit 64 distinct banks.
//   * MFMA operands by transposed reads (ds_read_b64_tr_b16).  The K index of this GEMM is the PIXEL, so an operand lane needs 8
//     consecutive pixels of ONE channel while the image is [pixel][channel].  The instruction takes a per-lane address (any unit
//     layout works) and transposes within groups of 16 lanes: group g = lane / 16 reads 4 pixel rows x 16 channels; lane 4q + p of
//     the group supplies the address of pixel row q, channels 4p .. 4p+3; lane i of the group receives channel i of the 4 rows, i.e.
//     4 k-values.  Groups 0 / 1: channels 0-15 / 16-31 of k-half 0, groups 2 / 3 the same of k-half 1 -- channel lane & 31, k-half
//     lane >> 5, as the 32x32x16 operand wants; a second read 4 pixels on completes the 8 k-values.  No pixel-pair packing, and ONE
//     input image serves all nine taps (a tap is an address offset).
//   * XCD-aware block map.  Blocks go to the 8 XCDs round-robin by linear id, and the blocks that share a tile of dY (all chunks y
//     of one pixel range z) or of the input (all n tiles x) had consecutive ids: every XCD's L2 fetched those tiles from HBM itself
//     (the three 3x3 layers of the generator each moved 1.34 GB per launch instead of 0.54).  The bijective 8-way remap gives each
//     XCD a contiguous range of the (z, y, x) order -- x fastest -- so co-resident blocks of one XCD walk the same tiles.
//   * Two blocks per CU.  Per tile: request (49 pieces) -> wait -> convert (+ the bias column sums) -> MFMA; nothing inside the
//     block overlaps, the co-resident block -- in another phase -- does.  For that the tile has to fit 80 KB: dY image 4 slabs
//     (32 channels) x 64 pixels x 128 B = 32 KB, input halo image 136 pixels x 128 B = 17 KB: 49 KB per block, 256 threads, 4 waves
//     = 4 n slabs, each wave reduces over the tile's four 16-pixel groups.
// History (a4b3174 is the last commit with their code): conv_wgrad_x3_kernel (round 2) staged through registers, converting and
// packing pixel pairs on the way to LDS; its staging loops serialised ~9 global round trips per tile, 10-12 k cycles against 3.5 k
// of MFMA work: 0.16 of the bf16x3 ceiling over the step.  conv_wgrad_tr_kernel (round 3) brought the feed, the transposed reads
// and the block map described here, as ONE 8-wave block per CU with 147 KB of LDS (DMA two tiles ahead, a second, converted image);
// its phases ADDED UP inside the one block (128->128 @512^2, ms: DMA 0.29 + conversion 0.19 + MFMA 0.39 of 0.68-0.75; handing the
// DMA pieces out between the taps was 30 % slower still), and the fix was not a deeper pipeline but the second block on the CU.
// NCH chunks (32 input channels each) per block, at most TM taps per chunk: <1, 9> for 3x3 tables; <2, 4> for tables whose chunks
// have <= 4 steps (transposed conv, stride-2 tables, 1x1): two input images share ONE dY image, i.e. a third fewer bytes per MFMA
// where a 4-tap chunk would otherwise do 4/9 of the MFMA work of a 3x3 chunk per staged tile (blockIdx.y = pair of chunks).
// X1: single-pass bf16 (precision mode 1, BASELINE configs[3]'s "bf16 compute, fp32 master weights"): only the hi halves are
// written and multiplied -- a third of the MFMA phase; the bias column sums still come from the fp32 values.
// EXACT: every chunk of the table has exactly TM steps (3x3 convs: 9; the transposed conv's phases: 4) -- the tap loop then has
// no `t < T` tests.  With the runtime count each tap was its own basic block behind a branch (hipcc's wait-count pass drains the
// LDS queue at every block entry, and the next tap's fragments could not be requested across it).
// HALO = false (1x1 tables: one step per chunk, no offsets): the input image is the tile's own 2 x 32 pixels (8 KB per chunk
// instead of the 17-KB halo image), so FOUR chunks share a block and one dY image at 64 KB of LDS.
#define WT_PX (WG_TR * WG_TC)                 // 64 pixels of dY per tile
#define WT_XW (WG_TC + 2)
#define WT_XPX ((WG_TR + 2) * WT_XW)          // 136 halo pixels of the input chunk
__device__ __attribute__((aligned(16))) float g_wg_zero[4] = {0.f, 0.f, 0.f, 0.f};
typedef short __attribute__((ext_vector_type(4))) wt_v4s;
template <int NCH, int TM, bool X1, bool EXACT, bool HALO = true>
__global__ __launch_bounds__(256, 2) void conv_wgrad_tr2_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const int4* __restrict__ steps, const int* __restrict__ chunk_start,
                                                              float* __restrict__ partial, float* __restrict__ csum, int B, int in_h,
                                                              int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps,
                                                              int tiles_x, int tiles_per_image, int tiles_total, int tiles_per_split) {
  constexpr int XW = HALO ? WT_XW : WG_TC, XPX = HALO ? WT_XPX : WT_PX, XO = HALO ? 1 : 0;      // input image: width, pixels, origin offset
  constexpr int XPC = XPX / 8;                                // DMA pieces (8 pixels x 128 B) per chunk: 17 / 8
  constexpr int IMG_DY = WT_PX * 128 * 4, IMG_X = XPX * 32 * 4;              // 32768 + 17408 (8192) bytes
  static_assert(!HALO ? TM == 1 : true, "the no-halo image serves 1x1 tables");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[IMG_DY + NCH * IMG_X];
  unsigned char* const imdy = smem;                           // [slab 0..3][64 px][8 quads][16 B]
  unsigned char* const imx = smem + IMG_DY;                   // NCH x [136 px][8 quads][16 B]
  const int tid = threadIdx.x, lane = tid & 63, nw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WgBlock blk = wg_block_xcd();
  const int n0 = blk.x * 128;
  WgChunk<TM> ck[NCH];
  int chan[NCH];                                              // (for wg_chan_of)
#pragma unroll
  for (int ci = 0; ci < NCH; ++ci) {
    wg_chunk_load(ck[ci], steps, chunk_start, blk.y * NCH + ci);
    chan[ci] = ck[ci].chan;
  }
  f32x16 acc[NCH][TM];
  wg_zero(acc);
  const WgRange tiles = wg_range(blk.z, tiles_per_split, tiles_total);
  const bool wave_live = n0 + nw * 32 < cout;
  const int nslab = min(4, (cout - n0 + 31) >> 5);            // 32-channel slabs of dY this block has any use for
  const bool want_csum = csum != nullptr && blk.y == 0;
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);               // this thread's 4 channels (quad tid % (8 nslab)) over its pixels of every tile
  // transposed-read lane geometry (the comment above): channel quad 4 (g & 1) + pp, pixel 8 kb + qd (+ 4 for the second read)
  const int g = lane >> 4, qd = (lane & 15) >> 2, pp = lane & 3;
  const int tr_unit = (8 * (g >> 1) + qd) * 128 + (4 * (g & 1) + pp) * 16;
  auto split4 = [](float4 v, uint2& hi, uint2& lo) { split_bf16x4(v, hi, lo); };
  // operand of 8 k-values (pixels) from the unit image: ``u`` = address of this lane's unit of the first pixel group, ``sw`` = 1
  // when that pixel pair stores [lo | hi]
  auto frag = [&](const unsigned char* u, int sw, bf16x8& h, bf16x8& l) {
    const unsigned char* ph = u + sw * 8;
    const unsigned char* pl = u + (sw ^ 1) * 8;
    const wt_v4s h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wt_v4s __attribute__((address_space(3)))*)ph);
    const wt_v4s h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wt_v4s __attribute__((address_space(3)))*)(ph + 4 * 128));
    h = (bf16x8){h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    if (!X1) {
      const wt_v4s l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wt_v4s __attribute__((address_space(3)))*)pl);
      const wt_v4s l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wt_v4s __attribute__((address_space(3)))*)(pl + 4 * 128));
      l = (bf16x8){l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
    } else {
      l = h;
    }
  };
  for (int tile = tiles.begin; tile < tiles.end; ++tile) {
    const auto [b, ty0, tx0] = wg_tile(tile, tiles_per_image, tiles_x);
    __syncthreads();                                        // the previous tile's MFMA reads are done
    // ---- LDS-DMA: 32 pieces of dY (slab s, pixels 8 j .. 8 j + 7: 8 x 128 B) + 17 per chunk of the input halo (8 pixels x 128 B)
    for (int wi = nw; wi < 32 + NCH * XPC; wi += 4) {
      const float* src = g_wg_zero;
      unsigned char* dst;
      const int q = lane & 7;
      if (wi < 32 && (wi >> 3) >= nslab) continue;          // slab beyond cout: no wave reads it (thin layers: 8 of 32 pieces)
      if (wi < 32) {
        const int p = 8 * (wi & 7) + (lane >> 3), n = n0 + (wi >> 3) * 32 + q * 4;
        const int y = ty0 + (p >> 5), xx = tx0 + (p & 31);
        if (y < oh && xx < ow && n < cout) src = dy + (((int64_t)b * oh + y) * ow + xx) * dy_ld + n;
        dst = imdy + wi * 1024;
      } else {
        const int ci = (wi - 32) / XPC, pj = (wi - 32) - ci * XPC;        // wave-uniform
        const int P = 8 * pj + (lane >> 3);
        const int row = P / XW, col = P - row * XW;
        const int iy = ty0 - XO + row, ix = tx0 - XO + col;
        if (iy >= 0 && iy < in_h && ix >= 0 && ix < in_w)
          src = x + (((int64_t)b * in_h + iy) * in_w + ix) * in_ld + wg_chan_of(chan, ci) + q * 4;
        dst = imx + (wi - 32) * 1024;
      }
      __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (hipcc adds no wait for LDS-DMA)
    __syncthreads();
    // ---- in-place conversion: unit (pixel p, quad) fp32 x 4 -> [hi | lo] bf16 x 4 (swapped for odd pixel pairs)
    if (nslab == 4) {
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int i = tid + it * 256;                         // pixel-major: channel quad (slab * 8 + quad) = tid & 31 for every it
        const int cq = i & 31, p = i >> 5;
        unsigned char* u = imdy + (cq >> 3) * 8192 + p * 128 + (cq & 7) * 16;
        const float4 v = *(const float4*)u;
        if (want_csum) { cs.x += v.x; cs.y += v.y; cs.z += v.z; cs.w += v.w; }
        uint2 hi, lo;
        split4(v, hi, lo);
        const int sw = (p >> 1) & 1;
        if (X1) *(uint2*)(u + sw * 8) = hi;
        else *(uint4*)u = sw ? make_uint4(lo.x, lo.y, hi.x, hi.y) : make_uint4(hi.x, hi.y, lo.x, lo.y);
      }
    } else {
      // fewer live slabs (cout - n0 <= 96): the unit walk of wg_units (the loop above is that walk at NQ = 32, unrolled)
      const WgUnits un = wg_units(nslab);
      if (tid < un.stride)
        for (int i = tid; i < 64 * un.NQ; i += un.stride) {
          const int p = i / un.NQ, cq = i - p * un.NQ;
          unsigned char* u = imdy + (cq >> 3) * 8192 + p * 128 + (cq & 7) * 16;
          const float4 v = *(const float4*)u;
          if (want_csum) { cs.x += v.x; cs.y += v.y; cs.z += v.z; cs.w += v.w; }
          uint2 hi, lo;
          split4(v, hi, lo);
          const int sw = (p >> 1) & 1;
          if (X1) *(uint2*)(u + sw * 8) = hi;
          else *(uint4*)u = sw ? make_uint4(lo.x, lo.y, hi.x, hi.y) : make_uint4(hi.x, hi.y, lo.x, lo.y);
        }
    }
#pragma unroll
    for (int ci = 0; ci < NCH; ++ci)
#pragma unroll
      for (int it = 0; it < (XPX * 8 + 255) / 256; ++it) {
        const int i = tid + it * 256;
        if (i < XPX * 8) {
          unsigned char* u = imx + ci * IMG_X + i * 16;
          const float4 v = *(const float4*)u;
          uint2 hi, lo;
          split4(v, hi, lo);
          const int sw = (i >> 4) & 1;                        // pixel = i >> 3
          if (X1) *(uint2*)(u + sw * 8) = hi;
          else *(uint4*)u = sw ? make_uint4(lo.x, lo.y, hi.x, hi.y) : make_uint4(hi.x, hi.y, lo.x, lo.y);
        }
      }
    __syncthreads();
    if (wave_live) {
#pragma unroll 1                                             // (unrolled, hipcc hoists 4 x 9 x 2 fragment addresses: 44 registers spilled)
      for (int ks = 0; ks < 4; ++ks) {                       // four groups of 16 pixels: tile row ks / 2, half ks % 2
        const int row = ks >> 1, xh = (ks & 1) * 16;
        bf16x8 a_h, a_l;
        frag(imdy + nw * 8192 + (row * 32 + xh) * 128 + tr_unit, (qd >> 1) & 1, a_h, a_l);
#pragma unroll
        for (int ci = 0; ci < NCH; ++ci) {
          const unsigned char* const im = imx + ci * IMG_X;
          const int pb0 = (row + XO + ck[ci].tdy[0]) * XW + xh + XO + ck[ci].tdx[0];
          bf16x8 b_h, b_l;
          frag(im + pb0 * 128 + tr_unit, (((pb0 & 3) + qd) >> 1) & 1, b_h, b_l);
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            if (EXACT || t < ck[ci].T) {
              bf16x8 n_h = b_h, n_l = b_l;
              if (t + 1 < TM && (EXACT || t + 1 < ck[ci].T)) {   // the next tap's fragments are requested before this tap's MFMAs
                const int pb = (row + XO + ck[ci].tdy[t + 1]) * XW + xh + XO + ck[ci].tdx[t + 1];
                frag(im + pb * 128 + tr_unit, (((pb & 3) + qd) >> 1) & 1, n_h, n_l);
              }
              if (!X1) {
                acc[ci][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_l, b_h, acc[ci][t], 0, 0, 0);
                acc[ci][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_l, acc[ci][t], 0, 0, 0);
              }
              acc[ci][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_h, acc[ci][t], 0, 0, 0);
              b_h = n_h; b_l = n_l;
            }
          }
        }
      }
    }
  }
  if (want_csum) wg_csum_finish(cs, (float4*)smem, nslab, tid, csum, blk.z, n0, cout);
  if (!wave_live) return;
#pragma unroll
  for (int ci = 0; ci < NCH; ++ci)
#pragma unroll
    for (int t = 0; t < TM; ++t)
      if (EXACT || t < ck[ci].T) WG_STORE_TILE(acc[ci][t], blk.z, ck[ci].s0 + t, n0 + nw * 32);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Round 5: the same weight gradient on bf16-STORED operands (precision mode 1 with half-precision storage of the training
// activations and their gradients: BASELINE configs[3]'s "bf16").  What bounded conv_wgrad_tr2_kernel in that mode was the feed:
// 49 KB of raw fp32 per tile through L2 -> LDS and a conversion pass, for a third of the MFMA work of the fp32-class mode.  Here the
// tile arrives as the MFMA operand type: LDS-DMA of [pixel][32 channels] bf16 rows (64 B per pixel: 16 + 9 pieces of 1 KB per tile
// instead of 32 + 17), NO conversion pass, the transposed reads (ds_read_b64_tr_b16) straight on the DMA'd image -- a half-wave's 32
// eight-byte reads cover four pixels x 64 B = 256 contiguous bytes: conflict-free without the [hi | lo] swap of the fp32 form.  With
// 25 KB per tile the images are DOUBLE-BUFFERED: the next tile's pieces are requested right behind the barrier that publishes the
// current one and land under its MFMAs (one barrier per tile).  The bias column sums read the dY image from LDS (chunk-0 blocks only).
template <int NCH, int TM, bool EXACT, bool HALO = true>
__global__ __launch_bounds__(256, 2) void conv_wgrad_tr2b_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy,
                                                               const int4* __restrict__ steps, const int* __restrict__ chunk_start,
                                                               float* __restrict__ partial, float* __restrict__ csum, int B, int in_h,
                                                               int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps,
                                                               int tiles_x, int tiles_per_image, int tiles_total, int tiles_per_split) {
  constexpr int XW = HALO ? WT_XW : WG_TC, XPX = HALO ? WT_XPX : WT_PX, XO = HALO ? 1 : 0;
  constexpr int PXB = 64;                                     // bytes of one pixel's 32 channels
  constexpr int XPC = (XPX + 15) / 16;                        // DMA pieces (16 pixels x 64 B) per chunk: 9 / 4
  constexpr int SLAB = WT_PX * PXB;                           // 4096: one 32-channel slab of the dY tile
  constexpr int IMG_DY = 4 * SLAB, IMG_X = XPC * 1024, BUF = IMG_DY + NCH * IMG_X;
  static_assert(!HALO ? TM == 1 : true, "the no-halo image serves 1x1 tables");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63, nw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WgBlock blk = wg_block_xcd();
  const int n0 = blk.x * 128;
  WgChunk<TM> ck[NCH];
  int chan[NCH];                                              // (for wg_chan_of)
#pragma unroll
  for (int ci = 0; ci < NCH; ++ci) {
    wg_chunk_load(ck[ci], steps, chunk_start, blk.y * NCH + ci);
    chan[ci] = ck[ci].chan;
  }
  f32x16 acc[NCH][TM];
  wg_zero(acc);
  const WgRange tiles = wg_range(blk.z, tiles_per_split, tiles_total);
  const int t_begin = tiles.begin, t_end = tiles.end;
  const bool wave_live = n0 + nw * 32 < cout;
  const int nslab = min(4, (cout - n0 + 31) >> 5);
  const bool want_csum = csum != nullptr && blk.y == 0;
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
  const int g = lane >> 4, qd = (lane & 15) >> 2, pp = lane & 3;
  const int tr_unit = (8 * (g >> 1) + qd) * PXB + (4 * (g & 1) + pp) * 8;
  auto frag = [&](const unsigned char* u, bf16x8& h) {
    const wt_v4s h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wt_v4s __attribute__((address_space(3)))*)u);
    const wt_v4s h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wt_v4s __attribute__((address_space(3)))*)(u + 4 * PXB));
    h = (bf16x8){h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
  };
  // LDS-DMA of one tile: 16 pieces of dY (slab, 16 pixels: 16 x 64 B) + XPC per chunk of the input image; lane = (pixel, 16-byte quarter)
  auto issue = [&](int tile, unsigned char* buf) {
    const auto [b, ty0, tx0] = wg_tile(tile, tiles_per_image, tiles_x);
    const int q = lane & 3, pl = lane >> 2;
    for (int wi = nw; wi < 16 + NCH * XPC; wi += 4) {
      const void* src = g_wg_zero;
      if (wi < 16 && (wi >> 2) >= nslab) continue;          // slab beyond cout: no wave reads it
      if (wi < 16) {
        const int p = 16 * (wi & 3) + pl, n = n0 + (wi >> 2) * 32 + q * 8;
        const int y = ty0 + (p >> 5), xx = tx0 + (p & 31);
        if (y < oh && xx < ow && n < cout) src = dy + (((int64_t)b * oh + y) * ow + xx) * dy_ld + n;
      } else {
        const int ci = (wi - 16) / XPC, pj = (wi - 16) - ci * XPC;        // wave-uniform
        const int P = 16 * pj + pl;
        const int row = P / XW, col = P - row * XW;
        const int iy = ty0 - XO + row, ix = tx0 - XO + col;
        if (P < XPX && iy >= 0 && iy < in_h && ix >= 0 && ix < in_w)
          src = x + (((int64_t)b * in_h + iy) * in_w + ix) * in_ld + wg_chan_of(chan, ci) + q * 8;
      }
      unsigned char* dst = buf + (wi < 16 ? wi * 1024 : IMG_DY + (wi - 16) * 1024);
      __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
    }
  };
  if (t_begin < t_end) issue(t_begin, smem);
  for (int tile = t_begin; tile < t_end; ++tile) {
    unsigned char* const cur = smem + ((tile - t_begin) & 1) * BUF;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's pieces of the current tile have landed (hipcc adds no wait for LDS-DMA)
    __syncthreads();                                        // ... everybody's have, and the previous tile's MFMA reads are done
    if (tile + 1 < t_end) issue(tile + 1, smem + (((tile - t_begin) & 1) ^ 1) * BUF);
    if (want_csum) {                                        // bias column sums: 4 channels per thread over its units of the dY image
      const WgUnits un = wg_units(nslab);
      if (tid < un.stride)
        for (int i = tid; i < 64 * un.NQ; i += un.stride) {
          const int p = i / un.NQ, cq = i - p * un.NQ;
          const uint2 u = *(const uint2*)(cur + (cq >> 3) * SLAB + p * PXB + (cq & 7) * 8);
          cs.x += __uint_as_float(u.x << 16); cs.y += __uint_as_float(u.x & 0xffff0000u);
          cs.z += __uint_as_float(u.y << 16); cs.w += __uint_as_float(u.y & 0xffff0000u);
        }
    }
    if (wave_live) {
#pragma unroll 1
      for (int ks = 0; ks < 4; ++ks) {
        const int row = ks >> 1, xh = (ks & 1) * 16;
        bf16x8 a_h;
        frag(cur + nw * SLAB + (row * 32 + xh) * PXB + tr_unit, a_h);
#pragma unroll
        for (int ci = 0; ci < NCH; ++ci) {
          const unsigned char* const im = cur + IMG_DY + ci * IMG_X;
          const int pb0 = (row + XO + ck[ci].tdy[0]) * XW + xh + XO + ck[ci].tdx[0];
          bf16x8 b_h;
          frag(im + pb0 * PXB + tr_unit, b_h);
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            if (EXACT || t < ck[ci].T) {
              bf16x8 n_h = b_h;
              if (t + 1 < TM && (EXACT || t + 1 < ck[ci].T)) {
                const int pb = (row + XO + ck[ci].tdy[t + 1]) * XW + xh + XO + ck[ci].tdx[t + 1];
                frag(im + pb * PXB + tr_unit, n_h);
              }
              acc[ci][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_h, b_h, acc[ci][t], 0, 0, 0);
              b_h = n_h;
            }
          }
        }
      }
    }
  }
  if (want_csum) wg_csum_finish(cs, (float4*)smem, nslab, tid, csum, blk.z, n0, cout);
  if (!wave_live) return;
#pragma unroll
  for (int ci = 0; ci < NCH; ++ci)
#pragma unroll
    for (int t = 0; t < TM; ++t)
      if (EXACT || t < ck[ci].T) WG_STORE_TILE(acc[ci][t], blk.z, ck[ci].s0 + t, n0 + nw * 32);
}

// profiling brackets of conv_mfma.hip: a weight-gradient launch is recorded with info = {B, oh, ow, nsteps, cout, nchunks, splits, 0}
// (bn = 0 marks it) and the algorithmic 2 * 32 * flop_steps * cout * B * oh * ow (flop_steps < nsteps where the table carries
// zero-weight pad steps)
int ppst_prof_begin_(double flop, const int* info8, hipStream_t st);
void ppst_prof_end_(int slot, hipStream_t st);
static int wgrad_prof_begin(int B, int oh, int ow, int cout, int nsteps, int flop_steps, int nchunks, int splits, hipStream_t st) {
  const int inf[8] = {B, oh, ow, nsteps, cout, nchunks, splits, 0};
  return ppst_prof_begin_(2.0 * 32.0 * (flop_steps > 0 ? flop_steps : nsteps) * (double)cout * (double)B * oh * ow, inf, st);
}
static int g_wgrad_flop_steps = 0;   // set by ppst_wgrad_flop_steps for the NEXT weight-gradient launch (profiling only)
extern "C" int ppst_wgrad_flop_steps(int flop_steps) { g_wgrad_flop_steps = flop_steps; return PPST_OK; }

// The argument checks of every weight-gradient launcher, in the order the return codes promise: sizes, the empty batch (PPST_OK and
// nothing to launch: the caller tests B == 0 itself), null pointers.  *aligned: 16-byte rows and pointers (the LDS-staged and the
// transposed-read kernels need them; every caller on the train path has them)
static int wgrad_check(const void* x, const void* dy, const void* steps, const void* chunk_start, const void* partial, int B, int in_h,
                       int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps, int nchunks, int splits, bool* aligned) {
  if (B < 0 || in_h <= 0 || in_w <= 0 || in_ld <= 0 || oh <= 0 || ow <= 0 || dy_ld < cout || cout <= 0 || nsteps <= 0 ||
      nchunks <= 0 || splits <= 0)
    return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!x || !dy || !steps || !chunk_start || !partial) return PPST_ENULL;
  *aligned = four_wide_ok(PPST_ST_F32, {cout, dy_ld, in_ld}, {x, dy});
  return PPST_OK;
}
// the 2 x 32-pixel tiles of the output, dealt out to ``splits`` pixel ranges
struct WgradTiles { int tiles_x, per_image, total, per_split; };
static WgradTiles wgrad_tiles(int B, int oh, int ow, int splits) {
  WgradTiles t;
  t.tiles_x = cdiv(ow, WG_TC);
  t.per_image = cdiv(oh, WG_TR) * t.tiles_x;
  t.total = B * t.per_image;
  t.per_split = cdiv(t.total, splits);
  return t;
}

// conv_wgrad_tr2_kernel on fp32 operands: ``splits`` partial slots = pixel ranges; csum (optional): [splits][cout] partial column
// sums of dy, written by the blocks of chunk 0 -- their column-wise sum is the bias gradient (ppst_wgrad_scatter finishes it)
extern "C" int ppst_conv_wgrad_tr2_st(const void* x, const void* dy, const void* steps, const void* chunk_start, void* partial, void* csum,
                                      int B, int in_h, int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps,
                                      int nchunks, int splits, int max_taps, int min_taps, int halo, int passes, int st, void* stream);
extern "C" int ppst_conv_wgrad_tr2(const void* x, const void* dy, const void* steps, const void* chunk_start, void* partial, void* csum,
                                   int B, int in_h, int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps,
                                   int nchunks, int splits, int max_taps, int min_taps, int halo, int passes, void* stream) {
  return ppst_conv_wgrad_tr2_st(x, dy, steps, chunk_start, partial, csum, B, in_h, in_w, in_ld, oh, ow, dy_ld, cout, nsteps, nchunks, splits,
                                max_taps, min_taps, halo, passes, PPST_ST_F32, stream);
}
// st: storage type of x and dy -- PPST_ST_F32, or PPST_ST_BF16 with passes == 1 (conv_wgrad_tr2b_kernel: the operands arrive as the
// MFMA type; cout, in_ld, dy_ld multiples of 8, 16-byte aligned x / dy)
extern "C" int ppst_conv_wgrad_tr2_st(const void* x, const void* dy, const void* steps, const void* chunk_start, void* partial, void* csum,
                                      int B, int in_h, int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps,
                                      int nchunks, int splits, int max_taps, int min_taps, int halo, int passes, int st, void* stream) {
  if (st != PPST_ST_F32 && st != PPST_ST_BF16) return PPST_EINVAL;
  if (st == PPST_ST_BF16 && (passes != 1 || cout % 8 || dy_ld % 8 || in_ld % 8)) return PPST_EINVAL;
  if (passes != 1 && passes != 3) return PPST_EINVAL;
  bool aligned = false;
  const int rc = wgrad_check(x, dy, steps, chunk_start, partial, B, in_h, in_w, in_ld, oh, ow, dy_ld, cout, nsteps, nchunks, splits, &aligned);
  if (rc != PPST_OK || B == 0) return rc;
  if (!aligned) return PPST_EINVAL;
  const WgradTiles t = wgrad_tiles(B, oh, ow, splits);
  // max_taps / min_taps: the caller's promise about the table's chunk lengths (the table lives on the device): <= 4 steps in every
  // chunk and an even chunk count select the two-chunks-per-block form
  const bool pair = max_taps > 0 && max_taps <= 4 && (nchunks & 1) == 0;
  // halo == 0: the caller's promise that every step has offset (0, 0) on an input of the output's extent (1x1 conv tables)
  const int one = (halo == 0 && max_taps == 1 && min_taps == 1 && in_h == oh && in_w == ow) ? ((nchunks & 3) == 0 ? 4 : ((nchunks & 1) == 0 ? 2 : 0)) : 0;
  dim3 grid(cdiv(cout, 128), one ? nchunks / one : (pair ? nchunks / 2 : nchunks), splits);
  const int slot = wgrad_prof_begin(B, oh, ow, cout, nsteps, g_wgrad_flop_steps, nchunks, splits, as_stream(stream));
  g_wgrad_flop_steps = 0;
  // the launch of one kernel instantiation (the variadic part: its name) on operands stored as T
#define WG_KERNEL(T, ...)                                                                                                             \
  PPST_LAUNCH((__VA_ARGS__), grid, dim3(256), 0, as_stream(stream), (const T*)x, (const T*)dy, (const int4*)steps,                      \
              (const int*)chunk_start, (float*)partial, (float*)csum, B, in_h, in_w, in_ld, oh, ow, dy_ld, cout, nsteps, t.tiles_x,    \
              t.per_image, t.total, t.per_split)
  // <chunks per block, taps per chunk, EXACT, HALO> of the storage type's kernel; fp32 storage: X1 = single pass
#define WG_LAUNCH(NCH, TM, EX, HALO)                                                                                                  \
  do {                                                                                                                                \
    if (st == PPST_ST_BF16) WG_KERNEL(unsigned short, conv_wgrad_tr2b_kernel<NCH, TM, EX, HALO>);                                     \
    else if (passes == 1) WG_KERNEL(float, conv_wgrad_tr2_kernel<NCH, TM, true, EX, HALO>);                                           \
    else WG_KERNEL(float, conv_wgrad_tr2_kernel<NCH, TM, false, EX, HALO>);                                                           \
  } while (0)
  if (one == 4) WG_LAUNCH(4, 1, true, false);
  else if (one == 2) WG_LAUNCH(2, 1, true, false);
  else if (pair && min_taps == 4 && max_taps == 4) WG_LAUNCH(2, 4, true, true);
  else if (pair) WG_LAUNCH(2, 4, false, true);
  else if (min_taps == WG_MAXT && max_taps == WG_MAXT) WG_LAUNCH(1, WG_MAXT, true, true);
  else WG_LAUNCH(1, WG_MAXT, false, true);
#undef WG_LAUNCH
#undef WG_KERNEL
  ppst_prof_end_(slot, as_stream(stream));
  return PPST_LAUNCH_CHECK();
}

// the exact-fp32 MFMA (precision 2: verification; and operands the kernels above cannot take)
extern "C" int ppst_conv_wgrad_f32(const void* x, const void* dy, const void* steps, const void* chunk_start, void* partial,
                                   int B, int in_h, int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps,
                                   int nchunks, int splits, void* stream) {
  bool aligned = false;
  const int rc = wgrad_check(x, dy, steps, chunk_start, partial, B, in_h, in_w, in_ld, oh, ow, dy_ld, cout, nsteps, nchunks, splits, &aligned);
  if (rc != PPST_OK || B == 0) return rc;
  // every split block must write its partial (the scatter sums all `splits` of them): an empty split writes zeros
  dim3 grid(cdiv(cout, 128), nchunks, splits);
  if (aligned) {                 // the LDS-staged kernel needs 16-B aligned rows; else the direct one
    const WgradTiles t = wgrad_tiles(B, oh, ow, splits);
    PPST_LAUNCH(conv_wgrad_lds_kernel, grid, dim3(256), 0, as_stream(stream), (const float*)x, (const float*)dy, (const int4*)steps,
                (const int*)chunk_start, (float*)partial, B, in_h, in_w, in_ld, oh, ow, dy_ld, cout, nsteps, t.tiles_x, t.per_image,
                t.total, t.per_split);
    return PPST_LAUNCH_CHECK();
  }
  PPST_LAUNCH(conv_wgrad_kernel, grid, dim3(256), 0, as_stream(stream), (const float*)x, (const float*)dy, (const int4*)steps,
              (const int*)chunk_start, (float*)partial, B, in_h, in_w, in_ld, oh, ow, dy_ld, cout, nsteps, cdiv(B * oh, splits));
  return PPST_LAUNCH_CHECK();
}

// dW[n][src_c+k][ky][kx] (strides sn, sc, sy, sx) (+)= scale * sum_splits partial[split][step][n][k]
// One block per (step s, output channel n): 32 k-values x 8 split lanes -- thread (k, j) adds the partial slots j, j + 8, ...,
// the eight sums meet in LDS in a fixed order.  (One thread per output walking ALL slots, the first form, was a chain of up to
// 2048 dependent-latency loads on 36 blocks for the thin layers -- 32 -> 32 @512^2: 0.13 of its 0.39 ms -- and the bias column
// sums rode on block 0 in front of its own outputs.)  The bias gradient (column sums of the weight-gradient kernel's per-block
// partial sums of dy) takes cdiv(cout, 32) extra blocks of the same shape.
__global__ __launch_bounds__(256) void wgrad_scatter_kernel(const float* __restrict__ partial, const int* __restrict__ src_c,
                                                            const int* __restrict__ src_ky, const int* __restrict__ src_kx,
                                                            float* __restrict__ dw, int64_t sn, int64_t sc, int64_t sy, int64_t sx,
                                                            int cout, int nsteps, int splits, float scale, int accumulate,
                                                            int nrows, const float* __restrict__ csum, float* __restrict__ db,
                                                            int csum_rows, int db_accumulate) {
  __shared__ float red[8][32];
  const int k = threadIdx.x & 31, j = threadIdx.x >> 5;
  if ((int)blockIdx.x >= nrows) {                           // bias blocks
    const int n = ((int)blockIdx.x - nrows) * 32 + k;
    float v = 0.f;
    if (n < cout)
      for (int r = j; r < csum_rows; r += 8) v += csum[(int64_t)r * cout + n];
    red[j][k] = v;
    __syncthreads();
    if (j == 0 && n < cout) {
      v = ((red[0][k] + red[1][k]) + (red[2][k] + red[3][k])) + ((red[4][k] + red[5][k]) + (red[6][k] + red[7][k]));
      db[n] = db_accumulate ? db[n] + v : v;
    }
    return;
  }
  const int s = (int)blockIdx.x / cout, n = (int)blockIdx.x - s * cout;
  const int c0 = src_c[s];
  if (c0 < 0) return;                                       // zero-weight pad step (block-uniform)
  float v = 0.f;
  for (int sp = j; sp < splits; sp += 8) v += partial[(((int64_t)sp * nsteps + s) * cout + n) * 32 + k];
  red[j][k] = v;
  __syncthreads();
  if (j == 0) {
    v = ((red[0][k] + red[1][k]) + (red[2][k] + red[3][k])) + ((red[4][k] + red[5][k]) + (red[6][k] + red[7][k]));
    float* o = dw + n * sn + (int64_t)(c0 + k) * sc + src_ky[s] * sy + src_kx[s] * sx;
    *o = accumulate ? *o + v * scale : v * scale;
  }
}
extern "C" int ppst_wgrad_scatter(const void* partial, const void* src_c, const void* src_ky, const void* src_kx, void* dw,
                                  int64_t sn, int64_t sc, int64_t sy, int64_t sx, int cout, int nsteps, int splits, float scale,
                                  int accumulate, const void* csum, void* db, int csum_rows, int db_accumulate, void* stream) {
  if (cout <= 0 || nsteps <= 0 || splits <= 0 || (csum && csum_rows <= 0)) return PPST_EINVAL;
  if (!partial || !src_c || !src_ky || !src_kx || !dw || (csum && !db)) return PPST_ENULL;
  const int64_t nrows = (int64_t)nsteps * cout;
  const int64_t blocks = nrows + (csum ? cdiv(cout, 32) : 0);
  if (blocks > 0x7fffffffll) return PPST_EINVAL;
  PPST_LAUNCH(wgrad_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const float*)partial, (const int*)src_c,
              (const int*)src_ky, (const int*)src_kx, (float*)dw, sn, sc, sy, sx, cout, nsteps, splits, scale, accumulate, (int)nrows,
              (const float*)csum, (float*)db, csum_rows, db_accumulate);
  return PPST_LAUNCH_CHECK();
}

// FromRGB weight gradient: dw[n][c] (+)= scale * sum_p dy[p][n] * x[p][c], c < cin <= 4.
// One block per 64-pixel-row slab: lane = n (<= 64 per pass), partial sums through atomics-free
// two-stage reduction: partial[block][n][cin] then summed by the scatter-style finalize below.
__global__ __launch_bounds__(256) void wgrad_small_cin_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ partial, int64_t npix, int cin, int in_ld,
                                                              int cout, int64_t pix_per_block) {
  __shared__ float sm[4][64][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * pix_per_block, p1 = min(p0 + pix_per_block, npix);
  for (int nb = 0; nb < cout; nb += 64) {
    const int n = nb + lane;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < cout) {
      int64_t p = p0 + w;
      for (; p + 12 < p1; p += 16) {            // four pixels in flight per wave (independent loads)
        const float g0 = dy[p * cout + n], g1 = dy[(p + 4) * cout + n], g2 = dy[(p + 8) * cout + n], g3 = dy[(p + 12) * cout + n];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < cin) a[c] += (g0 * x[p * in_ld + c] + g1 * x[(p + 4) * in_ld + c]) + (g2 * x[(p + 8) * in_ld + c] + g3 * x[(p + 12) * in_ld + c]);
      }
      for (; p < p1; p += 4) {
        float g = dy[p * cout + n];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < cin) a[c] += g * x[p * in_ld + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) sm[w][lane][c] = a[c];
    __syncthreads();
    if (w == 0 && n < cout)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < cin) partial[((int64_t)blockIdx.x * cout + n) * cin + c] = sm[0][lane][c] + sm[1][lane][c] + sm[2][lane][c] + sm[3][lane][c];
    __syncthreads();
  }
}
// float4 form for cout = 4 Q with Q a divisor of 256 (FromRGB: cout = 32 -> the scalar form above ran half its lanes, 128 B per
// wave load): thread = (pixel slot tid / Q, channel quad tid % Q); 256 / Q pixels per block pass, four passes in flight.
// (Another thread-to-pixel map and so another order of the sums than the scalar form: not a V = 4 copy of it.)
template <int ST = PPST_ST_F32>     // storage type of dy (x: the fp32 image / RGB gradient)
__global__ __launch_bounds__(256) void wgrad_small_cin4_kernel(const float* __restrict__ x, const void* __restrict__ dy,
                                                               float* __restrict__ partial, int64_t npix, int cin, int in_ld, int Q,
                                                               int64_t pix_per_block) {
  __shared__ float4 sm[4][256];                              // [input channel][thread]
  const int q = threadIdx.x % Q, slot = threadIdx.x / Q, P = 256 / Q;
  const int64_t p0 = (int64_t)blockIdx.x * pix_per_block, p1 = min(p0 + pix_per_block, npix);
  float4 a[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) a[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t p = p0 + slot;
  for (; p + 3 * P < p1; p += 4 * P) {
    const float4 g0 = st_ld4<ST>(dy, (p * Q + q) * 4), g1 = st_ld4<ST>(dy, ((p + P) * Q + q) * 4), g2 = st_ld4<ST>(dy, ((p + 2 * P) * Q + q) * 4),
                 g3 = st_ld4<ST>(dy, ((p + 3 * P) * Q + q) * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < cin) {
        const float x0 = x[p * in_ld + c], x1 = x[(p + P) * in_ld + c], x2 = x[(p + 2 * P) * in_ld + c], x3 = x[(p + 3 * P) * in_ld + c];
        a[c].x += (g0.x * x0 + g1.x * x1) + (g2.x * x2 + g3.x * x3);
        a[c].y += (g0.y * x0 + g1.y * x1) + (g2.y * x2 + g3.y * x3);
        a[c].z += (g0.z * x0 + g1.z * x1) + (g2.z * x2 + g3.z * x3);
        a[c].w += (g0.w * x0 + g1.w * x1) + (g2.w * x2 + g3.w * x3);
      }
  }
  for (; p < p1; p += P) {
    const float4 g = st_ld4<ST>(dy, (p * Q + q) * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < cin) {
        const float xv = x[p * in_ld + c];
        a[c].x += g.x * xv; a[c].y += g.y * xv; a[c].z += g.z * xv; a[c].w += g.w * xv;
      }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) sm[c][threadIdx.x] = a[c];
  __syncthreads();
  if (threadIdx.x < Q) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < cin) {
        float4 t = sm[c][q];
        for (int r = 1; r < P; ++r) { const float4 v = sm[c][r * Q + q]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
        float* o = partial + ((int64_t)blockIdx.x * 4 * Q + 4 * q) * cin + c;      // partial[block][n][cin]
        o[0] = t.x; o[cin] = t.y; o[2 * cin] = t.z; o[3 * cin] = t.w;
      }
  }
}
// out[i] (+)= scale * sum_b partial[b][i]: a block owns 32 consecutive outputs, its 8 thread groups walk the partial rows
// 8 apart with 4 loads in flight each (double accumulation, fixed order).  (The one-thread-per-output form walked
// `nblocks` dependent loads per thread: 0.1-0.3 ms for the 128-1280 partial rows of the FromRGB / bias gradients.)
__global__ __launch_bounds__(256) void sum_blocks_kernel(const float* __restrict__ partial, float* __restrict__ out, int nblocks,
                                                         int64_t n, float scale, int accumulate) {
  __shared__ double sm[8][32];
  const int il = threadIdx.x & 31, kk = threadIdx.x >> 5;
  const int64_t i = (int64_t)blockIdx.x * 32 + il;
  double s = 0.0;
  if (i < n) {
    int b = kk;
    for (; b + 24 < nblocks; b += 32) {
      const float v0 = partial[(int64_t)b * n + i], v1 = partial[(int64_t)(b + 8) * n + i], v2 = partial[(int64_t)(b + 16) * n + i],
                  v3 = partial[(int64_t)(b + 24) * n + i];
      s += (double)v0; s += (double)v1; s += (double)v2; s += (double)v3;
    }
    for (; b < nblocks; b += 8) s += (double)partial[(int64_t)b * n + i];
  }
  sm[kk][il] = s;
  __syncthreads();
  if (kk == 0 && i < n) {
#pragma unroll
    for (int r = 1; r < 8; ++r) s += sm[r][il];
    float v = (float)s * scale;
    out[i] = accumulate ? out[i] + v : v;
  }
}
#define WSC_PIX 1024    // pixels per block of the FromRGB weight gradient (4096 left half the chip idle at 2 x 512^2 pixels)
extern "C" int64_t ppst_wgrad_small_cin_ws(int64_t npix, int cin, int cout) { return cdiv64(npix, WSC_PIX) * cout * cin * (int64_t)sizeof(float); }
extern "C" int ppst_wgrad_small_cin_st(const void* x, const void* dy, void* dw, void* ws, int64_t npix, int cin, int in_ld, int cout,
                                       float scale, int accumulate, int dy_st, void* stream);
extern "C" int ppst_wgrad_small_cin(const void* x, const void* dy, void* dw, void* ws, int64_t npix, int cin, int in_ld, int cout,
                                    float scale, int accumulate, void* stream) {
  return ppst_wgrad_small_cin_st(x, dy, dw, ws, npix, cin, in_ld, cout, scale, accumulate, PPST_ST_F32, stream);
}
extern "C" int ppst_wgrad_small_cin_st(const void* x, const void* dy, void* dw, void* ws, int64_t npix, int cin, int in_ld, int cout,
                                       float scale, int accumulate, int dy_st, void* stream) {
  if ((unsigned)dy_st > 2u) return PPST_EINVAL;
  if (npix <= 0 || cin <= 0 || cin > 4 || in_ld < cin || cout <= 0) return PPST_EINVAL;
  if (!x || !dy || !dw || !ws) return PPST_ENULL;
  int nblocks = (int)cdiv64(npix, WSC_PIX);
  if (four_wide_ok(dy_st, {cout}, {dy}) && cout / 4 <= 256 && 256 % (cout / 4) == 0)
    PPST_ST_SWITCH(dy_st, PPST_LAUNCH(wgrad_small_cin4_kernel<ST_>, dim3(nblocks), dim3(256), 0, as_stream(stream), (const float*)x, dy,
                                      (float*)ws, npix, cin, in_ld, cout / 4, (int64_t)WSC_PIX));
  else if (dy_st)
    return PPST_EINVAL;
  else
    PPST_LAUNCH(wgrad_small_cin_kernel, dim3(nblocks), dim3(256), 0, as_stream(stream), (const float*)x, (const float*)dy, (float*)ws,
                npix, cin, in_ld, cout, (int64_t)WSC_PIX);
  int e = PPST_LAUNCH_CHECK();
  if (e) return e;
  int64_t n = (int64_t)cout * cin;
  PPST_LAUNCH(sum_blocks_kernel, dim3((unsigned)cdiv64(n, 32)), dim3(256), 0, as_stream(stream), (const float*)ws, (float*)dw, nblocks,
              n, scale, accumulate);
  return PPST_LAUNCH_CHECK();
}

// column sums: out[c] (+)= scale * sum over rows of x[row][c]  (bias gradients; rows = B*H*W)
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, float* __restrict__ partial, int64_t rows,
                                                             int C, int ld, int64_t rows_per_block) {
  __shared__ float sm[256];
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, rows);
  int lanes = 1;
  while (lanes < C && lanes < 256) lanes <<= 1;
  const int nrows = 256 / lanes, cl = threadIdx.x % lanes, pr = threadIdx.x / lanes;
  for (int cb = 0; cb < C; cb += lanes) {
    int c = cb + cl;
    float a = 0.f;
    if (c < C)
      for (int64_t r = r0 + pr; r < r1; r += nrows) a += x[r * ld + c];
    sm[threadIdx.x] = a;
    __syncthreads();
    if (pr == 0 && c < C) {
      for (int q = 1; q < nrows; ++q) a += sm[q * lanes + cl];
      partial[(int64_t)blockIdx.x * C + c] = a;
    }
    __syncthreads();
  }
}
// 16-B-per-lane version (C % 4 == 0, ld % 4 == 0): lane = 4 columns, 4 rows in flight per thread
// (four accumulators per column: another order of the sums than colsum_partial_kernel, not a V = 4 copy of it)
template <int ST = PPST_ST_F32>
__global__ __launch_bounds__(256) void colsum4_partial_kernel(const void* __restrict__ x, float* __restrict__ partial, int64_t rows,
                                                              int C, int ld, int64_t rows_per_block) {
  __shared__ float4 sm[256];
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, rows);
  const int c4n = C >> 2;
  int lanes = 1;
  while (lanes < c4n && lanes < 256) lanes <<= 1;
  const int nrows = 256 / lanes, cl = threadIdx.x % lanes, pr = threadIdx.x / lanes;
  for (int cb = 0; cb < c4n; cb += lanes) {
    const int c = (cb + cl) * 4;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
    if (c < C) {
      int64_t r = r0 + pr;
      for (; r + 3 * (int64_t)nrows < r1; r += 4 * (int64_t)nrows) {
        const float4 v0 = st_ld4<ST>(x, r * ld + c), v1 = st_ld4<ST>(x, (r + nrows) * ld + c);
        const float4 v2 = st_ld4<ST>(x, (r + 2 * nrows) * ld + c), v3 = st_ld4<ST>(x, (r + 3 * nrows) * ld + c);
        a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
        a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
        a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
        a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
      }
      for (; r < r1; r += nrows) {
        const float4 v0 = st_ld4<ST>(x, r * ld + c);
        a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
      }
    }
    float4 a = make_float4((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y), (a0.z + a1.z) + (a2.z + a3.z), (a0.w + a1.w) + (a2.w + a3.w));
    sm[threadIdx.x] = a;
    __syncthreads();
    if (pr == 0 && c < C) {
      for (int q = 1; q < nrows; ++q) { float4 u = sm[q * lanes + cl]; a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w; }
      *(float4*)(partial + (int64_t)blockIdx.x * C + c) = a;
    }
    __syncthreads();
  }
}
extern "C" int64_t ppst_colsum_ws(int64_t rows, int C) { return cdiv64(rows, 2048) * C * (int64_t)sizeof(float); }
extern "C" int ppst_colsum_st(const void* x, void* out, void* ws, int64_t rows, int C, int ld, float scale, int accumulate, int st, void* stream);
extern "C" int ppst_colsum(const void* x, void* out, void* ws, int64_t rows, int C, int ld, float scale, int accumulate, void* stream) {
  return ppst_colsum_st(x, out, ws, rows, C, ld, scale, accumulate, PPST_ST_F32, stream);
}
// st: storage type of x (round 5: the bf16-stored gradients of precision mode 1); sums and out fp32
extern "C" int ppst_colsum_st(const void* x, void* out, void* ws, int64_t rows, int C, int ld, float scale, int accumulate, int st, void* stream) {
  if ((unsigned)st > 2u) return PPST_EINVAL;
  if (rows <= 0 || C <= 0 || ld < C) return PPST_EINVAL;
  if (!x || !out || !ws) return PPST_ENULL;
  int nblocks = (int)cdiv64(rows, 2048);
  if (four_wide_ok(st, {C, ld}, {x}, {ws}))
    PPST_ST_SWITCH(st, PPST_LAUNCH(colsum4_partial_kernel<ST_>, dim3(nblocks), dim3(256), 0, as_stream(stream), x, (float*)ws, rows, C, ld,
                                   (int64_t)2048));
  else if (st)
    return PPST_EINVAL;
  else
    PPST_LAUNCH(colsum_partial_kernel, dim3(nblocks), dim3(256), 0, as_stream(stream), (const float*)x, (float*)ws, rows, C, ld, (int64_t)2048);
  int e = PPST_LAUNCH_CHECK();
  if (e) return e;
  PPST_LAUNCH(sum_blocks_kernel, dim3(cdiv(C, 32)), dim3(256), 0, as_stream(stream), (const float*)ws, (float*)out, nblocks, (int64_t)C,
              scale, accumulate);
  return PPST_LAUNCH_CHECK();
}

// ---------------------------------------------------------------- linear ----
// dW[n][k] (+)= scale * sum_b dY[b][n] * X[b][k] ;  dX[b][k] = scale * sum_n dY[b][n] * W[n][k]
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dw,
                                                           int B, int N, int K, float scale, int accumulate, int64_t total) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int k = (int)(t % K), n = (int)(t / K);
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dy[(int64_t)b * N + n] * x[(int64_t)b * K + k];
    dw[t] = accumulate ? dw[t] + s * scale : s * scale;
  }
}
// K % 4 == 0, 16-byte aligned x / dw: four columns per thread.  FUSED (round 5, LinearFn of ppst_amd/autograd.py: the E2 projector
// chains ran 7 launches per linear and backward) folds in the passes around the gradient: ``relu_in`` -- x is read as max(x, 0) (the
// linear sits behind nn.ReLU, encoder_col.py:47-93); ``db`` -- the bias gradient bscale * sum_b dY[b][n] from the thread that owns
// column 0 of row n (dY's rows are read by it anyway).  Without FUSED those four arguments are not read.
template <bool FUSED>
__global__ __launch_bounds__(256) void linear_wgrad4_kernel(const float* __restrict__ dy, const float4* __restrict__ x, float4* __restrict__ dw,
                                                            float* __restrict__ db, int B, int N, int K4, float scale, float bscale,
                                                            int accumulate, int b_accumulate, int relu_in, int64_t total4) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total4; t += (int64_t)gridDim.x * 256) {
    const int k4 = (int)(t % K4), n = (int)(t / K4);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    float sd = 0.f;
    for (int b = 0; b < B; ++b) {
      const float d = dy[(int64_t)b * N + n];
      float4 v = x[(int64_t)b * K4 + k4];
      if (FUSED && relu_in) { v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f; }
      s.x += d * v.x; s.y += d * v.y; s.z += d * v.z; s.w += d * v.w;
      sd += d;
    }
    float4 o = make_float4(s.x * scale, s.y * scale, s.z * scale, s.w * scale);
    if (accumulate) { const float4 p = dw[t]; o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w; }
    dw[t] = o;
    if (FUSED && db && k4 == 0) db[n] = b_accumulate ? db[n] + sd * bscale : sd * bscale;
  }
}
// dX = dY W streams the weight matrix once (4*N*K bytes): block (kx, ns) owns 256 columns k and the LDG_ROWS rows
// n of its slice, accumulates every batch row in registers (dY[b][n] is a wave-uniform broadcast) and writes a partial;
// a second launch sums the slices in a fixed order (deterministic).  (Round 1's version ran one thread per output with a
// sequential loop over n: 16 blocks, latency bound -- 17 % of the train step.)
#define LDG_ROWS 16                 // (32: 19 us per launch at N = 1024, 16: 12, 8: 11 with twice the partial traffic)
#define LDG_BMAX 16
__global__ __launch_bounds__(256) void linear_dgrad_partial_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                   float* __restrict__ partial, int B, int N, int K, int b0) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n0 = blockIdx.y * LDG_ROWS, n1 = min(n0 + LDG_ROWS, N);
  float acc[LDG_BMAX];
#pragma unroll
  for (int b = 0; b < LDG_BMAX; ++b) acc[b] = 0.f;
  if (k < K) {
    if (n1 - n0 == LDG_ROWS) {
      // full slice: all LDG_ROWS weight loads are issued before the first use (a runtime trip count left hipcc a chain of
      // partially unrolled dependent-latency loads: 27 us per launch for 8 MB of weights)
      float wv[LDG_ROWS];
#pragma unroll
      for (int i = 0; i < LDG_ROWS; ++i) wv[i] = w[(int64_t)(n0 + i) * K + k];
#pragma unroll
      for (int i = 0; i < LDG_ROWS; ++i)
#pragma unroll
        for (int b = 0; b < LDG_BMAX; ++b)
          if (b0 + b < B) acc[b] += dy[(int64_t)(b0 + b) * N + n0 + i] * wv[i];
    } else {
      for (int n = n0; n < n1; ++n) {
        const float wv = w[(int64_t)n * K + k];
#pragma unroll
        for (int b = 0; b < LDG_BMAX; ++b)
          if (b0 + b < B) acc[b] += dy[(int64_t)(b0 + b) * N + n] * wv;
      }
    }
#pragma unroll
    for (int b = 0; b < LDG_BMAX; ++b)
      if (b0 + b < B) partial[((int64_t)blockIdx.y * B + b0 + b) * K + k] = acc[b];
  }
}
// GATE: dX is multiplied by [gate > 0] (gate: B x K) in the slice reduction -- the backward of the nn.ReLU in front of the linear;
// without it ``gate`` is not read
template <bool GATE>
__global__ __launch_bounds__(256) void linear_dgrad_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ gate,
                                                                  float* __restrict__ dx, int nsplit, int64_t bk, float scale) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < bk; t += (int64_t)gridDim.x * 256) {
    float s = 0.f;
    int i = 0;
    for (; i + 8 <= nsplit; i += 8) {                       // eight slices in flight, fixed order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(int64_t)(i + u) * bk + t];
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; i < nsplit; ++i) s += partial[(int64_t)i * bk + t];
    dx[t] = (!GATE || gate[t] > 0.f) ? s * scale : 0.f;
  }
}
extern "C" int ppst_linear_wgrad(const void* dy, const void* x, void* dw, int B, int N, int K, float scale, int accumulate, void* stream) {
  if (B <= 0 || N <= 0 || K <= 0) return PPST_EINVAL;
  if (!dy || !x || !dw) return PPST_ENULL;
  int64_t total = (int64_t)N * K, blocks = cdiv64(total, 256);
  if (K % 4 == 0 && ((uintptr_t)x | (uintptr_t)dw) % 16 == 0) {
    blocks = cdiv64(total / 4, 256);
    if (blocks > 8192) blocks = 8192;
    PPST_LAUNCH(linear_wgrad4_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const float*)dy, (const float4*)x,
                (float4*)dw, (float*)nullptr, B, N, K / 4, scale, 0.f, accumulate, 0, 0, total / 4);
    return PPST_LAUNCH_CHECK();
  }
  if (blocks > 4096) blocks = 4096;
  PPST_LAUNCH(linear_wgrad_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const float*)dy, (const float*)x, (float*)dw, B, N,
              K, scale, accumulate, total);
  return PPST_LAUNCH_CHECK();
}
extern "C" int ppst_linear_wgrad_fused(const void* dy, const void* x, void* dw, void* db, int B, int N, int K, float scale, float bscale,
                                       int accumulate, int b_accumulate, int relu_in, void* stream) {
  if (B <= 0 || N <= 0 || K <= 0 || K % 4) return PPST_EINVAL;
  if (!dy || !x || !dw) return PPST_ENULL;
  if (((uintptr_t)x | (uintptr_t)dw) % 16) return PPST_EINVAL;
  const int64_t total4 = (int64_t)N * K / 4;
  int64_t blocks = cdiv64(total4, 256);
  if (blocks > 8192) blocks = 8192;
  PPST_LAUNCH(linear_wgrad4_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const float*)dy, (const float4*)x,
              (float4*)dw, (float*)db, B, N, K / 4, scale, bscale, accumulate, b_accumulate, relu_in, total4);
  return PPST_LAUNCH_CHECK();
}
// the partial launches and the slice reduction behind both input-gradient entries (gate null: the plain one)
static int linear_dgrad_launch(const void* dy, const void* w, void* dx, void* ws, const void* gate, int B, int N, int K, float scale,
                               void* stream) {
  const int nsplit = cdiv(N, LDG_ROWS);
  for (int b0 = 0; b0 < B; b0 += LDG_BMAX)
    PPST_LAUNCH(linear_dgrad_partial_kernel, dim3(cdiv(K, 256), nsplit), dim3(256), 0, as_stream(stream), (const float*)dy, (const float*)w,
                (float*)ws, B, N, K, b0);
  const int64_t bk = (int64_t)B * K;
  int64_t blocks = cdiv64(bk, 256);
  if (blocks > 4096) blocks = 4096;
  PPST_LAUNCH(gate ? linear_dgrad_reduce_kernel<true> : linear_dgrad_reduce_kernel<false>, dim3((unsigned)blocks), dim3(256), 0,
              as_stream(stream), (const float*)ws, (const float*)gate, (float*)dx, nsplit, bk, scale);
  return PPST_LAUNCH_CHECK();
}
extern "C" int ppst_linear_dgrad_gate(const void* dy, const void* w, void* dx, void* ws, const void* gate, int B, int N, int K, float scale,
                                      void* stream) {
  if (B <= 0 || N <= 0 || K <= 0) return PPST_EINVAL;
  if (!dy || !w || !dx || !ws || !gate) return PPST_ENULL;
  return linear_dgrad_launch(dy, w, dx, ws, gate, B, N, K, scale, stream);
}
extern "C" int64_t ppst_linear_dgrad_ws(int B, int N, int K) { return (int64_t)cdiv(N, LDG_ROWS) * B * K * (int64_t)sizeof(float); }
extern "C" int ppst_linear_dgrad(const void* dy, const void* w, void* dx, void* ws, int B, int N, int K, float scale, void* stream) {
  if (B <= 0 || N <= 0 || K <= 0) return PPST_EINVAL;
  if (!dy || !w || !dx || !ws) return PPST_ENULL;
  return linear_dgrad_launch(dy, w, dx, ws, nullptr, B, N, K, scale, stream);
}

// ------------------------------------------------------------ loss / Adam ----
// LSGAN (models/networks/loss.py:11-18): loss = weight * mean((p - target)^2); grad[i] = weight * 2 (p_i - target) / n
__global__ void lsgan_kernel(const float* __restrict__ pred, float* __restrict__ loss, float* __restrict__ grad, int n, float target,
                             float weight) {
  __shared__ float sm[64];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) {
    float d = pred[i] - target;
    s += d * d;
    if (grad) grad[i] = weight * 2.f * d / (float)n;
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < 64; ++i) t += sm[i];
    loss[0] = weight * t / (float)n;
  }
}
extern "C" int ppst_lsgan(const void* pred, void* loss, void* grad, int n, float target, float weight, void* stream) {
  if (n <= 0) return PPST_EINVAL;
  if (!pred || !loss) return PPST_ENULL;
  PPST_LAUNCH(lsgan_kernel, dim3(1), dim3(64), 0, as_stream(stream), (const float*)pred, (float*)loss, (float*)grad, n, target, weight);
  return PPST_LAUNCH_CHECK();
}

// torch.nn.L1Loss() (mean |a - b|) * weight: block partial sums, then one double-precision finish.
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ partial,
                                                         int64_t n) {
  __shared__ float sm[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += fabsf(a[i] - b[i]);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
extern "C" int64_t ppst_l1_mean_ws(int64_t n) { int64_t b = cdiv64(n, 256 * 16); return (b > 1024 ? 1024 : (b < 1 ? 1 : b)) * (int64_t)sizeof(float); }
extern "C" int ppst_l1_mean(const void* a, const void* b, void* out, void* ws, int64_t n, float weight, void* stream) {
  if (n <= 0) return PPST_EINVAL;
  if (!a || !b || !out || !ws) return PPST_ENULL;
  int nblocks = (int)(ppst_l1_mean_ws(n) / sizeof(float));
  PPST_LAUNCH(l1_partial_kernel, dim3(nblocks), dim3(256), 0, as_stream(stream), (const float*)a, (const float*)b, (float*)ws, n);
  int e = PPST_LAUNCH_CHECK();
  if (e) return e;
  PPST_LAUNCH(sum_blocks_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const float*)ws, (float*)out, nblocks, (int64_t)1,
              weight / (float)n, 0);
  return PPST_LAUNCH_CHECK();
}

// rsclLoss.forward (networks/rscl.py:42-64) for n <= 64 query rows of dimension C: row i's logits are
// [ q_i . k_i | n current-batch entries, all -10 (the reference's eye(1) mask broadcasts over the whole block) |
//   q_i . queue[:, j], j < K | q_i . k0_j, j < n0 ] / T ; loss = mean_i( logsumexp_i - logit_i0 ).
// One 1024-thread block per row (rscl_common.h): thread = (negative column j, quarter of the C reduction), four
// independent accumulators -- round 1/2's 256-thread form walked 2048 dependent L2 loads per thread (0.5-0.7 ms per row).
#include "rscl_common.h"
__global__ __launch_bounds__(RS_T) void rscl_rows_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ k0,
                                                         const float* __restrict__ queue, float* __restrict__ row_loss, int n, int n0, int C,
                                                         int K, float invT) {
  __shared__ RsclShared sh;
  const int i = blockIdx.x, t = threadIdx.x;
  float s_pos, m, ssum;
  rscl_logits(q + (int64_t)i * C, k + (int64_t)i * C, k0, queue, n, n0, C, K, invT, sh, s_pos, m, ssum);
  if (t == 0) row_loss[i] = (logf(ssum) + m) - s_pos;
}
extern "C" int ppst_rscl_loss(const void* q, const void* k, const void* k0, const void* queue, void* out, void* ws, int n, int n0, int C,
                              int K, float nce_T, void* stream) {
  if (n <= 0 || n > 64 || n0 < 0 || C <= 0 || K <= 0 || K + n0 > 512 || nce_T <= 0.f) return PPST_EINVAL;
  if (!q || !k || !queue || !out || !ws || (n0 > 0 && !k0)) return PPST_ENULL;
  PPST_LAUNCH(rscl_rows_kernel, dim3(n), dim3(RS_T), 0, as_stream(stream), (const float*)q, (const float*)k, (const float*)k0,
              (const float*)queue, (float*)ws, n, n0, C, K, 1.0f / nce_T);
  int e = PPST_LAUNCH_CHECK();
  if (e) return e;
  PPST_LAUNCH(sum_blocks_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const float*)ws, (float*)out, n, (int64_t)1, 1.0f / (float)n, 0);
  return PPST_LAUNCH_CHECK();
}

// torch.optim.Adam step (no weight decay / amsgrad): m, v updated in place, p <- p - lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   int64_t n, float lr, float b1, float b2, float eps, float bc1, float sqrt_bc2) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float gi = g[i];
    float mi = m[i] * b1 + gi * (1.f - b1);
    float vi = v[i] * b2 + gi * gi * (1.f - b2);
    m[i] = mi;
    v[i] = vi;
    p[i] -= (lr / bc1) * (mi / (sqrtf(vi) / sqrt_bc2 + eps));
  }
}
extern "C" int ppst_adam_step(void* p, const void* g, void* m, void* v, int64_t n, float lr, float beta1, float beta2, float eps, int step,
                              void* stream) {
  if (n < 0 || step <= 0) return PPST_EINVAL;
  if (n == 0) return PPST_OK;
  if (!p || !g || !m || !v) return PPST_ENULL;
  float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  int64_t blocks = cdiv64(n, 256);
  if (blocks > 4096) blocks = 4096;
  PPST_LAUNCH(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (float*)p, (const float*)g, (float*)m, (float*)v, n, lr, beta1,
              beta2, eps, bc1, sqrtf(bc2));
  return PPST_LAUNCH_CHECK();
}
