/*
 * libppst_hip.so -- C ABI of the MI355X (gfx950) PPST hot path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes and an
 * explicit HIP stream, never throws and returns
 *      0            success
 *      > 0          a hipError_t from the launch
 *      < 0          PPST_E* argument error (nothing was launched)
 * so it can be bound from ctypes / cgo / JNI alike.  The library allocates nothing
 * and keeps no state between calls: every buffer, workspaces included, is the
 * caller's.  The only process-wide settings are opt-in diagnostics: the profiling
 * event pool of ppst_prof_* (it creates its events) with its side channel
 * ppst_wgrad_flop_steps, and the tuning aid ppst_guided_filter_tune.  Each declaration cites the
 * reference interface (file:line under wangxb29/PPST) it replaces.
 *
 * Grouped entry points (ppst_linear_grouped, ppst_l2norm_rows_grouped, ppst_lerp_grouped,
 * ppst_gap_gmp_multi_level): up to PPST_GROUP_MAX INDEPENDENT problems of one small op -- no
 * problem reads what another of the same call writes -- run as one launch (two for the pooling).
 * The problem table travels in the kernel arguments: nothing is uploaded, the array is the
 * caller's and is not kept.  Every problem runs the code of its single-problem entry point, so
 * its result is that call's, bit for bit.
 *
 * Tensor layouts: "NCHW" = the reference's contiguous torch layout;
 * "NHWC" = channels-last [B][H][W][C], the internal layout of the fused path.
 * All tensors are fp32 unless stated.  Activation tensors of the single-pass precision
 * modes may be stored as IEEE half / bfloat16: the `*_st` entry points and
 * ppst_conv_args.io_st take a storage type (PPST_ST_* below, the values of the PPST_F32 /
 * PPST_F16 / PPST_BF16 dtype enum); the `dtype` argument of ppst_upfirdn2d and
 * ppst_fused_bias_act takes the same three types (the reference's
 * AT_DISPATCH_FLOATING_TYPES_AND_HALF: upfirdn2d_kernel.cu:225, fused_bias_act_kernel.cu:79;
 * fp32 arithmetic, one rounding; the FIR taps stay fp32) and PPST_F64 (round 5: every tensor
 * of the call -- the FIR taps too -- is double and the arithmetic runs in double, scalar_t = double
 * in the reference's dispatch: what a gradcheck-style caller of the two ops hands over).
 */
#ifndef PPST_HIP_H
#define PPST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPST_OK 0
#define PPST_EINVAL (-1)      /* bad size / flag combination */
#define PPST_EUNSUPPORTED (-2) /* valid but not implemented (e.g. dtype) */
#define PPST_ENULL (-3)       /* null pointer where data is required */

enum { PPST_F32 = 0, PPST_F16 = 1, PPST_BF16 = 2, PPST_F64 = 3 /* ppst_upfirdn2d / ppst_fused_bias_act only */ };

/* padding modes of the fused conv (nn.ReflectionPad2d / ReplicationPad2d /
 * zero padding, stylegan2_layers.py:528-531, generator.py:13-17) */
enum { PPST_PAD_ZERO = 0, PPST_PAD_REFLECT = 1, PPST_PAD_REPLICATE = 2 };

/* epilogue activation of the fused conv */
enum { PPST_ACT_NONE = 0, PPST_ACT_LRELU = 1 /* lrelu(0.2)*sqrt2 */, PPST_ACT_PRELU = 2 };

/* ABI revision: bumped whenever a struct of this header changes size or an entry point changes its arguments.
 *   1: rounds 1-3;  2: round 4 (ppst_pack_job gained `dual` -- it is the element of the job ARRAY ppst_conv_pack_batch walks, so its
 *   stride changed --, ppst_conv_args gained dual_b / io_st / k64, PPST_F64 for the two native ops);  3: ppst_conv_args gained
 *   in_res / in_res_ld / ksplit / ksplit_starts (round 5) and the caller-owned K-split workspace ksplit_scratch / ksplit_flags /
 *   ksplit_epoch, and the K-split check entry point is gone (the caller reads the give-up marker of its own flag buffer).
 *   Callers must zero-initialise ppst_conv_args: a zero field is the "off" value of every later addition.  A binding built against
 *   another revision must refuse to run (ppst_amd/_lib.py does). */
#define PPST_ABI_VERSION 3
int ppst_version(void);

/* Storage type of an NHWC activation tensor at the entry points that take one (`*_st` twins and ppst_conv_args.io_st; round 4):
 * fp32, IEEE half or bfloat16.  A kernel given a half type computes in fp32 exactly as its fp32 form and rounds once, to nearest
 * even, when it stores: f_st(x_half) == round(f(float(x_half))).  Leading dimensions stay in ELEMENTS; half tensors must be 8-byte
 * aligned and have a channel count (and leading dimensions) divisible by 4.  Each `_st` twin with every type 0 IS its plain form. */
#define PPST_ST_F32 0   /* == PPST_F32 */
#define PPST_ST_F16 1   /* == PPST_F16 */
#define PPST_ST_BF16 2  /* == PPST_BF16 */

/* ---------------------------------------------------------------- ops ----
 * upfirdn2d_op.upfirdn2d(input[major,H,W,minor], kernel[kh,kw], up_x, up_y,
 * down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
 *   -- models/networks/stylegan2_op/upfirdn2d.cpp:4-23,
 *      upfirdn2d_kernel.cu:52-137 (kernel), :140-272 (dispatch).
 * y must hold major*out_h*out_w*minor floats with
 *   out_h = (in_h*up_y + pad_y0 + pad_y1 - kh + down_y) / down_y  (.cu:166).
 * minor=1 is the reference's NCHW use; minor=C, major=B is NHWC.
 * Any kh,kw <= 8 is supported (the reference silently launches nothing for
 * combinations outside its 6 modes, .cu:172-223).  The backward of the op is
 * the same entry with the flipped kernel and g_pad (upfirdn2d.py:116-121). */
int ppst_upfirdn2d(const void* x, const void* k, void* y,
                   int major, int in_h, int in_w, int minor, int kh, int kw,
                   int up_x, int up_y, int down_x, int down_y,
                   int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                   int dtype, void* stream);

/* Fused-path Blur on NHWC activations (Blur inside ConvLayer(downsample=True),
 * stylegan2_layers.py:142-164,513-520): square FIR (ksize 3 or 4), pad (pad0 before,
 * pad1 after) with zero or reflection padding folded in (the reference runs
 * nn.ReflectionPad2d first, :151-159); down=2 keeps every second sample (all that a
 * following stride-2 1x1 conv reads); s2d=1 writes the output space-to-depth
 * y[B][ceil(oh/2)][ceil(ow/2)][4*C] (phase (oy&1)*2+(ox&1) major) for the stride-2
 * 3x3 conv that ppst_conv2d_mfma runs as a stride-1 conv over that layout (the padded
 * extent is written in full: zeros beyond (oh, ow), so y needs no initialisation).
 * in_scale_shift (optional, [B][C][2] (a, s)) + in_act (PPST_ACT_NONE / PPST_ACT_LRELU):
 * the input is read as in_act(a*x + s) -- the InstanceNorm + FusedLeakyReLU that
 * ConvLayer(norm='in') puts in front of the Blur (:542-549) without a pass of its own;
 * zero-padding positions stay 0.  x and y: 16-byte aligned in fp32, 8-byte aligned in a
 * half type, or PPST_EINVAL -- there is no one-channel form behind this entry. */
int ppst_blur_nhwc(const void* x, const void* k, void* y, int B, int in_h, int in_w, int C,
                   int ksize, int pad0, int pad1, int pad_mode, int down, int s2d,
                   const void* in_scale_shift, int in_act, void* stream);
int ppst_blur_nhwc_st(const void* x, const void* k, void* y, int B, int in_h, int in_w, int C,
                      int ksize, int pad0, int pad1, int pad_mode, int down, int s2d,
                      const void* in_scale_shift, int in_act, int st /* of x and y */, void* stream);

/* fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)
 *   -- stylegan2_op/fused_bias_act.cpp:4-20, fused_bias_act_kernel.cu:19-49.
 * y[i] = f(x[i] + b[(i/step_b) % size_b]) * scale; b==NULL => no bias,
 * ref==NULL => no reference.  act: 1 linear, 3 leaky-relu; grad: 0 forward,
 * 1 first derivative gated by sign(ref), 2 second derivative (= 0). */
int ppst_fused_bias_act(const void* x, const void* b, const void* ref, void* y,
                        int64_t n, int step_b, int size_b, int act, int grad,
                        float alpha, float scale, int dtype, void* stream);

/* -------------------------------------------------------------- layout --- */
int ppst_nchw_to_nhwc(const void* x, void* y, int B, int C, int H, int W, void* stream);
int ppst_nhwc_to_nchw(const void* x, void* y, int B, int C, int H, int W, void* stream);

/* ---------------------------------------------------- fused conv (MFMA) ---
 * Implicit-GEMM convolution on NHWC fp32 activations with bf16 MFMA
 * (v_mfma_f32_16x16x32_bf16).  precision 0: every fp32 operand is split into
 * hi+lo bf16 and 3 MFMAs (hi*hi, hi*lo, lo*hi) accumulate in fp32 ("bf16x3",
 * fp32-class, relative error ~1e-5); precision 1: single bf16 pass.
 * Replaces F.conv2d / F.conv_transpose2d inside EqualConv2d
 * (stylegan2_layers.py:184-193), EqualizedConv2d (:305-347, incl. the fused
 * 4x4 stride-2 transposed-conv upscale :312-321) and nn.Conv2d of the
 * generator heads (generator.py:174-238), with the StyledConv epilogue
 * (stylegan2_layers.py:467-475) fused in.
 *
 * The convolution is described by a packed-weight blob + step table built by
 * ppst_conv_pack (one-time per weight tensor). */

typedef struct ppst_conv_step {
  int32_t chan_off;   /* first input channel (in the in_ld-strided pixel) of this 32-ch chunk */
  int32_t dy, dx;     /* tap offset relative to the output pixel, each in [-1,1] */
  int32_t new_chunk;  /* 1 if this step starts a new input chunk (LDS restage) */
} ppst_conv_step;

/* Pack one weight tensor for ppst_conv2d_mfma (one-time per weight tensor).
 *  w        fp32 weights; element (n, c, ky, kx) at w[n*sn + c*sc + ky*sy + kx*sx]
 *  scale    multiplied in (EqualConv2d runtime scale, stylegan2_layers.py:177)
 *  src_*    DEVICE int32 arrays [n_groups*nsteps]: the K-slice of step s of group g is
 *           w[n][src_c .. src_c+31][src_ky][src_kx]
 *  bn       64, 128 or 256 = N tile of the kernel variant that will consume the blob
 *  out      n_groups * ceil(cout/bn) * nsteps * (precision==0 ? 8 : 4) * bn * 8 bf16 */
/* The same for ppst_conv_args.dual_b: bn = 256 = two column phases x 128 channels of N tile t (channels 128 t ..); src_kx[i] holds
 * (kx of phase 0) | (kx of phase 1) << 8.  out: n_groups * ceil(cout/128) * nsteps * (precision==0 ? 8 : 4) * 256 * 8 bf16. */
/* Weights for ppst_conv_args.variant 11 (the fused upscale of stylegan2_layers.py:312-321 as the UN-BLURRED 3x3 stride-2
 * transposed conv -- nine products per input pixel instead of the sixteen of the 4x4 kernel -- with the 2x2 box sum of the weight
 * blur applied to the OUTPUT in the kernel's epilogue): w = the layer's 3x3 weight (Cout, Cin, 3, 3) with element strides
 * sn / sc / sy / sx, scaled by ``scale``; cout % 64 == 0, cin % 32 == 0; out: ppst_conv_pack_up9_bytes(cout, cin) bytes. */
int64_t ppst_conv_pack_up9_bytes(int cout, int cin);
int ppst_conv_pack_up9(const void* w, int64_t sn, int64_t sc, int64_t sy, int64_t sx, float scale, int cout, int cin,
                       void* out, void* stream);
/* Weights for ppst_conv_args.k64: as ppst_conv_pack (dual = 0) / ppst_conv_pack_dual (dual = 1) with precision 1 / 3, but step i of
 * the table covers channels src_c[i] .. src_c[i] + 63; out: n_groups * n_tiles * nsteps * 8 * bn * 8 elements of the operand type. */
int ppst_conv_pack_k64(const void* w, int64_t sn, int64_t sc, int64_t sy, int64_t sx, float scale, int cout, int bn,
                       const int32_t* src_c, const int32_t* src_ky, const int32_t* src_kx, int nsteps, int n_groups,
                       int precision, int dual, void* out, void* stream);
int ppst_conv_pack_dual(const void* w, int64_t sn, int64_t sc, int64_t sy, int64_t sx, float scale, int cout,
                        const int32_t* src_c, const int32_t* src_ky, const int32_t* src_kx, int nsteps, int n_groups,
                        int precision, void* out, void* stream);
int ppst_conv_pack(const void* w, int64_t sn, int64_t sc, int64_t sy, int64_t sx,
                   float scale, int cout, int bn,
                   const int32_t* src_c, const int32_t* src_ky, const int32_t* src_kx,
                   int nsteps, int n_groups, int precision, void* out, void* stream);
/* Batched forms (training: every plan of a network is re-packed after each Adam step -- one launch instead of one per plan).
 * ``jobs`` is a DEVICE array; the caller fills block0 / nblocks: consecutive block ranges, nblocks = ppst_pack_job_blocks(total),
 * total_blocks = their sum.  Field meaning as the arguments of ppst_conv_pack / ppst_upscale_weight. */
typedef struct ppst_pack_job {
  const void* w;
  int64_t sn, sc, sy, sx;
  const int32_t* src_c;
  const int32_t* src_ky;
  const int32_t* src_kx;
  void* out;
  int64_t total;              /* n_groups * ceil(cout / bn) * nsteps * 4 * bn */
  int64_t block0;
  float scale;
  int32_t cout, bn, nsteps, n_groups, x3, f16, nblocks;   /* x3: precision 0 (hi + lo planes); f16: precision 3 */
  int32_t dual;               /* 1: ppst_conv_pack_dual semantics (the N tile holds two output column phases) */
                              /* (x3 = 2 with f16 = 0 / 1: ppst_conv_pack_k64 semantics -- the lo planes hold channels 32-63 of a 64-channel step) */
} ppst_pack_job;
typedef struct ppst_upscale_job {
  const void* w;
  void* out;
  int64_t total, block0;      /* total = cin * cout * 16 */
  float scale;
  int32_t cout, cin, nblocks;
} ppst_upscale_job;
int ppst_pack_job_blocks(int64_t total);
int ppst_conv_pack_batch(const void* jobs, int njobs, int total_blocks, void* stream);
int ppst_upscale_weight_batch(const void* jobs, int njobs, int total_blocks, void* stream);

/* EqualizedConv2d fused-upscale weight (stylegan2_layers.py:314-319):
 * w (Cout,Cin,3,3)*scale -> out (Cin,Cout,4,4), the F.conv_transpose2d operand */
int ppst_upscale_weight(const void* w, void* out, int cout, int cin, float scale, void* stream);
/* Round 5: the input gradient of the stride-2 3x3 conv (stylegan2_layers.py:497-555, ConvLayer(downsample=True)) as ONE stride-1 conv
 * with 2 x 2 taps whose 4 x cin output channels stack the four output phases -- out (4*cin, cout, 2, 2) from the forward weight w
 * (cout, cin, 3, 3): out[(py*2+px)*cin + n][c][ty][tx] = w[c][n][ky][kx], a phase p using tap offset 0 with k = (p == 0 ? 0 : 1) and
 * offset 1 (one position back) with k = 2 when p == 0; zero elsewhere.  The stacked output goes through ppst_depth_to_space_st.  For
 * thin layers (cin 32 / 64) the four-group scattered form ran 2 312-5 780 four-wave blocks that each staged the same tile. */
int ppst_dgrad_s2d_stack_weight(const void* w, void* out, int cout, int cin, void* stream);
/* x [B][th][tw][4 C] (channel block py*2+px = output phase) -> y [B][oh][ow][C], y[b][2q+py][2p+px][c] = x[b][q][p][(py*2+px)*C + c];
 * oh <= 2 th, ow <= 2 tw; st = PPST_ST_* of both tensors (C % 4 == 0 fp32, % 8 half; 16-byte aligned). */
int ppst_depth_to_space_st(const void* x, void* y, int B, int th, int tw, int oh, int ow, int C, int st, void* stream);

/* sizes of the caller-owned K-split workspace of ppst_conv_args (ksplit_scratch in bytes, ksplit_flags in 32-bit words):
 * 256 producer blocks x 512 threads x 128 accumulator registers (512 blocks of the tile kernel's 64) */
#define PPST_KSPLIT_SCRATCH_BYTES ((size_t)256 * 512 * 128 * 4)
#define PPST_KSPLIT_FLAG_WORDS 4096

typedef struct ppst_conv_args {
  const void* x;        /* NHWC fp32 input, pixel stride in_ld floats */
  const void* wpack;    /* from ppst_conv_pack */
  const void* steps;    /* device array ppst_conv_step[n_groups*nsteps + 4]: 4 padding entries at the end (the kernel
                           prefetches the descriptor of step s+3 without a bounds test; their content is ignored) */
  void* y;              /* NHWC fp32 output, pixel stride out_ld floats; one image (out_h * out_w * out_ld, and the same with
                           res_ld) must stay below 2^31 elements: the epilogues address inside an image with 32-bit offsets */
  const void* bias;     /* [cout] or NULL (sum of all per-channel biases) */
  const void* noise;    /* [B][out_h][out_w] or NULL (NoiseInjection, stylegan2_layers.py:376-399) */
  const void* prelu;    /* [1] PReLU slope (device) when act == PPST_ACT_PRELU */
  void* stats;          /* [B][tiles_per_image][cout][2] per-tile (sum, sumsq) of the stored output, or NULL */
  const void* residual; /* NHWC fp32 [B][out_h][out_w][res_ld] added before act, or NULL */
  float noise_weight;
  float out_scale;      /* multiplies the activated output (1.0 default) */
  int32_t B, in_h, in_w, in_ld;
  int32_t out_h, out_w, out_ld, cout;
  int32_t nsteps, n_groups;      /* n_groups: 1, or 4 output phases (transposed conv) */
  int32_t pad_mode;              /* PPST_PAD_* applied to out-of-image taps */
  int32_t in_off_y, in_off_x;    /* input pixel = tile pixel + tap + in_off (e.g. -pad) */
  int32_t out_sy, out_sx;        /* output pixel stride (2 for the transposed conv) ... */
  int32_t act;                   /* PPST_ACT_* | 0x100: residual joins AFTER the activation */
  int32_t precision;             /* 0 bf16x3 (fp32-class), 1 bf16 single pass, 3 fp16 single pass; ppst_conv_pack with the
                                    same value */
  int32_t res_ld;
  int32_t tile_h, tile_w;        /* logical (pre-scatter) output extent tiled by 16x16 */
  int32_t halo;                  /* 0: every tap is (0,0) (1x1 conv); 1: taps in [-1,1]^2 */
  int32_t bn;                    /* N tile the weights were packed for (64 or 128) */
  const void* in_scale_shift;    /* optional [B][in_c][2] (a, s): the input is read as in_act(a*x + s) --
                                    "normalise on load" of the producer's InstanceNorm/StyleMod/activation; padding
                                    positions stay 0 (they pad the normalised tensor).  NULL: input used as is */
  const void* in_prelu;          /* [1] slope when in_act == PPST_ACT_PRELU */
  int32_t in_c, in_act;          /* channel count of the in_scale_shift table; PPST_ACT_* */
  int32_t flop_steps;            /* steps that carry real weights (profiling only; 0 = nsteps) */
  int32_t tile_rows;             /* (32 only with variant 7, 24 only with variant 9) 16: 16x16-pixel tiles, 512- (bn 128) / 256-thread blocks, 1 block per CU;
                                    8:  8x16-pixel tiles, 256-thread blocks, 2 blocks per CU, a two-slot activation ring: variant 0,
                                    bn 128, halo 1, precision 0 and the early_a promise (chunks of >= 2 steps).  Bit-identical
                                    outputs; for launches whose 16-row grid would under-fill the chip */
  int32_t a_slots;               /* depth of the activation-tile ring in LDS: 0 = default (3).  1 or 2 may be given when
                                    NO group of the step table has more chunks (steps with new_chunk = 1) than that:
                                    with bn = 64 the smaller footprint lets two blocks share a CU (small-K layers are
                                    latency/HBM-bound with one).  The caller owns this promise: the table is on the
                                    device and is not re-read by the host. */
  int32_t early_a;               /* 1: every chunk of the step table spans >= 2 steps AND steps[i].w carries, besides bit 0
                                    (step i opens a chunk), bit 1 = step i+1 opens a chunk and bits 8.. = that chunk's
                                    channel offset: the kernel then requests a chunk's activations one step earlier
                                    (HBM latency no longer stalls the staging store).  0: bits 1.. are ignored. */
  int32_t variant;               /* 0: the 8-wave kernel (512 threads, wave tile 64 px x 64 ch; bn 64 / 128).
                                    1, 3, 8: retired numbers (forms that were measured, lost and removed: DESIGN.md section 4);
                                    not reused, PPST_EINVAL.
                                    2: conv_mfma2.hip -- 8 waves x (128 px x 64 ch), bn = 256 (the production kernel for
                                    Cout % 256 == 0); its activation ring has two slots: every chunk of the step table must
                                    span >= 2 steps (the early_a promise).
                                    4 / 5 / 6 (conv1x1.hip, precision 0, one group, unit output stride, no in_off):
                                    4: all taps (0,0) (halo 0), bn = 64, in and out extents equal;
                                    5: any taps in [-1,1]^2, bn = 64;
                                    6: plain 3x3 stride-1 tables only -- nsteps = 9 * chunks and step 9c + 3(dy+1) + (dx+1)
                                       is tap (dy, dx) of chunk c; bn = 64, or 128 for Cout in 65..128.  The table lives on
                                       the device and is not re-read: the CALLER owns this promise (as with a_slots).
                                    7: conv_mfma2.hip with 8 waves as 4 (M) x 2 (N): block tile 32 x 16 px x 128 ch, two
                                       activation slots; bn = 128, tile_rows = 32, halo 1, the early_a promise, precision 1 / 3 only
                                       (the Cout = 128-class layers of the single-pass modes; precision 0: PPST_EINVAL).
                                    10: conv_wino.hip -- plain 3x3 stride-1 tables only (the variant-6 promise: nsteps = 9 * chunks,
                                       steps[9c].x = first channel of chunk c), wpack from ppst_conv_pack_wino, bn = 128,
                                       tile_rows = 16, one group, unit strides, precision 0.  Winograd F(2,3) along x: fp32-class
                                       like the others (<= 3e-5 against float64) but NOT bit-identical to them.
                                   11: conv_mfma2.hip "UP9" -- the fused 4x4 stride-2 upscale computed as the un-blurred 3x3 transposed
                                       conv (u types ee / eo / oe / oo of 4 / 2 / 2 / 1 taps: 9 products per input pixel instead of
                                       16) whose 2x2 box sum runs in the epilogue; bn = 256 = 4 N-waves x 4 types x 16 channels,
                                       n_groups 1, tile_rows 15 (blocks of 15 x 15 input positions: the 16 x 16 grid of a block
                                       feeds its neighbours' row / column), halo 1, zero padding, out_sy = out_sx = 2, precision
                                       0, no normalise-on-load / residual / PReLU; wpack from ppst_conv_pack_up9, steps = per
                                       32-channel chunk the shifts (0,0), (-1,0), (0,-1), (-1,-1).  fp32-class (<= 3e-5 against
                                       float64), NOT bit-identical to the 4x4 forms (other summation order).
                                    9: conv_mfma2.hip with 6 m-tiles per wave: block tile 24 x 16 px x 128 ch (wave tile 96 px x 64 ch),
                                       TWO activation slots; bn = 128, tile_rows = 24, the early_a promise, with k64 only
                                       (precision 1 / 3, io_st != 0: the Cout = 128-class layers of the single-pass modes on
                                       half-stored activations; without k64: PPST_EINVAL).
                                    Variants 0, 2, 4-7 and 9 give bit-identical outputs; the per-tile statistics differ in the last
                                    bit between variants (other summation tree).  The library returns PPST_EINVAL for a
                                    variant whose shape conditions do not hold. */
  int32_t reserved0;             /* must be 0 (PPST_EINVAL otherwise): the slot of a removed experiment, kept so that the fields
                                    behind it stay where they are */
  int32_t dual_b;                /* 1 (variant 2, bn 256, n_groups 2, halo 1, precision 0 / 1 / 3, out_sy = out_sx = 2): the fused 4x4 stride-2
                                    upscale (stylegan2_layers.py:312-321) with Cout % 128 == 0 as TWO row phases whose N tile of 256
                                    is [column phase 0: 128 channels | column phase 1: 128 channels] -- wpack from
                                    ppst_conv_pack_dual, steps[i].dx = (dx of phase 0 + 1) | (dx of phase 1 + 1) << 8.  The
                                    activation tile is staged once for two phases and the layer runs on the 128 x 64 wave
                                    tiles; outputs bit-identical to the four-group form, stats [B][4 * tiles][cout][2] as there. */
  int32_t io_st;                 /* storage type of x, residual and y (PPST_ST_*): 0 fp32; PPST_ST_F16 with precision 3 / PPST_ST_BF16
                                    with precision 1 only -- "half-precision activation storage": the generator / encoder activations
                                    of the fp16 and bf16 modes (BASELINE configs[4] / [3]) live in HBM in the operand type of the mode.
                                    Accumulation, bias / noise / activation, the instance-norm statistics and (a, s) of
                                    normalise-on-load stay fp32; the output is rounded once, to nearest even, at the store.
                                    variant 0 (tile_rows 16), 2, 4, 5, 6; pointers 8-byte aligned; in_ld / out_ld / res_ld in ELEMENTS. */
  int32_t k64;                   /* 1 (io_st != 0, precision 1 / 3, halo 1, variant 2 [also with dual_b] or variant 9 with tile_rows 24):
                                    a step of the table covers SIXTY-FOUR input channels (steps[i].chan .. + 63; wpack from
                                    ppst_conv_pack_k64: channels 0-31 of the chunk where the fp32-class blob keeps its hi planes,
                                    32-63 where it keeps its lo planes) -- half the steps per MFMA of the 32-channel single-pass
                                    form.  Outputs equal that form's up to fp32 summation order (the two halves of a chunk are
                                    accumulated alternately instead of chunk after chunk). */
  const void* in_res;            /* round 5, variant 4 with in_scale_shift only: a second input tensor of the conv's own extent and
                                    channel count, added BEFORE in_act -- the input is read as in_act(a*x + s + in_res): the resnet
                                    merge of generator.py:28-31 (prelu(IN(conv2) + x)) applied while the 1x1 conv that is its only
                                    consumer loads its fragments, so the merged tensor is never written (layert1 -> layert1.1).
                                    Same fp32 operations in the same order as ppst_affine_act(res_before_act) followed by the plain
                                    conv (the test holds the pair to 2e-6 of each other).  fp32 storage, precision 0; NULL: none */
  int32_t in_res_ld;             /* pixel stride of in_res in elements */
  int32_t ksplit;                /* round 5: 0 / 1 none; S = 2, 4 or 8 (variant 0, 2 or 10; S = 8 on variant 0 only: the other two hold 128
                                    accumulator registers per thread; nsteps % S == 0 and -- the CALLER's promise -- step
                                    i * nsteps / S opens a chunk for every i): the reduction is split over S blocks per output
                                    tile (grid y), each running nsteps / S steps of the table; the first S - 1 leave their raw
                                    accumulators in ksplit_scratch and raise a flag in ksplit_flags, the last block of the tile
                                    (dispatched behind them) adds them in a fixed order and runs the epilogue.  For launches whose
                                    grid fills a fraction of the chip and whose blocks are one long serial chain of steps (the
                                    64^2 ... 4^2 layers of a train step at batch 2: 4-128 blocks, 72-160 steps): S x the blocks,
                                    1 / S of the chain.  Results equal the unsplit launch's up to fp32 summation order.  At most
                                    256 (S - 1) x tiles per launch. */
  const int32_t* ksplit_starts;  /* HOST pointer to ksplit + 1 ascending step indices, starts[0] = 0, starts[ksplit] = nsteps, every one of
                                    them a step that opens a chunk (the caller's promise): block row i runs steps
                                    [starts[i], starts[i + 1]) -- tables whose chunks differ in length (the stride-2 conv on a
                                    space-to-depth tensor: 4 / 2 / 2 / 2 taps per phase).  NULL: equal shares of nsteps / ksplit
                                    steps.  Read during the call, not kept. */
  /* The K-split workspace (ksplit > 1; ignored otherwise) belongs to the CALLER, like every other buffer:
   *  - ksplit_scratch: PPST_KSPLIT_SCRATCH_BYTES bytes of device memory (the hand-over of the partial sums);
   *  - ksplit_flags: PPST_KSPLIT_FLAG_WORDS 32-bit words of device memory, zero-filled once when it is allocated;
   *  - one workspace never serves two launches that can run at the same time: in practice one workspace per stream;
   *  - ksplit_epoch: non-zero, and different from the epoch of the previous launch on the same workspace (a flag left by an
   *    earlier launch is then stale without a fill between launches) -- a counter that skips 0 when it wraps;
   *  - word PPST_KSPLIT_FLAG_WORDS - 1 of ksplit_flags is the give-up marker: non-zero after a block of a launch stopped waiting
   *    for its partner blocks (that launch's output is wrong; cannot happen while blocks are dispatched in grid order).  The
   *    caller reads it after synchronising the stream, and resets it to zero.
   * A NULL buffer returns PPST_ENULL, epoch 0 PPST_EINVAL. */
  void* ksplit_scratch;
  unsigned* ksplit_flags;
  uint32_t ksplit_epoch;
} ppst_conv_args;

int ppst_conv2d_mfma(const ppst_conv_args* a, void* stream);
/* Weights of a plain 3x3 stride-1 conv for ppst_conv_args.variant 10 (conv_wino.hip: Winograd F(2,3) along x, direct along y --
 * 12 K-steps per 32-channel chunk and pixel PAIR instead of 9 per pixel, 1.5x fewer MFMAs; EqualConv2d / StyledConv conv,
 * stylegan2_layers.py:184-193, 275-348, 439-475).  Element (n, c, ky, kx) of the kernel at w[n*sn + c*sc + ky*sy + kx*sx] (any
 * strides: the input-gradient plan passes the transposed, flipped view of the same tensor), scaled by ``scale``; the row
 * transform U = (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2) is formed in double and stored as bf16 hi + lo in the register-fragment
 * order of the kernel's waves: [Cout/128][4 positions][2 channel halves][Cin/32][3 ky][4 n-tiles][hi|lo][64 lanes][8 k].
 * cin % 32 == 0; ``out`` holds ppst_conv_pack_wino_bytes(cout, cin) bytes. */
int64_t ppst_conv_pack_wino_bytes(int cout, int cin);
int ppst_conv_pack_wino(const void* w, int64_t sn, int64_t sc, int64_t sy, int64_t sx, float scale, int cout, int cin,
                        void* out, void* stream);
/* Exact-fp32 twin of ppst_conv2d_mfma (v_mfma_f32_32x32x2_f32; a->wpack, bn, precision, a_slots, early_a are ignored):
 * same step table / padding / epilogue semantics, weights read from the fp32 tensor itself -- element (n, c, ky, kx) at
 * w[n*sn + c*sc + ky*sy + kx*sx], step s of group g uses w[n][src_c .. src_c+31][src_ky][src_kx] * wscale (src_c < 0:
 * zero-weight step).  A verification path (10-30x slower): it tells rounding of the bf16 hi+lo split apart from defects. */
int ppst_conv2d_f32(const ppst_conv_args* a, const void* w, int64_t sn, int64_t sc, int64_t sy, int64_t sx, float wscale,
                    const int32_t* src_c, const int32_t* src_ky, const int32_t* src_kx, void* stream);
/* number of tile_rows x 16 tiles per image for (tile_h, tile_w) -- size of the stats buffer */
int ppst_conv_tiles(int tile_h, int tile_w, int tile_rows);

/* FromRGB-type conv: 1x1, Cin <= 4 (HBM-bound), NHWC in (in_ld) -> NHWC out, fused
 * bias + leaky relu (ConvLayer(3, C, 1), stylegan2_layers.py:497-555). */
int ppst_conv1x1_small_cin(const void* x, const void* w, const void* bias, void* y,
                           int64_t npix, int cin, int in_ld, int cout, float wscale,
                           int act, void* stream);
int ppst_conv1x1_small_cin_st(const void* x, const void* w, const void* bias, void* y,
                              int64_t npix, int cin, int in_ld, int cout, float wscale,
                              int act, int y_st /* x stays fp32: the image */, void* stream);
/* the same conv reading the NCHW image x [B][cin][hw] itself (no layout pass in front): the same products in the same order */
int ppst_conv1x1_small_cin_nchw_st(const void* x, const void* w, const void* bias, void* y, int B, int64_t hw, int cin, int cout,
                                   float wscale, int act, int y_st, void* stream);
/* ToRGB-type conv: 1x1, Cout <= 4 (stylegan2_layers.py:487-489); y NHWC [npix][cout] */
int ppst_conv1x1_small_cout(const void* x, const void* w, const void* bias, void* y,
                            int64_t npix, int cin, int cout, float wscale, void* stream);
int ppst_conv1x1_small_cout_st(const void* x, const void* w, const void* bias, void* y,
                               int64_t npix, int cin, int cout, float wscale, int x_st /* y stays fp32 */, void* stream);
/* the same with a pixel stride in_ld (>= cin, % 4 == 0) of x: a channel slice of a wider tensor is read in place */
int ppst_conv1x1_small_cout_ld_st(const void* x, const void* w, const void* bias, void* y, int64_t npix, int cin, int in_ld, int cout,
                                  float wscale, int x_st, void* stream);
/* ToRGB's 1x1 conv (stylegan2_layers.py:477-495, Cout = 3) reading the merge of the block in front of it,
 *   (a[b][c] * x + s[b][c] + bilinear_x2(res)) * out_scale      (IN + StyleMod of conv2 + the x2-upsampled skip, / sqrt2:
 * the last UpsamplingResnetBlock, generator.py:63-78, whose only consumer in the image pass is this conv), by linearity: the skip's
 * share is proj = ppst_conv1x1_small_cout_ld_st(res, w, no bias, scale wscale * out_scale), [B][H/2][W/2][3] fp32, sampled x2-bilinearly
 * where the three outputs are stored; the 128-channel merge is never formed.
 * x [B][H][W][cin] dense (storage type x_st), scale_shift [B][cin][2] or NULL (a = 1, s = 0), proj or NULL, w [3][cin], bias [3] or
 * NULL -> y [B][H][W][3] fp32; partial != NULL: also the instance-norm partials of y, [B][*n_partials][3][2] as ppst_in_finalize
 * reads them.  x == y == NULL: size query (*n_partials only).  Equal to ppst_affine_act (res_up2) followed by
 * ppst_conv1x1_small_cout up to the order of one sum.  (Replaces ppst_torgb_apply_st, which sampled res per channel of every pixel.) */
int ppst_torgb_linear_st(const void* x, const void* scale_shift, const void* proj, float out_scale, const void* w, const void* bias,
                        void* y, void* partial, int* n_partials, int B, int H, int W, int cin, float wscale, int x_st, void* stream);
/* ToRGB's end: out [B][3][hw] (NCHW) = a * y + s of y [B][hw][3], scale_shift [B][3][2]: ppst_affine_act then ppst_nhwc_to_nchw */
int ppst_rgb_affine_nchw(const void* y, const void* scale_shift, void* out, int B, int64_t hw, void* stream);
/* The encoders' first ResBlock without norm (stylegan2_layers.py:552-579, reflection_pad) in one launch, every intermediate in LDS:
 *   y = (lrelu(conv2(blur(lrelu(conv1(x) + b1))) + b2) + skip(blur_down2(x))) / sqrt 2,  lrelu(t) = sqrt 2 * max(t, 0.2 t);
 * conv1 3x3 reflect pad 1, blur = the 3x3 FIR `blur` (9 floats, as ppst_upfirdn2d takes it) with reflect pad (2, 1), conv2 3x3
 * stride 2 on that extent, skip = `blur` with zero pad (1, 0) keeping every second sample, then the 1x1 conv.
 * fp32 storage, precision mode 0 (bf16 hi + lo, three MFMAs per product), channels 32 -> 32 -> 64 only.
 * x [B][H][W][32] dense (x_ld = 32 = its pixel stride, x_st = PPST_ST_F32), H and W even and >= 4 -> y [B][H/2][W/2][64].
 * w1, w2, ws: the ppst_conv_pack blobs (bn = 64, precision 0, scale folded in) of the (32,32,3,3), (64,32,3,3) and (64,32,1,1)
 * weights under the plain conv step table (one step per tap, ky-major); b1 [32], b2 [64].  x, y and the blobs 16-byte aligned.
 * Anything else is PPST_EINVAL: the caller keeps such inputs on the unfused path.  Equal to that path up to the order of conv2's
 * nine-tap sum. */
int ppst_encoder_resblock(const void* x, int x_st, int B, int H, int W, int cin, int cmid, int cout, int x_ld, const void* w1, const void* w2,
                          const void* ws, const void* b1, const void* b2, const void* blur, void* y, void* stream);

/* ------------------------------------------- instance norm / style mod ---
 * nn.InstanceNorm2d (eps 1e-5, biased var) + StyleMod (stylegan2_layers.py:361-374,
 * :414-437).  Statistics come either from the conv epilogue partials or from
 * ppst_in_stats (optionally weighting the border as if the tensor had been
 * ReplicationPad2d(1)-padded first: generator.py:175-176). */
int ppst_in_stats(const void* x, void* partial, int B, int H, int W, int C, int ld,
                  int rep_pad, int* n_partials, void* stream);
/* reduce partials -> per (b,c) scale a and shift s with  y = a*x + s:
 *   a = rstd * (style0+1), s = style1 - mean*a   (style==NULL: a=rstd, s=-mean*rstd)
 * style: [B][style_ld] rows whose first 2*C entries are the StyleMod linear output.
 * count = #elements per (b,c). */
int ppst_in_finalize(const void* partial, int n_partials, const void* style,
                     int style_ld /* row stride of style (>= 2C): slices of a batched StyleMod GEMV */,
                     const void* post_bias /* [C] added to the shift, or NULL */,
                     void* scale_shift /* [B][C][2] */, int B, int C, double count,
                     float eps, void* stream);
/* y = act(a*x + s [+ res]) * out_scale ; (skip + res)/sqrt2 of the resnet blocks
 * (generator.py:47-78) is res + out_scale. act as PPST_ACT_*; PReLU slope ptr. */
int ppst_affine_act(const void* x, const void* scale_shift, const void* res,
                    const void* res_scale_shift /* optional affine of res */, void* y,
                    int B, int64_t hw, int C, int x_ld, int res_ld, int y_ld,
                    int act /* | 0x100: res joins before act */, const void* prelu,
                    float out_scale,
                    int res_up2_w /* >0: res is a HALF-resolution tensor, upsampled x2 bilinearly on the
                                     fly (resnet skip, generator.py:75); value = output width W.  Vector
                                     forms only: C and every ld multiples of 4, x / res / y 16-byte aligned
                                     (8 with a half type), else PPST_EINVAL */,
                    void* stream);
/* x_st: storage of x and res; y_st: of y (either may be fp32 beside a half type; two different half types are refused) */
int ppst_affine_act_st(const void* x, const void* scale_shift, const void* res, const void* res_scale_shift, void* y,
                       int B, int64_t hw, int C, int x_ld, int res_ld, int y_ld, int act, const void* prelu,
                       float out_scale, int res_up2_w, int x_st, int y_st, void* stream);
/* ppst_affine_act that also emits the instance-norm partials of its OUTPUT (the layout
 * ppst_in_stats produces for (H, W); rep_pad as there), so the norm that follows needs no
 * read pass of its own.  C % 4 == 0. */
int ppst_affine_act_stats(const void* x, const void* scale_shift, const void* res,
                          const void* res_scale_shift, void* y, void* partial,
                          int B, int H, int W, int C, int x_ld, int res_ld, int y_ld,
                          int act, const void* prelu, float out_scale, int rep_pad,
                          int res_up2 /* as res_up2_w, boolean */, void* stream);
/* nearest x2 upsample NHWC (Upscale2d, stylegan2_layers.py:86-97) */
int ppst_upsample_nearest2(const void* x, void* y, int B, int H, int W, int C, void* stream);
int ppst_upsample_nearest2_st(const void* x, void* y, int B, int H, int W, int C, int st, void* stream); /* C % 8 == 0 for half */

/* ------------------------------------------------- pooling / resizing ---- */
/* GAP + GMP over HxW per (b,c): out [B][2C] = cat(mean, max)  (encoder_col.py:159-161).
 * mask: optional [B][H][W] multiplier (mask channel i of encoder_col.py:176-178). */
int64_t ppst_gap_gmp_ws(int B, int64_t hw, int C); /* workspace bytes */
int ppst_gap_gmp(const void* x, const void* mask, void* out, void* ws, int B, int H, int W,
                 int C, int ld, void* stream);
int ppst_gap_gmp_st(const void* x, const void* mask, void* out, void* ws, int B, int H, int W,
                    int C, int ld, int x_st, void* stream);
/* Grouped calls take at most this many problems; more: PPST_EINVAL, 0: PPST_OK without a launch. */
#define PPST_GROUP_MAX 32
/* ppst_gap_gmp_st of n feature maps of one batch (the four pyramid levels of an E2 pass, encoder_col.py:159-161, plain / warped /
 * masked) as ONE reduction launch and ONE finalize launch.  Every level keeps the chunking and the summation order it has alone:
 * out of level i == ppst_gap_gmp_st on level i, bit for bit, for any batch.  All levels share B and the storage type x_st;
 * C % 4 == 0, ld % 4 == 0, x 16-byte aligned (8 for a half type), else PPST_EINVAL; a null x / out / ws: PPST_ENULL.
 * ws: ppst_gap_gmp_multi_level_ws bytes (the levels' ppst_gap_gmp_ws, summed). */
typedef struct {
  const void* x;     /* [B][H][W][ld] */
  const void* mask;  /* optional [B][H][W] */
  void* out;         /* [B][2C] */
  int32_t H, W, C, ld;
} ppst_gap_gmp_level;
int64_t ppst_gap_gmp_multi_level_ws(const ppst_gap_gmp_level* levels, int n, int B);
int ppst_gap_gmp_multi_level(const ppst_gap_gmp_level* levels, int n, int B, void* ws, int x_st, void* stream);
/* integer-factor average pool (adaptive_avg_pool2d to H/f) NHWC -> dst slice */
int ppst_avgpool(const void* x, void* y, int B, int H, int W, int C, int x_ld, int f,
                 int y_ld, void* stream);
/* bilinear resize, align_corners=False (F.interpolate; generator.py:75,274-277,
 * encoder_col.py:129) NHWC -> dst slice with pixel stride y_ld */
int ppst_bilinear(const void* x, void* y, int B, int H, int W, int C, int x_ld,
                  int OH, int OW, int y_ld, void* stream);
/* Tail of a correspondence feature head (generator.py:174-238, the layer128 / layer256 heads): with
 * f = act(a*x + s) the activated output of the head's last conv, writes feat = PxP average pool of f
 * ([B][H/P][W/P], pixel stride feat_ld) and feat1 = F.interpolate(f, (H/D, W/D), bilinear) for the exact
 * factors D = 1 (f itself) and D = 2 (2x2 mean) in one read of x -- f is never stored at full size. */
int ppst_head_tail(const void* x, const void* scale_shift, const void* prelu, void* feat, void* feat1,
                   int B, int H, int W, int C, int x_ld, int feat_ld, int feat1_ld, int P, int D, int act,
                   void* stream);
/* 2x2 max pool on masks (encoder_col.py:218) NHWC */
int ppst_maxpool2(const void* x, void* y, int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------- linear ----
 * y[b][n] = act( sum_k f(x[b][k]) * w[n][k] * wscale + bias[n]*bscale )
 * (EqualLinear stylegan2_layers.py:222-242, EqualizedLinear :268-273,
 * nn.Linear of the E2 projectors encoder_col.py:52-88).  relu_in applies ReLU
 * to x first (the projectors' leading nn.ReLU). act: PPST_ACT_NONE/LRELU. */
int ppst_linear(const void* x, const void* w, const void* bias, void* y,
                int B, int K, int N, float wscale, float bscale, int relu_in, int act,
                void* stream);
/* rows: y = x * rsqrt(sum x^2 + eps)  (util.normalize, util/util.py:18-22; mode 0)
 *       y = x / max(||x||, eps)        (F.normalize; mode 1) */
int ppst_l2norm_rows(const void* x, void* y, int B, int K, float eps, int mode, void* stream);
/* y = a*(1-r) + b*r (util.lerp, util/util.py:32-35) */
int ppst_lerp(const void* a, const void* b, void* y, int64_t n, float r, void* stream);
/* n <= PPST_GROUP_MAX independent problems of the three ops above in ONE launch each (the E2 projector levels of a pass, the
 * generator's StyleMod / GeneratorModulation linears, the four code vectors of a swap).  A problem is the argument list of the
 * single call; it runs the kernel form that call would pick (a linear of more than 16 rows stays the 16-row pieces it is there;
 * pieces beyond the 32 one launch holds go out in a further launch) and gives its result bit for bit.  An empty problem (B or n
 * of 0) is skipped; a bad size in any problem: PPST_EINVAL, a null pointer in any non-empty problem: PPST_ENULL -- checked for
 * the whole table before anything is launched. */
typedef struct {
  const void* x; const void* w; const void* bias /* may be NULL */; void* y;
  int32_t B, K, N;
  float wscale, bscale;
  int32_t relu_in, act;
} ppst_linear_problem;
typedef struct { const void* x; void* y; int32_t B, K; float eps; int32_t mode; } ppst_l2norm_problem;
typedef struct { const void* a; const void* b; void* y; int64_t n; float r; } ppst_lerp_problem;
int ppst_linear_grouped(const ppst_linear_problem* problems, int n, void* stream);
int ppst_l2norm_rows_grouped(const ppst_l2norm_problem* problems, int n, void* stream);
int ppst_lerp_grouped(const ppst_lerp_problem* problems, int n, void* stream);
/* GeneratorModulation (generator.py:80-91): y[b,p,c] = x[b,p,c]*scale[b,c] + bias[b,c] */
int ppst_spatial_modulation(const void* x, const void* scale, const void* bias, void* y,
                            int B, int64_t hw, int C, void* stream);
int ppst_spatial_modulation_st(const void* x, const void* scale, const void* bias, void* y,
                               int B, int64_t hw, int C, int y_st /* x (the spatial code) stays fp32 */, void* stream);

/* ------------------------------------------------------ correspondence --- */
/* PPSTModel.Rselfcorr (ppst_model.py:330-339): fea NHWC [B][H][W][C] ->
 * out NHWC slice [B][H/4][W/4][256] at pixel stride out_ld. */
int ppst_rselfcorr(const void* fea, void* out, int B, int H, int W, int C, int out_ld,
                   void* stream);
/* corrm feature prep (ppst_model.py:349-361): per pixel, mean-centre the first
 * `ncenter` channels, then L2-normalise all C channels (+eps). [B][P][C] rows. */
int ppst_corr_prep(const void* fea, void* out, int B, int P, int C, int ncenter, void* stream);
/* corrm with opt.match_kernel = k != 1 (ppst_model.py:345-347): F.unfold(fea, k, padding = k / 2) of an NHWC map
 * [B][H][W][C] written as rows [B][H*W][C*k*k], column c*k*k + ky*k + kx (F.unfold's order), zeros outside; k odd.
 * _bwd: dx [B][H][W][C] from the gradient of those rows.  (ppst_corr_prep takes rows of any length.) */
int ppst_unfold_rows(const void* x, void* out, int B, int H, int W, int C, int k, void* stream);
int ppst_unfold_rows_bwd(const void* g, void* dx, int B, int H, int W, int C, int k, void* stream);
/* fp32 MFMA GEMM, C[b] = alpha * A[b] (MxK, row-major) * B[b]^T (NxK row-major) */
int ppst_gemm_nt_f32(const void* A, const void* Bm, void* C, int batch, int M, int N, int K,
                     float alpha, void* stream);
/* fp32 MFMA GEMM, C[b] = A[b] (MxK row-major) * B[b] (KxN row-major, ldb) -> ldc */
int ppst_gemm_nn_f32(const void* A, const void* Bm, void* C, int batch, int M, int N, int K,
                     int ldb, int ldc, void* stream);
/* The same two products on the bf16 matrix pipe (torch.matmul of ppst_model.py:363 / :377 / :385, fp32 in and out).
 * passes = 6: three bf16 planes per operand (all 24 mantissa bits), fp32-class results -- the cosine logits the softmax
 *             multiplies by 1 / T = 100; K % 16 == 0.
 * passes = 3: two planes (the convs' bf16x3, ~2^-16 relative per product) -- softmax rows times feature / gradient
 *             matrices; K % 32 == 0.
 * A, Bm 16-byte aligned; other values of passes: PPST_EINVAL. */
int ppst_gemm_nt_split(const void* A, const void* Bm, void* C, int batch, int M, int N, int K,
                       float alpha, int passes, void* stream);
int ppst_gemm_nn_split(const void* A, const void* Bm, void* C, int batch, int M, int N, int K,
                       int ldb, int ldc, int passes, void* stream);
/* in-place row softmax of x/div (F.softmax(matmul/0.01, dim=-1), ppst_model.py:363) */
int ppst_softmax_rows(void* x, int64_t rows, int cols, float div, void* stream);
/* PPSTModel.warp unfold/fold plumbing (ppst_model.py:366-387): NCHW image
 * [B][C][H][W] <-> patch rows [B][P][C*s*s] */
int ppst_unfold_patches(const void* x, void* y, int B, int C, int H, int W, int s, void* stream);
int ppst_fold_patches(const void* x, void* y, int B, int C, int H, int W, int s, void* stream);

/* -------------------------------------------------------- pre-process ---- */
/* One pass of Pillow's 8-bit resample (Image.resize(..., BICUBIC): data/base_dataset.py:141-168
 * __make_power_2 / __scale_shortside) over interleaved uint8 images x [B][in_h][in_w][C]:
 * horizontal != 0 resizes the width to out_size, else the height.  bounds int32 [out_size][2] =
 * (first input sample, count), coef int32 [out_size][ksize] = 22-bit fixed-point weights (host
 * logic: Pillow's precompute_coeffs + normalize_coeffs_8bpc, ppst_amd/imageio.py).
 * y = clip8((2^21 + sum in*coef) >> 22): integer arithmetic, bit-exact.  Pillow runs the
 * horizontal pass first, then the vertical one, each rounding to uint8. */
int ppst_resample_u8(const void* x, void* y, int B, int in_h, int in_w, int C, int out_size, int horizontal,
                     const void* bounds, const void* coef, int ksize, void* stream);
/* transforms.ToTensor + transforms.Normalize(mean, std) (base_dataset.py:133-138): uint8 HWC
 * [B][H][W][C] -> fp32 NCHW, (v/255 - mean)/std in that operation order. */
int ppst_u8_to_tensor(const void* x, void* y, int B, int H, int W, int C, float mean, float stdv, void* stream);
/* The same filter (Pillow's antialiased bicubic: Keys a = -0.5, support 2 * max(1, in / out), window bounds of
 * precompute_coeffs) on fp32 planes, both axes in ONE launch: x [B][in_h][in_w] -> y [B][out_h][out_w], B = batch * channels.
 * bounds_* int32 [out][2] = (first input sample, count <= ksize_*), coef_* fp32 [out][ksize_*] = weights that sum to 1 per
 * output position (host logic, float64 rounded once: ppst_amd/imageio.py); the windows advance with the output index.  A
 * block filters the input rows its 16 x 64 output tile needs horizontally into LDS and then vertically from LDS (fp32 fma,
 * taps in ascending order): the half-filtered image never reaches memory.  An axis with in == out is copied: its tables are
 * not read and may be null.  clamp != 0: the result is clamped to [lo, hi] at the store (a bicubic overshoots; Pillow's
 * 8-bit path clips the same way).
 * The vertical window of one tile must fit the LDS: min(in_h, 15 * in_h / out_h + ksize_v + 1) <= 192 rows (integer division;
 * ksize_v = 1 for a copied axis), else PPST_EINVAL -- every reduction up to 8 : 1 fits.  B * in_h * in_w and B * out_h * out_w
 * at most 2^32 - 1; clamp with lo > hi: PPST_EINVAL. */
int ppst_resample_f32(const void* x, void* y, int B, int in_h, int in_w, int out_h, int out_w,
                      const void* bounds_h, const void* coef_h, int ksize_h,
                      const void* bounds_v, const void* coef_v, int ksize_v,
                      int clamp, float lo, float hi, void* stream);
/* An aligned square crop of a photograph under a similarity transform, antialiased: photo uint8 [B][H][W][3] -> out uint8
 * [B][n][n][3].  A transform is four int64 (a, b, cu, cv): the photo pixel in column X, row Y (centre X + 1/2, Y + 1/2) lies at
 *   U = a (2X + 1) + b (2Y + 1) + cu,   V = -b (2X + 1) + a (2Y + 1) + cv      (units of 2^-24 crop pixel)
 * in the crop's frame; the crop is 0 <= U, V < n 2^24 and s = 2^23 / sqrt(a^2 + b^2) is photo pixels per crop pixel
 * (ppst_amd/imageio.py: crop_transform).  xf_host [B][4] is read by the entry point (rule, tile choice), xf_dev is the same table
 * on the device (read by the kernel).  out[j][i][c] = clamp(rint(sum w photo[clamp(Y)][clamp(X)][c] / sum w), 0, 255) with
 * w = k((U - (2i + 1) 2^23) / 2^24) k((V - (2j + 1) 2^23) / 2^24), k Pillow's bicubic (Keys a = -0.5), over every integer (X, Y),
 * inside the photo or not (edge replication), with both arguments below 2 in magnitude: Pillow's antialiased bicubic in the
 * crop's frame.  No float position is floored: which pixels enter a sum is decided in integers.
 * PPST_EINVAL, with nothing written: n <= 0, n > 4096, H W > 2^28, a transform with s < 1 or s > 8 (2^40 <= a^2 + b^2 <= 2^46
 * required: the upper end of s bounds the staged footprint of a tile) or |cu|, |cv| > 2^56. */
int ppst_extract_similarity(const void* photo_u8, int B, int H, int W, const void* xf_host, const void* xf_dev, int n,
                            void* out_u8, void* stream);

/* PNG encode on the device (ppst_amd/csrc/png.hip): uint8 HWC [B][H][W][C], C = 1 (grey) or 3 (RGB), 8 bits per sample, ->
 * B complete PNG files.  Per row the filter with the smallest sum of absolute signed bytes (libpng's heuristic, ties to the
 * lowest filter number); the filtered stream is cut into 32 KB pieces, each one dynamic-Huffman deflate block of literals
 * (or a stored block when that is not smaller) in an IDAT chunk of its own; deterministic, independent of the batch.
 *   ppst_png_bound   bytes one file can take (stored-block worst case included; a multiple of 16); PPST_EINVAL for bad sizes
 *   ppst_png_ws      bytes of the caller-owned workspace (> 0, also for B = 0)
 *   ppst_png_encode  files: [B][ppst_png_bound(H, W, C)] bytes, file i starts at i * bound; sizes: int64 [B], the file lengths.
 *                    Bytes of a slot behind its file's length are not written.  img_u8, files, work: 16-byte aligned.
 * H, W >= 1; C other than 1 / 3, or H * (1 + W * C) >= 2^31 - 64: PPST_EINVAL. */
int64_t ppst_png_bound(int H, int W, int C);
int64_t ppst_png_ws(int B, int H, int W, int C);
int ppst_png_encode(const void* img_u8, void* files, void* sizes, int B, int H, int W, int C, void* work, void* stream);

/* JPEG encode on the device (ppst_amd/csrc/jpeg.hip): uint8 HWC [B][H][W][C], C = 1 (grey, one component) or 3 (RGB -> YCbCr), ->
 * B complete baseline sequential JPEG files (ITU-T T.81, JFIF 1.01).  The format, so that a host model can restate it:
 *   quality      1 .. 100, libjpeg's scaling of the Annex K tables: s = 5000 / q (q < 50) or 200 - 2 q, Q = clamp((base * s + 50) / 100,
 *                1, 255) in integer arithmetic; DQT in zigzag order, table 0 luma, table 1 chroma
 *   subsampling  PPST_JPEG_444 or PPST_JPEG_420 (Pillow's numbers); grey ignores which of the two
 *   colour       Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *                Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16; partial MCUs repeat the last column / row of the
 *                pixels; 4:2:0 chroma = (sum of the 2 x 2 + bias) >> 2, bias 1, 2, 1, 2 .. along x
 *   DCT          level shift 128; integer fixed point: T[u][x] = round(2^14 c(u) / 2 cos((2 x + 1) u pi / 16)); rows
 *                a = (sum s T + 128) >> 8, columns b = sum a T (scale 2^20), q = sign(b) ((|b| + (Q << 19)) / (Q << 20)): to nearest,
 *                halves away from zero.  No floating point anywhere: the bytes are a pure function of the pixels
 *   entropy      the four Annex K "typical" Huffman tables, written as DHT (DC 0, AC 0, DC 1, AC 1)
 *   restarts     DRI = 96 MCUs (grey), 32 (4:4:4), 16 (4:2:0): 96 blocks, one workgroup's interval whatever the width; DC predictors
 *                start at 0 in each, each is padded with 1-bits to a byte, FF is followed by 00, RSTm (m = 0 .. 7, cycling) between
 *   segments     SOI, APP0 (JFIF, density 1:1), DQT x 1 | 2, SOF0, DHT x 2 | 4, DRI, SOS, the scan, EOI
 *   ppst_jpeg_bound   bytes one file can take: a true worst case, a multiple of 16; PPST_EINVAL for bad arguments.  A block takes at
 *                     most 11 + 11 bits (longest DC code, chroma; 11 magnitude bits) + 63 x (16 + 10) (longest AC code, 10 magnitude
 *                     bits) = 1660 bits (EOB and ZRL only replace coefficients, by less); an interval of n blocks is padded to
 *                     ceil(1660 n / 8) bytes, every one of which may be an FF with its 00: x 2; + 2 for the marker behind it (RSTm
 *                     or EOI); + the header (SOI through SOS: 334 bytes grey, 629 colour)
 *   ppst_jpeg_ws      bytes of the caller-owned workspace (> 0, also for B = 0)
 *   ppst_jpeg_header  host code, no GPU: the bytes from SOI through SOS, written from the constant tables the kernels read; returns
 *                     their count; out may be null (count only); cap < count: PPST_EINVAL, nothing written
 *   ppst_jpeg_encode  files: [B][ppst_jpeg_bound(H, W, C, subsampling)] bytes, file i starts at i * bound; sizes: int64 [B], the
 *                     file lengths.  Bytes of a slot behind its file's length are not written.  img_u8, files, work: 16-byte aligned.
 * 1 <= H, W <= 65535; C other than 1 / 3, another subsampling or quality, or a worst-case file of 2^32 bytes or more (a file's scan
 * offsets are 32-bit): PPST_EINVAL, reported ahead of null pointers (PPST_ENULL); B = 0: PPST_OK, nothing touched. */
#define PPST_JPEG_444 0
#define PPST_JPEG_420 2
int64_t ppst_jpeg_bound(int H, int W, int C, int subsampling);
int64_t ppst_jpeg_ws(int B, int H, int W, int C, int subsampling);
int64_t ppst_jpeg_header(int H, int W, int C, int quality, int subsampling, void* out, int64_t cap);
int ppst_jpeg_encode(const void* img_u8, void* files, void* sizes, int B, int H, int W, int C, int quality, int subsampling,
                     void* work, void* stream);

/* JPEG decode on the device (ppst_amd/csrc/jpeg_parse.hip: host parser; ppst_amd/csrc/jpeg_decode.hip: kernels): B baseline JPEG
 * files of DIFFERENT sizes and samplings, packed into one byte buffer, -> uint8 HWC images, equal byte for byte to libjpeg-turbo's
 * default decoder (jidctint "islow", fancy upsampling), which is what Pillow runs.  Integer arithmetic only.
 *   accepted     SOF0, 8 bits; one component (its sampling factors are ignored, T.81 A.2.2), or three with Y at 1x1 (4:4:4) or 2x2
 *                (4:2:0) and both chroma at 1x1; ONE interleaved scan with Ss, Se, Ah/Al = 0, 63, 0; 8-bit DQT; DC / AC tables 0 and 1,
 *                any contents (optimised files); DRI or none; APPn / COM are skipped
 *   refused      by ppst_jpeg_parse with one PPST_JPEG_E* each (below); the parser bounds every read by n and trusts no length
 *   descriptor   ppst_jpeg_dec_image, plain data: the parser fills everything but the caller's four fields (file_off: where the
 *                file starts in the packed buffer; out_off: where image i starts in out_u8; mirror: columns reversed; expand_grey:
 *                a one-component file is written as three equal channels).  scan_off / scan_len: the entropy-coded segment, from
 *                behind SOS to the first FF D9 behind it.  qt: per component, 64 entries in the file's (zigzag) order.  bits / vals:
 *                BITS[16] and HUFFVAL of the tables DC 0, DC 1, AC 0, AC 1; dc_tab / ac_tab: each component's table number.
 *   stages       (a) clean: per 4096-byte chunk of the segment, the 00 behind an FF and both bytes of RSTm are dropped (a prefix
 *                over the chunks' counts in a second launch places the bytes); the clean offset behind RSTm number r is the start
 *                of interval r + 1; m must be r mod 8 and there must be ceil(MCUs / DRI) - 1 of them;
 *                (b) entropy: one workgroup per restart interval (a file without DRI: one).  The interval's bits are cut into
 *                subsequences of 32 * subseq_words bits (0: the default, 32 words; at least 2).  The state at a boundary is
 *                (p, b, k): bit position of the first codeword at or behind it, block within the MCU, zigzag index.  Subsequence 0
 *                enters at (0, 0, 0), every other one is guessed as (its boundary, 0, 0); a round decodes every subsequence whose
 *                entry changed from its entry until p passes its end and hands (p, b, k) to its successor; rounds repeat until no
 *                entry changes -- after round r the first r subsequences are final, so the fixed point is the sequential decode
 *                and there are at most #subsequences rounds.  A code the tables do not define advances one bit, k beyond 63
 *                starts a new block, bits behind the interval are zero.  Then a prefix over the blocks each subsequence completed
 *                gives it its first block, a second decode stores the coefficients (int16 [blocks][64], zigzag; every store
 *                checked against the interval's block count), and DC differences are summed per component within the interval;
 *                (c) IDCT: coefficient x table, libjpeg's jidctint: CONST_BITS 13, PASS1_BITS 2, FIX 2446 3196 4433 6270 7373 9633
 *                12299 15137 16069 16819 20995 25172; columns descaled by 11, rows by 18, + 128, clamped to 0 .. 255; planes padded to whole MCUs;
 *                (d) 4:2:0 chroma by libjpeg's fancy h2v2: rows 3 near + far (the neighbour row replicated at the top and bottom
 *                of the ceil(H / 2) rows), columns (3 this + left + 8) >> 4 and (3 this + right + 7) >> 4 (this for the missing
 *                neighbour at both ends); a chroma plane at most 2 samples wide: plain 2 x 2 replication.  Colour, Cb' = Cb - 128:
 *                R = Y + ((91881 Cr' + 32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16),
 *                G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16), arithmetic shifts, clamped.
 *   status       int32 [B], 0 = decoded; else a sum of PPST_JPEG_S_* (below): the image's pixels are then undefined (but written
 *                within its own H x W x C bytes only) and every other image of the batch is unaffected
 *   ppst_jpeg_parse      host code, no GPU
 *   ppst_jpeg_decode_ws  host code: bytes of the caller-owned workspace for these B descriptors (> 0; grows with every file's size);
 *                        PPST_EINVAL for B < 0, subseq_words of 1 or above 65536, or a descriptor the parser would not have made
 *   ppst_jpeg_decode     bytes: the packed files on the device (nbytes of them); imgs_host: the descriptors (launch geometry);
 *                        imgs_dev: a copy of the same B descriptors on the device (what the kernels read); out_u8: out_bytes
 *                        bytes, image i is HWC at out_off, C = 1 (grey) or 3; every file and image must lie inside its buffer:
 *                        PPST_EINVAL.  work, out_u8, imgs_dev: 16-byte aligned.  After the call the first B int32 of work hold, per
 *                        image, the largest number of rounds one of its intervals took.  B = 0: PPST_OK, nothing touched. */
#define PPST_JPEG_E_TRUNCATED (-101)   /* the file ends inside a segment, or has no EOI behind its scan */
#define PPST_JPEG_E_NOT_JPEG (-102)    /* no SOI */
#define PPST_JPEG_E_ORDER (-103)       /* a segment out of order, missing or unknown, or of an impossible length */
#define PPST_JPEG_E_PROGRESSIVE (-104) /* SOF2 (or any other non-baseline Huffman process) */
#define PPST_JPEG_E_ARITHMETIC (-105)  /* SOF9 .. SOF15 */
#define PPST_JPEG_E_PRECISION (-106)   /* not 8 bits per sample */
#define PPST_JPEG_E_SAMPLING (-107)    /* 4:2:2, 4:4:0, 4:1:1, ... */
#define PPST_JPEG_E_COMPONENTS (-108)  /* two, four or more components */
#define PPST_JPEG_E_ADOBE_RGB (-109)   /* RGB, not YCbCr, by libjpeg's rule: no JFIF APP0 and Adobe transform 0, or neither and ids 'R' 'G' 'B' */
#define PPST_JPEG_E_MULTISCAN (-110)   /* a scan that does not hold every component */
#define PPST_JPEG_E_DQT16 (-111)       /* 16-bit quantisation table */
#define PPST_JPEG_E_SIZE (-112)        /* H or W 0 (or the file too large for 32-bit offsets) */
#define PPST_JPEG_E_HUFFMAN (-113)     /* a Huffman table missing, over-subscribed or with an id above 1 */
#define PPST_JPEG_E_SCAN (-114)        /* Ss, Se, Ah/Al other than 0, 63, 0 */
#define PPST_JPEG_S_MARKER 1           /* status bits: an FF inside the scan followed by neither 00 nor RSTm */
#define PPST_JPEG_S_RST_COUNT 2        /*   not ceil(MCUs / DRI) - 1 restart markers */
#define PPST_JPEG_S_RST_ORDER 4        /*   RSTm out of its 0 .. 7 cycle */
#define PPST_JPEG_S_CODE 8             /*   a code no table defines, or a run beyond the block */
#define PPST_JPEG_S_BLOCKS 16          /*   an interval does not hold its number of blocks */
typedef struct ppst_jpeg_dec_image {
  int32_t H, W, ncomp;
  int32_t ss;                 /* 1: grey and 4:4:4 (8 x 8 MCUs); 2: 4:2:0 (16 x 16 MCUs) */
  int32_t hs[3], vs[3];       /* the sampling factors as the file states them */
  int32_t dri;                /* MCUs per restart interval, 0: none */
  int32_t scan_off, scan_len; /* within the file */
  uint8_t qt[3][64];
  uint8_t dc_tab[3], ac_tab[3];
  uint8_t pad_[2];
  uint8_t bits[4][16];
  uint8_t vals[4][256];
  int64_t file_off, out_off;  /* the caller's */
  int32_t mirror, expand_grey;
} ppst_jpeg_dec_image;
int ppst_jpeg_parse(const void* file, int64_t n, ppst_jpeg_dec_image* out);
int64_t ppst_jpeg_decode_ws(const ppst_jpeg_dec_image* imgs, int B, int subseq_words);
int ppst_jpeg_decode(const void* bytes, int64_t nbytes, const ppst_jpeg_dec_image* imgs_host, const void* imgs_dev, void* out_u8,
                     int64_t out_bytes, void* status, int B, int subseq_words, void* work, void* stream);

/* PNG decode on the device (ppst_amd/csrc/png_parse.hip: host parser; ppst_amd/csrc/png_decode.hip: kernels): B PNG files of
 * DIFFERENT sizes and colour types, packed into one byte buffer, -> uint8 HWC images, equal byte for byte to what Pillow reads
 * (numpy.asarray(Image.open(f)); with expand_grey / drop_alpha: Image.open(f).convert("RGB")).  Integer code only.
 *   accepted     8 bits per sample; colour type 0 (grey), 2 (RGB) or 6 (RGBA); no interlace; compression and filter method 0; at
 *                least one IDAT, all IDAT chunks consecutive; IEND.  Ancillary chunks (tRNS included) and PLTE in a colour file
 *                are skipped.
 *   refused      by ppst_png_parse with one PPST_PNG_E_* each (below); the parser bounds every read by n, trusts no chunk length,
 *                computes no CRC and inflates nothing
 *   descriptor   ppst_png_dec_image, plain data: the parser fills everything but the caller's fields (file_off: where the file
 *                starts in the packed buffer; out_off: where image i starts in out_u8; span_off: index of the file's first span
 *                in the device span array; mirror: columns reversed; expand_grey: a grey file is written as three equal
 *                channels; drop_alpha: an RGBA file is written as RGB).  The span table, one ppst_png_span per chunk in file
 *                order, is the caller's array: type (the four bytes, big-endian), off (of the chunk's DATA within the file), len,
 *                crc (as stored), idat.  When span_cap is too small the parser returns PPST_PNG_E_SPANS and nspans holds the
 *                count a second call needs.
 *   stages       (a) per chunk: CRC-32 over type + data against the stored one; IDAT payloads concatenated to one zlib stream;
 *                the zlib header (CM 8, CINFO <= 7, no FDICT, a multiple of 31);
 *                (b) inflate, one workgroup per image, deflate blocks in order: stored blocks copied; for a fixed or dynamic
 *                block the code tables are built in LDS and the block's bits are cut into subsequences of 32 * subseq_words
 *                bits (0: the default, 4 words; 2 .. 128).  The state at a boundary is the bit position of the first token at or
 *                behind it; subsequence 0 enters exactly, every other one is guessed to enter at its boundary; a round decodes
 *                every subsequence whose entry changed and hands its exit to its successor; rounds repeat until no entry
 *                changes (at most #subsequences rounds per window of one subsequence per lane).  A second decode writes, for
 *                the n = H (1 + W C) bytes of the stream, raw[pos] (literals) and src[pos]: pos for a literal,
 *                pos + (i mod d) - d for byte i of a match at distance d;
 *                (c) pointer jumping src[i] <- src[src[i]] in place, ceil(log2 n) + 1 launches; stream[i] = raw[src[i]];
 *                Adler-32 of the stream against the trailer;
 *                (d) the five row filters undone (one workgroup per image, a row per lane, skewed by one pixel per row), HWC
 *                store with mirror / expand_grey / drop_alpha.
 *   status       int32 [B], 0 = decoded; else a sum of PPST_PNG_S_* (below): the image's pixels are then undefined (but written
 *                within its own bytes only) and every other image of the batch is unaffected
 *   ppst_png_parse      host code, no GPU
 *   ppst_png_decode_ws  host code: bytes of the caller-owned workspace for these B descriptors (> 0); PPST_EINVAL for B < 0,
 *                       subseq_words of 1 or above 128, or a descriptor the parser would not have made
 *   ppst_png_decode     files: the packed files on the device (files_bytes of them); descs_host: the descriptors (launch
 *                       geometry); descs_dev: a copy of the same B descriptors on the device; spans_dev: the span tables on the
 *                       device, file i's nspans entries from span_off; out_u8: out_bytes bytes, image i is HWC at out_off with
 *                       C = 1, 3 or 4; every file and image must lie inside its buffer: PPST_EINVAL.  work, out_u8, descs_dev,
 *                       spans_dev: 16-byte aligned.  After the call the first B int32 of work hold, per image, the largest
 *                       number of rounds one window of the subsequence iteration took.  B = 0: PPST_OK, nothing touched.
 *                       spans_dev and work carry no length in this interface: the entry point trusts that spans_dev holds
 *                       span_off + nspans entries for every file and that work has ppst_png_decode_ws bytes (the kernels still
 *                       clamp every span to its file before reading through it). */
#define PPST_PNG_E_SIGNATURE (-201)  /* not the eight signature bytes */
#define PPST_PNG_E_TRUNCATED (-202)  /* the file ends inside a chunk */
#define PPST_PNG_E_IHDR (-203)       /* the first chunk is not IHDR, or not of 13 bytes; a second IHDR */
#define PPST_PNG_E_DEPTH (-204)      /* bit depth other than 8 */
#define PPST_PNG_E_COLOUR (-205)     /* palette (3), grey + alpha (4), or no colour type at all */
#define PPST_PNG_E_INTERLACE (-206)  /* Adam7 (or an unknown interlace method) */
#define PPST_PNG_E_SIZE (-207)       /* H or W 0 (or beyond 2^31 - 1) */
#define PPST_PNG_E_TOO_LARGE (-208)  /* H (1 + W C) >= 2^31, or a file of 2^28 bytes or more */
#define PPST_PNG_E_IDAT (-209)       /* no IDAT, or IDAT chunks that are not consecutive */
#define PPST_PNG_E_IEND (-210)       /* no IEND */
#define PPST_PNG_E_APNG (-211)       /* acTL: an animation */
#define PPST_PNG_E_METHOD (-212)     /* compression or filter method other than 0 */
#define PPST_PNG_E_SPANS (-213)      /* span_cap too small: nspans holds the count needed */
#define PPST_PNG_S_CRC 1             /* status bits: a chunk's CRC-32 */
#define PPST_PNG_S_ZLIB 2            /*   zlib header */
#define PPST_PNG_S_BTYPE 4           /*   block type 3 */
#define PPST_PNG_S_STORED 8          /*   LEN / NLEN of a stored block, or a stored block beyond the stream */
#define PPST_PNG_S_LENGTHS 16        /*   code lengths: over-subscribed, incomplete, bad repeat, too many symbols, no end-of-block */
#define PPST_PNG_S_CODE 32           /*   a code no table defines */
#define PPST_PNG_S_DISTANCE 64       /*   a distance beyond the bytes produced so far */
#define PPST_PNG_S_STREAM 128        /*   more or fewer than H (1 + W C) bytes, or the bits end before the final block does */
#define PPST_PNG_S_ADLER 256         /*   Adler-32 */
#define PPST_PNG_S_FILTER 512        /*   a filter byte above 4 */
typedef struct ppst_png_span {
  uint32_t type;              /* 'I' << 24 | 'D' << 16 | 'A' << 8 | 'T' */
  int32_t off, len;           /* the chunk's data within the file */
  uint32_t crc;               /* as the file states it */
  int32_t idat;               /* 1: an IDAT chunk */
} ppst_png_span;
typedef struct ppst_png_dec_image {
  int32_t H, W, colour, channels;
  int32_t nspans;             /* chunks of the file */
  int32_t first_idat, nidat;  /* span indices: the IDAT chunks are first_idat .. first_idat + nidat - 1 */
  int32_t idat_bytes;         /* the sum of their lengths: the zlib stream */
  int64_t file_len;
  int64_t file_off, out_off, span_off;       /* the caller's */
  int32_t mirror, expand_grey, drop_alpha;
  int32_t pad_;
} ppst_png_dec_image;
int ppst_png_parse(const void* file, int64_t n, ppst_png_dec_image* out, ppst_png_span* spans, int span_cap);
int64_t ppst_png_decode_ws(const ppst_png_dec_image* descs, int B, int subseq_words);
int ppst_png_decode(const void* files, int64_t files_bytes, const ppst_png_dec_image* descs_host, const void* descs_dev,
                    const void* spans_dev, void* out_u8, int64_t out_bytes, void* status, int B, int subseq_words, void* work,
                    void* stream);

/* ------------------------------------------------ LPIPS-AlexNet metric ---- */
/* LPIPS v0.1, net = 'alex', lpips = True, spatial = False, normalize = False, eval mode (csrc/lpips.hip): for two fp32 image
 * batches a, b (B, 3, H, W)
 *   x' = (x - shift) / scale per channel;  relu1..relu5 of torchvision's AlexNet `features` (conv 11x11 s4 p2 -> 64, pool 3 s2,
 *   conv 5x5 p2 -> 192, pool 3 s2, conv 3x3 p1 -> 384 -> 256 -> 256; floor sizes, zero padding, bias);
 *   per layer n(f) = f / (sqrt(sum_c f^2) + 1e-10), s_l = mean_hw sum_c lin_l[c] (n(fa) - n(fb))^2;  result sum_l s_l per image.
 * The weights are frozen: there is a forward and an INPUT gradient, no weight gradient.  fp32 storage and arithmetic.  Where
 * sqrt(sum_c f^2) is exactly 0 the gradient to that pixel's features is defined as 0 (autograd of the formula gives NaN).
 * Pool ties go to the first maximum in row-major window order.  Every reduction has a fixed order: repeated calls are
 * bit-identical.  The caller owns every buffer; all of them 16-byte aligned.
 *   ppst_lpips_pack_floats  floats of the packed weights
 *   ppst_lpips_pack     once per weight set: weight / bias / lin are host arrays of five device pointers -- the conv weights in
 *                       torch layout [Cout][Cin][K][K] (64x3x11x11, 192x64x5x5, 384x192x3x3, 256x384x3x3, 256x256x3x3), their
 *                       biases, and the lin weights [C_l]; shift, scale: 3 floats each.  Forward and (flipped, transposed)
 *                       gradient forms are both written to `pack`.
 *   ppst_lpips_dims     hw[10] = (h, w) of the five feature maps of an H x W image
 *   ppst_lpips_ws       bytes of the forward workspace for n images through the trunk (n = 2B for the metric)
 *   ppst_lpips_trunk    the na images of a, then the nb images of b (either count may be 0), as ONE batch through the trunk;
 *                       *_strides: 4 element strides (n, c, y, x) of the source tensors (any layout).  Leaves the five maps,
 *                       the pooled maps and the pools' arg-max bytes in ws.
 *   ppst_lpips_feature  copies map `layer` (0..4) of a workspace filled by ppst_lpips_trunk(n images) to contiguous NCHW
 *   ppst_lpips_tail     after ppst_lpips_trunk(na = nb = B): out[B] = the metric.  ws is written (block partial sums).
 *   ppst_lpips_bwd_ws   bytes of the backward scratch; which: 1 = gradient to a, 2 = to b, 3 = both
 *   ppst_lpips_backward ga / gb (B, 3, H, W) contiguous = d(sum_b gout[b] * out[b]) / d a, b, from the workspace the forward
 *                       left (read only).  Only the requested half of the trunk is walked back.
 * H, W < 31 (the second pool would have no full window) or > 16384, a negative count, which outside 1..3: PPST_EINVAL; a
 * count of 0 is a no-op; null pointers PPST_ENULL. */
int64_t ppst_lpips_pack_floats(void);
int ppst_lpips_pack(const void* const* weight, const void* const* bias, const void* const* lin, const void* shift, const void* scale,
                    void* pack, void* stream);
int ppst_lpips_dims(int H, int W, int* hw);
int64_t ppst_lpips_ws(int n, int H, int W);
int ppst_lpips_trunk(const void* pack, const void* a, const int64_t* a_strides, int na, const void* b, const int64_t* b_strides, int nb,
                     int H, int W, void* ws, void* stream);
int ppst_lpips_feature(const void* ws, int n, int H, int W, int layer, void* out_nchw, void* stream);
int ppst_lpips_tail(const void* pack, void* ws, int B, int H, int W, void* out, void* stream);
int64_t ppst_lpips_bwd_ws(int B, int H, int W, int which);
int ppst_lpips_backward(const void* pack, const void* ws, const void* gout, int B, int H, int W, int which, void* ga, void* gb,
                        void* bws, void* stream);

/* ------------------------------------------------ image-quality metrics ---- */
/* SSIM (Wang et al. 2004, Gaussian form), MS-SSIM (Wang et al. 2003) and PSNR of two image batches a, b (B, C, H, W), C >= 1,
 * data range L (csrc/ssim.hip).
 *   window g: 11 taps exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in float64, rounded once to fp32; separable, applied
 *   "valid": the maps are (H - 10) x (W - 10).  Per channel mu_a = g*a, mu_b = g*b, s_a = g*(a^2) - mu_a^2, s_b likewise,
 *   s_ab = g*(ab) - mu_a mu_b;  C1 = (0.01 L)^2, C2 = (0.03 L)^2;  cs = (2 s_ab + C2) / (s_a + s_b + C2),
 *   ssim = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1) * cs;  per (image, channel) the mean over the valid pixels, per image the
 *   mean of that over the channels.
 * The kernels work at L = 1 on inputs divided by data_range (SSIM is invariant under a common scale of a, b and L: for uint8
 * input that keeps the g*(a^2) - mu^2 cancellation at the size it has for [-1, 1] images).  fp32 arithmetic; the per-block partial sums are added in a fixed order in float64: repeated
 * calls are bit-identical, and no floating-point atomic is used.  The caller owns every buffer.
 * Inputs: `u8` = 0: fp32; 1: uint8 (forward only).  *_strides: 4 ELEMENT strides (n, c, y, x) of the source tensor, any layout
 * (a uint8 (B, H, W, C) image is the strides (H W C, 1, W C, C)).
 *   ppst_ssim_ws        bytes of the forward workspace (block partial sums)
 *   ppst_ssim_forward   ssim_bc[B * C], cs_bc[B * C] = the per-(image, channel) means of ssim and cs; out[B] (may be null) = the
 *                       per-image SSIM
 *   ppst_ssim_backward  grad (B, C, H, W) contiguous fp32 = d(sum_b gout[b] * out[b]) / d a (the first argument only; fp32
 *                       inputs).  With A = d ssim / d mu_a, Bm = d ssim / d (g*a^2), Cm = d ssim / d (g*ab) on the valid grid:
 *                       grad(q) = (g^T*A)(q) + 2 a(q) (g^T*Bm)(q) + b(q) (g^T*Cm)(q) (the full correlation of the zero-extended
 *                       maps) times gout[b] / (C (H - 10)(W - 10)).  One launch: every block recomputes the moments that reach
 *                       its tile; no map reaches memory, no workspace
 *   ppst_pool2x2        out (B, C, H / 2, W / 2) contiguous fp32 = the 2 x 2 mean with stride 2 (an odd trailing row / column is
 *                       dropped), in the input's own units: the step between two MS-SSIM scales
 *   ppst_msssim_combine vals[5][B * C]: rows 0..3 the mean cs of scales 1..4, row 4 the mean ssim of scale 5;
 *                       out[B] = mean_c prod_j max(vals[j], 0)^w_j, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
 *   ppst_sqerr_ws       bytes of the squared-error pass's workspace
 *   ppst_sqerr          out[B][3] = (mean (a - b)^2, mean |a - b|, 10 log10(L^2 / mean (a - b)^2): +inf for equal images), in
 *                       the inputs' own units
 * B < 0, C < 1, H or W < 11 (ppst_pool2x2: < 2; ppst_sqerr, ppst_msssim_combine: < 1), data_range <= 0, u8 outside {0, 1} or
 * B * C * H * W > 2^32 - 1: PPST_EINVAL (the *_ws functions return it as a negative size); B == 0 is a no-op (PPST_OK) before
 * any pointer is looked at; null pointers PPST_ENULL. */
int64_t ppst_ssim_ws(int B, int C, int H, int W);
int ppst_ssim_forward(const void* a, const int64_t* a_strides, const void* b, const int64_t* b_strides, int u8, int B, int C, int H,
                      int W, float data_range, void* out, void* ssim_bc, void* cs_bc, void* ws, void* stream);
int ppst_ssim_backward(const void* a, const int64_t* a_strides, const void* b, const int64_t* b_strides, const void* gout, int B,
                       int C, int H, int W, float data_range, void* grad, void* stream);
int ppst_pool2x2(const void* x, const int64_t* strides, int u8, int B, int C, int H, int W, void* out, void* stream);
int ppst_msssim_combine(const void* vals, int B, int C, void* out, void* stream);
int64_t ppst_sqerr_ws(int B, int C, int H, int W);
int ppst_sqerr(const void* a, const int64_t* a_strides, const void* b, const int64_t* b_strides, int u8, int B, int C, int H, int W,
               float data_range, void* out, void* ws, void* stream);

/* ---------------------------------------------------- colour statistics ---- */
/* Per-region colour statistics of uint8 RGB images and exact 1-Wasserstein distances between their histograms
 * (csrc/colour_stats.hip): what the style-fidelity metrics of ppst_amd/metrics.py are made of.
 *   img     (B, H, W, 3) uint8; ELEMENT strides img_sn (image), img_sy (row), img_sx (pixel: must be 3, the channels are
 *           adjacent), so a crop view of a larger image is read in place
 *   labels  (B, H, W) uint8 with strides lab_sn, lab_sy (pixels adjacent), or null: one region that holds every pixel.  A
 *           pixel whose label is >= R belongs to no region (255 = "ignore")
 *   dirs    HOST pointer, P rows of 3 int16 with sum_c |d_c| <= 4096 each (validated here, passed to the kernel by value)
 * Per image b and region r < R:
 *   hist[b][r][p][256] uint32  the exact histogram of t = (d_p . (r, g, b) + 255 * sum_{d_c < 0} |d_c|) >> 12, all integer;
 *                       0 <= t <= 255 by construction, and the row (4096, 0, 0) gives the red channel itself
 *   count[b][r] uint32  pixels of the region
 *   lab_mean[b][r][3], lab_cov[b][r][6] float64: mean and POPULATION covariance (divided by count; entries LL, La, Lb, aa,
 *                       ab, bb) of the pixels' CIELAB values.  Per pixel, in fp32: channel c -> lin(c) by a 256-entry table,
 *                       lin(c) = c / 255 / 12.92 below 0.04045, else ((c / 255 + 0.055) / 1.055)^2.4, built in float64 and
 *                       rounded once to fp32; (X / Xn, Y / Yn, Z / Zn) = M lin with M = the sRGB (D65) matrix rows
 *                       (0.4124564 0.3575761 0.1804375; 0.2126729 0.7151522 0.0721750; 0.0193339 0.1191920 0.9503041) divided
 *                       by the white point (0.95047, 1, 1.08883) in float64 and rounded once to fp32;
 *                       f(t) = cbrt(t) above (6/29)^3, else t * 841 / 108 + 4 / 29; L = 116 f(Y) - 16, a = 500 (f(X) - f(Y)),
 *                       b = 200 (f(Y) - f(Z)).  A wave of the kernel owns 1024 consecutive pixels: it sums (lab - pivot) and
 *                       its products per region, the pivot being the Lab value of the region's mean colour there (rounded to
 *                       integers: a flat region cancels exactly), and writes those sums to the workspace; a finishing launch
 *                       combines them in a fixed order in float64.  No floating-point atomic: repeats are bit-identical and an
 *                       image's numbers do not depend on its batch.  An empty region: count 0, moments 0
 *   ppst_colour_stats_ws  bytes of the workspace (partial sums and the constant tables)
 *   ppst_hist_w1    hist_a (Ba, R, P, 256), hist_b (Bb, R, P, 256) uint32; pairs (K, 2) int32 on the device.  num[k][r][p]
 *                   int64 = sum_{v = 0..255} |cumA(v) nB - cumB(v) nA| of histograms i_k of a and j_k of b: W1 in grey
 *                   levels is num / (nA nB), the caller's division.  Exact for n <= 2^22 (the sum stays below 2^52).  0 where a
 *                   side is empty; -1 where an index is outside [0, Ba) x [0, Bb) (nothing is read)
 * B < 0, H or W < 1, H * W > 2^22, R outside [1, 4], P outside [1, 16], img_sx != 3 (ppst_hist_w1: Ba, Bb or K < 0, R, P
 * likewise): PPST_EINVAL (ppst_colour_stats_ws returns it as a negative size); B == 0 (K == 0) is a no-op (PPST_OK) before any
 * pointer is looked at; null pointers (labels excepted) PPST_ENULL; then a row of
 * dirs with sum |d_c| > 4096: PPST_EINVAL.  Nothing is launched in any of these cases. */
int64_t ppst_colour_stats_ws(int B, int H, int W);
int ppst_colour_stats(const void* img, int64_t img_sn, int64_t img_sy, int64_t img_sx, const void* labels, int64_t lab_sn,
                      int64_t lab_sy, int B, int H, int W, int R, const int16_t* dirs, int P, void* hist, void* count, void* lab_mean,
                      void* lab_cov, void* ws, void* stream);
int ppst_hist_w1(const void* hist_a, int Ba, const void* hist_b, int Bb, const void* pairs, int K, int R, int P, void* num,
                 void* stream);

/* ------------------------------------------------------- colour transfer ---- */
/* Classical per-region colour transfer (csrc/colour_transfer.hip): the baselines the style-fidelity numbers are read against.
 * Regions R <= 4; a label >= R belongs to no region and its pixel keeps its bytes.
 *   ppst_hist_match_lut   exact histogram specification per RGB channel, in integers.  hist_c (Bc, R, P, 256), hist_s
 *                   (Bs, R, P, 256) uint32 as ppst_colour_stats writes them (P >= 3; projections 0..2 must be the channel axes,
 *                   the rest is not read); pairs (K, 2) int32 on the device.  luts[k][r][c][256] uint8: with hC, hS the
 *                   histograms of (region, channel) of content i_k and style j_k, nC, nS their counts and cum the inclusive
 *                   cumulative sum (cum(-1) = 0),
 *                     LUT[v] = min{u in 0..255 : 2 cumS(u) nC >= (cumC(v - 1) + cumC(v)) nS}
 *                   -- the mid-point form: a flat content region goes to the style's median, not to its maximum.  Every product
 *                   is below 2^46 (counts <= 2^22) and is taken in int64.  nC == 0 or nS == 0, or an index outside
 *                   [0, Bc) x [0, Bs) (nothing is read): the identity table
 *   ppst_colour_transfer_apply   img (B, H, W, 3) uint8 and labels (B, H, W) uint8 or null (every pixel is region 0) with the
 *                   stride rules of ppst_colour_stats; out uint8 [B][H][W][3], dense.  mode PPST_CT_LUT: maps = uint8
 *                   [B][R][3][256], out_c = LUT[label][c][in_c].  mode PPST_CT_AFFINE: maps = fp32 [B][R][12], a row
 *                   (T row-major | t): lab' = T lab + t in fp32 (fma chains, the offset innermost), with sRGB -> Lab as
 *                   "colour statistics" defines it and Lab -> sRGB its inverse: fy = (L + 16) / 116, fx = fy + a / 500,
 *                   fz = fy - b / 200; t = f^3 above 6/29, else (f - 4/29) * 108 / 841; linear RGB = Minv t, Minv the float64
 *                   inverse of the float64 matrix rounded once to fp32; clamp to [0, 1]; s = 12.92 c up to 0.0031308, else
 *                   1.055 c^(1/2.4) - 0.055; the byte is rint(255 s).
 *                   weights (may be null): fp32 [B][R][H][W], >= 0, normalised per pixel here: with W = sum_r w_r > 0 the LUT
 *                   mode gives rint(sum_r w_r LUT[r][c][in_c] / W) and the affine mode blends the 12 coefficients,
 *                   sum_r w_r k_r / W, before its one conversion (sums in region order, fp32); W == 0 falls back to the pixel's
 *                   label.  A pixel of no region is copied whatever its weights.  Pixels move as dwords, four pixels in three;
 *                   no atomics: repeats are bit-identical and an image gives the same bits alone as inside a batch.
 * B (K, Bc, Bs) < 0, H or W < 1, H * W > 2^22, R outside [1, 4], P outside [3, 16], img_sx != 3, a mode other than the two:
 * PPST_EINVAL; B == 0 (K == 0) is a no-op (PPST_OK) before any pointer is looked at; null pointers (labels and weights
 * excepted) PPST_ENULL.  Nothing is launched in any of these cases. */
#define PPST_CT_LUT 0
#define PPST_CT_AFFINE 1
int ppst_hist_match_lut(const void* hist_c, int Bc, const void* hist_s, int Bs, const void* pairs, int K, int R, int P, void* luts,
                        void* stream);
int ppst_colour_transfer_apply(const void* img, int64_t img_sn, int64_t img_sy, int64_t img_sx, const void* labels, int64_t lab_sn,
                               int64_t lab_sy, int B, int H, int W, int R, int mode, const void* maps, const void* weights, void* out,
                               void* stream);

/* ------------------------------------------------------- post-process ---- */
/* util.tensor2im quantisation (util/util.py:98-131): NCHW fp32 [-1,1] ->
 * HWC uint8, ((x+1)/2*255) clipped and truncated. */
int ppst_tensor2im_u8(const void* x, void* y, int B, int C, int H, int W, void* stream);
/* colour-guided filter (photo_gif.py:43 cv2.ximgproc.guidedFilter): guide, src
 * uint8 HWC [B][H][W][3]; out fp32 NCHW = (q/255 - 0.5)*2 as
 * PPSTModel.decode does (ppst_model.py:296-305).  work: >= ppst_guided_filter_ws() bytes.
 * r = 30, 60 and 90 (the radius of 512^2 images and its multiples for 1024^2 and 1536^2) run as two fused launches; every other
 * r <= 64 runs five launches through fp32 planes in the workspace.  PPST_EINVAL, with nothing written: any other r > 64, r <= 0,
 * r >= H, r >= W, W > 2048. */
int64_t ppst_guided_filter_ws(int B, int H, int W);
int ppst_guided_filter(const void* guide_u8, const void* src_u8, void* out, void* out_u8,
                       int B, int H, int W, int r, float eps, void* work, void* stream);
/* tuning aid (process-wide, diagnostic like ppst_prof_enable): rows per block of the two fused launches, for all three fused radii;
 * 0 = the library's default for that radius, 32 / 64 / 128 = forced.  Results do not depend on it beyond the rounding of the sliding
 * fp32 sums of the second launch. */
int ppst_guided_filter_tune(int vs1, int vs2);
/* native-size output of the filter (He and Sun, "Fast Guided Filter", arXiv:1505.00996): the mean coefficient planes of the filter
 * at (h, w), then their bilinear upsample applied to a guide of (H, W) >= (h, w).
 * ppst_guided_filter_coeffs: guide, src uint8 [B][h][w][3] -> coeffs fp32 [B][12][h][w], plane 4c + k: k = 0..2 the mean of a_ck,
 * k = 3 the mean of b_c (q_c = sum_k a_ck I_k + b_c).  Five launches through fp32 planes at every radius it accepts; work:
 * >= ppst_guided_filter_ws(B, h, w) bytes.  PPST_EINVAL, with nothing written: r <= 0, r > 64 (90 included), r >= h, r >= w, w > 2048.
 * ppst_guided_filter_apply: coeffs [B][12][h][w], guide uint8 [B][H][W][3] -> out_u8 [B][H][W][3] and / or out_f32 NCHW
 * (q/255 - 0.5)*2 of the stored byte (either may be NULL, not both).  Bilinear taps with half-pixel centres and edge replication
 * (F.interpolate(mode="bilinear", align_corners=False)) at positions computed in integers, horizontally then vertically; any ratio
 * H/h >= 1 and W/w >= 1 per axis.  PPST_EINVAL, with nothing written: H < h, W < w, H W > 2^28. */
int ppst_guided_filter_coeffs(const void* guide_u8, const void* src_u8, void* coeffs, int B, int h, int w, int r, float eps,
                              void* work, void* stream);
int ppst_guided_filter_apply(const void* coeffs, int h, int w, const void* guide_u8, void* out_u8, void* out_f32,
                             int B, int H, int W, void* stream);
/* the filter's coefficients applied INSIDE a photograph: coeffs fp32 [B][12][n][n] (ppst_guided_filter_coeffs of an n x n crop
 * taken by ppst_extract_similarity), photo uint8 [B][H][W][3], the crop's transforms (xf_host / xf_dev as there) -> out_u8
 * [B][H][W][3], which may be photo_u8 itself.  Only photo pixels inside the crop square 0 <= U, V < n 2^24 are written: the
 * caller's out_u8 keeps every other byte (copy the photo into it first, or work in place); one launch over the tiles of the
 * quads' bounding boxes.  Inside: the 12 coefficients by bilinear interpolation at (U / 2^24 - 1/2, V / 2^24 - 1/2) -- tap
 * floor by an arithmetic shift of the integer, fraction = its low 24 bits / 2^24, taps clamped to [0, n - 1], horizontally
 * first, then vertically --, q_c = A_c0 I0 + A_c1 I1 + A_c2 I2 + B_c on the photo's own pixel I, and
 * out = clamp(rint(g q + (1 - g) I), 0, 255), g = t^2 (3 - 2t), t = clamp(d / feather, 0, 1),
 * d = min(U, n 2^24 - U, V, n 2^24 - V) / 2^24; feather = 0: g = 1.
 * PPST_EINVAL, with nothing written: n <= 0, n > 4096, feather < 0, 2 feather > n, H W > 2^28, a transform refused by
 * ppst_extract_similarity. */
int ppst_guided_filter_paste(const void* coeffs, int n, const void* photo_u8, void* out_u8, int B, int H, int W,
                             const void* xf_host, const void* xf_dev, int feather, void* stream);
/* the same paste through a matte: matte_f32 fp32 [B][n][n] in the crop's frame (ppst_label_matte, or the caller's own, whose
 * values the caller keeps in [0, 1]: nothing is clamped here).  ppst_guided_filter_paste's arithmetic with g = g_edge * m^, m^ the
 * matte sampled by the same taps, fractions and clamps as the 12 coefficient planes (horizontally, then vertically);
 * out = clamp(rint(g q + (1 - g) I), 0, 255).  A pixel with g == 0 is NOT written: its byte stays the caller's, and a non-finite
 * coefficient where the matte is 0 cannot leak.  The refusals of ppst_guided_filter_paste, and PPST_ENULL for a null matte. */
int ppst_guided_filter_paste_matte(const void* coeffs, const void* matte_f32, int n, const void* photo_u8, void* out_u8, int B, int H,
                                   int W, const void* xf_host, const void* xf_dev, int feather, void* stream);
/* a matte refined by the photo's own pixels (He et al.'s "guided feathering": a coarse mask filtered with the image as guide; the
 * refined alpha a . I + b follows the image's edges).
 * ppst_guided_matte_coeffs: guide uint8 [B][h][w][3] (the crop), matte_f32 fp32 [B][h][w] -> mcoeffs fp32 [B][4][h][w]: plane
 * k = 0..2 the window mean of a_k, plane 3 the window mean of b.  The source is p = rintf(255 fminf(fmaxf(m, 0), 1)): an integer
 * in 0..255, ties to even, a NaN gives 0 (8 bits keep every stage-1 row sum an exact integer in fp32, as the colour entry relies
 * on).  The filter is the colour guided filter of ppst_guided_filter_coeffs with this one source channel: the same windows
 * (radius r, symmetric border), the same eps on the covariance diagonal, the same solve and the same second box mean, and the
 * result is BIT-EQUAL to planes 0..3 of ppst_guided_filter_coeffs(guide, src) with src[..., c] = p for all three c -- a matte does
 * not depend on which entry computed it -- through 13 of its 21 moment planes and 4 of its 12 coefficient planes.  work:
 * >= ppst_guided_matte_ws(B, h, w) bytes; five launches, nothing allocated.  The refusals of ppst_guided_filter_coeffs, nothing
 * written: PPST_EINVAL for r <= 0, r > 64, r >= h, r >= w, w > 2048; PPST_ENULL for a null pointer.
 * ppst_guided_filter_paste_gmatte: ppst_guided_filter_paste_matte's arithmetic with one change: the four planes mcoeffs
 * [B][4][n][n] are sampled at the photo pixel by the same taps, fractions and clamps as the 12 colour planes, giving
 * (M0, M1, M2, Mb), and m^ = fminf(fmaxf((M0 I0 + M1 I1 + M2 I2 + Mb) (1/255), 0), 1) with I the photo's own pixel (a NaN gives
 * 0); g = g_edge m^, and a pixel with g == 0 is not written.  weight_u8 uint8 [B][H][W] (NULL: no weight output) receives
 * rint(255 g) for every pixel inside the square, 0 where g == 0 included; nothing is written outside the square.  The refusals of
 * ppst_guided_filter_paste_matte. */
int64_t ppst_guided_matte_ws(int B, int h, int w);
int ppst_guided_matte_coeffs(const void* guide_u8, const void* matte_f32, void* mcoeffs, int B, int h, int w, int r, float eps,
                             void* work, void* stream);
int ppst_guided_filter_paste_gmatte(const void* coeffs, const void* mcoeffs, int n, const void* photo_u8, void* out_u8, void* weight_u8,
                                    int B, int H, int W, const void* xf_host, const void* xf_dev, int feather, void* stream);
/* a feathered matte from a label map: the exact, clipped, signed Euclidean distance transform of "label kept", then a smoothstep.
 * labels_u8 uint8 [B][h][w]; a pixel is INSIDE iff its label L < 32 and bit L of ``keep`` is set (labels >= 32 are outside whatever
 * keep says).  R = max(grow, max(feather - grow, 0)) + 1.  D2(p) = min(R^2, min |p - q|^2) over the pixels q OF THE PLANE whose
 * inside-ness differs from p's (the plane's edge is no boundary; no such pixel: D2 = R^2).  sd2_i32 int32 [B][h][w] = + D2 for an
 * inside pixel, - D2 for an outside one (exact).  sd = sign (sqrt(D2) - 1/2): the boundary lies midway between pixel centres.
 * matte_f32 fp32 [B][h][w] (may be NULL): feather > 0: t = clamp((sd + grow) / feather, 0, 1), m = t^2 (3 - 2t); feather == 0:
 * m = 1 if sd + grow > 0, else 0.  grow = 0 feathers inwards only (outside pixels get exactly 0); grow = feather / 2 centres the
 * ramp on the boundary.  Clipping at R^2 never changes m (csrc/matte.hip shows why).  Two launches, nothing allocated: sd2_i32 is
 * required and holds the packed column distances between them.
 * PPST_EINVAL: B < 0, h or w outside [1, 4096], feather or grow outside [0, 255].  B == 0: PPST_OK before any pointer is looked
 * at.  PPST_ENULL: labels_u8 or sd2_i32 NULL.  Nothing is launched in any of these cases. */
int ppst_label_matte(const void* labels_u8, int B, int h, int w, unsigned int keep, int feather, int grow, void* sd2_i32,
                     void* matte_f32, void* stream);

/* local-affine photo smoothing (smooth_filter.py:332-378 smooth_local_affine and its three NVRTC kernels :149-321):
 * output (stylised), input (content = guide), result: planar fp32 [B][3][H][W]; model_ws: >= ppst_smooth_local_affine_ws()
 * bytes, 16-B aligned (the per-pixel 3x4 maps); filtered_model: optional [B][H*W][12] fp32 (the smoothed maps), or NULL.
 * patch_radius = (patch - 1) / 2, filter_radius = f_r, sigma1 = f_r / 3, sigma2 = f_e as the reference's driver sets them. */
int64_t ppst_smooth_local_affine_ws(int B, int H, int W);
int ppst_smooth_local_affine(const void* output, const void* input, void* result, void* model_ws, void* filtered_model,
                             int B, int H, int W, int patch_radius, int filter_radius, float sigma1, float sigma2,
                             void* stream);

/* ------------------------------------------------- train step (backward) ---
 * Gradients of the discriminator update (optimizers/ppst_optimizer.py:96-130; torch autograd
 * of F.conv2d / F.linear in stylegan2_layers.py).  The conv INPUT gradient is
 * ppst_conv2d_mfma itself on a transposed/flipped pack of the weights. */
/* conv weight gradient, exact-fp32 MFMA, reduction over pixels; shares the forward step table
 * (steps: device ppst_conv_step[nsteps]; chunk_start: device int32[nchunks+1], steps of one
 * chunk share chan_off, at most 9 per chunk).  partial: [splits][nsteps][cout][32] fp32. */
int ppst_conv_wgrad_f32(const void* x, const void* dy, const void* steps, const void* chunk_start,
                        void* partial, int B, int in_h, int in_w, int in_ld, int oh, int ow,
                        int dy_ld, int cout, int nsteps, int nchunks, int splits, void* stream);
/* the same gradient on the bf16 matrix pipe (the production path; ppst_conv_wgrad_f32 stays the exact verification path):
 * fp32-class through the bf16 hi / lo split of both operands, three MFMA passes, fp32 accumulation.  Rows must be 16-B aligned,
 * taps in [-1,1]^2.  Raw fp32 tiles arrive by LDS-DMA and are converted to hi | lo in place in LDS (49 KB per 256-thread block),
 * the MFMA operands come from transposed LDS reads (ds_read_b64_tr_b16); two blocks per CU: the
 * phases of one block (request, wait, convert, MFMA) overlap the other block's.  ``splits`` = partial slots = pixel ranges (any
 * positive count); csum NULL or [splits][cout]: partial fp32 column sums of dy, fused into the conversion pass -- summed over
 * the rows (ppst_wgrad_scatter) they are the bias gradient.  max_taps / min_taps: longest / shortest chunk of the step table (0 = unknown):
 * <= 4 and an even chunk count select the two-chunks-per-block form, min == max == 9 (or 4) the form without per-tap tests.
 * halo: 1 in general; 0 = every step has offset (0, 0) and the input has the output's extent (1x1 convs): with one step per
 * chunk the block then stages no halo and takes four (two) chunks per dY image.
 * passes: 3 = bf16x3 (fp32-class), 1 = single-pass bf16 (precision mode 1: the
 * "bf16 compute, fp32 master weights" of BASELINE configs[3]); anything else PPST_EINVAL. */
int ppst_conv_wgrad_tr2(const void* x, const void* dy, const void* steps, const void* chunk_start, void* partial, void* csum,
                        int B, int in_h, int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps, int nchunks,
                        int splits, int max_taps, int min_taps, int halo, int passes, void* stream);   /* max_taps: 0 = unknown (<= 9); 1..4 = the caller's promise that
                        no chunk of the table has more steps: with an even chunk count two chunks then share one block / dY image */
/* dw[n*sn + (src_c+k)*sc + ky*sy + kx*sx] (+)= scale * sum_splits partial[.][step][n][k] */
int ppst_wgrad_scatter(const void* partial, const void* src_c, const void* src_ky, const void* src_kx,
                       void* dw, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int cout, int nsteps,
                       int splits, float scale, int accumulate, const void* csum, void* db, int csum_rows, int db_accumulate,
                       void* stream);   /* csum (NULL or [csum_rows][cout] from ppst_conv_wgrad_tr2 / ppst_conv_wgrad_tr2_st): db[n] (+)= sum of its rows */
/* FromRGB (Cin <= 4) weight gradient: dw[n][c] (+)= scale * sum_p dy[p][n]*x[p][c] */
int64_t ppst_wgrad_small_cin_ws(int64_t npix, int cin, int cout);
int ppst_wgrad_small_cin(const void* x, const void* dy, void* dw, void* ws, int64_t npix, int cin,
                         int in_ld, int cout, float scale, int accumulate, void* stream);
/* out[c] (+)= scale * sum_rows x[row][c]  (bias gradients) */
int64_t ppst_colsum_ws(int64_t rows, int C);
int ppst_colsum(const void* x, void* out, void* ws, int64_t rows, int C, int ld, float scale,
                int accumulate, void* stream);
/* F.linear gradients: dW[n][k] (+)= scale*sum_b dY[b][n] X[b][k];  dX[b][k] = scale*sum_n dY[b][n] W[n][k] */
int ppst_linear_wgrad(const void* dy, const void* x, void* dw, int B, int N, int K, float scale,
                      int accumulate, void* stream);
/* ws: ppst_linear_dgrad_ws(B, N, K) bytes of scratch (partial sums over row slices, reduced in a fixed order) */
int64_t ppst_linear_dgrad_ws(int B, int N, int K);
int ppst_linear_dgrad(const void* dy, const void* w, void* dx, void* ws, int B, int N, int K, float scale,
                      void* stream);
/* Round 5: the two linear gradients with the passes around them folded in (the E2 projector chains, encoder_col.py:47-93, ran seven
 * launches per linear and backward).  ppst_linear_wgrad_fused: ``relu_in`` reads x as max(x, 0) (the linear sits behind nn.ReLU);
 * ``db`` (optional, [N]) receives bscale * sum_b dy[b][n] (written, or added with b_accumulate); K % 4 == 0, 16-byte aligned x / dw.
 * ppst_linear_dgrad_gate: dx[b][k] = [gate[b][k] > 0] * scale * sum_n dy[b][n] w[n][k] (the ReLU's backward rides on the slice
 * reduction); ws as ppst_linear_dgrad_ws. */
int ppst_linear_wgrad_fused(const void* dy, const void* x, void* dw, void* db, int B, int N, int K, float scale, float bscale,
                            int accumulate, int b_accumulate, int relu_in, void* stream);
int ppst_linear_dgrad_gate(const void* dy, const void* w, void* dx, void* ws, const void* gate, int B, int N, int K, float scale,
                           void* stream);
/* LSGAN (models/networks/loss.py:11-18): loss = weight*mean((p-target)^2), grad = d loss / d p */
/* torch.nn.L1Loss (mean |a-b|) times weight -> out[0]; ws >= ppst_l1_mean_ws(n) bytes (ppst_model.py:47,183,203). */
int64_t ppst_l1_mean_ws(int64_t n);
int ppst_l1_mean(const void* a, const void* b, void* out, void* ws, int64_t n, float weight, void* stream);
/* rsclLoss.forward (networks/rscl.py:42-64): q, k [n][C] rows, k0 [n0][C] extra negatives, queue [C][K]; out[0] = mean
 * cross entropy at temperature nce_T with the reference's quirk that all n current-batch logits are -10 (its eye(1)
 * mask broadcasts).  n <= 64, K + n0 <= 512; ws >= n floats. */
int ppst_rscl_loss(const void* q, const void* k, const void* k0, const void* queue, void* out, void* ws,
                   int n, int n0, int C, int K, float nce_T, void* stream);
int ppst_lsgan(const void* pred, void* loss, void* grad, int n, float target, float weight, void* stream);
/* torch.optim.Adam step (ppst_optimizer.py:34-49), step counted from 1 */
int ppst_adam_step(void* p, const void* g, void* m, void* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, int step, void* stream);

/* ---- generator / encoder update of the train step (optimizers/ppst_optimizer.py:73-94: g_loss.backward()
 * through models/ppst_model.py:161-235).  These replace what torch autograd derives for the reference's
 * InstanceNorm2d + StyleMod (stylegan2_layers.py:361-374, 414-437), F.pad(reflect / replicate), F.interpolate,
 * adaptive avg / max pooling (encoder_col.py:150-251), F.normalize / util.normalize (util/util.py:18-22), L1Loss,
 * softmax and PReLU.  Conv input / weight gradients reuse ppst_conv2d_mfma / ppst_conv_wgrad_f32 with other step
 * tables. ---- */
/* ppst_in_finalize that also returns mean_rstd [B][C][2] (needed by the backward of the norm) */
int ppst_in_finalize_train(const void* partial, int n_partials, const void* style, int style_ld, const void* post_bias,
                           void* scale_shift, void* mean_rstd, int B, int C, double count, float eps, void* stream);
/* instance-norm backward, pass 1: partial [B][n][C][2] = (sum g', sum g'*y) over pixel chunks; g' = g, or with
 * `gate` (the activation FOLLOWS the norm, ConvLayer norm='in') g * lrelu'(gate).  x == partial == NULL: size query. */
int ppst_dual_stats(const void* g, const void* y, const void* gate, void* partial, int B, int64_t hw, int C, int g_ld, int y_ld,
                    int gate_ld, int* n_partials, void* stream);
/* pass 2: coef [B][C][4] = (k0, k1, k2, 0) with dy = k0*g' + k1*y + k2; dstyle [B][2C] = (sum g*n, sum g) when given
 * (style = the StyleMod linear output [B][>=C], row stride style_ld; NULL = no modulation).  mean_rstd == NULL:
 * no norm -- dstyle = (sum g*y, sum g) only (SpatialCodeModulation scale / shift gradient, generator.py:80-91). */
int ppst_in_bwd_finalize(const void* partial, int n_partials, const void* mean_rstd, const void* style, int style_ld, void* coef,
                         void* dstyle, int B, int C, double count, void* stream);
/* pass 3: dx = post * (k0*g' + k1*y + k2); post = lrelu'(y) when post_gate (StyledConv: activation before the norm) */
int ppst_in_bwd_apply(const void* g, const void* y, const void* gate, const void* coef, void* dx, int B, int64_t hw, int C, int g_ld,
                      int y_ld, int gate_ld, int dx_ld, int post_gate, void* stream);
/* PReLU backward over z = a*y + s [+ res]: gpre = g * (z >= 0 ? 1 : slope) (dense [.,C]); ws receives per-block partial
 * sums of dslope = sum g*z*[z<0] (ppst_prelu_bwd_ws bytes; reduce with ppst_sum_partials) */
int64_t ppst_prelu_bwd_ws(int64_t total_elements);
int ppst_prelu_bwd(const void* g, const void* y, const void* scale_shift, const void* res, const void* prelu, void* gpre, void* ws,
                   int B, int64_t hw, int C, int g_ld, int y_ld, int res_ld, void* stream);
int ppst_sum_partials(const void* partial, void* out, int n, float scale, void* stream);
/* F.pad (PPST_PAD_*) of an NHWC tensor and its adjoint (dx = sum of dy over the padded positions that read it) */
int ppst_pad2d(const void* x, void* y, int B, int H, int W, int C, int x_ld, int py0, int py1, int px0, int px1, int mode,
               void* stream);
int ppst_pad2d_bwd(const void* dy, void* dx, int B, int H, int W, int C, int py0, int py1, int px0, int px1, int mode, void* stream);
/* adjoints of ppst_bilinear (dx must be zero-initialised; float atomics), ppst_avgpool and ppst_gap_gmp
 * (v = the forward's [B][2C] output, g = its gradient; the max routes to the FIRST maximal pixel like nn.AdaptiveMaxPool2d;
 * accumulate != 0 adds into dx) */
int ppst_bilinear_bwd(const void* dy, void* dx, int B, int H, int W, int C, int dx_ld, int OH, int OW, int dy_ld, void* stream);
int ppst_avgpool_bwd(const void* dy, void* dx, int B, int H, int W, int C, int dx_ld, int f, int dy_ld, void* stream);
int ppst_gap_gmp_bwd(const void* x, const void* mask, const void* v, const void* g, void* dx, void* arg_ws /* B*C int32 */, int B,
                     int64_t hw, int C, int ld, int accumulate, void* stream);
/* Round 5: GAP || GMP of x * mask (encoder_col.py:162-168, 217-245) for SEVERAL masks in one read of the feature map, and its adjoint
 * in one pass.  heads: h = 0 the unmasked pooling (with_plain = 1), then one per channel of masks [B][hw][nm] (nm in 1..3: the NHWC
 * planes of the one-hot mask pyramid); out / v / g are [(nm + with_plain) * B][2C], head-major.  A head's forward values are the
 * single-head launch's bit for bit (same block geometry and summation order); the backward writes the SUM over the heads once
 * (accumulate: adds into dx).  C % 4 == 0, 16-byte aligned rows; the backward needs hw % 16 == 0.
 * ws: ppst_gap_gmp_multi_ws bytes; arg_ws: (nm + with_plain) * B * C ints. */
int64_t ppst_gap_gmp_multi_ws(int B, int64_t hw, int C, int heads);
int ppst_gap_gmp_multi(const void* x, const void* masks, void* out, void* ws, int B, int H, int W, int C, int ld, int nm,
                       int with_plain, int x_st, void* stream);
int ppst_gap_gmp_multi_bwd(const void* x, const void* masks, const void* v, const void* g, void* dx, void* arg_ws, int B, int64_t hw,
                           int C, int ld, int nm, int with_plain, int accumulate, int st /* x and dx */, void* stream);
/* backward of ppst_l2norm_rows (mode 0: util.normalize, 1: F.normalize), ppst_softmax_rows (in place on g) and
 * ppst_corr_prep (ppst_model.py:343-356) */
int ppst_l2norm_rows_bwd(const void* g, const void* x, void* dx, int B, int K, float eps, int mode, void* stream);
int ppst_softmax_rows_bwd(const void* p, void* g, int64_t rows, int cols, float div, void* stream);
int ppst_corr_prep_bwd(const void* g, const void* x, void* dx, int64_t rows, int C, int ncenter, float eps, void* stream);
/* d(weight * mean|a-b|)/da */
int ppst_l1_grad(const void* a, const void* b, void* da, int64_t n, float weight, void* stream);
/* backward of ppst_rscl_loss wrt the queries (keys / queue are detached, ppst_model.py:214-217): dq (n, C); gout = d/d(loss) (1) */
int ppst_rscl_loss_bwd(const void* q, const void* k, const void* k0, const void* queue, const void* gout, void* dq, int n, int n0,
                       int C, int K, float nce_T, void* stream);
/* backward of ppst_rselfcorr: dfea [B][H][W][64] from dout [B][H/4][W/4][>=256] (pixel stride dout_ld) */
int ppst_rselfcorr_bwd(const void* fea, const void* dout, void* dfea, int B, int H, int W, int C, int dout_ld, void* stream);
/* y = x * s[0], s a device scalar (chain rule through a scalar loss) */
int ppst_scale_by(const void* x, const void* s, void* y, int64_t n, void* stream);
/* NoiseInjection weight gradient: out[0] = sum dpre[p][c] * noise[p] (stylegan2_layers.py:376-399) */
int64_t ppst_noise_wgrad_ws(int64_t npix);
int ppst_noise_wgrad(const void* dpre, const void* noise, void* out, void* ws, int64_t npix, int C, int ld, int accumulate, void* stream);
/* adjoint of ppst_upscale_weight: dw4 (Cin,Cout,4,4) -> dw (Cout,Cin,3,3); accumulate != 0 adds into dw (like the other
 * parameter-gradient entry points: the trainers point them at the flat gradient buffer, no separate accumulation pass) */
int ppst_upscale_weight_bwd(const void* dw4, void* dw, int cout, int cin, float scale, int accumulate, void* stream);
/* NHWC [B][H][W][C] -> space-to-depth [B][ceil(H/2)][ceil(W/2)][4C] (channel block (py*2+px)*C) */
int ppst_space_to_depth(const void* x, void* y, int B, int H, int W, int C, int x_ld, void* stream);

/* ---------------------------------------------------------- profiling ----
 * Opt-in HIP-event timing of the conv launches (bench.py roofline): when
 * enabled every ppst_conv2d_mfma call is bracketed by events on its stream. */
int ppst_prof_enable(int on);
/* launches that were NOT bracketed since the last enable because the event pool was full */
int ppst_prof_dropped(void);
/* after a stream sync: total ms, launches, algorithmic flop of bracketed calls */
int ppst_prof_collect(double* ms, int64_t* launches, double* flop);
/* per-launch detail of bracketed call idx (before ppst_prof_collect resets the pool):
 * info = {B, tile_h, tile_w, nsteps, cout, n_groups, halo, bn}; a ppst_conv_wgrad_tr2 / ppst_conv_wgrad_tr2_st launch is bracketed too, with
 * info = {B, oh, ow, nsteps, cout, nchunks, splits, 0} (bn = 0 marks it) */
int ppst_prof_detail(int idx, double* ms, double* flop, int32_t* info);
/* profiling only: number of steps of the NEXT weight-gradient launch that carry real weights (default: all of them) */
int ppst_wgrad_flop_steps(int flop_steps);

/* ---- Round 5: half-precision storage of the TRAINING activations and their gradients (precision mode 1: BASELINE configs[3]'s
 * "bf16" -- the accuracy class of bf16 autocast, where conv outputs and their gradients are bfloat16 tensors).  `_st` twins of the
 * backward kernels: ``st`` = the storage type (PPST_ST_*) of every ACTIVATION-shaped tensor of the call (inputs, gradients, outputs);
 * partial sums, coefficient tables, parameter gradients and pooled vectors stay fp32.  Arithmetic in fp32, one rounding at the store
 * (the contract of the forward `_st` kernels).  With st = PPST_ST_F32 each IS its plain form.  Half tensors: C and every leading
 * dimension a multiple of 4, 8-byte aligned. */
int ppst_dual_stats_st(const void* g, const void* y, const void* gate, void* partial, int B, int64_t hw, int C, int g_ld, int y_ld,
                       int gate_ld, int* n_partials, int st, void* stream);
int ppst_in_bwd_apply_st(const void* g, const void* y, const void* gate, const void* coef, void* dx, int B, int64_t hw, int C, int g_ld,
                         int y_ld, int gate_ld, int dx_ld, int post_gate, int st, void* stream);
int ppst_pad2d_st(const void* x, void* y, int B, int H, int W, int C, int x_ld, int py0, int py1, int px0, int px1, int mode, int st,
                  void* stream);
int ppst_pad2d_bwd_st(const void* dy, void* dx, int B, int H, int W, int C, int py0, int py1, int px0, int px1, int mode, int st,
                      void* stream);
int ppst_bilinear_bwd_st(const void* dy, void* dx, int B, int H, int W, int C, int dx_ld, int OH, int OW, int dy_ld, int st, void* stream);
int ppst_gap_gmp_bwd_st(const void* x, const void* mask, const void* v, const void* g, void* dx, void* arg_ws, int B, int64_t hw, int C,
                        int ld, int accumulate, int st, void* stream);          /* st: x and dx */
int ppst_noise_wgrad_st(const void* dpre, const void* noise, void* out, void* ws, int64_t npix, int C, int ld, int accumulate, int st,
                        void* stream);                                          /* st: dpre */
int ppst_space_to_depth_st(const void* x, void* y, int B, int H, int W, int C, int x_ld, int st, void* stream);
int ppst_colsum_st(const void* x, void* out, void* ws, int64_t rows, int C, int ld, float scale, int accumulate, int st, void* stream);
int ppst_wgrad_small_cin_st(const void* x, const void* dy, void* dw, void* ws, int64_t npix, int cin, int in_ld, int cout, float scale,
                            int accumulate, int dy_st, void* stream);           /* x stays fp32 (the image / RGB gradient) */
/* ppst_conv_wgrad_tr2 on bf16-STORED operands (st = PPST_ST_BF16, passes = 1 only): the tiles arrive as the MFMA operand type by
 * LDS-DMA -- half the bytes of the fp32 tiles, no conversion pass, double-buffered images (conv_wgrad_tr2b_kernel).  cout, in_ld and
 * dy_ld multiples of 8, x / dy 16-byte aligned.  partial / csum as ppst_conv_wgrad_tr2. */
int ppst_conv_wgrad_tr2_st(const void* x, const void* dy, const void* steps, const void* chunk_start, void* partial, void* csum, int B,
                           int in_h, int in_w, int in_ld, int oh, int ow, int dy_ld, int cout, int nsteps, int nchunks, int splits,
                           int max_taps, int min_taps, int halo, int passes, int st, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PPST_HIP_H */
