// Small-batch linear layers (weight-read bound GEMV batches) and row normalisation.
// y[b][n] = act( sum_k f(x[b][k]) * w[n][k] * wscale + bias[n] * bscale )
// Covers EqualLinear (stylegan2_layers.py:222-242), EqualizedLinear/StyleMod (:268-273,
// :364-374), GeneratorModulation (generator.py:80-91) and the nn.Linear chain of the E2
// projectors (encoder_col.py:52-88).  One wave per output row n streams the weight row
// once with 16-B loads (algorithmic bytes = 4*N*K, x stays L1/L2 resident) and keeps one
// accumulator per batch row; xor-shuffle reduction at the end.
#include "common.h"

#define LIN_BMAX 16

// Which kernel form and batch tile a launch of (nb batch rows, K, N) takes: ONE rule for ppst_linear and ppst_linear_grouped.
static inline bool lin_ksplit(int K, int N) { return K >= 1024 && (K & 3) == 0 && N <= 8192; }
static inline int lin_bt(int nb) { return nb <= 1 ? 1 : nb <= 2 ? 2 : nb <= 4 ? 4 : nb <= 8 ? 8 : 16; }

// The per-block bodies.  `blk` is the block's index inside ITS problem: blockIdx.x of a single launch, blockIdx.x minus the
// problem's first block inside a grouped launch -- the arithmetic of an output element is the same instructions either way.
template <int BT>
__device__ __forceinline__ void linear_rows_body(const float* __restrict__ x, const float* __restrict__ w,
                                                 const float* __restrict__ bias, float* __restrict__ y, int B, int K, int N,
                                                 float wscale, float bscale, int relu_in, int act, int b0, int blk) {
  const int lane = threadIdx.x & 63;
  const int n = blk * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  float acc[BT];
#pragma unroll
  for (int b = 0; b < BT; ++b) acc[b] = 0.f;
  const float* wr = w + (int64_t)n * K;
  if ((K & 3) == 0) {
    for (int k = lane * 4; k < K; k += 256) {
      float4 ww = *(const float4*)(wr + k);
#pragma unroll
      for (int b = 0; b < BT; ++b) {
        if (b0 + b < B) {
          float4 xv = *(const float4*)(x + (int64_t)(b0 + b) * K + k);
          if (relu_in) { xv.x = fmaxf(xv.x, 0.f); xv.y = fmaxf(xv.y, 0.f); xv.z = fmaxf(xv.z, 0.f); xv.w = fmaxf(xv.w, 0.f); }
          acc[b] += xv.x * ww.x + xv.y * ww.y + xv.z * ww.z + xv.w * ww.w;
        }
      }
    }
  } else {
    for (int k = lane; k < K; k += 64) {
      float ww = wr[k];
#pragma unroll
      for (int b = 0; b < BT; ++b)
        if (b0 + b < B) {
          float xv = x[(int64_t)(b0 + b) * K + k];
          if (relu_in) xv = fmaxf(xv, 0.f);
          acc[b] += xv * ww;
        }
    }
  }
#pragma unroll
  for (int b = 0; b < BT; ++b) acc[b] = wave_sum(acc[b]);
  if (lane == 0) {
    float bb = bias ? bias[n] * bscale : 0.f;
#pragma unroll
    for (int b = 0; b < BT; ++b)
      if (b0 + b < B) {
        float v = acc[b] * wscale + bb;
        if (act == PPST_ACT_LRELU) v = (v > 0.f ? v : v * 0.2f) * 1.41421356237309515f;
        y[(int64_t)(b0 + b) * N + n] = v;
      }
  }
}

// Same contract, long rows (K >= 1024, K % 4 == 0): the 4 waves of a block share ONE output row
// (each streams a quarter of it), so a 512-row layer runs 512 blocks instead of 128 -- the
// one-wave-per-row form leaves half the CUs idle on the StyleMod / projector GEMVs.
template <int BT>
__device__ __forceinline__ void linear_ksplit_body(const float* __restrict__ x, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ y, int B, int K, int N,
                                                   float wscale, float bscale, int relu_in, int act, int b0, int blk) {
  __shared__ float sm[4][BT];
  const int n = blk;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float acc[BT];
#pragma unroll
  for (int b = 0; b < BT; ++b) acc[b] = 0.f;
  const float* wr = w + (int64_t)n * K;
  for (int k = threadIdx.x * 4; k < K; k += 1024) {
    float4 ww = *(const float4*)(wr + k);
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      if (b0 + b < B) {
        float4 xv = *(const float4*)(x + (int64_t)(b0 + b) * K + k);
        if (relu_in) { xv.x = fmaxf(xv.x, 0.f); xv.y = fmaxf(xv.y, 0.f); xv.z = fmaxf(xv.z, 0.f); xv.w = fmaxf(xv.w, 0.f); }
        acc[b] += xv.x * ww.x + xv.y * ww.y + xv.z * ww.z + xv.w * ww.w;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BT; ++b) acc[b] = wave_sum(acc[b]);
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < BT; ++b) sm[wv][b] = acc[b];
  }
  __syncthreads();
  if (threadIdx.x < BT && b0 + (int)threadIdx.x < B) {
    const int b = threadIdx.x;
    float v = ((sm[0][b] + sm[1][b]) + (sm[2][b] + sm[3][b])) * wscale + (bias ? bias[n] * bscale : 0.f);
    if (act == PPST_ACT_LRELU) v = (v > 0.f ? v : v * 0.2f) * 1.41421356237309515f;
    y[(int64_t)(b0 + b) * N + n] = v;
  }
}

template <int BT>
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ y, int B, int K,
                                                     int N, float wscale, float bscale, int relu_in, int act, int b0) {
  linear_rows_body<BT>(x, w, bias, y, B, K, N, wscale, bscale, relu_in, act, b0, blockIdx.x);
}
template <int BT>
__global__ __launch_bounds__(256) void linear_ksplit_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y, int B, int K,
                                                            int N, float wscale, float bscale, int relu_in, int act, int b0) {
  linear_ksplit_body<BT>(x, w, bias, y, B, K, N, wscale, bscale, relu_in, act, b0, blockIdx.x);
}

extern "C" int ppst_linear(const void* x, const void* w, const void* bias, void* y, int B, int K, int N, float wscale,
                           float bscale, int relu_in, int act, void* stream) {
  if (B < 0 || K <= 0 || N <= 0) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!x || !w || !y) return PPST_ENULL;
  for (int b0 = 0; b0 < B; b0 += LIN_BMAX) {
    int nb = B - b0 < LIN_BMAX ? B - b0 : LIN_BMAX;
    const bool ksplit = lin_ksplit(K, N);
    dim3 grid(ksplit ? N : cdiv(N, 4));
#define LAUNCH(BT)                                                                                                          \
  do {                                                                                                                      \
    if (ksplit)                                                                                                             \
      PPST_LAUNCH(linear_ksplit_kernel<BT>, grid, dim3(256), 0, as_stream(stream), (const float*)x, (const float*)w,       \
                  (const float*)bias, (float*)y, B, K, N, wscale, bscale, relu_in, act, b0);                                \
    else                                                                                                                    \
      PPST_LAUNCH(linear_kernel<BT>, grid, dim3(256), 0, as_stream(stream), (const float*)x, (const float*)w,              \
                  (const float*)bias, (float*)y, B, K, N, wscale, bscale, relu_in, act, b0);                                \
  } while (0)
    switch (lin_bt(nb)) {
      case 1: LAUNCH(1); break;
      case 2: LAUNCH(2); break;
      case 4: LAUNCH(4); break;
      case 8: LAUNCH(8); break;
      default: LAUNCH(16);
    }
#undef LAUNCH
    int e = PPST_LAUNCH_CHECK();
    if (e) return e;
  }
  return PPST_OK;
}

// ---- several INDEPENDENT linear problems in one launch (the E2 projector levels, the generator's StyleMod set: launches of 8 - 2048
// blocks at 8 - 24 batch rows each, bound by launch latency and not by the weight stream).  A segment is what ONE launch of
// ppst_linear would be -- a problem's batch rows [b0, b0 + 16) -- and runs that launch's body, picked by the same rule; the
// segments' blocks lie one after another in the grid, and a block finds its segment by a scan of the first-block table.  The table
// and the segments are kernel arguments (by value, read with scalar loads): nothing is uploaded.
#define LIN_SEGS 32
struct LinSeg {
  const float* x; const float* w; const float* bias; float* y;
  int B, K, N, b0;
  float wscale, bscale;
  int flags;  // bit 0 relu_in, bit 1 ksplit form, bits 8.. batch tile BT, bits 16.. act
  int pad_;
};
struct LinGroup {
  LinSeg seg[LIN_SEGS];
  int blk0[LIN_SEGS];  // first block of segment i; INT_MAX behind the last one
};
__global__ __launch_bounds__(256) void linear_grouped_kernel(const LinGroup g) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < LIN_SEGS; ++i)
    if ((int)blockIdx.x >= g.blk0[i]) s = i;
  const LinSeg& q = g.seg[s];
  const int blk = (int)blockIdx.x - g.blk0[s];
  const int relu_in = q.flags & 1, act = q.flags >> 16;
#define RUN(BT)                                                                                                             \
  do {                                                                                                                      \
    if (q.flags & 2) linear_ksplit_body<BT>(q.x, q.w, q.bias, q.y, q.B, q.K, q.N, q.wscale, q.bscale, relu_in, act, q.b0, blk); \
    else linear_rows_body<BT>(q.x, q.w, q.bias, q.y, q.B, q.K, q.N, q.wscale, q.bscale, relu_in, act, q.b0, blk);           \
  } while (0)
  switch ((q.flags >> 8) & 0xff) {
    case 1: RUN(1); break;
    case 2: RUN(2); break;
    case 4: RUN(4); break;
    case 8: RUN(8); break;
    default: RUN(16);
  }
#undef RUN
}

static int linear_group_launch(LinGroup& g, int nseg, int64_t nblk, void* stream) {
  if (nseg == 0) return PPST_OK;
  for (int i = nseg; i < LIN_SEGS; ++i) g.blk0[i] = 0x7fffffff;
  PPST_LAUNCH(linear_grouped_kernel, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), g);
  return PPST_LAUNCH_CHECK();
}

extern "C" int ppst_linear_grouped(const ppst_linear_problem* p, int n, void* stream) {
  if (n < 0 || n > PPST_GROUP_MAX) return PPST_EINVAL;
  if (n == 0) return PPST_OK;
  if (!p) return PPST_ENULL;
  for (int i = 0; i < n; ++i) {
    if (p[i].B < 0 || p[i].K <= 0 || p[i].N <= 0) return PPST_EINVAL;
    if (p[i].B > 0 && (!p[i].x || !p[i].w || !p[i].y)) return PPST_ENULL;
  }
  LinGroup g;
  int nseg = 0;
  int64_t nblk = 0;
  for (int i = 0; i < n; ++i) {
    const ppst_linear_problem& q = p[i];
    const bool ksplit = lin_ksplit(q.K, q.N);
    const int blocks = ksplit ? q.N : cdiv(q.N, 4);
    for (int b0 = 0; b0 < q.B; b0 += LIN_BMAX) {
      if (nseg == LIN_SEGS || nblk + blocks > 0x7fffffffll) {   // (problems of more than 16 rows: a full table goes out, the rest follows)
        int e = linear_group_launch(g, nseg, nblk, stream);
        if (e) return e;
        nseg = 0; nblk = 0;
      }
      const int nb = q.B - b0 < LIN_BMAX ? q.B - b0 : LIN_BMAX;
      LinSeg& s = g.seg[nseg];
      s.x = (const float*)q.x; s.w = (const float*)q.w; s.bias = (const float*)q.bias; s.y = (float*)q.y;
      s.B = q.B; s.K = q.K; s.N = q.N; s.b0 = b0;
      s.wscale = q.wscale; s.bscale = q.bscale;
      s.flags = (q.relu_in ? 1 : 0) | (ksplit ? 2 : 0) | (lin_bt(nb) << 8) | (q.act << 16);
      s.pad_ = 0;
      g.blk0[nseg++] = (int)nblk;
      nblk += blocks;
    }
  }
  return linear_group_launch(g, nseg, nblk, stream);
}

// mode 0: y = x * rsqrt(sum x^2 + eps)   (util.normalize, util/util.py:18-22)
// mode 1: y = x / max(sqrt(sum x^2), eps) (F.normalize, encoder_col.py:168)
__device__ __forceinline__ void l2norm_row_body(const float* __restrict__ x, float* __restrict__ y, int K, float eps, int mode, int row) {
  __shared__ float sm[4];
  const float* xr = x + (int64_t)row * K;
  float* yr = y + (int64_t)row * K;
  float s = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) { float v = xr[k]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  s = sm[0] + sm[1] + sm[2] + sm[3];
  float f = mode == 0 ? rsqrtf(s + eps) : 1.f / fmaxf(sqrtf(s), eps);
  for (int k = threadIdx.x; k < K; k += 256) yr[k] = xr[k] * f;
}
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int K, float eps, int mode) {
  l2norm_row_body(x, y, K, eps, mode, blockIdx.x);
}
extern "C" int ppst_l2norm_rows(const void* x, void* y, int B, int K, float eps, int mode, void* stream) {
  if (B < 0 || K <= 0 || mode < 0 || mode > 1) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!x || !y) return PPST_ENULL;
  PPST_LAUNCH(l2norm_rows_kernel, dim3(B), dim3(256), 0, as_stream(stream), (const float*)x, (float*)y, K, eps, mode);
  return PPST_LAUNCH_CHECK();
}

// several independent row normalisations in one launch (the four code vectors of a generator pass, the E2 heads of a pass): one
// block per row as above, problem i owns blocks [blk0[i], blk0[i + 1])
struct L2Seg { const float* x; float* y; int K; float eps; int mode; int pad_; };
struct L2Group { L2Seg seg[PPST_GROUP_MAX]; int blk0[PPST_GROUP_MAX]; };
__global__ __launch_bounds__(256) void l2norm_rows_grouped_kernel(const L2Group g) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < PPST_GROUP_MAX; ++i)
    if ((int)blockIdx.x >= g.blk0[i]) s = i;
  const L2Seg& q = g.seg[s];
  l2norm_row_body(q.x, q.y, q.K, q.eps, q.mode, (int)blockIdx.x - g.blk0[s]);
}
extern "C" int ppst_l2norm_rows_grouped(const ppst_l2norm_problem* p, int n, void* stream) {
  if (n < 0 || n > PPST_GROUP_MAX) return PPST_EINVAL;
  if (n == 0) return PPST_OK;
  if (!p) return PPST_ENULL;
  int64_t rows = 0;
  for (int i = 0; i < n; ++i) {
    if (p[i].B < 0 || p[i].K <= 0 || p[i].mode < 0 || p[i].mode > 1) return PPST_EINVAL;
    if (p[i].B > 0 && (!p[i].x || !p[i].y)) return PPST_ENULL;
    rows += p[i].B;
  }
  if (rows > 0x7fffffffll) return PPST_EINVAL;
  if (rows == 0) return PPST_OK;
  L2Group g;
  int nseg = 0, nblk = 0;
  for (int i = 0; i < n; ++i) {
    if (p[i].B == 0) continue;
    L2Seg& s = g.seg[nseg];
    s.x = (const float*)p[i].x; s.y = (float*)p[i].y; s.K = p[i].K; s.eps = p[i].eps; s.mode = p[i].mode; s.pad_ = 0;
    g.blk0[nseg++] = nblk;
    nblk += p[i].B;
  }
  for (int i = nseg; i < PPST_GROUP_MAX; ++i) g.blk0[i] = 0x7fffffff;
  PPST_LAUNCH(l2norm_rows_grouped_kernel, dim3(nblk), dim3(256), 0, as_stream(stream), g);
  return PPST_LAUNCH_CHECK();
}
