// JPEG decode on the device: baseline sequential DCT files of any origin -> uint8 HWC, equal to libjpeg-turbo's default decoder
// (DESIGN.md "JPEG decode on the device"; the format and arithmetic: include/ppst_hip.h).  A batch holds files of different sizes
// and samplings: every kernel runs on a grid (largest per-image count, B) and a workgroup beyond its image's count leaves.
//   0. plan_kernel<JdImg> one workgroup: every image's geometry, layout and place in the workspace (a serial prefix over the B
//                         images), stored for the other kernels; status and round counts to zero (codec_common.h, with the head
//                         of the workspace and the workgroup scan; the format's part: codec_fill);  jd_zero_kernel: the coefficient arrays to zero
//   1. jd_count_kernel    one workgroup per 4096-byte chunk of the entropy-coded segment: bytes that stay, restart markers
//      jd_offsets_kernel  one workgroup per image: exclusive prefix over the chunks' counts, the marker total against the header's
//      jd_compact_kernel  per chunk again: the clean stream (no stuffed 00, no RSTm), the clean offset behind every RSTm
//   2. jd_entropy_kernel  one workgroup per restart interval: subsequence iteration to the fixed point, block prefix, the write
//                         pass, DC prediction
//   3. jd_idct_kernel     32 blocks per workgroup: dequantise, jidctint columns then rows, planar Y / Cb / Cr padded to whole MCUs
//   4. jd_colour_kernel   one thread per pixel: fancy h2v2 chroma, YCbCr -> RGB, crop, mirror
// Integer code throughout.  No workgroup waits for another: the stages meet at launch boundaries only.
// Shared with the encoder (jpeg_common.h): the zigzag order.
#include "common.h"
#include "codec_common.h"
#include "jpeg_common.h"

#define JD_CHUNK_T 256                         // threads of the stream kernels
#define JD_CHUNK 4096                           // bytes of the segment per workgroup: 16 per thread
#define JD_ENT_T 1024                           // threads of the entropy workgroup
#define JD_IDCT_BLOCKS 32                       // 8 x 8 blocks per IDCT workgroup of 256 threads
#define JD_SUBSEQ_DEFAULT 32                    // words: 1024 bits
#define JD_SUBSEQ_MAX 65536
#define JD_SCAN_MAX (1 << 28)                   // bytes of one file's segment: its bit positions stay below 2^31

// ---------------------------------------------------------------------------------------------------------------- geometry
struct JdGeom {
  int ss, bpm, mw, mh, nmcu, nblk;
  int R, NI;                // MCUs per interval (the whole image without DRI), intervals
  int pwy, phy, pwc, phc;   // plane sizes: luma, chroma (whole MCUs)
  int cout;                 // channels of the output
  unsigned L;               // bytes of the segment
  int nchunk;
  unsigned SB;              // bits per subsequence
  unsigned nsub;            // subsequence slots of the image: floor(8 L / SB) + NI + 1
};
// byte offsets of one image's arrays from its base (each a multiple of 16)
struct JdLayout { int64_t chunk, ivl, clean, sub, coef, plane, total; };

__host__ __device__ inline void jd_geom(const ppst_jpeg_dec_image& d, int sw, JdGeom* g) {
  g->ss = d.ss;
  g->bpm = d.ncomp == 1 ? 1 : (d.ss == 2 ? 6 : 3);
  const int mcu = 8 * d.ss;
  g->mw = (d.W + mcu - 1) / mcu;
  g->mh = (d.H + mcu - 1) / mcu;
  g->nmcu = g->mw * g->mh;
  g->nblk = g->nmcu * g->bpm;
  g->R = (d.dri > 0 && d.dri < g->nmcu) ? d.dri : g->nmcu;
  g->NI = (g->nmcu + g->R - 1) / g->R;
  g->pwy = g->mw * mcu; g->phy = g->mh * mcu;
  g->pwc = g->mw * 8; g->phc = g->mh * 8;
  g->cout = (d.ncomp == 3 || d.expand_grey) ? 3 : 1;
  g->L = (unsigned)d.scan_len;
  g->nchunk = (int)((g->L + JD_CHUNK - 1) / JD_CHUNK);
  if (g->nchunk < 1) g->nchunk = 1;
  g->SB = 32u * (unsigned)(sw > 0 ? sw : JD_SUBSEQ_DEFAULT);
  g->nsub = (unsigned)(((uint64_t)g->L * 8u) / g->SB) + (unsigned)g->NI + 1u;
}

__host__ __device__ inline void jd_layout(const ppst_jpeg_dec_image& d, const JdGeom& g, JdLayout* l) {
  int64_t at = 0;
  l->chunk = at; at = a16(at + (int64_t)g.nchunk * 8);
  l->ivl = at;   at = a16(at + ((int64_t)g.NI + 1) * 4);
  l->clean = at; at = a16(at + (int64_t)g.L + 8);
  l->sub = at;   at = a16(at + (int64_t)g.nsub * 6 * 4);
  l->coef = at;  at = a16(at + (int64_t)g.nblk * 128);
  l->plane = at; at = a16(at + (int64_t)g.pwy * g.phy + (d.ncomp == 3 ? 2 * (int64_t)g.pwc * g.phc : 0));
  l->total = at;
}

struct JdImg {                                  // what a workgroup needs of its image: written once by plan_kernel (codec_common.h)
  JdGeom g;
  JdLayout l;
  int64_t base_off;                             // the image's arrays start here in the workspace
};
__host__ __device__ inline void codec_fill(const ppst_jpeg_dec_image& d, int sw, JdImg* im) {
  jd_geom(d, sw, &im->g);
  jd_layout(d, im->g, &im->l);
}

__global__ __launch_bounds__(256) void jd_zero_kernel(const ppst_jpeg_dec_image* __restrict__ imgs, int B, int sw, void* work) {
  const JdImg& im = open_plan<JdImg>(B, work, blockIdx.y);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  const int64_t n16 = (int64_t)im.g.nblk * 8;                        // 16-byte pieces of the coefficient array
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) ((uint4*)(base + im.l.coef))[i] = make_uint4(0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------------------------- stream
// What byte q of the segment is: 0 stays (data, a data FF included); 1 dropped (the 00 behind an FF, or the FF of a marker);
// 2 dropped, the second byte of RSTm; 3 dropped, and not allowed here.  A byte is a SECOND byte when an odd number of FF bytes
// stand in front of it (looked back over at most 8: more than one only happens in files that are refused anyway, and all that
// matters then is that both passes over the segment decide alike).
__device__ __forceinline__ int jd_class(const unsigned char* __restrict__ s, unsigned q, unsigned L) {
  const int c = s[q];
  unsigned run = 0;
  while (run < 8 && q > run && s[q - 1 - run] == 0xFF) ++run;
  if (run & 1) return c == 0 ? 1 : ((c >= 0xD0 && c <= 0xD7) ? 2 : 3);
  if (c == 0xFF) {
    if (q + 1 >= L) return 3;
    return s[q + 1] == 0 ? 0 : 1;
  }
  return 0;
}

__global__ __launch_bounds__(JD_CHUNK_T) void jd_count_kernel(const unsigned char* __restrict__ bytes, const ppst_jpeg_dec_image* __restrict__ imgs,
                                                              int B, int sw, void* work, int* __restrict__ status) {
  __shared__ int wt[2][JD_CHUNK_T / 64];
  const int i = blockIdx.y;
  const JdImg& im = open_plan<JdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  if ((int)blockIdx.x >= im.g.nchunk) return;
  const unsigned char* s = bytes + imgs[i].file_off + imgs[i].scan_off;
  const unsigned q0 = blockIdx.x * JD_CHUNK + threadIdx.x * 16;
  int kept = 0, rst = 0, bad = 0;
  for (int j = 0; j < 16; ++j) {
    const unsigned q = q0 + j;
    if (q >= im.g.L) break;
    const int c = jd_class(s, q, im.g.L);
    kept += c == 0;
    rst += c == 2;
    bad |= c == 3;
  }
  int tk, tr;
  wg_scan<JD_CHUNK_T, false>(kept, tk, wt, 0);
  wg_scan<JD_CHUNK_T, false>(rst, tr, wt, 1);
  if (threadIdx.x == 0) {
    unsigned* ci = (unsigned*)(base + im.l.chunk);
    ci[2 * blockIdx.x] = (unsigned)tk;
    ci[2 * blockIdx.x + 1] = (unsigned)tr;
  }
  if (bad) atomicOr(&status[i], PPST_JPEG_S_MARKER);
}

__global__ __launch_bounds__(JD_CHUNK_T) void jd_offsets_kernel(const ppst_jpeg_dec_image* __restrict__ imgs, int B, int sw, void* work,
                                                                int* __restrict__ status) {
  __shared__ int wt[2][JD_CHUNK_T / 64];
  const int i = blockIdx.x;
  const JdImg& im = open_plan<JdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  unsigned* ci = (unsigned*)(base + im.l.chunk);
  int base_k = 0, base_r = 0;
  for (int c0 = 0; c0 < im.g.nchunk; c0 += JD_CHUNK_T) {
    const int c = c0 + threadIdx.x;
    const int k = c < im.g.nchunk ? (int)ci[2 * c] : 0, r = c < im.g.nchunk ? (int)ci[2 * c + 1] : 0;
    int tk, tr;
    const int pk = wg_scan<JD_CHUNK_T, false>(k, tk, wt, 0);
    const int pr = wg_scan<JD_CHUNK_T, false>(r, tr, wt, 1);
    if (c < im.g.nchunk) { ci[2 * c] = (unsigned)(base_k + pk); ci[2 * c + 1] = (unsigned)(base_r + pr); }
    base_k += tk; base_r += tr;
    __syncthreads();                                               // wt is reused by the next round
  }
  if (threadIdx.x == 0) {
    unsigned* ivl = (unsigned*)(base + im.l.ivl);
    ivl[0] = 0;
    ivl[im.g.NI] = (unsigned)base_k;
    if (base_r != im.g.NI - 1) atomicOr(&status[i], PPST_JPEG_S_RST_COUNT);
  }
}

__global__ __launch_bounds__(JD_CHUNK_T) void jd_compact_kernel(const unsigned char* __restrict__ bytes, const ppst_jpeg_dec_image* __restrict__ imgs,
                                                                int B, int sw, void* work, int* __restrict__ status) {
  __shared__ int wt[2][JD_CHUNK_T / 64];
  const int i = blockIdx.y;
  const JdImg& im = open_plan<JdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  if ((int)blockIdx.x >= im.g.nchunk) return;
  const unsigned char* s = bytes + imgs[i].file_off + imgs[i].scan_off;
  const unsigned q0 = blockIdx.x * JD_CHUNK + threadIdx.x * 16;
  int cls[16];
  int kept = 0, rst = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned q = q0 + j;
    cls[j] = q < im.g.L ? jd_class(s, q, im.g.L) : 1;
    kept += cls[j] == 0;
    rst += cls[j] == 2;
  }
  int tot;
  const int pos = wg_scan<JD_CHUNK_T, false>(kept | (rst << 16), tot, wt, 0);      // kept <= 4096, markers <= 2048 per chunk
  const unsigned* ci = (const unsigned*)(base + im.l.chunk);
  unsigned at = ci[2 * blockIdx.x] + (unsigned)(pos & 0xFFFF);                      // < L: every kept byte is a byte of the segment
  int ord = (int)ci[2 * blockIdx.x + 1] + (pos >> 16);
  unsigned char* clean = base + im.l.clean;
  unsigned* ivl = (unsigned*)(base + im.l.ivl);
  int bad = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned q = q0 + j;
    if (cls[j] == 0) {
      if (at < im.g.L) clean[at] = s[q];
      ++at;
    } else if (cls[j] == 2) {
      bad |= (s[q] - 0xD0) != (ord & 7);
      if (ord + 1 < im.g.NI) ivl[ord + 1] = at;
      ++ord;
    }
  }
  if (bad) atomicOr(&status[i], PPST_JPEG_S_RST_ORDER);
}

// ------------------------------------------------------------------------------------------------------------------ entropy
struct JdTabs {
  unsigned short lut[4][512];      // the first 9 bits -> (length << 8) | symbol, 0: no code of at most 9 bits
  int maxcode[4][17];              // [length]: the largest code of that length, -1: none
  int valoff[4][17];               // [length]: index of the length's first symbol minus its first code
  unsigned char vals[4][256];
  int slot_dc[6], slot_ac[6];      // block of the MCU -> table
  int wt[2][JD_ENT_T / 64];
  int skip;
};

// 32 bits at bit `p` of the interval (MSB first); bits at and behind `nbits` read as zero.  `origin`: the interval's first bit in
// the image's clean stream, which is read as aligned words (the array is 8 bytes longer than the stream).
__device__ __forceinline__ unsigned jd_peek(const unsigned* __restrict__ cw, unsigned origin, unsigned nbits, unsigned p) {
  if (p >= nbits) return 0u;
  const unsigned a = origin + p, w = a >> 5, sh = a & 31u;
  const unsigned hi = __builtin_bswap32(cw[w]), lo = __builtin_bswap32(cw[w + 1]);
  unsigned v = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
  const unsigned rem = nbits - p;
  if (rem < 32) v &= ~0u << (32 - rem);
  return v;
}

// Decodes from (p, b, k) until p reaches `end`; n counts the blocks completed.  WRITE: coefficients go to coef[blk][k] (blk counts
// from the interval's first block, stores stop at nb blocks), undefined codes and runs beyond the block set `bad`.
struct JdState { unsigned p; int b, k, n, bad; };
template <bool WRITE>
__device__ __forceinline__ JdState jd_run(const JdTabs& T, const unsigned* __restrict__ cw, unsigned origin, unsigned nbits, unsigned end, int bpm,
                                          unsigned p, unsigned bk, short* __restrict__ coef, int blk, int nb) {
  int b = (int)(bk >> 8), k = (int)(bk & 255u), n = 0, bad = 0;
  while (p < end) {
    if (WRITE && blk >= nb) break;
    const unsigned v = jd_peek(cw, origin, nbits, p);
    const int t = k == 0 ? T.slot_dc[b] : T.slot_ac[b];
    const unsigned e = T.lut[t][v >> 23];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (!e) {
      for (int l = 10; l <= 16; ++l) {
        const int code = (int)(v >> (32 - l));
        if (code <= T.maxcode[t][l]) { sym = T.vals[t][(T.valoff[t][l] + code) & 255]; len = l; break; }
      }
    }
    if (!len) {                                   // no such code: one bit on
      if (WRITE) bad = 1;
      p += 1;
      continue;
    }
    p += (unsigned)len;
    const int s = sym & 15;
    int val = 0;
    if (s) {
      const int m = (int)((v << len) >> (32 - s));
      val = (m >> (s - 1)) ? m : m - (1 << s) + 1;
    }
    if (k == 0) {
      p += (unsigned)s;
      if (WRITE) coef[(int64_t)blk * 64] = (short)val;
      k = 1;
    } else if (s == 0) {
      const int r = sym >> 4;
      if (r == 15) {
        if (WRITE && k + 16 > 63) bad = 1;
        k += 16;
      } else {
        if (WRITE && r) bad = 1;                  // EOBn belongs to progressive scans
        k = 64;
      }
    } else {
      k += sym >> 4;
      p += (unsigned)s;
      if (k <= 63) {
        if (WRITE) coef[(int64_t)blk * 64 + k] = (short)val;
      } else if (WRITE) bad = 1;
      k += 1;
    }
    if (k >= 64) {
      k = 0;
      b = b + 1 == bpm ? 0 : b + 1;
      ++n;
      ++blk;
    }
  }
  JdState o = {p, b, k, n, bad};
  return o;
}

__global__ __launch_bounds__(JD_ENT_T) void jd_entropy_kernel(const ppst_jpeg_dec_image* __restrict__ imgs, int B, int sw, void* work,
                                                              int* __restrict__ status) {
  __shared__ JdTabs T;
  const int i = blockIdx.y, it = blockIdx.x, tid = threadIdx.x;
  const JdImg& im = open_plan<JdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  if (it >= im.g.NI) return;
  // the stream stage refused the file: its interval table may be incomplete.  Only the bits earlier launches set are looked at:
  // other intervals of this image may be setting S_CODE / S_BLOCKS right now, and whether this one runs must not depend on that
  if (tid == 0) T.skip = (status[i] & (PPST_JPEG_S_MARKER | PPST_JPEG_S_RST_COUNT | PPST_JPEG_S_RST_ORDER)) != 0;
  const ppst_jpeg_dec_image& d = imgs[i];
  for (int e = tid; e < 4 * 512; e += JD_ENT_T) (&T.lut[0][0])[e] = 0;
  for (int e = tid; e < 4 * 256; e += JD_ENT_T) (&T.vals[0][0])[e] = d.vals[e >> 8][e & 255];
  if (tid < 6) {
    const int comp = d.ncomp == 1 ? 0 : (im.g.ss == 2 ? (tid < 4 ? 0 : tid - 3) : (tid < 3 ? tid : 0));
    T.slot_dc[tid] = d.dc_tab[comp] & 1;
    T.slot_ac[tid] = 2 + (d.ac_tab[comp] & 1);
  }
  __syncthreads();
  if (T.skip) return;
  if (tid < 4) {                                    // T.81 Annex C: canonical codes by length
    int code = 0, k = 0;
    T.maxcode[tid][0] = -1; T.valoff[tid][0] = 0;
    for (int l = 1; l <= 16; ++l) {
      const int nl = d.bits[tid][l - 1];
      T.valoff[tid][l] = k - code;
      for (int j = 0; j < nl; ++j) {
        if (l <= 9) {
          const unsigned short ent = (unsigned short)((l << 8) | d.vals[tid][k & 255]);
          const int first = code << (9 - l);
          for (int f = 0; f < (1 << (9 - l)); ++f) T.lut[tid][(first + f) & 511] = ent;
        }
        ++code; ++k;
      }
      T.maxcode[tid][l] = nl ? code - 1 : -1;
      code <<= 1;
    }
  }
  __syncthreads();

  const unsigned* ivl = (const unsigned*)(base + im.l.ivl);
  const unsigned s0 = ivl[it], s1 = ivl[it + 1];                              // clean bytes [s0, s1) (s0 <= s1 <= L: status is 0)
  const unsigned nbits = (s1 - s0) * 8u, origin = s0 * 8u, SB = im.g.SB;
  const unsigned nsub = nbits ? (nbits + SB - 1) / SB : 1u;
  const unsigned sub0 = (unsigned)(((uint64_t)s0 * 8u) / SB) + (unsigned)it;   // this interval's slots: sub0 + nsub <= the next one's sub0
  unsigned* S = (unsigned*)(base + im.l.sub);
  unsigned* Ep = S + sub0;                          // entry: bit position
  unsigned* Es = Ep + im.g.nsub;                    //        b << 8 | k
  unsigned* Xp = Es + im.g.nsub;                    // exit of the last decode
  unsigned* Xs = Xp + im.g.nsub;
  unsigned* N = Xs + im.g.nsub;                     // blocks completed
  unsigned* D = N + im.g.nsub;                      // entry changed: decode again
  const unsigned* cw = (const unsigned*)(base + im.l.clean);
  const int nm = min(im.g.R, im.g.nmcu - it * im.g.R);
  const int nb = nm * im.g.bpm, bpm = im.g.bpm;
  short* coef = (short*)(base + im.l.coef) + (int64_t)it * im.g.R * bpm * 64;

  const unsigned per = (nsub + JD_ENT_T - 1) / JD_ENT_T;                      // lanes loop over their subsequences
  const unsigned i0 = min(nsub, tid * per), i1 = min(nsub, i0 + per);
  for (unsigned q = i0; q < i1; ++q) { Ep[q] = q * SB; Es[q] = 0; Xp[q] = 0xFFFFFFFFu; Xs[q] = 0xFFFFFFFFu; D[q] = 1; }
  int rounds = 0;
  for (;;) {
    for (unsigned q = i0; q < i1; ++q) {
      if (!D[q]) continue;
      const JdState x = jd_run<false>(T, cw, origin, nbits, min(nbits, (q + 1) * SB), bpm, Ep[q], Es[q], nullptr, 0, 0);
      Xp[q] = x.p; Xs[q] = (unsigned)(x.b << 8 | x.k); N[q] = (unsigned)x.n; D[q] = 0;
    }
    __syncthreads();
    ++rounds;
    int changed = 0;
    for (unsigned q = max(i0, 1u); q < i1; ++q)
      if (Xp[q - 1] != Ep[q] || Xs[q - 1] != Es[q]) { Ep[q] = Xp[q - 1]; Es[q] = Xs[q - 1]; D[q] = 1; changed = 1; }
    if (!__syncthreads_or(changed)) break;
    if ((unsigned)rounds > nsub) break;                                       // (never: after round r the first r entries are final)
  }
  if (tid == 0) atomicMax((int*)work + i, rounds);

  // ---- first block of every subsequence, the write pass
  int mine = 0;
  for (unsigned q = i0; q < i1; ++q) mine += (int)N[q];
  int total;
  int blk = wg_scan<JD_ENT_T, false>(mine, total, T.wt, 0);
  int bad = 0;
  for (unsigned q = i0; q < i1; ++q) {
    bad |= jd_run<true>(T, cw, origin, nbits, min(nbits, (q + 1) * SB), bpm, Ep[q], Es[q], coef, blk, nb).bad;
    blk += (int)N[q];
  }
  if (bad) atomicOr(&status[i], PPST_JPEG_S_CODE);
  if (tid == 0 && total != nb) atomicOr(&status[i], PPST_JPEG_S_BLOCKS);
  __syncthreads();

  // ---- DC: differences -> values, per component from 0 at the interval's start; a lane takes a run of MCUs
  const int perm = (nm + JD_ENT_T - 1) / JD_ENT_T;
  const int m0 = min(nm, tid * perm), m1 = min(nm, m0 + perm);
  int sum0 = 0, sum1 = 0, sum2 = 0;                 // (three names, not an array indexed by the component: that goes to scratch memory)
  for (int m = m0; m < m1; ++m)
    for (int j = 0; j < bpm; ++j) {
      const int c = bpm == 6 ? (j < 4 ? 0 : j - 3) : j;
      const int v = coef[((int64_t)m * bpm + j) * 64];
      sum0 += c == 0 ? v : 0; sum1 += c == 1 ? v : 0; sum2 += c == 2 ? v : 0;
    }
  int t;
  int pre0 = wg_scan<JD_ENT_T, false>(sum0, t, T.wt, 1);
  int pre1 = wg_scan<JD_ENT_T, false>(sum1, t, T.wt, 0);
  int pre2 = wg_scan<JD_ENT_T, false>(sum2, t, T.wt, 1);
  for (int m = m0; m < m1; ++m)
    for (int j = 0; j < bpm; ++j) {
      const int c = bpm == 6 ? (j < 4 ? 0 : j - 3) : j;
      short* q = &coef[((int64_t)m * bpm + j) * 64];
      const int v = (c == 0 ? pre0 : (c == 1 ? pre1 : pre2)) + *q;
      pre0 = c == 0 ? v : pre0; pre1 = c == 1 ? v : pre1; pre2 = c == 2 ? v : pre2;
      *q = (short)v;
    }
}

// --------------------------------------------------------------------------------------------------------------------- IDCT
// libjpeg's jidctint ("islow") on eight values: the column pass descales by CONST_BITS - PASS1_BITS = 11, the row pass by
// CONST_BITS + PASS1_BITS + 3 = 18
template <int SHIFT>
__device__ __forceinline__ void jd_idct8(const int* in, int* out) {
  int z1 = (in[2] + in[6]) * 4433;
  const int t2 = z1 - in[6] * 15137, t3 = z1 + in[2] * 6270;
  const int t0 = (in[0] + in[4]) * 8192, t1 = (in[0] - in[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
  z1 = o0 + o3;
  int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const int z5 = (z3 + z4) * 9633;
  o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  const int r = 1 << (SHIFT - 1);
  out[0] = (t10 + o3 + r) >> SHIFT; out[7] = (t10 - o3 + r) >> SHIFT;
  out[1] = (t11 + o2 + r) >> SHIFT; out[6] = (t11 - o2 + r) >> SHIFT;
  out[2] = (t12 + o1 + r) >> SHIFT; out[5] = (t12 - o1 + r) >> SHIFT;
  out[3] = (t13 + o0 + r) >> SHIFT; out[4] = (t13 - o0 + r) >> SHIFT;
}

__global__ __launch_bounds__(256) void jd_idct_kernel(const ppst_jpeg_dec_image* __restrict__ imgs, int B, int sw, void* work) {
  __shared__ int ws[JD_IDCT_BLOCKS][64];
  const int i = blockIdx.y, tid = threadIdx.x;
  const JdImg& im = open_plan<JdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  const int64_t blk0 = (int64_t)blockIdx.x * JD_IDCT_BLOCKS;
  if (blk0 >= im.g.nblk) return;
  const ppst_jpeg_dec_image& d = imgs[i];
  const short* coef = (const short*)(base + im.l.coef);
  const int bpm = im.g.bpm;
  for (int e = tid; e < JD_IDCT_BLOCKS * 64; e += 256) {
    const int j = e >> 6, k = e & 63;
    const int64_t blk = blk0 + j;
    int v = 0;
    if (blk < im.g.nblk) {
      const int slot = (int)(blk % bpm);
      const int c = bpm == 6 ? (slot < 4 ? 0 : slot - 3) : slot;
      v = (int)coef[blk * 64 + k] * (int)d.qt[c][k];
    }
    ws[j][D_ZIGZAG[k]] = v;
  }
  __syncthreads();
  const int j = tid >> 3, c8 = tid & 7;
  int in[8], out[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) in[r] = ws[j][r * 8 + c8];
  jd_idct8<11>(in, out);
#pragma unroll
  for (int r = 0; r < 8; ++r) ws[j][r * 8 + c8] = out[r];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) in[r] = ws[j][c8 * 8 + r];
  jd_idct8<18>(in, out);
  const int64_t blk = blk0 + j;
  if (blk >= im.g.nblk) return;
  unsigned px[2] = {0u, 0u};
#pragma unroll
  for (int r = 0; r < 8; ++r) px[r >> 2] |= (unsigned)min(max(out[r] + 128, 0), 255) << (8 * (r & 3));
  const int mcu = (int)(blk / bpm), slot = (int)(blk - (int64_t)mcu * bpm);
  const int my = mcu / im.g.mw, mx = mcu - my * im.g.mw;
  unsigned char* plane = base + im.l.plane;
  int64_t at;
  if (bpm == 6 && slot < 4) at = (int64_t)(my * 16 + (slot >> 1) * 8 + c8) * im.g.pwy + mx * 16 + (slot & 1) * 8;
  else if (bpm == 6) at = (int64_t)im.g.pwy * im.g.phy + (int64_t)(slot - 4) * im.g.pwc * im.g.phc + (int64_t)(my * 8 + c8) * im.g.pwc + mx * 8;
  else at = (int64_t)slot * im.g.pwy * im.g.phy + (int64_t)(my * 8 + c8) * im.g.pwy + mx * 8;       // (4:4:4: all planes the luma size)
  *(uint2*)(plane + at) = make_uint2(px[0], px[1]);
}

// ------------------------------------------------------------------------------------------------------------------- colour
// libjpeg's fancy h2v2 upsampling of one chroma sample for pixel (y, x): ch x cw = the ceil(H / 2) x ceil(W / 2) samples that count
__device__ __forceinline__ int jd_fancy(const unsigned char* __restrict__ c, int stride, int ch, int cw, int y, int x) {
  const int cy = y >> 1, cx = x >> 1;
  if (cw <= 2) return c[(int64_t)cy * stride + cx];
  const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const unsigned char* rn = c + (int64_t)cy * stride;
  const unsigned char* rf = c + (int64_t)fy * stride;
  const int here = 3 * rn[cx] + rf[cx];
  if (x & 1) {
    const int ox = min(cx + 1, cw - 1);
    return (3 * here + 3 * rn[ox] + rf[ox] + 7) >> 4;
  }
  const int ox = max(cx - 1, 0);
  return (3 * here + 3 * rn[ox] + rf[ox] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jd_colour_kernel(const ppst_jpeg_dec_image* __restrict__ imgs, int B, int sw, void* work,
                                                        unsigned char* __restrict__ out_u8) {
  const int i = blockIdx.y;
  const JdImg& im = open_plan<JdImg>(B, work, i);
  unsigned char* const base = (unsigned char*)work + im.base_off;
  const ppst_jpeg_dec_image& d = imgs[i];
  const int64_t px = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (px >= (int64_t)d.H * d.W) return;
  const int y = (int)(px / d.W), x = (int)(px - (int64_t)y * d.W);
  const unsigned char* plane = base + im.l.plane;
  const int Y = plane[(int64_t)y * im.g.pwy + x];
  const int xo = d.mirror ? d.W - 1 - x : x;
  unsigned char* o = out_u8 + d.out_off + ((int64_t)y * d.W + xo) * im.g.cout;
  if (d.ncomp == 1) {
    o[0] = (unsigned char)Y;
    if (im.g.cout == 3) { o[1] = (unsigned char)Y; o[2] = (unsigned char)Y; }
    return;
  }
  const int64_t ysz = (int64_t)im.g.pwy * im.g.phy;
  int cb, cr;
  if (im.g.ss == 2) {
    const int64_t csz = (int64_t)im.g.pwc * im.g.phc;
    const int ch = (d.H + 1) >> 1, cw = (d.W + 1) >> 1;
    cb = jd_fancy(plane + ysz, im.g.pwc, ch, cw, y, x);
    cr = jd_fancy(plane + ysz + csz, im.g.pwc, ch, cw, y, x);
  } else {
    cb = plane[ysz + (int64_t)y * im.g.pwy + x];
    cr = plane[2 * ysz + (int64_t)y * im.g.pwy + x];
  }
  cb -= 128; cr -= 128;
  const int r = Y + ((91881 * cr + 32768) >> 16);
  const int b = Y + ((116130 * cb + 32768) >> 16);
  const int g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
  o[0] = (unsigned char)min(max(r, 0), 255);
  o[1] = (unsigned char)min(max(g, 0), 255);
  o[2] = (unsigned char)min(max(b, 0), 255);
}

// --------------------------------------------------------------------------------------------------------------------- host
// a descriptor ppst_jpeg_parse can have made (the kernels index with these fields)
static bool jd_valid(const ppst_jpeg_dec_image& d) {
  if (d.H < 1 || d.W < 1 || d.H > 65535 || d.W > 65535) return false;
  if (d.ncomp != 1 && d.ncomp != 3) return false;
  if (d.ss != 1 && d.ss != 2) return false;
  if (d.ncomp == 1 && d.ss != 1) return false;
  if (d.dri < 0 || d.dri > 65535 || d.scan_off < 0 || d.scan_len < 0 || d.scan_len >= JD_SCAN_MAX) return false;
  if (d.file_off < 0 || d.out_off < 0) return false;
  for (int c = 0; c < 3; ++c)
    if (d.dc_tab[c] > 1 || d.ac_tab[c] > 1) return false;
  for (int t = 0; t < 4; ++t) {
    unsigned code = 0;
    int cnt = 0;
    for (int l = 0; l < 16; ++l) {
      code += d.bits[t][l];
      cnt += d.bits[t][l];
      if (code > (1u << (l + 1))) return false;
      code <<= 1;
    }
    if (cnt > 256) return false;
  }
  return true;
}

static bool jd_sw_ok(int sw) { return sw == 0 || (sw >= 2 && sw <= JD_SUBSEQ_MAX); }

extern "C" int64_t ppst_jpeg_decode_ws(const ppst_jpeg_dec_image* imgs, int B, int subseq_words) {
  if (B < 0 || B > 65535 || !jd_sw_ok(subseq_words)) return PPST_EINVAL;
  if (B > 0 && !imgs) return PPST_ENULL;
  int64_t total = head_bytes<JdImg>(B > 0 ? B : 1);
  for (int i = 0; i < B; ++i) {
    if (!jd_valid(imgs[i])) return PPST_EINVAL;
    JdImg im;
    codec_fill(imgs[i], subseq_words, &im);
    total += im.l.total;
  }
  return total;
}

extern "C" int ppst_jpeg_decode(const void* bytes, int64_t nbytes, const ppst_jpeg_dec_image* imgs_host, const void* imgs_dev, void* out_u8,
                                int64_t out_bytes, void* status, int B, int subseq_words, void* work, void* stream) {
  if (B < 0 || B > 65535 || !jd_sw_ok(subseq_words) || nbytes < 0 || out_bytes < 0) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!imgs_host) return PPST_ENULL;
  int max_chunk = 1, max_ni = 1;
  int64_t max_blk = 1, max_px = 1;
  for (int i = 0; i < B; ++i) {
    const ppst_jpeg_dec_image& d = imgs_host[i];
    if (!jd_valid(d)) return PPST_EINVAL;
    JdGeom g;
    jd_geom(d, subseq_words, &g);
    if (d.file_off > nbytes || (int64_t)d.scan_off + d.scan_len > nbytes - d.file_off) return PPST_EINVAL;
    if (d.out_off > out_bytes || (int64_t)d.H * d.W * g.cout > out_bytes - d.out_off) return PPST_EINVAL;
    if (g.nchunk > max_chunk) max_chunk = g.nchunk;
    if (g.NI > max_ni) max_ni = g.NI;
    if (g.nblk > max_blk) max_blk = g.nblk;
    if ((int64_t)d.H * d.W > max_px) max_px = (int64_t)d.H * d.W;
  }
  if (!bytes || !imgs_dev || !out_u8 || !status || !work) return PPST_ENULL;
  if (((uintptr_t)work | (uintptr_t)out_u8 | (uintptr_t)imgs_dev) & 15) return PPST_EINVAL;
  hipStream_t st = as_stream(stream);
  const ppst_jpeg_dec_image* dd = (const ppst_jpeg_dec_image*)imgs_dev;
  const unsigned char* by = (const unsigned char*)bytes;
  int* stt = (int*)status;
  const int sw = subseq_words;
  static_assert(sizeof(JdTabs) <= 16 * 1024, "the entropy workgroup's tables");
  PPST_LAUNCH(plan_kernel<JdImg>, dim3(1), dim3(256), 0, st, dd, B, sw, work, stt);
  PPST_LAUNCH(jd_zero_kernel, dim3((unsigned)cdiv64(max_blk * 8, 256), (unsigned)B), dim3(256), 0, st, dd, B, sw, work);
  PPST_LAUNCH(jd_count_kernel, dim3((unsigned)max_chunk, (unsigned)B), dim3(JD_CHUNK_T), 0, st, by, dd, B, sw, work, stt);
  PPST_LAUNCH(jd_offsets_kernel, dim3((unsigned)B), dim3(JD_CHUNK_T), 0, st, dd, B, sw, work, stt);
  PPST_LAUNCH(jd_compact_kernel, dim3((unsigned)max_chunk, (unsigned)B), dim3(JD_CHUNK_T), 0, st, by, dd, B, sw, work, stt);
  PPST_LAUNCH(jd_entropy_kernel, dim3((unsigned)max_ni, (unsigned)B), dim3(JD_ENT_T), 0, st, dd, B, sw, work, stt);
  PPST_LAUNCH(jd_idct_kernel, dim3((unsigned)cdiv64(max_blk, JD_IDCT_BLOCKS), (unsigned)B), dim3(256), 0, st, dd, B, sw, work);
  PPST_LAUNCH(jd_colour_kernel, dim3((unsigned)cdiv64(max_px, 256), (unsigned)B), dim3(256), 0, st, dd, B, sw, work, (unsigned char*)out_u8);
  return PPST_LAUNCH_CHECK();
}
