// PNG encode on the device: the "uint8 batch -> files" end of the evaluators (DESIGN.md "PNG encode on the device").
//   1. png_filter_kernel   one wave per image row: PNG's five row filters, libpng's heuristic (smallest sum of |signed byte|,
//                          ties to the lowest filter number), 1 + W*C bytes per row into the workspace.
//   2. png_deflate_kernel  one workgroup per PNG_PIECE bytes of the filtered stream: byte histogram, length-limited Huffman code
//                          (15 bits; 7 bits for the code-length alphabet), ONE dynamic block of literals (no match search: on
//                          filtered photo-like rows LZ77 costs more than it saves), byte-aligned by an empty stored block the way
//                          pigz does; a stored block instead when that is not smaller.  The workgroup wraps its bytes into an IDAT
//                          chunk of its own (it owns that chunk's CRC-32) in its own slot of the workspace and records
//                          (chunk bytes, Adler-32 partial sums).  No block waits for another one.
//   3. png_layout_kernel   one workgroup per image: piece offsets, signature + IHDR, the combined Adler-32 (an IDAT chunk of
//                          four bytes), IEND, the file size;  png_gather_kernel copies the chunks to their offsets.
// All of it is integer code on bytes, bits and LDS words: deterministic, the same file for the same pixels whatever the batch.
// Shared with the other coders: the workgroup scan and the slot-to-file copy (codec_common.h); the CRC-32, the Paeth predictor, the
// code-length order and the joining of Adler-32 partial sums (png_common.h).
#include "common.h"
#include "codec_common.h"
#include "png_common.h"

#define PNG_PIECE 32768                       // bytes of the filtered stream per deflate block / workgroup / IDAT chunk
#define PNG_NT 512                            // threads of the deflate workgroup
#define PNG_SLOT (PNG_PIECE + 32)             // chunk(12) + zlib header(2) + stored header(5) + piece, rounded up to 16
#define PNG_HEAD 33                           // signature + IHDR chunk
#define PNG_TAIL 28                           // Adler-32 IDAT chunk (16) + IEND (12)
#define PNG_NLIT 257                          // literals + end-of-block: the whole lit/len alphabet of a block without matches
#define PNG_NSYM_MAX 320
#define PNG_INF 0xFFFFFFFFu
static_assert(PNG_PIECE % 16 == 0 && PNG_PIECE <= 65535, "one stored block per piece");
static_assert(PNG_NT >= 20 + PNG_NLIT + 2, "the header round has one item per thread");
static_assert(PNG_SLOT % 16 == 0 && PNG_SLOT >= PNG_PIECE + 12 + 2 + 5 + 3, "slot holds the stored worst case");

struct PngGeom {
  int H, W, C;
  int row;                 // 1 + W*C
  int64_t n;               // H * row: bytes of the filtered stream of one image
  int64_t n_pad;           // n rounded up to 16
  int P;                   // pieces per image
  int64_t bound;           // bytes of one file slot
};
struct PngHead { unsigned w[9]; };            // the 33 bytes in front of the first IDAT (built on the host), little-endian words

__device__ __forceinline__ int png_abs8(int v) { v &= 255; return v < 128 ? v : 256 - v; }

// ---------------------------------------------------------------------------------------------------------------- filter
// One wave per row (4 rows per block).  A row's candidates read the raw row above only: rows are independent.
__global__ __launch_bounds__(256) void png_filter_kernel(const unsigned char* __restrict__ img, unsigned char* __restrict__ filt,
                                                         PngGeom g, int64_t rows_total) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows_total) return;
  const int64_t b = r / g.H;
  const int y = (int)(r - b * g.H);
  const int bpp = g.C, nb = g.row - 1;
  const unsigned char* cur = img + (b * g.H + y) * (int64_t)nb;
  const unsigned char* up = y > 0 ? cur - nb : cur;    // the raw row above (read only when there is one)
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
  for (int i = lane; i < nb; i += 64) {
    const int x = cur[i];
    const int a = i >= bpp ? cur[i - bpp] : 0;
    const int u = y > 0 ? up[i] : 0;
    const int c = (y > 0 && i >= bpp) ? up[i - bpp] : 0;
    c0 += png_abs8(x);
    c1 += png_abs8(x - a);
    c2 += png_abs8(x - u);
    c3 += png_abs8(x - ((a + u) >> 1));
    c4 += png_abs8(x - png_paeth(a, u, c));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64);
    c3 += __shfl_xor(c3, o, 64); c4 += __shfl_xor(c4, o, 64);
  }
  int f = 0, best = c0;
  if (c1 < best) { best = c1; f = 1; }
  if (c2 < best) { best = c2; f = 2; }
  if (c3 < best) { best = c3; f = 3; }
  if (c4 < best) { best = c4; f = 4; }
  unsigned char* out = filt + b * g.n_pad + (int64_t)y * g.row;
  if (lane == 0) out[0] = (unsigned char)f;
  for (int i = lane; i < nb; i += 64) {
    const int x = cur[i];
    const int a = i >= bpp ? cur[i - bpp] : 0;
    const int u = y > 0 ? up[i] : 0;
    const int c = (y > 0 && i >= bpp) ? up[i - bpp] : 0;
    int v = x;
    if (f == 1) v = x - a;
    else if (f == 2) v = x - u;
    else if (f == 3) v = x - ((a + u) >> 1);
    else if (f == 4) v = x - png_paeth(a, u, c);
    out[1 + i] = (unsigned char)v;
  }
}

// (the span-joining CRC-32: png_common.h)
__device__ __forceinline__ unsigned bswap32(unsigned v) { return __builtin_bswap32(v); }

// ------------------------------------------------------------------------------------------------ Huffman code lengths
struct HuffScratch {
  unsigned sf[PNG_NSYM_MAX + 2];        // frequencies in ascending order (+ 2 sentinels)
  unsigned intf[PNG_NSYM_MAX + 2];      // internal nodes, in creation order (ascending too)
  unsigned short ssym[PNG_NSYM_MAX];    // symbol of sorted rank r
  unsigned short parent[2 * PNG_NSYM_MAX];
  unsigned num[16];                     // codes per length
  unsigned m;
};

// freq[0..n) -> len[0..n): an optimal prefix code limited to `maxbits`, complete (Kraft sum exactly 1) whenever at least two
// symbols occur; *ok = 0 otherwise.  Whole workgroup; ends with a barrier.
// Rank sort, the two-queue merge by one lane (<= 256 steps, one LDS round trip each), depths by walking up from every leaf,
// then the counts per length are cut to `maxbits` and re-balanced (the Kraft sum is brought back to 1 one unit at a time: a
// code of the last length and the deepest shorter code become two siblings one level down), and lengths are handed out again in
// frequency order -- identical to the tree's when nothing was cut.
__device__ void huff_lengths(const unsigned* freq, int n, int maxbits, unsigned char* len, HuffScratch& s, int* ok) {
  const int tid = threadIdx.x;
  for (int i = tid; i < PNG_NSYM_MAX + 2; i += PNG_NT) { s.sf[i] = PNG_INF; s.intf[i] = PNG_INF; }
  if (tid < 16) s.num[tid] = 0;
  for (int i = tid; i < n; i += PNG_NT) len[i] = 0;
  __syncthreads();
  int m = 0;
  for (int sidx = tid; sidx < n; sidx += PNG_NT) {      // (n <= PNG_NT: one pass)
    const unsigned f = freq[sidx];
    int rank = 0, cnt = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned fj = freq[j];
      cnt += fj > 0;
      rank += (fj > 0) && (fj < f || (fj == f && j < sidx));
    }
    m = cnt;
    if (f > 0) { s.sf[rank] = f; s.ssym[rank] = (unsigned short)sidx; }
  }
  if (tid == 0) s.m = (unsigned)m;
  __syncthreads();
  m = (int)s.m;
  if (m < 2) { if (tid == 0) *ok = 0; __syncthreads(); return; }
  if (tid == 0) {
    int li = 0, ii = 0;
    for (int k = 0; k < m - 1; ++k) {
      unsigned a0 = s.sf[li], a1 = s.sf[li + 1], b0 = s.intf[ii], b1 = s.intf[ii + 1];
      unsigned x, y;
      int n1, n2;
      if (a0 <= b0) { x = a0; n1 = li++; a0 = a1; } else { x = b0; n1 = m + ii++; b0 = b1; }
      if (a0 <= b0) { y = a0; n2 = li++; } else { y = b0; n2 = m + ii++; }
      s.intf[k] = x + y;
      s.parent[n1] = (unsigned short)(m + k);
      s.parent[n2] = (unsigned short)(m + k);
    }
  }
  __syncthreads();
  if (tid < m) {
    int d = 0, node = tid;
    const int root = 2 * m - 2;
    while (node != root && d < 2 * PNG_NSYM_MAX) { node = s.parent[node]; ++d; }
    atomicAdd(&s.num[d < maxbits ? d : maxbits], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned total = 0;
    for (int i = maxbits; i > 0; --i) total += s.num[i] << (maxbits - i);
    while (total > (1u << maxbits)) {
      s.num[maxbits]--;
      for (int i = maxbits - 1; i > 0; --i)
        if (s.num[i]) { s.num[i]--; s.num[i + 1] += 2; break; }
      total--;
    }
    *ok = (total == (1u << maxbits)) ? 1 : 0;
  }
  __syncthreads();
  if (tid < m) {
    int l = maxbits;
    unsigned end = s.num[maxbits];
    while (l > 1 && (unsigned)tid >= end) { --l; end += s.num[l]; }
    len[s.ssym[tid]] = (unsigned char)l;
  }
  __syncthreads();
}

// canonical codes from lengths (RFC 1951 3.2.2), bit-reversed for LSB-first packing: code[i] = (len << 16) | reversed code.
// num[l] = codes of length l (as huff_lengths leaves it).  No barrier inside.
__device__ void huff_codes(const unsigned char* len, int n, const unsigned* num, unsigned* code) {
  for (int sidx = threadIdx.x; sidx < n; sidx += PNG_NT) {
    const int l = len[sidx];
    unsigned c = 0;
    for (int bits = 1; bits <= l; ++bits) c = (c + (bits > 1 ? num[bits - 1] : 0u)) << 1;
    for (int j = 0; j < sidx; ++j) c += (len[j] == l);
    code[sidx] = l ? (((unsigned)l << 16) | (__brev(c) >> (32 - l))) : 0u;
  }
}

// ---------------------------------------------------------------------------------------------------------------- deflate
struct DeflateLds {
  unsigned out[PNG_SLOT / 4];
  unsigned hist[4][PNG_NLIT + 3];
  unsigned freq[PNG_NSYM_MAX];
  unsigned clfreq[19];
  unsigned char len[PNG_NSYM_MAX];      // [0, 257): lit/len, [257, 259): the two distance codes
  unsigned char cllen[32];
  unsigned code[PNG_NSYM_MAX];
  unsigned clcode[19];
  unsigned num_ll[16];
  HuffScratch hs;
  int wave_tot[2][PNG_NT / 64];
  unsigned bits, adler_a, adler_b, crc;
  int ok;
};

// `nbits` low bits of v at bit `pos` of the LDS image (the image starts as zeros: OR-ing is placing)
__device__ __forceinline__ void put_bits(unsigned* out, unsigned pos, unsigned long long v, int nbits) {
  if (nbits == 0) return;
  const unsigned w = pos >> 5, sh = pos & 31;
  const unsigned long long lo = v << sh;
  const unsigned hi = sh ? (unsigned)(v >> (64 - sh)) : 0u;
  if ((unsigned)lo) atomicOr(&out[w], (unsigned)lo);
  if ((unsigned)(lo >> 32)) atomicOr(&out[w + 1], (unsigned)(lo >> 32));
  if (hi) atomicOr(&out[w + 2], hi);
}

__global__ __launch_bounds__(PNG_NT) void png_deflate_kernel(const unsigned char* __restrict__ filt, unsigned char* __restrict__ slots,
                                                              unsigned* __restrict__ meta, PngGeom g) {
  __shared__ DeflateLds s;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int64_t b = blk / g.P;
  const int p = (int)(blk - b * g.P);
  const int64_t off = (int64_t)p * PNG_PIECE;
  const int np = (int)((g.n - off) < PNG_PIECE ? (g.n - off) : PNG_PIECE);       // 1 .. PNG_PIECE
  const int nwords = (np + 3) >> 2;
  const bool final_piece = p == g.P - 1;
  const int zhdr = p == 0 ? 2 : 0;
  const int data0 = 8 + zhdr;                                                      // byte of the chunk where deflate data starts

  // the piece as words (its start is 16-byte aligned: n_pad and the piece size are multiples of 16; the last word may reach into
  // the padding, whose bytes are masked out).  Read twice from L2 -- histogram, then coding -- one coalesced word per lane.
  const unsigned* inw = reinterpret_cast<const unsigned*>(filt + b * g.n_pad + off);
  // ---- zeroed output image and histograms
  {
    for (int i = tid; i < PNG_SLOT / 4; i += PNG_NT) s.out[i] = 0;
    for (int i = tid; i < 4 * (PNG_NLIT + 3); i += PNG_NT) (&s.hist[0][0])[i] = 0;
    if (tid < 19) s.clfreq[tid] = 0;
    if (tid == 0) { s.bits = 0; s.adler_a = 0; s.adler_b = 0; s.crc = 0; s.ok = 1; }
  }
  __syncthreads();
  // ---- histogram (per pair of waves) + Adler-32 partial sums: A = sum d_i, B = sum (np - i) d_i, both mod 65521
  {
    unsigned* h = s.hist[wave & 3];
    unsigned a = 0, bb = 0;
    for (int w = tid; w < nwords; w += PNG_NT) {
      const unsigned v = inw[w];
      const int nv = np - 4 * w < 4 ? np - 4 * w : 4;
      unsigned s1 = 0, s2 = 0;
      for (int k = 0; k < nv; ++k) {
        const unsigned d = (v >> (8 * k)) & 255u;
        atomicAdd(&h[d], 1u);
        s1 += d;
        s2 += (unsigned)(np - (4 * w + k)) * d;        // <= 32768 * 255 each, four of them: < 2^32
      }
      a += s1;                                         // <= 64 words * 1020
      bb = (bb + s2 % 65521u);                         // <= 64 * 65520
    }
    atomicAdd(&s.adler_a, a % 65521u);
    atomicAdd(&s.adler_b, bb % 65521u);                // <= 512 * 65520 < 2^32
  }
  __syncthreads();
  for (int i = tid; i < PNG_NSYM_MAX; i += PNG_NT)
    s.freq[i] = i < 256 ? s.hist[0][i] + s.hist[1][i] + s.hist[2][i] + s.hist[3][i] : (i == 256 ? 1u : 0u);
  __syncthreads();

  // ---- code lengths: lit/len (15 bits), the two distance codes of one bit each (a block without matches still has to send a
  // distance code; two one-bit codes are the complete set zlib itself sends), then the code-length alphabet (7 bits)
  int ok_ll = 1;
  huff_lengths(s.freq, PNG_NLIT, 15, s.len, s.hs, &s.ok);
  if (tid < 16) s.num_ll[tid] = s.hs.num[tid];
  if (tid < 2) s.len[PNG_NLIT + tid] = 1;
  __syncthreads();
  ok_ll = s.ok;
  huff_codes(s.len, PNG_NLIT, s.num_ll, s.code);
  if (tid < PNG_NLIT + 2) atomicAdd(&s.clfreq[s.len[tid]], 1u);
  __syncthreads();
  if (tid == 0) s.ok = 1;
  huff_lengths(s.clfreq, 19, 7, s.cllen, s.hs, &s.ok);
  const int ok = ok_ll && s.ok;
  huff_codes(s.cllen, 19, s.hs.num, s.clcode);
  // ---- size of the dynamic block: 17 header bits + 19 * 3 + the coded lengths + the symbols (end-of-block is in freq)
  {
    unsigned bits = 0;
    if (tid < PNG_NLIT) bits += s.freq[tid] * s.len[tid];
    if (tid < PNG_NLIT + 2) bits += s.cllen[s.len[tid]];
    if (tid == 0) bits += 17 + 57;
    atomicAdd(&s.bits, bits);
  }
  __syncthreads();
  // bytes with the byte-aligning empty stored block (3 bits, pad, 00 00 FF FF) behind every piece but the last
  const unsigned huff_bits = s.bits;
  const unsigned huff_bytes = final_piece ? (huff_bits + 7) >> 3 : ((huff_bits + 3 + 7) >> 3) + 4;
  const bool stored = !ok || huff_bytes >= (unsigned)np + 5;
  unsigned datalen;
  unsigned char* outb = reinterpret_cast<unsigned char*>(s.out);

  if (stored) {
    datalen = (unsigned)np + 5;
    if (tid == 0) {
      outb[data0 + 0] = final_piece ? 1 : 0;
      outb[data0 + 1] = (unsigned char)(np & 255);
      outb[data0 + 2] = (unsigned char)(np >> 8);
      outb[data0 + 3] = (unsigned char)(~np & 255);
      outb[data0 + 4] = (unsigned char)((~np >> 8) & 255);
    }
    const unsigned char* inb = reinterpret_cast<const unsigned char*>(inw);
    for (int i = tid; i < np; i += PNG_NT) outb[data0 + 5 + i] = inb[i];
  } else {
    // every round places its bits behind `base`: the exclusive prefix over the workgroup (wg_scan, codec_common.h), then base
    // advances by the round's total in every thread's copy
    unsigned base = (unsigned)data0 * 8;
    int round_bits;
    // header round: thread 0 = BFINAL, BTYPE = 2, HLIT = 0 (257), HDIST = 1 (2), HCLEN = 15 (19); threads 1..19 = the code-length
    // code's lengths in the format's order; threads 20..278 = the 259 lengths, coded (no repeat codes 16 / 17 / 18)
    {
      unsigned long long v = 0;
      int nb = 0;
      if (tid == 0) { v = (final_piece ? 1u : 0u) | (2u << 1) | (0u << 3) | (1u << 8) | (15u << 13); nb = 17; }
      else if (tid < 20) { v = s.cllen[PNG_CL_ORDER[tid - 1]]; nb = 3; }
      else if (tid < 20 + PNG_NLIT + 2) { const unsigned c = s.clcode[s.len[tid - 20]]; v = c & 0xffffu; nb = (int)(c >> 16); }
      const unsigned pos = base + (unsigned)wg_scan<PNG_NT, false>(nb, round_bits, s.wave_tot, 0);
      base += (unsigned)round_bits;
      put_bits(s.out, pos, v, nb);
    }
    // symbol rounds: one word (4 bytes, <= 60 bits) per thread
    int slot = 1;
    for (int w0 = 0; w0 < nwords; w0 += PNG_NT, slot ^= 1) {
      const int w = w0 + tid;
      unsigned long long v = 0;
      int nb = 0;
      if (w < nwords) {
        const unsigned word = inw[w];
        const int nv = np - 4 * w < 4 ? np - 4 * w : 4;
        for (int k = 0; k < nv; ++k) {
          const unsigned c = s.code[(word >> (8 * k)) & 255u];
          v |= (unsigned long long)(c & 0xffffu) << nb;
          nb += (int)(c >> 16);
        }
      }
      const unsigned pos = base + (unsigned)wg_scan<PNG_NT, false>(nb, round_bits, s.wave_tot, slot);
      base += (unsigned)round_bits;
      put_bits(s.out, pos, v, nb);
    }
    // end of block, then the aligning empty stored block
    unsigned end = base;
    if (tid == 0) { const unsigned c = s.code[256]; put_bits(s.out, end, c & 0xffffu, (int)(c >> 16)); }
    end += s.code[256] >> 16;
    if (!final_piece) {
      end = (end + 3 + 7) & ~7u;
      if (tid == 0) put_bits(s.out, end + 16, 0xFFFFull, 16);                            // LEN = 0 is already there, NLEN = FFFF
      end += 32;
    } else {
      end = (end + 7) & ~7u;
    }
    datalen = (end >> 3) - (unsigned)data0;
  }
  if (tid == 0) {
    s.out[0] = bswap32(datalen + (unsigned)zhdr);
    s.out[1] = 0x54414449u;                            // "IDAT"
    if (zhdr) atomicOr(&s.out[2], 0x0178u);            // zlib header 78 01 (deflate, 32 KB window, no dictionary, check bits)
  }
  __syncthreads();
  // ---- the chunk's CRC-32 over type + data = bytes [4, 8 + zhdr + datalen): word-aligned spans, one per thread
  const unsigned crc_len = 4 + (unsigned)zhdr + datalen;
  {
    const unsigned span = (((crc_len + PNG_NT - 1) / PNG_NT) + 3) & ~3u;               // bytes per thread, a multiple of 4
    const unsigned s0 = (unsigned)tid * span;
    if (s0 < crc_len) {
      const unsigned s1 = s0 + span < crc_len ? s0 + span : crc_len;
      unsigned c = tid == 0 ? 0xFFFFFFFFu : 0u;
      for (unsigned i = s0; i < s1; i += 4) c = crc_word(c, s.out[1 + (i >> 2)], (int)(s1 - i < 4 ? s1 - i : 4));
      atomicXor(&s.crc, crc_mul(crc_xpow8(crc_len - s1), c));
    }
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned crc = bswap32(s.crc ^ 0xFFFFFFFFu);
    const unsigned at = 4 + crc_len;                                                    // any alignment: bytes
    for (int k = 0; k < 4; ++k) outb[at + k] = (unsigned char)(crc >> (8 * k));
  }
  __syncthreads();
  // ---- out: whole words into this workgroup's slot, and its record
  const unsigned chunk = 12 + (unsigned)zhdr + datalen;
  unsigned* dst = reinterpret_cast<unsigned*>(slots + blk * PNG_SLOT);
  for (unsigned i = tid; i < (chunk + 3) >> 2; i += PNG_NT) dst[i] = s.out[i];
  if (tid == 0) {
    unsigned* mrec = meta + blk * 4;
    mrec[0] = chunk; mrec[1] = s.adler_a % 65521u; mrec[2] = s.adler_b % 65521u; mrec[3] = (unsigned)np;
  }
}

// --------------------------------------------------------------------------------------------------------------- assemble
// One workgroup per image: offsets of its chunks (exclusive sum of their sizes behind the 33 leading bytes), the Adler-32 of
// the whole filtered stream from the pieces' partial sums, and every byte of the file that is not a piece's chunk.
__global__ __launch_bounds__(256) void png_layout_kernel(const unsigned* __restrict__ meta, int64_t* __restrict__ offs,
                                                         unsigned char* __restrict__ files, int64_t* __restrict__ sizes, PngGeom g,
                                                         PngHead head) {
  __shared__ unsigned rec[256][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned char* file = files + (int64_t)b * g.bound;
  int64_t off = PNG_HEAD;
  unsigned a = 1, bb = 0;
  for (int p0 = 0; p0 < g.P; p0 += 256) {
    const int cnt = g.P - p0 < 256 ? g.P - p0 : 256;
    __syncthreads();
    if (tid < cnt) {
      const uint4 v = *reinterpret_cast<const uint4*>(meta + ((int64_t)b * g.P + p0 + tid) * 4);
      rec[tid][0] = v.x; rec[tid][1] = v.y; rec[tid][2] = v.z; rec[tid][3] = v.w;
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < cnt; ++i) {
        offs[(int64_t)b * g.P + p0 + i] = off;
        off += rec[i][0];
        adler_join(a, bb, rec[i][3], rec[i][1], rec[i][2]);
      }
    }
  }
  if (tid < PNG_HEAD) file[tid] = (unsigned char)(head.w[tid >> 2] >> (8 * (tid & 3)));
  if (tid == 0) {
    const unsigned adler = (bb << 16) | a;
    unsigned char t[PNG_TAIL] = {0, 0, 0, 4, 'I', 'D', 'A', 'T', 0, 0, 0, 0, 0, 0, 0, 0,
                                 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int k = 0; k < 4; ++k) t[8 + k] = (unsigned char)(adler >> (24 - 8 * k));
    unsigned c = 0xFFFFFFFFu;
    for (int k = 4; k < 12; ++k) c = crc_word(c, t[k], 1);
    c ^= 0xFFFFFFFFu;
    for (int k = 0; k < 4; ++k) t[12 + k] = (unsigned char)(c >> (24 - 8 * k));
    for (int k = 0; k < PNG_TAIL; ++k) file[off + k] = t[k];
    sizes[b] = off + PNG_TAIL;
  }
}

// one workgroup per chunk: slot -> its place in the file (any byte alignment there)
__global__ __launch_bounds__(256) void png_gather_kernel(const unsigned char* __restrict__ slots, const unsigned* __restrict__ meta,
                                                         const int64_t* __restrict__ offs, unsigned char* __restrict__ files, PngGeom g) {
  const int64_t blk = blockIdx.x;
  const int64_t b = blk / g.P;
  slot_to_file<256>(slots + blk * PNG_SLOT, files + b * g.bound + offs[blk], meta[blk * 4]);
}

// ------------------------------------------------------------------------------------------------------------------- host
static unsigned host_crc32(const unsigned char* p, int n) {
  unsigned c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return c ^ 0xFFFFFFFFu;
}

// 0 = fine; the filtered stream of one image is addressed with 32-bit offsets, the launches with 31-bit block indices
static int png_geom(int H, int W, int C, PngGeom* g) {
  if (H < 1 || W < 1 || (C != 1 && C != 3)) return PPST_EINVAL;
  const int64_t row = 1 + (int64_t)W * C;
  const int64_t n = row * H;
  if (row > 0x7FFFFFFFll || n > 0x7FFFFFFFll - 64) return PPST_EINVAL;
  g->H = H; g->W = W; g->C = C;
  g->row = (int)row;
  g->n = n;
  g->n_pad = (n + 15) & ~15ll;
  g->P = (int)cdiv64(n, PNG_PIECE);
  // signature + IHDR, per piece an IDAT chunk (12) around a stored block (5 + bytes), the zlib header, Adler-32 chunk + IEND
  g->bound = (PNG_HEAD + 2 + n + 17 * (int64_t)g->P + PNG_TAIL + 15) & ~15ll;
  return PPST_OK;
}

extern "C" int64_t ppst_png_bound(int H, int W, int C) {
  PngGeom g;
  if (png_geom(H, W, C, &g) != PPST_OK) return PPST_EINVAL;
  return g.bound;
}

// [B][n_pad] filtered stream | [B][P][PNG_SLOT] chunks | [B][P] records of 4 words | [B][P] int64 offsets
extern "C" int64_t ppst_png_ws(int B, int H, int W, int C) {
  PngGeom g;
  if (B < 0 || png_geom(H, W, C, &g) != PPST_OK) return PPST_EINVAL;
  const int64_t bp = (int64_t)(B > 0 ? B : 1) * g.P;
  return (int64_t)(B > 0 ? B : 1) * g.n_pad + bp * PNG_SLOT + bp * 16 + bp * 8;
}

extern "C" int ppst_png_encode(const void* img_u8, void* files, void* sizes, int B, int H, int W, int C, void* work, void* stream) {
  PngGeom g;
  if (B < 0 || png_geom(H, W, C, &g) != PPST_OK) return PPST_EINVAL;
  const int64_t bp = (int64_t)B * g.P, rows = (int64_t)B * H;
  if (bp > 0x7FFFFFFFll || cdiv64(rows, 4) > 0x7FFFFFFFll) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!img_u8 || !files || !sizes || !work) return PPST_ENULL;
  unsigned char* filt = (unsigned char*)work;
  unsigned char* slots = filt + (int64_t)B * g.n_pad;
  unsigned* meta = (unsigned*)(slots + bp * PNG_SLOT);
  int64_t* offs = (int64_t*)((unsigned char*)meta + bp * 16);
  PngHead head;
  {
    unsigned char h[36] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    for (int k = 0; k < 4; ++k) { h[16 + k] = (unsigned char)((unsigned)W >> (24 - 8 * k)); h[20 + k] = (unsigned char)((unsigned)H >> (24 - 8 * k)); }
    h[24] = 8; h[25] = C == 1 ? 0 : 2; h[26] = h[27] = h[28] = 0;
    const unsigned c = host_crc32(h + 12, 17);
    for (int k = 0; k < 4; ++k) h[29 + k] = (unsigned char)(c >> (24 - 8 * k));
    h[33] = h[34] = h[35] = 0;
    for (int k = 0; k < 9; ++k) head.w[k] = (unsigned)h[4 * k] | ((unsigned)h[4 * k + 1] << 8) | ((unsigned)h[4 * k + 2] << 16) | ((unsigned)h[4 * k + 3] << 24);
  }
  hipStream_t st = as_stream(stream);
  static_assert(sizeof(DeflateLds) <= 48 * 1024, "three deflate workgroups per CU");
  PPST_LAUNCH(png_filter_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, st, (const unsigned char*)img_u8, filt, g, rows);
  PPST_LAUNCH(png_deflate_kernel, dim3((unsigned)bp), dim3(PNG_NT), 0, st, (const unsigned char*)filt, slots, meta, g);
  PPST_LAUNCH(png_layout_kernel, dim3((unsigned)B), dim3(256), 0, st, (const unsigned*)meta, offs, (unsigned char*)files, (int64_t*)sizes, g, head);
  PPST_LAUNCH(png_gather_kernel, dim3((unsigned)bp), dim3(256), 0, st, (const unsigned char*)slots, (const unsigned*)meta, (const int64_t*)offs,
              (unsigned char*)files, g);
  return PPST_LAUNCH_CHECK();
}
