// JPEG encode on the device: baseline sequential DCT (ITU-T T.81), JFIF 1.01 (DESIGN.md "JPEG encode on the device").
//   1. jpeg_scan_kernel    one workgroup per RESTART INTERVAL (JPEG_NBLK blocks: 96 grey, 32 MCUs at 4:4:4, 16 MCUs at 4:2:0 --
//                          a count of MCUs, never of rows: the LDS footprint does not know the image width).
//                          samples    pixels -> Y / Cb / Cr in 16-bit fixed point, 2 x 2 chroma mean, level shift, edge replication,
//                                     int16 in LDS;
//                          DCT        separable 8 x 8 DCT-II in INTEGER fixed point (a 2^14-scaled table, rows then columns),
//                                     quantised to nearest (halves away from zero), int16 in zigzag order in LDS;
//                          entropy    one wave per block, lane k = zigzag coefficient k: the zero run in front of a coefficient is
//                                     the ballot mask below the lane and a count of leading zeros; bit lengths are summed over lanes
//                                     and then over the interval's blocks in scan order, every lane ORs its code MSB-first into
//                                     the LDS image; the four Annex K tables, DC predictors start at 0 in every interval;
//                          stuffing   pad with 1-bits to a byte, a prefix over the count of FF bytes places every byte (and the 00
//                                     behind an FF) in the workgroup's own slot; one record: the bytes.
//   2. jpeg_layout_kernel  one workgroup per image: interval offsets (exclusive sum), the header, EOI, the file length;
//      jpeg_gather_kernel  one workgroup per interval: slot -> its offset at any byte alignment, RSTm behind it.
// All of it is integer code: the bytes are a pure function of the pixels, whatever the batch.  No workgroup waits for another.
// Shared with the other coders: the workgroup scan and the slot-to-file copy (codec_common.h), the zigzag order (jpeg_common.h).
#include "common.h"
#include "codec_common.h"
#include "jpeg_common.h"
#include <string.h>

#define JPEG_NT 256                            // threads of the scan workgroup
#define JPEG_NBLK 96                           // blocks per restart interval (a multiple of 1, 3 and 6 blocks per MCU)
// longest DC code (11, chroma) + 11 magnitude bits, then 63 x (longest AC code (16) + 10 magnitude bits): no block takes more
#define JPEG_BLOCK_BITS (11 + 11 + 63 * (16 + 10))
#define JPEG_BLOCK_WORDS ((JPEG_BLOCK_BITS + 31) / 32)
#define JPEG_IMG_WORDS (JPEG_NBLK * JPEG_BLOCK_WORDS + 4)
// bytes of an interval of nb blocks: the bits padded to a byte, every byte an FF with its 00
#define JPEG_IVL_BYTES(nb) (2 * (((int64_t)(nb) * JPEG_BLOCK_BITS + 7) >> 3))
#define JPEG_SLOT 39840
#define JPEG_HEAD_MAX 640
static_assert(JPEG_SLOT == JPEG_IVL_BYTES(JPEG_NBLK) && JPEG_SLOT % 16 == 0, "slot = the worst interval, 16-byte aligned");
static_assert(JPEG_NBLK <= 128 && JPEG_NBLK % 6 == 0, "two scan rounds of one wave; whole MCUs");

// ------------------------------------------------------------------------------------------------------------- the tables
// T.81 Annex K: K.1 / K.2 (quantisation, natural order), K.3 - K.6 (the "typical" Huffman tables).  One initialiser each, read by
// the host (header) and the device (codes): both write from the same constants.  The zigzag order (H_ZIGZAG, D_ZIGZAG): jpeg_common.h.
#define JPEG_QBASE { \
  {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, \
   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99}, \
  {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, \
   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}}
#define JPEG_DC_BITS {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}}
#define JPEG_DC_VALS {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}
#define JPEG_AC_BITS {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}}
#define JPEG_AC_VALS { \
  {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, \
   0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, \
   0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, \
   0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, \
   0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, \
   0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, \
   0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}, \
  {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, \
   0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, \
   0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, \
   0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, \
   0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, \
   0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, \
   0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}
#define JPEG_NDC 12
#define JPEG_NAC 162

static const unsigned char H_QBASE[2][64] = JPEG_QBASE;
static const unsigned char H_DC_BITS[2][16] = JPEG_DC_BITS;
static const unsigned char H_DC_VALS[JPEG_NDC] = JPEG_DC_VALS;
static const unsigned char H_AC_BITS[2][16] = JPEG_AC_BITS;
static const unsigned char H_AC_VALS[2][JPEG_NAC] = JPEG_AC_VALS;
__constant__ unsigned char D_DC_BITS[2][16] = JPEG_DC_BITS;
__constant__ unsigned char D_DC_VALS[JPEG_NDC] = JPEG_DC_VALS;
__constant__ unsigned char D_AC_BITS[2][16] = JPEG_AC_BITS;
__constant__ unsigned char D_AC_VALS[2][JPEG_NAC] = JPEG_AC_VALS;
// The DCT in fixed point: T[u][x] = round(2^14 * c(u) / 2 * cos((2 x + 1) u pi / 16)), c(0) = 1 / sqrt 2, else 1 -- literals, not
// a call of cos: 8192 * cos(k pi / 16) = 8034.6, 7568.4, 6811.4, 5792.6, 4551.2, 3134.9, 1598.2 for k = 1 .. 7.
// Rows: a[u] = (sum_x s[x] T[u][x] + 128) >> 8 (scale 2^6; |a| <= 362 * 64: an int16); columns: b[v] = sum_y a[y] T[v][y] (scale
// 2^20; |b| < 1.08e9: an int32); quantised q = sign(b) * ((|b| + (Q << 19)) / (Q << 20)): to nearest, halves away from zero.
__constant__ short D_DCT[8][8] = {{5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793},
                                  {8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035},
                                  {7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568},
                                  {6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811},
                                  {5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793},
                                  {4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551},
                                  {3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135},
                                  {1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598}};

struct JpegGeom {
  int H, W, C;
  int ss;                  // 1: one block per component and MCU (grey, 4:4:4); 2: 4:2:0, an MCU is 16 x 16 pixels
  int bpm;                 // blocks per MCU: 1, 3, 6
  int mw;                  // MCUs per MCU row
  int nmcu;                // MCUs per image
  int R;                   // MCUs per restart interval: JPEG_NBLK / bpm
  int NI;                  // intervals per image
  int head;                // bytes from SOI through SOS
  int64_t bound;           // bytes of one file slot
};
struct JpegQ { unsigned char q[2][64]; };                  // the scaled tables, natural order
struct JpegHead { unsigned w[JPEG_HEAD_MAX / 4]; };        // the header bytes (built on the host), little-endian words

// ------------------------------------------------------------------------------------------------------------------- scan
struct JpegLds {
  union {
    short smp[JPEG_NBLK][64];          // level-shifted samples, then the row pass in place
    unsigned img[JPEG_IMG_WORDS];      // the interval's bits, MSB-first: byte i = img[i / 4] >> (24 - 8 * (i % 4))
  } u;
  short coef[JPEG_NBLK][64];           // quantised, zigzag order
  unsigned ac[2][256];                 // (length << 16) | code by symbol; [0] luma, [1] chroma
  unsigned dc[2][JPEG_NDC];
  unsigned char izz[64];               // natural index -> zigzag position
  unsigned blkbits[JPEG_NBLK];
  unsigned blkoff[JPEG_NBLK];
  int wave_tot[2][JPEG_NT / 64];
  unsigned total;
};

// `n` (1 .. 64) low bits of v at bit `pos` of the image, MSB-first (the image starts as zeros: OR-ing is placing)
__device__ __forceinline__ void jpeg_put_bits(unsigned* img, unsigned pos, unsigned long long v, int n) {
  const unsigned w = pos >> 5, s = pos & 31;
  if (n == 0 || w + 2 >= JPEG_IMG_WORDS) return;        // (no code of the tables reaches the end of the image: JPEG_BLOCK_BITS)
  const unsigned long long top = v << (64 - n);
  const unsigned long long a = top >> s;
  const unsigned lo = s ? (unsigned)((top << (64 - s)) >> 32) : 0u;
  if ((unsigned)(a >> 32)) atomicOr(&img[w], (unsigned)(a >> 32));
  if ((unsigned)a) atomicOr(&img[w + 1], (unsigned)a);
  if (lo) atomicOr(&img[w + 2], lo);
}

// The code of lane `lane`'s coefficient v (lane 0: the DC difference) of a block whose non-zero AC lanes are `acmask`:
// ZRL x (run >> 4), the code of (run & 15) << 4 | size, the magnitude bits; lane 63 sends EOB when its coefficient is zero (the
// last non-zero one is in front of it).  At most 3 * 11 + 16 + 10 bits.
__device__ __forceinline__ void jpeg_lane_code(int v, int lane, unsigned long long acmask, const unsigned* dc, const unsigned* ac,
                                               unsigned long long& bits, int& nbits) {
  bits = 0; nbits = 0;
  const int mag = v < 0 ? -v : v;
  const int size = mag ? 32 - __clz(mag) : 0;
  const unsigned low = (unsigned)(v + (v >> 31)) & ((1u << size) - 1u);        // v, or v - 1 when negative: `size` low bits
  if (lane == 0) {
    const unsigned h = dc[size];
    bits = ((unsigned long long)(h & 0xffffu) << size) | low;
    nbits = (int)(h >> 16) + size;
  } else if (v != 0) {
    const unsigned long long below = acmask & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;               // the DC's place when no AC is in front
    const int run = lane - 1 - prev;
    const unsigned z = ac[0xF0], h = ac[((run & 15) << 4) | size];
    for (int k = 0; k < (run >> 4); ++k) { bits = (bits << (z >> 16)) | (z & 0xffffu); nbits += (int)(z >> 16); }
    bits = (((bits << (h >> 16)) | (h & 0xffffu)) << size) | low;
    nbits += (int)(h >> 16) + size;
  } else if (lane == 63) {
    const unsigned h = ac[0x00];
    bits = h & 0xffffu;
    nbits = (int)(h >> 16);
  }
}

__device__ __forceinline__ int jpeg_ycc(int comp, int r, int g, int b) {
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(JPEG_NT) void jpeg_scan_kernel(const unsigned char* __restrict__ img, unsigned char* __restrict__ slots,
                                                            unsigned* __restrict__ meta, JpegGeom g, JpegQ qt) {
  __shared__ JpegLds s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int64_t b = blk / g.NI;
  const int it = (int)(blk - b * g.NI);
  const int m0 = it * g.R;
  const int nm = g.nmcu - m0 < g.R ? g.nmcu - m0 : g.R;           // 1 .. R MCUs
  const int nb = nm * g.bpm;                                       // 1 .. JPEG_NBLK blocks
  const unsigned char* src = img + b * (int64_t)g.H * g.W * g.C;

  // ---- the code tables from the BITS / HUFFVAL lists (T.81 Annex C), the inverse zigzag; a symbol without a code has length 0
  for (int e = tid; e < 2 * 256; e += JPEG_NT) (&s.ac[0][0])[e] = 0;
  __syncthreads();
  for (int e = tid; e < 2 * (JPEG_NDC + JPEG_NAC); e += JPEG_NT) {
    const int t = e / (JPEG_NDC + JPEG_NAC);
    int p = e - t * (JPEG_NDC + JPEG_NAC);
    const bool is_ac = p >= JPEG_NDC;
    if (is_ac) p -= JPEG_NDC;
    const unsigned char* nbits = is_ac ? D_AC_BITS[t] : D_DC_BITS[t];
    unsigned code = 0, len = 0;
    int first = 0;
    for (int l = 1; l <= 16; ++l) {
      const int n = nbits[l - 1];
      if (p < first + n) { code += (unsigned)(p - first); len = (unsigned)l; break; }
      code = (code + (unsigned)n) << 1;
      first += n;
    }
    if (is_ac) s.ac[t][D_AC_VALS[t][p]] = (len << 16) | code;
    else s.dc[t][D_DC_VALS[p]] = (len << 16) | code;
  }
  if (tid < 64) s.izz[D_ZIGZAG[tid]] = (unsigned char)tid;

  // ---- samples: coordinates beyond the image repeat its last column / row
  for (int e = tid; e < nb * 64; e += JPEG_NT) {
    const int j = e >> 6, sy = (e >> 3) & 7, sx = e & 7;
    const int mcu = j / g.bpm, k = j - mcu * g.bpm;
    const int m = m0 + mcu;
    const int my = m / g.mw, mx = m - my * g.mw;
    int val;
    if (g.C == 1) {
      const int x = min(mx * 8 + sx, g.W - 1), y = min(my * 8 + sy, g.H - 1);
      val = src[(int64_t)y * g.W + x];
    } else if (g.ss == 1 || k < 4) {
      const int x0 = g.ss == 1 ? mx * 8 + sx : mx * 16 + (k & 1) * 8 + sx;
      const int y0 = g.ss == 1 ? my * 8 + sy : my * 16 + (k >> 1) * 8 + sy;
      const int x = min(x0, g.W - 1), y = min(y0, g.H - 1);
      const unsigned char* p = src + ((int64_t)y * g.W + x) * 3;
      val = jpeg_ycc(g.ss == 1 ? k : 0, p[0], p[1], p[2]);
    } else {
      int sum = 0;
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
          const int x = min(mx * 16 + 2 * sx + dx, g.W - 1), y = min(my * 16 + 2 * sy + dy, g.H - 1);
          const unsigned char* p = src + ((int64_t)y * g.W + x) * 3;
          sum += jpeg_ycc(k - 3, p[0], p[1], p[2]);
        }
      val = (sum + 1 + (sx & 1)) >> 2;                             // the bias alternates 1, 2 along x
    }
    s.u.smp[j][sy * 8 + sx] = (short)(val - 128);
  }
  __syncthreads();
  // ---- DCT rows, in place (one thread per row of a block)
  for (int e = tid; e < nb * 8; e += JPEG_NT) {
    short* row = &s.u.smp[e >> 3][(e & 7) * 8];
    int x[8], a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = row[i];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int acc = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += x[i] * D_DCT[u][i];
      a[u] = (acc + 128) >> 8;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) row[u] = (short)a[u];
  }
  __syncthreads();
  // ---- DCT columns + quantiser (one thread per column of a block), zigzag order out
  for (int e = tid; e < nb * 8; e += JPEG_NT) {
    const int j = e >> 3, col = e & 7;
    const int k = j % g.bpm;
    const unsigned char* q = qt.q[(g.C == 1 || k < g.bpm - 2) ? 0 : 1];
    int y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = s.u.smp[j][i * 8 + col];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      int acc = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += y[i] * D_DCT[v][i];
      const unsigned d = (unsigned)q[v * 8 + col] << 20;
      const unsigned r = ((unsigned)abs(acc) + (d >> 1)) / d;
      s.coef[j][s.izz[v * 8 + col]] = (short)(acc < 0 ? -(int)r : (int)r);
    }
  }
  __syncthreads();
  // ---- the bit image starts as zeros (the samples it overlays are spent)
  for (int i = tid; i < JPEG_IMG_WORDS; i += JPEG_NT) s.u.img[i] = 0;
  // ---- entropy, first pass: bits per block
  for (int j = wave; j < nb; j += JPEG_NT / 64) {
    const int k = j % g.bpm;
    const int cls = (g.C == 1 || k < g.bpm - 2) ? 0 : 1;
    // the block of the same component in front of this one: the Y blocks of a 4:2:0 MCU follow each other
    const int back = (g.ss == 2 && k < 4) ? (k > 0 ? 1 : 3) : g.bpm;
    int v = s.coef[j][lane];
    if (lane == 0) v -= (j >= back) ? s.coef[j - back][0] : 0;
    const unsigned long long acmask = __ballot(v != 0) & ~1ull;
    unsigned long long bits;
    int n;
    jpeg_lane_code(v, lane, acmask, s.dc[cls], s.ac[cls], bits, n);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) s.blkbits[j] = (unsigned)n;
  }
  __syncthreads();
  if (wave == 0) {                                                  // exclusive sum over the blocks in scan order
    const unsigned v0 = lane < nb ? s.blkbits[lane] : 0u, v1 = lane + 64 < nb ? s.blkbits[lane + 64] : 0u;
    unsigned i0 = v0, i1 = v1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t0 = __shfl_up(i0, o, 64), t1 = __shfl_up(i1, o, 64);
      if (lane >= o) { i0 += t0; i1 += t1; }
    }
    const unsigned tot0 = __shfl(i0, 63, 64), tot1 = __shfl(i1, 63, 64);
    if (lane < nb) s.blkoff[lane] = i0 - v0;
    if (lane + 64 < nb) s.blkoff[lane + 64] = tot0 + i1 - v1;
    if (lane == 0) s.total = tot0 + tot1;
  }
  __syncthreads();
  // ---- second pass: every lane places its code
  for (int j = wave; j < nb; j += JPEG_NT / 64) {
    const int k = j % g.bpm;
    const int cls = (g.C == 1 || k < g.bpm - 2) ? 0 : 1;
    const int back = (g.ss == 2 && k < 4) ? (k > 0 ? 1 : 3) : g.bpm;
    int v = s.coef[j][lane];
    if (lane == 0) v -= (j >= back) ? s.coef[j - back][0] : 0;
    const unsigned long long acmask = __ballot(v != 0) & ~1ull;
    unsigned long long bits;
    int n;
    jpeg_lane_code(v, lane, acmask, s.dc[cls], s.ac[cls], bits, n);
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    jpeg_put_bits(s.u.img, s.blkoff[j] + (unsigned)(inc - n), bits, n);
  }
  __syncthreads();
  const unsigned total = s.total;                                   // <= nb * JPEG_BLOCK_BITS
  if (tid == 0 && (total & 7u)) jpeg_put_bits(s.u.img, total, (1ull << (8 - (total & 7u))) - 1ull, 8 - (int)(total & 7u));
  __syncthreads();
  // ---- stuffing: a word (four bytes) per thread and round; a prefix over the FF count gives every byte its place in the slot
  const unsigned nbytes = min((total + 7u) >> 3, (unsigned)(JPEG_SLOT / 2));       // (the bound holds by the tables; never write past the slot)
  unsigned char* out = slots + blk * JPEG_SLOT;
  unsigned base = 0;
  int slot = 0;
  for (unsigned w0 = 0; w0 * 4 < nbytes; w0 += JPEG_NT, slot ^= 1) {
    const unsigned w = w0 + tid;
    const int nv = 4 * w < nbytes ? (nbytes - 4 * w < 4 ? (int)(nbytes - 4 * w) : 4) : 0;
    const unsigned word = nv ? s.u.img[w] : 0u;
    unsigned nff = 0;
    for (int i = 0; i < nv; ++i) nff += ((word >> (24 - 8 * i)) & 255u) == 255u;
    int round_bytes;                                                // (wg_scan: codec_common.h; <= 8 bytes per thread)
    unsigned at = base + (unsigned)wg_scan<JPEG_NT, false>(nv + (int)nff, round_bytes, s.wave_tot, slot);
    base += (unsigned)round_bytes;
    for (int i = 0; i < nv; ++i) {
      const unsigned c = (word >> (24 - 8 * i)) & 255u;
      out[at++] = (unsigned char)c;
      if (c == 255u) out[at++] = 0;
    }
  }
  if (tid == 0) meta[blk] = base;                                   // <= 2 * nbytes <= JPEG_SLOT
}

// --------------------------------------------------------------------------------------------------------------- assemble
// One workgroup per image: interval i starts behind the header, the intervals in front of it and their RST markers.
__global__ __launch_bounds__(JPEG_NT) void jpeg_layout_kernel(const unsigned* __restrict__ meta, int64_t* __restrict__ offs,
                                                              unsigned char* __restrict__ files, int64_t* __restrict__ sizes, JpegGeom g,
                                                              JpegHead head) {
  __shared__ int wave_tot[2][JPEG_NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned char* file = files + (int64_t)b * g.bound;
  // (the bound is below 2^32: jpeg_geom.  The base passes 2^31 in a large file; a round's prefix, <= 256 slots, fits an int)
  unsigned base = (unsigned)g.head;
  int slot = 0;
  for (int i0 = 0; i0 < g.NI; i0 += JPEG_NT, slot ^= 1) {
    const int i = i0 + tid;
    const unsigned v = i < g.NI ? meta[(int64_t)b * g.NI + i] + (i < g.NI - 1 ? 2u : 0u) : 0u;
    int round_bytes;
    const unsigned at = base + (unsigned)wg_scan<JPEG_NT, false>((int)v, round_bytes, wave_tot, slot);
    base += (unsigned)round_bytes;
    if (i < g.NI) offs[(int64_t)b * g.NI + i] = at;
  }
  for (int i = tid; i < g.head; i += JPEG_NT) file[i] = (unsigned char)(head.w[i >> 2] >> (8 * (i & 3)));
  if (tid == 0) {
    file[base] = 0xFF; file[base + 1] = 0xD9;                       // EOI
    sizes[b] = (int64_t)base + 2;
  }
}

// one workgroup per interval: slot -> its place in the file (any byte alignment there), RSTm behind every interval but the last
__global__ __launch_bounds__(256) void jpeg_gather_kernel(const unsigned char* __restrict__ slots, const unsigned* __restrict__ meta,
                                                          const int64_t* __restrict__ offs, unsigned char* __restrict__ files, JpegGeom g) {
  const int64_t blk = blockIdx.x;
  const int64_t b = blk / g.NI;
  const int it = (int)(blk - b * g.NI);
  const unsigned n = meta[blk];
  const unsigned char* src = slots + blk * JPEG_SLOT;
  unsigned char* dst = files + b * g.bound + offs[blk];
  if (threadIdx.x == 0 && it < g.NI - 1) { dst[n] = 0xFF; dst[n + 1] = (unsigned char)(0xD0 + (it & 7)); }
  slot_to_file<256>(src, dst, n);
}

// ------------------------------------------------------------------------------------------------------------------- host
// libjpeg's scaling of the Annex K tables, clamped to 1 .. 255 (baseline)
static void jpeg_qtables(int quality, JpegQ* q) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = (H_QBASE[t][i] * s + 50) / 100;
      q->q[t][i] = (unsigned char)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

// SOI, APP0 (JFIF 1.01, density 1:1), DQT x 1 | 2, SOF0, DHT x 2 | 4 (DC, AC per table), DRI, SOS -> bytes written (<= JPEG_HEAD_MAX)
static int jpeg_header_bytes(const JpegGeom& g, const JpegQ& q, unsigned char* o) {
  const int nc = g.C == 1 ? 1 : 3, ntab = g.C == 1 ? 1 : 2;
  int n = 0;
  auto u8 = [&](int v) { o[n++] = (unsigned char)v; };
  auto u16 = [&](int v) { u8(v >> 8); u8(v & 255); };
  u16(0xFFD8);
  u16(0xFFE0); u16(16); u8('J'); u8('F'); u8('I'); u8('F'); u8(0); u8(1); u8(1); u8(0); u16(1); u16(1); u8(0); u8(0);
  for (int t = 0; t < ntab; ++t) {
    u16(0xFFDB); u16(67); u8(t);
    for (int k = 0; k < 64; ++k) u8(q.q[t][H_ZIGZAG[k]]);
  }
  u16(0xFFC0); u16(8 + 3 * nc); u8(8); u16(g.H); u16(g.W); u8(nc);
  for (int c = 0; c < nc; ++c) { u8(c + 1); u8(c == 0 ? (g.ss << 4) | g.ss : 0x11); u8(c == 0 ? 0 : 1); }
  for (int t = 0; t < ntab; ++t) {
    u16(0xFFC4); u16(2 + 1 + 16 + JPEG_NDC); u8(t);
    for (int k = 0; k < 16; ++k) u8(H_DC_BITS[t][k]);
    for (int k = 0; k < JPEG_NDC; ++k) u8(H_DC_VALS[k]);
    u16(0xFFC4); u16(2 + 1 + 16 + JPEG_NAC); u8(0x10 | t);
    for (int k = 0; k < 16; ++k) u8(H_AC_BITS[t][k]);
    for (int k = 0; k < JPEG_NAC; ++k) u8(H_AC_VALS[t][k]);
  }
  u16(0xFFDD); u16(4); u16(g.R);
  u16(0xFFDA); u16(6 + 2 * nc); u8(nc);
  for (int c = 0; c < nc; ++c) { u8(c + 1); u8(c == 0 ? 0x00 : 0x11); }
  u8(0); u8(63); u8(0);
  return n;
}

// 0 = fine.  A file's scan offsets are 32-bit: the worst-case file has to stay below 2^32 bytes.
static int jpeg_geom(int H, int W, int C, int subsampling, JpegGeom* g) {
  if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return PPST_EINVAL;
  if (subsampling != PPST_JPEG_444 && subsampling != PPST_JPEG_420) return PPST_EINVAL;
  g->H = H; g->W = W; g->C = C;
  g->ss = (C == 3 && subsampling == PPST_JPEG_420) ? 2 : 1;
  g->bpm = C == 1 ? 1 : (g->ss == 2 ? 6 : 3);
  const int mcu = 8 * g->ss;
  g->mw = cdiv(W, mcu);
  const int64_t nmcu = (int64_t)g->mw * cdiv(H, mcu);
  g->R = JPEG_NBLK / g->bpm;
  const int64_t full = nmcu / g->R, rem = nmcu % g->R;
  g->head = 2 + 18 + 69 * (C == 1 ? 1 : 2) + (10 + 3 * (C == 1 ? 1 : 3)) + 216 * (C == 1 ? 1 : 2) + 6 + (8 + 2 * (C == 1 ? 1 : 3));
  // header; per interval its worst-case bytes and a marker (RSTm, behind the last one EOI)
  const int64_t bytes = g->head + full * (JPEG_SLOT + 2) + (rem ? JPEG_IVL_BYTES(rem * g->bpm) + 2 : 0);
  if (bytes > 0xFFFFFFFFll - 16) return PPST_EINVAL;
  g->nmcu = (int)nmcu;
  g->NI = (int)(full + (rem ? 1 : 0));
  g->bound = (bytes + 15) & ~15ll;
  return PPST_OK;
}

extern "C" int64_t ppst_jpeg_bound(int H, int W, int C, int subsampling) {
  JpegGeom g;
  if (jpeg_geom(H, W, C, subsampling, &g) != PPST_OK) return PPST_EINVAL;
  return g.bound;
}

// [B][NI][JPEG_SLOT] interval slots | [B][NI] int64 offsets | [B][NI] records (bytes)
extern "C" int64_t ppst_jpeg_ws(int B, int H, int W, int C, int subsampling) {
  JpegGeom g;
  if (B < 0 || jpeg_geom(H, W, C, subsampling, &g) != PPST_OK) return PPST_EINVAL;
  const int64_t bi = (int64_t)(B > 0 ? B : 1) * g.NI;
  return bi * JPEG_SLOT + bi * 8 + ((bi * 4 + 15) & ~15ll);
}

extern "C" int64_t ppst_jpeg_header(int H, int W, int C, int quality, int subsampling, void* out, int64_t cap) {
  JpegGeom g;
  if (quality < 1 || quality > 100 || jpeg_geom(H, W, C, subsampling, &g) != PPST_OK) return PPST_EINVAL;
  JpegQ q;
  jpeg_qtables(quality, &q);
  unsigned char h[JPEG_HEAD_MAX];
  const int n = jpeg_header_bytes(g, q, h);
  if (out) {
    if (cap < n) return PPST_EINVAL;
    memcpy(out, h, (size_t)n);
  }
  return n;
}

extern "C" int ppst_jpeg_encode(const void* img_u8, void* files, void* sizes, int B, int H, int W, int C, int quality, int subsampling,
                                void* work, void* stream) {
  JpegGeom g;
  if (B < 0 || quality < 1 || quality > 100 || jpeg_geom(H, W, C, subsampling, &g) != PPST_OK) return PPST_EINVAL;
  const int64_t bi = (int64_t)B * g.NI;
  if (bi > 0x7FFFFFFFll) return PPST_EINVAL;
  if (B == 0) return PPST_OK;
  if (!img_u8 || !files || !sizes || !work) return PPST_ENULL;
  unsigned char* slots = (unsigned char*)work;
  int64_t* offs = (int64_t*)(slots + bi * JPEG_SLOT);
  unsigned* meta = (unsigned*)((unsigned char*)offs + bi * 8);
  JpegQ q;
  jpeg_qtables(quality, &q);
  JpegHead head;
  {
    unsigned char h[JPEG_HEAD_MAX] = {0};
    const int n = jpeg_header_bytes(g, q, h);
    if (n != g.head) return PPST_EINVAL;
    for (int k = 0; k < JPEG_HEAD_MAX / 4; ++k)
      head.w[k] = (unsigned)h[4 * k] | ((unsigned)h[4 * k + 1] << 8) | ((unsigned)h[4 * k + 2] << 16) | ((unsigned)h[4 * k + 3] << 24);
  }
  hipStream_t st = as_stream(stream);
  static_assert(sizeof(JpegLds) <= 40 * 1024, "four scan workgroups per CU");
  PPST_LAUNCH(jpeg_scan_kernel, dim3((unsigned)bi), dim3(JPEG_NT), 0, st, (const unsigned char*)img_u8, slots, meta, g, q);
  PPST_LAUNCH(jpeg_layout_kernel, dim3((unsigned)B), dim3(JPEG_NT), 0, st, (const unsigned*)meta, offs, (unsigned char*)files, (int64_t*)sizes, g, head);
  PPST_LAUNCH(jpeg_gather_kernel, dim3((unsigned)bi), dim3(256), 0, st, (const unsigned char*)slots, (const unsigned*)meta, (const int64_t*)offs,
              (unsigned char*)files, g);
  return PPST_LAUNCH_CHECK();
}
