// What the PNG encoder (png.hip) and decoder (png_decode.hip) share: the span-joining CRC-32, the Paeth predictor, deflate's
// code-length order, the joining of Adler-32 partial sums.  (What all four coders share: codec_common.h.)
#pragma once

// PNG's Paeth predictor: of left, above and upper left the one nearest to a + b - c, ties in that order
__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the order in which a dynamic deflate block sends the lengths of its code-length code (RFC 1951 3.2.7)
static __constant__ unsigned char PNG_CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Adler-32 over consecutive pieces: (a, b) are the sums of everything in front (1, 0 at the start); the piece of `len` bytes d_i
// that follows has the partial sums pa = sum d_i, pb = sum (len - i) d_i, both mod 65521.  32-bit arithmetic is exact: with
// a, b, pb and len mod 65521 all at most 65520, b + len a + pb <= 65520 * 65522 < 2^32.
#define PNG_ADLER 65521u
__device__ __forceinline__ void adler_join(unsigned& a, unsigned& b, unsigned len, unsigned pa, unsigned pb) {
  b = (b + (len % PNG_ADLER) * a + pb) % PNG_ADLER;
  a = (a + pa) % PNG_ADLER;
}

// --------------------------------------------------------------------------------------------------------------- CRC-32
// Reflected CRC-32 (polynomial 0xEDB88320) as arithmetic in GF(2)[x] / P: the register after n bytes from register I is
// I * x^(8n) + raw(message), so spans are summed by independent threads and joined by multiplying with x^(8 * bytes behind).
__device__ __forceinline__ unsigned crc_word(unsigned crc, unsigned w, int nbytes) {   // nbytes low bytes of w, in memory order
  crc ^= nbytes < 4 ? (w & ((1u << (8 * nbytes)) - 1u)) : w;
  for (int k = 0; k < nbytes * 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  return crc;
}
__device__ __forceinline__ unsigned crc_mul(unsigned a, unsigned b) {                  // a * b mod P (bit 31 = x^0)
  unsigned p = 0;
  for (unsigned m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return p;
}
__device__ __forceinline__ unsigned crc_xpow8(unsigned n) {                            // x^(8n) mod P
  unsigned r = 0x80000000u, q = 0x00800000u;                                           // x^0, x^8
  for (; n; n >>= 1) {
    if (n & 1u) r = crc_mul(r, q);
    q = crc_mul(q, q);
  }
  return r;
}
