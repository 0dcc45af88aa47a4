// What the PNG encoder (png.hip) and decoder (png_decode.hip) share: the span-joining CRC-32.
#pragma once

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
