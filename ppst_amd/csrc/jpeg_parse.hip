// JPEG decode on the device, the host half: ppst_jpeg_parse walks a file's markers and fills the descriptor the kernels of
// jpeg_decode.hip read (include/ppst_hip.h "JPEG decode on the device").  Plain C++ with no GPU call and no dependency but the
// header: tests/jpeg_parse_san.cpp compiles this file as host code under the address and undefined-behaviour sanitizers.
// Every read goes through Rd (parse_reader.h, shared with png_parse.hip), which knows n: no segment length is trusted.
#include <string.h>
#include "../../include/ppst_hip.h"
#include "parse_reader.h"

extern "C" int ppst_jpeg_parse(const void* file, int64_t n, ppst_jpeg_dec_image* out) {
  if (!out) return PPST_ENULL;
  memset(out, 0, sizeof(*out));
  if (n < 0) return PPST_EINVAL;
  if (!file) return n == 0 ? PPST_JPEG_E_TRUNCATED : PPST_ENULL;
  if (n >= 0x7FFFFFF0ll) return PPST_JPEG_E_SIZE;                             // scan_off / scan_len are 32-bit
  const Rd r = {(const unsigned char*)file, n};
  if (!r.has(0, 2)) return PPST_JPEG_E_TRUNCATED;
  if (r.u8(0) != 0xFF || r.u8(1) != 0xD8) return PPST_JPEG_E_NOT_JPEG;
  unsigned char qt[4][64];
  bool have_qt[4] = {false, false, false, false}, have_ht[4] = {false, false, false, false}, have_sof = false;
  int tq[3] = {0, 0, 0}, cid[3] = {0, 0, 0};
  int adobe_transform = -1;                                                   // -1: no Adobe APP14
  bool jfif = false;
  int64_t at = 2;
  for (;;) {
    if (!r.has(at, 2)) return PPST_JPEG_E_TRUNCATED;
    if (r.u8(at) != 0xFF) return PPST_JPEG_E_ORDER;
    const int m = r.u8(at + 1);
    if (m == 0xFF) { at += 1; continue; }                                     // fill byte in front of a marker
    if (m == 0xD8 || m == 0xD9 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return PPST_JPEG_E_ORDER;
    if (!r.has(at + 2, 2)) return PPST_JPEG_E_TRUNCATED;
    const int len = r.u16(at + 2);                                            // counts its own two bytes
    if (len < 2) return PPST_JPEG_E_ORDER;
    if (!r.has(at + 2, len)) return PPST_JPEG_E_TRUNCATED;
    const int64_t body = at + 4, end = at + 2 + len;
    const int blen = len - 2;
    if (m == 0xC0) {
      if (have_sof) return PPST_JPEG_E_ORDER;
      if (blen < 6) return PPST_JPEG_E_ORDER;
      if (r.u8(body) != 8) return PPST_JPEG_E_PRECISION;
      out->H = r.u16(body + 1);
      out->W = r.u16(body + 3);
      const int nc = r.u8(body + 5);
      if (out->H == 0 || out->W == 0) return PPST_JPEG_E_SIZE;
      if (nc != 1 && nc != 3) return PPST_JPEG_E_COMPONENTS;
      if (blen != 6 + 3 * nc) return PPST_JPEG_E_ORDER;
      out->ncomp = nc;
      for (int c = 0; c < nc; ++c) {
        cid[c] = r.u8(body + 6 + 3 * c);
        out->hs[c] = r.u8(body + 7 + 3 * c) >> 4;
        out->vs[c] = r.u8(body + 7 + 3 * c) & 15;
        tq[c] = r.u8(body + 8 + 3 * c);
        if (tq[c] > 3 || out->hs[c] < 1 || out->hs[c] > 4 || out->vs[c] < 1 || out->vs[c] > 4) return PPST_JPEG_E_ORDER;
      }
      if (nc == 1) out->ss = 1;
      else {
        if (out->hs[1] != 1 || out->vs[1] != 1 || out->hs[2] != 1 || out->vs[2] != 1 || out->hs[0] != out->vs[0] || out->hs[0] > 2)
          return PPST_JPEG_E_SAMPLING;
        out->ss = out->hs[0];
      }
      have_sof = true;
    } else if (m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7)) {
      return PPST_JPEG_E_PROGRESSIVE;
    } else if (m >= 0xC9 && m <= 0xCF && m != 0xCC) {
      return PPST_JPEG_E_ARITHMETIC;
    } else if (m == 0xCC) {
      return PPST_JPEG_E_ARITHMETIC;                                          // DAC: arithmetic conditioning
    } else if (m == 0xDB) {
      int64_t i = body;
      while (i < end) {
        const int pq = r.u8(i) >> 4, id = r.u8(i) & 15;
        if (pq != 0) return PPST_JPEG_E_DQT16;
        if (id > 3 || end - i < 65) return PPST_JPEG_E_ORDER;
        for (int k = 0; k < 64; ++k) qt[id][k] = (unsigned char)r.u8(i + 1 + k);
        have_qt[id] = true;
        i += 65;
      }
    } else if (m == 0xC4) {
      int64_t i = body;
      while (i < end) {
        if (end - i < 17) return PPST_JPEG_E_ORDER;
        const int tc = r.u8(i) >> 4, id = r.u8(i) & 15;
        if (tc > 1 || id > 1) return PPST_JPEG_E_HUFFMAN;
        const int t = tc * 2 + id;
        int cnt = 0;
        unsigned code = 0;
        for (int l = 0; l < 16; ++l) {
          const int b = r.u8(i + 1 + l);
          out->bits[t][l] = (uint8_t)b;
          cnt += b;
          code += (unsigned)b;
          if (code > (1u << (l + 1))) return PPST_JPEG_E_HUFFMAN;               // more codes than the length has
          code <<= 1;
        }
        if (cnt > 256) return PPST_JPEG_E_HUFFMAN;
        if (end - i < 17 + cnt) return PPST_JPEG_E_ORDER;
        memset(out->vals[t], 0, 256);
        for (int k = 0; k < cnt; ++k) out->vals[t][k] = (uint8_t)r.u8(i + 17 + k);
        have_ht[t] = true;
        i += 17 + cnt;
      }
    } else if (m == 0xDD) {
      if (blen != 2) return PPST_JPEG_E_ORDER;
      out->dri = r.u16(body);
    } else if (m == 0xEE) {
      if (blen >= 12 && memcmp(r.p + body, "Adobe", 5) == 0) adobe_transform = r.u8(body + 11);
    } else if (m == 0xE0) {
      if (blen >= 5 && memcmp(r.p + body, "JFIF", 5) == 0) jfif = true;
    } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
      // APPn / COM: skipped
    } else if (m == 0xDA) {
      if (!have_sof) return PPST_JPEG_E_ORDER;
      if (blen < 1) return PPST_JPEG_E_ORDER;
      const int ns = r.u8(body);
      if (ns < 1 || ns > 4 || blen != 4 + 2 * ns) return PPST_JPEG_E_ORDER;
      if (ns != out->ncomp) return PPST_JPEG_E_MULTISCAN;
      for (int c = 0; c < ns; ++c) {
        if (r.u8(body + 1 + 2 * c) != cid[c]) return PPST_JPEG_E_ORDER;
        const int td = r.u8(body + 2 + 2 * c) >> 4, ta = r.u8(body + 2 + 2 * c) & 15;
        if (td > 1 || ta > 1 || !have_ht[td] || !have_ht[2 + ta]) return PPST_JPEG_E_HUFFMAN;
        out->dc_tab[c] = (uint8_t)td;
        out->ac_tab[c] = (uint8_t)ta;
      }
      if (r.u8(body + 1 + 2 * ns) != 0 || r.u8(body + 2 + 2 * ns) != 63 || r.u8(body + 3 + 2 * ns) != 0) return PPST_JPEG_E_SCAN;
      // libjpeg's colour-space rule for three components: JFIF says YCbCr; else Adobe's transform flag says; else the ids 'R' 'G' 'B'
      // say RGB (anything else is taken as YCbCr)
      if (out->ncomp == 3 && !jfif &&
          (adobe_transform == 0 || (adobe_transform < 0 && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B')))
        return PPST_JPEG_E_ADOBE_RGB;
      for (int c = 0; c < out->ncomp; ++c) {
        if (!have_qt[tq[c]]) return PPST_JPEG_E_ORDER;
        memcpy(out->qt[c], qt[tq[c]], 64);
      }
      at = end;
      break;
    } else {
      return PPST_JPEG_E_ORDER;
    }
    at = end;
  }
  // the entropy-coded segment: up to the first FF D9
  int64_t e = at;
  for (;; ++e) {
    if (!r.has(e, 2)) return PPST_JPEG_E_TRUNCATED;
    if (r.u8(e) == 0xFF && r.u8(e + 1) == 0xD9) break;
  }
  out->scan_off = (int32_t)at;
  out->scan_len = (int32_t)(e - at);
  return PPST_OK;
}
