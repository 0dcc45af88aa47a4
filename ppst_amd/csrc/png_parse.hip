// PNG decode on the device, the host half: ppst_png_parse walks a file's chunks and fills the descriptor and the span table the
// kernels of png_decode.hip read (include/ppst_hip.h "PNG decode on the device").  Plain C++ with no GPU call and no dependency
// but the header: tests/png_parse_san.cpp compiles this file as host code under the address and undefined-behaviour sanitizers.
// Every read goes through Rd (parse_reader.h, shared with jpeg_parse.hip), which knows n: no chunk length is trusted.  No CRC is computed and nothing is inflated here.
#include <string.h>
#include "../../include/ppst_hip.h"
#include "parse_reader.h"

namespace {
constexpr uint32_t tag(char a, char b, char c, char d) {
  return ((uint32_t)(unsigned char)a << 24) | ((uint32_t)(unsigned char)b << 16) | ((uint32_t)(unsigned char)c << 8) | (uint32_t)(unsigned char)d;
}
const unsigned char SIGNATURE[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
}  // namespace

extern "C" int ppst_png_parse(const void* file, int64_t n, ppst_png_dec_image* out, ppst_png_span* spans, int span_cap) {
  if (!out) return PPST_ENULL;
  memset(out, 0, sizeof(*out));
  if (n < 0 || span_cap < 0) return PPST_EINVAL;
  if (!file) return n == 0 ? PPST_PNG_E_TRUNCATED : PPST_ENULL;
  if (span_cap > 0 && !spans) return PPST_ENULL;
  if (n >= 0x10000000ll) return PPST_PNG_E_TOO_LARGE;                         // bit positions of the zlib stream stay below 2^31
  const Rd r = {(const unsigned char*)file, n};
  out->file_len = n;
  for (int k = 0; k < 8; ++k) {
    if (!r.has(k, 1)) return PPST_PNG_E_TRUNCATED;
    if (r.u8(k) != SIGNATURE[k]) return PPST_PNG_E_SIGNATURE;
  }
  int64_t at = 8;
  int count = 0, first_idat = -1, nidat = 0;
  int64_t idat_bytes = 0;
  bool have_iend = false, idat_closed = false;
  int rc = PPST_OK;
  while (!have_iend) {
    if (at == n) break;                                                       // the file ends between chunks: IEND is missing
    if (!r.has(at, 8)) return PPST_PNG_E_TRUNCATED;
    const uint32_t len = r.u32(at), type = r.u32(at + 4);
    if (len > 0x7FFFFFFFu || !r.has(at + 8, (int64_t)len + 4)) return PPST_PNG_E_TRUNCATED;
    const int64_t data = at + 8;
    if (count == 0) {
      if (type != tag('I', 'H', 'D', 'R') || len != 13) return PPST_PNG_E_IHDR;
      const uint32_t W = r.u32(data), H = r.u32(data + 4);
      const int depth = r.u8(data + 8), colour = r.u8(data + 9), comp = r.u8(data + 10), filt = r.u8(data + 11), lace = r.u8(data + 12);
      if (W == 0 || H == 0 || W > 0x7FFFFFFFu || H > 0x7FFFFFFFu) return PPST_PNG_E_SIZE;
      if (colour != 0 && colour != 2 && colour != 6) return PPST_PNG_E_COLOUR;
      if (depth != 8) return PPST_PNG_E_DEPTH;
      if (comp != 0 || filt != 0) return PPST_PNG_E_METHOD;
      if (lace != 0) return PPST_PNG_E_INTERLACE;
      const int C = colour == 0 ? 1 : (colour == 2 ? 3 : 4);
      // H (1 + W C) < 2^31, without overflow: W C < 2^34, H < 2^31
      const uint64_t row = 1u + (uint64_t)W * (uint64_t)C;
      if (row >= 0x80000000ull || (uint64_t)H * row >= 0x80000000ull) return PPST_PNG_E_TOO_LARGE;
      out->H = (int32_t)H; out->W = (int32_t)W; out->colour = colour; out->channels = C;
    } else if (type == tag('I', 'H', 'D', 'R')) {
      return PPST_PNG_E_IHDR;
    } else if (type == tag('a', 'c', 'T', 'L')) {
      return PPST_PNG_E_APNG;
    }
    const bool idat = type == tag('I', 'D', 'A', 'T');
    if (idat) {
      if (idat_closed) return PPST_PNG_E_IDAT;
      if (first_idat < 0) first_idat = count;
      ++nidat;
      idat_bytes += len;
    } else if (first_idat >= 0) {
      idat_closed = true;
    }
    if (type == tag('I', 'E', 'N', 'D')) have_iend = true;
    if (count < span_cap) {
      ppst_png_span* s = &spans[count];
      s->type = type; s->off = (int32_t)data; s->len = (int32_t)len; s->crc = r.u32(data + len); s->idat = idat ? 1 : 0;
    } else {
      rc = PPST_PNG_E_SPANS;
    }
    if (count == 0x7FFFFFFF) return PPST_PNG_E_TOO_LARGE;
    ++count;
    at = data + (int64_t)len + 4;
  }
  if (count == 0) return PPST_PNG_E_TRUNCATED;
  if (!have_iend) return first_idat < 0 ? PPST_PNG_E_IDAT : PPST_PNG_E_IEND;
  if (first_idat < 0) return PPST_PNG_E_IDAT;
  out->nspans = count;
  out->first_idat = first_idat;
  out->nidat = nidat;
  out->idat_bytes = (int32_t)idat_bytes;                                      // < n < 2^28
  return rc;
}
