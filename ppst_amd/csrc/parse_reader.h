// The reader of the two host-side parsers (jpeg_parse.hip, png_parse.hip): a file's bytes and their count.  Host code only, no
// dependency: every read of a parser goes through Rd, which knows n, so that no length field of the file is trusted.
#pragma once
#include <stdint.h>

namespace {
struct Rd {
  const unsigned char* p;
  int64_t n;
  bool has(int64_t at, int64_t len) const { return at >= 0 && len >= 0 && at <= n && len <= n - at; }
  int u8(int64_t at) const { return p[at]; }                                  // callers check has() first
  int u16(int64_t at) const { return (p[at] << 8) | p[at + 1]; }              // big-endian
  uint32_t u32(int64_t at) const {
    return ((uint32_t)p[at] << 24) | ((uint32_t)p[at + 1] << 16) | ((uint32_t)p[at + 2] << 8) | (uint32_t)p[at + 3];
  }
};
}  // namespace
