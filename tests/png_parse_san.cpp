// Stand-alone sanitizer program for the host PNG parser (ppst_amd/csrc/png_parse.hip): not a test pytest collects, not loaded
// into python, host code that needs no GPU.  Build both files as HOST code under the sanitizers and feed it the robustness
// corpus (every prefix of a file, corrupted chunk data with and without the CRCs recomputed, one file per refusal) that
// tests/png_decode_cases.dump_corpus writes:
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import png_decode_cases as P; P.dump_corpus('/tmp/png_corpus')"
//   clang++ -x c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       ppst_amd/csrc/png_parse.hip tests/png_parse_san.cpp -o /tmp/png_parse_san
//   /tmp/png_parse_san /tmp/png_corpus
//
// Every file is copied into a heap block of EXACTLY its length, so one byte read past n is a heap-buffer-overflow report, and
// the span array is a heap block of exactly the capacity stated: first 2 entries (the parser must ask for more), then what it asks.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../include/ppst_hip.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <directory of files>\n", argv[0]);
    return 2;
  }
  DIR* dir = opendir(argv[1]);
  if (!dir) {
    perror(argv[1]);
    return 2;
  }
  std::vector<std::string> names;
  while (dirent* e = readdir(dir))
    if (e->d_name[0] != '.') names.push_back(std::string(argv[1]) + "/" + e->d_name);
  closedir(dir);
  std::map<int, int> by_code;
  long files = 0;
  for (const std::string& name : names) {
    FILE* f = fopen(name.c_str(), "rb");
    if (!f) {
      perror(name.c_str());
      return 2;
    }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char* buf = (unsigned char*)malloc(n > 0 ? (size_t)n : 1);      // (n = 0: a block the parser must not touch)
    if (n > 0 && fread(buf, 1, (size_t)n, f) != (size_t)n) {
      perror(name.c_str());
      return 2;
    }
    fclose(f);
    ppst_png_dec_image d;
    int cap = 2;
    ppst_png_span* spans = (ppst_png_span*)malloc(sizeof(ppst_png_span) * cap);
    int rc = ppst_png_parse(n > 0 ? buf : nullptr, n, &d, spans, cap);
    if (rc == PPST_PNG_E_SPANS) {
      if (d.nspans <= cap) {
        fprintf(stderr, "%s: asks for %d spans, had %d\n", name.c_str(), d.nspans, cap);
        return 1;
      }
      cap = d.nspans;
      free(spans);
      spans = (ppst_png_span*)malloc(sizeof(ppst_png_span) * cap);
      rc = ppst_png_parse(buf, n, &d, spans, cap);
      if (rc != PPST_OK) {
        fprintf(stderr, "%s: the second call returned %d\n", name.c_str(), rc);
        return 1;
      }
    }
    if (rc == PPST_OK) {
      bool ok = d.H >= 1 && d.W >= 1 && d.nspans >= 1 && d.nspans <= cap && d.nidat >= 1 && d.first_idat >= 0 &&
                d.first_idat + d.nidat <= d.nspans && d.file_len == n;
      long idat = 0;
      for (int k = 0; ok && k < d.nspans; ++k) {
        const ppst_png_span& s = spans[k];
        ok = s.off >= 16 && s.len >= 0 && (long)s.off + s.len + 4 <= n;
        ok = ok && (s.idat != 0) == (k >= d.first_idat && k < d.first_idat + d.nidat);
        if (s.idat) idat += s.len;
      }
      if (!ok || idat != d.idat_bytes) {
        fprintf(stderr, "%s: accepted with a span outside the file or a wrong count\n", name.c_str());
        return 1;
      }
    } else if (rc > PPST_PNG_E_SIGNATURE || rc < PPST_PNG_E_METHOD) {
      fprintf(stderr, "%s: unexpected return code %d\n", name.c_str(), rc);
      return 1;
    }
    ++by_code[rc];
    ++files;
    free(spans);
    free(buf);
  }
  printf("%ld files:", files);
  for (const auto& kv : by_code) printf("  code %d x %d", kv.first, kv.second);
  printf("\n");
  return 0;
}
