// Stand-alone sanitizer program for the host JPEG parser (ppst_amd/csrc/jpeg_parse.hip): not a test pytest collects, not loaded
// into python, host code that needs no GPU.  Build both files as HOST code under the sanitizers and feed it the truncated and
// corrupted files that tests/jpeg_decode_cases.dump_damaged writes:
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import jpeg_decode_cases as D; D.dump_damaged('/tmp/jpeg_damaged')"
//   clang++ -x c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       ppst_amd/csrc/jpeg_parse.hip tests/jpeg_parse_san.cpp -o /tmp/jpeg_parse_san
//   /tmp/jpeg_parse_san /tmp/jpeg_damaged
//
// Every file is copied into a heap block of EXACTLY its length, so one byte read past n is a heap-buffer-overflow report.
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
    ppst_jpeg_dec_image d;
    const int rc = ppst_jpeg_parse(n > 0 ? buf : nullptr, n, &d);
    if (rc == PPST_OK) {
      if (d.scan_off < 0 || d.scan_len < 0 || (long)d.scan_off + d.scan_len + 2 > n || d.H < 1 || d.W < 1) {
        fprintf(stderr, "%s: accepted with a scan outside the file\n", name.c_str());
        return 1;
      }
    } else if (rc > PPST_JPEG_E_TRUNCATED || rc < PPST_JPEG_E_SCAN) {
      fprintf(stderr, "%s: unexpected return code %d\n", name.c_str(), rc);
      return 1;
    }
    ++by_code[rc];
    ++files;
    free(buf);
  }
  printf("%ld files:", files);
  for (const auto& kv : by_code) printf("  code %d x %d", kv.first, kv.second);
  printf("\n");
  return 0;
}
