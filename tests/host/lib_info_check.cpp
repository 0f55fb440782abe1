// Driver of tests/test_host_lib_info.py: mhxio::read_lib_info_libs on the file named by argv[1] (a library prefix);
// prints one line per library: start end max_len paired|description
#include <cstdio>

#include "formats.h"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  mhxio::g_fatal_throws = true;
  try {
    for (const mhxio::LibInfo &l : mhxio::read_lib_info_libs(argv[1]))
      printf("%lld %lld %u %d|%s\n", (long long)l.start, (long long)l.end, l.max_len, (int)l.paired, l.description.c_str());
  } catch (const mhxio::Fatal &) {
    return 1;
  }
  return 0;
}
