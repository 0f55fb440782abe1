// CPU check of the BGZF scan (bgzf_scan.h) and of the inflate core (inflate_core.h) on one lane: the decode logic the GPU kernel
// runs, on the fixture files tests/test_host_bgzf.py writes.  Built there with -fsanitize=address,undefined: every file and every
// text lies in a heap block of exactly its size, so a read or a store out of bounds ends the program.
//
// usage: bgzf_check <dir>; <dir>/cases.txt has one line per case: name status reason bad_block.  <dir>/<name>.gz is the file and,
// for status 0, <dir>/<name>.txt its text; reason 255 stands for any reason and block.  Prints "ok" when every case gives what its line says.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bgzf_scan.h"
#include "inflate_core.h"

struct Bytes {
  uint8_t *p = nullptr;
  size_t n = 0;
  ~Bytes() { free(p); }
};

static bool read_file(const std::string &path, Bytes *b) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  b->n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  b->p = static_cast<uint8_t *>(malloc(b->n ? b->n : 1));
  const bool ok = fread(b->p, 1, b->n, f) == b->n;
  fclose(f);
  return ok;
}

struct Outcome {
  int status = 0;
  uint32_t reason = 0;
  uint64_t bad_block = 0;
};

// what mhx_bgzf_inflate does, on one lane: scan, inflate every block, check every block's CRC
static Outcome inflate_file(const Bytes &gz, Bytes *text) {
  Outcome o;
  const mhx::BgzfScan scan = mhx::bgzf_scan(gz.p, gz.n);
  if (scan.reason) {
    o.status = 2;
    o.reason = scan.reason;
    o.bad_block = scan.bad_block;
    return o;
  }
  text->n = scan.n_text;
  text->p = static_cast<uint8_t *>(malloc(text->n ? text->n : 1));
  auto state = std::make_unique<mhx::InflateState>();
  for (size_t b = 0; b < scan.blocks.size(); ++b) {
    const mhx::BgzfBlock &bl = scan.blocks[b];
    // the payload in a block of its own: the bit reader's bounds are this block's, not the file's
    Bytes payload;
    payload.n = bl.in_size;
    payload.p = static_cast<uint8_t *>(malloc(payload.n ? payload.n : 1));
    memcpy(payload.p, gz.p + bl.in_off, bl.in_size);
    const uint32_t why = mhx::inflate_block(mhx::InflateOneLane{}, *state, payload.p, bl.in_size, text->p + bl.out_off, bl.isize);
    if (why) {
      o.status = 2;
      o.reason = why;
      o.bad_block = b;
      return o;
    }
  }
  uint32_t table[256], shift[64];
  for (uint32_t i = 0; i < 256; ++i) table[i] = mhx::crc_table_entry(i);
  mhx::crc_shift_table(shift);
  for (size_t b = 0; b < scan.blocks.size(); ++b) {
    const mhx::BgzfBlock &bl = scan.blocks[b];
    uint32_t x = 0;
    for (uint32_t l = 0; l < 64; ++l) x ^= mhx::crc_chunk_share(text->p + bl.out_off, bl.isize, l, table, shift);
    if (mhx::crc_finish(x, bl.isize) != bl.crc) {
      o.status = 2;
      o.reason = mhx::kInfCrc;
      o.bad_block = b;
      return o;
    }
  }
  return o;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE *cases = fopen((dir + "/cases.txt").c_str(), "r");
  if (!cases) return 2;
  char name[256];
  int status;
  unsigned reason;
  unsigned long long bad_block;
  int n_cases = 0, n_bad = 0;
  while (fscanf(cases, "%255s %d %u %llu", name, &status, &reason, &bad_block) == 4) {
    ++n_cases;
    Bytes gz, text, want;
    if (!read_file(dir + "/" + name + ".gz", &gz)) {
      fprintf(stderr, "%s: cannot read the file\n", name);
      ++n_bad;
      continue;
    }
    const Outcome o = inflate_file(gz, &text);
    // (reason 255: a mutated file, only zlib's verdict is known)
    if (o.status != status || (reason != 255 && (o.reason != reason || (status && o.bad_block != bad_block)))) {
      fprintf(stderr, "%s: status %d reason %u block %llu, expected %d %u %llu\n", name, o.status, o.reason, (unsigned long long)o.bad_block, status, reason,
              bad_block);
      ++n_bad;
      continue;
    }
    if (status == 0) {
      if (!read_file(dir + "/" + name + ".txt", &want) || want.n != text.n || memcmp(want.p, text.p, text.n) != 0) {
        fprintf(stderr, "%s: the text differs\n", name);
        ++n_bad;
      }
    }
  }
  fclose(cases);
  if (n_bad || !n_cases) return 1;
  printf("ok %d\n", n_cases);
  return 0;
}
