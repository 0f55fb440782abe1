// BGZF (the blocked gzip of bgzip / htslib): the walk over a file's members that finds, without inflating anything, where every block's
// DEFLATE payload lies, how many bytes it inflates to, its CRC32 and where its text goes (inflate.hip inflates the blocks, one per
// wavefront).  Plain C++, host only: no HIP, no other header of the library (tests/host/bgzf_check.cpp drives it on the CPU).
//
// A member is: 1f 8b 08 FLG=04 MTIME[4] XFL OS XLEN[2] | XLEN bytes of subfields (SI1 SI2 SLEN[2] data), one of them 'B' 'C' 2 BSIZE[2],
// BSIZE = the member's size - 1 | the payload, BSIZE + 1 - XLEN - 20 bytes | CRC32[4] ISIZE[4].  All numbers little endian.
#pragma once
#include <cstdint>
#include <vector>

namespace mhx {

// reasons of the scan (the values of enum mhx_bgzf_reason in include/mhx.h; inflate.hip asserts that they agree)
enum : uint32_t {
  kBgzfOk = 0,
  kBgzfNotGzip = 1,     // a member does not begin 1f 8b 08
  kBgzfFlg = 2,         // FLG is not exactly 4 (FEXTRA alone): plain gzip, or a name / comment / header CRC
  kBgzfNoBc = 3,        // no 'B','C' subfield of length 2 among the extra subfields (or subfields that overrun XLEN)
  kBgzfShortBlock = 4,  // BSIZE + 1 is less than 26 or than the header, the subfields and the trailer
  kBgzfPastEof = 5,     // the header's subfields or the block run past the end of the file
  kBgzfTrailing = 6,    // bytes behind the last member that cannot hold a member's fixed header
  kBgzfIsize = 7        // ISIZE above 65536
};

struct BgzfBlock {      // 32 bytes, the device's view too
  uint64_t in_off;      // the payload's offset in the file
  uint64_t out_off;     // where the block's text starts: the sum of ISIZE over the blocks before it
  uint32_t in_size;     // payload bytes
  uint32_t isize;       // text bytes
  uint32_t crc;         // CRC32 of the text
  uint32_t pad;
};

struct BgzfScan {
  uint32_t reason = kBgzfOk;  // kBgzfOk: BGZF throughout
  uint64_t bad_block = 0;     // the member the reason is about
  uint64_t n_text = 0;
  std::vector<BgzfBlock> blocks;
};

inline uint32_t bgzf_le16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t bgzf_le32(const unsigned char *p) { return bgzf_le16(p) | (bgzf_le16(p + 2) << 16); }

// O(blocks); reads 12 + XLEN + 8 bytes of every member
inline BgzfScan bgzf_scan(const void *file, uint64_t n) {
  const unsigned char *f = static_cast<const unsigned char *>(file);
  BgzfScan s;
  uint64_t o = 0;
  auto fail = [&](uint32_t why) {
    s.reason = why;
    s.bad_block = s.blocks.size();
    s.blocks.clear();
    s.n_text = 0;
    return s;
  };
  while (o < n) {
    const uint64_t rem = n - o;
    const unsigned char *h = f + o;
    if (rem < 12) return fail(kBgzfTrailing);
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return fail(kBgzfNotGzip);
    if (h[3] != 4) return fail(kBgzfFlg);
    const uint32_t xlen = bgzf_le16(h + 10);
    if (12ull + xlen > rem) return fail(kBgzfPastEof);
    uint32_t total = 0;  // BSIZE + 1
    for (uint32_t x = 0; x + 4 <= xlen;) {
      const unsigned char *sf = h + 12 + x;
      const uint32_t slen = bgzf_le16(sf + 2);
      if (x + 4 + slen > xlen) break;
      if (sf[0] == 'B' && sf[1] == 'C' && slen == 2) {
        total = bgzf_le16(sf + 4) + 1;
        break;
      }
      x += 4 + slen;
    }
    if (!total) return fail(kBgzfNoBc);
    if (total < 26 || total < 12 + xlen + 8) return fail(kBgzfShortBlock);
    if (total > rem) return fail(kBgzfPastEof);
    BgzfBlock b;
    b.in_off = o + 12 + xlen;
    b.in_size = total - xlen - 20;
    b.crc = bgzf_le32(h + total - 8);
    b.isize = bgzf_le32(h + total - 4);
    b.out_off = s.n_text;
    b.pad = 0;
    if (b.isize > 65536) return fail(kBgzfIsize);
    s.blocks.push_back(b);
    s.n_text += b.isize;
    o += total;
  }
  return s;
}

}  // namespace mhx
