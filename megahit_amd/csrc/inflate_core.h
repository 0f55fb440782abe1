// RFC 1951 inflate of one BGZF block (at most 64 KiB of text, an empty window at its start), written once for the GPU kernel
// (inflate.hip k_bgzf_inflate: the 64 lanes of one wavefront) and for one lane on the host (tests/host/bgzf_check.cpp): the bit reader,
// the code-length reader, the canonical-code tables, the symbol-to-token step, the window and every check.
// Plain C++, host and device: no HIP, no other header of the library.
//
// The symbol chain is serial: every lane of the wavefront runs it with the same values (the state below is the same in all lanes).
// What is dealt to the lanes, through the `Lanes` policy (lane(), kLanes, sync()): the tables' build, a match's copy, the stores.
// sync() orders the memory operations of the wavefront's lanes on the state (InflateState, in LDS on the GPU): one wavefront's LDS
// operations complete in issue order, so a wavefront-scope fence that keeps the compiler from moving them is all it has to be.
//
// The window is a ring of the last 32 KiB of text in the state; the text goes out to `out` in stretches of whole 4-byte words as the
// ring fills (flush), never later than 4 KiB + 258 bytes behind the decoder, so nothing unwritten is overwritten.
// Every access is bounded by construction: the bit reader returns zeros past `n_in` (and the token loop ends the block on it), ring
// indices are masked, table indices are masked or below the tables' sizes, and nothing is stored at or past out + isize.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MHX_INF_HD __host__ __device__ inline
#else
#define MHX_INF_HD inline
#endif

namespace mhx {

// reasons of the decoder (the values of enum mhx_bgzf_reason in include/mhx.h, behind the scan's in bgzf_scan.h)
enum : uint32_t {
  kInfOk = 0,
  kInfPayloadEnd = 8,       // the payload ended before the final block's end-of-block symbol
  kInfBtype = 9,            // BTYPE 3
  kInfStoredLen = 10,       // stored block: LEN != ~NLEN
  kInfCodeOver = 11,        // an over-subscribed set of code lengths
  kInfCodeIncomplete = 12,  // an incomplete set (other than the single code of length 1 zlib accepts for literal/length and distance)
  kInfBadSymbol = 13,       // a bit pattern no code has, literal/length 286 / 287, distance 30 / 31, a repeat with nothing to repeat or
                            // past the counts, no end-of-block code, HLIT > 286, HDIST > 30
  kInfDistFar = 14,         // a match that starts before the block's text
  kInfOutOver = 15,         // more text than ISIZE
  kInfOutShort = 16,        // the stream ended with less text than ISIZE
  kInfCrc = 17              // (k_bgzf_crc) the text's CRC32 is not the trailer's
};

constexpr uint32_t kInfWin = 32768;      // the ring
constexpr uint32_t kInfLitBits = 10;     // first-level table of the literal/length code
constexpr uint32_t kInfDistBits = 9;     // ... of the distance code (and of the code-length code, 7 bits used)
constexpr uint32_t kInfFlushAt = 4096;   // text kept back before a flush

// one canonical code: the first-level table answers codes of up to `bits` bits (entry = len << 9 | symbol, 0: longer or none); the
// overflow is the canonical walk over count / first / index / sorted (one more bit per step, lengths 1 .. 15)
struct InflateCode {
  uint16_t count[16];  // codes of each length
  uint16_t first[16];  // first code of each length
  uint16_t index[16];  // where that length's symbols start in `sorted`
};

struct InflateState {
  uint8_t ring[kInfWin];
  uint16_t lit_tab[1u << kInfLitBits];
  uint16_t dist_tab[1u << kInfDistBits];
  uint16_t lit_sorted[288];
  uint16_t dist_sorted[32];
  InflateCode lit, dist;
  uint8_t lens[288 + 32];  // code lengths: literal/length, then distance
  uint8_t cl_lens[32];     // code lengths of the code-length code (19 used)
};

// the host's policy: one lane
struct InflateOneLane {
  static constexpr uint32_t kLanes = 1;
  MHX_INF_HD uint32_t lane() const { return 0; }
  MHX_INF_HD void sync() const {}
};

// ---- bits ------------------------------------------------------------------------------------------------------------------------
struct InflateBits {
  const uint8_t *p;
  uint32_t n;        // payload bytes
  uint32_t pos = 0;  // bytes taken into buf (may pass n: zeros)
  uint32_t cnt = 0;  // bits in buf
  uint64_t buf = 0;
  MHX_INF_HD InflateBits(const uint8_t *p_, uint32_t n_) : p(p_), n(n_) {}
  // at least 56 bits in buf
  MHX_INF_HD void refill() {
    if (pos + 8 <= n) {
      uint64_t w;
      memcpy(&w, p + pos, 8);
      buf |= w << cnt;
      pos += (63 - cnt) >> 3;
      cnt |= 56;
    } else {
      while (cnt <= 56) {
        const uint64_t b = pos < n ? p[pos] : 0;
        buf |= b << cnt;
        ++pos;
        cnt += 8;
      }
    }
  }
  MHX_INF_HD uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }
  MHX_INF_HD void drop(uint32_t k) {
    buf >>= k;
    cnt -= k;
  }
  MHX_INF_HD uint32_t take(uint32_t k) {
    const uint32_t v = peek(k);
    drop(k);
    return v;
  }
  // bits consumed so far lie past the payload's end
  MHX_INF_HD bool overrun() const { return (uint64_t)pos * 8 - cnt > (uint64_t)n * 8; }
  MHX_INF_HD uint32_t byte_pos() const { return (uint32_t)(((uint64_t)pos * 8 - cnt) >> 3); }
};

MHX_INF_HD uint32_t inflate_rev(uint32_t code, uint32_t len) {  // the low `len` bits of code, reversed
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// ---- tables ----------------------------------------------------------------------------------------------------------------------
// lens[0 .. n) -> the code c, its first-level table tab (2^bits entries) and sorted symbols.  single_ok: an incomplete set that is one
// code of length 1 is accepted (its other bit pattern has no symbol).  A set without any code is accepted under single_ok too (every
// pattern is without a symbol).  -> kInfOk, kInfCodeOver or kInfCodeIncomplete, the same in every lane.
template <class Lanes>
MHX_INF_HD uint32_t inflate_build(const Lanes &L, const uint8_t *lens, uint32_t n, InflateCode &c, uint16_t *tab, uint32_t bits, uint16_t *sorted,
                                  bool single_ok) {
  const uint32_t lane = L.lane();
  L.sync();  // the lengths are written
  for (uint32_t len = lane; len < 16; len += Lanes::kLanes) {
    uint32_t k = 0;
    for (uint32_t s = 0; s < n; ++s) k += lens[s] == len;
    c.count[len] = (uint16_t)k;
  }
  for (uint32_t e = lane; e < (1u << bits); e += Lanes::kLanes) tab[e] = 0;
  L.sync();
  int32_t left = 1;
  uint32_t code = 0, idx = 0, max_len = 0;
  bool over = false;
  for (uint32_t len = 1; len < 16; ++len) {
    const uint32_t k = c.count[len];
    if (len % Lanes::kLanes == lane) {  // (one lane per length; the host's one lane takes them all)
      c.first[len] = (uint16_t)code;
      c.index[len] = (uint16_t)idx;
    }
    left = (left << 1) - (int32_t)k;
    if (left < 0) over = true;
    if (over) left = 0;  // (keeps the shifts small; the answer is fixed already)
    if (k) max_len = len;
    code = (code + k) << 1;
    idx += k;
  }
  if (over) return kInfCodeOver;
  if (left > 0 && !(single_ok && max_len <= 1)) return kInfCodeIncomplete;
  L.sync();
  for (uint32_t s = lane; s < n; s += Lanes::kLanes) {
    const uint32_t len = lens[s];
    if (!len) continue;
    uint32_t r = 0;
    for (uint32_t t = 0; t < s; ++t) r += lens[t] == len;
    sorted[c.index[len] + r] = (uint16_t)s;  // index[len] + r < the number of coded symbols <= n
    if (len <= bits) {
      const uint32_t rv = inflate_rev(c.first[len] + r, len);  // < 2^len: the set is not over-subscribed
      const uint16_t e = (uint16_t)(len << 9 | s);
      for (uint32_t x = rv; x < (1u << bits); x += 1u << len) tab[x] = e;
    }
  }
  L.sync();
  return kInfOk;
}

// the next symbol of code c (at least 15 bits are in the reader): -> symbol, or -1 when the bits are no code's
MHX_INF_HD int32_t inflate_symbol(InflateBits &br, const InflateCode &c, const uint16_t *tab, uint32_t bits, const uint16_t *sorted) {
  const uint32_t e = tab[br.peek(bits)];
  if (e) {
    br.drop(e >> 9);
    return (int32_t)(e & 511u);
  }
  uint32_t code = 0;
  const uint32_t v = br.peek(15);
  for (uint32_t len = 1; len < 16; ++len) {
    code |= (v >> (len - 1)) & 1u;
    const uint32_t k = c.count[len], f = c.first[len];
    if (code >= f && code - f < k) {
      br.drop(len);
      return sorted[c.index[len] + (code - f)];
    }
    code <<= 1;
  }
  return -1;
}

// ---- the text --------------------------------------------------------------------------------------------------------------------
struct InflateOut {
  uint8_t *out;
  uint32_t isize;
  uint32_t pos = 0;      // text bytes decoded (in the ring)
  uint32_t flushed = 0;  // text bytes written to out: a multiple of 4 until the last flush
};

// ring [flushed, upto) -> out; upto <= pos <= isize
template <class Lanes>
MHX_INF_HD void inflate_flush(const Lanes &L, const InflateState &S, InflateOut &o, uint32_t upto, bool last) {
  L.sync();
  const uint32_t words = (upto - o.flushed) >> 2;
  for (uint32_t w = L.lane(); w < words; w += Lanes::kLanes) {
    const uint32_t at = o.flushed + 4 * w;  // a multiple of 4: the ring does not wrap inside the word
    memcpy(o.out + at, S.ring + (at & (kInfWin - 1)), 4);
  }
  uint32_t done = o.flushed + 4 * words;
  if (last) {
    for (uint32_t at = done + L.lane(); at < upto; at += Lanes::kLanes) o.out[at] = S.ring[at & (kInfWin - 1)];
    done = upto;
  }
  o.flushed = done;
}

// ---- one block -------------------------------------------------------------------------------------------------------------------
// in[0 .. n_in): the DEFLATE payload; out[0 .. isize): the text.  -> kInfOk or the reason; the same in every lane.
template <class Lanes>
MHX_INF_HD uint32_t inflate_block(const Lanes &L, InflateState &S, const uint8_t *in, uint32_t n_in, uint8_t *out, uint32_t isize) {
  constexpr uint32_t kMask = kInfWin - 1;
  const uint32_t lane = L.lane();
  InflateBits br(in, n_in);
  InflateOut o{out, isize};
  // base values and extra bits of the length codes 257 .. 285 and the distance codes 0 .. 29 (RFC 1951 3.2.5), computed not stored
  auto len_base = [](uint32_t c, uint32_t *extra) -> uint32_t {  // c = symbol - 257, 0 .. 28
    if (c < 8) return *extra = 0, 3 + c;
    if (c == 28) return *extra = 0, 258;
    const uint32_t e = (c >> 2) - 1;
    *extra = e;
    return 3 + ((4 + (c & 3)) << e);
  };
  auto dist_base = [](uint32_t c, uint32_t *extra) -> uint32_t {  // c = 0 .. 29
    if (c < 4) return *extra = 0, 1 + c;
    const uint32_t e = (c >> 1) - 1;
    *extra = e;
    return 1 + ((2 + (c & 1)) << e);
  };
  // the order in which the code-length code's own lengths are stored (RFC 1951 3.2.7)
  const uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (bool final_block = false; !final_block;) {
    br.refill();
    final_block = br.take(1) != 0;
    const uint32_t btype = br.take(2);
    if (br.overrun()) return kInfPayloadEnd;
    if (btype == 3) return kInfBtype;
    if (btype == 0) {
      // stored: to the next byte, LEN, NLEN, LEN bytes
      br.drop(br.cnt & 7);
      br.refill();
      const uint32_t len = br.take(16), nlen = br.take(16);
      if (br.overrun()) return kInfPayloadEnd;
      if ((len ^ 0xFFFFu) != nlen) return kInfStoredLen;
      const uint8_t *src = br.p + br.byte_pos();  // (no overrun: at or before the payload's end)
      const uint32_t rest = br.n - br.byte_pos();
      if (len > rest) return kInfPayloadEnd;
      if (len > isize - o.pos) return kInfOutOver;
      for (uint32_t done = 0; done < len;) {
        const uint32_t m = len - done < kInfFlushAt ? len - done : kInfFlushAt;
        L.sync();
        for (uint32_t i = lane; i < m; i += Lanes::kLanes) S.ring[(o.pos + i) & kMask] = src[done + i];
        o.pos += m;
        done += m;
        if (o.pos - o.flushed >= kInfFlushAt) inflate_flush(L, S, o, o.pos, false);
      }
      br = InflateBits(src + len, rest - len);
      continue;
    }
    if (btype == 1) {
      for (uint32_t s = lane; s < 288 + 32; s += Lanes::kLanes) S.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
      uint32_t why = inflate_build(L, S.lens, 288, S.lit, S.lit_tab, kInfLitBits, S.lit_sorted, true);
      if (!why) why = inflate_build(L, S.lens + 288, 32, S.dist, S.dist_tab, kInfDistBits, S.dist_sorted, true);
      if (why) return why;
    } else {
      const uint32_t hlit = 257 + br.take(5), hdist = 1 + br.take(5), hclen = 4 + br.take(4);
      if (br.overrun()) return kInfPayloadEnd;
      if (hlit > 286 || hdist > 30) return kInfBadSymbol;
      L.sync();
      for (uint32_t s = lane; s < 32; s += Lanes::kLanes) S.cl_lens[s] = 0;
      L.sync();
      for (uint32_t i = 0; i < hclen; ++i) {
        br.refill();
        const uint32_t v = br.take(3);
        if (lane == 0) S.cl_lens[kOrder[i]] = (uint8_t)v;
      }
      if (br.overrun()) return kInfPayloadEnd;
      // the code-length code borrows the distance code's tables
      uint32_t why = inflate_build(L, S.cl_lens, 19, S.dist, S.dist_tab, 7, S.dist_sorted, false);
      if (why) return why;
      const uint32_t total = hlit + hdist;
      uint32_t have = 0, prev = 0;
      while (have < total) {
        br.refill();
        const int32_t sym = inflate_symbol(br, S.dist, S.dist_tab, 7, S.dist_sorted);
        if (sym < 0) return br.overrun() ? kInfPayloadEnd : kInfBadSymbol;
        uint32_t rep = 1, val = (uint32_t)sym;
        if (sym == 16) {
          if (!have) return kInfBadSymbol;
          val = prev;
          rep = 3 + br.take(2);
        } else if (sym == 17) {
          val = 0;
          rep = 3 + br.take(3);
        } else if (sym == 18) {
          val = 0;
          rep = 11 + br.take(7);
        }
        if (br.overrun()) return kInfPayloadEnd;
        if (rep > total - have) return kInfBadSymbol;
        // the two counts are one sequence (a repeat may cross from the literal/length lengths into the distance lengths)
        for (uint32_t i = lane; i < rep; i += Lanes::kLanes) {
          const uint32_t at = have + i;
          S.lens[at < hlit ? at : 288 + (at - hlit)] = (uint8_t)val;
        }
        have += rep;
        prev = val;
      }
      for (uint32_t s = hlit + lane; s < 288; s += Lanes::kLanes) S.lens[s] = 0;
      for (uint32_t s = hdist + lane; s < 32; s += Lanes::kLanes) S.lens[288 + s] = 0;
      L.sync();
      if (S.lens[256] == 0) return kInfBadSymbol;  // no end-of-block code
      why = inflate_build(L, S.lens, 288, S.lit, S.lit_tab, kInfLitBits, S.lit_sorted, true);
      if (!why) why = inflate_build(L, S.lens + 288, 32, S.dist, S.dist_tab, kInfDistBits, S.dist_sorted, true);
      if (why) return why;
    }
    // the tokens
    for (;;) {
      br.refill();  // 56 bits: a length code (15 + 5) and a distance code (15 + 13) fit
      const int32_t sym = inflate_symbol(br, S.lit, S.lit_tab, kInfLitBits, S.lit_sorted);
      if (br.overrun()) return kInfPayloadEnd;
      if (sym < 0) return kInfBadSymbol;
      if (sym < 256) {
        if (o.pos >= isize) return kInfOutOver;
        if (lane == 0) S.ring[o.pos & kMask] = (uint8_t)sym;
        ++o.pos;
      } else if (sym == 256) {
        break;
      } else {
        if (sym > 285) return kInfBadSymbol;
        uint32_t xb;
        uint32_t len = len_base((uint32_t)sym - 257, &xb);
        len += br.take(xb);
        const int32_t ds = inflate_symbol(br, S.dist, S.dist_tab, kInfDistBits, S.dist_sorted);
        if (ds < 0 || ds > 29) return br.overrun() ? kInfPayloadEnd : kInfBadSymbol;
        uint32_t dist = dist_base((uint32_t)ds, &xb);
        dist += br.take(xb);
        if (br.overrun()) return kInfPayloadEnd;
        if (dist > o.pos) return kInfDistFar;
        if (len > isize - o.pos) return kInfOutOver;
        // byte i of the match is text[pos - dist + i mod dist]: all of them were decoded before this token, so the lanes read and then
        // write without looking at one another (dist <= 32768 and pos - flushed <= 4096 + 258 keep source and target in the ring)
        L.sync();
        const uint32_t from = o.pos - dist;
        if (dist >= len) {
          for (uint32_t i = lane; i < len; i += Lanes::kLanes) S.ring[(o.pos + i) & kMask] = S.ring[(from + i) & kMask];
        } else if (dist == 1) {
          const uint8_t b = S.ring[from & kMask];
          for (uint32_t i = lane; i < len; i += Lanes::kLanes) S.ring[(o.pos + i) & kMask] = b;
        } else {
          for (uint32_t i = lane; i < len; i += Lanes::kLanes) S.ring[(o.pos + i) & kMask] = S.ring[(from + i % dist) & kMask];
        }
        o.pos += len;
      }
      if (o.pos - o.flushed >= kInfFlushAt) inflate_flush(L, S, o, o.pos, false);
    }
  }
  if (o.pos != isize) return kInfOutShort;
  inflate_flush(L, S, o, o.pos, true);
  return kInfOk;
}

// ---- CRC32 (the gzip polynomial, reflected) ---------------------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcChunk = 1024;  // bytes per lane of k_bgzf_crc: 64 chunks cover a block

MHX_INF_HD uint32_t crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}
// a * b mod P, both in the reflected form (bit 31 is x^0)
MHX_INF_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = b & 1 ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// shift[l] = x^(8 * kCrcChunk * (63 - l)) mod P: what the raw CRC of chunk l is multiplied by, with 63 - l chunks behind it
inline void crc_shift_table(uint32_t shift[64]) {
  uint32_t x = 1u << 31;
  for (uint32_t i = 0; i < 8 * kCrcChunk; ++i) x = x & 1 ? (x >> 1) ^ kCrcPoly : x >> 1;
  shift[63] = 1u << 31;
  for (int l = 62; l >= 0; --l) shift[l] = crc_mulmod(shift[l + 1], x);
}
// The standard CRC32 of text[0 .. n) from the raw CRCs (initial value 0, no final inversion) of chunks aligned from the END of the text,
// chunk l = [n - (64 - l) * kCrcChunk, n - (63 - l) * kCrcChunk) cut at 0.  The initial inversion is folded in by inverting the text's
// first four bytes (a text of n < 4 bytes: its n bytes, and the rest of the inversion, shifted past them, is added at the end).
// table: the 256 byte entries.  -> chunk l's share; the XOR over l = 0 .. 63, then crc_finish, is the CRC.
MHX_INF_HD uint32_t crc_chunk_share(const uint8_t *text, uint32_t n, uint32_t l, const uint32_t *table, const uint32_t *shift) {
  const uint32_t behind = (63 - l) * kCrcChunk;
  if (behind >= n) return 0;
  const uint32_t end = n - behind, begin = end > kCrcChunk ? end - kCrcChunk : 0;
  uint32_t c = 0;
  for (uint32_t i = begin; i < end; ++i) {
    const uint32_t b = text[i] ^ (i < 4 ? 0xFFu : 0u);
    c = table[(c ^ b) & 0xFFu] ^ (c >> 8);
  }
  return crc_mulmod(c, shift[l]);
}
MHX_INF_HD uint32_t crc_finish(uint32_t x, uint32_t n) { return x ^ (n < 4 ? 0xFFFFFFFFu >> (8 * n) : 0u) ^ 0xFFFFFFFFu; }

}  // namespace mhx
