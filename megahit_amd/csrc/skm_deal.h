// The index arithmetic of the group-by's dealing (s1_skm.hip k_s1_skm, form s1_skm_deal = 2): which record a dealt window belongs to and
// where in it, from the wavefront's bitmap of run heads alone, and the window's reverse complement from the window itself — so that a
// window's lane fetches three words of its record (the 64 base bits, the position) and nothing derived from them.
// Plain C++, host and device: no HIP, no other header of the library (tests/host/skm_deal_check.cpp drives it on the CPU).
//
// A trip of the kernel gives every lane of a wavefront one record of 0 .. 8 windows (0: a lane past the end of the bin; those come
// last).  The windows of the 64 records, T <= 512, are numbered in record order; bit g of the bitmap is set when window g is the first
// of its record (a run head).  They are dealt in chunks of 64: window g = 64 c + lane goes to `lane` in chunk c.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MHX_SKM_HD __host__ __device__ inline
#else
#define MHX_SKM_HD inline
#endif

namespace mhx {

// what the chunks so far leave for the next one (the same in every lane: scalar registers)
struct SkmDealCarry {
  uint32_t heads_m1 = 0xFFFFFFFFu;  // run heads in the chunks so far, minus one
  uint32_t gap = 0;                 // windows behind the last run head so far, up to the end of its chunk
};
struct SkmDealAt {
  uint32_t o;  // the record: its rank among the records that have windows = its lane (the records without windows come last)
  uint32_t j;  // the window's index within the record's run
};

// window `lane` of the chunk whose word of the bitmap is w; advances the carry to the next chunk.  Chunks are taken in order, from 0.
// Means something for windows g < T only (a window past the end gets the last record and a j past its run).
MHX_SKM_HD SkmDealAt skm_deal_at(uint64_t w, uint32_t lane, SkmDealCarry &c) {
  const uint64_t at = w & ((2ull << lane) - 1ull);  // the run heads at or before this lane (lane 63: 2 << 63 is 0, the mask all ones)
  SkmDealAt d;
  d.o = c.heads_m1 + (uint32_t)__builtin_popcountll(at);
  // the run's head is the highest bit of `at`; without one the run came over from an earlier chunk
  d.j = at ? lane - 63u + (uint32_t)__builtin_clzll(at) : lane + 1u + c.gap;
  c.heads_m1 += (uint32_t)__builtin_popcountll(w);
  c.gap = w ? (uint32_t)__builtin_clzll(w) : c.gap + 64u;
  return d;
}

// reverse complement of the 32 characters of x (2 bits each, first character in the top bits)
MHX_SKM_HD uint64_t skm_rc32(uint64_t x) {
#if defined(__has_builtin) && __has_builtin(__builtin_bitreverse64)
  uint64_t r = __builtin_bitreverse64(x);  // (one instruction per word on the GPU)
  r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);  // the two bits of a character back in order
#else
  uint64_t r = __builtin_bswap64(x);  // the characters reversed: bytes, then the halves of a byte, then the pairs in them
  r = ((r >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((r & 0x0F0F0F0F0F0F0F0Full) << 4);
  r = ((r >> 2) & 0x3333333333333333ull) | ((r & 0x3333333333333333ull) << 2);
#endif
  return ~r;
}

// win: a record's 64 base bits shifted up by 2 j, so that the window's (k+1)-mer head.S.tail leads.  -> the reverse complement of its
// (k-1)-mer S in the top 2 (k - 1) bits (kmask), the rest 0: what (rc(record) << 2 (32 - k - j)) & kmask is.  The zeros that the shift
// by 2 j let in become 2 j one bits on top of rc(win); the shift by 2 (32 - k) drops them (j <= 7 < 32 - k: k <= 24).
MHX_SKM_HD uint64_t skm_win_rc(uint64_t win, int k, uint64_t kmask) { return (skm_rc32(win) << (2 * (32 - k))) & kmask; }

}  // namespace mhx
