// Host-only checks of the dealing's index arithmetic (megahit_amd/csrc/skm_deal.h; no GPU, no libmhx): skm_deal_at against the plain
// definition — the record whose run of windows holds window g, and g minus the run's start — over every chunk of many vectors of 64
// record lengths, and skm_win_rc against the reverse complement of the whole record, shifted, as the six-shuffle form computes it.
// Prints "ok" and exits 0, or a message and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "skm_deal.h"

using mhx::SkmDealAt;
using mhx::SkmDealCarry;

#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "skm_deal_check:%d: %s: ", __LINE__, #cond);    \
      fprintf(stderr, __VA_ARGS__);                                   \
      fprintf(stderr, "\n");                                          \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

constexpr int kLanes = 64, kChunks = 8;

// One trip of a wavefront with these record lengths (0 .. 8 each).  The kernel's records without windows come last, and then a record's
// rank among those with windows is its lane; the arithmetic itself is defined by the rank, so vectors with zeros anywhere are checked
// too, against the rank — and against the lane as well wherever the two agree by construction (lane_is_rank).
static void check_lengths(const int *len, const char *what) {
  int owner_rank[kLanes * 8], owner_lane[kLanes * 8], within[kLanes * 8];
  uint64_t heads[kChunks] = {0};
  int chunk_heads[kChunks] = {0}, chunk_last_head[kChunks] = {0};  // per chunk: its run heads, and where the last of them is
  int T = 0, rank = 0;
  bool lane_is_rank = true, seen_zero = false;
  for (int l = 0; l < kLanes; ++l) {
    CHECK(len[l] >= 0 && len[l] <= 8, "%s: lane %d", what, l);
    if (!len[l]) {
      seen_zero = true;
      continue;
    }
    if (seen_zero) lane_is_rank = false;
    heads[T >> 6] |= 1ull << (T & 63);  // (as the kernel sets it: at the record's start, records with windows only)
    ++chunk_heads[T >> 6];
    chunk_last_head[T >> 6] = T;
    for (int j = 0; j < len[l]; ++j, ++T) owner_rank[T] = rank, owner_lane[T] = l, within[T] = j;
    ++rank;
  }
  SkmDealCarry c;
  int last_head = -1;  // the plain carry: position of the last run head in the chunks before this one, and how many there were
  uint32_t heads_before = 0;
  for (int ch = 0; ch < kChunks; ++ch) {  // every chunk, in the kernel's order, those past T included (a group of four is taken whole)
    const SkmDealCarry before = c;
    if (ch * 64 < T) {  // (window 0 is a head whenever there is a window: from chunk 1 on the carry is defined)
      if (ch > 0) CHECK(before.gap == (uint32_t)(ch * 64 - 1 - last_head), "%s: chunk %d: gap %u, last head %d", what, ch, before.gap, last_head);
      CHECK(before.heads_m1 + 1u == heads_before, "%s: chunk %d: %u heads so far, want %u", what, ch, before.heads_m1 + 1u, heads_before);
    }
    const int n_lanes = ch * 64 < T ? kLanes : 1;  // (a chunk past the end: only its carry is looked at, by the chunks behind it)
    for (int lane = 0; lane < n_lanes; ++lane) {
      SkmDealCarry cl = before;  // (every lane advances its own copy, as on the GPU: all copies end up equal)
      const SkmDealAt d = skm_deal_at(heads[ch], (uint32_t)lane, cl);
      if (lane == 0) c = cl;
      CHECK(cl.heads_m1 == c.heads_m1 && cl.gap == c.gap, "%s: chunk %d lane %d: the carry differs between lanes", what, ch, lane);
      const int g = ch * 64 + lane;
      if (g >= T) continue;
      CHECK(d.o == (uint32_t)owner_rank[g] && d.j == (uint32_t)within[g], "%s: window %d of %d: (o, j) = (%u, %u), want (%d, %d)", what, g, T, d.o, d.j,
            owner_rank[g], within[g]);
      if (lane_is_rank) CHECK(d.o == (uint32_t)owner_lane[g], "%s: window %d: o = %u, lane %d", what, g, d.o, owner_lane[g]);
    }
    if (chunk_heads[ch]) last_head = chunk_last_head[ch];
    heads_before += (uint32_t)chunk_heads[ch];
  }
}

static int total(const int *len) {
  int t = 0;
  for (int l = 0; l < kLanes; ++l) t += len[l];
  return t;
}

static void edge_vectors() {
  int len[kLanes];
  for (int l = 0; l < kLanes; ++l) len[l] = 8;
  CHECK(total(len) == 512, "T");
  check_lengths(len, "all 8");
  for (int l = 0; l < kLanes; ++l) len[l] = 1;
  check_lengths(len, "all 1");
  for (int only = 0; only < kLanes; ++only)  // a single record, in every lane, of every length
    for (int n = 1; n <= 8; ++n) {
      memset(len, 0, sizeof len);
      len[only] = n;
      check_lengths(len, "a single record");
    }
  memset(len, 0, sizeof len);
  check_lengths(len, "no record");
  for (int z = 1; z < kLanes; ++z) {  // z lanes without a record: in front, at the end, scattered
    for (int l = 0; l < kLanes; ++l) len[l] = l < z ? 0 : 1 + (int)(rnd() % 8);
    check_lengths(len, "zeros in front");
    for (int l = 0; l < kLanes; ++l) len[l] = l >= kLanes - z ? 0 : 1 + (int)(rnd() % 8);
    check_lengths(len, "zeros at the end");
    for (int l = 0; l < kLanes; ++l) len[l] = 8;
    for (int l = kLanes - z; l < kLanes; ++l) len[l] = 0;
    check_lengths(len, "eights, zeros at the end");
    for (int l = 0; l < kLanes; ++l) len[l] = 1 + (int)(rnd() % 8);
    for (int q = 0; q < z; ++q) len[rnd() % kLanes] = 0;
    check_lengths(len, "zeros scattered");
  }
  // T = 255, 256, 257: the second group of four chunks does not run, does not run, runs for one window
  for (int T : {255, 256, 257})
    for (int rep = 0; rep < 200; ++rep) {
      for (int l = 0; l < kLanes; ++l) len[l] = 4;  // 256
      int t = 256;
      for (int q = 0; q < 400; ++q) {  // move windows between records, the sum unchanged
        const int a = (int)(rnd() % kLanes), b = (int)(rnd() % kLanes);
        if (len[a] > (rep & 1) && len[b] < 8) --len[a], ++len[b];  // (odd rep: down to empty records)
      }
      while (t != T) {
        const int a = (int)(rnd() % kLanes);
        if (t < T && len[a] < 8) ++len[a], ++t;
        if (t > T && len[a] > 1) --len[a], --t;
      }
      CHECK(total(len) == T, "T = %d", T);
      check_lengths(len, "T = 255 .. 257");
    }
  // runs that straddle every chunk boundary at every offset: records of 8 behind s windows of single-window records
  for (int s = 0; s < 8; ++s) {
    for (int l = 0; l < kLanes; ++l) len[l] = l < s ? 1 : 8;
    check_lengths(len, "eights behind ones");
  }
}

static void random_vectors(int n) {
  int len[kLanes];
  for (int it = 0; it < n; ++it) {
    const int mode = it & 3;  // uniform 0 .. 8; long records mostly (chunks without a head cannot occur, gaps of 7 do); short; uniform 1 .. 8
    for (int l = 0; l < kLanes; ++l) {
      const uint64_t x = rnd();
      len[l] = mode == 0 ? (int)(x % 9) : mode == 1 ? ((x & 7) ? 8 : (int)((x >> 3) % 9)) : mode == 2 ? (int)((x % 9) % 3) : 1 + (int)(x % 8);
    }
    check_lengths(len, "random");
  }
}

// the reverse complement of the n characters in the top 2n bits, one character at a time
static uint64_t plain_rc(uint64_t x, int n) {
  uint64_t r = 0;
  for (int i = 0; i < n; ++i) {
    const uint64_t ch = (x >> (62 - 2 * i)) & 3u;
    r |= (3u - ch) << (62 - 2 * (n - 1 - i));
  }
  return r;
}

static void reverse_complements() {
  for (int it = 0; it < 3000; ++it) {
    uint64_t rec = rnd();
    if (it < 4) rec = it == 0 ? 0ull : it == 1 ? ~0ull : it == 2 ? 0xAAAAAAAAAAAAAAAAull : 0x0123456789ABCDEFull;
    const uint64_t rec_r = plain_rc(rec, 32);
    CHECK(mhx::skm_rc32(rec) == rec_r, "rc32 of %016llx", (unsigned long long)rec);
    for (int k = 19; k <= 22; ++k) {
      const uint64_t kmask = ~0ull << (64 - 2 * (k - 1));
      for (int j = 0; j < 8; ++j) {
        const uint64_t want = (rec_r << (2 * (32 - k - j))) & kmask;  // what the six-shuffle form makes of the record's reverse complement
        const uint64_t win = rec << (2 * j);
        const uint64_t got = mhx::skm_win_rc(win, k, kmask);
        CHECK(got == want, "record %016llx k %d j %d: %016llx, want %016llx", (unsigned long long)rec, k, j, (unsigned long long)got, (unsigned long long)want);
        CHECK(got == plain_rc(win << 2, k - 1), "record %016llx k %d j %d: not the (k-1)-mer's reverse complement", (unsigned long long)rec, k, j);
      }
    }
  }
}

int main() {
  edge_vectors();
  random_vectors(100000);
  reverse_complements();
  printf("ok\n");
  return 0;
}
