// Host-only checks of the record stage 1 leaves for stage 2 (megahit_amd/csrc/s1_handoff.h; no GPU, no libmhx): the record is driven
// through the sequences the library goes through, and every query is asked after each step.
// Prints "ok" and exits 0, or a message and exits 1.
#include <cstdio>
#include <cstdlib>

#include "s1_handoff.h"

using mhx::S1Handoff;

static const uint64_t kSig = 0x5157ull, kOtherSig = 0x5158ull;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "s1_handoff_check:%d: %s\n", __LINE__, #cond);         \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static bool bound_is(const S1Handoff &h, uint32_t k, uint32_t m, uint64_t want) {
  uint64_t b = ~0ull;
  return h.bound_for(k, m, &b) && b == want;
}
static bool no_bound(const S1Handoff &h, uint32_t k, uint32_t m) {
  uint64_t b = 77;
  return !h.bound_for(k, m, &b) && b == 77;  // (nothing written when there is none)
}
// the end of a stage 1 on one GPU: items with `passes` histogram rows, its own bitmap, the bound
static void stage1(S1Handoff &h, uint32_t k, uint32_t m, int passes, uint64_t sig, uint64_t n, uint64_t bound) {
  h.open_items(k, m, false);
  h.agg_n = n;
  h.publish_items(k, m, passes, sig);
  h.publish_bitmap(k, m, true);
  h.publish_bound(k, bound);
}
// no query answers, for any of the (k, m) and signatures the checks use
static void nothing_answers(const S1Handoff &h) {
  CHECK(!h.has_items() && h.items_m() == 0);
  for (uint32_t k : {0u, 19u, 21u, 22u})
    for (uint32_t m : {0u, 1u, 2u, 3u}) {
      CHECK(!h.items_for(k, m) && !h.bitmap_is_s1s(k, m) && no_bound(h, k, m));
    }
  for (int p : {0, 5, 6})
    for (uint64_t s : {(uint64_t)0, kSig, kOtherSig}) CHECK(!h.hist_for(p, s));
}

int main() {
  {  // a new handle
    S1Handoff h;
    nothing_answers(h);
    h.drop();
    nothing_answers(h);
  }
  {  // published at (21, 2) with 6 histogram passes and a bound
    S1Handoff h;
    stage1(h, 21, 2, 6, kSig, 1000, 40);
    CHECK(h.has_items() && h.items_for(21, 2) && h.items_m() == 2 && h.agg_n == 1000);
    CHECK(h.bitmap_is_s1s(21, 2) && bound_is(h, 21, 2, 40) && h.hist_for(6, kSig));
    CHECK(!h.items_for(22, 2) && !h.bitmap_is_s1s(22, 2) && no_bound(h, 22, 2));
    CHECK(!h.items_for(21, 3) && !h.bitmap_is_s1s(21, 3) && no_bound(h, 21, 3));
    CHECK(!h.hist_for(6, kOtherSig) && !h.hist_for(5, kSig) && !h.hist_for(0, kSig) && !h.hist_for(0, 0));
    // stage 2 sorts the items where they lie: items and rows are gone, what is said of the bitmap stays
    h.consume_items();
    CHECK(!h.has_items() && !h.items_for(21, 2) && !h.hist_for(6, kSig) && !h.hist_for(0, 0));
    CHECK(h.bitmap_is_s1s(21, 2) && bound_is(h, 21, 2, 40));
    h.drop();
    nothing_answers(h);
  }
  {  // (19, 2), then (21, 2): nothing of the first answers
    S1Handoff h;
    stage1(h, 19, 2, 5, kOtherSig, 900, 30);
    stage1(h, 21, 2, 6, kSig, 1000, 40);
    CHECK(!h.items_for(19, 2) && !h.bitmap_is_s1s(19, 2) && no_bound(h, 19, 2) && !h.hist_for(5, kOtherSig));
    CHECK(h.items_for(21, 2) && h.bitmap_is_s1s(21, 2) && bound_is(h, 21, 2, 40) && h.hist_for(6, kSig));
    // ... and a stage 1 whose pack kernel counted no run ends (another marking polarity) says nothing of the earlier bound
    h.open_items(21, 2, false);
    h.publish_items(21, 2, 0, 0);
    h.publish_bitmap(21, 2, true);
    CHECK(h.items_for(21, 2) && h.bitmap_is_s1s(21, 2) && no_bound(h, 21, 2) && !h.hist_for(6, kSig) && !h.hist_for(0, 0));
    h.drop();
    nothing_answers(h);
  }
  {  // a pass that continues the items of an earlier one (accumulate)
    S1Handoff h;
    stage1(h, 21, 2, 6, kSig, 1000, 40);
    CHECK(h.open_items(21, 2, true).continues);
    CHECK(!h.has_items() && !h.hist_for(6, kSig) && h.agg_n == 1000);  // (the count of the earlier passes is still there to be read)
    CHECK(!h.open_items(21, 2, true).continues);                      // (nothing was published in between)
    stage1(h, 21, 2, 6, kSig, 1000, 40);
    CHECK(!h.open_items(21, 2, false).continues);
    const uint32_t other[2][2] = {{22, 2}, {21, 3}};
    for (const auto &km : other) {
      stage1(h, 21, 2, 6, kSig, 1000, 40);
      CHECK(!h.open_items(km[0], km[1], true).continues);
      CHECK(!h.has_items() && !h.hist_for(6, kSig));
    }
    h.drop();
    nothing_answers(h);
  }
  {  // several GPUs: the bitmap is not stage 1's own, and nothing is said of a bound
    S1Handoff h;
    stage1(h, 21, 2, 6, kSig, 1000, 40);
    h.open_items(21, 2, false);
    h.publish_items(21, 2, 0, 0);
    h.publish_bitmap(21, 2, false);
    h.publish_bound(21, 40);
    CHECK(h.items_for(21, 2) && !h.bitmap_is_s1s(21, 2) && no_bound(h, 21, 2));
    // the bound of another k than the bitmap's does not stand either
    h.publish_bitmap(21, 2, true);
    h.publish_bound(22, 40);
    CHECK(h.bitmap_is_s1s(21, 2) && no_bound(h, 21, 2) && no_bound(h, 22, 2));
    h.drop();
    nothing_answers(h);
  }
  {  // the histograms' rows went with their workspace: the items stay
    S1Handoff h;
    stage1(h, 21, 2, 6, kSig, 1000, 40);
    h.drop_hist();
    CHECK(h.items_for(21, 2) && !h.hist_for(6, kSig) && h.bitmap_is_s1s(21, 2) && bound_is(h, 21, 2, 40));
    h.drop();
    nothing_answers(h);
    CHECK(h.agg_n == 1000);  // (drop leaves the count alone: nothing asks for it)
  }
  {  // the home of a count on its way to the device
    S1Handoff h;
    const uint64_t *first = h.count_home(11);
    const uint64_t *p[64];
    for (int i = 0; i < 64; ++i) p[i] = h.count_home(100 + i);
    CHECK(*first == 11);
    for (int i = 0; i < 64; ++i) {
      CHECK(*p[i] == 100u + i && p[i] != first);
      for (int j = 0; j < i; ++j) CHECK(p[i] != p[j]);
    }
    {
      const S1Handoff::Opened o = h.open_items(21, 2, false);
      CHECK(o.in_flight.size() == 65 && &o.in_flight.front() == first && *first == 11);  // (alive while the caller synchronises)
    }
    CHECK(h.open_items(21, 2, false).in_flight.empty());
    CHECK(*h.count_home(5) == 5 && h.open_items(21, 2, true).in_flight.size() == 1);
  }
  printf("ok\n");
  return 0;
}
