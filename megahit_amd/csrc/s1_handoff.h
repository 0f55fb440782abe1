// What stage 1 (read2sdbg_s1) leaves in the handle for stage 2 to take instead of computing it again: one record (mhx_ctx::s1),
// one way in (the publish calls at the end of stage 1), one way out (the queries, consume_items).  Plain C++: no HIP, no other header
// of the library (tests/host/s1_handoff_check.cpp drives it on the CPU).
//
// It speaks for four things, each for one (k, m):
//   items   ws "s2_agg_items" holds agg_n aggregated 8-byte stage-2 items (k <= 22, m >= 2; k = 23..27 in the compact
//           form where s1_agg_wide had the bucket streaming leave them), until a stage 2 sorts them where they lie
//   rows    ws "s2_pre_hist" holds the digit histograms of stage 2's sort passes (s2_agg_sort_passes(k), their count and
//           passes_signature()) over exactly those agg_n items, taken where stage 1 packed them; stage 2 adds its '$' items
//   bitmap  the is_solid bitmap is exactly what stage 1 found — no mercy edges added, not set by the caller, not a rank's share of
//           several GPUs': stage 2 may then take its solid items from a count of the (k+1)-mers instead of from every occurrence
//           (s2.hip s2_agg_from_count)
//   bound   what k_s2d_bound would count in that bitmap (two '$' items per run end), summed by the kernel that packed it
//
// Invariants, which hold by construction (the fields are private):
//   - the rows are never valid unless the items are;
//   - the bound is never valid unless the bitmap claim holds, for the same k;
//   - after drop() every query is false.
// Whatever changes the reads or the bitmap calls drop(); a missed call gives a wrong SdBG, not a crash — so there is one call to make.
#pragma once
#include <cstdint>
#include <deque>

namespace mhx {

class S1Handoff {
 public:
  // the item count: the asynchronous copy that ends stage 1 writes it (settled by the synchronisation stage 1 ends with); means something
  // only while the items are valid
  uint64_t agg_n = 0;

  // the reads or the bitmap changed
  void drop() {
    agg_valid = false;
    agg_hist_passes = 0;
    solid_plain_k = solid_plain_m = 0;
    s2_bound_k = 0;
  }

  // Stage 1 opens its items for (k, m); accumulate: a bucket-range pass after the first (passes.hip).  continues: the items of the
  // earlier passes stay in front (agg_n of them).  Items and rows are not valid again before publish_items.  in_flight: the counts that
  // were on their way to the device (count_home) — the caller synchronises before it lets go of them when there are any.
  struct Opened {
    bool continues = false;
    std::deque<uint64_t> in_flight;
  };
  Opened open_items(uint32_t k, uint32_t m, bool accumulate) {
    Opened o;
    o.continues = accumulate && items_for(k, m);
    agg_valid = false;
    agg_hist_passes = 0;
    o.in_flight.swap(agg_n_home);
    return o;
  }
  // the home of an item count on its way to the device cursor: an asynchronous copy reads it, and the handle outlives whatever call sent
  // it, also one that ends in an exception.  The address stays good until the next open_items
  const uint64_t *count_home(uint64_t n) {
    agg_n_home.push_back(n);
    return &agg_n_home.back();
  }

  // ---- the end of stage 1 ----
  // the items of (k, m) are complete (agg_n: see above); hist_passes rows over them with signature hist_sig, 0: none
  void publish_items(uint32_t k, uint32_t m, int hist_passes, uint64_t hist_sig) {
    agg_valid = true;
    agg_k = k;
    agg_m = m;
    agg_hist_passes = hist_passes > 0 ? hist_passes : 0;
    agg_hist_sig = hist_sig;
  }
  // stage 1 wrote the bitmap for (k, m); own: it is the whole of it (false on several GPUs).  A new bitmap: no bound yet
  void publish_bitmap(uint32_t k, uint32_t m, bool own) {
    solid_plain_k = own ? k : 0;
    solid_plain_m = own ? m : 0;
    s2_bound_k = 0;
  }
  // ... and the kernel that packed it counted its run ends (behind publish_bitmap; nothing to say about a bitmap that is not stage 1's)
  void publish_bound(uint32_t k, uint64_t bound) {
    if (!k || solid_plain_k != k) return;
    s2_bound = bound;
    s2_bound_k = k;
  }

  // ---- stage 2 ----
  bool has_items() const { return agg_valid; }
  bool items_for(uint32_t k, uint32_t m) const { return agg_valid && agg_k == k && agg_m == m; }
  uint32_t items_m() const { return agg_valid ? agg_m : 0; }  // the min count the items were made for
  bool hist_for(int passes, uint64_t sig) const { return agg_valid && passes > 0 && agg_hist_passes == passes && agg_hist_sig == sig; }
  bool bitmap_is_s1s(uint32_t k, uint32_t m) const { return k && solid_plain_k == k && solid_plain_m == m; }
  bool bound_for(uint32_t k, uint32_t m, uint64_t *bound) const {
    if (!bitmap_is_s1s(k, m) || s2_bound_k != k) return false;
    *bound = s2_bound;
    return true;
  }
  // a stage 2 sorts the items where they lie, and the rows count its '$' items from here on.  What is said of the bitmap stays: a second
  // stage 2 may still take s2_agg_from_count
  void consume_items() {
    agg_valid = false;
    agg_hist_passes = 0;
  }
  // the rows went with their workspace (mhx_trim): stage 2's sort takes its histograms itself
  void drop_hist() { agg_hist_passes = 0; }

 private:
  bool agg_valid = false;
  uint32_t agg_k = 0, agg_m = 0;
  int agg_hist_passes = 0;
  uint64_t agg_hist_sig = 0;
  std::deque<uint64_t> agg_n_home;
  uint32_t solid_plain_k = 0, solid_plain_m = 0;
  uint64_t s2_bound = 0;
  uint32_t s2_bound_k = 0;
};

}  // namespace mhx
