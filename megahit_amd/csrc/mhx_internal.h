// Internal host-side declarations of libmhx (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mhx.h"
#include "mhx_options.h"
#include "s1_handoff.h"

using mhx::Opt;

namespace mhx {

struct OnesweepLaunch;
void set_error(const char *fmt, ...);

struct Error : std::runtime_error {
  explicit Error(const std::string &s) : std::runtime_error(s) {}
};

#define MHX_HIP(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      char buf_[512];                                                                          \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
               __LINE__);                                                                      \
      throw mhx::Error(buf_);                                                                  \
    }                                                                                          \
  } while (0)

// A grow-only device allocation that is kept between engine calls.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;   // bytes allocated
  size_t used = 0;  // bytes holding valid data (for result buffers)
  void reserve(size_t bytes);
  void release();
  template <class T>
  T *as() const { return reinterpret_cast<T *>(p); }
};

struct KernelStat {
  uint32_t launches = 0;
  double ms = 0, bytes = 0;
};

struct PendingEvent {
  const char *name;
  hipEvent_t a, b;
  double bytes;
};

// device-resident packed sequence set
struct SeqSet {
  DevBuf words;      // uint32, padded with >= 32 zero words
  DevBuf start;      // uint64[n_seqs+1] (always materialised on device)
  DevBuf mult;       // uint16[n_seqs]
  uint64_t n_seqs = 0, n_bases = 0, n_words = 0;
  uint32_t fixed_len = 0, max_len = 0;
  std::vector<uint64_t> h_start;  // host copy when variable length (small path helpers)
};

}  // namespace mhx

struct mhx_ctx {
  int device = 0;
  int n_cus = 0;  // compute units of the device (0: unknown)
  hipStream_t stream = nullptr;
  mhx::SeqSet seqs;
  std::map<int, mhx::DevBuf> results;      // keyed by enum mhx_buffer
  std::map<std::string, mhx::DevBuf> work; // named scratch workspaces
  uint32_t sorted_item_words = 0;
  // multi-GPU: lv1-bucket partition and this rank's place in the global read set
  int my_part = 0, n_parts = 1;
  std::vector<uint32_t> part_begin;
  uint64_t pos_base = 0, global_bases = 0;
  mhx::S1Handoff s1;  // what stage 1 left for stage 2: aggregated items, their histograms, its claim on the bitmap, the '$' items' bound (s1_handoff.h)
  uint64_t n_route = 0;      // multi-GPU: records in ws("route_records") (count events)
  uint32_t filter_kept = 0;           // lv1 buckets the filter keeps
  // stage 1: records per lv1 bucket the ranks of a multi-GPU run agreed on (comm.hip; 0: each call derives it from its own
  // item count, s1.hip s1_density) — every rank must make the same sort plan
  double s1_density = 0;
  // several GPUs: this stage 1 runs inside mhx_dist_read2sdbg, which makes the ranks agree on whether all of them hold the compact aggregated
  // items of k = 23..27 (s1_agg_wide) before stage 2 exchanges anything.  A caller that drives the building blocks itself
  // (mhx_dist_process_s1, mhx_dist_extract, its own exchange, mhx_dist_process_s2) has no such agreement: no such items there
  bool s1_agg_wide_agreed = false;
  std::string last_s1_plan;           // what the last stage 1 ran as (mhx_last_s1_plan; bench.py prints it)
  // memory-bounded passes (passes.hip): only items of the kept lv1 buckets are materialised
  bool filter_on = false, accumulate = false;
  uint64_t filter_expected = 0, filter_batch_bytes = 0;
  bool global_marks_inverted = false;  // multi-GPU stage 1 marked the non-solid occurrences (s1.hip)
  uint64_t s1_acc_bits = 0, mercy_acc_n = 0;  // stage-1 state that accumulate continues
  uint32_t s1_acc_k = 0, s1_acc_m = 0;
  uint32_t count_acc_k = 0, count_acc_m = 0;  // (k, m) of the count state that accumulate continues
  uint64_t n_marks = 0;          // multi-GPU, sparse marks: positions in ws("s1_marks") waiting to be routed
  uint64_t dist_local_solid = 0; // multi-GPU, sparse marks: solid occurrences in the local reads after the marks arrived
  bool dist_s2_agg = false;  // the items of the current multi-GPU stage-2 exchange are aggregated ones
  // the unitig graph mhx_sdbg_unitigs left in MHX_BUF_UNITIG_VERTICES (sdbg_unitig.hip) and the cleaning steps change
  // (unitig_clean.hip): valid until the SdBG or its index is replaced.  ut_owner: ws "uc_owner" maps every edge to its vertex
  bool ut_ready = false, ut_owner = false;
  uint64_t ut_edges = 0, ut_nv = 0;
  // MHX_BUF_UNITIG_SEQ / _OFFSET describe the vertex table as it is now (no Refresh ran since they were written)
  bool ut_text_fresh = false;
  uint64_t ub_stats[4] = {0, 0, 0, 0};  // the last mhx_unitig_pop_bubbles: candidates, pairs passed, pairs failed, mid-run finishes
  // `local`, first half (local_map.hip): the contigs and seed table of mhx_local_index live in workspaces "lm_*" (lm_ready: they are
  // there); lm_mapped: MHX_BUF_LOCAL_REC holds the records of lm_n_reads loaded reads against that index
  bool lm_ready = false, lm_mapped = false;
  uint64_t lm_n_ctg = 0, lm_cap = 0, lm_n_reads = 0;
  uint32_t lm_seed = 0;
  // tuning knobs (mhx_set_option): explicit value, else environment MHX_<NAME>, else the default.  mhx_options.h declares every
  // knob with its default and holds the rule (DESIGN.md "Tuning knobs"; include/mhx.h describes them)
  std::map<std::string, long long> options;
  // tuned defaults of this installation: `name = value` lines of mhx_tuning.conf beside libmhx.so (MHX_TUNING_FILE names
  // another file, MHX_NO_TUNING=1 ignores it), read at mhx_create; consulted after explicit options and the environment
  std::map<std::string, long long> tuned;
  template <mhx::Opt O>
  long long opt() const { return mhx::resolve_option<O>(options, tuned); }
  template <mhx::Opt O>
  long long opt(long long fallback) const { return mhx::resolve_option<O>(options, tuned, fallback); }  // derived knobs
  long long opt(const char *name, long long dflt) const { return mhx::resolve_option(options, tuned, name, dflt); }  // mhx_get_option only
  // pinned staging buffers of upload_pinned (capi.hip)
  void *pinned[2] = {nullptr, nullptr};
  hipEvent_t pinned_free[2] = {nullptr, nullptr};
  // profiling
  bool profiling = false;
  std::vector<mhx::PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
  // side streams for kernels that run next to each other (kmsort_emu.hip) and the events that fork / join them
  std::vector<hipStream_t> side_streams;
  std::vector<hipEvent_t> side_events;
  std::map<std::string, mhx::KernelStat> stats;

  mhx::DevBuf &ws(const char *name, size_t bytes) {
    mhx::DevBuf &b = work[name];
    b.reserve(bytes);
    return b;
  }
  mhx::DevBuf &result(int which, size_t bytes) {
    mhx::DevBuf &b = results[which];
    b.reserve(bytes);
    b.used = bytes;
    return b;
  }
  void prof_begin(const char *name, double bytes);
  void prof_end();
  void prof_collect();
};

// Launch wrapper: records a HIP-event pair around the launch when profiling is on.
#define MHX_LAUNCH(ctx, name, bytes, ...) \
  do {                                    \
    (ctx)->prof_begin(name, bytes);       \
    __VA_ARGS__;                          \
    MHX_HIP(hipGetLastError());           \
    (ctx)->prof_end();                    \
  } while (0)

namespace mhx {

// ---- sort.hip ----
struct SortPass {
  int shift;       // bit offset from the LSB of the big-endian key (key_words*32 bits)
  int bits;        // digit = bits [shift, shift+bits) ...
  int shift2 = 0;  // ... optionally continued by bits [shift2, shift2+bits2) as its upper part
  int bits2 = 0;   // bits + bits2 <= 8
  // >= 0: the earlier passes of the plan sorted bits [prev_lo, shift), and the consumer does not look at the order of records
  // that agree on every bit the plan sorts — lets the pass rank with LDS atomics where that cannot matter (sort_kernels.h RANK 2)
  int prev_lo = -1;
};
// What an extraction prepared for the very next sort of the records it stands for.  It travels by value from the extraction
// to that sort; the sort that receives it empties it, one that is never handed it cannot meet it.
struct SortPrep {
  const void *buf = nullptr;  // the sort buffer it was made for
  uint64_t n = 0;             // records the sort handles (what a generated first pass leaves)
  // digit histograms of the sort's passes, taken by the extraction kernel (ws "sort_pre_hist"); hist_passes == 0: none
  int hist_passes = 0;
  uint64_t hist_sig = 0;  // passes_signature() of the plan they were taken for
  const unsigned long long *hist = nullptr;  // where their rows lie when not in ws "sort_pre_hist" (device, [hist_passes][256])
  // first sort pass whose records are generated instead of loaded (sort_kernels.h OnesweepLaunch): the buffer holds NO items yet
  std::function<void(const OnesweepLaunch &)> gen;
  uint64_t gen_slots = 0;  // item slots it walks (> n when it drops the items of filtered-out lv1 buckets)
  bool gen_var = false;    // ... padded to the longest read's count: reads of several lengths (S1GenVarT; the plan text says so)
  // first sort pass over an array SPLIT by the digit before the plan's first (sort_kernels.h SrcSplit; 16-byte records): the buffer holds
  // 256 ranges of split_range_cap slots, range d filled with split_fill[d] (device, [256]) records; n is their sum; range d is read by
  // the units [split_ubase[d], split_ubase[d + 1]) (device, [257]: ceil(fill / kSortSplitUnit) units each), split_units in all.  The histograms
  // of the plan's passes then start at row hist_first of "sort_pre_hist" (the rows before it belong to the digits the extraction split by)
  const unsigned long long *split_fill = nullptr, *split_ubase = nullptr;
  uint64_t split_range_cap = 0, split_units = 0;
  int hist_first = 0;
};
// Sorts n items of `stride` uint32 words held in buf_a (ping-pong with buf_b) by the digit passes
// (least-significant pass first).  Returns the buffer holding the result.  prep: what the extraction of exactly these
// records left for this sort (consumed).
uint32_t *radix_sort(mhx_ctx *c, uint32_t *buf_a, uint32_t *buf_b, uint64_t n, int stride, int key_words,
                     const std::vector<SortPass> &passes, SortPrep *prep = nullptr);
// prefix passes + segment finish in LDS when that saves passes (sort.hip); same result as radix_sort with `passes`
uint32_t *sort_whole_key(mhx_ctx *c, uint32_t *buf_a, uint32_t *buf_b, uint64_t n, int stride, int key_words,
                         const std::vector<SortPass> &passes, SortPrep *prep = nullptr);
std::vector<SortPass> make_passes(int key_words, int lo_bit, int hi_bit);
bool sort_takes_generated_first_pass(const mhx_ctx *c, uint64_t n, int stride, const std::vector<SortPass> &passes);
// true when radix_sort(stride 4, these passes) will read a split array in its first pass (SortPrep::split_fill)
bool sort_takes_split_first_pass(const mhx_ctx *c, const std::vector<SortPass> &passes);
constexpr uint64_t kSortSplitUnit = 4096;  // records of a unit of that pass (256 threads x 8 x 2): what split_range_cap is a multiple of
uint64_t passes_signature(const std::vector<SortPass> &ps);
// kmsort_emu.hip: sort with the reference's exact (unstable) tie order, one GPU thread per lv1 bucket
uint32_t *kmsort_exact(mhx_ctx *c, uint32_t *buf_a, uint32_t *buf_b, uint64_t n, int S, int key_words, SortPrep *prep = nullptr);

// ---- scan.hip ----
// exclusive scan of n uint32 values into uint64 (in != out); returns total via d_total (device, uint64[1])
void exclusive_scan_u32_u64(mhx_ctx *c, const uint32_t *in, uint64_t *out, uint64_t n, uint64_t *d_total);
void exclusive_scan_u64(mhx_ctx *c, const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *d_total);
// positions i in [0,n) where item i differs from item i-1 in the first `cmp_bits` bits of the key
// (big-endian words), written ascending to heads[]; *d_count receives their number.
void find_group_heads(mhx_ctx *c, const uint32_t *items, uint64_t n, int stride, int cmp_bits,
                      uint64_t *heads, uint64_t *d_count);
uint64_t count_group_heads(mhx_ctx *c, const uint32_t *items, uint64_t n, int stride, int cmp_bits);

struct DigitSpec;
DigitSpec spec_of_pass(const SortPass &ps, int key_words);
std::vector<SortPass> make_passes_ranges(int key_words, const std::vector<std::pair<int, int>> &ranges);
// s2.hip: SdBG records from sorted lv2 items (shared by read2sdbg S2 and seq2sdbg)
void emit_sdbg(mhx_ctx *c, const uint32_t *sorted, uint64_t n_items, int S, int kw, uint32_t k, int is_seq, mhx_sdbg_result *out, int compact_bits = 0);

void partition_by_owner(mhx_ctx *c, const uint32_t *a, uint32_t *b, uint64_t n, int stride, const uint8_t *lut, int n_parts,
                        uint64_t *counts);
uint64_t s1_extract(mhx_ctx *c, uint32_t k, bool compact, SortPrep *prep, bool defer_items = false, bool filter_in_gen = false);
bool s1_compact(const mhx_ctx *c, uint32_t k, int want_mercy);
bool s1_rank_tagged(const mhx_ctx *c, uint32_t k);
int s1_stride(uint32_t k, bool compact);
// stage-1 records pre-sorted by lv1 bucket, in n arrays (multi-GPU: one per sending rank; comm.hip)
struct S1Sources {
  int n = 0;
  std::vector<const uint32_t *> ptr;
  std::vector<uint64_t> count;
  uint32_t *spare = nullptr;  // scratch of >= 12 bytes per record for the group-by's output regions
  int pbits = 16;             // key prefix bits the sources are sorted on (the stream plan's seg_bits)
};
// ---- stage 1 on super-k-mer records (s1_skm.hip) ----
constexpr int kSkmBatch = 8;   // bins per ticket of the group-by
constexpr int kSkmSrcMax = 8;  // sources of the group-by: one array on a single GPU, one per sending rank on several
struct SkmFront {
  int n_src;
  const uint4 *src[kSkmSrcMax];            // the records, ordered by minimizer bin
  const uint64_t *src_bounds[kSkmSrcMax];  // [n_bins + 1] each: where the bins start in the source
  uint32_t *spare;       // the other sort buffer (the workgroups' output regions)
  uint64_t spare_bytes;
  uint64_t n_records, n_windows;
  uint64_t n_items;        // what the reference sorts: L - k + 4 items per read that holds an edge
  uint32_t n_bins, max_bin;
  uint32_t bin_lo, bin_hi;  // the bins of this pass / of this owner
  int bin_bits;
  unsigned long long *hp;   // the homopolymer windows counted beside the records (stage 1, one GPU: [0..1] counts, [2..3] a position each; count: [8..]), else nullptr
  bool rep;                 // s1_skm_rep: the windows of period <= 4 were counted beside the records too, in the table behind hp (s1_skm.hip kSkmRepAt)
  // s1_skm_giant (one GPU; skm_giant.h): the bins of more than giant_limit records leave the batches and are worked in slices — giants[i] =
  // (bin, sub0 << 16 | rj0), n_giant_items of them on the device, the largest bins first; 0 items: no such bin, or the option is off
  const uint2 *giants;
  uint32_t n_giant_items, giant_limit;
  uint32_t giant_bins, giant_largest;  // for the plan line: giant bins of this pass, the records of the largest
  const char *why;                     // the front returned false for a reason of the option's (cap, work budget, list), else nullptr
};
bool s1_skm_applies(const mhx_ctx *c, uint32_t k, uint32_t m, int want_mercy);
bool s1_skm_dist_applies(const mhx_ctx *c, uint32_t k, uint32_t m);
int s1_skm_passes(const mhx_ctx *c, uint32_t k);
// (bins_whole: no bin is cut into slices, whatever s1_skm_giant says — min count 3 and 4)
bool s1_skm_front(mhx_ctx *c, uint32_t k, SkmFront *f, int pass, int n_passes, int bin_bits_agreed = 0, bool for_count = false, bool bins_whole = false);
uint32_t s1_skm_max_m(const mhx_ctx *c);  // s1_skm_max_m: the largest min count served on super-k-mer records on one GPU (2 .. 4)
// min count 3 and 4: a key counted beside the records (a homopolymer; s1_skm_rep: of period <= 4) keeps ONE position — one of 1 < count < m
// windows cannot be marked.  -> that count, 0: none (asked behind pass 0's front, before anything is published)
uint64_t s1_skm_beside_below(mhx_ctx *c, const SkmFront &f, uint32_t k, uint32_t m);
void s1_skm_bounds_of(mhx_ctx *c, const uint4 *recs, uint64_t n, uint32_t n_bins, uint64_t *bounds);
void s1_skm_groups_launch(mhx_ctx *c, bool agg, unsigned grid, const SkmFront &f, uint32_t k, uint32_t m, uint8_t *solid_bytes, unsigned long long *hist,
                          uint2 *agg_raw, uint32_t agg_cap, uint32_t *agg_counts, uint32_t *err, unsigned long long *marks_raw, uint32_t marks_cap,
                          uint32_t *marks_counts);
struct DigitSpecs;
// (agg_hist: the digit histograms of agg_specs that the items are added to, or nullptr)
void s1_skm_hp_publish(mhx_ctx *c, const SkmFront &f, uint32_t k, uint32_t m, uint8_t *solid_bytes, unsigned long long *hist, uint2 *agg_items,
                       uint64_t *agg_cursor, bool agg, const DigitSpecs *agg_specs = nullptr, unsigned long long *agg_hist = nullptr);
// (s1_skm_rep: the keys of the windows of period <= 4; -> how many windows were counted beside the records)
uint64_t s1_skm_rep_publish(mhx_ctx *c, const SkmFront &f, uint32_t k, uint32_t m, uint8_t *solid_bytes, unsigned long long *hist, uint2 *agg_items,
                            uint64_t *agg_cursor, bool agg, const DigitSpecs *agg_specs = nullptr, unsigned long long *agg_hist = nullptr);
// the owner's half on several GPUs (s1.hip): group-by over the received sources, marks as a list, aggregated items.  -> false: a region overflowed
bool s1_skm_owner(mhx_ctx *c, uint32_t k, uint32_t m, const SkmFront &f, mhx_s1_result *out);

bool s1_presort_applies(const mhx_ctx *c, uint32_t k, uint64_t n_local_items);
uint32_t *s1_presort(mhx_ctx *c, uint32_t k, uint32_t *buf_a, uint32_t *buf_b, uint64_t n_items, int *pbits, SortPrep *prep);
bool s1_filter_in_gen_applies(const mhx_ctx *c, uint32_t k);
bool s1_bucket_histogram_fast(mhx_ctx *c, uint32_t k, unsigned long long *hist);
uint32_t s1_pos_bits(const mhx_ctx *c);
uint64_t s1_pos_stride(const mhx_ctx *c, uint32_t k);
std::string s1_plan_text(const mhx_ctx *c, uint32_t k, uint64_t n_items);
int s1_process(mhx_ctx *c, uint32_t k, uint32_t m, int want_mercy, uint32_t *buf_a, uint32_t *buf_b, uint64_t n_items, mhx_s1_result *out,
               const S1Sources *pre = nullptr, SortPrep *prep = nullptr, bool var_gen = false);
__global__ void k_add_u64(unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b, int n);
void sdbg_accumulate(mhx_ctx *c, bool first);
void sdbg_publish_accumulated(mhx_ctx *c);
uint64_t s2_extract(mhx_ctx *c, uint32_t k, uint32_t m, bool filter_in_extract = false);
int s2_process(mhx_ctx *c, uint32_t k, uint32_t *buf_a, uint32_t *buf_b, uint64_t n_items, mhx_sdbg_result *out);
bool s2_use_aggregated(const mhx_ctx *c, uint32_t k, uint32_t m);
uint64_t s2_agg_extract(mhx_ctx *c, uint32_t k);
int s2_agg_process(mhx_ctx *c, uint32_t k, uint32_t *buf_a, uint32_t *buf_b, uint64_t n_items, mhx_sdbg_result *out, SortPrep *prep = nullptr);
// the sort passes of aggregated stage-2 items: flag | W above the count_bits count bits, then the chars of the k-mer
std::vector<SortPass> s2_agg_sort_passes(uint32_t k, int count_bits);  // count_bits: s2_agg_count_bits(k)
struct StageItems {
  uint64_t n;      // items in ws("items_a")
  int S;           // words per item
  bool agg;        // stage 2: aggregated items (s2.hip)
  bool batchable;  // produced by a scan over reads
  SortPrep prep;   // for the sort of exactly these items (empty: nothing prepared)
};
StageItems extract_stage(mhx_ctx *c, int stage, uint32_t k, uint32_t m, bool s1_defer_items = false);
void bucket_histogram(mhx_ctx *c, int stage, uint32_t k, uint32_t m, uint64_t *h_out);
int s2_stride(uint32_t k);
constexpr int MHX_BUF_IS_SOLID_LOCAL = 100;  // internal: this rank's slice of the global bitmap (multi-GPU)
constexpr int MHX_BUF_MERCY_CAND_LOCAL = 101;  // internal: routed mercy candidates of the local reads, local positions
uint64_t count_extract(mhx_ctx *c, uint32_t k, uint32_t m, SortPrep *prep);
int count_stride(uint32_t k);
int count_process(mhx_ctx *c, uint32_t k, uint32_t m, uint32_t *buf_a, uint32_t *buf_b, uint64_t n_items, mhx_count_result *out, SortPrep *prep = nullptr);
void count_apply_events(mhx_ctx *c, const unsigned long long *ev, uint64_t n);
uint64_t seq2sdbg_extract(mhx_ctx *c, uint32_t k);
int seq2sdbg_stride(uint32_t k);
int seq2sdbg_process(mhx_ctx *c, uint32_t k, uint32_t *buf_a, uint32_t *buf_b, uint64_t n_items, mhx_sdbg_result *out);
const uint64_t *sort_u64(mhx_ctx *c, const void *src, uint64_t n, int hi_bit);
void invert_local_marks(mhx_ctx *c, unsigned long long *words, uint64_t n_words);
DevBuf &grow_preserving(mhx_ctx *c, DevBuf &b, size_t bytes, size_t keep);
void stash_route_records(mhx_ctx *c, const void *src, uint64_t n, int hi_bit);
void mercy_adopt_routed(mhx_ctx *c, const long long *recv, uint64_t n);
void s1_apply_marks(mhx_ctx *c, const unsigned long long *recv, uint64_t n);
int sdbg_build_index(mhx_ctx *c, uint32_t k, mhx_sdbg_index_info *out);
int sdbg_remove_tips(mhx_ctx *c, const mhx_sdbg_index_info *info, int max_tip_len, uint64_t *n_removed);
int sdbg_mul_histogram(mhx_ctx *c, const mhx_sdbg_index_info *info, uint64_t *n_valid, std::vector<uint64_t> *host = nullptr);
int infer_min_depth(const uint64_t *hist, double *min_depth, int *converged);
int sdbg_unitigs(mhx_ctx *c, const mhx_sdbg_index_info *info, mhx_unitig_result *out);
int sdbg_unitig_text(mhx_ctx *c, const mhx_sdbg_index_info *info, uint64_t nv, uint64_t n_loop, mhx_unitig_result *out);
int unitig_disconnect_weak_links(mhx_ctx *c, const mhx_sdbg_index_info *info, double ratio, uint64_t *n_flagged);
int unitig_remove_tips(mhx_ctx *c, const mhx_sdbg_index_info *info, uint32_t max_tip_len, uint64_t *n_removed);
int unitig_remove_local_low_depth(mhx_ctx *c, const mhx_sdbg_index_info *info, double min_depth, uint32_t max_len, uint32_t local_width,
                                  double local_ratio, int mark_changed, uint64_t *n_removed, int *is_changed);
int unitig_iterate_local_low_depth(mhx_ctx *c, const mhx_sdbg_index_info *info, double min_depth, uint32_t max_len, uint32_t local_width,
                                   double local_ratio, int mark_changed, uint64_t *n_removed);
int unitig_finish(mhx_ctx *c, const mhx_sdbg_index_info *info, mhx_unitig_result *out);
int unitig_remove_low_depth(mhx_ctx *c, const mhx_sdbg_index_info *info, double min_depth, uint64_t *n_removed);
int unitig_pop_bubbles(mhx_ctx *c, const mhx_sdbg_index_info *info, uint32_t max_len, double similarity, double careful_threshold, int mark_changed,
                       uint64_t *n_removed, uint64_t *n_records);
int unitig_similarity(mhx_ctx *c, const char *a, uint32_t n, const char *b, uint32_t m, double sim, double *out);
int iterate_edges(mhx_ctx *c, uint32_t k, uint32_t step, const uint32_t *ctg_words, uint64_t ctg_n_words, uint64_t n_ctg, const uint64_t *ctg_start,
                  mhx_iterate_result *out);
int local_index(mhx_ctx *c, const uint32_t *ctg_words, uint64_t ctg_n_words, uint64_t n_ctg, const uint64_t *ctg_start, uint32_t seed,
                uint32_t sparsity, uint64_t *index_size);
int local_map(mhx_ctx *c, int32_t min_mapping_len, double similarity, uint64_t *n_valid);
int local_collect(mhx_ctx *c, uint32_t n_libs, const uint64_t *lib_begin, const uint64_t *lib_end, const int32_t *lib_paired,
                  const int32_t *lib_local_range, uint64_t *n_mapped, uint64_t *n_added);
int local_insert_size(const mhx_local_record *rec, const uint32_t *read_len, uint64_t lib_begin, uint64_t lib_end, uint32_t max_read_len,
                      int paired, double *mean, double *sd, int32_t *local_range);
int fastx_to_records(mhx_ctx *c, const char *text1, uint64_t n1, const char *text2, uint64_t n2, mhx_fastx_result *out);
// the same for texts that lie on the device (n bytes and 64 more that may be read); edge: a text's first, last and last but one byte
int fastx_device_to_records(mhx_ctx *c, const char *d_text1, uint64_t n1, const char edge1[3], const char *d_text2, uint64_t n2, const char edge2[3],
                            bool paired, mhx_fastx_result *out);
// ---- inflate.hip ----
void bgzf_inflate(mhx_ctx *c, const void *gz, uint64_t n, mhx_bgzf_result *out);
void fastx_bgzf_to_records(mhx_ctx *c, const void *gz1, uint64_t n1, const void *gz2, uint64_t n2, mhx_fastx_result *out);
int sdbg_load_bytes(mhx_ctx *c, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *off, const uint64_t *items, const uint64_t *tips,
                    const uint64_t *large);

// ---- engines ----
int run_count(mhx_ctx *c, uint32_t k, uint32_t m, mhx_count_result *out);
// count on the bucket streaming of stage 1 (s1.hip: CountGenT, k_s1_stream<COUNT>)
int s2_agg_compact_bits(uint32_t k);
inline int s2_agg_count_bits(uint32_t k) {  // the count field of an aggregated item of this k: 16 bits up to k = 22, the compact form's beyond
  const int cb = s2_agg_compact_bits(k);
  return cb ? cb : 16;
}
bool s2_agg_from_count_applies(const mhx_ctx *c, uint32_t k, uint32_t m);  // s2.hip: stage 2's solid items from a count of the (k+1)-mers  // count bits of a compact aggregated stage-2 item (k = 23..28), 0: none
// ... with the count in passes over its own lv1 bucket ranges (s2_count_pass_items): at most kS2CountMaxPasses of them; s2_count_records: the
// records of the whole count; s2_from_count_need: the device bytes the route holds beyond the stage's fixed state with passes of pass_records
// records and n_items aggregated + '$' items (mhx_s2_from_count_bytes, and the route's own check against s2_count_budget_mb).
// kS2CountItemBytes per item: two 8-byte buffers, the first grown by a quarter of headroom with old and new held during the copy (20),
// the emission's 4-byte word per item, and a byte for the sort's status words and the SdBG records
constexpr int kS2CountMaxPasses = 64;
constexpr uint64_t kS2CountItemBytes = 25;
uint64_t s2_count_records(const mhx_ctx *c, uint32_t k);
uint64_t s2_from_count_need(const mhx_ctx *c, uint32_t m, uint64_t pass_records, uint64_t n_items);
struct CountStreamOut {
  unsigned grid;      // workgroups = edge regions
  uint32_t cap;       // 8-byte edges a region holds
  uint32_t *counts;   // device: edges per region
  uint32_t *spare;    // the sort buffer the regions live in
  uint32_t *sorted;   // the records, ordered by the plan's prefix
  uint64_t n_items, n_distinct;
  std::string plan;
  unsigned long long *events;  // several GPUs: position << 1 | kind, for the ranks that hold the reads (count.hip k_apply_count_events)
  uint64_t n_events;
  // count_skm_owner: `events` are still per-workgroup regions of ev_cap entries, ev_counts[workgroup] of them filled
  uint32_t ev_cap = 0;
  uint32_t *ev_counts = nullptr;
  // count on super-k-mer records: what a pass made (the caller sums the passes for the plan line)
  const unsigned long long *skm_hp = nullptr;  // the homopolymer windows k_skm_make counted beside the records (nullptr: none)
  bool skm_rep = false;                        // ... and the windows of period <= 4 in the table behind them (s1_skm_rep)
  uint64_t skm_records = 0, skm_windows = 0;
  uint32_t skm_max_bin = 0;
  int skm_bin_bits = 0;
  uint32_t skm_giant_bins = 0, skm_giant_slices = 0, skm_giant_largest = 0;  // s1_skm_giant: the pass's giant bins, their slices, the largest
  std::string skm_why;  // ... and why the option's plan gave the job up (empty: for no reason of the option's)
};
// edges_only: only the solid edges are wanted (no first_0_out / last_0_in: positions do not matter)
bool count_stream_applies(const mhx_ctx *c, uint32_t k, uint32_t m, bool edges_only = false);
// `count` on super-k-mer records (s1_skm.hip): one GPU, 19 <= k <= 21, min count <= 2 (s1_skm_max_m: up to 4).  *touched: the caller's arrays may hold partial results
bool count_skm_applies(const mhx_ctx *c, uint32_t k, uint32_t m);
bool count_skm_groups(mhx_ctx *c, uint32_t k, uint32_t m, uint32_t *first_0_out, uint32_t *last_0_in_p1, unsigned long long *hist, CountStreamOut *o, bool *touched,
                      int pass, int n_passes);
void count_skm_hp_publish(mhx_ctx *c, const unsigned long long *hp, uint32_t k, uint32_t m, unsigned long long *hist, unsigned long long *edges_at,
                          uint64_t *n_edges, uint64_t *n_keys, bool *flagged);
void count_skm_rep_publish(mhx_ctx *c, const unsigned long long *hp, uint32_t k, uint32_t m, unsigned long long *hist, unsigned long long *edges_at,
                           uint64_t *n_edges, uint64_t *n_keys, bool *flagged, uint64_t *n_windows);
// ... on several GPUs, records exchanged by bin (comm.hip dist_count_skm; opt-in: count_skm_dist).  count_skm_owner (s1_skm.hip): the group-by over
// the sources the ranks sent for this rank's bins, edges and events to per-workgroup regions.  count.hip: count_skm_dist_open readies the rank's
// result arrays and runs it (-> false: a region overflowed), count_skm_dist_edges packs the solid edges (hp_sum: this rank publishes the homopolymer
// keys of the tallies summed over the ranks) and splits them by the owner of their lv1 bucket (-> the send buffer, counts per owner),
// count_skm_dist_close orders the n_recv edges received in ws "items_recv", publishes them and stashes the events for their route
bool count_skm_dist_applies(const mhx_ctx *c, uint32_t k, uint32_t m);
bool count_skm_owner(mhx_ctx *c, uint32_t k, uint32_t m, const SkmFront &f, unsigned long long *hist, CountStreamOut *o);
bool count_skm_dist_open(mhx_ctx *c, uint32_t k, uint32_t m, const SkmFront &f, CountStreamOut *o);
const uint32_t *count_skm_dist_edges(mhx_ctx *c, uint32_t k, uint32_t m, CountStreamOut *o, const unsigned long long *hp_sum, uint64_t *counts);
void count_skm_dist_close(mhx_ctx *c, uint32_t k, uint32_t m, const SkmFront &f, const CountStreamOut &o, uint64_t n_recv, uint64_t n_items, mhx_count_result *out);
bool count_presort_applies(const mhx_ctx *c, uint32_t k, uint32_t m);
uint32_t *count_presort(mhx_ctx *c, uint32_t k, uint64_t *n_items, uint32_t **other, int *pbits);
int count_process_presorted(mhx_ctx *c, uint32_t k, uint32_t m, const S1Sources &src, mhx_count_result *out);  // count.hip; -1: gave up
bool count_bucket_histogram_fast(mhx_ctx *c, uint32_t k, unsigned long long *hist);  // s1_front.hip
bool count_stream_groups(mhx_ctx *c, uint32_t k, uint32_t m, uint32_t *first_0_out, uint32_t *last_0_in_p1, unsigned long long *hist, CountStreamOut *o,
                         const S1Sources *pre = nullptr, bool edges_only = false);
int run_s1(mhx_ctx *c, uint32_t k, uint32_t m, int want_mercy, mhx_s1_result *out);
int run_s1_mercy(mhx_ctx *c, uint32_t k, uint64_t *num_mercy);
int run_s2(mhx_ctx *c, uint32_t k, uint32_t m, mhx_sdbg_result *out);
int run_seq2sdbg(mhx_ctx *c, uint32_t k, mhx_sdbg_result *out);
struct MercyShare {  // multi-GPU seq2sdbg --need_mercy (mercy.hip / comm.hip)
  int my_part = 0, n_parts = 1;
  std::function<void(uint8_t *d_flags, uint64_t n)> reduce_flags;  // bitwise OR of the per-position flags over the ranks
};
int run_gen_mercy(mhx_ctx *c, uint32_t k, const uint32_t *cand_packed, uint64_t cand_words, uint64_t n_cand,
                  const uint64_t *cand_start, uint64_t *n_mercy, const MercyShare *share = nullptr);
void upload_sequences(mhx_ctx *c, const uint32_t *packed, uint64_t n_words, uint64_t n_seqs, uint32_t fixed_len,
                      const uint64_t *start_pos);
void upload_fixed_starts(mhx_ctx *c);
void upload_edges(mhx_ctx *c, const uint32_t *raw, uint64_t n_edges, uint32_t k, uint32_t wpe);
void upload_pinned(mhx_ctx *c, void *d_dst, const void *h_src, size_t bytes);
void append_sequences(mhx_ctx *c, const uint32_t *packed, uint64_t n_words, uint64_t n_new, uint32_t fixed_len, const uint64_t *start_pos,
                      const uint16_t *mult);
void upload_bin_records(mhx_ctx *c, const uint32_t *records, uint64_t n_words, uint64_t n_seqs, int reverse);

inline int round_up2(int x) { return (x + 1) & ~1; }
inline uint64_t div_ceil(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

}  // namespace mhx
