// Navigation of the device-resident succinct de Bruijn graph (the MHX_BUF_SDBG_* buffers mhx_sdbg_build_index leaves in
// HBM), shared by tip trimming (sdbg_tips.hip) and the unitig graph (sdbg_unitig.hip): the reference's SDBG member
// functions (src/sdbg/sdbg.h) as device functions over one DevSdbg.  rank / select are answered from the
// reference-layout tables (l2 + l1 + in-interval popcounts; select = binary search over the intervals between two select
// samples, then a word scan).
#pragma once
#include "dev_prims.h"
#include "mhx_internal.h"

namespace mhx {

struct DevSdbg {
  const unsigned long long *w, *last, *tip;
  unsigned long long *invalid;
  uint64_t n;
  const long long *w_l2;      // [9][num_l2_w]
  const uint16_t *w_l1;       // [9][num_l1_w]
  const uint32_t *w_sel;      // concatenated, offsets w_sel_off[c]
  const long long *last_l2;
  const uint16_t *last_l1;
  const uint32_t *last_sel;
  uint64_t num_l1_w, num_l2_w, num_l1_b, num_l2_b;
  uint64_t w_sel_off[10];
  uint64_t w_count[9], last_count;
  long long f[6], rank_f[6];
  // GetLabel / EdgeReverseComplement / EdgeMultiplicity (sdbg_unitig.hip)
  const long long *tip_l2;    // rank-only structure over tip
  const uint16_t *tip_l1;
  const uint32_t *labels;     // words_per_tip_label words per tip, chars reversed inside each word
  const long long *lkt;       // [65536][2] first / last item of every bucket
  const uint16_t *mul;
  uint32_t k, wpt;
};
constexpr uint64_t kNull = ~0ull;

static __device__ __forceinline__ unsigned sd_w(const DevSdbg &g, uint64_t x) { return (unsigned)(g.w[x >> 4] >> (4 * (x & 15))) & 15u; }
static __device__ __forceinline__ bool sd_bit(const unsigned long long *v, uint64_t x) { return (v[x >> 6] >> (x & 63)) & 1ull; }
static __device__ __forceinline__ bool sd_last_or_tip(const DevSdbg &g, uint64_t x) { return ((g.last[x >> 6] | g.tip[x >> 6]) >> (x & 63)) & 1ull; }
static __device__ __forceinline__ bool sd_valid(const DevSdbg &g, uint64_t x) { return !sd_bit(g.invalid, x); }

static __device__ __forceinline__ unsigned nib_count(unsigned long long x, unsigned c) {  // nibbles of x equal to c
  unsigned long long y = x ^ ~(0x1111111111111111ull * (unsigned long long)c);
  y &= y >> 2;
  y &= y >> 1;
  return (unsigned)__builtin_popcountll(y & 0x1111111111111111ull);
}
// occurrences of character c in W[0 .. pos]  (RankAndSelect::rank(c, pos), kmrns.h:177-183)
static __device__ uint64_t sd_rank_w(const DevSdbg &g, unsigned c, uint64_t pos) {
  const uint64_t itv = (pos + 1) >> 8;  // 256 items per level-1 interval
  uint64_t r = (uint64_t)g.w_l2[c * g.num_l2_w + (itv >> 6)] + g.w_l1[c * g.num_l1_w + itv];
  const uint64_t first = itv << 8, cnt = pos + 1 - first;  // items first .. pos
  const uint64_t w0 = first >> 4;
  uint64_t full = cnt >> 4;
  for (uint64_t i = 0; i < full; ++i) r += nib_count(g.w[w0 + i], c);
  const unsigned rem = (unsigned)(cnt & 15);
  if (rem) {
    // count only the low `rem` nibbles: make the others differ from every c by a per-nibble mask
    unsigned long long x = g.w[w0 + full], y = x ^ ~(0x1111111111111111ull * (unsigned long long)c);
    y &= y >> 2;
    y &= y >> 1;
    r += (unsigned)__builtin_popcountll(y & 0x1111111111111111ull & ((1ull << (4 * rem)) - 1));
  }
  return r;
}
// ones in last[0 .. pos]
static __device__ uint64_t sd_rank_last(const DevSdbg &g, uint64_t pos) {
  const uint64_t itv = (pos + 1) >> 10;  // 1024 bits per level-1 interval
  uint64_t r = (uint64_t)g.last_l2[itv >> 6] + g.last_l1[itv];
  const uint64_t first = itv << 10, cnt = pos + 1 - first;
  const uint64_t w0 = first >> 6;
  const uint64_t full = cnt >> 6;
  for (uint64_t i = 0; i < full; ++i) r += (uint64_t)__builtin_popcountll(g.last[w0 + i]);
  const unsigned rem = (unsigned)(cnt & 63);
  if (rem) r += (uint64_t)__builtin_popcountll(g.last[w0 + full] & ((1ull << rem) - 1));
  return r;
}
// position of the (k+1)-th one of last (k 0-based); n if k == #ones  (RankAndSelect::select, kmrns.h:185-191,282-320)
static __device__ uint64_t sd_select_last(const DevSdbg &g, uint64_t k) {
  if (k > g.last_count) return kNull;
  if (k == g.last_count) return g.n;
  uint64_t lo = g.last_sel[k >> 12], hi = g.last_sel[(k + 4095) >> 12];
  auto occ = [&](uint64_t i) -> uint64_t { return (uint64_t)g.last_l2[i >> 6] + g.last_l1[i]; };
  while (hi > lo) {  // largest interval whose start count is <= k
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (occ(mid) > k) hi = mid - 1;
    else lo = mid;
  }
  uint64_t remain = k + 1 - occ(lo);
  uint64_t wi = (lo << 10) >> 6;
  for (;; ++wi) {
    const unsigned pc = (unsigned)__builtin_popcountll(g.last[wi]);
    if (pc >= remain) break;
    remain -= pc;
  }
  unsigned long long x = g.last[wi];
  for (uint64_t t = 1; t < remain; ++t) x &= x - 1;  // drop the lowest remain-1 ones
  return (wi << 6) + (uint64_t)__builtin_ctzll(x);
}
// position of the (k+1)-th occurrence of character c in W
static __device__ uint64_t sd_select_w(const DevSdbg &g, unsigned c, uint64_t k) {
  if (k > g.w_count[c]) return kNull;
  if (k == g.w_count[c]) return g.n;
  const uint32_t *sel = g.w_sel + g.w_sel_off[c];
  uint64_t lo = sel[k >> 12], hi = sel[(k + 4095) >> 12];
  auto occ = [&](uint64_t i) -> uint64_t { return (uint64_t)g.w_l2[c * g.num_l2_w + (i >> 6)] + g.w_l1[c * g.num_l1_w + i]; };
  while (hi > lo) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (occ(mid) > k) hi = mid - 1;
    else lo = mid;
  }
  uint64_t remain = k + 1 - occ(lo);
  uint64_t wi = (lo << 8) >> 4;
  unsigned long long y;
  for (;; ++wi) {
    y = g.w[wi] ^ ~(0x1111111111111111ull * (unsigned long long)c);
    y &= y >> 2;
    y &= y >> 1;
    y &= 0x1111111111111111ull;
    const unsigned pc = (unsigned)__builtin_popcountll(y);
    if (pc >= remain) break;
    remain -= pc;
  }
  for (uint64_t t = 1; t < remain; ++t) y &= y - 1;
  return (wi << 4) + (uint64_t)(__builtin_ctzll(y) >> 2);
}
static __device__ __forceinline__ unsigned sd_last_char_of(const DevSdbg &g, uint64_t x) {  // sdbg.h:83-90
  for (unsigned i = 1; i < 6; ++i)
    if (g.f[i] > (long long)x) return i - 1;
  return 6;
}
static __device__ uint64_t sd_forward(const DevSdbg &g, uint64_t e) {  // sdbg.h:106-113
  unsigned a = sd_w(g, e);
  if (a > 4) a -= 4;
  const uint64_t count_a = sd_rank_w(g, a, e);
  return sd_select_last(g, (uint64_t)g.rank_f[a] + count_a - 1);
}
static __device__ uint64_t sd_backward(const DevSdbg &g, uint64_t e) {  // sdbg.h:115-121
  const unsigned a = sd_last_char_of(g, e);
  const uint64_t count_a = (e == 0 ? 0 : sd_rank_last(g, e - 1)) - (uint64_t)g.rank_f[a];
  return sd_select_w(g, a, count_a);
}
// ComputeIncomings (sdbg.h:240-283).  mode 0: the in-degree; kMustEq0: -1 as soon as one exists; kUnique: the in-degree,
// -1 as soon as a second exists, *one = the incoming edge when there is exactly one
enum { kAny = 0, kMustEq0 = 1, kUnique = 2 };
static __device__ int sd_incomings(const DevSdbg &g, uint64_t e, int mode, uint64_t *one) {
  if (!sd_valid(g, e)) return -1;
  const uint64_t first = sd_backward(g, e);
  const unsigned c = sd_w(g, first);
  unsigned count_ones = sd_last_or_tip(g, first);
  int indeg = sd_valid(g, first) ? 1 : 0;
  if (mode == kMustEq0 && indeg) return -1;
  if (indeg && one) *one = first;
  for (uint64_t y = first + 1; count_ones < 5 && y < g.n; ++y) {
    count_ones += sd_last_or_tip(g, y);
    const unsigned cur = sd_w(g, y);
    if (cur == c) break;
    if (cur == c + 4 && sd_valid(g, y)) {
      if (mode == kMustEq0) return -1;
      if (mode == kUnique && indeg == 1) return -1;
      if (one) *one = y;  // (only meaningful when it stays the single one)
      ++indeg;
    }
  }
  return indeg;
}
// ComputeOutgoings (sdbg.h:294-323)
static __device__ int sd_outgoings(const DevSdbg &g, uint64_t e, int mode, uint64_t *one) {
  if (!sd_valid(g, e)) return -1;
  int outdeg = 0;
  uint64_t next = sd_forward(g, e);
  do {
    if (sd_valid(g, next)) {
      if (mode == kMustEq0) return -1;
      if (mode == kUnique && outdeg == 1) return -1;
      if (one) *one = next;
      ++outdeg;
    }
    --next;
  } while (next != kNull && !sd_last_or_tip(g, next));
  return outdeg;
}
// OutgoingEdges (sdbg.h:354-356): all outgoing edges in the reference's order (from Forward(e) downwards), at most 4
static __device__ int sd_outgoings_all(const DevSdbg &g, uint64_t e, uint64_t out[4]) {
  if (!sd_valid(g, e)) return -1;
  int outdeg = 0;
  uint64_t next = sd_forward(g, e);
  do {
    if (sd_valid(g, next)) {
      if (outdeg < 4) out[outdeg] = next;
      ++outdeg;
    }
    --next;
  } while (next != kNull && !sd_last_or_tip(g, next));
  return outdeg < 4 ? outdeg : 4;
}
static __device__ __forceinline__ bool sd_indeg_zero(const DevSdbg &g, uint64_t e) { return sd_incomings(g, e, kMustEq0, nullptr) == 0; }
static __device__ __forceinline__ bool sd_outdeg_zero(const DevSdbg &g, uint64_t e) { return sd_outgoings(g, e, kMustEq0, nullptr) == 0; }
static __device__ __forceinline__ uint64_t sd_unique_prev(const DevSdbg &g, uint64_t e) {
  uint64_t r = 0;
  return sd_incomings(g, e, kUnique, &r) == 1 ? r : kNull;
}
static __device__ __forceinline__ uint64_t sd_unique_next(const DevSdbg &g, uint64_t e) {
  uint64_t r = 0;
  return sd_outgoings(g, e, kUnique, &r) == 1 ? r : kNull;
}
static __device__ __forceinline__ void bit_set(unsigned long long *v, uint64_t x) { atomicOr(&v[x >> 6], 1ull << (x & 63)); }
static __device__ __forceinline__ void bit_unset(unsigned long long *v, uint64_t x) { atomicAnd(&v[x >> 6], ~(1ull << (x & 63))); }

// ones in tip[0 .. pos] (rs_is_tip_.rank, sdbg.h:124-127)
static __device__ uint64_t sd_rank_tip(const DevSdbg &g, uint64_t pos) {
  const uint64_t itv = (pos + 1) >> 10;
  uint64_t r = (uint64_t)g.tip_l2[itv >> 6] + g.tip_l1[itv];
  const uint64_t first = itv << 10, cnt = pos + 1 - first;
  const uint64_t w0 = first >> 6;
  const uint64_t full = cnt >> 6;
  for (uint64_t i = 0; i < full; ++i) r += (uint64_t)__builtin_popcountll(g.tip[w0 + i]);
  const unsigned rem = (unsigned)(cnt & 63);
  if (rem) r += (uint64_t)__builtin_popcountll(g.tip[w0 + full] & ((1ull << rem) - 1));
  return r;
}
static __device__ __forceinline__ const uint32_t *sd_tip_label(const DevSdbg &g, uint64_t x) {  // TipLabelStartPtr, sdbg.h:123-128
  return g.labels + (uint64_t)g.wpt * (sd_rank_tip(g, x) - 1);
}
static __device__ __forceinline__ unsigned sd_tip_char(const uint32_t *label, unsigned j) {  // CharAtTipLabel: 1..4
  return ((label[j >> 4] >> (2 * (j & 15))) & 3u) + 1u;
}
// GetLabel (sdbg.h:214-233): the k characters (1..4) of the node edge `id` leaves
static __device__ void sd_label(const DevSdbg &g, uint64_t id, uint8_t *seq) {
  uint64_t x = id;
  for (int i = (int)g.k - 1; i >= 0; --i) {
    if (sd_bit(g.tip, x)) {
      const uint32_t *tl = sd_tip_label(g, x);
      for (int j = 0; j <= i; ++j) seq[i - j] = (uint8_t)sd_tip_char(tl, (unsigned)j);
      break;
    }
    x = sd_backward(g, x);
    unsigned c = sd_w(g, x);
    seq[i] = (uint8_t)(c > 4 ? c - 4 : c);
  }
}
// first position >= x whose last bit is set (GetLastIndex = rs_last_.succ, kmrns.h:216-222)
static __device__ __forceinline__ uint64_t sd_last_index(const DevSdbg &g, uint64_t x) {
  if (sd_bit(g.last, x)) return x;
  return sd_select_last(g, x == 0 ? 0 : sd_rank_last(g, x - 1));
}
// IndexBinarySearch (sdbg.h:141-212): the last edge of the node whose label is seq[0 .. k), or kNull
static __device__ uint64_t sd_index_search(const DevSdbg &g, const uint8_t *seq) {
  const int k = (int)g.k;
  uint64_t prefix = 0;
  for (int i = 0; i < 8; ++i) {  // 65536 buckets: the last 8 characters
    if (seq[k - 1 - i] < 1 || seq[k - 1 - i] > 4) return kNull;
    prefix = prefix * 4 + seq[k - 1 - i] - 1;
  }
  long long l = g.lkt[2 * prefix], r = g.lkt[2 * prefix + 1];
  while (l <= r) {
    int cmp = 0;
    const uint64_t mid = (uint64_t)(l + r) / 2;
    uint64_t y = mid;
    for (int i = k - 1; i >= 0; --i) {
      if (sd_bit(g.tip, y)) {
        const uint32_t *tl = sd_tip_label(g, y);
        for (int j = 0; j < i; ++j) {
          const unsigned c = sd_tip_char(tl, (unsigned)j);
          if (c < seq[i - j]) { cmp = -1; break; }
          if (c > seq[i - j]) { cmp = 1; break; }
        }
        if (cmp == 0) {
          if (sd_bit(g.tip, mid)) {
            cmp = -1;
          } else {
            const unsigned c = sd_tip_char(tl, (unsigned)i);
            if (c < seq[0]) cmp = -1;
            else if (c > seq[0]) cmp = 1;
          }
        }
        break;
      }
      y = sd_backward(g, y);
      const unsigned c = sd_w(g, y);
      if (c < seq[i]) { cmp = -1; break; }
      if (c > seq[i]) { cmp = 1; break; }
    }
    if (cmp == 0) return sd_last_index(g, mid);
    if (cmp > 0) r = (long long)mid - 1;
    else l = (long long)mid + 1;
  }
  return kNull;
}
// EdgeReverseComplement (sdbg.h:432-467)
static __device__ uint64_t sd_edge_rc(const DevSdbg &g, uint64_t e) {
  if (!sd_valid(g, e)) return kNull;
  uint8_t seq[MHX_MAX_K + 1];
  sd_label(g, e, seq);
  unsigned we = sd_w(g, e);
  seq[g.k] = (uint8_t)(we > 4 ? we - 4 : we);
  for (int i = 0, j = (int)g.k; i < j; ++i, --j) {
    const uint8_t t = seq[i];
    seq[i] = seq[j];
    seq[j] = t;
  }
  for (unsigned i = 0; i < g.k + 1; ++i) seq[i] = (uint8_t)(5 - seq[i]);
  uint64_t rev = sd_index_search(g, seq);
  if (rev == kNull) return kNull;
  do {
    const int lab = (int)sd_w(g, rev);
    if (lab == seq[g.k] || lab - 4 == seq[g.k]) return rev;
    --rev;
  } while (rev != kNull && !sd_last_or_tip(g, rev));
  return kNull;
}
// PrevSimplePathEdge / NextSimplePathEdge (sdbg.h:405-429)
static __device__ __forceinline__ uint64_t sd_prev_simple(const DevSdbg &g, uint64_t e) {
  const uint64_t p = sd_unique_prev(g, e);
  return p != kNull && sd_unique_next(g, p) != kNull ? p : kNull;
}
static __device__ __forceinline__ uint64_t sd_next_simple(const DevSdbg &g, uint64_t e) {
  const uint64_t n = sd_unique_next(g, e);
  return n != kNull && sd_unique_prev(g, n) != kNull ? n : kNull;
}
// the out-degree of an edge (EdgeOutdegree / OutgoingEdges, sdbg.h:336-357), what UnitigGraph::GetNextAdapters counts
static __device__ __forceinline__ int sd_outdegree(const DevSdbg &g, uint64_t e) { return sd_outgoings(g, e, kAny, nullptr); }

// the DevSdbg view of the buffers mhx_sdbg_build_index left in the handle (`who` names the caller in the error)
DevSdbg dev_sdbg(mhx_ctx *c, const mhx_sdbg_index_info *info, const char *who);

}  // namespace mhx
