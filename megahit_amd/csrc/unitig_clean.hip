// Graph cleaning on the device-resident unitig graph: what `assemble --bubble_level 0..2 --prune_level 0..3 --cleaning_rounds N`
// does between UnitigGraph::UnitigGraph and the last OutputContigs (reference src/main_assemble.cpp:182-301) —
//   DisconnectWeakLinks  assembly/weak_link_remover.cpp
//   RemoveTips           assembly/tip_remover.cpp (on the unitig graph, not the SdBG-level one of sdbg_tips.hip)
//   RemoveLocalLowDepth, IterateLocalLowDepth  assembly/low_depth_remover.cpp:10-102 (prune levels 1 and 2)
//   RemoveLowDepth       assembly/low_depth_remover.cpp:104-117 (prune level 3)
//   PopBubbles           assembly/bubble_remover.cpp (NaiveBubbleRemover, ComplexBubbleRemover with GetSimilarity, the
//                        --careful_bubble records; bubble levels 1 and 2)
//   UnitigGraph::Refresh assembly/unitig_graph.cpp:140-355 (RefreshDisconnected, deletion, path and cycle merging, compaction,
//                        the is_changed mark of Refresh(true))
// on MHX_BUF_UNITIG_VERTICES (the vertex table mhx_sdbg_unitigs left) and MHX_BUF_SDBG_INVALID.  The result is the
// reference's at -t 1, where every step is independent of the order the vertices are visited in.
//
//   owner     the reference's id_map_ for every edge, not only the begins: own[e] = the vertex edge e lies on (either strand).
//             Filled once from the chain heads of the edge ranking, renamed after every Refresh (one thread per edge).
//   marking   one thread per vertex; flags (to delete, to disconnect per strand) in a word per vertex, set with atomicOr —
//             the count is the flags newly set, as in the reference.
//   Refresh   RefreshDisconnected: one thread per vertex plans its new ends (reads only), a second kernel invalidates the
//             four dropped edges.  Deleted vertices: one thread per EDGE looks its owner up — nobody walks a vertex.
//             Merging: (vertex, strand) nodes, next[(v,s)] = the node NextSimplePathEdge(end(v,s)) begins; pointer jumping
//             (unitig_rank.h) gives every node its path's head and the sums of length and depth head..itself, so a path's
//             survivor — the lower-indexed of its two end vertices, walking from its end that has no predecessor — reads
//             its totals at the path's tail.  Nodes left over lie on cycles: min-propagation names the lowest node, the
//             cycle is cut there and summed by the same jumps.  A hairpin path meets its survivor again in the other
//             orientation and a self-complementary cycle meets every vertex twice: the sums count them twice, as the
//             reference's walks do (and such a cycle's survivor deletes itself there, unless it is palindromic: it does here).
//             Survivors are compacted in index order by a prefix sum.  Refresh(true) marks the survivor of a merged path or
//             cycle MHX_UNITIG_CHANGED (unitig_graph.cpp:293,334); a vertex that merged with nothing keeps the flag it had.
//   cost      log2(longest merged path) jump rounds with one host synchronisation each, everything else O(1) launches.
#include "sdbg_nav.h"
#include "unitig_rank.h"

namespace mhx {

namespace {

constexpr uint32_t kNoVtx = 0xffffffffu;
enum : uint32_t { kDel = 1u, kDisc0 = 2u, kDisc1 = 4u };  // UnitigGraphVertex::flag bits 5, 6, 7

struct DevUg {
  mhx_unitig_vertex *vtx;
  uint32_t *mark;  // [nv]
  uint32_t *own;   // [n edges]
  uint64_t nv;
};

__device__ __forceinline__ uint64_t v_begin(const mhx_unitig_vertex &v, unsigned s) { return s ? v.rb : v.b; }
__device__ __forceinline__ uint64_t v_end(const mhx_unitig_vertex &v, unsigned s) { return s ? v.re : v.e; }
__device__ __forceinline__ double v_avg(const mhx_unitig_vertex &v) { return (double)v.total_depth / (double)v.length; }  // GetAvgDepth
// MakeVertexAdapterWithSdbgId (unitig_graph.h:143-150): the node 2 * vertex + strand that begins at edge x
__device__ __forceinline__ uint64_t node_of_edge(const DevUg &u, uint64_t x) {
  const uint32_t w = u.own[x];
  if (w >= u.nv) return kNull;
  return 2ull * w + (u.vtx[w].b == x ? 0u : 1u);
}
// navigation from a vertex end; an end without an edge (no reverse complement in the graph) has no neighbour
__device__ __forceinline__ int outs_of(const DevSdbg &g, uint64_t e, uint64_t out[4]) { return e < g.n ? sd_outgoings_all(g, e, out) : 0; }
__device__ __forceinline__ uint64_t next_simple_of(const DevSdbg &g, uint64_t e) { return e < g.n ? sd_next_simple(g, e) : kNull; }
__device__ __forceinline__ uint64_t prev_simple_of(const DevSdbg &g, uint64_t e) { return e < g.n ? sd_prev_simple(g, e) : kNull; }
__device__ __forceinline__ void wave_count(bool hit, unsigned long long *cnt) {
  const uint64_t m = __ballot(hit);
  if (m && lane_id() == __builtin_ctzll(m)) atomicAdd(cnt, (unsigned long long)__builtin_popcountll(m));
}

// ---- owner map ----
__global__ __launch_bounds__(256) void k_uc_head_vid(const mhx_unitig_vertex *__restrict__ vtx, uint64_t nv, uint64_t n, uint32_t *__restrict__ hv) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  if (vtx[v].b < n) hv[vtx[v].b] = (uint32_t)v;
  if (vtx[v].rb < n) hv[vtx[v].rb] = (uint32_t)v;
}
__global__ __launch_bounds__(256) void k_uc_own_init(DevSdbg g, const Rk *__restrict__ rk, const uint32_t *__restrict__ hv, uint32_t *__restrict__ own) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  uint32_t w = kNoVtx;
  if (sd_valid(g, i)) {
    const uint64_t h = rk[i].head;
    if (h < g.n) w = hv[h];
  }
  own[i] = w;
}
__global__ __launch_bounds__(256) void k_uc_own_rename(uint32_t *__restrict__ own, uint64_t n, uint64_t nv, const uint32_t *__restrict__ rep,
                                                      const uint64_t *__restrict__ newid) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t w = own[i];
  if (w >= nv) return;
  const uint32_t r = rep[w];
  own[i] = r == kNoVtx ? kNoVtx : (uint32_t)newid[r];
}

// ---- DisconnectWeakLinks (weak_link_remover.cpp:8-34) ----
__global__ __launch_bounds__(256) void k_uc_weak(DevSdbg g, DevUg u, double ratio, unsigned long long *__restrict__ cnt) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned newly = 0;
  if (v < u.nv && !(u.vtx[v].flags & (MHX_UNITIG_LOOP | MHX_UNITIG_PALINDROME))) {
    const mhx_unitig_vertex vx = u.vtx[v];
    for (unsigned s = 0; s < 2; ++s) {
      uint64_t outs[4];
      const int deg = outs_of(g, v_end(vx, s), outs);
      if (deg <= 1) continue;
      uint64_t nd[4];
      double dep[4], total = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        nd[j] = kNull;
        dep[j] = 0;
        if (j < deg) {
          nd[j] = node_of_edge(u, outs[j]);
          if (nd[j] != kNull) dep[j] = v_avg(u.vtx[nd[j] >> 1]);
          total += dep[j];
        }
      }
      const double limit = __dmul_rn(ratio, total);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < deg && nd[j] != kNull && dep[j] <= limit) {
          const uint32_t bit = kDisc0 << (nd[j] & 1);  // SetToDisconnect on the strand it is entered by
          newly += !(atomicOr(&u.mark[nd[j] >> 1], bit) & bit);
        }
      }
    }
  }
  if (newly) atomicAdd(cnt, (unsigned long long)newly);
}

// ---- RemoveTips, one threshold (tip_remover.cpp:12-45): degrees and depths of before the pass, flags only ----
__global__ __launch_bounds__(256) void k_uc_tips(DevSdbg g, DevUg u, uint32_t thre, unsigned long long *__restrict__ cnt) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool del = false;
  if (v < u.nv && u.vtx[v].length < thre) {
    const mhx_unitig_vertex vx = u.vtx[v];
    if (vx.flags & MHX_UNITIG_LOOP) {
      del = true;
    } else {
      uint64_t nexts[4], prevs[4];
      const int outd = outs_of(g, vx.e, nexts), ind = outs_of(g, vx.re, prevs);
      uint64_t nb = kNull;
      if (ind + outd == 0) del = true;
      else if (outd == 1 && ind == 0) nb = node_of_edge(u, nexts[0]);
      else if (outd == 0 && ind == 1) nb = node_of_edge(u, prevs[0]);
      if (nb != kNull) del = v_avg(u.vtx[nb >> 1]) > __dmul_rn(8.0, v_avg(vx));
    }
    if (del) del = !(atomicOr(&u.mark[v], kDel) & kDel);
  }
  wave_count(del, cnt);
}

// ---- RemoveLocalLowDepth, one pass (low_depth_remover.cpp:10-86) ----
// Every decision reads only what the pass never writes: the vertex's own length and average depth, the SdBG degrees at its two
// ends, and length / total depth of its neighbours; the pass sets to-delete flags and nothing else (Refresh invalidates edges
// afterwards).  The one thing that depends on the visiting order in the reference is the early `continue` of line 60
// (is_changed already set and depth > min_depth) — and it changes nothing: threshold is min_depth or, in the else branch,
// mean * local_ratio <= min_depth, so such a vertex has depth > threshold and is not deleted, and is_changed is already true.
// Hence, whatever the order:  deleted = the qualifying vertices with depth < threshold;  is_changed = some qualifying vertex has
// min_depth < mean * local_ratio, or some vertex is deleted;  removed = the number deleted (SetToDelete succeeds once each).
// Qualifying (lines 49-58): no loop, length <= max_len, in + out degree > 0, and (in <= 1 and out <= 1) or in == 0 or out == 0.
// LocalDepth in the reference's order and in plain IEEE double, nothing contracted: strand 0's out-neighbours in OutgoingEdges
// order, then strand 1's (a palindromic vertex has e == re and counts its neighbours twice, as the strand loop does).
// cnt[0] += flags newly set, cnt[1] |= 1 when is_changed — one atomic each per wavefront that needs it.
__global__ __launch_bounds__(256) void k_uc_low_depth(DevSdbg g, DevUg u, double min_depth, uint32_t max_len, uint32_t local_width, double local_ratio,
                                                     unsigned long long *__restrict__ cnt) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool del = false, chg = false;
  if (v < u.nv && !(u.vtx[v].flags & MHX_UNITIG_LOOP) && u.vtx[v].length <= max_len) {
    const mhx_unitig_vertex vx = u.vtx[v];
    uint64_t outs[2][4];
    int deg[2];
    deg[0] = outs_of(g, vx.e, outs[0]);   // OutDegree
    deg[1] = outs_of(g, vx.re, outs[1]);  // InDegree
    if (deg[0] + deg[1] != 0 && ((deg[1] <= 1 && deg[0] <= 1) || deg[1] == 0 || deg[0] == 0)) {
      double total = 0;
      uint64_t added = 0;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j >= deg[s]) continue;
          const uint64_t nb = node_of_edge(u, outs[s][j]);
          if (nb == kNull) continue;
          const mhx_unitig_vertex &w = u.vtx[nb >> 1];
          if (w.length <= local_width) {
            added += w.length;
            total = __dadd_rn(total, (double)w.total_depth);
          } else {
            added += local_width;
            total = __dadd_rn(total, __dmul_rn(v_avg(w), (double)local_width));
          }
        }
      }
      const double mean = added ? total / (double)added : 0.0;
      const double limit = __dmul_rn(mean, local_ratio);
      double threshold = min_depth;
      if (min_depth < limit) chg = true;
      else threshold = limit;
      if (v_avg(vx) < threshold) {
        chg = true;
        del = !(atomicOr(&u.mark[v], kDel) & kDel);
      }
    }
  }
  wave_count(del, cnt);
  const uint64_t m = __ballot(chg);
  if (m && lane_id() == __builtin_ctzll(m)) atomicOr(cnt + 1, 1ull);
}

// ---- RemoveLowDepth (low_depth_remover.cpp:104-117): every vertex below min_depth, loops included ----
__global__ __launch_bounds__(256) void k_uc_remove_low_depth(DevUg u, double min_depth, unsigned long long *__restrict__ cnt) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool del = false;
  if (v < u.nv && v_avg(u.vtx[v]) < min_depth) del = !(atomicOr(&u.mark[v], kDel) & kDel);
  wave_count(del, cnt);
}

// ---- BaseBubbleRemover::PopBubbles (bubble_remover.cpp:58-152) ----
// SearchAndPopBubble reads only what the pass never writes (SdBG degrees and neighbours, vertex lengths, total depths, begin and
// end edges) and writes only to-delete flags, whose fetch-or return value is the count.  So the deleted set is the union over the
// (vertex, strand) nodes of what each search finds and the count is the number of distinct vertices in it, whatever the order:
// one thread per node.  A bubble whose left and right are the same vertex is found from both sides and a palindromic left twice
// from the same end: the second visit sets no new flag — but writes its careful records again, as the reference does.
//   find   the structural tests and the sort of the middles (average depth descending, canonical id ascending).  Naive mode
//          (the checker is always true) marks at once; complex mode runs the checker's two length-ratio tests and lists the
//          node as a candidate.  With careful records or in complex mode the sorted middles and the right vertex are kept per node.
//   score  complex mode: GetSimilarity of (middle[0], middle[j]) for every candidate, one wavefront per pair (k_uc_similarity).
//   mark   complex mode: the candidates whose pairs all passed.
//   records  --careful_bubble: rec_n[node] = middles j >= 1 with avg >= avg(middle[0]) * threshold, + 2 (left, right) when there
//          is one; a prefix sum over the nodes is the reference's -t 1 order (vertex index, strand 0 then 1, then j).
struct BubArgs {
  uint32_t max_len, k;
  double sim;      // <= 0: naive
  double careful;  // < 0: no records
};
struct BubBuf {
  uint32_t *mid;    // [4 * nodes] the sorted middles' vertices
  uint32_t *right;  // [nodes] the right vertex
  uint32_t *deg;    // [nodes] the bubble's degree; 0: no bubble starts here
  uint32_t *rec_n;  // [nodes]
};
__device__ __forceinline__ uint64_t v_canon(const mhx_unitig_vertex &v) { return v.b < v.rb ? v.b : v.rb; }
// marks middle[1..] and counts this node's records; returns the flags newly set
__device__ __forceinline__ unsigned bubble_pop(const DevUg &u, const uint32_t mid[4], int deg, double careful, uint32_t *rec_n) {
  unsigned newly = 0, recs = 0;
  const double limit = careful >= 0 ? __dmul_rn(v_avg(u.vtx[mid[0]]), careful) : 0.0;
  for (int j = 1; j < deg; ++j) {
    newly += !(atomicOr(&u.mark[mid[j]], kDel) & kDel);
    if (careful >= 0 && v_avg(u.vtx[mid[j]]) >= limit) ++recs;
  }
  if (rec_n) *rec_n = recs ? recs + 2 : 0;
  return newly;
}
__global__ __launch_bounds__(256) void k_uc_bubble_find(DevSdbg g, DevUg u, BubArgs a, BubBuf bb, uint64_t *__restrict__ cand, unsigned long long *__restrict__ cnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool keep = a.sim > 0 || a.careful >= 0;
  unsigned newly = 0;
  int found = 0;  // the degree of the bubble that starts here
  uint32_t mid[4] = {kNoVtx, kNoVtx, kNoVtx, kNoVtx}, rv = kNoVtx;
  if (t < 2 * u.nv && !(u.vtx[t >> 1].flags & MHX_UNITIG_LOOP)) {
    const mhx_unitig_vertex left = u.vtx[t >> 1];
    uint64_t outs[4], tmp[4];
    const int deg = outs_of(g, v_end(left, (unsigned)(t & 1)), outs);
    bool ok = deg > 1;
    uint64_t nd[4] = {kNull, kNull, kNull, kNull}, right_b = kNull;
    for (int j = 0; ok && j < deg; ++j) {
      nd[j] = node_of_edge(u, outs[j]);
      ok = nd[j] != kNull && u.vtx[nd[j] >> 1].length <= a.max_len;
    }
    for (int j = 0; ok && j < deg; ++j) {
      const mhx_unitig_vertex &m = u.vtx[nd[j] >> 1];
      const unsigned s = (unsigned)(nd[j] & 1);
      ok = outs_of(g, v_end(m, s ^ 1), tmp) == 1 && outs_of(g, v_end(m, s), tmp) == 1;  // InDegree, GetNextAdapters
      if (!ok) break;
      if (j == 0) {
        right_b = tmp[0];
        const uint64_t r = node_of_edge(u, right_b);
        ok = r != kNull;
        if (ok) {
          const mhx_unitig_vertex &rx = u.vtx[r >> 1];
          rv = (uint32_t)(r >> 1);
          ok = v_canon(rx) >= v_canon(left) && outs_of(g, v_end(rx, (unsigned)(r & 1) ^ 1), tmp) == deg;
        }
      } else {
        ok = tmp[0] == right_b;
      }
    }
    if (ok) {
      // std::sort of at most four adapters: an insertion sort with the reference's comparator
      double avg[4] = {0, 0, 0, 0};
      uint64_t can[4] = {0, 0, 0, 0};
      for (int j = 0; j < deg; ++j) {
        const mhx_unitig_vertex &m = u.vtx[nd[j] >> 1];
        const double d = v_avg(m);
        const uint64_t cid = v_canon(m);
        const uint32_t w = (uint32_t)(nd[j] >> 1);
        int p = j;
        while (p > 0 && (d != avg[p - 1] ? d > avg[p - 1] : cid < can[p - 1])) {
          avg[p] = avg[p - 1];
          can[p] = can[p - 1];
          mid[p] = mid[p - 1];
          --p;
        }
        avg[p] = d;
        can[p] = cid;
        mid[p] = w;
      }
      if (a.sim > 0) {  // ComplexBubbleRemover's checker, the length part (bubble_remover.cpp:164-165)
        const double l0 = (double)(u.vtx[mid[0]].length + a.k - 1);
        for (int j = 1; ok && j < deg; ++j) {
          const double lj = (double)(u.vtx[mid[j]].length + a.k - 1);
          ok = __dmul_rn(lj, a.sim) <= l0 && __dmul_rn(l0, a.sim) <= lj;
        }
      }
      if (ok) found = deg;
    }
  }
  uint32_t rec_n = 0;
  if (found && !(a.sim > 0)) newly = bubble_pop(u, mid, found, a.careful, &rec_n);
  if (keep && t < 2 * u.nv) {
    bb.deg[t] = (uint32_t)found;
    bb.rec_n[t] = rec_n;
    if (found) {
      for (int j = 0; j < 4; ++j) bb.mid[4 * t + j] = mid[j];
      bb.right[t] = rv;
    }
  }
  if (a.sim > 0) push_list(found != 0, t, cand, cnt + 1);
  const unsigned total = wave_sum(newly);
  if (total && lane_id() == 0) atomicAdd(cnt, (unsigned long long)total);
}

// ---- GetSimilarity (bubble_remover.cpp:10-54): the banded edit distance of two strings, one wavefront per pair ----
// Cell c of row i stands for column j = i + c - D (D = max_indel), c in [0, 2D].  The cell above-left (j - 1 of row i - 1) is
// the same c of the previous row, the cell above (j of row i - 1) is c + 1 of it, and the cell to the left is c - 1 of this row:
//   t[c]  = min(INF, prev[c] + (a[i-1] != b[j-1]), prev[c+1] + 1 when c < 2D)        every lane on its own
//   dp[c] = min(t[c], dp[c-1] + 1) = c + min over c' <= c of (t[c'] - c')            a prefix minimum: integer min-plus, exact
// The cells of a row that the reference computes are contiguous: j = max(i - D, 1) .. min(m, i + D), and j = 0 (value i) to
// their left while i <= D; every other cell of the row is INF (0x3f3f3f3f) as its std::fill leaves it.  Row 0 is j for j >= 0
// and 0 below, as its resize leaves it.  Rows of more than 64 cells go in 64-cell chunks with the running minimum carried
// from chunk to chunk.  The two rows live in LDS: lane l reads words c and c + 1 = consecutive banks, no conflict.
// Cap: max_indel <= kSimMaxIndel (band of 4095 cells, 2 rows * 4096 * 4 bytes = 32 KB of LDS) and strings of <= kSimMaxLen.
constexpr int kSimMaxIndel = MHX_SIM_MAX_INDEL, kSimRow = 2 * kSimMaxIndel + 2, kSimInf = 0x3f3f3f3f;
constexpr uint32_t kSimMaxLen = MHX_SIM_MAX_LEN;
static_assert(2 * kSimRow * sizeof(int) <= 32768, "the two rows of the band take half of a workgroup's default 64 KB of LDS");
struct SimPair {
  uint64_t a, b;  // where the two strings start in the text
  uint32_t n, m;
};
__device__ __forceinline__ int wave_inclusive_min(int v) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(v, d, kWave);
    if (lane_id() >= d) v = o < v ? o : v;
  }
  return v;
}
__device__ double wave_similarity(const char *__restrict__ sa, int n, const char *__restrict__ sb, int m, double one_minus_sim, int (*row)[kSimRow]) {
  const int lane = lane_id();
  const int mx = n > m ? n : m;
  const int D = (int)__dmul_rn((double)mx, one_minus_sim);
  if (abs(n - m) > D || D < 1 || D > kSimMaxIndel) return 0.0;  // (beyond the cap: the host refused before the launch)
  const int W = 2 * D + 1;
  for (int c = lane; c < W; c += kWave) row[0][c] = c >= D ? c - D : 0;
  __syncthreads();
  for (int i = 1; i <= n; ++i) {
    int *cur = row[i & 1];
    const int *prev = row[(i & 1) ^ 1];
    const char ca = sa[i - 1];
    const int c_lo = i <= D ? D - i : 0, c_hi = (m - i + D < 2 * D) ? m - i + D : 2 * D;
    int carry = 0x7fffffff;
    for (int cb = 0; cb < W; cb += kWave) {
      const int c = cb + lane;
      const bool valid = c >= c_lo && c <= c_hi;
      int x = 0x7fffffff;
      if (valid) {
        const int j = i + c - D;
        int tv = i;  // j == 0
        if (j > 0) {
          tv = kSimInf;
          const int dg = prev[c] + (ca != sb[j - 1]);
          tv = dg < tv ? dg : tv;
          if (c < 2 * D) {
            const int up = prev[c + 1] + 1;
            tv = up < tv ? up : tv;
          }
        }
        x = tv - c;
      }
      x = wave_inclusive_min(x);
      x = carry < x ? carry : x;
      carry = __shfl(x, kWave - 1, kWave);
      if (c < W) cur[c] = valid ? x + c : kSimInf;
    }
    __syncthreads();
  }
  const int d = row[n & 1][m - n + D];
  return __dsub_rn(1.0, __ddiv_rn((double)d, (double)mx));  // 1 - d * 1.0 / max(n, m)
}
// one block of one wavefront per pair (blocks stride over the pairs)
__global__ __launch_bounds__(64) void k_uc_similarity(const char *__restrict__ text, const SimPair *__restrict__ pairs, uint64_t n_pairs, double one_minus_sim,
                                                     double *__restrict__ out) {
  __shared__ int row[2][kSimRow];
  for (uint64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const SimPair q = pairs[p];
    const double r = q.n == 0xffffffffu ? 2.0 : wave_similarity(text + q.a, (int)q.n, text + q.b, (int)q.m, one_minus_sim, row);  // (n = ~0: no such pair)
    if (lane_id() == 0) out[p] = r;
    __syncthreads();
  }
}
// the pairs of the candidates: slot 3 * i + j - 1 is (middle[0], middle[j]) of candidate i, each in its own unique format —
// the text of mhx_unitig_finish — so the two may lie on opposite strands, as in the reference
__global__ __launch_bounds__(256) void k_uc_bubble_pairs(BubBuf bb, const uint64_t *__restrict__ cand, uint64_t n_cand, const uint64_t *__restrict__ off,
                                                       SimPair *__restrict__ pairs) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 3 * n_cand) return;
  const uint64_t t = cand[x / 3];
  const int j = (int)(x % 3) + 1;
  SimPair q{0, 0, 0xffffffffu, 0};
  if (j < (int)bb.deg[t]) {
    const uint32_t va = bb.mid[4 * t], vb = bb.mid[4 * t + j];
    q = SimPair{off[va], off[vb], (uint32_t)(off[va + 1] - off[va]), (uint32_t)(off[vb + 1] - off[vb])};
  }
  pairs[x] = q;
}
// cnt[0] += flags newly set; cnt[2] += pairs that passed, cnt[3] += pairs that failed
__global__ __launch_bounds__(256) void k_uc_bubble_mark(DevUg u, BubArgs a, BubBuf bb, const uint64_t *__restrict__ cand, uint64_t n_cand,
                                                      const double *__restrict__ score, unsigned long long *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned newly = 0, pass = 0, fail = 0;
  if (i < n_cand) {
    const uint64_t t = cand[i];
    const int deg = (int)bb.deg[t];
    // the reference stops at the first failing pair; the later ones are scored here all the same and counted as they fall
    for (int j = 1; j < deg; ++j) (score[3 * i + j - 1] >= a.sim ? pass : fail) += 1;
    uint32_t rec_n = 0;
    if (!fail) {
      uint32_t mid[4];
      for (int j = 0; j < 4; ++j) mid[j] = bb.mid[4 * t + j];
      newly = bubble_pop(u, mid, deg, a.careful, &rec_n);
    } else {
      bb.deg[t] = 0;
    }
    bb.rec_n[t] = rec_n;
  }
  const unsigned tn = wave_sum(newly), tp = wave_sum(pass), tf = wave_sum(fail);
  if (lane_id() == 0) {
    if (tn) atomicAdd(cnt, (unsigned long long)tn);
    if (tp) atomicAdd(cnt + 2, (unsigned long long)tp);
    if (tf) atomicAdd(cnt + 3, (unsigned long long)tf);
  }
}
// --careful_bubble records (bubble_remover.cpp:109-132) of node t at rec_off[t] ..: the middles that pass, then left, right
__global__ __launch_bounds__(256) void k_uc_bubble_records(DevUg u, BubArgs a, BubBuf bb, const uint64_t *__restrict__ rec_off, mhx_bubble_record *__restrict__ rec,
                                                         uint64_t *__restrict__ rec_len) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * u.nv || !bb.rec_n[t]) return;
  uint64_t o = rec_off[t];
  const int deg = (int)bb.deg[t];
  const double limit = __dmul_rn(v_avg(u.vtx[bb.mid[4 * t]]), a.careful);
  auto put = [&](uint32_t w) {
    const mhx_unitig_vertex &vx = u.vtx[w];
    rec[o] = mhx_bubble_record{0, vx.length + a.k, w, v_avg(vx)};
    rec_len[o] = (uint64_t)vx.length + a.k;
    ++o;
  };
  for (int j = 1; j < deg; ++j)
    if (v_avg(u.vtx[bb.mid[4 * t + j]]) >= limit) put(bb.mid[4 * t + j]);
  put((uint32_t)(t >> 1));
  put(bb.right[t]);
}
__global__ __launch_bounds__(256) void k_uc_bubble_text(const char *__restrict__ text, const uint64_t *__restrict__ off, const uint64_t *__restrict__ rec_pos, uint64_t n_rec,
                                                      mhx_bubble_record *__restrict__ rec, char *__restrict__ out) {
  for (uint64_t r = blockIdx.x; r < n_rec; r += gridDim.x) {
    const uint64_t src = off[rec[r].vertex], dst = rec_pos[r];
    const uint32_t len = rec[r].length;
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) out[dst + i] = text[src + i];
    if (threadIdx.x == 0) rec[r].offset = dst;
  }
}

// ---- RefreshDisconnected (unitig_graph.cpp:140-208) ----
// plan: the new ends of every trimmed vertex (navigation on the SdBG as it is: a unitig's inner edges see only each other,
// whatever other vertices drop); inv[4v ..] = the edges to invalidate.  bad: a navigation that found no edge.
__global__ __launch_bounds__(256) void k_uc_disc_plan(DevSdbg g, DevUg u, uint64_t *__restrict__ inv, unsigned long long *__restrict__ bad) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= u.nv) return;
  uint64_t drop[4] = {kNull, kNull, kNull, kNull};
  const uint32_t m = u.mark[v];
  mhx_unitig_vertex vx = u.vtx[v];
  const uint32_t d0 = (m & kDisc0) ? 1u : 0u, d1 = (m & kDisc1) ? 1u : 0u;
  if (!(m & kDel) && !(vx.flags & (MHX_UNITIG_LOOP | MHX_UNITIG_PALINDROME)) && (d0 | d1)) {
    if (vx.length <= d0 + d1) {
      u.mark[v] = m | kDel;
    } else {
      uint64_t nb = vx.b, ne = vx.e, nrb = vx.rb, nre = vx.re;
      if (d0) {
        nb = next_simple_of(g, vx.b);
        nre = prev_simple_of(g, vx.re);
        drop[0] = vx.b;
        drop[1] = vx.re;
      }
      if (d1) {
        nrb = next_simple_of(g, vx.rb);
        ne = prev_simple_of(g, vx.e);
        drop[2] = vx.rb;
        drop[3] = vx.e;
      }
      if (nb == kNull || ne == kNull || nrb == kNull || nre == kNull) {
        atomicAdd(bad, 1ull);
        for (int i = 0; i < 4; ++i) drop[i] = kNull;
      } else {
        const uint32_t new_len = vx.length - d0 - d1;
        vx.total_depth = (uint64_t)lround(__dmul_rn(v_avg(vx), (double)new_len));  // not contracted
        vx.length = new_len;
        vx.b = nb;
        vx.e = ne;
        vx.rb = nrb;
        vx.re = nre;
        vx.flags = (vx.flags & ~MHX_UNITIG_PALINDROME) | (nb == nrb ? MHX_UNITIG_PALINDROME : 0u);
        u.vtx[v] = vx;
      }
    }
  }
  for (int i = 0; i < 4; ++i) inv[4 * v + i] = drop[i];
}
__global__ __launch_bounds__(256) void k_uc_disc_apply(unsigned long long *__restrict__ invalid, const uint64_t *__restrict__ inv, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && inv[i] != kNull) bit_set(invalid, inv[i]);  // (only edges the plan navigated from: all inside the graph)
}
// every edge of a to-delete vertex that is no loop becomes invalid (unitig_graph.cpp:214-238): one thread per edge
__global__ __launch_bounds__(256) void k_uc_delete_edges(DevSdbg g, DevUg u) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n || !sd_valid(g, i)) return;
  const uint32_t w = u.own[i];
  if (w < u.nv && (u.mark[w] & kDel) && !(u.vtx[w].flags & MHX_UNITIG_LOOP)) bit_set(g.invalid, i);
}

// ---- merging ----
// next[(v, s)] = NextSimplePathAdapter; deleted vertices and loops take no part.  A palindromic vertex is its own reverse
// complement and is only ever entered as strand 0 (MakeVertexAdapterWithSdbgId), so its strand-1 node stays unlinked and
// its strand-0 node stands for both: the reverse complement of a path through it is that same path (a hairpin).
__global__ __launch_bounds__(256) void k_uc_links(DevSdbg g, DevUg u, uint64_t *__restrict__ succ) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * u.nv) return;
  const uint64_t w = t >> 1;
  uint64_t nx = kNull;
  const uint32_t f = u.vtx[w].flags;
  if (!(u.mark[w] & kDel) && !(f & MHX_UNITIG_LOOP) && !((f & MHX_UNITIG_PALINDROME) && (t & 1))) {
    const uint64_t x = next_simple_of(g, v_end(u.vtx[w], (unsigned)(t & 1)));
    if (x != kNull) nx = node_of_edge(u, x);
  }
  succ[t] = nx;
}
// ranking records: val = depth sum, d = length sum over head..itself.  cut != nullptr: the listed cycle nodes, cut at their
// cycle's minimum (lab[i] = rk[i].val of the min-propagation is kept for the resolve step)
__global__ __launch_bounds__(256) void k_uc_rank_init(DevUg u, const uint64_t *__restrict__ pred, const uint64_t *__restrict__ cyc, uint64_t n_nodes,
                                                     uint64_t *__restrict__ lab, Rk *__restrict__ rk, uint64_t *__restrict__ list, unsigned long long *__restrict__ cnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool take = false;
  uint64_t i = 0;
  if (t < n_nodes) {
    i = cyc ? cyc[t] : t;
    uint64_t p = pred[i];
    if (cyc) {
      const uint64_t m = rk[i].val;
      lab[i] = m;
      if (m == i) p = kNull;
    }
    const mhx_unitig_vertex &vx = u.vtx[i >> 1];
    rk[i] = Rk{p, vx.total_depth, (uint64_t)vx.length, i};
    take = p != kNull;
  }
  push_list(take, i, list, cnt);
}
// who survives (unitig_graph.cpp:240-336): alive[w], rep[w] = the vertex w's edges belong to afterwards (kNoVtx: none)
__global__ __launch_bounds__(256) void k_uc_resolve(DevUg u, const uint64_t *__restrict__ succ, const uint64_t *__restrict__ pred, const Rk *__restrict__ rk,
                                                   const uint64_t *__restrict__ lab, uint32_t *__restrict__ alive, uint32_t *__restrict__ rep) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= u.nv) return;
  const uint64_t n0 = 2 * w, n1 = (u.vtx[w].flags & MHX_UNITIG_PALINDROME) ? n0 : n0 + 1;  // the node of the other strand
  uint32_t a = 1, r = (uint32_t)w;
  if (u.mark[w] & kDel) {
    a = 0;
    r = kNoVtx;
  } else if (u.vtx[w].flags & MHX_UNITIG_LOOP) {
  } else if (lab[n0] != kNull) {
    // on a cycle: its lowest vertex walks it from strand 0 and survives — unless the walk meets that vertex again on its
    // other strand (a cycle that is its own reverse complement; a palindromic vertex has one strand and is met once)
    const uint64_t surv = lab[n0] >> 1;
    const bool meets_itself = !(u.vtx[surv].flags & MHX_UNITIG_PALINDROME) && lab[2 * surv] == lab[2 * surv + 1];
    a = w == surv && !meets_itself;
    r = meets_itself ? kNoVtx : (uint32_t)surv;
  } else if (succ[n0] != kNull || pred[n0] != kNull) {  // on a path H .. T: the lower-indexed end vertex survives
    const uint64_t H = rk[n0].head, T = rk[n1].head ^ 1;
    const uint64_t surv = (H >> 1) < (T >> 1) ? (H >> 1) : (T >> 1);
    a = w == surv;
    r = (uint32_t)surv;
  }
  alive[w] = a;
  rep[w] = r;
}
// the survivors' new records, compacted in index order
__global__ __launch_bounds__(256) void k_uc_write(DevUg u, const uint64_t *__restrict__ succ, const uint64_t *__restrict__ pred, const Rk *__restrict__ rk,
                                                 const uint64_t *__restrict__ lab, const uint32_t *__restrict__ alive, const uint64_t *__restrict__ newid,
                                                 uint32_t set_changed, mhx_unitig_vertex *__restrict__ out) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= u.nv || !alive[w]) return;
  const uint64_t n0 = 2 * w, n1 = (u.vtx[w].flags & MHX_UNITIG_PALINDROME) ? n0 : n0 + 1;
  mhx_unitig_vertex o = u.vtx[w];
  o.flags &= MHX_UNITIG_LOOP | MHX_UNITIG_PALINDROME | MHX_UNITIG_CHANGED;
  // is_changed: kept, and set on the survivor of a merge when this Refresh marks (set_changed = MHX_UNITIG_CHANGED, else 0)
  const uint32_t chg = (o.flags & MHX_UNITIG_CHANGED) | set_changed;
  if (o.flags & MHX_UNITIG_LOOP) {
  } else if (lab[n0] != kNull) {  // unitig_graph.cpp:309-333: the walk from (w, 0) round the cycle, cut at (w, 0)
    const uint64_t P = pred[n0], N = succ[n1];
    o.e = v_end(u.vtx[P >> 1], (unsigned)(P & 1));            // PrevSimplePathEdge(b)
    if (N != kNull) o.rb = v_begin(u.vtx[N >> 1], (unsigned)(N & 1));  // NextSimplePathEdge(re)
    o.total_depth = rk[P].val;
    o.length = (uint32_t)rk[P].d;
    o.flags = MHX_UNITIG_LOOP | (o.b == o.rb ? MHX_UNITIG_PALINDROME : 0u) | chg;
  } else if (succ[n0] != kNull || pred[n0] != kNull) {  // unitig_graph.cpp:275-292: the walk X .. Y from the end without a predecessor
    const uint64_t H = rk[n0].head, T = rk[n1].head ^ 1;
    const uint64_t X = (H >> 1) <= (T >> 1) ? H : (T ^ 1), Y = (H >> 1) <= (T >> 1) ? T : (H ^ 1);
    const unsigned s = (unsigned)(X & 1), ys = (unsigned)(Y & 1);
    const mhx_unitig_vertex y = u.vtx[Y >> 1], x = u.vtx[w];
    const uint64_t nb = v_begin(x, s), ne = v_end(y, ys), nrb = v_begin(y, ys ^ 1), nre = v_end(x, s ^ 1);
    o.b = s ? nrb : nb;  // SetBeginEnd writes relative to the adapter's strand: stored strand 0 stays strand 0
    o.e = s ? nre : ne;
    o.rb = s ? nb : nrb;
    o.re = s ? ne : nre;
    o.total_depth = rk[Y].val;
    o.length = (uint32_t)rk[Y].d;
    o.flags = (o.b == o.rb ? MHX_UNITIG_PALINDROME : 0u) | chg;
  }
  out[newid[w]] = o;
}

// ---- after the last round ----
__global__ __launch_bounds__(256) void k_uc_final_flags(DevSdbg g, mhx_unitig_vertex *__restrict__ vtx, uint64_t nv, unsigned long long *__restrict__ n_loop) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool loop = false;
  if (v < nv) {
    uint32_t f = vtx[v].flags & (MHX_UNITIG_LOOP | MHX_UNITIG_PALINDROME | MHX_UNITIG_CHANGED);
    loop = f & MHX_UNITIG_LOOP;
    uint64_t outs[4];
    if (loop || (outs_of(g, vtx[v].e, outs) == 0 && outs_of(g, vtx[v].re, outs) == 0)) f |= MHX_UNITIG_STANDALONE;
    vtx[v].flags = f;
  }
  wave_count(loop, n_loop);
}

struct Clean {
  mhx_ctx *c;
  hipStream_t st;
  DevSdbg g;
  DevUg u;
  unsigned long long *cnt;

  static dim3 grid(uint64_t m) { return Ranker::grid(m); }

  const mhx_sdbg_index_info *info;

  Clean(mhx_ctx *c_, const mhx_sdbg_index_info *info_, const char *who) : c(c_), st(c_->stream), info(info_) {
    if (!info) throw Error(std::string(who) + ": no index info");
    if (!c->ut_ready || info->n_items != c->ut_edges) throw Error(std::string(who) + ": run mhx_sdbg_unitigs on this index first");
    g = dev_sdbg(c, info, who);
    auto it = c->results.find(MHX_BUF_UNITIG_VERTICES);
    if (it == c->results.end() || !it->second.p || it->second.used != c->ut_nv * sizeof(mhx_unitig_vertex))
      throw Error(std::string(who) + ": run mhx_sdbg_unitigs on this index first");
    // the owner map and the flags live in workspaces (and the owner map is made from the edge ranking's): whoever frees the
    // workspaces (mhx_trim) drops ut_ready; checked here once more so that a stale state is an error, never a read of fresh memory
    if (c->ut_owner ? !c->work.count("uc_owner") || !c->work.count("uc_mark") : !c->work.count("ut_rank"))
      throw Error(std::string(who) + ": run mhx_sdbg_unitigs on this index first");
    u.nv = c->ut_nv;
    u.vtx = it->second.as<mhx_unitig_vertex>();
    cnt = c->ws("uc_count", 64).as<unsigned long long>();
    u.own = c->ws("uc_owner", g.n * 4 + 64).as<uint32_t>();
    const bool fresh = !c->ut_owner;
    u.mark = c->ws("uc_mark", u.nv * 4 + 64).as<uint32_t>();
    if (fresh) {
      // the edge ranking of mhx_sdbg_unitigs is still in its workspace: every edge knows its chain head, a begin edge
      uint32_t *hv = c->ws("uc_head_vid", g.n * 4 + 64).as<uint32_t>();
      const Rk *rk = c->ws("ut_rank", g.n * sizeof(Rk) + 64).as<Rk>();
      MHX_HIP(hipMemsetAsync(hv, 0xff, g.n * 4 + 4, st));
      MHX_HIP(hipMemsetAsync(u.mark, 0, u.nv * 4 + 4, st));
      if (u.nv) hipLaunchKernelGGL(k_uc_head_vid, grid(u.nv), dim3(256), 0, st, u.vtx, u.nv, g.n, hv);
      if (g.n) MHX_LAUNCH(c, "clean_owner", (double)g.n * 44, hipLaunchKernelGGL(k_uc_own_init, grid(g.n), dim3(256), 0, st, g, rk, hv, u.own));
      MHX_HIP(hipGetLastError());
      c->ut_owner = true;
    }
  }
  uint64_t read_count(int i = 0) {
    unsigned long long h = 0;
    MHX_HIP(hipMemcpyAsync(&h, cnt + i, 8, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipStreamSynchronize(st));
    return (uint64_t)h;
  }

  // UnitigGraph::Refresh(set_changed)
  void refresh(bool set_changed = false) {
    const uint64_t nv = u.nv, n = g.n, nn = 2 * nv;
    if (!nv) return;
    c->ut_text_fresh = false;
    uint64_t *inv = c->ws("uc_inv", nn * 2 * 8 + 64).as<uint64_t>();
    MHX_HIP(hipMemsetAsync(cnt, 0, 16, st));
    MHX_LAUNCH(c, "clean_disconnect", (double)nv * 96, hipLaunchKernelGGL(k_uc_disc_plan, grid(nv), dim3(256), 0, st, g, u, inv, cnt + 1));
    hipLaunchKernelGGL(k_uc_disc_apply, grid(4 * nv), dim3(256), 0, st, g.invalid, inv, 4 * nv);
    MHX_LAUNCH(c, "clean_delete", (double)n * 5, hipLaunchKernelGGL(k_uc_delete_edges, grid(n), dim3(256), 0, st, g, u));
    // links between the (vertex, strand) nodes and their ranking
    uint64_t *succ = c->ws("uc_succ", nn * 8 + 64).as<uint64_t>();
    uint64_t *pred = c->ws("uc_pred", nn * 8 + 64).as<uint64_t>();
    uint64_t *lab = c->ws("uc_label", nn * 8 + 64).as<uint64_t>();
    Ranker rr;
    rr.c = c;
    rr.stat = "clean_rank";
    rr.rk = c->ws("uc_rank", nn * sizeof(Rk) + 64).as<Rk>();
    rr.nx = c->ws("uc_next", nn * sizeof(Rk) + 64).as<Rk>();
    rr.list[0] = c->ws("uc_list0", nn * 8 + 64).as<uint64_t>();
    rr.list[1] = c->ws("uc_list1", nn * 8 + 64).as<uint64_t>();
    rr.cnt = cnt;
    MHX_HIP(hipMemsetAsync(pred, 0xff, nn * 8 + 8, st));
    MHX_HIP(hipMemsetAsync(lab, 0xff, nn * 8 + 8, st));
    MHX_LAUNCH(c, "clean_links", (double)nn * 64, hipLaunchKernelGGL(k_uc_links, grid(nn), dim3(256), 0, st, g, u, succ));
    hipLaunchKernelGGL(k_ut_pred, grid(nn), dim3(256), 0, st, succ, nn, pred);
    if (read_count(1)) throw Error("unitig Refresh: a trimmed vertex has no inner edge to end at");
    MHX_HIP(hipMemsetAsync(cnt, 0, 8, st));
    hipLaunchKernelGGL(k_uc_rank_init, grid(nn), dim3(256), 0, st, u, pred, (const uint64_t *)nullptr, nn, lab, rr.rk, rr.list[0], cnt);
    MHX_HIP(hipGetLastError());
    const uint64_t n_cyc = rr.jump_rounds(kSum, rr.count(), 128);
    if (n_cyc) {
      const uint64_t *cyc = rr.keep_cycles(c->ws("uc_list2", n_cyc * 8 + 64).as<uint64_t>());
      rr.cycle_minima(cyc, n_cyc, pred);
      MHX_HIP(hipMemsetAsync(cnt, 0, 8, st));
      rr.cur = 0;
      hipLaunchKernelGGL(k_uc_rank_init, grid(n_cyc), dim3(256), 0, st, u, pred, cyc, n_cyc, lab, rr.rk, rr.list[0], cnt);
      MHX_HIP(hipGetLastError());
      if (rr.jump_rounds(kSum, rr.count(), 128)) throw Error("unitig Refresh: a cycle without a cut");
    }
    // survivors, their new ids and records
    uint32_t *alive = c->ws("uc_alive", nv * 4 + 64).as<uint32_t>();
    uint32_t *rep = c->ws("uc_rep", nv * 4 + 64).as<uint32_t>();
    uint64_t *newid = c->ws("uc_newid", (nv + 2) * 8).as<uint64_t>();
    mhx_unitig_vertex *tmp = c->ws("uc_vtx", nv * sizeof(mhx_unitig_vertex) + 64).as<mhx_unitig_vertex>();
    MHX_LAUNCH(c, "clean_merge", (double)nv * 96, hipLaunchKernelGGL(k_uc_resolve, grid(nv), dim3(256), 0, st, u, succ, pred, rr.rk, lab, alive, rep));
    exclusive_scan_u32_u64(c, alive, newid, nv, newid + nv);
    MHX_LAUNCH(c, "clean_merge", (double)nv * 160,
               hipLaunchKernelGGL(k_uc_write, grid(nv), dim3(256), 0, st, u, succ, pred, rr.rk, lab, alive, newid,
                                  set_changed ? MHX_UNITIG_CHANGED : 0u, tmp));
    MHX_LAUNCH(c, "clean_owner", (double)n * 12, hipLaunchKernelGGL(k_uc_own_rename, grid(n), dim3(256), 0, st, u.own, n, nv, rep, newid));
    uint64_t nv_new = 0;
    MHX_HIP(hipMemcpyAsync(&nv_new, newid + nv, 8, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipStreamSynchronize(st));
    if (nv_new > nv) throw Error("unitig Refresh: more survivors than vertices");
    MHX_HIP(hipMemcpyAsync(u.vtx, tmp, nv_new * sizeof(mhx_unitig_vertex), hipMemcpyDeviceToDevice, st));
    MHX_HIP(hipMemsetAsync(u.mark, 0, nv * 4, st));
    u.nv = c->ut_nv = nv_new;
    c->results[MHX_BUF_UNITIG_VERTICES].used = nv_new * sizeof(mhx_unitig_vertex);
  }

  // RemoveLocalLowDepth: one marking pass, one host read of both words, and a Refresh only when something was deleted
  bool low_depth(double min_depth, uint32_t max_len, uint32_t local_width, double local_ratio, bool mark_changed, uint64_t *n_removed) {
    *n_removed = 0;
    if (!u.nv) return false;
    MHX_HIP(hipMemsetAsync(cnt, 0, 16, st));
    MHX_LAUNCH(c, "clean_low_depth", (double)u.nv * 240,
               hipLaunchKernelGGL(k_uc_low_depth, grid(u.nv), dim3(256), 0, st, g, u, min_depth, max_len, local_width, local_ratio, cnt));
    unsigned long long h[2] = {0, 0};
    MHX_HIP(hipMemcpyAsync(h, cnt, 16, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipStreamSynchronize(st));
    if (h[0]) refresh(mark_changed);
    *n_removed = (uint64_t)h[0];
    return h[1] != 0;
  }

  // the text of the vertex table as it is now: MHX_BUF_UNITIG_SEQ / _OFFSET are those of the last finish (or of
  // mhx_sdbg_unitigs) and stay good until a Refresh runs; a mid-run finish rebuilds them (and clobbers cnt)
  void need_text() {
    if (c->ut_text_fresh) return;
    mhx_unitig_result r;
    unitig_finish(c, info, &r);
    ++c->ub_stats[3];
  }
  // BaseBubbleRemover::PopBubbles; sim <= 0: NaiveBubbleRemover's checker, else ComplexBubbleRemover's (bubble_remover.cpp:154-170)
  void pop_bubbles(uint32_t max_len, double sim, double careful, bool mark_changed, uint64_t *n_removed, uint64_t *n_records) {
    *n_removed = *n_records = 0;
    for (uint64_t &x : c->ub_stats) x = 0;
    c->result(MHX_BUF_UNITIG_BUBBLE_REC, 0);
    c->result(MHX_BUF_UNITIG_BUBBLE_SEQ, 0);
    const bool complex_mode = sim > 0, want_records = careful >= 0;
    if (complex_mode && (double)max_len * (1 - sim) < 1) return;  // the reference returns before its Refresh
    const uint64_t nv = u.nv, nn = 2 * nv;
    if (!nv) return;
    if (complex_mode) {
      const uint64_t longest = (uint64_t)max_len + g.k;
      if (longest > kSimMaxLen || (double)longest * (1 - sim) >= (double)(kSimMaxIndel + 1))
        throw Error("unitig_pop_bubbles: max_len and similarity are beyond the cap of the similarity kernel (MHX_SIM_MAX_LEN, MHX_SIM_MAX_INDEL)");
    }
    const BubArgs a{max_len, g.k, complex_mode ? sim : 0.0, want_records ? careful : -1.0};
    BubBuf bb{nullptr, nullptr, nullptr, nullptr};
    uint64_t *cand = nullptr;
    if (complex_mode || want_records) {
      bb.mid = c->ws("ub_mid", nn * 16 + 64).as<uint32_t>();
      bb.right = c->ws("ub_right", nn * 4 + 64).as<uint32_t>();
      bb.deg = c->ws("ub_deg", nn * 4 + 64).as<uint32_t>();
      bb.rec_n = c->ws("ub_rec_n", nn * 4 + 64).as<uint32_t>();
    }
    if (complex_mode) cand = c->ws("ub_cand", nn * 8 + 64).as<uint64_t>();
    MHX_HIP(hipMemsetAsync(cnt, 0, 32, st));
    MHX_LAUNCH(c, "clean_bubbles", (double)nn * 300, hipLaunchKernelGGL(k_uc_bubble_find, grid(nn), dim3(256), 0, st, g, u, a, bb, cand, cnt));
    unsigned long long h[4] = {0, 0, 0, 0};
    MHX_HIP(hipMemcpyAsync(h, cnt, 32, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipStreamSynchronize(st));
    uint64_t removed = h[0];
    const uint64_t n_cand = complex_mode ? h[1] : 0;
    if (n_cand) {
      c->ub_stats[0] = n_cand;
      need_text();
      const char *text = c->results[MHX_BUF_UNITIG_SEQ].as<char>();
      const uint64_t *off = c->results[MHX_BUF_UNITIG_OFFSET].as<uint64_t>();
      const uint64_t n_pairs = 3 * n_cand;
      SimPair *pairs = c->ws("ub_pairs", n_pairs * sizeof(SimPair) + 64).as<SimPair>();
      double *score = c->ws("ub_score", n_pairs * 8 + 64).as<double>();
      MHX_HIP(hipMemsetAsync(cnt, 0, 32, st));
      hipLaunchKernelGGL(k_uc_bubble_pairs, grid(n_pairs), dim3(256), 0, st, bb, cand, n_cand, off, pairs);
      const unsigned blocks = (unsigned)std::min<uint64_t>(n_pairs, 1u << 20);
      MHX_LAUNCH(c, "clean_similarity", (double)n_pairs * 2 * (max_len + g.k),
                 hipLaunchKernelGGL(k_uc_similarity, dim3(blocks), dim3(64), 0, st, text, pairs, n_pairs, 1 - sim, score));
      MHX_LAUNCH(c, "clean_bubbles", (double)n_cand * 100,
                 hipLaunchKernelGGL(k_uc_bubble_mark, grid(n_cand), dim3(256), 0, st, u, a, bb, cand, n_cand, score, cnt));
      MHX_HIP(hipMemcpyAsync(h, cnt, 32, hipMemcpyDeviceToHost, st));
      MHX_HIP(hipStreamSynchronize(st));
      removed = h[0];
      c->ub_stats[1] = h[2];
      c->ub_stats[2] = h[3];
    }
    if (want_records && removed) {  // (a record needs a popped bubble, and its flags are among this pass's)
      uint64_t *rec_off = c->ws("ub_rec_off", (nn + 2) * 8).as<uint64_t>();
      exclusive_scan_u32_u64(c, bb.rec_n, rec_off, nn, rec_off + nn);
      uint64_t n_rec = 0;
      MHX_HIP(hipMemcpyAsync(&n_rec, rec_off + nn, 8, hipMemcpyDeviceToHost, st));
      MHX_HIP(hipStreamSynchronize(st));
      if (n_rec) {
        need_text();  // before the Refresh: the records are the vertices as the pass saw them
        const char *text = c->results[MHX_BUF_UNITIG_SEQ].as<char>();
        const uint64_t *off = c->results[MHX_BUF_UNITIG_OFFSET].as<uint64_t>();
        mhx_bubble_record *rec = c->result(MHX_BUF_UNITIG_BUBBLE_REC, n_rec * sizeof(mhx_bubble_record)).as<mhx_bubble_record>();
        uint64_t *rec_len = c->ws("ub_rec_len", n_rec * 8 + 64).as<uint64_t>();
        uint64_t *rec_pos = c->ws("ub_rec_pos", (n_rec + 2) * 8).as<uint64_t>();
        hipLaunchKernelGGL(k_uc_bubble_records, grid(nn), dim3(256), 0, st, u, a, bb, rec_off, rec, rec_len);
        MHX_HIP(hipGetLastError());
        exclusive_scan_u64(c, rec_len, rec_pos, n_rec, rec_pos + n_rec);
        uint64_t n_chars = 0;
        MHX_HIP(hipMemcpyAsync(&n_chars, rec_pos + n_rec, 8, hipMemcpyDeviceToHost, st));
        MHX_HIP(hipStreamSynchronize(st));
        char *out = c->result(MHX_BUF_UNITIG_BUBBLE_SEQ, n_chars).as<char>();
        MHX_LAUNCH(c, "clean_bubbles", (double)n_chars * 2,
                   hipLaunchKernelGGL(k_uc_bubble_text, dim3((unsigned)std::min<uint64_t>(n_rec, 1u << 16)), dim3(256), 0, st, text, off, rec_pos, n_rec, rec, out));
        *n_records = n_rec;
      }
    }
    // The reference refreshes after every pass.  With no flag set a Refresh changes nothing: the flag words are zero between
    // calls (every Refresh clears them), so nothing is trimmed or deleted, and every vertex is a maximal simple path already
    // (the constructor and every earlier Refresh leave them so, and no edge changed since), so nothing merges and no
    // vertex gets the is_changed mark.  low_depth skips it in the same way.
    if (removed) refresh(mark_changed);
    *n_removed = removed;
  }
};

}  // namespace

int unitig_disconnect_weak_links(mhx_ctx *c, const mhx_sdbg_index_info *info, double ratio, uint64_t *n_flagged) {
  Clean k(c, info, "unitig_disconnect_weak_links");
  if (n_flagged) *n_flagged = 0;
  if (!k.u.nv) return 0;
  MHX_HIP(hipMemsetAsync(k.cnt, 0, 8, k.st));
  MHX_LAUNCH(c, "clean_weak_links", (double)k.u.nv * 200, hipLaunchKernelGGL(k_uc_weak, Clean::grid(k.u.nv), dim3(256), 0, k.st, k.g, k.u, ratio, k.cnt));
  const uint64_t n = k.read_count();
  k.refresh();
  if (n_flagged) *n_flagged = n;
  return 0;
}

int unitig_remove_tips(mhx_ctx *c, const mhx_sdbg_index_info *info, uint32_t max_tip_len, uint64_t *n_removed) {
  Clean k(c, info, "unitig_remove_tips");
  if (n_removed) *n_removed = 0;
  uint64_t total = 0;
  // tip_remover.cpp:10-11 as it is: 2, 4, 8, ... while below max_tip_len (max_tip_len itself is never a threshold)
  for (uint32_t thre = 2; thre < max_tip_len; thre = std::min(thre * 2, max_tip_len)) {
    if (k.u.nv) {
      MHX_HIP(hipMemsetAsync(k.cnt, 0, 8, k.st));
      MHX_LAUNCH(c, "clean_tips", (double)k.u.nv * 200, hipLaunchKernelGGL(k_uc_tips, Clean::grid(k.u.nv), dim3(256), 0, k.st, k.g, k.u, thre, k.cnt));
      total += k.read_count();
    }
    k.refresh();
  }
  if (n_removed) *n_removed = total;
  return 0;
}

int unitig_remove_local_low_depth(mhx_ctx *c, const mhx_sdbg_index_info *info, double min_depth, uint32_t max_len, uint32_t local_width,
                                  double local_ratio, int mark_changed, uint64_t *n_removed, int *is_changed) {
  Clean k(c, info, "unitig_remove_local_low_depth");
  uint64_t n = 0;
  const bool chg = k.low_depth(min_depth, max_len, local_width, local_ratio, mark_changed != 0, &n);
  if (n_removed) *n_removed = n;
  if (is_changed) *is_changed = chg ? 1 : 0;
  return 0;
}

int unitig_iterate_local_low_depth(mhx_ctx *c, const mhx_sdbg_index_info *info, double min_depth, uint32_t max_len, uint32_t local_width,
                                   double local_ratio, int mark_changed, uint64_t *n_removed) {
  Clean k(c, info, "unitig_iterate_local_low_depth");
  uint64_t total = 0;
  // low_depth_remover.cpp:88-102: until a pass changes nothing, min_depth * 1.1 each time (host double), below kMaxMul
  while (min_depth < 65535.0) {
    uint64_t n = 0;
    if (!k.low_depth(min_depth, max_len, local_width, local_ratio, mark_changed != 0, &n)) break;
    total += n;
    min_depth *= 1.1;
  }
  if (n_removed) *n_removed = total;
  return 0;
}

int unitig_finish(mhx_ctx *c, const mhx_sdbg_index_info *info, mhx_unitig_result *out) {
  Clean k(c, info, "unitig_finish");
  MHX_HIP(hipMemsetAsync(k.cnt, 0, 8, k.st));
  if (k.u.nv)
    MHX_LAUNCH(c, "clean_flags", (double)k.u.nv * 64, hipLaunchKernelGGL(k_uc_final_flags, Clean::grid(k.u.nv), dim3(256), 0, k.st, k.g, k.u.vtx, k.u.nv, k.cnt));
  const uint64_t n_loop = k.read_count();
  sdbg_unitig_text(c, info, k.u.nv, n_loop, out);
  c->ut_text_fresh = true;
  return 0;
}

int unitig_remove_low_depth(mhx_ctx *c, const mhx_sdbg_index_info *info, double min_depth, uint64_t *n_removed) {
  Clean k(c, info, "unitig_remove_low_depth");
  if (n_removed) *n_removed = 0;
  if (!k.u.nv) return 0;
  MHX_HIP(hipMemsetAsync(k.cnt, 0, 8, k.st));
  MHX_LAUNCH(c, "clean_low_depth", (double)k.u.nv * 40,
             hipLaunchKernelGGL(k_uc_remove_low_depth, Clean::grid(k.u.nv), dim3(256), 0, k.st, k.u, min_depth, k.cnt));
  const uint64_t n = k.read_count();
  if (n) k.refresh(false);  // (with no flag set a Refresh changes nothing: see Clean::pop_bubbles)
  if (n_removed) *n_removed = n;
  return 0;
}

int unitig_pop_bubbles(mhx_ctx *c, const mhx_sdbg_index_info *info, uint32_t max_len, double similarity, double careful_threshold, int mark_changed,
                       uint64_t *n_removed, uint64_t *n_records) {
  Clean k(c, info, "unitig_pop_bubbles");
  uint64_t removed = 0, records = 0;
  k.pop_bubbles(max_len, similarity, careful_threshold, mark_changed != 0, &removed, &records);
  if (n_removed) *n_removed = removed;
  if (n_records) *n_records = records;
  return 0;
}

int unitig_similarity(mhx_ctx *c, const char *a, uint32_t n, const char *b, uint32_t m, double sim, double *out) {
  if (!out || (n && !a) || (m && !b)) throw Error("unitig_similarity: bad arguments");
  if (!(sim > 0 && sim <= 1)) throw Error("unitig_similarity: the similarity must be in (0, 1]");
  const uint32_t mx = std::max(n, m);
  if (mx > kSimMaxLen) throw Error("unitig_similarity: a string is longer than MHX_SIM_MAX_LEN");
  if ((int)((double)mx * (1 - sim)) > kSimMaxIndel) throw Error("unitig_similarity: max_indel is beyond MHX_SIM_MAX_INDEL");
  hipStream_t st = c->stream;
  char *text = c->ws("ub_sim_text", (size_t)n + m + 64).as<char>();
  SimPair *pair = c->ws("ub_pairs", sizeof(SimPair) + 64).as<SimPair>();
  double *score = c->ws("ub_score", 64).as<double>();
  const SimPair q{0, n, n, m};
  if (n) MHX_HIP(hipMemcpyAsync(text, a, n, hipMemcpyHostToDevice, st));
  if (m) MHX_HIP(hipMemcpyAsync(text + n, b, m, hipMemcpyHostToDevice, st));
  MHX_HIP(hipMemcpyAsync(pair, &q, sizeof q, hipMemcpyHostToDevice, st));
  MHX_LAUNCH(c, "clean_similarity", (double)n + m, hipLaunchKernelGGL(k_uc_similarity, dim3(1), dim3(64), 0, st, text, pair, (uint64_t)1, 1 - sim, score));
  MHX_HIP(hipMemcpyAsync(out, score, 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // namespace mhx
