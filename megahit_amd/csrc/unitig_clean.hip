// Graph cleaning on the device-resident unitig graph: what `assemble --bubble_level 0 --prune_level 0..2 --cleaning_rounds N`
// does between UnitigGraph::UnitigGraph and the last OutputContigs (reference src/main_assemble.cpp:182-301) —
//   DisconnectWeakLinks  assembly/weak_link_remover.cpp
//   RemoveTips           assembly/tip_remover.cpp (on the unitig graph, not the SdBG-level one of sdbg_tips.hip)
//   RemoveLocalLowDepth, IterateLocalLowDepth  assembly/low_depth_remover.cpp:10-102 (prune levels 1 and 2)
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

  Clean(mhx_ctx *c_, const mhx_sdbg_index_info *info, const char *who) : c(c_), st(c_->stream) {
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
  return sdbg_unitig_text(c, info, k.u.nv, n_loop, out);
}

}  // namespace mhx
