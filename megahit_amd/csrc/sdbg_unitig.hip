// The unitig graph and its contig text on the device-resident SdBG — what `assemble` does after tip trimming:
// UnitigGraph::UnitigGraph (reference src/assembly/unitig_graph.cpp:13-138) and the strings of OutputContigs
// (contig_output.cpp:62-119 over UnitigGraph::VertexToDNAString, unitig_graph.cpp:357-394), on the buffers that
// mhx_sdbg_build_index left in HBM with MHX_BUF_SDBG_INVALID as mhx_sdbg_remove_tips left it.
//
// The reference walks every simple path serially over rank/select.  Here:
//   links     one thread per edge: succ[i] = NextSimplePathEdge(i); pred[succ[i]] = i (the two agree by construction:
//             succ[i] = j exactly when PrevSimplePathEdge(j) = i).  The only per-edge rank/select navigation.
//   ranking   pointer jumping (Wyllie) over pred with compaction of the still-active edges: every chain edge learns its
//             chain head, its rank from the head and the multiplicity sum head..itself in ceil(log2 L) rounds.  A round
//             in which no edge finishes leaves only cycle edges (a chain edge of rank r >= 2^(t-1) that is still active
//             has a predecessor of rank in [2^(t-1), 2^t) that finishes in round t).  The cycles' minimum edges then
//             come from min-propagation over the same jumps, each cycle is cut at the start its vertex needs and ranked
//             once more.
//   vertices  chains: kept at the tail t when t <= the tail of the reverse-complement chain (= RC(head)); loops: kept at
//             the cycle minimum M when M <= the minimum of the reverse-complement cycle.  Ids come from bitmaps of those
//             keys + a popcount prefix (chains ascending by tail, then loops ascending by M: the reference's order on
//             one thread), without a sort.
//   text      ToUniqueFormat picks the strand that begins at min(b, rb); every edge of that strand's chain writes its
//             character at offset[v] + k + rank, one thread per vertex writes GetLabel(begin).
#include "sdbg_nav.h"
#include "unitig_rank.h"

namespace mhx {

namespace {

__global__ __launch_bounds__(256) void k_ut_links(DevSdbg g, uint64_t *__restrict__ succ) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  succ[i] = sd_valid(g, i) ? sd_next_simple(g, i) : kNull;
}
// first ranking: every valid edge; roots (no predecessor) are final at once
__global__ __launch_bounds__(256) void k_ut_rank_init(DevSdbg g, const uint64_t *__restrict__ pred, Rk *__restrict__ rk, uint64_t *__restrict__ list,
                                                     unsigned long long *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool take = false;
  if (i < g.n && sd_valid(g, i)) {
    const uint64_t p = pred[i];
    rk[i] = Rk{p, g.mul[i], p == kNull ? 0ull : 1ull, i};
    take = p != kNull;
  }
  push_list(take, i, list, cnt);
}
// each cycle's minimum edge x (head := the cycle minimum): the cycle pair is kept at x when x <= the minimum of the reverse
// complement cycle (reference: the loop pass meets the pair first at its smaller minimum; a self-complementary cycle is
// its own pair).  Cuts: b = succ[x] in this cycle and rb = RC(x) in the reverse-complement one (one cut, at
// min(b, rb), when the cycle is its own reverse complement) — the output strand (ToUniqueFormat) begins at min(b, rb).
__global__ __launch_bounds__(256) void k_ut_cyc_cut(DevSdbg g, const uint64_t *__restrict__ succ, const uint64_t *__restrict__ list, uint64_t n_cyc,
                                                    Rk *__restrict__ rk, unsigned long long *__restrict__ cut, unsigned long long *__restrict__ loop_key,
                                                    unsigned long long *__restrict__ out_head) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_cyc) return;
  const uint64_t x = list[t];
  if (rk[x].val != x) return;
  const uint64_t r = sd_edge_rc(g, x);
  const uint64_t mr = r == kNull ? kNull : rk[r].val;
  if (x > mr) return;  // the reverse-complement cycle's minimum thread cuts both
  const uint64_t b = succ[x];
  bit_set(loop_key, x);
  if (mr == x) {
    bit_set(cut, b < r ? b : r);
  } else {
    bit_set(cut, b);
    if (r != kNull) bit_set(cut, r);
  }
  bit_set(out_head, b < r ? b : r);
}
// second ranking of the cycle edges, cut at the starts above
__global__ __launch_bounds__(256) void k_ut_cyc_rank_init(DevSdbg g, const uint64_t *__restrict__ pred, const uint64_t *__restrict__ cyc, uint64_t n_cyc,
                                                         const unsigned long long *__restrict__ cut, Rk *__restrict__ rk, uint64_t *__restrict__ list,
                                                         unsigned long long *__restrict__ cnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool take = false;
  uint64_t i = 0;
  if (t < n_cyc) {
    i = cyc[t];
    const bool start = sd_bit(cut, i);
    rk[i] = Rk{start ? kNull : pred[i], g.mul[i], start ? 0ull : 1ull, i};
    take = !start;
  }
  push_list(take, i, list, cnt);
}
// chain tails: kept when t <= RC(head) (the tail of the reverse-complement chain: the reference's pass meets the pair at
// its smaller tail; a palindromic chain is its own pair).  rc_tail[t] = RC(t) for the vertex kernel.
__global__ __launch_bounds__(256) void k_ut_chain_keys(DevSdbg g, const uint64_t *__restrict__ succ, const Rk *__restrict__ rk, unsigned long long *__restrict__ chain_key,
                                                       unsigned long long *__restrict__ out_head, uint64_t *__restrict__ rc_tail) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= g.n || !sd_valid(g, t) || succ[t] != kNull) return;
  const uint64_t h = rk[t].head;
  const uint64_t re = sd_edge_rc(g, h);
  if (t > re) return;
  const uint64_t rb = sd_edge_rc(g, t);
  rc_tail[t] = rb;
  bit_set(chain_key, t);
  bit_set(out_head, h < rb ? h : rb);
}
__global__ __launch_bounds__(256) void k_ut_word_pop(const unsigned long long *__restrict__ bits, uint64_t n_words, uint32_t *__restrict__ cnt) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n_words) cnt[w] = (uint32_t)__builtin_popcountll(bits[w]);
}
__device__ __forceinline__ uint64_t bit_rank(const unsigned long long *bits, const uint64_t *woff, uint64_t x) {  // set bits before x
  return woff[x >> 6] + (uint64_t)__builtin_popcountll(bits[x >> 6] & ((1ull << (x & 63)) - 1));
}
// one thread per word of the key bitmaps: vertex v = id of the key; fields as the reference's constructor leaves them
__global__ __launch_bounds__(256) void k_ut_vertices(DevSdbg g, const uint64_t *__restrict__ succ, const uint64_t *__restrict__ pred, const Rk *__restrict__ rk,
                                                     const unsigned long long *__restrict__ key, const uint64_t *__restrict__ key_off, uint64_t id0, bool loops,
                                                     const uint64_t *__restrict__ rc_tail, uint64_t n_words, const unsigned long long *__restrict__ out_head,
                                                     const uint64_t *__restrict__ oh_off, mhx_unitig_vertex *__restrict__ vtx, uint64_t *__restrict__ out_vid,
                                                     uint64_t *__restrict__ len) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  uint64_t v = id0 + key_off[w];
  for (unsigned long long m = key[w]; m; m &= m - 1, ++v) {
    const uint64_t x = w * 64 + (uint64_t)__builtin_ctzll(m);
    mhx_unitig_vertex o;
    if (!loops) {  // unitig_graph.cpp:77-79
      const uint64_t h = rk[x].head;
      o.b = h;
      o.e = x;
      o.rb = rc_tail[x];
      o.re = sd_edge_rc(g, h);
      o.total_depth = rk[x].val;
      o.length = (uint32_t)(rk[x].d + 1);
      const bool isolated = sd_outdegree(g, x) == 0 && (o.re == kNull || sd_outdegree(g, o.re) == 0);
      o.flags = (h == o.rb ? MHX_UNITIG_PALINDROME : 0u) | (isolated ? MHX_UNITIG_STANDALONE : 0u);
    } else {  // unitig_graph.cpp:108-113: depth = mul(M) + the cycle's sum
      const uint64_t b = succ[x], rb = sd_edge_rc(g, x);
      o.b = b;
      o.e = x;
      o.rb = rb;
      o.re = sd_edge_rc(g, b);
      const bool self_rc = rb != kNull && rk[rb].head == rk[b].head;  // one cycle, cut once
      const uint64_t tail = pred[self_rc ? (b < rb ? b : rb) : b];
      o.total_depth = rk[tail].val + g.mul[x];
      o.length = (uint32_t)(rk[tail].d + 1);
      o.flags = MHX_UNITIG_LOOP | MHX_UNITIG_STANDALONE | (b == rb ? MHX_UNITIG_PALINDROME : 0u);
    }
    vtx[v] = o;
    const uint64_t ob = o.b < o.rb ? o.b : o.rb;  // ToUniqueFormat
    out_vid[bit_rank(out_head, oh_off, ob)] = v;
    len[v] = (uint64_t)g.k + o.length;
  }
}
// every edge of an output strand: its character at offset[v] + k + rank
__global__ __launch_bounds__(256) void k_ut_text(DevSdbg g, const Rk *__restrict__ rk, const unsigned long long *__restrict__ out_head, const uint64_t *__restrict__ oh_off,
                                                 const uint64_t *__restrict__ out_vid, const uint64_t *__restrict__ off, char *__restrict__ seq) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n || !sd_valid(g, i)) return;
  const Rk r = rk[i];
  if (!sd_bit(out_head, r.head)) return;
  const uint64_t v = out_vid[bit_rank(out_head, oh_off, r.head)];
  unsigned c = sd_w(g, i);
  if (c > 4) c -= 4;
  const uint64_t pos = off[v] + g.k + r.d;
  if (pos < off[v + 1]) seq[pos] = "ACGT"[c - 1];
}
// GetLabel of every vertex's output begin
__global__ __launch_bounds__(256) void k_ut_labels(DevSdbg g, const mhx_unitig_vertex *__restrict__ vtx, uint64_t nv, const uint64_t *__restrict__ off, char *__restrict__ seq) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const uint64_t b = vtx[v].b < vtx[v].rb ? vtx[v].b : vtx[v].rb;
  uint8_t lab[MHX_MAX_K];
  sd_label(g, b, lab);
  char *o = seq + off[v];
  for (uint32_t i = 0; i < g.k; ++i) o[i] = "ACGT"[lab[i] - 1];
}
__global__ void k_ut_flag_count(const mhx_unitig_vertex *__restrict__ vtx, uint64_t nv, unsigned long long *__restrict__ cnt) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t f = v < nv ? vtx[v].flags : 0u;
  const uint64_t pal = __ballot((f & MHX_UNITIG_PALINDROME) && !(f & MHX_UNITIG_LOOP)), sa = __ballot(f & MHX_UNITIG_STANDALONE);
  if (lane_id() == 0) {  // one atomic per wavefront
    if (pal) atomicAdd(&cnt[0], (unsigned long long)__builtin_popcountll(pal));
    if (sa) atomicAdd(&cnt[1], (unsigned long long)__builtin_popcountll(sa));
  }
}

// the cleaned vertex table's part in the text (sdbg_unitig_text): every vertex's output strand begins at min(b, rb); a loop's
// cycle is cut there; len[v] = k + length
__global__ __launch_bounds__(256) void k_ut_tab_heads(const mhx_unitig_vertex *__restrict__ vtx, uint64_t nv, uint32_t k, unsigned long long *__restrict__ out_head,
                                                      unsigned long long *__restrict__ cut, uint64_t *__restrict__ len) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const uint64_t ob = vtx[v].b < vtx[v].rb ? vtx[v].b : vtx[v].rb;
  bit_set(out_head, ob);
  if (vtx[v].flags & MHX_UNITIG_LOOP) bit_set(cut, ob);
  len[v] = (uint64_t)k + vtx[v].length;
}
__global__ __launch_bounds__(256) void k_ut_tab_vid(const mhx_unitig_vertex *__restrict__ vtx, uint64_t nv, const unsigned long long *__restrict__ out_head,
                                                    const uint64_t *__restrict__ oh_off, uint64_t *__restrict__ out_vid) {
  const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  out_vid[bit_rank(out_head, oh_off, vtx[v].b < vtx[v].rb ? vtx[v].b : vtx[v].rb)] = v;
}

// the workspaces of one edge-level ranking
struct EdgeRank {
  uint64_t n, nw;
  uint64_t *succ, *pred;
  Ranker rr;
  EdgeRank(mhx_ctx *c, uint64_t n_) : n(n_), nw(div_ceil(n_, 64) + 1) {
    succ = c->ws("ut_succ", n * 8 + 64).as<uint64_t>();
    pred = c->ws("ut_pred", n * 8 + 64).as<uint64_t>();
    rr.c = c;
    rr.stat = "unitig_rank";
    rr.rk = c->ws("ut_rank", n * sizeof(Rk) + 64).as<Rk>();
    rr.nx = c->ws("ut_next", n * sizeof(Rk) + 64).as<Rk>();
    rr.list[0] = c->ws("ut_list0", n * 8 + 64).as<uint64_t>();
    rr.list[1] = c->ws("ut_list1", n * 8 + 64).as<uint64_t>();
    rr.cnt = c->ws("ut_count", 64).as<unsigned long long>();
  }
  // links + the first ranking; returns the cycle edges left (in rr.list[rr.cur])
  uint64_t chains(const DevSdbg &g) {
    mhx_ctx *c = rr.c;
    hipStream_t st = c->stream;
    MHX_HIP(hipMemsetAsync(pred, 0xff, n * 8 + 8, st));
    if (!n) return 0;
    MHX_LAUNCH(c, "unitig_links", (double)n * 16, hipLaunchKernelGGL(k_ut_links, Ranker::grid(n), dim3(256), 0, st, g, succ));
    hipLaunchKernelGGL(k_ut_pred, Ranker::grid(n), dim3(256), 0, st, succ, n, pred);
    MHX_HIP(hipMemsetAsync(rr.cnt, 0, 8, st));
    rr.cur = 0;
    hipLaunchKernelGGL(k_ut_rank_init, Ranker::grid(n), dim3(256), 0, st, g, pred, rr.rk, rr.list[0], rr.cnt);
    MHX_HIP(hipGetLastError());
    return rr.jump_rounds(kSum, rr.count(), 128);
  }
  // the cycle edges, set aside
  const uint64_t *keep_cycles(uint64_t n_cyc) { return rr.keep_cycles(rr.c->ws("ut_list2", n_cyc * 8 + 64).as<uint64_t>()); }
  // second ranking of the cycle edges, cut at the bits of `cut`; returns the edges of cycles without a cut
  uint64_t rank_cut_cycles(const DevSdbg &g, const uint64_t *cyc, uint64_t n_cyc, const unsigned long long *cut) {
    hipStream_t st = rr.c->stream;
    MHX_HIP(hipMemsetAsync(rr.cnt, 0, 8, st));
    rr.cur = 0;
    hipLaunchKernelGGL(k_ut_cyc_rank_init, Ranker::grid(n_cyc), dim3(256), 0, st, g, pred, cyc, n_cyc, cut, rr.rk, rr.list[0], rr.cnt);
    MHX_HIP(hipGetLastError());
    return rr.jump_rounds(kSum, rr.count(), 128);
  }
};

// offsets, text and flag counts of the vertex table in MHX_BUF_UNITIG_VERTICES, given every output strand's edges ranked from
// its head (rk) and the head -> vertex map (out_head / oh_off / out_vid)
void write_text(mhx_ctx *c, const DevSdbg &g, const Rk *rk, uint64_t nv, uint64_t n_loop, const uint64_t *len, const unsigned long long *out_head,
                const uint64_t *oh_off, const uint64_t *out_vid, unsigned long long *cnt, mhx_unitig_result *out) {
  hipStream_t st = c->stream;
  const uint64_t n = g.n;
  auto grid = Ranker::grid;
  const mhx_unitig_vertex *vtx = c->results[MHX_BUF_UNITIG_VERTICES].as<mhx_unitig_vertex>();
  uint64_t *off = c->result(MHX_BUF_UNITIG_OFFSET, (nv + 2) * 8).as<uint64_t>();
  c->results[MHX_BUF_UNITIG_OFFSET].used = (nv + 1) * 8;
  if (nv) exclusive_scan_u64(c, len, off, nv, off + nv);
  else MHX_HIP(hipMemsetAsync(off, 0, 8, st));
  uint64_t n_bases = 0;
  MHX_HIP(hipMemcpyAsync(&n_bases, off + nv, 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  char *seq = c->result(MHX_BUF_UNITIG_SEQ, n_bases + 64).as<char>();
  c->results[MHX_BUF_UNITIG_SEQ].used = n_bases;
  if (nv) {
    MHX_LAUNCH(c, "unitig_text", (double)n * 40 + (double)n_bases,
               hipLaunchKernelGGL(k_ut_text, grid(n), dim3(256), 0, st, g, rk, out_head, oh_off, out_vid, off, seq));
    MHX_LAUNCH(c, "unitig_labels", (double)nv * g.k, hipLaunchKernelGGL(k_ut_labels, grid(nv), dim3(256), 0, st, g, vtx, nv, off, seq));
  }
  MHX_HIP(hipMemsetAsync(cnt, 0, 16, st));
  if (nv) hipLaunchKernelGGL(k_ut_flag_count, grid(nv), dim3(256), 0, st, vtx, nv, cnt);
  unsigned long long fc[2] = {0, 0};
  MHX_HIP(hipMemcpyAsync(fc, cnt, 16, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  out->n_vertices = nv;
  out->n_loops = n_loop;
  out->n_palindromes = fc[0];
  out->n_standalone = fc[1];
  out->n_bases = n_bases;
}

}  // namespace

int sdbg_unitigs(mhx_ctx *c, const mhx_sdbg_index_info *info, mhx_unitig_result *out) {
  hipStream_t st = c->stream;
  const DevSdbg g = dev_sdbg(c, info, "sdbg_unitigs");
  c->ut_ready = c->ut_owner = c->ut_text_fresh = false;
  memset(out, 0, sizeof *out);
  auto grid = Ranker::grid;
  EdgeRank er(c, g.n);
  const uint64_t n = er.n, nw = er.nw;
  uint64_t *succ = er.succ, *pred = er.pred;
  Rk *rk = er.rr.rk;
  unsigned long long *cnt = er.rr.cnt;
  // bitmaps: chain keys, loop keys, output-strand heads, cycle cuts; per-word popcounts and their prefixes
  unsigned long long *bits = c->ws("ut_bits", 4 * nw * 8).as<unsigned long long>();
  unsigned long long *chain_key = bits, *loop_key = bits + nw, *out_head = bits + 2 * nw, *cut = bits + 3 * nw;
  uint32_t *wcnt = c->ws("ut_wcnt", nw * 4 + 64).as<uint32_t>();
  uint64_t *woff = c->ws("ut_woff", 3 * (nw + 2) * 8).as<uint64_t>();
  uint64_t *chain_off = woff, *loop_off = woff + (nw + 2), *oh_off = woff + 2 * (nw + 2);
  MHX_HIP(hipMemsetAsync(bits, 0, 4 * nw * 8, st));
  const uint64_t n_cyc = er.chains(g);
  if (n_cyc) {
    // the cycle edges: minimum by min-propagation, then cut and rank again
    const uint64_t *cyc = er.keep_cycles(n_cyc);
    er.rr.cycle_minima(cyc, n_cyc, pred);
    MHX_LAUNCH(c, "unitig_cycles", (double)n_cyc * 16,
               hipLaunchKernelGGL(k_ut_cyc_cut, grid(n_cyc), dim3(256), 0, st, g, succ, cyc, n_cyc, rk, cut, loop_key, out_head));
    if (er.rank_cut_cycles(g, cyc, n_cyc, cut)) throw Error("sdbg_unitigs: a cycle without a cut (is the graph its own reverse complement?)");
  }
  // chain keys (the reverse complements of chain ends: one EdgeReverseComplement per tail and per kept head)
  uint64_t *rc_tail = c->ws("ut_rc_tail", n * 8 + 64).as<uint64_t>();
  if (n)
    MHX_LAUNCH(c, "unitig_vertices", (double)n * 9,
               hipLaunchKernelGGL(k_ut_chain_keys, grid(n), dim3(256), 0, st, g, succ, rk, chain_key, out_head, rc_tail));
  uint64_t tot[3] = {0, 0, 0};
  uint64_t *offs[3] = {chain_off, loop_off, oh_off};
  unsigned long long *maps[3] = {chain_key, loop_key, out_head};
  for (int m = 0; m < 3; ++m) {
    hipLaunchKernelGGL(k_ut_word_pop, grid(nw), dim3(256), 0, st, maps[m], nw, wcnt);
    exclusive_scan_u32_u64(c, wcnt, offs[m], nw, offs[m] + nw + 1);
    MHX_HIP(hipMemcpyAsync(&tot[m], offs[m] + nw + 1, 8, hipMemcpyDeviceToHost, st));
  }
  MHX_HIP(hipStreamSynchronize(st));
  const uint64_t n_chain = tot[0], n_loop = tot[1], nv = n_chain + n_loop;
  if (tot[2] != nv) throw Error("sdbg_unitigs: output strands and vertices disagree (is the graph its own reverse complement?)");
  if (nv >= 0xfffffffeull)  // UnitigGraph::kMaxNumVertices (unitig_graph.h:19-20, unitig_graph.cpp:122-127)
    throw Error("Too many vertices in the unitig graph (" + std::to_string(nv) + " >= 4294967294), you may increase the kmer size to remove tons of erroneous kmers.");
  mhx_unitig_vertex *vtx = c->result(MHX_BUF_UNITIG_VERTICES, nv * sizeof(mhx_unitig_vertex) + 64).as<mhx_unitig_vertex>();
  c->results[MHX_BUF_UNITIG_VERTICES].used = nv * sizeof(mhx_unitig_vertex);
  uint64_t *len = c->ws("ut_len", nv * 8 + 64).as<uint64_t>();
  uint64_t *out_vid = c->ws("ut_out_vid", nv * 8 + 64).as<uint64_t>();
  if (nv) {
    MHX_LAUNCH(c, "unitig_vertices", (double)nv * 64,
               hipLaunchKernelGGL(k_ut_vertices, grid(nw), dim3(256), 0, st, g, succ, pred, rk, chain_key, chain_off, (uint64_t)0, false, rc_tail, nw,
                                  out_head, oh_off, vtx, out_vid, len));
    MHX_LAUNCH(c, "unitig_vertices", (double)nv * 64,
               hipLaunchKernelGGL(k_ut_vertices, grid(nw), dim3(256), 0, st, g, succ, pred, rk, loop_key, loop_off, n_chain, true, rc_tail, nw,
                                  out_head, oh_off, vtx, out_vid, len));
  }
  write_text(c, g, rk, nv, n_loop, len, out_head, oh_off, out_vid, cnt, out);
  c->ut_ready = c->ut_text_fresh = true;
  c->ut_edges = n;
  c->ut_nv = nv;
  return 0;
}

// Offsets, text and counts for the vertex table as the cleaning steps left it (unitig_clean.hip): the cleaned SdBG's maximal
// simple paths are exactly the vertices, so the edge-level ranking runs again and every chain is attached to the vertex whose
// output strand begins at its head.  Vertex order, length and depth are the table's.
int sdbg_unitig_text(mhx_ctx *c, const mhx_sdbg_index_info *info, uint64_t nv, uint64_t n_loop, mhx_unitig_result *out) {
  hipStream_t st = c->stream;
  const DevSdbg g = dev_sdbg(c, info, "unitig_finish");
  memset(out, 0, sizeof *out);
  auto grid = Ranker::grid;
  EdgeRank er(c, g.n);
  const uint64_t nw = er.nw;
  unsigned long long *bits = c->ws("ut_bits", 4 * nw * 8).as<unsigned long long>();
  unsigned long long *out_head = bits + 2 * nw, *cut = bits + 3 * nw;
  uint32_t *wcnt = c->ws("ut_wcnt", nw * 4 + 64).as<uint32_t>();
  uint64_t *oh_off = c->ws("ut_woff", 3 * (nw + 2) * 8).as<uint64_t>() + 2 * (nw + 2);
  const mhx_unitig_vertex *vtx = c->results[MHX_BUF_UNITIG_VERTICES].as<mhx_unitig_vertex>();
  uint64_t *len = c->ws("ut_len", nv * 8 + 64).as<uint64_t>();
  uint64_t *out_vid = c->ws("ut_out_vid", nv * 8 + 64).as<uint64_t>();
  MHX_HIP(hipMemsetAsync(bits, 0, 4 * nw * 8, st));
  if (nv) hipLaunchKernelGGL(k_ut_tab_heads, grid(nv), dim3(256), 0, st, vtx, nv, g.k, out_head, cut, len);
  const uint64_t n_cyc = er.chains(g);
  // cycles: the loops' output strands are cut at their begin; the other strand's cycle and the cycles of deleted loops have
  // no cut, stay unranked and belong to no vertex
  if (n_cyc) er.rank_cut_cycles(g, er.keep_cycles(n_cyc), n_cyc, cut);
  uint64_t n_heads = 0;
  hipLaunchKernelGGL(k_ut_word_pop, grid(nw), dim3(256), 0, st, out_head, nw, wcnt);
  exclusive_scan_u32_u64(c, wcnt, oh_off, nw, oh_off + nw + 1);
  MHX_HIP(hipMemcpyAsync(&n_heads, oh_off + nw + 1, 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  if (n_heads != nv) throw Error("unitig_finish: two vertices begin at one edge");
  if (nv) hipLaunchKernelGGL(k_ut_tab_vid, grid(nv), dim3(256), 0, st, vtx, nv, out_head, oh_off, out_vid);
  write_text(c, g, er.rr.rk, nv, n_loop, len, out_head, oh_off, out_vid, er.rr.cnt, out);
  return 0;
}

}  // namespace mhx
