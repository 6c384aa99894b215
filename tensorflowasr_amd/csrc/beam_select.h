// What the two device beam searches (ctc_beam.hip, rnnt_beam.hip) share: how the hypotheses that survive a frame are chosen.  The
// pieces are templated on the score type S: float totals in the CTC search, double totals in the transducer search.
//
// One frame of one utterance.  A beam has nb <= W rows, each a label sequence (a node of beam_trie.h's trie) with a total.
// 1. The frame pass, one wave per row of logits: lse (f32 max, f64 sum of exp, f32 log), and the row's top K = min(2W, V-1)
//    NON-blank classes by (lp desc, class asc), lp = S(x) - S(lse): K rounds of a wave arg-max under cls_before.  Its code is
//    written out in ctc_beam_frame_kernel and rb_frame_kernel: one templated copy measured slower in the transducer search
//    (profiles/beam_select_refactor_timing.json).
// 2. Candidates (total, cand_code(row, label)) in LDS: a row itself ("stay", label -1), the row extended by a class that is SPECIAL
//    to it - scored by the search from logits - lse, because something else joins the extension (the stay of the beam row that
//    already holds that sequence; in the CTC search also a repeat of the row's last label, which adds pb, not the total) - and
//    push_regulars: the row's first W top-K classes that are not special to it, at row total + lp.
//    Why 2W classes are enough: a regular extension scores row total + lp[c], monotone in lp[c].  A row has at most nb <= W specials,
//    so at least W of the top 2W classes are regular for it, and they are its best W regular extensions; an extension outside them
//    is beaten by W candidates of its own row and cannot enter a beam of width W.  A frame is O(W^2) candidates instead of O(W*V).
// 3. rank_candidates: rank = number of better candidates by (total desc, label sequence asc), early exit at `keep`; the order is
//    exact, so ranks are distinct.  The trie is walked only on an exact tie of totals.
// 4. grow_trie: one node per label sequence for the whole utterance, so a prefix that leaves the beam and comes back keeps its mass:
//    the search looks the winners up in the (parent, label) table, the missing ones become nodes numbered in rank order.
// write_paths, commit_stream and clear_stream are the n-best output, the stable-prefix commit and the reset of the searches in pieces;
// horizon_point / horizon_target / descends_from are the commit horizon's rule and compact_stream the trie compaction.
#pragma once
#include "beam_trie.h"
#include <algorithm>

namespace beam_select {

using beam_trie::Seq;
using beam_trie::Trie;

constexpr int MAXW = 64;      // a beam lives in one workgroup's LDS; a row index takes the low 6 bits of a candidate code
constexpr int THREADS = 256;  // of the per-utterance kernels
enum { CNT_LIVE = 0, CNT_NODES = 1, CNT_FRAMES = 2, CNT_N = 4 };  // per-utterance counters: live rows, trie nodes, frames searched

// a candidate: beam row `row` extended by `label`; label -1 = the row itself ("stay")
__device__ __forceinline__ unsigned cand_code(int row, int label) { return (unsigned)row | ((unsigned)(label + 1) << 6); }
__device__ __forceinline__ int cand_row(unsigned code) { return code & 63; }
__device__ __forceinline__ int cand_label(unsigned code) { return (int)(code >> 6) - 1; }

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Geometry {  // of a search over at most T frames of V classes at width W
  int K;           // classes listed per row
  long nmax;       // trie nodes per utterance: at most W new ones per frame
  unsigned hcap;   // slots of its (parent, label) table
  Geometry(int T, int V, int W) : K(std::min(2 * W, V - 1)), nmax(1 + (long)W * T), hcap(beam_trie::table_cap(nmax)) {}
};
// T * W bounded so that node ids and table sizes stay in int / unsigned range; V bounded by the candidate code's label field
inline bool shape_ok(int T, int V, int W) { return T > 0 && V >= 2 && V < (1 << 25) && W >= 1 && W <= MAXW && (long)T * W < (1L << 28); }

__device__ __forceinline__ Trie trie_at(int* parent, int* label, int* depth, long n0) { return Trie{parent + n0, label + n0, depth + n0}; }

__device__ __forceinline__ float log1p_exp_neg_abs(float d) { return log1pf(expf(-fabsf(d))); }
__device__ __forceinline__ double log1p_exp_neg_abs(double d) { return log1p(exp(-fabs(d))); }
template <class S>
__device__ __forceinline__ S lae(S a, S b) {  // log(exp(a) + exp(b)), the host routine's operation order
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const S m = a > b ? a : b;
  return m + log1p_exp_neg_abs(a - b);
}

// (lp, c) comes before (lq, d) in a row's class order
template <class S>
__device__ __forceinline__ bool cls_before(S lp, int c, S lq, int d) { return lp > lq || (lp == lq && c < d); }

// One wave, beam row `row` of total `tot`, lane per top-K class: the first W classes with !special(c) become candidates.  (Once W
// regular classes have been seen no lane can rank below W: the k0 loop ends.)
template <class S, class Special>
__device__ __forceinline__ void push_regulars(int row, S tot, const int* kc, const S* klp, int K, int W, int lane, Special special, S* ctot,
                                              unsigned* ccode, int* nc) {
  int seen = 0;
  for (int k0 = 0; k0 < K && seen < W; k0 += 64) {
    const int k = k0 + lane;
    bool reg = false;
    int c = -1;
    if (k < K) {
      c = kc[k];
      reg = !special(c);
    }
    const unsigned long long mask = __ballot(reg);
    const int rank = seen + __popcll(mask & ((1ull << lane) - 1ull));
    seen += __popcll(mask);
    if (reg && rank < W && tot != -INFINITY) {
      const S t = tot + klp[k];
      if (t != -INFINITY) {
        const int q = atomicAdd(nc, 1);
        ctot[q] = t;
        ccode[q] = cand_code(row, c);
      }
    }
  }
}

// The same under LM fusion (ctc_beam.hip): EVERY top-K class with !special(c) becomes a candidate, at (tot + lp) + lm_of(c), lm_of(c)
// = the LM score of the row's sequence extended by c.  The total is no longer monotone in lp, so the first W are not enough.
template <class S, class Special, class LmOf>
__device__ __forceinline__ void push_all_regulars(int row, S tot, const int* kc, const S* klp, int K, int lane, Special special, LmOf lm_of,
                                                  S* ctot, unsigned* ccode, int* nc) {
  if (tot == -INFINITY) return;
  for (int k = lane; k < K; k += 64) {
    const int c = kc[k];
    if (special(c)) continue;
    const S t = tot + klp[k];
    if (t == -INFINITY) continue;
    const S key = t + lm_of(c);
    const int q = atomicAdd(nc, 1);
    ctot[q] = key;
    ccode[q] = cand_code(row, c);
  }
}

// The whole workgroup: win[r] = the candidate of rank r < keep; bnode[i] = the node of beam row i.
template <class S>
__device__ __forceinline__ void rank_candidates(const S* ctot, const unsigned* ccode, int nc, int keep, const int* bnode, const Trie& tr,
                                                int* win, int tid) {
  for (int q = tid; q < nc; q += THREADS) {
    const S tq = ctot[q];
    const unsigned cq = ccode[q];
    const Seq sq{bnode[cand_row(cq)], cand_label(cq)};
    int rank = 0;
    for (int p = 0; p < nc && rank < keep; ++p) {
      const S tp = ctot[p];
      if (tp > tq) ++rank;
      else if (tp == tq && p != q) {
        const unsigned cp = ccode[p];
        if (beam_trie::seq_less(tr, Seq{bnode[cand_row(cp)], cand_label(cp)}, sq)) ++rank;
      }
    }
    if (rank < keep) win[rank] = q;
  }
}

// Wave 0 (the other waves return 0), lane = rank of a winner (keep <= 64: wave 0 holds them all): the `fresh` lanes, whose
// (npar, nlab) has no node yet, get nodes *nodes, *nodes + 1, .. in rank order, written to nnode.  Returns how many.
__device__ __forceinline__ int grow_trie(bool fresh, int tid, const int* nodes, const Trie& tr, unsigned long long* hk, int* hv,
                                         unsigned hcap, int* nnode, const int* npar, const int* nlab, const int* ndep) {
  if (tid >= 64) return 0;
  const unsigned long long mask = __ballot(fresh);
  if (fresh) {
    const int node = *nodes + __popcll(mask & ((1ull << tid) - 1ull));
    nnode[tid] = node;
    tr.parent[node] = npar[tid]; tr.label[node] = nlab[tid]; tr.depth[node] = ndep[tid];
    beam_trie::insert(hk, hv, hcap, npar[tid], nlab[tid], node);
  }
  return __popcll(mask);
}

// The whole workgroup: P paths, of which the first min(nb, P) live, path p = the sequence of node_of(p): tokens [P, OW] padded with
// `pad` and lengths [P].  (A row as wide as the frames searched holds every label.)
template <class NodeOf>
__device__ __forceinline__ void write_paths(const Trie& tr, int nb, int P, int OW, int pad, int tid, NodeOf node_of,
                                            int32_t* __restrict__ tokens, int32_t* __restrict__ tokens_len) {
  for (int p = tid; p < P; p += THREADS) tokens_len[p] = p < nb ? tr.depth[node_of(p)] : 0;
  for (long e = tid; e < (long)P * OW; e += THREADS) {
    const int p = (int)(e / OW), pos = (int)(e % OW);
    if (p >= nb || pos >= tr.depth[node_of(p)]) tokens[e] = pad;
  }
  if (tid < min(nb, P)) {
    int32_t* out = tokens + (long)tid * OW;
    for (int n = node_of(tid), d = tr.depth[n]; n > 0; n = tr.parent[n])
      if (--d < OW) out[d] = tr.label[n];
  }
}

// The whole workgroup: an empty table and the root node (the empty sequence) alone.
__device__ __forceinline__ void clear_stream(const Trie& tr, unsigned long long* hk, unsigned hcap, int tid) {
  for (unsigned i = tid; i < hcap; i += THREADS) hk[i] = beam_trie::EMPTY;
  if (tid == 0) { tr.parent[0] = -1; tr.label[0] = -1; tr.depth[0] = 0; }
}

// One wave per stream, lane i holds the node of live row i (nb live rows): commit the sequence of lane `best`, or with best < 0 the
// part that every live row shares.
__device__ __forceinline__ void commit_stream(const Trie& tr, int node, bool live, int nb, int best, int lane, int32_t* committed,
                                              int32_t* out, int32_t* count, int width, int pad) {
  int target = 0;
  if (nb > 0) target = best >= 0 ? __shfl(node, best, 64) : beam_trie::common_ancestor(tr, node, live);
  beam_trie::commit_labels(tr, target, lane, committed, out, count, width, pad);
}

// ---- the commit horizon (tfasr_*_beam_commit_horizon) --------------------------------------------------------------------------------
// Horizon state of one stream, int32 [horizon_stride(H)], owned by the caller and written by the horizon commit and the compaction
// alone: HS_ABS the frames the stream has consumed since its reset (never rebased), HS_SEEN the stream's CNT_FRAMES when HS_ABS was
// last brought up to date, then a ring of R = H + 1 prune points (frame count, trie node count), HS_HEAD the next slot, HS_FILL how
// many hold a point.  A point is logged by every call that finds new frames, so the logged frame counts are distinct integers: at most
// H of them lie in (now - H, now], the current one included, and the latest point at or before now - H is the one logged just before
// those - among the last H + 1.
enum { HS_ABS = 0, HS_SEEN = 1, HS_HEAD = 2, HS_FILL = 3, HS_RING = 4 };
__device__ __forceinline__ int horizon_stride(int H) { return HS_RING + 2 * (H + 1); }

// One wave.  Brings the state up to the stream's counters; when the stream has consumed frames since the last call this is a prune
// point: it is logged, and the node count X logged at the latest point at least H frames back is returned (>= 1), -1 when there is
// none or this is no prune point.  A node with id < X was in the trie H frames ago.
__device__ __forceinline__ int horizon_point(int32_t* hs, int H, const int* cnt, int lane) {
  int X = -1;
  if (lane == 0) {
    const int fr = cnt[CNT_FRAMES], d = fr - hs[HS_SEEN];
    hs[HS_SEEN] = fr;
    if (d > 0) {
      const int R = H + 1, now = hs[HS_ABS] + d;
      int head = min(max(hs[HS_HEAD], 0), R - 1);
      const int fill = min(max(hs[HS_FILL], 0) + 1, R);
      hs[HS_ABS] = now;
      hs[HS_RING + 2 * head] = now; hs[HS_RING + 2 * head + 1] = cnt[CNT_NODES];
      for (int i = 1; i < fill; ++i) {  // from the point before this one backwards
        const int slot = (head - i + R) % R;
        if (hs[HS_RING + 2 * slot] <= now - H) { X = max(hs[HS_RING + 2 * slot + 1], 1); break; }
      }
      hs[HS_HEAD] = (head + 1) % R;
      hs[HS_FILL] = fill;
    }
  }
  return __shfl(X, 0, 64);
}
// the deepest ancestor-or-self of `node` with id < X (X >= 1; ids grow from parent to child)
__device__ __forceinline__ int horizon_target(const Trie& tr, int node, int X) {
  while (node >= X) node = tr.parent[node];
  return node;
}
__device__ __forceinline__ bool descends_from(const Trie& tr, int node, int anc) {
  for (int d = tr.depth[node], da = tr.depth[anc]; d > da; --d) node = tr.parent[node];
  return node == anc;
}

// ---- compaction of one stream's trie (tfasr_*_beam_compact), the whole workgroup, in place -------------------------------------------
// New root = the ancestor of the live rows' common ancestor at depth min(*committed, its depth); kept = the nodes on the paths from the
// root to the live rows' nodes, in their old order (ids stay creation ordered, parent < child), depths rebased, the root keeps its LABEL
// (parent -1, depth 0).  The table doubles as scratch while it is empty of meaning: hv[i] = kept nodes below old id i (bit-inverted for
// a dropped node), the keys' bytes stage the kept (parent, label, depth) triples (3 nk <= 4 nmax <= 2 hcap ints) - then the table is
// rebuilt.  node_at(i) / set_node(i, n) read and write live row i's node; `hs` (may be NULL) is the stream's horizon state, whose logged
// node counts are remapped; out3 = (dropped depth, nodes kept, new CNT_FRAMES = the deepest live row).
// `payload` is what a search keeps per node beside the trie's three arrays (default: nothing): Payload::WORDS <= 3 ints per node,
// get(old id, dst) / put(new id, src).  It moves in a pass of its own, staged in the same key bytes once the triples are back in the
// trie (WORDS nk <= 3 nk ints) and before the table is rebuilt, while hv still maps old ids to new ones.
struct NoPayload { static constexpr int WORDS = 0; };
template <class NodeAt, class SetNode, class Payload = NoPayload>
__device__ __forceinline__ void compact_stream(const Trie& tr, unsigned long long* hk, int* hv, unsigned hcap, int* cnt, int nb,
                                               int32_t* committed, int32_t* hs, int H, int32_t* out3, int tid, NodeAt node_at,
                                               SetNode set_node, Payload payload = Payload{}) {
  __shared__ int sums[THREADS];
  __shared__ int s_root, s_drop, s_maxdep;
  const int n = cnt[CNT_NODES], frames_old = cnt[CNT_FRAMES], have = max(*committed, 0);
  if (nb < 1) {  // (a stream always holds a row; nothing to anchor a root on otherwise)
    if (tid == 0) { out3[0] = 0; out3[1] = n; out3[2] = frames_old; }
    return;
  }
  const int my = tid < nb ? node_at(tid) : 0;
  if (tid < 64) {
    const bool live = tid < nb;
    int md = live ? tr.depth[my] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) md = max(md, __shfl_xor(md, o, 64));
    int root = beam_trie::common_ancestor(tr, my, live);
    if (tid == 0) {
      const int rd = min(have, tr.depth[root]);
      for (int d = tr.depth[root]; d > rd; --d) root = tr.parent[root];
      s_root = root; s_drop = rd; s_maxdep = md;
    }
  }
  for (int i = tid; i < n; i += THREADS) hv[i] = 0;
  __syncthreads();
  const int root = s_root, drop = s_drop;
  if (tid < nb)  // mark the path up to the root, or up to a node another row has marked (that row goes on from there)
    for (int x = my; x >= root && atomicExch(&hv[x], 1) == 0 && x != root;) x = tr.parent[x];  // (ids fall towards the root)
  __syncthreads();
  const int chunk = (n + THREADS - 1) / THREADS, lo = min(tid * chunk, n), hi = min(lo + chunk, n);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += hv[i];
  sums[tid] = c;
  __syncthreads();
  int base = 0, nk = 0;
  for (int j = 0; j < THREADS; ++j) { if (j == tid) base = nk; nk += sums[j]; }
  for (int i = lo; i < hi; ++i) { const int m = hv[i]; hv[i] = m ? base : ~base; base += m; }
  __syncthreads();
  int* stage = (int*)hk;
  for (int i = tid; i < n; i += THREADS) {
    const int j = hv[i];
    if (j < 0) continue;
    stage[3 * j] = i == root ? -1 : hv[tr.parent[i]];  // (the kept set is closed towards the root)
    stage[3 * j + 1] = tr.label[i];
    stage[3 * j + 2] = tr.depth[i] - drop;
  }
  const int mine = tid < nb ? hv[my] : 0;
  if (hs)
    for (int k = tid; k < H + 1; k += THREADS) {
      const int v = hs[HS_RING + 2 * k + 1];
      hs[HS_RING + 2 * k + 1] = v >= n ? nk : v < 0 ? 0 : hv[v] >= 0 ? hv[v] : ~hv[v];
    }
  __syncthreads();
  for (int j = tid; j < nk; j += THREADS) { tr.parent[j] = stage[3 * j]; tr.label[j] = stage[3 * j + 1]; tr.depth[j] = stage[3 * j + 2]; }
  __syncthreads();
  if constexpr (Payload::WORDS > 0) {
    static_assert(Payload::WORDS <= 3, "the staging space holds 3 ints per kept node");
    for (int i = tid; i < n; i += THREADS)
      if (hv[i] >= 0) payload.get(i, stage + Payload::WORDS * hv[i]);
    __syncthreads();
    for (int j = tid; j < nk; j += THREADS) payload.put(j, stage + Payload::WORDS * j);
    __syncthreads();
  }
  for (unsigned i = tid; i < hcap; i += THREADS) hk[i] = beam_trie::EMPTY;
  __syncthreads();
  for (int j = 1 + tid; j < nk; j += THREADS) beam_trie::insert(hk, hv, hcap, tr.parent[j], tr.label[j], j);
  if (tid < nb) set_node(tid, mine);
  if (tid == 0) {
    const int frames = s_maxdep - drop;
    cnt[CNT_NODES] = nk; cnt[CNT_FRAMES] = frames;
    if (hs) hs[HS_SEEN] = frames - (frames_old - hs[HS_SEEN]);  // frames no commit has seen yet stay unseen
    *committed = have - drop;
    out3[0] = drop; out3[1] = nk; out3[2] = frames;
  }
}

}  // namespace beam_select
