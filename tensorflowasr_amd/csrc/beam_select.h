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
// write_paths, commit_stream and clear_stream are the n-best output, the stable-prefix commit and the reset of the searches in pieces.
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

}  // namespace beam_select
