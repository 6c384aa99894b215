// CTC prefix beam search (CtcModel.recognize_beam, models/ctc/base_ctc.py:127-149 -> tf.nn.ctc_beam_search_decoder: a HOST op in
// the reference too).  Host code only: the caller hands over the logits of one batch in host memory; the search works in the
// log domain with the usual (blank-ending, label-ending) probability pair per prefix, no repeated-label merging beyond CTC's
// own collapse (merge_repeated = False in the v2 API), top path only.
//
// Reference quirk kept on purpose: tf.nn.ctc_beam_search_decoder always treats the LAST class as blank, while this code
// base's blank is 0 (base_ctc.py passes no blank index to the beam decoder) - so `blank_index` is a parameter and the Python
// host passes V-1 to reproduce recognize_beam, 0 for a self-consistent decoder.
#include "common.h"
#include "beam_select.h"
#include "ngram_lm.h"
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

namespace {

constexpr float NEG_INF = -INFINITY;
inline float lse2(float a, float b) {
  if (a == NEG_INF) return b;
  if (b == NEG_INF) return a;
  const float m = a > b ? a : b;
  return m + log1pf(expf(-fabsf(a - b)));
}

// Prefixes live in a trie (node = parent + last label), so extending a prefix costs O(1) instead of a vector copy + an ordered-map
// insertion keyed by the whole label sequence (the first version spent 79 s on 32 x 250 frames x 1000 classes at width 10).
struct Node { int parent, label, depth; };
struct Beam { int node; float pb, pnb; };
struct Cand { float total; int src; int label; };  // label >= 0: beam `src` extended by `label`; label < 0: beam `src` itself

}  // namespace

extern "C" int tfasr_ctc_beam_search_host(const float* logits, const int32_t* logit_len, int B, int T, int V, int beam_width,
                                          int blank_index, int32_t* tokens, int32_t* tokens_len, float* log_prob) {
  if (!logits || !logit_len || !tokens || !tokens_len || B <= 0 || T <= 0 || V <= 1 || beam_width <= 0 || blank_index < 0 || blank_index >= V)
    return TFASR_STATUS_INVALID_VALUE;
  std::vector<float> lp(V);
  std::vector<Node> trie;
  std::vector<Beam> beams, next;
  std::vector<float> ext;        // [nb][V] label-ending probability of beam i extended by label c (incl. merged "stay" mass)
  std::vector<float> ext_pb;     // [nb][V] blank-ending probability of that same prefix when it is ALSO a current beam
  std::vector<Cand> cand;
  std::vector<int32_t> pa, pc;
  // (parent node, label) -> node, for the whole utterance: a label sequence has exactly ONE node, also when a prefix drops out of the
  // beam and is re-created later from its parent while one of its own extensions stayed (their probability mass must merge, as in
  // TensorFlow's beam-entry children map)
  std::unordered_map<uint64_t, int> child;
  auto prefix_of = [&](int node, std::vector<int32_t>& out) {
    out.clear();
    for (int n = node; n > 0; n = trie[n].parent) out.push_back(trie[n].label);
    std::reverse(out.begin(), out.end());
  };
  for (int b = 0; b < B; ++b) {
    const int Tb = std::min(std::max(logit_len[b], 0), T);
    trie.clear();
    child.clear();
    trie.push_back(Node{-1, -1, 0});  // node 0 = the empty prefix
    beams.assign(1, Beam{0, 0.f, NEG_INF});
    for (int t = 0; t < Tb; ++t) {
      const float* x = logits + ((size_t)b * T + t) * V;
      float mx = x[0];
      for (int v = 1; v < V; ++v) mx = std::max(mx, x[v]);
      double se = 0.0;
      for (int v = 0; v < V; ++v) se += std::exp((double)x[v] - mx);
      const float lz = mx + (float)std::log(se);
      for (int v = 0; v < V; ++v) lp[v] = x[v] - lz;
      const int nb = (int)beams.size();
      ext.assign((size_t)nb * V, NEG_INF);
      ext_pb.assign((size_t)nb * V, NEG_INF);
      // "stay" candidates: prefix unchanged (emit blank, or repeat its last label).  If the prefix's parent is itself a current beam,
      // the same prefix is also reachable as (parent extended by its last label): both contributions belong to ONE candidate.
      std::vector<int> merged_into(nb, -1);
      for (int i = 0; i < nb; ++i) {
        const Node& nd = trie[beams[i].node];
        if (nd.parent < 0) continue;
        for (int j = 0; j < nb; ++j)
          if (beams[j].node == nd.parent) { merged_into[i] = j; break; }
      }
      cand.clear();
      // extensions of every beam by one label
      for (int i = 0; i < nb; ++i) {
        const float pb = beams[i].pb, ptot = lse2(pb, beams[i].pnb);
        const Node& nd = trie[beams[i].node];
        float* row = ext.data() + (size_t)i * V;
        for (int c = 0; c < V; ++c) {
          if (c == blank_index) continue;
          const float add = (nd.label == c && nd.parent >= 0) ? pb : ptot;  // a repeat needs a blank in between
          if (add != NEG_INF) row[c] = add + lp[c];
        }
      }
      // staying on a prefix (emit blank, or repeat its last label): merged into (parent, last label) when the parent is a beam too
      for (int i = 0; i < nb; ++i) {
        const Node& nd = trie[beams[i].node];
        const float s_pb = lse2(beams[i].pb, beams[i].pnb) + lp[blank_index];
        const float s_pnb = nd.parent >= 0 ? beams[i].pnb + lp[nd.label] : NEG_INF;
        if (merged_into[i] >= 0) {
          const size_t k = (size_t)merged_into[i] * V + nd.label;
          ext_pb[k] = s_pb;
          ext[k] = lse2(ext[k], s_pnb);
        } else {
          cand.push_back(Cand{lse2(s_pb, s_pnb), i, -1});
        }
      }
      for (int i = 0; i < nb; ++i)
        for (int c = 0; c < V; ++c) {
          const size_t k = (size_t)i * V + c;
          if (ext[k] != NEG_INF || ext_pb[k] != NEG_INF) cand.push_back(Cand{lse2(ext_pb[k], ext[k]), i, c});
        }
      const size_t keep = std::min<size_t>(beam_width, cand.size());
      auto better = [&](const Cand& a, const Cand& c) {
        if (a.total != c.total) return a.total > c.total;
        // exact tie: order by the label sequences (what the reference-style ordered container did)
        prefix_of(beams[a.src].node, pa);
        if (a.label >= 0) pa.push_back(a.label);
        prefix_of(beams[c.src].node, pc);
        if (c.label >= 0) pc.push_back(c.label);
        return pa < pc;
      };
      std::partial_sort(cand.begin(), cand.begin() + keep, cand.end(), better);
      next.clear();
      for (size_t q = 0; q < keep; ++q) {
        const Cand& cd = cand[q];
        if (cd.label < 0) {
          const Beam& bm = beams[cd.src];
          const Node& nd = trie[bm.node];
          const float ptot = lse2(bm.pb, bm.pnb);
          next.push_back(Beam{bm.node, ptot + lp[blank_index], nd.parent >= 0 ? bm.pnb + lp[nd.label] : NEG_INF});
        } else {
          const size_t k = (size_t)cd.src * V + cd.label;
          // the extended prefix may already be a node (it is a beam now, or was one earlier): reuse it
          const int par = beams[cd.src].node;
          const uint64_t key = (uint64_t)par * (uint64_t)V + (uint64_t)cd.label;
          int node;
          auto it = child.find(key);
          if (it != child.end()) {
            node = it->second;
          } else {
            trie.push_back(Node{par, cd.label, trie[par].depth + 1});
            node = (int)trie.size() - 1;
            child.emplace(key, node);
          }
          next.push_back(Beam{node, ext_pb[k], ext[k]});
        }
      }
      beams.swap(next);
    }
    int best = -1;
    float bestp = NEG_INF;
    for (int i = 0; i < (int)beams.size(); ++i) {
      const float p = lse2(beams[i].pb, beams[i].pnb);
      bool take = best < 0 || p > bestp;
      if (!take && p == bestp) {
        prefix_of(beams[i].node, pa);
        prefix_of(beams[best].node, pc);
        take = pa < pc;
      }
      if (take) { best = i; bestp = p; }
    }
    int32_t* out = tokens + (size_t)b * T;
    std::vector<int32_t> seq;
    if (best >= 0) prefix_of(beams[best].node, seq);
    const int n = (int)seq.size();
    for (int i = 0; i < T; ++i) out[i] = i < n ? seq[i] : 0;  // tf.sparse.to_dense default value 0
    tokens_len[b] = n;
    if (log_prob) log_prob[b] = bestp;
  }
  return TFASR_STATUS_SUCCESS;
}

// ---- the same search with an n-gram LM fused in (tfasr_hip.h, "N-gram LM shallow fusion"): the structure above with three
// differences - the ranking key is float(acoustic total + lm of the label sequence), a row is extended only by the frame's K =
// min(2W, V-1) acoustically best non-blank classes and by the classes special to it, and the final order adds the end-of-sentence
// term.  The pb / pnb bookkeeping is untouched.  A trie node carries lm of its sequence and the LM state after it.
namespace {
struct LmNode { int parent, label, depth, state; float lm; };
struct LmCand { float key; int src; int label; };
}  // namespace

extern "C" int tfasr_ctc_beam_search_lm_host(const float* logits, const int32_t* logit_len, int B, int T, int V, int beam_width, int top_paths,
                                             int blank_index, const tfasr_ngram_lm_t* lm_, int32_t* tokens, int32_t* tokens_len, float* score,
                                             float* log_prob, float* lm_score) {
  if (!logits || !logit_len || !tokens || !tokens_len || !score || !log_prob || !lm_score || !ngram_lm::tables_ok(lm_))
    return TFASR_STATUS_INVALID_VALUE;
  if (B <= 0 || T <= 0 || V <= 1 || beam_width <= 0 || top_paths < 1 || top_paths > beam_width || blank_index < 0 || blank_index >= V)
    return TFASR_STATUS_INVALID_VALUE;
  if (beam_width > TFASR_CTC_LM_MAX_BEAM) return TFASR_STATUS_UNSUPPORTED;
  const ngram_lm::Tables lm = ngram_lm::tables_of(*lm_);
  const int W = beam_width, P = top_paths, K = std::min(2 * W, V - 1);
  std::vector<float> lp(V);
  std::vector<LmNode> trie;
  std::vector<Beam> beams, next;
  std::vector<float> ext, ext_pb;  // as in tfasr_ctc_beam_search_host
  std::vector<char> cand_of;       // [nb][V] class c extends beam i: listed this frame, or special to the beam
  std::vector<int> listed(V), merged_into;
  std::vector<LmCand> cand;
  std::vector<int32_t> pa, pc;
  std::unordered_map<uint64_t, int> child;
  auto prefix_of = [&](int node, std::vector<int32_t>& out) {
    out.clear();
    for (int n = node; n > 0; n = trie[n].parent) out.push_back(trie[n].label);
    std::reverse(out.begin(), out.end());
  };
  for (int b = 0; b < B; ++b) {
    const int Tb = std::min(std::max(logit_len[b], 0), T);
    trie.clear();
    child.clear();
    trie.push_back(LmNode{-1, -1, 0, lm.start, 0.f});
    beams.assign(1, Beam{0, 0.f, NEG_INF});
    for (int t = 0; t < Tb; ++t) {
      const float* x = logits + ((size_t)b * T + t) * V;
      float mx = x[0];
      for (int v = 1; v < V; ++v) mx = std::max(mx, x[v]);
      double se = 0.0;
      for (int v = 0; v < V; ++v) se += std::exp((double)x[v] - mx);
      const float lz = mx + (float)std::log(se);
      for (int v = 0; v < V; ++v) lp[v] = x[v] - lz;
      // the frame's K best non-blank classes by (lp desc, class asc)
      int nl = 0;
      for (int v = 0; v < V; ++v)
        if (v != blank_index) listed[nl++] = v;
      // (NaN logits are outside the contract; a NaN counts as -inf here so that the comparator stays a strict weak order)
      auto rank_lp = [&](int c) { return std::isnan(lp[c]) ? NEG_INF : lp[c]; };
      std::partial_sort(listed.begin(), listed.begin() + K, listed.begin() + nl, [&](int c, int d) {
        const float a = rank_lp(c), e = rank_lp(d);
        return a > e || (a == e && c < d);
      });
      const int nb = (int)beams.size();
      ext.assign((size_t)nb * V, NEG_INF);
      ext_pb.assign((size_t)nb * V, NEG_INF);
      cand_of.assign((size_t)nb * V, 0);
      merged_into.assign(nb, -1);
      for (int i = 0; i < nb; ++i) {
        const LmNode& nd = trie[beams[i].node];
        if (nd.parent < 0) continue;
        for (int j = 0; j < nb; ++j)
          if (beams[j].node == nd.parent) { merged_into[i] = j; break; }
      }
      cand.clear();
      for (int i = 0; i < nb; ++i) {
        const float pb = beams[i].pb, ptot = lse2(pb, beams[i].pnb);
        const LmNode& nd = trie[beams[i].node];
        float* row = ext.data() + (size_t)i * V;
        char* use = cand_of.data() + (size_t)i * V;
        for (int k = 0; k < K; ++k) use[listed[k]] = 1;
        if (nd.parent >= 0) use[nd.label] = 1;  // a repeat of the row's own last label
        for (int c = 0; c < V; ++c) {
          if (c == blank_index) continue;
          const float add = (nd.label == c && nd.parent >= 0) ? pb : ptot;  // a repeat needs a blank in between
          if (add != NEG_INF) row[c] = add + lp[c];
        }
      }
      for (int i = 0; i < nb; ++i) {
        const LmNode& nd = trie[beams[i].node];
        const float s_pb = lse2(beams[i].pb, beams[i].pnb) + lp[blank_index];
        const float s_pnb = nd.parent >= 0 ? beams[i].pnb + lp[nd.label] : NEG_INF;
        if (merged_into[i] >= 0) {
          const size_t k = (size_t)merged_into[i] * V + nd.label;
          ext_pb[k] = s_pb;
          ext[k] = lse2(ext[k], s_pnb);
          cand_of[k] = 1;  // a merge target of the parent's row
        } else {
          cand.push_back(LmCand{lse2(s_pb, s_pnb) + nd.lm, i, -1});
        }
      }
      for (int i = 0; i < nb; ++i) {
        const LmNode& nd = trie[beams[i].node];
        for (int c = 0; c < V; ++c) {
          const size_t k = (size_t)i * V + c;
          if (!cand_of[k] || (ext[k] == NEG_INF && ext_pb[k] == NEG_INF)) continue;
          int st;
          const float lmv = nd.lm + ngram_lm::walk(lm, lm.wlogp, nd.state, c, &st);
          cand.push_back(LmCand{lse2(ext_pb[k], ext[k]) + lmv, i, c});
        }
      }
      const size_t keep = std::min<size_t>(W, cand.size());
      auto better = [&](const LmCand& a, const LmCand& c) {
        if (a.key != c.key) return a.key > c.key;
        prefix_of(beams[a.src].node, pa);
        if (a.label >= 0) pa.push_back(a.label);
        prefix_of(beams[c.src].node, pc);
        if (c.label >= 0) pc.push_back(c.label);
        return pa < pc;
      };
      std::partial_sort(cand.begin(), cand.begin() + keep, cand.end(), better);
      next.clear();
      for (size_t q = 0; q < keep; ++q) {
        const LmCand& cd = cand[q];
        if (cd.label < 0) {
          const Beam& bm = beams[cd.src];
          const LmNode& nd = trie[bm.node];
          const float ptot = lse2(bm.pb, bm.pnb);
          next.push_back(Beam{bm.node, ptot + lp[blank_index], nd.parent >= 0 ? bm.pnb + lp[nd.label] : NEG_INF});
        } else {
          const size_t k = (size_t)cd.src * V + cd.label;
          const int par = beams[cd.src].node;
          const uint64_t key = (uint64_t)par * (uint64_t)V + (uint64_t)cd.label;
          int node;
          auto it = child.find(key);
          if (it != child.end()) {
            node = it->second;
          } else {
            int st;
            const float lmv = trie[par].lm + ngram_lm::walk(lm, lm.wlogp, trie[par].state, cd.label, &st);
            trie.push_back(LmNode{par, cd.label, trie[par].depth + 1, st, lmv});
            node = (int)trie.size() - 1;
            child.emplace(key, node);
          }
          next.push_back(Beam{node, ext_pb[k], ext[k]});
        }
      }
      beams.swap(next);
    }
    // the final beam by score = acoustic total + (lm + end-of-sentence term), ties: the smaller label sequence
    const int nb = (int)beams.size();
    std::vector<float> ac(nb), lmt(nb), sc(nb);
    std::vector<int> order(nb);
    for (int i = 0; i < nb; ++i) {
      const LmNode& nd = trie[beams[i].node];
      ac[i] = lse2(beams[i].pb, beams[i].pnb);
      lmt[i] = nd.lm + ngram_lm::end_of_sentence(lm, nd.state);
      sc[i] = ac[i] + lmt[i];
      order[i] = i;
    }
    std::sort(order.begin(), order.end(), [&](int a, int c) {
      if (sc[a] != sc[c]) return sc[a] > sc[c];
      prefix_of(beams[a].node, pa);
      prefix_of(beams[c].node, pc);
      return pa < pc;
    });
    for (int p = 0; p < P; ++p) {
      int32_t* out = tokens + ((size_t)b * P + p) * T;
      std::vector<int32_t> seq;
      if (p < nb) prefix_of(beams[order[p]].node, seq);
      const int n = (int)seq.size();
      for (int i = 0; i < T; ++i) out[i] = i < n ? seq[i] : 0;
      tokens_len[(size_t)b * P + p] = n;
      score[(size_t)b * P + p] = p < nb ? sc[order[p]] : NEG_INF;
      log_prob[(size_t)b * P + p] = p < nb ? ac[order[p]] : NEG_INF;
      lm_score[(size_t)b * P + p] = p < nb ? lmt[order[p]] : 0.f;
    }
  }
  return TFASR_STATUS_SUCCESS;
}

// ================================================================================================================================
// Device prefix beam search (tfasr_ctc_beam_search): the same decoder as tfasr_ctc_beam_search_host above, stream ordered, with the
// top `top_paths` paths of the final beam.  Two launches:
//
// 1. ctc_beam_frame_kernel, one wave per (b, t) row: beam_select.h's frame pass in f32 (the host routine's arithmetic, so
//    lp = x - lse comes out as the host's value).
// 2. ctc_beam_search_kernel, one workgroup per utterance, all frames in one launch, the beam in LDS.  Per frame beam_select.h's
//    selection over at most W^2 + 3W candidates, with what is CTC's own: a row carries the (blank-ending, label-ending) pair, a
//    stay is merged into its parent's extension when the parent is a beam (as in the host routine), and the classes special to
//    row i are its own last label (a repeat adds pb_i, not ptot_i) and its merge targets (the labels of the beams whose parent
//    is beam i: their stay mass joins the extension).
//
// The search in pieces (tfasr_ctc_beam_reset / _advance / _commit / _nbest, streaming sessions) is the same two kernels: the search
// kernel loads its LDS beam from the workspace's carry area instead of starting from the empty prefix, runs the chunk's frames and
// stores the beam back; the n-best of a carried beam is the same kernel over zero frames.  tfasr_ctc_beam_commit_horizon and
// tfasr_ctc_beam_compact (commit horizon, trie compaction: DESIGN.md 4a) work on the carry area and the trie between two advances.
// ================================================================================================================================
namespace {

using namespace beam_select;
using beam_trie::seq_less;

constexpr int BEAM_MAXK = 2 * MAXW;
constexpr int BEAM_MAXC = MAXW * MAXW + 3 * MAXW;  // stays + specials (<= 2 per beam) + W regulars per beam

template <typename T>
__global__ __launch_bounds__(256) void ctc_beam_frame_kernel(const T* __restrict__ logits, const int32_t* __restrict__ logit_len,
                                                             float* __restrict__ lse, float* __restrict__ lp_blank,
                                                             int32_t* __restrict__ top_c, float* __restrict__ top_lp, int B, int Tm,
                                                             int V, int K, int blank) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)B * Tm;
  const long w0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (long)gridDim.x * (blockDim.x >> 6);
  for (long r = w0; r < rows; r += nw) {
    const int b = (int)(r / Tm), t = (int)(r % Tm);
    if (t >= min(max(logit_len[b], 0), Tm)) continue;  // frames past the utterance are never read
    const T* row = logits + r * V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, Num<T>::ld(row + v));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    double s = 0.0;
    for (int v = lane; v < V; v += 64) s += exp((double)Num<T>::ld(row + v) - (double)m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float lz = m + (float)log(s);
    // K rounds of a wave arg-max, each restricted to the classes after the previous winner in (lp desc, class asc) order
    float plp = INFINITY;
    int pc = -1;
    for (int k = 0; k < K; ++k) {
      float bl = -INFINITY;
      int bc = 0x7fffffff;
      for (int v = lane; v < V; v += 64) {
        if (v == blank) continue;
        const float l = Num<T>::ld(row + v) - lz;
        if (cls_before(plp, pc, l, v) && cls_before(l, v, bl, bc)) { bl = l; bc = v; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ol = __shfl_xor(bl, o, 64);
        const int oc = __shfl_xor(bc, o, 64);
        if (cls_before(ol, oc, bl, bc)) { bl = ol; bc = oc; }
      }
      if (lane == 0) { top_c[r * K + k] = min(bc, V - 1); top_lp[r * K + k] = bl; }  // clamp: only NaN rows leave bc unset
      plp = bl;
      pc = bc;
    }
    if (lane == 0) { lse[r] = lz; lp_blank[r] = Num<T>::ld(row + blank) - lz; }
  }
}

// the beam of every stream between two advances: what the search kernel holds in LDS, [B][W] each, and [B][CNT_N] counters
struct CtcCarry { int *node, *par, *lab, *dep; float *pb, *pnb; int* cnt; };
enum { BEAM_LOAD = 1, BEAM_STORE = 2, BEAM_OUTPUT = 4 };  // one-shot search: BEAM_OUTPUT alone

// LM fusion (the LM = true instantiations): the tables, per trie node lm of its sequence and the LM state after it (written when the
// node is created, beside the trie's three arrays: they ARE the carried LM state of a stream, a beam row reads its own from its node),
// the two extra outputs, and which streams have ended: those rank with the end-of-sentence term (all_final: every stream, the one-shot
// search; else the streams with fin[b] != 0, fin NULL: none)
struct LmDev { ngram_lm::Tables t; float* node_lm; int* node_state; float *score, *lm_score; const int32_t* fin; int all_final; };

// the LM part of the key a carried row ranks by: lm of its node's sequence, with the end-of-sentence term when its stream has ended
__device__ __forceinline__ float lm_rank_term(const LmDev& lmd, const float* node_lm, const int* node_state, long nmax, int node, bool ended) {
  const long n = min(max((long)node, 0L), nmax - 1);
  const float lm = node_lm[n];
  return ended ? lm + ngram_lm::end_of_sentence(lmd.t, ngram_lm::clamp_node(node_state[n], lmd.t.nodes)) : lm;
}

template <typename T, bool LM>
__global__ __launch_bounds__(THREADS) void ctc_beam_search_kernel(
    const T* __restrict__ logits, const int32_t* __restrict__ logit_len, const float* __restrict__ lse_ws,
    const float* __restrict__ lpb_ws, const int32_t* __restrict__ top_c, const float* __restrict__ top_lp, int* trie_parent,
    int* trie_label, int* trie_depth, unsigned long long* hkeys, int* hvals, int Tm, int V, int W, int K, int P, long nmax,
    unsigned hcap, int32_t* __restrict__ tokens, int32_t* __restrict__ tokens_len, float* __restrict__ log_prob, CtcCarry cy, int mode,
    int Tcap, int OW, LmDev lmd) {
  // Tm = frames per utterance of `logits` (the whole utterance or one chunk), OW = the row width of `tokens`, Tcap = the most frames a
  // carried beam takes (its trie holds 1 + W * Tcap nodes)
  // beam state (node, its parent / last label / depth, probabilities) and per-frame scratch
  __shared__ int bnode[MAXW], bpar[MAXW], blab[MAXW], bdep[MAXW], merged[MAXW];
  __shared__ float bpb[MAXW], bpnb[MAXW], bptot[MAXW], lpl[MAXW], spb[MAXW], spnb[MAXW];
  __shared__ int nnode[MAXW], npar[MAXW], nlab[MAXW], ndep[MAXW], win[MAXW];
  __shared__ float npb[MAXW], npnb[MAXW];
  __shared__ int kc[BEAM_MAXK];
  __shared__ float klp[BEAM_MAXK];
  __shared__ float ctot[BEAM_MAXC];
  __shared__ unsigned ccode[BEAM_MAXC];
  __shared__ int s_nc, s_nb, s_ntrie;
  // LM only.  The plain instantiation (LM = false) must not reference these four arrays or lm_ext below outside `if constexpr (LM)`:
  // unreferenced, they are dropped from its LDS and it compiles to the code it was before the fusion existed.
  __shared__ float blm[MAXW], nlm[MAXW];  // lm of each row's sequence, and of the next beam's
  __shared__ int blms[MAXW], nlms[MAXW];  // the LM state after it

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int Tb = logit_len ? min(max(logit_len[b], 0), Tm) : 0;
  if ((mode & BEAM_LOAD) && !(mode & BEAM_OUTPUT) && Tb == 0) return;  // an idle stream keeps every byte of its beam
  const Trie tr = trie_at(trie_parent, trie_label, trie_depth, (long)b * nmax);
  unsigned long long* hk = hkeys + (long)b * hcap;
  int* hv = hvals + (long)b * hcap;
  float* node_lm = nullptr;
  int* node_state = nullptr;
  if constexpr (LM) { node_lm = lmd.node_lm + (long)b * nmax; node_state = lmd.node_state + (long)b * nmax; }
  // lm of row i's sequence extended by class c
  auto lm_ext = [&](int i, int c) {
    int st;
    return blm[i] + ngram_lm::walk(lmd.t, lmd.t.wlogp, blms[i], c, &st);
  };
  int frames0 = 0;
  if (mode & BEAM_LOAD) {
    const int* cnt = cy.cnt + b * CNT_N;
    const int nb0 = min(max(cnt[CNT_LIVE], 0), W);
    const long c0 = (long)b * W;
    if (tid < nb0) {
      bnode[tid] = cy.node[c0 + tid]; bpar[tid] = cy.par[c0 + tid]; blab[tid] = cy.lab[c0 + tid]; bdep[tid] = cy.dep[c0 + tid];
      bpb[tid] = cy.pb[c0 + tid]; bpnb[tid] = cy.pnb[c0 + tid];
      if constexpr (LM) {  // a row's lm and state are its node's: the values the one-shot search holds in LDS at this frame
        const long n = min(max((long)bnode[tid], 0L), nmax - 1);
        blm[tid] = node_lm[n]; blms[tid] = ngram_lm::clamp_node(node_state[n], lmd.t.nodes);
      }
    }
    if (tid == 0) { s_nb = nb0; s_ntrie = cnt[CNT_NODES]; }
    frames0 = cnt[CNT_FRAMES];
    Tb = min(Tb, max(Tcap - frames0, 0));
  } else {
    clear_stream(tr, hk, hcap, tid);
    if (tid == 0) {
      bnode[0] = 0; bpar[0] = -1; blab[0] = -1; bdep[0] = 0; bpb[0] = 0.f; bpnb[0] = -INFINITY;
      s_nb = 1; s_ntrie = 1;
      if constexpr (LM) { blm[0] = 0.f; blms[0] = lmd.t.start; node_lm[0] = 0.f; node_state[0] = lmd.t.start; }
    }
  }
  if (tid < MAXW) win[tid] = 0;
  __syncthreads();

  for (int t = 0; t < Tb; ++t) {
    const long r = (long)b * Tm + t;
    const T* row = logits + r * V;
    const float lz = lse_ws[r], lpblank = lpb_ws[r];
    const int nb = s_nb;
    if (tid < K) { kc[tid] = top_c[r * K + tid]; klp[tid] = top_lp[r * K + tid]; }
    if (tid < nb) {
      bptot[tid] = lae(bpb[tid], bpnb[tid]);
      lpl[tid] = bpar[tid] >= 0 ? Num<T>::ld(row + blab[tid]) - lz : -INFINITY;
    }
    if (tid < MAXW) win[tid] = 0;
    if (tid == 0) s_nc = 0;
    __syncthreads();
    if (tid < nb) {
      int m = -1;
      if (bpar[tid] >= 0)
        for (int j = 0; j < nb; ++j)
          if (bnode[j] == bpar[tid]) { m = j; break; }
      merged[tid] = m;
      spb[tid] = bptot[tid] + lpblank;
      spnb[tid] = bpar[tid] >= 0 ? bpnb[tid] + lpl[tid] : -INFINITY;
    }
    __syncthreads();
    // --- candidates: stays not merged into a parent's extension
    if (tid < nb && merged[tid] < 0) {
      const int q = atomicAdd(&s_nc, 1);
      if constexpr (LM) ctot[q] = lae(spb[tid], spnb[tid]) + blm[tid];
      else ctot[q] = lae(spb[tid], spnb[tid]);
      ccode[q] = cand_code(tid, -1);
    }
    // --- specials: pair (i, j): beam j's stay merged into (beam i, label of j); (i, i): beam i repeating its own last label
    for (int pq = tid; pq < nb * nb; pq += THREADS) {
      const int i = pq / nb, j = pq % nb;
      int c = -1, child = -1;
      if (j != i && merged[j] == i) { c = blab[j]; child = j; }
      if (j == i && bpar[i] >= 0) {
        c = blab[i];
        for (int k = 0; k < nb; ++k)
          if (merged[k] == i && blab[k] == c) c = -1;  // counted with that child
      }
      if (c < 0) continue;
      const bool rep = bpar[i] >= 0 && c == blab[i];
      const float add = rep ? bpb[i] : bptot[i];
      const float lpc = child >= 0 ? lpl[child] : lpl[i];
      float ext = add != -INFINITY ? add + lpc : -INFINITY, ext_pb = -INFINITY;
      if (child < 0)
        for (int k = 0; k < nb; ++k)
          if (merged[k] == i && blab[k] == c) child = k;
      if (child >= 0) { ext_pb = spb[child]; ext = lae(ext, spnb[child]); }
      const float tot = lae(ext_pb, ext);
      if (tot != -INFINITY) {
        float key = tot;
        if constexpr (LM) key = tot + (child >= 0 ? blm[child] : lm_ext(i, c));  // a merged child holds that very sequence
        const int q = atomicAdd(&s_nc, 1);
        ctot[q] = key;
        ccode[q] = cand_code(i, c);
      }
    }
    // --- regulars: wave per beam; special to row i = its own last label and its merge targets
    for (int i = wid; i < nb; i += THREADS / 64) {
      auto special_to_row = [&](int c) {
        bool special = bpar[i] >= 0 && c == blab[i];
        for (int j = 0; j < nb && !special; ++j) special = merged[j] == i && blab[j] == c;
        return special;
      };
      if constexpr (LM) push_all_regulars(i, bptot[i], kc, klp, K, lane, special_to_row, [&](int c) { return lm_ext(i, c); }, ctot, ccode, &s_nc);
      else push_regulars(i, bptot[i], kc, klp, K, W, lane, special_to_row, ctot, ccode, &s_nc);
    }
    __syncthreads();
    const int nc = s_nc, keep = min(W, nc);
    rank_candidates(ctot, ccode, nc, keep, bnode, tr, win, tid);
    __syncthreads();
    // --- the next beam: probabilities and (parent, label) of each winner; look the extended prefix up in the table
    bool fresh = false;
    if (tid < keep) {
      const unsigned code = ccode[win[tid]];
      const int i = cand_row(code), c = cand_label(code);
      if (c < 0) {
        nnode[tid] = bnode[i]; npar[tid] = bpar[i]; nlab[tid] = blab[i]; ndep[tid] = bdep[i];
        npb[tid] = spb[i]; npnb[tid] = spnb[i];
        if constexpr (LM) { nlm[tid] = blm[i]; nlms[tid] = blms[i]; }
      } else {
        const bool rep = bpar[i] >= 0 && c == blab[i];
        const float add = rep ? bpb[i] : bptot[i];
        float ext = add != -INFINITY ? add + (Num<T>::ld(row + c) - lz) : -INFINITY, ext_pb = -INFINITY;
        for (int k = 0; k < nb; ++k)
          if (merged[k] == i && blab[k] == c) { ext_pb = spb[k]; ext = lae(ext, spnb[k]); }
        npb[tid] = ext_pb; npnb[tid] = ext;
        npar[tid] = bnode[i]; nlab[tid] = c; ndep[tid] = bdep[i] + 1;
        const int node = beam_trie::lookup(hk, hv, hcap, bnode[i], c);
        nnode[tid] = node;
        fresh = node < 0;
        if constexpr (LM) {
          if (node >= 0) {
            nlm[tid] = node_lm[node]; nlms[tid] = node_state[node];
          } else {
            int st;
            nlm[tid] = blm[i] + ngram_lm::walk(lmd.t, lmd.t.wlogp, blms[i], c, &st);
            nlms[tid] = st;
          }
        }
      }
    }
    const int nfresh = grow_trie(fresh, tid, &s_ntrie, tr, hk, hv, hcap, nnode, npar, nlab, ndep);
    if constexpr (LM)
      if (fresh) { node_lm[nnode[tid]] = nlm[tid]; node_state[nnode[tid]] = nlms[tid]; }  // (fresh lanes are wave 0's: nnode is their own)
    __syncthreads();
    if (tid < keep) {
      bnode[tid] = nnode[tid]; bpar[tid] = npar[tid]; blab[tid] = nlab[tid]; bdep[tid] = ndep[tid];
      bpb[tid] = npb[tid]; bpnb[tid] = npnb[tid];
      if constexpr (LM) { blm[tid] = nlm[tid]; blms[tid] = nlms[tid]; }
    }
    if (tid == 0) {
      s_nb = keep;
      s_ntrie += nfresh;
    }
    __syncthreads();
  }

  const int nb = s_nb;
  if (mode & BEAM_STORE) {
    const long c0 = (long)b * W;
    if (tid < nb) {
      cy.node[c0 + tid] = bnode[tid]; cy.par[c0 + tid] = bpar[tid]; cy.lab[c0 + tid] = blab[tid]; cy.dep[c0 + tid] = bdep[tid];
      cy.pb[c0 + tid] = bpb[tid]; cy.pnb[c0 + tid] = bpnb[tid];
    }
    if (tid == 0) {
      int* cnt = cy.cnt + b * CNT_N;
      cnt[CNT_LIVE] = nb; cnt[CNT_NODES] = s_ntrie; cnt[CNT_FRAMES] = frames0 + Tb;
    }
  }
  if (!(mode & BEAM_OUTPUT)) return;
  const long obase = (long)b * P;
  if constexpr (LM) {
    // final beam by score = acoustic total + (lm + the end-of-sentence term), ties: smaller label sequence; a stream that has not
    // ended ranks by acoustic total + lm, the key its rows were selected by
    const bool ended = lmd.all_final || (lmd.fin && lmd.fin[b]);
    if (tid < nb) {
      bptot[tid] = lae(bpb[tid], bpnb[tid]);
      nlm[tid] = ended ? blm[tid] + ngram_lm::end_of_sentence(lmd.t, blms[tid]) : blm[tid];
      spb[tid] = bptot[tid] + nlm[tid];
    }
    __syncthreads();
    if (tid < nb) {
      const float sq = spb[tid];
      int rank = 0;
      for (int p = 0; p < nb; ++p) {
        const float sp = spb[p];
        if (sp > sq || (sp == sq && p != tid && seq_less(tr, Seq{bnode[p], -1}, Seq{bnode[tid], -1}))) ++rank;
      }
      if (rank < P) win[rank] = tid;
    }
    __syncthreads();
    for (int p = tid; p < P; p += THREADS) {
      const int i = p < nb ? win[p] : 0;
      log_prob[obase + p] = p < nb ? bptot[i] : -INFINITY;
      lmd.lm_score[obase + p] = p < nb ? nlm[i] : 0.f;
      lmd.score[obase + p] = p < nb ? spb[i] : -INFINITY;
    }
    write_paths(tr, nb, P, OW, 0, tid, [&](int p) { return bnode[win[p]]; }, tokens + obase * OW, tokens_len + obase);
    return;
  }
  // final beam, best first (ties: smaller label sequence); top P paths, dense and 0 padded
  if (tid < nb) {
    const float tq = lae(bpb[tid], bpnb[tid]);
    int rank = 0;
    for (int p = 0; p < nb; ++p) {
      const float tp = lae(bpb[p], bpnb[p]);
      if (tp > tq || (tp == tq && p != tid && seq_less(tr, Seq{bnode[p], -1}, Seq{bnode[tid], -1}))) ++rank;
    }
    if (rank < P) {
      win[rank] = tid;
      npb[rank] = tq;
    }
  }
  __syncthreads();
  for (int p = tid; p < P; p += THREADS) log_prob[obase + p] = p < nb ? npb[p] : -INFINITY;
  write_paths(tr, nb, P, OW, 0, tid, [&](int p) { return bnode[win[p]]; }, tokens + obase * OW, tokens_len + obase);
}

// ---- tfasr_ctc_beam_reset: the streams named by `mask` (NULL: all) hold the empty prefix alone ----
// (LM: the root's lm and LM state as well, lm_start = the state a sequence begins in)
template <bool LM>
__global__ __launch_bounds__(THREADS) void ctc_beam_reset_kernel(const int32_t* __restrict__ mask, int* trie_parent, int* trie_label,
                                                                 int* trie_depth, unsigned long long* hkeys, CtcCarry cy, int W, long nmax,
                                                                 unsigned hcap, float* node_lm, int* node_state, int lm_start) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (mask && !mask[b]) return;
  clear_stream(trie_at(trie_parent, trie_label, trie_depth, (long)b * nmax), hkeys + (long)b * hcap, hcap, tid);
  if (tid == 0) {
    const long c0 = (long)b * W;
    cy.node[c0] = 0; cy.par[c0] = -1; cy.lab[c0] = -1; cy.dep[c0] = 0; cy.pb[c0] = 0.f; cy.pnb[c0] = -INFINITY;
    int* cnt = cy.cnt + b * CNT_N;
    cnt[CNT_LIVE] = 1; cnt[CNT_NODES] = 1; cnt[CNT_FRAMES] = 0;
    if constexpr (LM) { node_lm[(long)b * nmax] = 0.f; node_state[(long)b * nmax] = lm_start; }
  }
}

// lane of the best live row in the n-best order (total desc, then the smaller label sequence); lane i holds the node of live row i.
// LM: the order of the fused n-best, float(total + lm), lm with the end-of-sentence term when the stream has `ended`.
template <bool LM>
__device__ __forceinline__ int ctc_best_lane(const Trie& tr, const CtcCarry& cy, long c0, int nb, int lane, int node, bool live,
                                             const LmDev& lmd, long n0, long nmax, bool ended) {
  auto key = [&](int p, int nd) {
    const float t = lae(cy.pb[c0 + p], cy.pnb[c0 + p]);
    if constexpr (LM) return t + lm_rank_term(lmd, lmd.node_lm + n0, lmd.node_state + n0, nmax, nd, ended);
    else return t;
  };
  const float tq = live ? key(lane, node) : -INFINITY;
  bool best = live;
  for (int p = 0; p < nb && best; ++p) {
    const float tp = key(p, cy.node[c0 + p]);
    if (tp > tq || (tp == tq && p != lane && seq_less(tr, Seq{cy.node[c0 + p], -1}, Seq{node, -1}))) best = false;
  }
  const unsigned long long m = __ballot(best);
  return m ? __ffsll((long long)m) - 1 : 0;
}

// ---- tfasr_ctc_beam_commit: one wave per stream, a lane per live row; `fin` streams commit their best row (the n-best order) ----
template <bool LM>
__global__ __launch_bounds__(64) void ctc_beam_commit_kernel(int* trie_parent, int* trie_label, int* trie_depth, CtcCarry cy,
                                                            const int32_t* __restrict__ fin, int32_t* __restrict__ committed,
                                                            int32_t* __restrict__ tokens, int32_t* __restrict__ ntokens, int W, int width,
                                                            long nmax, LmDev lmd) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nb = min(max(cy.cnt[b * CNT_N + CNT_LIVE], 0), W);
  const Trie tr = trie_at(trie_parent, trie_label, trie_depth, (long)b * nmax);
  const bool live = lane < nb;
  const long c0 = (long)b * W;
  const int node = live ? cy.node[c0 + lane] : 0;
  int best_lane = -1;
  if (nb > 0 && fin && fin[b]) best_lane = ctc_best_lane<LM>(tr, cy, c0, nb, lane, node, live, lmd, (long)b * nmax, nmax, true);
  commit_stream(tr, node, live, nb, best_lane, lane, committed + b, tokens + (long)b * width, ntokens + b, width, 0);
}

// ---- tfasr_ctc_beam_commit_horizon: the same, and at a prune point (beam_select.h) the rows that do not descend from the best row's
// deepest node older than the horizon leave the carried beam: the survivors move up in their order, the commit goes up to that node ----
template <bool LM>
__global__ __launch_bounds__(64) void ctc_beam_commit_horizon_kernel(int* trie_parent, int* trie_label, int* trie_depth, CtcCarry cy,
                                                                    const int32_t* __restrict__ fin, int32_t* __restrict__ committed,
                                                                    int32_t* __restrict__ tokens, int32_t* __restrict__ ntokens,
                                                                    int32_t* hstate, int H, int W, int width, long nmax, LmDev lmd) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int* cnt = cy.cnt + b * CNT_N;
  const int nb = min(max(cnt[CNT_LIVE], 0), W);
  const Trie tr = trie_at(trie_parent, trie_label, trie_depth, (long)b * nmax);
  const bool live = lane < nb;
  const long c0 = (long)b * W;
  const int node = live ? cy.node[c0 + lane] : 0;
  const int X = horizon_point(hstate + (long)b * horizon_stride(H), H, cnt, lane);
  const bool final = fin && fin[b];
  int best_lane = -1;
  if (nb > 0 && (final || X >= 0)) best_lane = ctc_best_lane<LM>(tr, cy, c0, nb, lane, node, live, lmd, (long)b * nmax, nmax, final);
  if (nb > 0 && !final && X >= 0) {
    int target = horizon_target(tr, __shfl(node, best_lane, 64), X);
    const int ca = beam_trie::common_ancestor(tr, node, live);
    if (tr.depth[target] > tr.depth[ca]) {
      const bool keep = live && descends_from(tr, node, target);
      const unsigned long long mask = __ballot(keep);
      const int par = live ? cy.par[c0 + lane] : 0, lab = live ? cy.lab[c0 + lane] : 0, dep = live ? cy.dep[c0 + lane] : 0;
      const float pb = live ? cy.pb[c0 + lane] : 0.f, pnb = live ? cy.pnb[c0 + lane] : 0.f;
      __syncthreads();  // (one wave: every row is read before any is written)
      if (keep) {
        const long q = c0 + __popcll(mask & ((1ull << lane) - 1ull));
        cy.node[q] = node; cy.par[q] = par; cy.lab[q] = lab; cy.dep[q] = dep; cy.pb[q] = pb; cy.pnb[q] = pnb;
      }
      if (lane == 0) cnt[CNT_LIVE] = __popcll(mask);
    } else {
      target = ca;
    }
    beam_trie::commit_labels(tr, target, lane, committed + b, tokens + (long)b * width, ntokens + b, width, 0);
    return;
  }
  commit_stream(tr, node, live, nb, final ? best_lane : -1, lane, committed + b, tokens + (long)b * width, ntokens + b, width, 0);
}

// ---- tfasr_ctc_beam_compact: one workgroup per stream named by `mask`.  The search tells "this row has a last label" by par >= 0 and
// finds a row's parent ROW by comparing par with the rows' nodes: a live row that is the new root keeps its last label, so its par is
// CTC_ROOT_PAR, a value no node id takes (ids stay below nmax < 2^28), unless the root is still the empty sequence (label -1) ----
constexpr int CTC_ROOT_PAR = 0x7fffffff;
// what a kept node takes along under LM fusion: lm of its sequence (the absolute sum from `start`, never rebased) and the LM state
struct LmPayload {
  static constexpr int WORDS = 2;
  float* node_lm;
  int* node_state;
  __device__ void get(int node, int* dst) const { dst[0] = __float_as_int(node_lm[node]); dst[1] = node_state[node]; }
  __device__ void put(int node, const int* src) const { node_lm[node] = __int_as_float(src[0]); node_state[node] = src[1]; }
};
template <bool LM>
__global__ __launch_bounds__(THREADS) void ctc_beam_compact_kernel(const int32_t* __restrict__ mask, int* trie_parent, int* trie_label,
                                                                   int* trie_depth, unsigned long long* hkeys, int* hvals, CtcCarry cy,
                                                                   int32_t* __restrict__ committed, int32_t* hstate, int H,
                                                                   int32_t* __restrict__ out, int W, long nmax, unsigned hcap,
                                                                   float* node_lm, int* node_state) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int* cnt = cy.cnt + b * CNT_N;
  if (!mask[b]) {
    if (tid == 0) { out[3 * b] = 0; out[3 * b + 1] = cnt[CNT_NODES]; out[3 * b + 2] = cnt[CNT_FRAMES]; }
    return;
  }
  const Trie tr = trie_at(trie_parent, trie_label, trie_depth, (long)b * nmax);
  const long c0 = (long)b * W;
  const int nb = min(max(cnt[CNT_LIVE], 0), W);
  auto node_at = [&](int i) { return cy.node[c0 + i]; };
  auto set_node = [&](int i, int n) {
    cy.node[c0 + i] = n; cy.lab[c0 + i] = tr.label[n]; cy.dep[c0 + i] = tr.depth[n];
    cy.par[c0 + i] = n > 0 ? tr.parent[n] : tr.label[0] >= 0 ? CTC_ROOT_PAR : -1;
  };
  int32_t* hs = hstate ? hstate + (long)b * horizon_stride(H) : nullptr;
  if constexpr (LM)
    compact_stream(tr, hkeys + (long)b * hcap, hvals + (long)b * hcap, hcap, cnt, nb, committed + b, hs, H, out + 3 * b, tid, node_at, set_node,
                   LmPayload{node_lm + (long)b * nmax, node_state + (long)b * nmax});
  else
    compact_stream(tr, hkeys + (long)b * hcap, hvals + (long)b * hcap, hcap, cnt, nb, committed + b, hs, H, out + 3 * b, tid, node_at, set_node);
}

struct BeamLayout : Geometry {
  size_t off_lse, off_lpb, off_tc, off_tlp, off_par, off_lab, off_dep, off_hk, off_hv, off_carry, total;
};

// C = frames per launch (the per-frame scratch), Tcap = frames per beam (the trie); the one-shot search has C = Tcap = T
inline BeamLayout beam_layout(int B, int C, int Tcap, int V, int W) {
  BeamLayout L{Geometry(Tcap, V, W)};
  const size_t rows = (size_t)B * C;
  size_t o = 0;
  L.off_lse = o; o += align256(rows * 4);
  L.off_lpb = o; o += align256(rows * 4);
  L.off_tc = o; o += align256(rows * L.K * 4);
  L.off_tlp = o; o += align256(rows * L.K * 4);
  L.off_par = o; o += align256((size_t)B * L.nmax * 4);
  L.off_lab = o; o += align256((size_t)B * L.nmax * 4);
  L.off_dep = o; o += align256((size_t)B * L.nmax * 4);
  L.off_hk = o; o += align256((size_t)B * L.hcap * 8);
  L.off_hv = o; o += align256((size_t)B * L.hcap * 4);
  L.off_carry = o; o += 6 * align256((size_t)B * W * 4) + align256((size_t)B * CNT_N * 4);
  L.total = o;
  return L;
}

struct BeamWs { float *lse, *lpb, *tlp; int32_t* tc; int *par, *lab, *dep, *hv; unsigned long long* hk; CtcCarry cy; };

inline BeamWs beam_carve(const BeamLayout& L, void* workspace, int B, int W) {
  char* ws = (char*)workspace;
  BeamWs w;
  w.lse = (float*)(ws + L.off_lse); w.lpb = (float*)(ws + L.off_lpb); w.tc = (int32_t*)(ws + L.off_tc); w.tlp = (float*)(ws + L.off_tlp);
  w.par = (int*)(ws + L.off_par); w.lab = (int*)(ws + L.off_lab); w.dep = (int*)(ws + L.off_dep);
  w.hk = (unsigned long long*)(ws + L.off_hk); w.hv = (int*)(ws + L.off_hv);
  const size_t a = align256((size_t)B * W * 4);
  char* c = ws + L.off_carry;
  w.cy = CtcCarry{(int*)c, (int*)(c + a), (int*)(c + 2 * a), (int*)(c + 3 * a), (float*)(c + 4 * a), (float*)(c + 5 * a), (int*)(c + 6 * a)};
  return w;
}

// the frame kernel over logits [B, C, V], then the search kernel: both searches, whole and in pieces
template <typename T, bool LM = false>
int beam_launch(const BeamLayout& L, const BeamWs& w, const void* logits, const int32_t* logit_len, int B, int C, int Tcap, int V, int W, int P,
                int blank, int mode, int OW, int32_t* tokens, int32_t* tokens_len, float* log_prob, hipStream_t s, const LmDev& lmd = LmDev{}) {
  if (logit_len) {
    const long rows = (long)B * C;
    const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
    TFASR_KLAUNCH(ctc_beam_frame_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)logits, logit_len, w.lse, w.lpb, w.tc, w.tlp, B, C, V, L.K, blank);
  }
  TFASR_KLAUNCH((ctc_beam_search_kernel<T, LM>), dim3(B), dim3(THREADS), 0, s, (const T*)logits, logit_len, w.lse, w.lpb, w.tc, w.tlp, w.par,
                w.lab, w.dep, w.hk, w.hv, C, V, W, L.K, P, L.nmax, L.hcap, tokens, tokens_len, log_prob, w.cy, mode, Tcap, OW, lmd);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

inline bool beam_shape_ok(int B, int T, int V, int W) { return B > 0 && shape_ok(T, V, W); }

}  // namespace

extern "C" int tfasr_ctc_beam_search_workspace_size(int B, int T, int V, int beam_width, size_t* bytes) {
  if (!bytes || !beam_shape_ok(B, T, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  *bytes = beam_layout(B, T, T, V, beam_width).total;
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_search(const void* logits, const int32_t* logit_len, int B, int T, int V, int beam_width, int top_paths,
                                     int blank_index, int dtype, int32_t* tokens, int32_t* tokens_len, float* log_prob, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
  if (!logits || !logit_len || !tokens || !tokens_len || !log_prob || !workspace) return TFASR_STATUS_INVALID_VALUE;
  if (!beam_shape_ok(B, T, V, beam_width) || top_paths < 1 || top_paths > beam_width || blank_index < 0 || blank_index >= V)
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  const BeamLayout L = beam_layout(B, T, T, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  hipStream_t s = (hipStream_t)stream_;
  // begin + all T frames + n-best in one launch of the kernel the chunked entries run
  if (dtype == TFASR_F32)
    return beam_launch<float>(L, w, logits, logit_len, B, T, T, V, beam_width, top_paths, blank_index, BEAM_OUTPUT, T, tokens, tokens_len, log_prob, s);
  return beam_launch<bf16_t>(L, w, logits, logit_len, B, T, T, V, beam_width, top_paths, blank_index, BEAM_OUTPUT, T, tokens, tokens_len, log_prob, s);
}

// ---- the fused search: the workspace of the plain search, then lm and LM state per trie node ----
namespace {
inline size_t lm_node_bytes(int B, const BeamLayout& L) { return align256((size_t)B * L.nmax * 4); }
}  // namespace

extern "C" int tfasr_ctc_beam_search_lm_workspace_size(int B, int T, int V, int beam_width, size_t* bytes) {
  if (!bytes || !beam_shape_ok(B, T, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  if (beam_width > TFASR_CTC_LM_MAX_BEAM) return TFASR_STATUS_UNSUPPORTED;
  const BeamLayout L = beam_layout(B, T, T, V, beam_width);
  *bytes = L.total + 2 * lm_node_bytes(B, L);
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_search_lm(const void* logits, const int32_t* logit_len, int B, int T, int V, int beam_width, int top_paths,
                                        int blank_index, int dtype, const tfasr_ngram_lm_t* lm, int32_t* tokens, int32_t* tokens_len,
                                        float* score, float* log_prob, float* lm_score, void* workspace, size_t workspace_bytes,
                                        void* stream_) {
  if (!logits || !logit_len || !tokens || !tokens_len || !score || !log_prob || !lm_score || !workspace || !ngram_lm::tables_ok(lm))
    return TFASR_STATUS_INVALID_VALUE;
  if (!beam_shape_ok(B, T, V, beam_width) || top_paths < 1 || top_paths > beam_width || blank_index < 0 || blank_index >= V)
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  // a frame's candidate list (W stays, <= 2W specials, W * K regulars) must fit the LDS arrays sized for the plain search
  static_assert(3 * TFASR_CTC_LM_MAX_BEAM + TFASR_CTC_LM_MAX_BEAM * 2 * TFASR_CTC_LM_MAX_BEAM <= BEAM_MAXC, "fused candidate list exceeds LDS");
  if (beam_width > TFASR_CTC_LM_MAX_BEAM) return TFASR_STATUS_UNSUPPORTED;
  const BeamLayout L = beam_layout(B, T, T, V, beam_width);
  const size_t nb = lm_node_bytes(B, L);
  if (workspace_bytes < L.total + 2 * nb) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  char* extra = (char*)workspace + L.total;
  const LmDev lmd{ngram_lm::tables_of(*lm), (float*)extra, (int*)(extra + nb), score, lm_score, nullptr, 1};
  hipStream_t s = (hipStream_t)stream_;
  if (dtype == TFASR_F32)
    return beam_launch<float, true>(L, w, logits, logit_len, B, T, T, V, beam_width, top_paths, blank_index, BEAM_OUTPUT, T, tokens, tokens_len,
                                    log_prob, s, lmd);
  return beam_launch<bf16_t, true>(L, w, logits, logit_len, B, T, T, V, beam_width, top_paths, blank_index, BEAM_OUTPUT, T, tokens, tokens_len,
                                   log_prob, s, lmd);
}

// ---- the search in pieces (streaming sessions).  The workspace (tfasr_ctc_beam_stream_workspace_size) IS the carried state of B
// streams: per-frame scratch for chunks of at most C frames, a trie for Tcap frames per stream, and the beam rows ----
namespace {
inline bool stream_shape_ok(int B, int C, int Tcap, int V, int W) { return beam_shape_ok(B, Tcap, V, W) && C >= 1 && C <= Tcap; }
}  // namespace

extern "C" int tfasr_ctc_beam_stream_workspace_size(int B, int C, int Tcap, int V, int beam_width, size_t* bytes) {
  if (!bytes || !stream_shape_ok(B, C, Tcap, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  *bytes = beam_layout(B, C, Tcap, V, beam_width).total;
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_reset(const int32_t* mask, int B, int C, int Tcap, int V, int beam_width, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
  if (!workspace || !stream_shape_ok(B, C, Tcap, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  const BeamLayout L = beam_layout(B, C, Tcap, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  TFASR_KLAUNCH(ctc_beam_reset_kernel<false>, dim3(B), dim3(THREADS), 0, (hipStream_t)stream_, mask, w.par, w.lab, w.dep, w.hk, w.cy,
                beam_width, L.nmax, L.hcap, (float*)nullptr, (int*)nullptr, 0);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_advance(const void* logits, const int32_t* nvalid, int B, int C, int Cn, int Tcap, int V, int beam_width,
                                      int blank_index, int dtype, int frames_max_after, void* workspace, size_t workspace_bytes,
                                      void* stream_) {
  // logits [B, Cn, V], Cn <= C (the chunk capacity the workspace was sized with)
  if (!logits || !nvalid || !workspace || !stream_shape_ok(B, C, Tcap, V, beam_width) || Cn < 1 || Cn > C || blank_index < 0 ||
      blank_index >= V || frames_max_after < 0 || frames_max_after > Tcap)
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  const BeamLayout L = beam_layout(B, C, Tcap, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  hipStream_t s = (hipStream_t)stream_;
  const int mode = BEAM_LOAD | BEAM_STORE;
  if (dtype == TFASR_F32)
    return beam_launch<float>(L, w, logits, nvalid, B, Cn, Tcap, V, beam_width, 1, blank_index, mode, 1, nullptr, nullptr, nullptr, s);
  return beam_launch<bf16_t>(L, w, logits, nvalid, B, Cn, Tcap, V, beam_width, 1, blank_index, mode, 1, nullptr, nullptr, nullptr, s);
}

extern "C" int tfasr_ctc_beam_commit(const int32_t* final_mask, int32_t* committed, int32_t* tokens, int32_t* ntokens, int B, int C, int Tcap,
                                     int V, int beam_width, int width, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!committed || !tokens || !ntokens || !workspace || !stream_shape_ok(B, C, Tcap, V, beam_width) || width < 1)
    return TFASR_STATUS_INVALID_VALUE;
  const BeamLayout L = beam_layout(B, C, Tcap, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  TFASR_KLAUNCH(ctc_beam_commit_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream_, w.par, w.lab, w.dep, w.cy, final_mask, committed,
                tokens, ntokens, beam_width, width, L.nmax, LmDev{});
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_nbest(int B, int C, int Tcap, int V, int beam_width, int top_paths, int width, int32_t* tokens,
                                    int32_t* tokens_len, float* log_prob, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!tokens || !tokens_len || !log_prob || !workspace || !stream_shape_ok(B, C, Tcap, V, beam_width) || top_paths < 1 ||
      top_paths > beam_width || width < 1 || width > Tcap)
    return TFASR_STATUS_INVALID_VALUE;
  const BeamLayout L = beam_layout(B, C, Tcap, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  // the search kernel over zero frames: load the beam, rank it, write the paths
  return beam_launch<float>(L, w, nullptr, nullptr, B, C, Tcap, V, beam_width, top_paths, 0, BEAM_LOAD | BEAM_OUTPUT, width, tokens, tokens_len,
                            log_prob, (hipStream_t)stream_);
}

// ---- the commit horizon and the compaction: the horizon state [B, 4 + 2 (horizon + 1)] int32 is the caller's ----
extern "C" int tfasr_ctc_beam_commit_horizon(const int32_t* final_mask, int32_t* committed, int32_t* tokens, int32_t* ntokens,
                                             int32_t* horizon_state, int horizon, int B, int C, int Tcap, int V, int beam_width, int width,
                                             void* workspace, size_t workspace_bytes, void* stream_) {
  if (!committed || !tokens || !ntokens || !horizon_state || !workspace || !stream_shape_ok(B, C, Tcap, V, beam_width) || width < 1 ||
      horizon < 1 || horizon > TFASR_BEAM_MAX_HORIZON)
    return TFASR_STATUS_INVALID_VALUE;
  const BeamLayout L = beam_layout(B, C, Tcap, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  TFASR_KLAUNCH(ctc_beam_commit_horizon_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream_, w.par, w.lab, w.dep, w.cy, final_mask,
                committed, tokens, ntokens, horizon_state, horizon, beam_width, width, L.nmax, LmDev{});
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_compact(const int32_t* mask, int32_t* committed, int32_t* horizon_state, int horizon, int32_t* out, int B, int C,
                                      int Tcap, int V, int beam_width, void* workspace, size_t workspace_bytes, void* stream_) {
  // horizon_state NULL (then horizon must be 0): a stream that never ran a horizon commit
  if (!mask || !committed || !out || !workspace || !stream_shape_ok(B, C, Tcap, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  if (horizon_state ? (horizon < 1 || horizon > TFASR_BEAM_MAX_HORIZON) : horizon != 0) return TFASR_STATUS_INVALID_VALUE;
  const BeamLayout L = beam_layout(B, C, Tcap, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  const BeamWs w = beam_carve(L, workspace, B, beam_width);
  TFASR_KLAUNCH(ctc_beam_compact_kernel<false>, dim3(B), dim3(THREADS), 0, (hipStream_t)stream_, mask, w.par, w.lab, w.dep, w.hk, w.hv, w.cy,
                committed, horizon_state, horizon, out, beam_width, L.nmax, L.hcap, (float*)nullptr, (int*)nullptr);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

// ---- the fused search in pieces (tfasr_ctc_beam_lm_*): the entries above on the LM = true instantiations.  The workspace is the plain
// stream layout, then lm and LM state per trie node; a beam row carries no LM values of its own (it reads its node's) ----
namespace {
struct LmStreamWs { BeamLayout L{Geometry(1, 2, 1)}; BeamWs w; float* node_lm; int* node_state; };

// the checks every fused stream entry shares -> SUCCESS and the carved workspace
inline int lm_stream_ws(int B, int C, int Tcap, int V, int W, void* workspace, size_t workspace_bytes, LmStreamWs* out) {
  if (!workspace || !stream_shape_ok(B, C, Tcap, V, W)) return TFASR_STATUS_INVALID_VALUE;
  if (W > TFASR_CTC_LM_MAX_BEAM) return TFASR_STATUS_UNSUPPORTED;
  out->L = beam_layout(B, C, Tcap, V, W);
  const size_t nb = lm_node_bytes(B, out->L);
  if (workspace_bytes < out->L.total + 2 * nb) return TFASR_STATUS_INVALID_VALUE;
  out->w = beam_carve(out->L, workspace, B, W);
  char* extra = (char*)workspace + out->L.total;
  out->node_lm = (float*)extra;
  out->node_state = (int*)(extra + nb);
  return TFASR_STATUS_SUCCESS;
}
}  // namespace

extern "C" int tfasr_ctc_beam_lm_stream_workspace_size(int B, int C, int Tcap, int V, int beam_width, size_t* bytes) {
  if (!bytes || !stream_shape_ok(B, C, Tcap, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  if (beam_width > TFASR_CTC_LM_MAX_BEAM) return TFASR_STATUS_UNSUPPORTED;
  const BeamLayout L = beam_layout(B, C, Tcap, V, beam_width);
  *bytes = L.total + 2 * lm_node_bytes(B, L);
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_lm_reset(const int32_t* mask, int B, int C, int Tcap, int V, int beam_width, const tfasr_ngram_lm_t* lm,
                                       void* workspace, size_t workspace_bytes, void* stream_) {
  if (!ngram_lm::tables_ok(lm)) return TFASR_STATUS_INVALID_VALUE;
  LmStreamWs x;
  if (const int st = lm_stream_ws(B, C, Tcap, V, beam_width, workspace, workspace_bytes, &x)) return st;
  TFASR_KLAUNCH(ctc_beam_reset_kernel<true>, dim3(B), dim3(THREADS), 0, (hipStream_t)stream_, mask, x.w.par, x.w.lab, x.w.dep, x.w.hk, x.w.cy,
                beam_width, x.L.nmax, x.L.hcap, x.node_lm, x.node_state, (int)lm->start);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_lm_advance(const void* logits, const int32_t* nvalid, int B, int C, int Cn, int Tcap, int V, int beam_width,
                                         int blank_index, int dtype, int frames_max_after, const tfasr_ngram_lm_t* lm, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
  if (!logits || !nvalid || !ngram_lm::tables_ok(lm) || Cn < 1 || Cn > C || blank_index < 0 || blank_index >= V || frames_max_after < 0 ||
      frames_max_after > Tcap)
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  LmStreamWs x;
  if (const int st = lm_stream_ws(B, C, Tcap, V, beam_width, workspace, workspace_bytes, &x)) return st;
  const LmDev lmd{ngram_lm::tables_of(*lm), x.node_lm, x.node_state, nullptr, nullptr, nullptr, 0};
  hipStream_t s = (hipStream_t)stream_;
  const int mode = BEAM_LOAD | BEAM_STORE;
  if (dtype == TFASR_F32)
    return beam_launch<float, true>(x.L, x.w, logits, nvalid, B, Cn, Tcap, V, beam_width, 1, blank_index, mode, 1, nullptr, nullptr, nullptr, s,
                                    lmd);
  return beam_launch<bf16_t, true>(x.L, x.w, logits, nvalid, B, Cn, Tcap, V, beam_width, 1, blank_index, mode, 1, nullptr, nullptr, nullptr, s,
                                   lmd);
}

extern "C" int tfasr_ctc_beam_lm_commit(const int32_t* final_mask, int32_t* committed, int32_t* tokens, int32_t* ntokens, int B, int C,
                                        int Tcap, int V, int beam_width, int width, const tfasr_ngram_lm_t* lm, void* workspace,
                                        size_t workspace_bytes, void* stream_) {
  if (!committed || !tokens || !ntokens || !ngram_lm::tables_ok(lm) || width < 1) return TFASR_STATUS_INVALID_VALUE;
  LmStreamWs x;
  if (const int st = lm_stream_ws(B, C, Tcap, V, beam_width, workspace, workspace_bytes, &x)) return st;
  const LmDev lmd{ngram_lm::tables_of(*lm), x.node_lm, x.node_state, nullptr, nullptr, final_mask, 0};
  TFASR_KLAUNCH(ctc_beam_commit_kernel<true>, dim3(B), dim3(64), 0, (hipStream_t)stream_, x.w.par, x.w.lab, x.w.dep, x.w.cy, final_mask,
                committed, tokens, ntokens, beam_width, width, x.L.nmax, lmd);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_lm_commit_horizon(const int32_t* final_mask, int32_t* committed, int32_t* tokens, int32_t* ntokens,
                                                int32_t* horizon_state, int horizon, int B, int C, int Tcap, int V, int beam_width, int width,
                                                const tfasr_ngram_lm_t* lm, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!committed || !tokens || !ntokens || !horizon_state || !ngram_lm::tables_ok(lm) || width < 1 || horizon < 1 ||
      horizon > TFASR_BEAM_MAX_HORIZON)
    return TFASR_STATUS_INVALID_VALUE;
  LmStreamWs x;
  if (const int st = lm_stream_ws(B, C, Tcap, V, beam_width, workspace, workspace_bytes, &x)) return st;
  const LmDev lmd{ngram_lm::tables_of(*lm), x.node_lm, x.node_state, nullptr, nullptr, final_mask, 0};
  TFASR_KLAUNCH(ctc_beam_commit_horizon_kernel<true>, dim3(B), dim3(64), 0, (hipStream_t)stream_, x.w.par, x.w.lab, x.w.dep, x.w.cy, final_mask,
                committed, tokens, ntokens, horizon_state, horizon, beam_width, width, x.L.nmax, lmd);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_lm_compact(const int32_t* mask, int32_t* committed, int32_t* horizon_state, int horizon, int32_t* out, int B,
                                         int C, int Tcap, int V, int beam_width, void* workspace, size_t workspace_bytes, void* stream_) {
  // (no tables: the per-node lm and state move as they are)
  if (!mask || !committed || !out) return TFASR_STATUS_INVALID_VALUE;
  if (horizon_state ? (horizon < 1 || horizon > TFASR_BEAM_MAX_HORIZON) : horizon != 0) return TFASR_STATUS_INVALID_VALUE;
  LmStreamWs x;
  if (const int st = lm_stream_ws(B, C, Tcap, V, beam_width, workspace, workspace_bytes, &x)) return st;
  TFASR_KLAUNCH(ctc_beam_compact_kernel<true>, dim3(B), dim3(THREADS), 0, (hipStream_t)stream_, mask, x.w.par, x.w.lab, x.w.dep, x.w.hk, x.w.hv,
                x.w.cy, committed, horizon_state, horizon, out, beam_width, x.L.nmax, x.L.hcap, x.node_lm, x.node_state);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_beam_lm_nbest(const int32_t* final_mask, int B, int C, int Tcap, int V, int beam_width, int top_paths, int width,
                                       int32_t* tokens, int32_t* tokens_len, float* score, float* log_prob, float* lm_score,
                                       const tfasr_ngram_lm_t* lm, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!tokens || !tokens_len || !score || !log_prob || !lm_score || !ngram_lm::tables_ok(lm) || top_paths < 1 || top_paths > beam_width ||
      width < 1 || width > Tcap)
    return TFASR_STATUS_INVALID_VALUE;
  LmStreamWs x;
  if (const int st = lm_stream_ws(B, C, Tcap, V, beam_width, workspace, workspace_bytes, &x)) return st;
  const LmDev lmd{ngram_lm::tables_of(*lm), x.node_lm, x.node_state, score, lm_score, final_mask, 0};
  // the search kernel over zero frames: load the beam, rank it by the fused score, write the paths
  return beam_launch<float, true>(x.L, x.w, nullptr, nullptr, B, C, Tcap, V, beam_width, top_paths, 0, BEAM_LOAD | BEAM_OUTPUT, width, tokens,
                                  tokens_len, log_prob, (hipStream_t)stream_, lmd);
}
