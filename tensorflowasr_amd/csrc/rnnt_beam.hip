// Transducer beam search on the device (ConformerTransducer.recognize_beam(device_search=True), recognize_nbest): the batched
// "modified beam search" - at most one symbol per frame, candidates with equal label sequences merged (log-add-exp of their
// totals), the next beam = the first W candidates by (total desc, label sequence asc).  The reference's own recognize_beam is a
// TODO that returns the greedy result (base_transducer.py:841-842); its commented-out Graves loop (:844-1083) is not reproduced.
//
// Beam of utterance b = rows b*W .. b*W+W-1 of the workspace, best first; rows past the live count have total -inf.  A row holds
// its label sequence (a trie node), its total (f64), its last token and the prediction state BEFORE that token was fed (the greedy
// search's continuation convention), plus the state after it and its prediction projection.  One frame t:
//   rb_join_kernel   z = tanh(encj[b, t] + pred[row])                                             (every row of a live utterance)
//   tfasr_gemm       logits = z @ vocab_w + vocab_b, exact f32 on the matrix cores
//   rb_frame_kernel  one wave per live row: beam_select.h's frame pass in f64, lp = (double)x - (double)lse
//   rb_select_kernel one workgroup per utterance: beam_select.h's selection over at most W^2 + 2W candidates - the classes special to
//                    a row are its merge targets (the labels of the beam rows whose parent it is) - and the gather of the next
//                    rows' pre-states (extension: the parent's post-state; stay and merge: the row's own pre-state)
//   prediction step  h_pre @ lstm_rk (tfasr_gemm) -> rb_cell_kernel (+ G[token] + b, LSTM cell, LayerNorm) -> @ joint_pred_w + b
// The prediction step runs for every row; a stay row recomputes its post-state and projection from unchanged inputs, and the f32
// GEMM's k order per element does not depend on the row's position (split_k 1): the same bits as the cached values.
// The search in pieces (tfasr_rnnt_beam_reset / _advance / _commit / _nbest_states, streaming sessions): the workspace sized with
// T = Tcap is the carried state of B streams, rb_frames is the one frame loop (the one-shot search = begin + rb_frames over all T
// frames + n-best).  Between two advances a beam is what the select leaves - node, total, token, gathered pre-state - and the
// advance starts with the prediction step, which rebuilds the rest with the same bits.  tfasr_rnnt_beam_commit_horizon (which moves
// exactly those four when it drops rows) and tfasr_rnnt_beam_compact are the commit horizon and the trie compaction of DESIGN.md 4a.
// Arithmetic: products f32 on the f32 master weights; totals, merges (max + log1p(exp(-|a-b|))) and comparisons f64; scores f32.
#include "beam_select.h"
#include <string.h>

namespace {

using namespace beam_select;

constexpr int RB_MAXC = MAXW * MAXW + 2 * MAXW;  // stays + specials (< W) + W regulars per row

struct Ws {  // the workspace carved into its arrays (rb_layout)
  float *G, *hpre, *cpre, *hnx, *cnx, *hpost, *cpost, *y, *hr, *pred, *z, *logits, *lse;
  double *lpb, *tlp, *tot;
  int *tc, *node, *tok, *cnt, *par, *lab, *dep, *hv;
  unsigned long long* hk;
};

struct RbLayout : Geometry {
  size_t off[24], total;
};

inline RbLayout rb_layout(int B, int T, int U, int J, int V, int W) {
  RbLayout L{Geometry(T, V, W)};
  const size_t R = (size_t)B * W;
  const size_t sz[24] = {(size_t)V * 4 * U * 4,                                               // G = emb @ lstm_k (no `packed`)
                         R * U * 4, R * U * 4, R * U * 4, R * U * 4, R * U * 4, R * U * 4, R * U * 4,  // hpre cpre hnx cnx hpost cpost y
                         R * 4 * U * 4, R * J * 4, R * J * 4, R * V * 4, R * 4,              // hr pred z logits lse
                         R * 8, R * L.K * 8, R * 8,                                             // lpb tlp tot
                         R * L.K * 4, R * 4, R * 4, (size_t)B * CNT_N * 4,                      // tc node tok cnt
                         (size_t)B * L.nmax * 4, (size_t)B * L.nmax * 4, (size_t)B * L.nmax * 4,  // trie parent label depth
                         (size_t)B * L.hcap * 4 + (size_t)B * L.hcap * 8};                     // table values + keys
  size_t o = 0;
  for (int i = 0; i < 24; ++i) { L.off[i] = o; o += align256(sz[i]); }
  L.total = o;
  return L;
}

inline Ws rb_carve(const RbLayout& L, void* ws, int B) {
  char* w = (char*)ws;
  Ws s;
  float** f[13] = {&s.G, &s.hpre, &s.cpre, &s.hnx, &s.cnx, &s.hpost, &s.cpost, &s.y, &s.hr, &s.pred, &s.z, &s.logits, &s.lse};
  for (int i = 0; i < 13; ++i) *f[i] = (float*)(w + L.off[i]);
  s.lpb = (double*)(w + L.off[13]); s.tlp = (double*)(w + L.off[14]); s.tot = (double*)(w + L.off[15]);
  s.tc = (int*)(w + L.off[16]); s.node = (int*)(w + L.off[17]); s.tok = (int*)(w + L.off[18]); s.cnt = (int*)(w + L.off[19]);
  s.par = (int*)(w + L.off[20]); s.lab = (int*)(w + L.off[21]); s.dep = (int*)(w + L.off[22]);
  s.hv = (int*)(w + L.off[23]);
  s.hk = (unsigned long long*)(w + L.off[23] + align256((size_t)B * L.hcap * 4));
  return s;
}

inline bool rb_shape_ok(int B, int T, int U, int J, int V, int W) {
  return B > 0 && U > 0 && J > 0 && shape_ok(T, V, W) && (long)B * W < (1L << 22);
}

// ---- one empty hypothesis per utterance: row b*W = (empty sequence, total 0, initial token), the other rows dead; the initial
// state goes to every row's gather slot (hnx / cnx) when the caller runs the prediction network.  `mask` [B] (optional) names the
// utterances to begin: the others are not touched ----
__global__ __launch_bounds__(THREADS) void rb_begin_kernel(const int32_t* __restrict__ init_tok, const float* __restrict__ init_h,
                                                          const float* __restrict__ init_c, const int32_t* __restrict__ mask, Ws s,
                                                          int W, int U, int blank, long nmax, unsigned hcap, bool state) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (mask && !mask[b]) return;  // (tfasr_rnnt_beam_reset: the other streams keep their beams)
  for (int i = tid; i < W; i += THREADS) {
    const long r = (long)b * W + i;
    s.node[r] = 0;
    s.tot[r] = i == 0 ? 0.0 : -INFINITY;
    s.tok[r] = init_tok ? init_tok[b] : blank;
  }
  clear_stream(trie_at(s.par, s.lab, s.dep, (long)b * nmax), s.hk + (long)b * hcap, hcap, tid);
  if (tid == 0) {
    int* cnt = s.cnt + b * CNT_N;
    cnt[CNT_LIVE] = 1; cnt[CNT_NODES] = 1; cnt[CNT_FRAMES] = 0;
  }
  if (state)
    for (long e = tid; e < (long)W * U; e += THREADS) {
      const int u = (int)(e % U);
      const long r = (long)b * W + e / U;
      s.hnx[r * U + u] = init_h ? init_h[(long)b * U + u] : 0.f;
      s.cnx[r * U + u] = init_c ? init_c[(long)b * U + u] : 0.f;
    }
}

// ---- LSTM cell + LayerNorm of one row per workgroup: z = (G[tok] + h_pre @ lstm_rk) + b (gate order i, f, c, o), the pre-state
// moves from the gather slot to hpre / cpre, y = LN(h_post) (or h_post) feeds the prediction projection ----
__global__ __launch_bounds__(THREADS) void rb_cell_kernel(const float* __restrict__ G, int g_packed, const float* __restrict__ bias,
                                                         const float* __restrict__ ln_g, const float* __restrict__ ln_b, Ws s, int U,
                                                         int V, float ln_eps) {
  __shared__ float red[THREADS / 64];
  const long r = blockIdx.x;
  const int tid = threadIdx.x;
  const int tok = min(max(s.tok[r], 0), V - 1);
  const float* hr = s.hr + r * 4 * U;
  float part = 0.f;
  for (int u = tid; u < U; u += THREADS) {
    float g4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)  // packed: decode_pack's G tiles, [V][U/4][16] with column (u % 4) * 4 + q inside a tile
      g4[q] = g_packed ? G[((long)tok * (U / 4) + u / 4) * 16 + (u % 4) * 4 + q] : G[(long)tok * 4 * U + q * U + u];
    const float zi = (g4[0] + hr[0 * U + u]) + bias[0 * U + u], zf = (g4[1] + hr[1 * U + u]) + bias[1 * U + u];
    const float zg = (g4[2] + hr[2 * U + u]) + bias[2 * U + u], zo = (g4[3] + hr[3 * U + u]) + bias[3 * U + u];
    const float ig = sigmoidf_(zi), fg = sigmoidf_(zf), gg = tanh_fast(zg), og = sigmoidf_(zo);
    const float hp = s.hnx[r * U + u], cp = s.cnx[r * U + u];
    const float cn = fg * cp + ig * gg, hn = og * tanh_fast(cn);
    s.hpre[r * U + u] = hp; s.cpre[r * U + u] = cp;
    s.hpost[r * U + u] = hn; s.cpost[r * U + u] = cn;
    if (ln_g) part += hn; else s.y[r * U + u] = hn;
  }
  if (!ln_g) return;
  // keras LayerNormalization: the mean, then the centred second moment
  auto block_sum = [&](float v) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) t += red[w];
    return t;
  };
  const float mu = block_sum(part) / U;
  part = 0.f;
  for (int u = tid; u < U; u += THREADS) { const float d = s.hpost[r * U + u] - mu; part += d * d; }
  const float rs = rsqrtf(block_sum(part) / U + ln_eps);
  for (int u = tid; u < U; u += THREADS) s.y[r * U + u] = (s.hpost[r * U + u] - mu) * rs * ln_g[u] + ln_b[u];
}

// ---- z = tanh(encj[b, t] + pred[row]) for the rows of utterances that still have frame t (TransducerJointMerge add + tanh); C = the
// frames per utterance of encj (the whole utterance, or one chunk of it) ----
__global__ __launch_bounds__(256) void rb_join_kernel(const float* __restrict__ encj, const int32_t* __restrict__ nframes, Ws s, int B, int C,
                                                     int J, int W, int t) {
  const long n = (long)B * W * J;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const long r = e / J;
    const int j = (int)(e % J), b = (int)(r / W);
    if (t >= nframes[b]) continue;
    s.z[e] = tanhf(encj[((long)b * C + t) * J + j] + s.pred[e]);
  }
}

__device__ __forceinline__ bool utt_active(const int32_t* nframes, const int* cnt, int b, int t, int T) {
  return t < nframes[b] && cnt[b * CNT_N + CNT_FRAMES] < T;  // (a frame is selected at most T times: the trie holds T*W + 1 nodes)
}
// ---- one wave per live row of a live utterance: lse, lp(blank), top K non-blank classes ----
__global__ __launch_bounds__(256) void rb_frame_kernel(const float* __restrict__ logits, const int32_t* __restrict__ nframes, Ws s, int B,
                                                      int T, int V, int W, int K, int blank, int t) {
  const int lane = threadIdx.x & 63;
  const long rows = (long)B * W;
  const long w0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (long)gridDim.x * (blockDim.x >> 6);
  for (long r = w0; r < rows; r += nw) {
    const int b = (int)(r / W), i = (int)(r % W);
    if (!utt_active(nframes, s.cnt, b, t, T) || i >= s.cnt[b * CNT_N + CNT_LIVE]) continue;
    const float* row = logits + r * V;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    double sum = 0.0;
    for (int v = lane; v < V; v += 64) sum += exp((double)row[v] - (double)m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float lz = m + (float)log(sum);
    // K rounds of a wave arg-max, each restricted to the classes after the previous winner in (lp desc, class asc) order
    double plp = INFINITY;
    int pc = -1;
    for (int k = 0; k < K; ++k) {
      double bl = -INFINITY;
      int bc = 0x7fffffff;
      for (int v = lane; v < V; v += 64) {
        if (v == blank) continue;
        const double l = (double)row[v] - (double)lz;
        if (cls_before(plp, pc, l, v) && cls_before(l, v, bl, bc)) { bl = l; bc = v; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ol = __shfl_xor(bl, o, 64);
        const int oc = __shfl_xor(bc, o, 64);
        if (cls_before(ol, oc, bl, bc)) { bl = ol; bc = oc; }
      }
      if (lane == 0) { s.tc[r * K + k] = min(bc, V - 1); s.tlp[r * K + k] = bl; }  // clamp: only NaN rows leave bc unset
      plp = bl;
      pc = bc;
    }
    if (lane == 0) { s.lse[r] = lz; s.lpb[r] = (double)row[blank] - (double)lz; }
  }
}

// ---- the next beam of one utterance ----
__global__ __launch_bounds__(THREADS) void rb_select_kernel(const float* __restrict__ logits, const int32_t* __restrict__ nframes, Ws s,
                                                           int T, int U, int V, int W, int K, int t, long nmax, unsigned hcap, bool state) {
  __shared__ int bnode[MAXW], btok[MAXW], merged[MAXW], win[MAXW];
  __shared__ int nnode[MAXW], npar[MAXW], nlab[MAXW], ndep[MAXW], ntok[MAXW], nsrc[MAXW];
  __shared__ double btot[MAXW], bstay[MAXW], ntot[MAXW];
  __shared__ double ctot[RB_MAXC];
  __shared__ unsigned ccode[RB_MAXC];
  __shared__ int s_nc;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (!utt_active(nframes, s.cnt, b, t, T)) return;
  int* cnt = s.cnt + b * CNT_N;
  const int nb = cnt[CNT_LIVE];
  const long r0 = (long)b * W;
  const Trie tr = trie_at(s.par, s.lab, s.dep, (long)b * nmax);
  unsigned long long* hk = s.hk + (long)b * hcap;
  int* hv = s.hv + (long)b * hcap;
  if (tid < nb) {
    bnode[tid] = s.node[r0 + tid];
    btok[tid] = s.tok[r0 + tid];
    btot[tid] = s.tot[r0 + tid];
    bstay[tid] = btot[tid] + s.lpb[r0 + tid];
  }
  if (tid == 0) s_nc = 0;
  __syncthreads();
  if (tid < nb) {  // the row whose sequence is this row's minus its last label (sequences of the beam are distinct: at most one)
    int m = -1;
    const int pn = tr.parent[bnode[tid]];
    for (int j = 0; j < nb && pn >= 0; ++j)
      if (bnode[j] == pn) m = j;
    merged[tid] = m;
  }
  __syncthreads();
  // --- stays that no extension reaches, and the merged pairs (stay of i + extension of its parent row p by i's last label)
  if (tid < nb) {
    const int p = merged[tid];
    double tot;
    unsigned code;
    if (p < 0) {
      tot = bstay[tid];
      code = cand_code(tid, -1);
    } else {
      const int c = tr.label[bnode[tid]];
      const double ext = btot[p] + ((double)logits[(r0 + p) * V + c] - (double)s.lse[r0 + p]);
      tot = lae(ext, bstay[tid]);
      code = cand_code(p, c);
    }
    const int q = atomicAdd(&s_nc, 1);
    ctot[q] = tot;
    ccode[q] = code;
  }
  // --- regulars: wave per row; special to row p = its merge targets
  for (int p = wid; p < nb; p += THREADS / 64)
    push_regulars(p, btot[p], s.tc + (r0 + p) * K, s.tlp + (r0 + p) * K, K, W, lane, [&](int c) {
      bool special = false;
      for (int j = 0; j < nb && !special; ++j) special = merged[j] == p && tr.label[bnode[j]] == c;
      return special;
    }, ctot, ccode, &s_nc);
  __syncthreads();
  const int nc = s_nc, keep = min(W, nc);
  rank_candidates(ctot, ccode, nc, keep, bnode, tr, win, tid);
  __syncthreads();
  // --- the next rows: sequence node, token, state source (row | 64 = the parent's post-state, else the row's pre-state)
  bool fresh = false;
  if (tid < keep) {
    const unsigned code = ccode[win[tid]];
    const int i = cand_row(code), c = cand_label(code);
    ntot[tid] = ctot[win[tid]];
    int child = -1;
    if (c >= 0)
      for (int k = 0; k < nb; ++k)
        if (merged[k] == i && tr.label[bnode[k]] == c) child = k;
    if (c < 0 || child >= 0) {  // a stay, or an extension merged with the stay of the row that holds its sequence
      const int k = c < 0 ? i : child;
      nnode[tid] = bnode[k]; ntok[tid] = btok[k]; nsrc[tid] = k;
    } else {
      npar[tid] = bnode[i]; nlab[tid] = c; ndep[tid] = tr.depth[bnode[i]] + 1;
      ntok[tid] = c; nsrc[tid] = i | 64;
      const int node = beam_trie::lookup(hk, hv, hcap, bnode[i], c);
      nnode[tid] = node;
      fresh = node < 0;
    }
  }
  const int nfresh = grow_trie(fresh, tid, cnt + CNT_NODES, tr, hk, hv, hcap, nnode, npar, nlab, ndep);
  __syncthreads();
  if (tid < W) {
    const bool live = tid < keep;
    s.node[r0 + tid] = live ? nnode[tid] : 0;
    s.tot[r0 + tid] = live ? ntot[tid] : -INFINITY;
    if (live) s.tok[r0 + tid] = ntok[tid];
  }
  if (tid == 0) {
    cnt[CNT_LIVE] = keep;
    cnt[CNT_NODES] += nfresh;
    cnt[CNT_FRAMES] += 1;
  }
  if (state)  // gather: the prediction step of the next frame reads the new rows' pre-states from hnx / cnx
    for (long e = tid; e < (long)keep * U; e += THREADS) {
      const int q = (int)(e / U), u = (int)(e % U), src = nsrc[q];
      const long from = (r0 + (src & 63)) * U + u, to = (r0 + q) * U + u;
      s.hnx[to] = (src & 64) ? s.hpost[from] : s.hpre[from];
      s.cnx[to] = (src & 64) ? s.cpost[from] : s.cpre[from];
    }
}

// ---- the best P rows of every utterance: tokens [B,P,T] (blank padded), lengths, f32 scores, and the continuation (last token,
// pre-state) when asked for ----
__global__ __launch_bounds__(THREADS) void rb_nbest_kernel(Ws s, int T, int U, int W, int P, int blank, long nmax,
                                                          int32_t* __restrict__ tokens, int32_t* __restrict__ tokens_len,
                                                          float* __restrict__ score, int32_t* __restrict__ next_tok,
                                                          float* __restrict__ next_h, float* __restrict__ next_c) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nb = s.cnt[b * CNT_N + CNT_LIVE];
  const long r0 = (long)b * W, o0 = (long)b * P;
  for (int p = tid; p < P; p += THREADS) {
    const bool live = p < nb;
    score[o0 + p] = live ? (float)s.tot[r0 + p] : -INFINITY;
    if (next_tok) next_tok[o0 + p] = live ? s.tok[r0 + p] : blank;
  }
  if (next_h)
    for (long e = tid; e < (long)P * U; e += THREADS) {
      const int p = (int)(e / U);
      const bool live = p < nb;
      next_h[o0 * U + e] = live ? s.hnx[r0 * U + e] : 0.f;  // (row p of the beam = element e of rows r0 ..)
      next_c[o0 * U + e] = live ? s.cnx[r0 * U + e] : 0.f;
    }
  write_paths(trie_at(s.par, s.lab, s.dep, (long)b * nmax), nb, P, T, blank, tid, [&](int p) { return s.node[r0 + p]; }, tokens + o0 * T,
              tokens_len + o0);
}

// ---- tfasr_rnnt_beam_commit: one wave per stream, a lane per live row ----
__global__ __launch_bounds__(64) void rb_commit_kernel(Ws s, const int32_t* __restrict__ fin, int32_t* __restrict__ committed,
                                                      int32_t* __restrict__ tokens, int32_t* __restrict__ ntokens, int W, int width, int blank,
                                                      long nmax) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nb = min(s.cnt[b * CNT_N + CNT_LIVE], W);
  const bool live = lane < nb;
  const int node = live ? s.node[(long)b * W + lane] : 0;
  // (rows are kept best first: a final stream commits row 0)
  commit_stream(trie_at(s.par, s.lab, s.dep, (long)b * nmax), node, live, nb, fin && fin[b] ? 0 : -1, lane, committed + b,
                tokens + (long)b * width, ntokens + b, width, blank);
}

// ---- tfasr_rnnt_beam_commit_horizon: the same, and at a prune point (beam_select.h) the rows that do not descend from the deepest
// node of row 0 (the best) older than the horizon leave the beam: the survivors move up in their order (node, total, token and the
// gathered pre-state, all a beam holds between two advances), the freed rows become dead rows as the select leaves them ----
__global__ __launch_bounds__(64) void rb_commit_horizon_kernel(Ws s, const int32_t* __restrict__ fin, int32_t* __restrict__ committed,
                                                              int32_t* __restrict__ tokens, int32_t* __restrict__ ntokens, int32_t* hstate,
                                                              int H, int W, int U, int width, int blank, long nmax) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int* cnt = s.cnt + b * CNT_N;
  const int nb = min(max(cnt[CNT_LIVE], 0), W);
  const bool live = lane < nb;
  const long r0 = (long)b * W;
  const int node = live ? s.node[r0 + lane] : 0;
  const Trie tr = trie_at(s.par, s.lab, s.dep, (long)b * nmax);
  const int X = horizon_point(hstate + (long)b * horizon_stride(H), H, cnt, lane);
  const bool final = fin && fin[b];
  if (nb > 0 && !final && X >= 0) {
    int target = horizon_target(tr, __shfl(node, 0, 64), X);
    const int ca = beam_trie::common_ancestor(tr, node, live);
    if (tr.depth[target] > tr.depth[ca]) {
      const bool keep = live && descends_from(tr, node, target);
      const unsigned long long mask = __ballot(keep);
      const int nk = __popcll(mask);
      const double tot = live ? s.tot[r0 + lane] : 0.0;
      const int tok = live ? s.tok[r0 + lane] : 0;
      __syncthreads();  // (one wave: every row is read before any is written)
      if (keep) {
        const long q = r0 + __popcll(mask & ((1ull << lane) - 1ull));
        s.node[q] = node; s.tot[q] = tot; s.tok[q] = tok;
      }
      if (lane >= nk && lane < W) { s.node[r0 + lane] = 0; s.tot[r0 + lane] = -INFINITY; }
      // pre-states: destination q <= source, in rising order, every lane its own columns: a source row is read before it is overwritten
      unsigned long long rest = mask;
      for (int q = 0; q < nk; ++q) {
        const int src = __ffsll((long long)rest) - 1;
        rest &= rest - 1;
        if (src == q) continue;
        for (int u = lane; u < U; u += 64) {
          s.hnx[(r0 + q) * U + u] = s.hnx[(r0 + src) * U + u];
          s.cnx[(r0 + q) * U + u] = s.cnx[(r0 + src) * U + u];
        }
      }
      if (lane == 0) cnt[CNT_LIVE] = nk;
    } else {
      target = ca;
    }
    beam_trie::commit_labels(tr, target, lane, committed + b, tokens + (long)b * width, ntokens + b, width, blank);
    return;
  }
  commit_stream(tr, node, live, nb, final ? 0 : -1, lane, committed + b, tokens + (long)b * width, ntokens + b, width, blank);
}

// ---- tfasr_rnnt_beam_compact: one workgroup per stream named by `mask` (a row's last token travels in s.tok, not in the trie) ----
__global__ __launch_bounds__(THREADS) void rb_compact_kernel(Ws s, const int32_t* __restrict__ mask, int32_t* __restrict__ committed,
                                                            int32_t* hstate, int H, int32_t* __restrict__ out, int W, long nmax,
                                                            unsigned hcap) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int* cnt = s.cnt + b * CNT_N;
  if (!mask[b]) {
    if (tid == 0) { out[3 * b] = 0; out[3 * b + 1] = cnt[CNT_NODES]; out[3 * b + 2] = cnt[CNT_FRAMES]; }
    return;
  }
  const long r0 = (long)b * W;
  compact_stream(trie_at(s.par, s.lab, s.dep, (long)b * nmax), s.hk + (long)b * hcap, s.hv + (long)b * hcap, hcap, cnt,
                 min(max(cnt[CNT_LIVE], 0), W), committed + b, hstate ? hstate + (long)b * horizon_stride(H) : nullptr, H, out + 3 * b, tid,
                 [&](int i) { return s.node[r0 + i]; }, [&](int i, int n) { s.node[r0 + i] = n; });
}

int rb_gemm(const float* A, const float* Bm, const float* bias, float* D, int M, int N, int Kd, hipStream_t st) {
  tfasr_gemm_args ga;
  memset(&ga, 0, sizeof(ga));
  ga.A = A; ga.B = Bm; ga.D = D; ga.bias = bias; ga.M = M; ga.N = N; ga.K = Kd; ga.lda = Kd; ga.ldb = N; ga.ldd = N;
  ga.nb1 = 1; ga.nb2 = 1; ga.alpha = 1.f; ga.beta = 0.f; ga.dtype = TFASR_F32; ga.split_k = 1;  // (split_k 1: no atomics, deterministic)
  return tfasr_gemm(&ga, st);
}

#define RB_TRY(x) do { const int st_ = (x); if (st_ != TFASR_STATUS_SUCCESS) return st_; } while (0)

int rb_begin(const RbLayout& L, const Ws& s, const int32_t* init_tok, const float* init_h, const float* init_c, const int32_t* mask, int B, int U,
             int W, int blank, bool state, hipStream_t st) {
  TFASR_KLAUNCH(rb_begin_kernel, dim3(B), dim3(THREADS), 0, st, init_tok, init_h, init_c, mask, s, W, U, blank, L.nmax, L.hcap, state);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

int rb_select(const RbLayout& L, const Ws& s, const float* logits, const int32_t* nframes, int t, int B, int T, int U, int V, int W, int blank,
              bool state, hipStream_t st) {
  const long rows = (long)B * W;
  const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
  TFASR_KLAUNCH(rb_frame_kernel, dim3(grid), dim3(256), 0, st, logits, nframes, s, B, T, V, W, L.K, blank, t);
  TFASR_CHECK_LAUNCH();
  TFASR_KLAUNCH(rb_select_kernel, dim3(B), dim3(THREADS), 0, st, logits, nframes, s, T, U, V, W, L.K, t, L.nmax, L.hcap, state);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

int rb_nbest(const RbLayout& L, const Ws& s, int B, int T, int U, int W, int P, int blank, int32_t* tokens, int32_t* tokens_len, float* score,
             int32_t* next_tok, float* next_h, float* next_c, hipStream_t st) {
  TFASR_KLAUNCH(rb_nbest_kernel, dim3(B), dim3(THREADS), 0, st, s, T, U, W, P, blank, L.nmax, tokens, tokens_len, score, next_tok, next_h,
                next_c);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

struct PredW { const float *G, *lstm_rk, *lstm_b, *ln_g, *ln_b, *wjp, *bjp; int g_packed; };

// the prediction network for every row from its gathered pre-state: hr, then the cell (hpre/cpre <- hnx/cnx, hpost, cpost, y), pred
int rb_predict(const Ws& s, const PredW& pw, int R, int U, int J, int V, float ln_eps, hipStream_t st) {
  RB_TRY(rb_gemm(s.hnx, pw.lstm_rk, nullptr, s.hr, R, 4 * U, U, st));
  TFASR_KLAUNCH(rb_cell_kernel, dim3(R), dim3(THREADS), 0, st, pw.G, pw.g_packed, pw.lstm_b, pw.ln_g, pw.ln_b, s, U, V, ln_eps);
  TFASR_CHECK_LAUNCH();
  return rb_gemm(s.y, pw.wjp, pw.bjp, s.pred, R, J, U, st);
}

// THE frame loop (the one-shot search and tfasr_rnnt_beam_advance): C frames of encj [B, C, J] from the beams the workspace holds, for
// the utterances with t < nframes[b] and fewer than Tcap frames behind them.  The prediction step comes first: it rebuilds hpre / cpre /
// hpost / cpost / y / pred from the gathered pre-states (hnx / cnx, tok), which are all of a beam's prediction state between calls.
int rb_frames(const RbLayout& L, const Ws& s, const PredW& pw, const float* vocab_w, const float* vocab_b, const float* encj,
              const int32_t* nframes, int B, int C, int Tcap, int U, int J, int V, int W, int blank, float ln_eps, hipStream_t st) {
  const int R = B * W;
  RB_TRY(rb_predict(s, pw, R, U, J, V, ln_eps, st));
  const long nz = (long)R * J;
  const int jgrid = (int)std::max<long>(1, std::min<long>((nz + 255) / 256, 4096));
  for (int t = 0; t < C; ++t) {
    TFASR_KLAUNCH(rb_join_kernel, dim3(jgrid), dim3(256), 0, st, encj, nframes, s, B, C, J, W, t);
    TFASR_CHECK_LAUNCH();
    RB_TRY(rb_gemm(s.z, vocab_w, vocab_b, s.logits, R, V, J, st));
    RB_TRY(rb_select(L, s, s.logits, nframes, t, B, Tcap, U, V, W, blank, true, st));
    if (t + 1 < C) RB_TRY(rb_predict(s, pw, R, U, J, V, ln_eps, st));
  }
  return TFASR_STATUS_SUCCESS;
}

// G = emb @ lstm_k, the input half of every token's pre-activation: `packed`'s G section (decode_pack's layout: after the recurrent,
// joint and vocabulary tiles), or computed into the workspace
int rb_weights(const Ws& s, PredW& pw, const float* emb, const float* lstm_k, const float* packed, int E, int U, int J, int V, hipStream_t st) {
  if (packed) {
    pw.G = packed + (long)(U / 4) * U * 16 + (long)((J + 15) / 16) * U * 16 + (long)((V + 15) / 16) * J * 16;
    pw.g_packed = 1;
    return TFASR_STATUS_SUCCESS;
  }
  return rb_gemm(emb, lstm_k, nullptr, s.G, V, 4 * U, E, st);
}

}  // namespace

extern "C" int tfasr_rnnt_beam_workspace_size(int B, int T, int U, int J, int V, int beam_width, size_t* bytes) {
  if (!bytes || !rb_shape_ok(B, T, U, J, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  *bytes = rb_layout(B, T, U, J, V, beam_width).total;
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_rnnt_beam_begin(const int32_t* init_tok, int B, int T, int U, int J, int V, int beam_width, int blank, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!workspace || !rb_shape_ok(B, T, U, J, V, beam_width) || blank < 0 || blank >= V) return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, T, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  return rb_begin(L, rb_carve(L, workspace, B), init_tok, nullptr, nullptr, nullptr, B, U, beam_width, blank, false, (hipStream_t)stream);
}

extern "C" int tfasr_rnnt_beam_select(const float* logits, const int32_t* nframes, int t, int B, int T, int U, int J, int V, int beam_width,
                                      int blank, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logits || !nframes || !workspace || !rb_shape_ok(B, T, U, J, V, beam_width) || blank < 0 || blank >= V || t < 0 || t >= T)
    return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, T, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  return rb_select(L, rb_carve(L, workspace, B), logits, nframes, t, B, T, U, V, beam_width, blank, false, (hipStream_t)stream);
}

extern "C" int tfasr_rnnt_beam_nbest(int B, int T, int U, int J, int V, int beam_width, int top_paths, int blank, int32_t* tokens,
                                     int32_t* tokens_len, float* score, void* workspace, size_t workspace_bytes, void* stream) {
  if (!tokens || !tokens_len || !score || !workspace || !rb_shape_ok(B, T, U, J, V, beam_width) || top_paths < 1 || top_paths > beam_width ||
      blank < 0 || blank >= V)
    return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, T, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  return rb_nbest(L, rb_carve(L, workspace, B), B, T, U, beam_width, top_paths, blank, tokens, tokens_len, score, nullptr, nullptr, nullptr,
                  (hipStream_t)stream);
}

extern "C" int tfasr_rnnt_beam_search(const float* emb, const float* lstm_k, const float* lstm_rk, const float* lstm_b, const float* ln_g,
                                      const float* ln_b, const float* joint_pred_w, const float* joint_pred_b, const float* vocab_w,
                                      const float* vocab_b, const float* packed, const float* encj, const int32_t* nframes,
                                      const int32_t* init_tok, const float* init_h, const float* init_c, int B, int T, int E, int U, int J,
                                      int V, int beam_width, int top_paths, int blank, float ln_eps, int32_t* tokens, int32_t* tokens_len,
                                      float* score, int32_t* next_tok, float* next_h, float* next_c, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!emb || !lstm_k || !lstm_rk || !lstm_b || !joint_pred_w || !joint_pred_b || !vocab_w || !vocab_b || !encj || !nframes || !tokens ||
      !tokens_len || !score || !next_tok || !next_h || !next_c || !workspace)
    return TFASR_STATUS_INVALID_VALUE;
  if (!ln_g != !ln_b || !init_h != !init_c) return TFASR_STATUS_INVALID_VALUE;
  if (!rb_shape_ok(B, T, U, J, V, beam_width) || E < 1 || top_paths < 1 || top_paths > beam_width || blank < 0 || blank >= V)
    return TFASR_STATUS_INVALID_VALUE;
  if (packed && (U % 16 || J % 16)) return TFASR_STATUS_INVALID_VALUE;  // (decode_pack makes no `packed` for other shapes)
  const RbLayout L = rb_layout(B, T, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t st = (hipStream_t)stream;
  const Ws s = rb_carve(L, workspace, B);
  const int W = beam_width;
  PredW pw{s.G, lstm_rk, lstm_b, ln_g, ln_b, joint_pred_w, joint_pred_b, 0};
  // the one-shot search = begin + one advance over all T frames + n-best
  RB_TRY(rb_weights(s, pw, emb, lstm_k, packed, E, U, J, V, st));
  RB_TRY(rb_begin(L, s, init_tok, init_h, init_c, nullptr, B, U, W, blank, true, st));
  RB_TRY(rb_frames(L, s, pw, vocab_w, vocab_b, encj, nframes, B, T, T, U, J, V, W, blank, ln_eps, st));
  return rb_nbest(L, s, B, T, U, W, top_paths, blank, tokens, tokens_len, score, next_tok, next_h, next_c, st);
}

// ---- the search in pieces (streaming sessions): the workspace, sized with T = Tcap, IS the carried beam state of B streams ----
extern "C" int tfasr_rnnt_beam_reset(const int32_t* mask, int B, int Tcap, int U, int J, int V, int beam_width, int blank, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!workspace || !rb_shape_ok(B, Tcap, U, J, V, beam_width) || blank < 0 || blank >= V) return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, Tcap, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  return rb_begin(L, rb_carve(L, workspace, B), nullptr, nullptr, nullptr, mask, B, U, beam_width, blank, true, (hipStream_t)stream);
}

extern "C" int tfasr_rnnt_beam_advance(const float* emb, const float* lstm_k, const float* lstm_rk, const float* lstm_b, const float* ln_g,
                                       const float* ln_b, const float* joint_pred_w, const float* joint_pred_b, const float* vocab_w,
                                       const float* vocab_b, const float* packed, const float* encj, const int32_t* nvalid, int B, int C,
                                       int Tcap, int E, int U, int J, int V, int beam_width, int blank, float ln_eps, int frames_max_after,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!emb || !lstm_k || !lstm_rk || !lstm_b || !joint_pred_w || !joint_pred_b || !vocab_w || !vocab_b || !encj || !nvalid || !workspace)
    return TFASR_STATUS_INVALID_VALUE;
  if (!ln_g != !ln_b) return TFASR_STATUS_INVALID_VALUE;
  if (!rb_shape_ok(B, Tcap, U, J, V, beam_width) || C < 1 || C > Tcap || E < 1 || blank < 0 || blank >= V) return TFASR_STATUS_INVALID_VALUE;
  if (frames_max_after < 0 || frames_max_after > Tcap) return TFASR_STATUS_INVALID_VALUE;  // (the trie holds 1 + W * Tcap nodes)
  if (packed && (U % 16 || J % 16)) return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, Tcap, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t st = (hipStream_t)stream;
  const Ws s = rb_carve(L, workspace, B);
  PredW pw{s.G, lstm_rk, lstm_b, ln_g, ln_b, joint_pred_w, joint_pred_b, 0};
  RB_TRY(rb_weights(s, pw, emb, lstm_k, packed, E, U, J, V, st));
  return rb_frames(L, s, pw, vocab_w, vocab_b, encj, nvalid, B, C, Tcap, U, J, V, beam_width, blank, ln_eps, st);
}

extern "C" int tfasr_rnnt_beam_commit(const int32_t* final_mask, int32_t* committed, int32_t* tokens, int32_t* ntokens, int B, int Tcap, int U,
                                      int J, int V, int beam_width, int width, int blank, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (!committed || !tokens || !ntokens || !workspace || !rb_shape_ok(B, Tcap, U, J, V, beam_width) || width < 1 || blank < 0 || blank >= V)
    return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, Tcap, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t st = (hipStream_t)stream;
  TFASR_KLAUNCH(rb_commit_kernel, dim3(B), dim3(64), 0, st, rb_carve(L, workspace, B), final_mask, committed, tokens, ntokens, beam_width, width,
                blank, L.nmax);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_rnnt_beam_nbest_states(int B, int Tcap, int U, int J, int V, int beam_width, int top_paths, int blank, int width,
                                            int32_t* tokens, int32_t* tokens_len, float* score, int32_t* next_tok, float* next_h,
                                            float* next_c, void* workspace, size_t workspace_bytes, void* stream) {
  if (!tokens || !tokens_len || !score || !next_tok || !next_h || !next_c || !workspace || !rb_shape_ok(B, Tcap, U, J, V, beam_width) ||
      top_paths < 1 || top_paths > beam_width || blank < 0 || blank >= V || width < 1 || width > Tcap)
    return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, Tcap, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  return rb_nbest(L, rb_carve(L, workspace, B), B, width, U, beam_width, top_paths, blank, tokens, tokens_len, score, next_tok, next_h, next_c,
                  (hipStream_t)stream);
}

// ---- the commit horizon and the compaction: the horizon state [B, 4 + 2 (horizon + 1)] int32 is the caller's ----
extern "C" int tfasr_rnnt_beam_commit_horizon(const int32_t* final_mask, int32_t* committed, int32_t* tokens, int32_t* ntokens,
                                              int32_t* horizon_state, int horizon, int B, int Tcap, int U, int J, int V, int beam_width,
                                              int width, int blank, void* workspace, size_t workspace_bytes, void* stream) {
  if (!committed || !tokens || !ntokens || !horizon_state || !workspace || !rb_shape_ok(B, Tcap, U, J, V, beam_width) || width < 1 ||
      blank < 0 || blank >= V || horizon < 1 || horizon > TFASR_BEAM_MAX_HORIZON)
    return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, Tcap, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t st = (hipStream_t)stream;
  TFASR_KLAUNCH(rb_commit_horizon_kernel, dim3(B), dim3(64), 0, st, rb_carve(L, workspace, B), final_mask, committed, tokens, ntokens,
                horizon_state, horizon, beam_width, U, width, blank, L.nmax);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_rnnt_beam_compact(const int32_t* mask, int32_t* committed, int32_t* horizon_state, int horizon, int32_t* out, int B,
                                       int Tcap, int U, int J, int V, int beam_width, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mask || !committed || !out || !workspace || !rb_shape_ok(B, Tcap, U, J, V, beam_width)) return TFASR_STATUS_INVALID_VALUE;
  if (horizon_state ? (horizon < 1 || horizon > TFASR_BEAM_MAX_HORIZON) : horizon != 0) return TFASR_STATUS_INVALID_VALUE;
  const RbLayout L = rb_layout(B, Tcap, U, J, V, beam_width);
  if (workspace_bytes < L.total) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t st = (hipStream_t)stream;
  TFASR_KLAUNCH(rb_compact_kernel, dim3(B), dim3(THREADS), 0, st, rb_carve(L, workspace, B), mask, committed, horizon_state, horizon, out,
                beam_width, L.nmax, L.hcap);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
