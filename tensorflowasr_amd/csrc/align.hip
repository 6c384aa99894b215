// Forced alignment (Viterbi) for gfx950: the best single path through the lattices the losses sum over, with its times.
//
// Transducer (lattice log-probabilities blank[t,u] / truth[t,u] as csrc/rnnt_loss.hip defines them):
//   v[0,0] = 0;  v[t,u] = max(v[t-1,u] + blank[t-1,u], v[t,u-1] + truth[t,u-1]);  score = v[Tl-1,Ul] + blank[Tl-1,Ul]
//   an exact tie emits the label as LATE as possible: the walk keeps taking blank moves while a best path continues that way, which in
//   the back-trace from (Tl-1, Ul) is the LABEL move into (t,u) on a tie (the label at this frame rather than an earlier one).  Best
//   paths that cross share a node, so "every label at its latest frame over all best paths" is itself a best path: that one.
//   Row 0 can only be reached by label moves.
// CTC (states s = 0..2Ul of the extended label sequence as csrc/ctc.hip, lp[t,s] = logit[t,lab_s] - lse[t], or the logit itself
// when the caller says the input is already normalised):
//   v[0,s] = lp[0,s] for s <= 1;  v[t,s] = max(v[t-1,s], v[t-1,s-1], v[t-1,s-2] if s odd and lab_s != lab_{s-2}) + lp[t,s]
//   score = max(v[Tl-1,2Ul], v[Tl-1,2Ul-1]);  an exact tie takes the SMALLEST move (stay, s-1, s-2), the final blank at the end.
// Every value is one f32 addition of two stored numbers: there is nothing for contraction to fuse.
//
// Kernels:
//   1. rnnt_viterbi_wave : one wave per utterance, the walk of rnnt_lattice_wave_kernel (a lane owns E adjacent columns, the left
//                          neighbour arrives by one DPP wave shift per anti-diagonal, operands from a register ring of prefetched
//                          diagonals) with max for log-add-exp; the decision bit of a diagonal's nodes is collected with a ballot
//                          and lane 0 stores the 64-bit word (one bit per node, nothing else is written per node).  U1 <= 256.
//   2. rnnt_viterbi_wg   : one workgroup per utterance, one thread per column, neighbours through a double-buffered LDS row
//                          (256 < U1 <= 1024).
//   3. rnnt_backtrace    : one wave per utterance; lane 0 follows the bits from (Tl-1, Ul), at most Tl+Ul dependent steps.
//   4. ctc_viterbi       : one workgroup per utterance, one thread per state, Tl sequential steps (the shape of ctc_scan_kernel);
//                          two ballots per step record the move (0, 1, 2) of every state.
//   5. ctc_backtrace     : lane 0 follows the moves and writes [start, end) of every label; then one lane per label adds its
//                          log-probabilities in frame order.
// N-best lists (tfasr_ctc_nbest_align): kernels 4 and 5 over B * P label rows, row b * P + p against the logits of utterance b - the same
// code as the one-row-per-utterance call, so the same bits - after ONE pass for the lse and the entropy of every frame (csrc/ctc.hip,
// ctc_frame_detail); kernel 5 then also averages the frame entropy over each label's span.
#include "common.h"
#include "lattice_lp.h"
#include <algorithm>

namespace {

typedef unsigned long long u64;

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

constexpr int kRnntMaxU1 = TFASR_ALIGN_MAX_U1;    // one workgroup of 1024 threads, one per lattice column
constexpr int kCtcMaxU = TFASR_ALIGN_CTC_MAX_U;  // 2U+1 states, one thread each

// Decision words of the transducer walk: the node (t,u) sits in word (t+u) * NW + widx(u), bit bit(u), of its utterance's block of
// (T + U1) * NW words.  Wave kernel (E columns per lane): widx = u % E, bit = u / E; workgroup kernel (E = 0): widx = u / 64, bit = u % 64.
inline int rnnt_wave_e(int U1) { return U1 <= 64 ? 1 : (U1 <= 128 ? 2 : (U1 <= 256 ? 4 : 0)); }
inline int rnnt_dec_nw(int U1) { const int e = rnnt_wave_e(U1); return e ? e : (U1 + 63) / 64; }
inline size_t rnnt_dec_bytes(int B, int T, int U1) { return align256((size_t)B * ((size_t)T + U1) * rnnt_dec_nw(U1) * sizeof(u64)); }
inline int ctc_dec_nw(int U) { return (2 * U + 1 + 63) / 64; }

// ---------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(64) void rnnt_viterbi_wave_kernel(const float* __restrict__ blank_lp, const float* __restrict__ truth_lp,
                                                               const int32_t* __restrict__ label_len, const int32_t* __restrict__ logit_len,
                                                               const long* __restrict__ cell_off, int Tm, int U1m, u64* __restrict__ dec,
                                                               long dec_stride, float* __restrict__ score) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tl = min(logit_len[b], Tm), Ul = max(min(label_len[b], U1m - 1), 0);
  const int U1 = cell_off ? Ul + 1 : U1m;
  const long base = cell_off ? cell_off[b] : (long)b * Tm * U1m;
  const float* bl = blank_lp + base;
  const float* tr = truth_lp + base;
  if (Tl <= 0) { if (lane == 0) score[b] = -INFINITY; return; }
  u64* d = dec + (long)b * dec_stride;
  const int ndiag = Tl + Ul;
  constexpr int PF = E == 1 ? 32 : (E == 2 ? 16 : 8);
  float rb[PF][E], rt[PF][E];
  int ue[E], uc[E];
  bool ucol[E];
#pragma unroll
  for (int e = 0; e < E; ++e) { ue[e] = lane * E + e; uc[e] = min(ue[e], Ul); ucol[e] = ue[e] <= Ul; }
  float self[E];
#pragma unroll
  for (int e = 0; e < E; ++e) self[e] = -INFINITY;
  // node (t,u) on diagonal n = t+u needs blank[t-1,u] and truth[t,u-1]; loads are unconditional from clamped (always valid) cells
  auto fetch = [&](int n, int e, float& fb, float& ft) {
    const int tc = min(max(n - ue[e], 0), Tl - 1);
    fb = bl[max(tc - 1, 0) * U1 + uc[e]];
    ft = tr[tc * U1 + max(uc[e] - 1, 0)];
  };
#pragma unroll
  for (int j = 0; j < PF; ++j)
#pragma unroll
    for (int e = 0; e < E; ++e) fetch(j, e, rb[j][e], rt[j][e]);
  for (int n0 = 0; n0 < ndiag; n0 += PF) {
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      const int n = n0 + j;  // diagonals past the lattice (padding up to a multiple of PF) have no active node and store nothing
      float left[E];
      left[0] = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(self[E - 1]), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
#pragma unroll
      for (int e = 1; e < E; ++e) left[e] = self[e - 1];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int t = n - ue[e];
        const bool act = ucol[e] && t >= 0 && t < Tl;
        const float pb = rb[j][e], pt = rt[j][e];
        fetch(n + PF, e, rb[j][e], rt[j][e]);
        bool label_move = false;
        if (act) {
          float a = 0.f;
          if (t > 0 || ue[e] > 0) {
            const float xb = (t > 0) ? self[e] + pb : -INFINITY;
            const float xt = (ue[e] > 0) ? left[e] + pt : -INFINITY;
            label_move = ue[e] > 0 && (t == 0 || xt >= xb);
            a = label_move ? xt : xb;
          }
          self[e] = a;
        }
        const u64 word = __ballot(label_move);
        if (lane == 0 && n < ndiag) d[(long)n * E + e] = word;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (ue[e] == Ul) score[b] = self[e] + bl[(Tl - 1) * U1 + Ul];
}

// grid B, blockDim = NW * 64 >= U1
__global__ void rnnt_viterbi_wg_kernel(const float* __restrict__ blank_lp, const float* __restrict__ truth_lp,
                                       const int32_t* __restrict__ label_len, const int32_t* __restrict__ logit_len,
                                       const long* __restrict__ cell_off, int Tm, int U1m, int NW, u64* __restrict__ dec, long dec_stride,
                                       float* __restrict__ score) {
  extern __shared__ float sh[];  // 2 * blockDim.x floats
  const int b = blockIdx.x, u = threadIdx.x, nthr = blockDim.x;
  const int Tl = min(logit_len[b], Tm), Ul = max(min(label_len[b], U1m - 1), 0);
  const int U1 = cell_off ? Ul + 1 : U1m;
  const long base = cell_off ? cell_off[b] : (long)b * Tm * U1m;
  const float* bl = blank_lp + base;
  const float* tr = truth_lp + base;
  float* buf0 = sh;
  float* buf1 = sh + nthr;
  buf0[u] = -INFINITY;
  buf1[u] = -INFINITY;
  __syncthreads();
  if (Tl <= 0) { if (u == 0) score[b] = -INFINITY; return; }
  u64* d = dec + (long)b * dec_stride;
  const int ndiag = Tl + Ul;
  float self = -INFINITY;
  for (int n = 0; n < ndiag; ++n) {
    float* cur = (n & 1) ? buf1 : buf0;
    const float* prev = (n & 1) ? buf0 : buf1;
    const int t = n - u;
    const bool act = u <= Ul && t >= 0 && t < Tl;
    bool label_move = false;
    if (act) {
      float a = 0.f;
      if (t > 0 || u > 0) {
        const float xb = (t > 0) ? self + bl[(long)(t - 1) * U1 + u] : -INFINITY;
        const float xt = (u > 0) ? prev[u - 1] + tr[(long)t * U1 + u - 1] : -INFINITY;
        label_move = u > 0 && (t == 0 || xt >= xb);
        a = label_move ? xt : xb;
      }
      self = a;
      cur[u] = a;
    }
    const u64 word = __ballot(label_move);
    if ((u & 63) == 0) d[(long)n * NW + (u >> 6)] = word;
    __syncthreads();
  }
  if (u == Ul) score[b] = self + bl[(long)(Tl - 1) * U1 + Ul];
}

// grid B, 64 threads.  E: columns per lane of the wave kernel that wrote the words, 0 for the workgroup kernel.
__global__ __launch_bounds__(64) void rnnt_backtrace_kernel(const float* __restrict__ truth_lp, const int32_t* __restrict__ label_len,
                                                            const int32_t* __restrict__ logit_len, const long* __restrict__ cell_off, int Tm,
                                                            int U1m, int E, int NW, const u64* __restrict__ dec, long dec_stride,
                                                            int32_t* __restrict__ frames, float* __restrict__ label_lp) {
  const int b = blockIdx.x, lane = threadIdx.x, U = U1m - 1;
  const int Tl = min(logit_len[b], Tm), Ul = max(min(label_len[b], U), 0);
  const int U1 = cell_off ? Ul + 1 : U1m;
  const long base = cell_off ? cell_off[b] : (long)b * Tm * U1m;
  const float* tr = truth_lp + base;
  for (int u = lane; u < U; u += 64)
    if (u >= Ul || Tl <= 0) { frames[(long)b * U + u] = -1; label_lp[(long)b * U + u] = 0.f; }
  if (lane != 0 || Tl <= 0) return;
  const u64* d = dec + (long)b * dec_stride;
  int t = Tl - 1, u = Ul;
  while (u > 0) {  // t never passes 0: row 0 is left by label moves only
    const int widx = E ? u % E : u >> 6, bit = E ? u / E : u & 63;
    const bool label_move = t == 0 || ((d[(long)(t + u) * NW + widx] >> bit) & 1);
    if (label_move) {
      frames[(long)b * U + u - 1] = t;
      label_lp[(long)b * U + u - 1] = tr[(long)t * U1 + u - 1];
      --u;
    } else {
      --t;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// grid B * P, blockDim = NW * 64 >= 2U+1: row r = b * P + p walks labels[r * ldl ..) over the logits of utterance b (P = 1, ldl = U: one
// label row per utterance, tfasr_ctc_align).  lse == nullptr: the logits are log-probabilities already.  nbest: a row with
// label_len < 0 or > U is dead (no walk, score -inf) instead of clamped.  The P workgroups of an utterance gather from the same logit
// rows, which they share through L2; a state's gather logit[t+1, lab_s] does not depend on the step before it and is issued ahead of
// the step's barrier.
template <typename T>
__global__ void ctc_viterbi_kernel(const T* __restrict__ logits, const float* __restrict__ lse, const int32_t* __restrict__ labels, long ldl,
                                   const int32_t* __restrict__ label_len, const int32_t* __restrict__ logit_len, int P, int Tm, int U, int V,
                                   int blank, int nbest, int NW, u64* __restrict__ dec, float* __restrict__ score,
                                   int32_t* __restrict__ final_state) {
  extern __shared__ float sh[];
  const int r = blockIdx.x, b = r / P, s = threadIdx.x, nthr = blockDim.x;
  const int ll = label_len[r];
  const int Tl = min(logit_len[b], Tm), Ul = max(min(ll, U), 0);
  const bool dead = nbest && (ll < 0 || ll > U);
  const int S = 2 * Ul + 1;
  float* buf0 = sh;
  float* buf1 = sh + nthr;
  buf0[s] = -INFINITY;
  buf1[s] = -INFINITY;
  __syncthreads();
  if (Tl <= 0 || dead) { if (s == 0) { score[r] = -INFINITY; final_state[r] = -1; } return; }
  const bool act = s < S;
  const int32_t* lb = labels + (long)r * ldl;
  int lab = blank;
  bool skip = false;  // transition s-2 -> s allowed
  if (act && (s & 1)) {  // labels and neighbours clamped as ctc_scan_kernel clamps them
    lab = min(max(lb[s >> 1], 0), V - 1);
    if (s >= 2) skip = lab != min(max(lb[(s >> 1) - 1], 0), V - 1);
  }
  const T* lg = logits + (long)b * Tm * V + lab;
  const float* ls = lse ? lse + (long)b * Tm : nullptr;
  u64* d = dec + (long)r * Tm * NW * 2;
  // the next frame's logit and lse wait in registers across the barrier; the subtraction (the only use) comes a step later
  float nx = act ? Num<T>::ld(lg) : 0.f, nl = ls ? ls[0] : 0.f;
  for (int t = 0; t < Tl; ++t) {
    float* cur = (t & 1) ? buf1 : buf0;
    const float* prev = (t & 1) ? buf0 : buf1;
    int mv = 0;
    const float lp = ls ? nx - nl : nx;
    if (t + 1 < Tl) {
      if (act) nx = Num<T>::ld(lg + (long)(t + 1) * V);
      if (ls) nl = ls[t + 1];
    }
    if (act) {
      float a;
      if (t == 0) a = (s <= 1) ? lp : -INFINITY;
      else {
        float best = prev[s];
        if (s >= 1) { const float v1 = prev[s - 1]; if (v1 > best) { best = v1; mv = 1; } }
        if (skip) { const float v2 = prev[s - 2]; if (v2 > best) { best = v2; mv = 2; } }
        a = best + lp;
      }
      cur[s] = a;
    }
    const u64 w0 = __ballot(mv & 1), w1 = __ballot(mv >> 1);
    if ((s & 63) == 0) {
      d[((long)t * NW + (s >> 6)) * 2] = w0;
      d[((long)t * NW + (s >> 6)) * 2 + 1] = w1;
    }
    __syncthreads();
  }
  if (s == 0) {
    const float* last = ((Tl - 1) & 1) ? buf1 : buf0;
    const float a1 = last[S - 1], a2 = (S >= 2) ? last[S - 2] : -INFINITY;
    const float sc = fmaxf(a1, a2);
    score[r] = sc;
    final_state[r] = (sc == -INFINITY) ? -1 : ((a2 > a1) ? S - 2 : S - 1);
  }
}

// grid B * P, 64 threads.  frame_ent / label_entropy (both or neither): the mean over [start, end) of the frame entropies, summed in frame
// order and then divided, as ctc_collapse_detail_kernel (csrc/ctc.hip) forms tok_entropy.
template <typename T>
__global__ __launch_bounds__(64) void ctc_backtrace_kernel(const T* __restrict__ logits, const float* __restrict__ lse,
                                                           const float* __restrict__ frame_ent, const int32_t* __restrict__ labels, long ldl,
                                                           const int32_t* __restrict__ label_len, const int32_t* __restrict__ logit_len, int P,
                                                           int Tm, int U, int V, int NW, const u64* __restrict__ dec,
                                                           const int32_t* __restrict__ final_state, int32_t* start, int32_t* end,
                                                           float* __restrict__ label_lp, float* __restrict__ label_entropy) {
  const int r = blockIdx.x, b = r / P, lane = threadIdx.x;
  const int Tl = min(logit_len[b], Tm), Ul = max(min(label_len[r], U), 0);
  const int fs = final_state[r];
  const long o = (long)r * U;
  for (int u = lane; u < U; u += 64)
    if (u >= Ul || fs < 0) {
      start[o + u] = -1;
      end[o + u] = -1;
      label_lp[o + u] = 0.f;
      if (label_entropy) label_entropy[o + u] = 0.f;
    }
  if (fs < 0) return;  // no frames, the labels do not fit them, or a dead row
  if (lane == 0) {
    const u64* d = dec + (long)r * Tm * NW * 2;
    int s = fs, open = -1;
    for (int t = Tl - 1; t >= 0; --t) {
      if (s & 1) {
        const int u = s >> 1;
        if (u != open) { end[o + u] = t + 1; open = u; }
        start[o + u] = t;  // the last write is the earliest frame
      }
      if (t > 0) {
        const long w = ((long)t * NW + (s >> 6)) * 2;
        const int mv = (int)((d[w] >> (s & 63)) & 1) | ((int)((d[w + 1] >> (s & 63)) & 1) << 1);
        s = max(s - mv, 0);
      }
    }
  }
  __threadfence_block();
  __syncthreads();
  const T* lg = logits + (long)b * Tm * V;
  const float* ls = lse ? lse + (long)b * Tm : nullptr;
  const float* fe = frame_ent ? frame_ent + (long)b * Tm : nullptr;
  for (int u = lane; u < Ul; u += 64) {
    const int t0 = max(start[o + u], 0), t1 = min(end[o + u], Tl);
    const int lab = min(max(labels[(long)r * ldl + u], 0), V - 1);
    float acc = 0.f, ent_run = 0.f;
    for (int t = t0; t < t1; ++t) {
      float lp = Num<T>::ld(lg + (long)t * V + lab);
      if (ls) lp = lp - ls[t];
      acc = (t == t0) ? lp : acc + lp;
      if (fe) ent_run += fe[t];
    }
    label_lp[o + u] = acc;
    if (label_entropy) label_entropy[o + u] = t1 > t0 ? ent_run / (float)(t1 - t0) : 0.f;
  }
}

// the two launches of a CTC alignment: B * P label rows over B utterances
template <typename T>
void ctc_walk(const T* logits, const float* lse, const float* frame_ent, const int32_t* labels, long ldl, const int32_t* label_len,
              const int32_t* logit_len, int B, int P, int Tm, int U, int V, int blank, int nbest, u64* dec, int32_t* fin, int32_t* start, int32_t* end,
              float* label_lp, float* label_entropy, float* score, hipStream_t s) {
  const int NW = ctc_dec_nw(U), nthr = NW * 64;
  TFASR_KLAUNCH(ctc_viterbi_kernel<T>, dim3(B * P), dim3(nthr), 2 * nthr * sizeof(float), s, logits, lse, labels, ldl, label_len, logit_len, P, Tm, U, V,
                blank, nbest, NW, dec, score, fin);
  if (U > 0)
    TFASR_KLAUNCH(ctc_backtrace_kernel<T>, dim3(B * P), dim3(64), 0, s, logits, lse, frame_ent, labels, ldl, label_len, logit_len, P, Tm, U, V, NW, dec,
                  fin, start, end, label_lp, label_entropy);
}

// ---------------------------------------------------------------------------------------------
int rnnt_shape_status(int B, int T, int U1) {
  if (B <= 0 || T <= 0 || U1 <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (U1 > kRnntMaxU1) return TFASR_STATUS_UNSUPPORTED;
  return TFASR_STATUS_SUCCESS;
}

int rnnt_walk(const float* blank_lp, const float* truth_lp, const int32_t* label_len, const int32_t* logit_len, const long* cell_off, int B,
              int T, int U1, int32_t* frames, float* label_lp, float* score, u64* dec, hipStream_t stream) {
  const int E = rnnt_wave_e(U1), NW = rnnt_dec_nw(U1);
  const long stride = ((long)T + U1) * NW;
#define TFASR_VW(E_) TFASR_KLAUNCH((rnnt_viterbi_wave_kernel<E_>), dim3(B), dim3(64), 0, stream, blank_lp, truth_lp, label_len, logit_len, cell_off, T, U1, dec, stride, score)
  if (E == 1) TFASR_VW(1);
  else if (E == 2) TFASR_VW(2);
  else if (E == 4) TFASR_VW(4);
  else
    TFASR_KLAUNCH(rnnt_viterbi_wg_kernel, dim3(B), dim3(NW * 64), 2 * NW * 64 * sizeof(float), stream, blank_lp, truth_lp, label_len, logit_len,
                  cell_off, T, U1, NW, dec, stride, score);
#undef TFASR_VW
  TFASR_CHECK_LAUNCH();
  if (U1 > 1) {
    TFASR_KLAUNCH(rnnt_backtrace_kernel, dim3(B), dim3(64), 0, stream, truth_lp, label_len, logit_len, cell_off, T, U1, E, NW, dec, stride, frames,
                  label_lp);
    TFASR_CHECK_LAUNCH();
  }
  return TFASR_STATUS_SUCCESS;
}

// the log-probability pass (from logits or from the GEMM's statistics), then the walk
int rnnt_align_impl(const void* logits, const float* lse_part, int lse_parts, const float* pick, const int32_t* labels, const int32_t* label_len,
                    const int32_t* logit_len, const long* cell_off, long total_cells, int B, int T, int U1, int V, int blank, int dtype,
                    int32_t* frames, float* label_lp, float* score, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!labels || !label_len || !logit_len || !score || !workspace || (U1 > 1 && (!frames || !label_lp))) return TFASR_STATUS_INVALID_VALUE;
  if (V <= 1 || blank < 0 || blank >= V) return TFASR_STATUS_INVALID_VALUE;
  const int st = rnnt_shape_status(B, T, U1);
  if (st != TFASR_STATUS_SUCCESS) return st;
  if (blank != 0) return TFASR_STATUS_UNSUPPORTED;  // the lattice log-probabilities take the blank from column 0, as the loss
  const long nrows = cell_off ? total_cells : (long)B * T * U1;
  if (nrows <= 0 || nrows > (long)B * T * U1) return TFASR_STATUS_INVALID_VALUE;
  const size_t seg = align256((size_t)nrows * sizeof(float));
  if (workspace_bytes < 3 * seg + rnnt_dec_bytes(B, T, U1)) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  float* lse = (float*)ws;
  float* bl = (float*)(ws + seg);
  float* tr = (float*)(ws + 2 * seg);
  const int lp = tfasr_detail::rnnt_lattice_logprobs(logits, labels, label_len, logit_len, cell_off, nrows, B, T, U1, V, dtype, lse_part, lse_parts,
                                                     pick, lse, bl, tr, stream);
  if (lp != TFASR_STATUS_SUCCESS) return lp;
  return rnnt_walk(bl, tr, label_len, logit_len, cell_off, B, T, U1, frames, label_lp, score, (u64*)(ws + 3 * seg), stream);
}

}  // namespace

extern "C" int tfasr_rnnt_align_workspace_size(int B, int T, int U1, int V, size_t* bytes) {
  if (!bytes || V <= 0) return TFASR_STATUS_INVALID_VALUE;
  const int st = rnnt_shape_status(B, T, U1);
  if (st != TFASR_STATUS_SUCCESS) return st;
  *bytes = 3 * align256((size_t)B * T * U1 * sizeof(float)) + rnnt_dec_bytes(B, T, U1);  // lse, blank, truth + one decision bit per node
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_rnnt_align_lattice(const float* blank_lp, const float* truth_lp, const int32_t* label_len, const int32_t* logit_len,
                                        const long* cell_off, long total_cells, int B, int T, int U1, int32_t* frames, float* label_lp,
                                        float* score, void* workspace, size_t workspace_bytes, void* stream) {
  if (!blank_lp || !truth_lp || !label_len || !logit_len || !score || !workspace || (U1 > 1 && (!frames || !label_lp))) return TFASR_STATUS_INVALID_VALUE;
  const int st = rnnt_shape_status(B, T, U1);
  if (st != TFASR_STATUS_SUCCESS) return st;
  if (cell_off && (total_cells <= 0 || total_cells > (long)B * T * U1)) return TFASR_STATUS_INVALID_VALUE;
  if (workspace_bytes < rnnt_dec_bytes(B, T, U1)) return TFASR_STATUS_INVALID_VALUE;
  return rnnt_walk(blank_lp, truth_lp, label_len, logit_len, cell_off, B, T, U1, frames, label_lp, score, (u64*)workspace, (hipStream_t)stream);
}

extern "C" int tfasr_rnnt_align(const void* logits, const int32_t* labels, const int32_t* label_len, const int32_t* logit_len, const long* cell_off,
                                long total_cells, int B, int T, int U1, int V, int blank, int dtype, int32_t* frames, float* label_lp, float* score,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!logits || (dtype != TFASR_F32 && dtype != TFASR_BF16)) return TFASR_STATUS_INVALID_VALUE;
  return rnnt_align_impl(logits, nullptr, 0, nullptr, labels, label_len, logit_len, cell_off, total_cells, B, T, U1, V, blank, dtype, frames, label_lp,
                         score, workspace, workspace_bytes, stream);
}

extern "C" int tfasr_rnnt_align_stats(const float* lse_part, int lse_parts, const float* pick, const int32_t* labels, const int32_t* label_len,
                                      const int32_t* logit_len, const long* cell_off, long total_cells, int B, int T, int U1, int V, int blank,
                                      int32_t* frames, float* label_lp, float* score, void* workspace, size_t workspace_bytes, void* stream) {
  if (!lse_part || !pick || lse_parts <= 0) return TFASR_STATUS_INVALID_VALUE;
  return rnnt_align_impl(nullptr, lse_part, lse_parts, pick, labels, label_len, logit_len, cell_off, total_cells, B, T, U1, V, blank, TFASR_F32, frames,
                         label_lp, score, workspace, workspace_bytes, stream);
}

extern "C" int tfasr_ctc_align_workspace_size(int B, int T, int U, int V, size_t* bytes) {
  if (!bytes || B <= 0 || T <= 0 || U < 0 || V <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (U > kCtcMaxU) return TFASR_STATUS_UNSUPPORTED;
  // lse per frame, final state per utterance, two decision bits per (frame, state)
  *bytes = align256((size_t)B * T * sizeof(float)) + align256((size_t)B * sizeof(int32_t)) + align256((size_t)B * T * ctc_dec_nw(U) * 2 * sizeof(u64));
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_align(const void* logits, const int32_t* labels, const int32_t* label_len, const int32_t* logit_len, int B, int T, int U, int V,
                               int blank, int dtype, int normalized, int32_t* start, int32_t* end, float* label_lp, float* score, void* workspace,
                               size_t workspace_bytes, void* stream_) {
  if (!logits || !label_len || !logit_len || !score || !workspace || (U > 0 && (!labels || !start || !end || !label_lp))) return TFASR_STATUS_INVALID_VALUE;
  if (B <= 0 || T <= 0 || U < 0 || V <= 1 || blank < 0 || blank >= V || (dtype != TFASR_F32 && dtype != TFASR_BF16)) return TFASR_STATUS_INVALID_VALUE;
  size_t need = 0;
  const int st = tfasr_ctc_align_workspace_size(B, T, U, V, &need);
  if (st != TFASR_STATUS_SUCCESS) return st;
  if (workspace_bytes < need) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  float* lse = (float*)ws;
  int32_t* fin = (int32_t*)(ws + align256((size_t)B * T * sizeof(float)));
  u64* dec = (u64*)(ws + align256((size_t)B * T * sizeof(float)) + align256((size_t)B * sizeof(int32_t)));
  if (!normalized) {
    const int lst = tfasr_detail::ctc_row_lse(logits, lse, (long)B * T, V, dtype, s);
    if (lst != TFASR_STATUS_SUCCESS) return lst;
  } else {
    lse = nullptr;
  }
  if (dtype == TFASR_F32)
    ctc_walk((const float*)logits, lse, nullptr, labels, U, label_len, logit_len, B, 1, T, U, V, blank, 0, dec, fin, start, end, label_lp, nullptr, score, s);
  else
    ctc_walk((const bf16_t*)logits, lse, nullptr, labels, U, label_len, logit_len, B, 1, T, U, V, blank, 0, dec, fin, start, end, label_lp, nullptr, score, s);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_row_lse_entropy(const void* x, long rows, int V, int dtype, float* lse, float* entropy, void* stream) {
  if (!x || !lse || rows <= 0 || V <= 0 || (dtype != TFASR_F32 && dtype != TFASR_BF16)) return TFASR_STATUS_INVALID_VALUE;
  return tfasr_detail::ctc_row_lse_entropy(x, lse, entropy, rows, V, dtype, (hipStream_t)stream);
}

extern "C" int tfasr_ctc_nbest_align_workspace_size(int B, int P, int T, int U, int V, size_t* bytes) {
  if (!bytes || B <= 0 || P <= 0 || T <= 0 || U < 0 || V <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (U > kCtcMaxU) return TFASR_STATUS_UNSUPPORTED;
  // lse and entropy per frame of an utterance, final state per label row, two decision bits per (label row, frame, state)
  *bytes = 2 * align256((size_t)B * T * sizeof(float)) + align256((size_t)B * P * sizeof(int32_t)) +
           align256((size_t)B * P * T * ctc_dec_nw(U) * 2 * sizeof(u64));
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_nbest_align(const void* logits, const int32_t* logit_len, const int32_t* labels, long ldl, const int32_t* label_len, int B,
                                     int P, int T, int U, int V, int blank, int dtype, int32_t* start, int32_t* end, float* label_lp,
                                     float* label_entropy, float* score, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!logits || !logit_len || !label_len || !score || !workspace || (U > 0 && (!labels || !start || !end || !label_lp || !label_entropy)))
    return TFASR_STATUS_INVALID_VALUE;
  if (B <= 0 || P <= 0 || T <= 0 || U < 0 || ldl < U || V <= 1 || blank < 0 || blank >= V || (dtype != TFASR_F32 && dtype != TFASR_BF16))
    return TFASR_STATUS_INVALID_VALUE;
  size_t need = 0;
  const int st = tfasr_ctc_nbest_align_workspace_size(B, P, T, U, V, &need);
  if (st != TFASR_STATUS_SUCCESS) return st;
  if (workspace_bytes < need) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  const size_t seg = align256((size_t)B * T * sizeof(float));
  float* lse = (float*)ws;
  float* ent = (float*)(ws + seg);
  int32_t* fin = (int32_t*)(ws + 2 * seg);
  u64* dec = (u64*)(ws + 2 * seg + align256((size_t)B * P * sizeof(int32_t)));
  const int lst = tfasr_detail::ctc_row_lse_entropy(logits, lse, ent, (long)B * T, V, dtype, s);  // once per utterance, not per path
  if (lst != TFASR_STATUS_SUCCESS) return lst;
  if (dtype == TFASR_F32)
    ctc_walk((const float*)logits, lse, ent, labels, ldl, label_len, logit_len, B, P, T, U, V, blank, 1, dec, fin, start, end, label_lp, label_entropy,
             score, s);
  else
    ctc_walk((const bf16_t*)logits, lse, ent, labels, ldl, label_len, logit_len, B, P, T, U, V, blank, 1, dec, fin, start, end, label_lp,
             label_entropy, score, s);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
