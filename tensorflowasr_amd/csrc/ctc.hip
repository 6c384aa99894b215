// CTC loss + gradient and CTC greedy decoding for gfx950.
//
// Reference: CtcLoss.call -> tf.nn.ctc_loss(labels dense [B,U], logits [B,T,V], label_length, logit_length,
// logits_time_major=False, blank_index=0) (losses/ctc_loss.py:47-66) and CtcModel.recognize ->
// tf.nn.ctc_greedy_decoder(merge_repeated=True, blank_index) (models/ctc/base_ctc.py:102-124).
// Standard CTC (Graves 2006) over the extended label sequence l' = (b, l1, b, l2, ..., b), S = 2U+1 states:
//   alpha_t(s) = lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if l'_s != b and l'_s != l'_{s-2}]) + lp_t(l'_s)
//   loss = -lse(alpha_{T-1}(S-1), alpha_{T-1}(S-2));  dL/dlogit_t(v) = softmax_t(v) - sum_{s: l'_s = v} exp(alpha_t(s)+beta_t(s)-lp_t(v)-logP)
// Kernels: per-frame log-sum-exp (one wave per frame, HBM-bound single pass over V), the state scan (one workgroup per
// (utterance, {alpha|beta}), one thread per state, T sequential steps through a double-buffered LDS row), the gradient
// (one workgroup per frame; per-label occupancies combined with LDS atomics, then one pass over V).
#include "common.h"
#include "lattice_lp.h"
#include <algorithm>

namespace {

template <typename T>
__global__ __launch_bounds__(256) void ctc_lse_kernel(const T* __restrict__ logits, float* __restrict__ lse,
                                                      int32_t* __restrict__ amax, long rows, int V) {
  const int lane = threadIdx.x & 63;
  const long w0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (long)gridDim.x * (blockDim.x >> 6);
  for (long r = w0; r < rows; r += nw) {
    const T* row = logits + r * V;
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) { const float x = Num<T>::ld(row + v); if (x > m) { m = x; mi = v; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(Num<T>::ld(row + v) - m);
    s = wave_sum(s);
    if (lane == 0) { if (lse) lse[r] = m + logf(s); if (amax) amax[r] = mi; }
  }
}

__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// grid (B, 2); blockDim >= S = 2*U+1
template <typename T>
__global__ void ctc_scan_kernel(const T* __restrict__ logits, const float* __restrict__ lse, const int32_t* __restrict__ labels,
                                const int32_t* __restrict__ label_len, const int32_t* __restrict__ logit_len, int Tm, int U,
                                int V, int blank, float* __restrict__ alpha, float* __restrict__ beta, float* __restrict__ costs) {
  extern __shared__ float sh[];
  const int b = blockIdx.x, s = threadIdx.x, nthr = blockDim.x;
  const int Tl = min(logit_len[b], Tm), Ul = max(min(label_len[b], U), 0);  // a negative length is an empty one, as in csrc/align.hip
  const int S = 2 * Ul + 1, Smax = 2 * U + 1;
  float* buf0 = sh;
  float* buf1 = sh + nthr;
  buf0[s] = -INFINITY;
  buf1[s] = -INFINITY;
  __syncthreads();
  if (Tl <= 0) { if (s == 0 && blockIdx.y == 0) costs[b] = (Ul == 0) ? 0.f : INFINITY; return; }
  const bool act = s < S;
  int lab = blank;
  bool skip = false;  // transition s-2 -> s (alpha) allowed
  bool skipb = false; // transition s -> s+2 (beta) allowed
  if (act && (s & 1)) {
    lab = min(max(labels[(long)b * U + (s >> 1)], 0), V - 1);
    // neighbours clamped like `lab` itself (an out-of-range label is folded into [0, V-1] everywhere, not only at its own state)
    if (s >= 2) skip = lab != min(max(labels[(long)b * U + (s >> 1) - 1], 0), V - 1);
    if (s + 2 < S) skipb = lab != min(max(labels[(long)b * U + (s >> 1) + 1], 0), V - 1);
  }
  const T* lg = logits + (long)b * Tm * V;
  const float* ls = lse + (long)b * Tm;
  const long abase = (long)b * Tm * Smax;
  if (blockIdx.y == 0) {
    for (int t = 0; t < Tl; ++t) {
      float* cur = (t & 1) ? buf1 : buf0;
      const float* prev = (t & 1) ? buf0 : buf1;
      if (act) {
        const float lp = Num<T>::ld(lg + (long)t * V + lab) - ls[t];
        float a;
        if (t == 0) a = (s <= 1) ? lp : -INFINITY;
        else a = lse3(prev[s], s >= 1 ? prev[s - 1] : -INFINITY, skip ? prev[s - 2] : -INFINITY) + lp;
        alpha[abase + (long)t * Smax + s] = a;
        cur[s] = a;
      }
      __syncthreads();
    }
    if (s == 0) {
      const float* last = ((Tl - 1) & 1) ? buf1 : buf0;
      const float a1 = last[S - 1], a2 = (S >= 2) ? last[S - 2] : -INFINITY;
      costs[b] = -lse3(a1, a2, -INFINITY);
    }
  } else {
    int it = 0;
    for (int t = Tl - 1; t >= 0; --t, ++it) {
      float* cur = (it & 1) ? buf1 : buf0;
      const float* prev = (it & 1) ? buf0 : buf1;
      if (act) {
        const float lp = Num<T>::ld(lg + (long)t * V + lab) - ls[t];
        float v;
        if (t == Tl - 1) v = (s >= S - 2) ? lp : -INFINITY;
        else v = lse3(prev[s], (s + 1 < S) ? prev[s + 1] : -INFINITY, skipb ? prev[s + 2] : -INFINITY) + lp;
        beta[abase + (long)t * Smax + s] = v;
        cur[s] = v;
      }
      __syncthreads();
    }
  }
}

// grid = B*T blocks
template <typename T>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const T* logits, T* grads, const float* __restrict__ lse,
                                                       const int32_t* __restrict__ labels, const int32_t* __restrict__ label_len,
                                                       const int32_t* __restrict__ logit_len, const float* __restrict__ grad_scale,
                                                       const float* __restrict__ alpha, const float* __restrict__ beta,
                                                       const float* __restrict__ costs, int Tm, int U, int V, int blank) {
  extern __shared__ float occ[];  // V floats
  const int b = blockIdx.x / Tm, t = blockIdx.x % Tm;
  const int Tl = min(logit_len[b], Tm), Ul = max(min(label_len[b], U), 0);  // a negative length is an empty one, as in csrc/align.hip
  const T* row = logits + ((long)b * Tm + t) * V;
  T* out = grads + ((long)b * Tm + t) * V;
  if (t >= Tl) { for (int v = threadIdx.x; v < V; v += blockDim.x) Num<T>::st(out + v, 0.f); return; }
  for (int v = threadIdx.x; v < V; v += blockDim.x) occ[v] = 0.f;
  __syncthreads();
  const int S = 2 * Ul + 1, Smax = 2 * U + 1;
  const float logp = -costs[b];
  const float l = lse[(long)b * Tm + t];
  const long abase = ((long)b * Tm + t) * Smax;
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    const int lab = (s & 1) ? min(max(labels[(long)b * U + (s >> 1)], 0), V - 1) : blank;
    const float lp = Num<T>::ld(row + lab) - l;
    const float e = alpha[abase + s] + beta[abase + s] - lp - logp;
    if (e > -80.f) atomicAdd(&occ[lab], expf(e));
  }
  __syncthreads();
  const float sc = grad_scale ? grad_scale[b] : 1.f;
  const bool finite = isfinite(logp);
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    const float p = expf(Num<T>::ld(row + v) - l);
    Num<T>::st(out + v, finite ? (p - occ[v]) * sc : 0.f);
  }
}

// merge repeated + drop blanks (tf.nn.ctc_greedy_decoder); one thread per utterance
__global__ void ctc_collapse_kernel(const int32_t* __restrict__ amax, const int32_t* __restrict__ logit_len, int32_t* __restrict__ out,
                                    int32_t* __restrict__ out_len, int B, int Tm, int blank, int32_t* __restrict__ last = nullptr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int Tl = min(logit_len[b], Tm);
  int prev = last ? last[b] : -1, n = 0;  // last: the class of the stream's previous frame (tfasr_ctc_greedy_decode_carry)
  for (int t = 0; t < Tl; ++t) {
    const int c = amax[(long)b * Tm + t];
    if (c != prev && c != blank) out[(long)b * Tm + n++] = c;
    prev = c;
  }
  for (int i = n; i < Tm; ++i) out[(long)b * Tm + i] = blank;
  out_len[b] = n;
  if (last && Tl > 0) last[b] = prev;
}

// The per-frame pass of tfasr_ctc_greedy_decode_detail: ctc_lse_kernel's arg-max (same loop, same tie rule: the tokens are those of
// tfasr_ctc_greedy_decode) plus the arg-max's log-softmax value, -log(sum_v e_v) with e_v = exp(x_v - max), and the entropy of the frame's
// distribution H = -sum_v p_v log p_v = log(sum_v e_v) + sum_v e_v (max - x_v) / sum_v e_v (two non-negative terms; a class with
// e_v == 0 is left out, so a logit of -inf contributes 0 and 0 * -inf never forms).  One wave per frame, grid-stride over the frames.
// ctc_frame_detail is one frame of it, by one wave: every lane returns the arg-max mi and the wave sums s = sum_v e_v and a = sum_v e_v (max -
// x_v); the offline kernel and the streamed one (ctc_carry_detail_kernel) finish them with the same three expressions, so both give a
// frame the same bits.
struct CtcFrame { int mi; float s, a; };

template <typename T>
__device__ __forceinline__ CtcFrame ctc_frame_detail(const T* __restrict__ row, int V, int lane) {
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int v = lane; v < V; v += 64) { const float x = Num<T>::ld(row + v); if (x > m) { m = x; mi = v; } }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  float s = 0.f, a = 0.f;
  for (int v = lane; v < V; v += 64) {
    const float d = Num<T>::ld(row + v) - m, e = expf(d);
    s += e;
    if (e > 0.f) a -= e * d;
  }
  s = wave_sum(s);
  a = wave_sum(a);
  return {mi, s, a};
}

template <typename T>
__global__ __launch_bounds__(256) void ctc_frame_detail_kernel(const T* __restrict__ logits, int32_t* __restrict__ amax, float* __restrict__ frame_lp,
                                                               float* __restrict__ frame_ent, long rows, int V) {
  const int lane = threadIdx.x & 63;
  const long w0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (long)gridDim.x * (blockDim.x >> 6);
  for (long r = w0; r < rows; r += nw) {
    const CtcFrame f = ctc_frame_detail(logits + r * V, V, lane);
    if (lane == 0) {
      const float ls = logf(f.s);
      amax[r] = f.mi;
      frame_lp[r] = -ls;
      frame_ent[r] = ls + f.a / f.s;
    }
  }
}

// tfasr_row_lse_entropy: ctc_frame_detail per row with ctc_lse_kernel's lse next to the entropy.  The maximum is the arg-max's own logit
// and s is ctc_lse_kernel's sum (the same terms in the same order), so lse = m + logf(s) has ctc_lse_kernel's bits.
template <typename T>
__global__ __launch_bounds__(256) void ctc_lse_entropy_kernel(const T* __restrict__ logits, float* __restrict__ lse, float* __restrict__ entropy,
                                                              long rows, int V) {
  const int lane = threadIdx.x & 63;
  const long w0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = (long)gridDim.x * (blockDim.x >> 6);
  for (long r = w0; r < rows; r += nw) {
    const T* row = logits + r * V;
    const CtcFrame f = ctc_frame_detail(row, V, lane);
    if (lane == 0) {
      const float m = (f.mi >= 0 && f.mi < V) ? Num<T>::ld(row + f.mi) : -INFINITY;  // (no class above -inf: ctc_lse_kernel's m)
      const float ls = logf(f.s);
      lse[r] = m + ls;
      entropy[r] = ls + f.a / f.s;
    }
  }
}

// tfasr_ctc_greedy_decode_carry_detail: one chunk [C, V] of a stream per workgroup, ONE launch.  The waves take the chunk's valid frames in
// tiles of CTC_CARRY_TILE (one wave per frame, ctc_frame_detail), the tile's arg-max / log-probability / entropy wait in LDS, and after the
// barrier thread 0 continues ctc_collapse_detail_kernel's serial loop over them from the carried state: the same additions in the same
// frame order, so a token's sums do not depend on where the chunks were cut.  Frames are global: g = seen + t.
// sti [B, 4] = {class of the previous frame (-1: none), frames seen, a token is open, its first frame}; stf [B, 3] = {its log-probability
// sum, its entropy sum, the path score}.  Output row b, C + 1 columns: column 0 = the token open on entry, columns 1 .. n = the tokens that
// start in this chunk.
constexpr int CTC_CARRY_TILE = 32;
constexpr int CTC_CARRY_THREADS = 1024;

template <typename T>
__global__ __launch_bounds__(CTC_CARRY_THREADS) void ctc_carry_detail_kernel(
    const T* __restrict__ logits, const int32_t* __restrict__ logit_len, const int32_t* __restrict__ final_flag, int32_t* __restrict__ sti,
    float* __restrict__ stf, int32_t* __restrict__ out, int32_t* __restrict__ out_len, int32_t* __restrict__ starts, int32_t* __restrict__ ends,
    float* __restrict__ tok_logp, float* __restrict__ tok_entropy, int C, int V, int blank) {
  __shared__ int32_t s_amax[CTC_CARRY_TILE];
  __shared__ float s_lp[CTC_CARRY_TILE], s_ent[CTC_CARRY_TILE];
  __shared__ int s_n;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int Tl = min(max(logit_len[b], 0), C);  // (uniform over the workgroup: every thread meets every barrier)
  const bool fin = final_flag[b] != 0;
  const long base = (long)b * (C + 1);
  // thread 0's registers: the collapse's state
  int prev = -1, seen = 0, start = 0, n = 0, col = 0;  // col: the column of the open token
  bool open = false;
  float lp_run = 0.f, ent_run = 0.f, total = 0.f;
  if (threadIdx.x == 0) {  // (nothing depends on these loads before the first barrier: their latency hides behind the frame pass)
    prev = sti[b * 4 + 0];
    seen = sti[b * 4 + 1];
    open = sti[b * 4 + 2] != 0;
    start = sti[b * 4 + 3];
    lp_run = stf[b * 3 + 0];
    ent_run = stf[b * 3 + 1];
    total = stf[b * 3 + 2];
  }
  const bool open0 = open;  // column 0: the token open on entry
  const int cls0 = prev, start0 = start;
  for (int t0 = 0; t0 < Tl; t0 += CTC_CARRY_TILE) {
    const int nt = min(CTC_CARRY_TILE, Tl - t0);
    for (int i = wave; i < nt; i += nwaves) {
      const CtcFrame f = ctc_frame_detail(logits + ((long)b * C + t0 + i) * V, V, lane);
      if (lane == 0) {
        const float ls = logf(f.s);
        s_amax[i] = f.mi;
        s_lp[i] = -ls;
        s_ent[i] = ls + f.a / f.s;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < nt; ++i) {
        const int c = s_amax[i], g = seen + t0 + i;
        if (c != prev) {
          if (open) {
            ends[base + col] = g;
            tok_logp[base + col] = lp_run;
            tok_entropy[base + col] = ent_run / (float)(g - start);
            open = false;
          }
          if (c != blank) {
            col = ++n;
            out[base + col] = c;
            starts[base + col] = g;
            start = g;
            lp_run = 0.f;
            ent_run = 0.f;
            open = true;
          }
        }
        const float lp = s_lp[i];
        total += lp;
        if (open) { lp_run += lp; ent_run += s_ent[i]; }
        prev = c;
      }
    }
    __syncthreads();  // (the next tile overwrites the LDS rows)
  }
  if (threadIdx.x == 0) {
    const int g = seen + Tl;
    out[base] = open0 ? cls0 : blank;
    starts[base] = open0 ? start0 : -1;
    if (!open0) { ends[base] = -1; tok_logp[base] = 0.f; tok_entropy[base] = 0.f; }
    if (open) {  // closed by the final flag, or left open with the sum and the mean over its frames so far
      ends[base + col] = fin ? g : -1;
      tok_logp[base + col] = lp_run;
      tok_entropy[base + col] = ent_run / (float)(g - start);
      if (fin) open = false;
    }
    out_len[b] = n;
    if (Tl > 0 || fin) {  // (a row without frames and without the flag keeps its state)
      sti[b * 4 + 0] = prev;
      sti[b * 4 + 1] = g;
      sti[b * 4 + 2] = open ? 1 : 0;
      sti[b * 4 + 3] = start;
      stf[b * 3 + 0] = lp_run;
      stf[b * 3 + 1] = ent_run;
      stf[b * 3 + 2] = total;
    }
    s_n = n;
  }
  __syncthreads();
  for (int i = s_n + 1 + threadIdx.x; i <= C; i += blockDim.x) {
    out[base + i] = blank;
    starts[base + i] = -1;
    ends[base + i] = -1;
    tok_logp[base + i] = 0.f;
    tok_entropy[base + i] = 0.f;
  }
}

// ctc_collapse_kernel with the span of every token: [starts, ends) = its run of equal arg-max classes, tok_logp = the frame log-probabilities
// summed over the run in frame order, tok_entropy = the mean frame entropy of the run; score = the sum over all valid frames, blanks
// included (the log-probability of the best path).  One thread per utterance.
__global__ void ctc_collapse_detail_kernel(const int32_t* __restrict__ amax, const float* __restrict__ frame_lp, const float* __restrict__ frame_ent,
                                           const int32_t* __restrict__ logit_len, int32_t* __restrict__ out, int32_t* __restrict__ out_len,
                                           int32_t* __restrict__ starts, int32_t* __restrict__ ends, float* __restrict__ tok_logp,
                                           float* __restrict__ tok_entropy, float* __restrict__ score, int B, int Tm, int blank) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int Tl = min(logit_len[b], Tm);
  const long base = (long)b * Tm;
  int prev = -1, n = 0, start = 0;
  bool open = false;  // a token's run is being summed
  float lp_run = 0.f, ent_run = 0.f, total = 0.f;
  for (int t = 0; t <= Tl; ++t) {
    const int c = t < Tl ? amax[base + t] : -1;  // (t == Tl: closes a run that reaches the last valid frame)
    if (c != prev || t == Tl) {
      if (open) {
        ends[base + n - 1] = t;
        tok_logp[base + n - 1] = lp_run;
        tok_entropy[base + n - 1] = ent_run / (float)(t - start);
        open = false;
      }
      if (t < Tl && c != blank) {
        out[base + n] = c;
        starts[base + n] = t;
        ++n;
        start = t;
        lp_run = 0.f;
        ent_run = 0.f;
        open = true;
      }
    }
    if (t < Tl) {
      const float lp = frame_lp[base + t];
      total += lp;
      if (open) { lp_run += lp; ent_run += frame_ent[base + t]; }
    }
    prev = c;
  }
  for (int i = n; i < Tm; ++i) {
    out[base + i] = blank;
    starts[base + i] = -1;
    ends[base + i] = -1;
    tok_logp[base + i] = 0.f;
    tok_entropy[base + i] = 0.f;
  }
  out_len[b] = n;
  score[b] = total;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// The per-frame pass of the loss, shared with the forced alignment (csrc/align.hip).
int tfasr_detail::ctc_row_lse(const void* logits, float* lse, long rows, int V, int dtype, hipStream_t stream) {
  const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
  if (dtype == TFASR_F32) TFASR_KLAUNCH(ctc_lse_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)logits, lse, (int32_t*)nullptr, rows, V);
  else if (dtype == TFASR_BF16) TFASR_KLAUNCH(ctc_lse_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)logits, lse, (int32_t*)nullptr, rows, V);
  else return TFASR_STATUS_INVALID_VALUE;
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

int tfasr_detail::ctc_row_lse_entropy(const void* logits, float* lse, float* entropy, long rows, int V, int dtype, hipStream_t stream) {
  if (!entropy) return ctc_row_lse(logits, lse, rows, V, dtype, stream);
  const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
  if (dtype == TFASR_F32) TFASR_KLAUNCH(ctc_lse_entropy_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)logits, lse, entropy, rows, V);
  else if (dtype == TFASR_BF16) TFASR_KLAUNCH(ctc_lse_entropy_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)logits, lse, entropy, rows, V);
  else return TFASR_STATUS_INVALID_VALUE;
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_loss_workspace_size(int B, int T, int U, int V, size_t* bytes) {
  if (!bytes || B <= 0 || T <= 0 || U < 0 || V <= 0) return TFASR_STATUS_INVALID_VALUE;
  const size_t S = 2 * (size_t)U + 1;
  *bytes = align256((size_t)B * T * 4) + 2 * align256((size_t)B * T * S * 4);
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_loss(const void* logits, void* grads, const int32_t* labels, const int32_t* label_len,
                              const int32_t* logit_len, const float* grad_scale, int B, int T, int U, int V, int blank,
                              int dtype, float* costs, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!logits || !labels || !label_len || !logit_len || !costs || !workspace) return TFASR_STATUS_INVALID_VALUE;
  if (B <= 0 || T <= 0 || U < 0 || V <= 1 || blank < 0 || blank >= V || 2 * U + 1 > 1024) return TFASR_STATUS_INVALID_VALUE;
  size_t need = 0;
  tfasr_ctc_loss_workspace_size(B, T, U, V, &need);
  if (workspace_bytes < need) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  const size_t S = 2 * (size_t)U + 1;
  char* ws = (char*)workspace;
  float* lse = (float*)ws;
  float* alpha = (float*)(ws + align256((size_t)B * T * 4));
  float* beta = (float*)(ws + align256((size_t)B * T * 4) + align256((size_t)B * T * S * 4));
  const long rows = (long)B * T;
  const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
  const int nthr = (int)((S + 63) / 64) * 64;
  if (dtype == TFASR_F32) {
    TFASR_KLAUNCH(ctc_lse_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)logits, lse, (int32_t*)nullptr, rows, V);
    TFASR_KLAUNCH(ctc_scan_kernel<float>, dim3(B, 2), dim3(nthr), 2 * nthr * sizeof(float), s, (const float*)logits, lse, labels, label_len, logit_len, T, U, V, blank, alpha, beta, costs);
    if (grads) TFASR_KLAUNCH(ctc_grad_kernel<float>, dim3(B * T), dim3(256), V * sizeof(float), s, (const float*)logits, (float*)grads, lse, labels, label_len, logit_len, grad_scale, alpha, beta, costs, T, U, V, blank);
  } else if (dtype == TFASR_BF16) {
    TFASR_KLAUNCH(ctc_lse_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)logits, lse, (int32_t*)nullptr, rows, V);
    TFASR_KLAUNCH(ctc_scan_kernel<bf16_t>, dim3(B, 2), dim3(nthr), 2 * nthr * sizeof(float), s, (const bf16_t*)logits, lse, labels, label_len, logit_len, T, U, V, blank, alpha, beta, costs);
    if (grads) TFASR_KLAUNCH(ctc_grad_kernel<bf16_t>, dim3(B * T), dim3(256), V * sizeof(float), s, (const bf16_t*)logits, (bf16_t*)grads, lse, labels, label_len, logit_len, grad_scale, alpha, beta, costs, T, U, V, blank);
  } else return TFASR_STATUS_INVALID_VALUE;
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_greedy_decode(const void* logits, const int32_t* logit_len, int32_t* workspace_argmax, int32_t* tokens,
                                       int32_t* tokens_len, int B, int T, int V, int blank, int dtype, void* stream_) {
  if (!logits || !logit_len || !workspace_argmax || !tokens || !tokens_len || B <= 0 || T <= 0 || V <= 0) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  const long rows = (long)B * T;
  const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
  if (dtype == TFASR_F32) TFASR_KLAUNCH(ctc_lse_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)logits, (float*)nullptr, workspace_argmax, rows, V);
  else if (dtype == TFASR_BF16) TFASR_KLAUNCH(ctc_lse_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)logits, (float*)nullptr, workspace_argmax, rows, V);
  else return TFASR_STATUS_INVALID_VALUE;
  TFASR_KLAUNCH(ctc_collapse_kernel, dim3((B + 63) / 64), dim3(64), 0, s, workspace_argmax, logit_len, tokens, tokens_len, B, T, blank);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_greedy_decode_carry(const void* logits, const int32_t* logit_len, int32_t* last_class, int32_t* workspace_argmax,
                                             int32_t* tokens, int32_t* tokens_len, int B, int T, int V, int blank, int dtype, void* stream_) {
  if (!logits || !logit_len || !last_class || !workspace_argmax || !tokens || !tokens_len || B <= 0 || T <= 0 || V <= 0)
    return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  const long rows = (long)B * T;
  const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
  if (dtype == TFASR_F32) TFASR_KLAUNCH(ctc_lse_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)logits, (float*)nullptr, workspace_argmax, rows, V);
  else if (dtype == TFASR_BF16) TFASR_KLAUNCH(ctc_lse_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)logits, (float*)nullptr, workspace_argmax, rows, V);
  else return TFASR_STATUS_INVALID_VALUE;
  TFASR_KLAUNCH(ctc_collapse_kernel, dim3((B + 63) / 64), dim3(64), 0, s, workspace_argmax, logit_len, tokens, tokens_len, B, T, blank, last_class);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_greedy_decode_detail(const void* logits, const int32_t* logit_len, int32_t* workspace, int32_t* tokens, int32_t* tokens_len,
                                              int32_t* starts, int32_t* ends, float* tok_logp, float* tok_entropy, float* score, int B, int T,
                                              int V, int blank, int dtype, void* stream_) {
  if (!logits || !logit_len || !workspace || !tokens || !tokens_len || !starts || !ends || !tok_logp || !tok_entropy || !score || B <= 0 ||
      T <= 0 || V <= 0)
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  const long rows = (long)B * T;
  const int grid = (int)std::max<long>(1, std::min<long>((rows + 3) / 4, 8192));
  int32_t* amax = workspace;
  float* frame_lp = (float*)(workspace + rows);
  float* frame_ent = (float*)(workspace + 2 * rows);
  if (dtype == TFASR_F32) TFASR_KLAUNCH(ctc_frame_detail_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)logits, amax, frame_lp, frame_ent, rows, V);
  else TFASR_KLAUNCH(ctc_frame_detail_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)logits, amax, frame_lp, frame_ent, rows, V);
  TFASR_KLAUNCH(ctc_collapse_detail_kernel, dim3((B + 63) / 64), dim3(64), 0, s, amax, frame_lp, frame_ent, logit_len, tokens, tokens_len, starts, ends,
                tok_logp, tok_entropy, score, B, T, blank);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_ctc_greedy_decode_carry_detail(const void* logits, const int32_t* logit_len, const int32_t* final_flag, int32_t* state_i,
                                                    float* state_f, int32_t* tokens, int32_t* tokens_len, int32_t* starts, int32_t* ends,
                                                    float* tok_logp, float* tok_entropy, int B, int C, int V, int blank, int dtype, void* stream_) {
  if (!logits || !logit_len || !final_flag || !state_i || !state_f || !tokens || !tokens_len || !starts || !ends || !tok_logp || !tok_entropy)
    return TFASR_STATUS_INVALID_VALUE;
  if (B <= 0 || C <= 0 || V < 2 || blank < 0 || blank >= V) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  if (dtype == TFASR_F32)
    TFASR_KLAUNCH(ctc_carry_detail_kernel<float>, dim3(B), dim3(CTC_CARRY_THREADS), 0, s, (const float*)logits, logit_len, final_flag, state_i, state_f,
                  tokens, tokens_len, starts, ends, tok_logp, tok_entropy, C, V, blank);
  else
    TFASR_KLAUNCH(ctc_carry_detail_kernel<bf16_t>, dim3(B), dim3(CTC_CARRY_THREADS), 0, s, (const bf16_t*)logits, logit_len, final_flag, state_i, state_f,
                  tokens, tokens_len, starts, ends, tok_logp, tok_entropy, C, V, blank);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
