// Batched edit distance (Levenshtein, unit costs) of P pairs of int32 sequences for gfx950, with the counts behind WER / MER / WIL.
//
// Pair p scores a hypothesis (row p of hyp [P,N]) against a reference (row p of ref [P,M]).  A row's sequence is its first
// clamp(len, 0, width) entries when a length array is given, and otherwise what is left of the row after dropping entries < 0 and
// entries == skip_id, order kept (the searches hand back blank-padded tokens, with -1 in sparse-to-dense decodes).  Either way the
// sequence is built in LDS by the kernel's load phase; nothing past a given length is ever read.
//
// counts[p] = (distance, hits, substitutions, deletions, insertions).  The distance is unique, the counts are not: they are those of the
// minimum-distance alignment with the MOST hits (equivalently the fewest substitutions).  With d, n = |hyp| and m = |ref| fixed the hit
// count H fixes the rest (I = d - (m - H), D = I + m - n, S = m - H - D), so one forward pass over the lexicographic value
// (distance, -hits) is all there is: no decision is stored and nothing is traced back.  The value is one int32 dist * 65536 - hits
// (both at most TFASR_EDIT_MAX_LEN = 4096):
//   v[0][j] = j << 16,  v[i][0] = i << 16,
//   v[i][j] = min(v[i-1][j-1] + (hyp[i-1] == ref[j-1] ? -1 : 65536), v[i-1][j] + 65536 /* insertion */, v[i][j-1] + 65536 /* deletion */)
// Integer arithmetic only.
//
// Kernels:
//   1. edit_wave<E> : one wave per pair, M <= 64 * E (E = 1, 2, 4, 8).  A lane owns E adjacent reference columns and walks the hypothesis
//                     rows skewed by its lane index (lane l is on row s - l + 1 at step s); its left neighbour's last column arrives by
//                     one DPP wave shift per step, the value it carried in the step before is the diagonal.  The hypothesis symbol of the
//                     next step is read from LDS a step ahead.  Nothing is written per cell; one lane stores the five counts.
//   2. edit_wg      : one workgroup per pair, a thread owns 4 columns (up to 1024 threads, M <= 4096), the same skewed walk with the
//                     neighbour's column through a double-buffered LDS row and one barrier per step.
// Columns past the reference's length compute on unused values; a column only ever feeds columns to its right, so they cannot reach
// the answer.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxLen = TFASR_EDIT_MAX_LEN;
constexpr int kUnit = 65536;   // one edit; a hit subtracts 1
constexpr int kWgCols = 4;     // columns per thread of the workgroup kernel
constexpr size_t kWorkspaceBytes = 256;  // both rows live in LDS; the workspace is reserved

// Builds the row's sequence in LDS (sh, room for `width` entries) with the threads of ONE wave and returns its length (wave-uniform).
__device__ __forceinline__ int load_row(const int32_t* __restrict__ row, const int32_t* __restrict__ len, int pair, int width, int skip_id,
                                        int lane, int32_t* sh) {
  if (len) {
    const int n = min(max(len[pair], 0), width);
    for (int k = lane; k < n; k += 64) sh[k] = row[k];
    return n;
  }
  int n = 0;
  for (int k0 = 0; k0 < width; k0 += 64) {
    const int k = k0 + lane;
    const int x = k < width ? row[k] : -1;
    const bool keep = x >= 0 && x != skip_id;
    const u64 mask = __ballot(keep);
    if (keep) sh[n + __popcll(mask & ((1ull << lane) - 1ull))] = x;
    n += __popcll(mask);
  }
  return n;
}

__device__ __forceinline__ void store_counts(int32_t* __restrict__ out, int v, int n, int m) {
  const int d = (v + kUnit - 1) >> 16;
  const int hits = d * kUnit - v;
  const int ins = d - (m - hits);
  const int del = ins + m - n;
  out[0] = d;
  out[1] = hits;
  out[2] = m - hits - del;
  out[3] = del;
  out[4] = ins;
}

// grid P, 64 threads, dynamic LDS (N + M) * 4 bytes
template <int E>
__global__ __launch_bounds__(64) void edit_wave_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
                                                       const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int N, int M,
                                                       int skip_id, int32_t* __restrict__ counts) {
  extern __shared__ int32_t sh[];
  int32_t* sh_hyp = sh;
  int32_t* sh_ref = sh + N;
  const int p = blockIdx.x, lane = threadIdx.x;
  const int n = load_row(hyp + (long)p * N, hyp_len, p, N, skip_id, lane, sh_hyp);
  const int m = load_row(ref + (long)p * M, ref_len, p, M, skip_id, lane, sh_ref);
  __syncthreads();
  int32_t* out = counts + (long)p * 5;
  if (n == 0 || m == 0) {
    if (lane == 0) store_counts(out, (n + m) * kUnit, n, m);
    return;
  }
  const int col0 = lane * E;  // this lane owns columns col0 + 1 .. col0 + E
  int rs[E], self[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    rs[e] = col0 + e < m ? sh_ref[col0 + e] : -1;
    self[e] = (col0 + e + 1) * kUnit;  // row 0
  }
  int diag = col0 * kUnit;
  const int steps = n + (m + E - 1) / E - 1;  // the lane of column m finishes row n in the last one
  int hs_next = sh_hyp[0];                    // the symbol of row 1 (only lane 0 is on it in step 0)
  for (int s = 0; s < steps; ++s) {
    const int i = s - lane + 1;  // the row this lane is on
    const bool act = i >= 1 && i <= n;
    const int hs = hs_next;
    hs_next = sh_hyp[min(max(i, 0), n - 1)];  // row i + 1
    int left = __builtin_amdgcn_update_dpp(0, self[E - 1], 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    if (lane == 0) left = max(i, 0) * kUnit;
    int dg = diag, lf = left;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int up = self[e];
      const int v = min(min(up, lf) + kUnit, dg + (hs == rs[e] ? -1 : kUnit));
      dg = up;
      self[e] = act ? v : up;
      lf = self[e];
    }
    diag = left;
  }
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (col0 + e + 1 == m) store_counts(out, self[e], n, m);
}

// grid P, NT threads (a multiple of 64 with NT * kWgCols >= M), dynamic LDS (N + M + 2 * NT) * 4 bytes
__global__ __launch_bounds__(1024) void edit_wg_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
                                                       const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int N, int M,
                                                       int skip_id, int32_t* __restrict__ counts) {
  extern __shared__ int32_t sh[];
  __shared__ int sh_nm[2];
  int32_t* sh_hyp = sh;
  int32_t* sh_ref = sh + N;
  int32_t* edge = sh + N + M;  // [2][NT]: a thread's last column after the even / odd steps
  const int p = blockIdx.x, t = threadIdx.x, NT = blockDim.x;
  if (t < 64) {  // one wave builds a row (the compaction's running position is a wave's)
    const int n_ = load_row(hyp + (long)p * N, hyp_len, p, N, skip_id, t, sh_hyp);
    if (t == 0) sh_nm[0] = n_;
  } else if (t < 128) {
    const int m_ = load_row(ref + (long)p * M, ref_len, p, M, skip_id, t - 64, sh_ref);
    if (t == 64) sh_nm[1] = m_;
  }
  const int col0 = t * kWgCols;
  edge[t] = edge[NT + t] = (col0 + kWgCols) * kUnit;  // row 0
  __syncthreads();
  const int n = sh_nm[0], m = sh_nm[1];
  int32_t* out = counts + (long)p * 5;
  if (n == 0 || m == 0) {
    if (t == 0) store_counts(out, (n + m) * kUnit, n, m);
    return;
  }
  int rs[kWgCols], self[kWgCols];
#pragma unroll
  for (int e = 0; e < kWgCols; ++e) {
    rs[e] = col0 + e < m ? sh_ref[col0 + e] : -1;
    self[e] = (col0 + e + 1) * kUnit;
  }
  int diag = col0 * kUnit;
  const int steps = n + (m + kWgCols - 1) / kWgCols - 1;
  for (int s = 0; s < steps; ++s) {
    const int i = s - t + 1;
    const bool act = i >= 1 && i <= n;
    const int32_t* prev = edge + ((s + 1) & 1) * NT;  // written in step s - 1
    int32_t* cur = edge + (s & 1) * NT;
    const int left = t == 0 ? max(i, 0) * kUnit : prev[t - 1];
    if (act) {
      const int hs = sh_hyp[i - 1];
      int dg = diag, lf = left;
#pragma unroll
      for (int e = 0; e < kWgCols; ++e) {
        const int up = self[e];
        self[e] = min(min(up, lf) + kUnit, dg + (hs == rs[e] ? -1 : kUnit));
        dg = up;
        lf = self[e];
      }
    }
    diag = left;
    cur[t] = self[kWgCols - 1];
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < kWgCols; ++e)
    if (col0 + e + 1 == m) store_counts(out, self[e], n, m);
}

int shape_status(int P, int N, int M) {
  if (P <= 0 || N < 0 || M < 0) return TFASR_STATUS_INVALID_VALUE;
  if (N > kMaxLen || M > kMaxLen) return TFASR_STATUS_UNSUPPORTED;
  return TFASR_STATUS_SUCCESS;
}

}  // namespace

extern "C" int tfasr_edit_distance_workspace_size(int P, int N, int M, size_t* bytes) {
  if (!bytes) return TFASR_STATUS_INVALID_VALUE;
  const int st = shape_status(P, N, M);
  if (st != TFASR_STATUS_SUCCESS) return st;
  *bytes = kWorkspaceBytes;
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_edit_distance(const int32_t* hyp, const int32_t* hyp_len, const int32_t* ref, const int32_t* ref_len, int P, int N, int M,
                                   int skip_id, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!hyp || !ref || !counts || !workspace) return TFASR_STATUS_INVALID_VALUE;
  const int st = shape_status(P, N, M);
  if (st != TFASR_STATUS_SUCCESS) return st;
  if (workspace_bytes < kWorkspaceBytes) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t rows = ((size_t)N + M) * sizeof(int32_t);
#define TFASR_EW(E_) TFASR_KLAUNCH((edit_wave_kernel<E_>), dim3(P), dim3(64), rows, stream, hyp, hyp_len, ref, ref_len, N, M, skip_id, counts)
  if (M <= 64) TFASR_EW(1);
  else if (M <= 128) TFASR_EW(2);
  else if (M <= 256) TFASR_EW(4);
  else if (M <= 512) TFASR_EW(8);
  else {
    const int NT = ((M + kWgCols - 1) / kWgCols + 63) / 64 * 64;
    TFASR_KLAUNCH(edit_wg_kernel, dim3(P), dim3(NT), rows + 2 * NT * sizeof(int32_t), stream, hyp, hyp_len, ref, ref_len, N, M, skip_id, counts);
  }
#undef TFASR_EW
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
