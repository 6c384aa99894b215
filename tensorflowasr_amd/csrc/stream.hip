// Streaming (chunk-by-chunk) Conformer encoder for gfx950: the kernels that read or write state carried between chunks.
//
// One step processes B streams x at most C encoder frames (C = chunk_size of the streaming config, multihead_attention.py:104-143
// compute_streaming_mask: query chunk c sees keys [c C - hist, c C + C)).  The dense pieces of a block run on the forward kernels of
// training with T = C; what is here:
//   stream_attn_kernel       : the chunk's queries against (key / value ring of the last `hist` frames) ++ (the chunk's own keys)
//   stream_kv_append_kernel  : the chunk's keys / values into the ring (its own launch AFTER the attention: every head of the attention
//                              launch still reads the slots this overwrites - they lie inside the chunk's window)
//   stream_glu_dwconv_kernel : GLU + causal depthwise conv whose left context is a carried [K-1, d] state, updated in place
// Streams of one batch stand at different offsets (seen[b]) and may be idle (nvalid[b] == 0): both are DEVICE vectors, nothing goes
// through the host, and an idle stream's state is not written at all.
// At these sizes (16 x 80 scores per head) every kernel is latency-bound: plain f32 FMAs (exact f32 products, as the search step
// kernels), no MFMA tiles, one launch per layer each.
#include "common.h"

namespace {

constexpr int MAXC = TFASR_STREAM_MAX_CHUNK, MAXK = TFASR_STREAM_MAX_KEYS, MAXDH = TFASR_STREAM_MAX_HEAD;
constexpr int S_FLOATS = 8192;  // score tile in LDS: query rows are walked in groups of floor(S_FLOATS / keys) >= 16 rows

template <typename T> __device__ __forceinline__ float round_as(float v);
template <> __device__ __forceinline__ float round_as<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_as<bf16_t>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// dot products of one (query, key) pair: (q + u) . k and (q + v) . p, dh elements, 8 at a time when VEC
template <typename T, bool VEC>
__device__ __forceinline__ float score_pair(const float* __restrict__ qu, const float* __restrict__ qv, const T* __restrict__ k,
                                            const T* __restrict__ p, int dh) {
  float a = 0.f, c = 0.f;
  if (VEC) {
    for (int e = 0; e < dh; e += 8) {
      float kk[8], pp[8];
      ld8(k + e, kk);
      ld8(p + e, pp);
#pragma unroll
      for (int t = 0; t < 8; ++t) { a = fmaf(qu[e + t], kk[t], a); c = fmaf(qv[e + t], pp[t], c); }
    }
  } else {
    for (int e = 0; e < dh; ++e) { a = fmaf(qu[e], Num<T>::ld(k + e), a); c = fmaf(qv[e], Num<T>::ld(p + e), c); }
  }
  return a + c;
}

// grid (H, B), 256 threads.  Key jj of stream b: jj < nh = min(seen, hist) is frame seen - nh + jj, ring slot (seen - nh + jj) % hist;
// jj >= nh is row jj - nh of this chunk.  Query row i is frame seen + i, so key jj sits at relative position i + nh - jj, which is row
// hist + C - 1 - (i + nh - jj) of the constant table pos [hist + 2C - 1, HD] (row r <-> position hist + C - 1 - r): an index skew.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void stream_attn_kernel(const T* __restrict__ qkv, const float* __restrict__ ub, const float* __restrict__ vb,
                                                          const T* __restrict__ pos, const T* __restrict__ kc, const T* __restrict__ vc,
                                                          const int32_t* __restrict__ seen, const int32_t* __restrict__ nvalid,
                                                          T* __restrict__ out, int C, int H, int dh, int hist, float scale) {
  __shared__ float S[S_FLOATS];
  __shared__ float Q[2][MAXC * MAXDH];
  const int h = blockIdx.x, b = blockIdx.y, HD = H * dh;
  const int nv = min(max(nvalid[b], 0), C), sn = max(seen[b], 0);
  T* ob = out + (long)b * C * HD + h * dh;
  for (int i = nv * dh + threadIdx.x; i < C * dh; i += blockDim.x) Num<T>::st(ob + (long)(i / dh) * HD + i % dh, 0.f);
  if (nv == 0) return;
  const int nh = min(sn, hist), nk = nh + nv;
  const int rg = min(nv, S_FLOATS / nk);  // nk <= MAXK = 512: at least 16 rows per group
  const T* qb = qkv + (long)b * C * 3 * HD + h * dh;
  const T* kcb = kc + (long)b * hist * HD + h * dh;
  const T* vcb = vc + (long)b * hist * HD + h * dh;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i0 = 0; i0 < nv; i0 += rg) {
    const int nr = min(rg, nv - i0);
    __syncthreads();
    for (int i = threadIdx.x; i < nr * dh; i += blockDim.x) {
      const int r = i / dh, e = i % dh;
      const float q = Num<T>::ld(qb + (long)(i0 + r) * 3 * HD + e);
      Q[0][r * dh + e] = q + ub[h * dh + e];
      Q[1][r * dh + e] = q + vb[h * dh + e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nr * nk; i += blockDim.x) {
      const int r = i / nk, jj = i % nk;
      const T* kp = jj < nh ? kcb + (long)((sn - nh + jj) % hist) * HD : qb + (long)(jj - nh) * 3 * HD + HD;
      const int rel = i0 + r + nh - jj;
      const T* pp = pos + (long)(hist + C - 1 - rel) * HD + h * dh;
      S[r * nk + jj] = score_pair<T, VEC>(&Q[0][r * dh], &Q[1][r * dh], kp, pp, dh) * scale;
    }
    __syncthreads();
    for (int r = w; r < nr; r += 4) {  // softmax of a row by one wave
      float* row = S + r * nk;
      float m = -INFINITY;
      for (int j = lane; j < nk; j += 64) m = fmaxf(m, row[j]);
      m = wave_max(m);
      float s = 0.f;
      for (int j = lane; j < nk; j += 64) { const float e = expf(row[j] - m); row[j] = e; s += e; }
      s = wave_sum(s);
      const float inv = 1.f / s;
      for (int j = lane; j < nk; j += 64) row[j] *= inv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nr * dh; i += blockDim.x) {
      const int r = i / dh, e = i % dh;
      const float* row = S + r * nk;
      float acc = 0.f;
      for (int jj = 0; jj < nh; ++jj) acc = fmaf(row[jj], Num<T>::ld(vcb + (long)((sn - nh + jj) % hist) * HD + e), acc);
      for (int jj = nh; jj < nk; ++jj) acc = fmaf(row[jj], Num<T>::ld(qb + (long)(jj - nh) * 3 * HD + 2 * HD + e), acc);
      Num<T>::st(ob + (long)(i0 + r) * HD + e, acc);
    }
  }
}

// grid (B): rows r of the chunk into slots (seen + r) % hist; with more valid rows than slots only the last `hist` rows (no two rows of
// one launch share a slot)
template <typename T>
__global__ __launch_bounds__(256) void stream_kv_append_kernel(const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc,
                                                               const int32_t* __restrict__ seen, const int32_t* __restrict__ nvalid, int C,
                                                               int HD, int hist) {
  const int b = blockIdx.x;
  const int nv = min(max(nvalid[b], 0), C), sn = max(seen[b], 0);
  const int r0 = max(0, nv - hist);
  for (int i = r0 * HD + threadIdx.x; i < nv * HD; i += blockDim.x) {
    const int r = i / HD, e = i % HD;
    const long src = ((long)b * C + r) * 3 * HD + HD + e;
    const long dst = ((long)b * hist + (sn + r) % hist) * HD + e;
    kc[dst] = qkv[src];
    vc[dst] = qkv[src + HD];
  }
}

// grid (ceil(d / 64), B), 256 threads = 64 channels x 4 row phases.  The K-1 state rows and the GLU of the chunk's valid rows go to LDS
// first; outputs and the new state are computed from LDS only, so the state is updated in place.
template <typename T>
__global__ __launch_bounds__(256) void stream_glu_dwconv_kernel(const T* __restrict__ a, T* __restrict__ state, const float* __restrict__ w,
                                                                const float* __restrict__ bias, const int32_t* __restrict__ nvalid,
                                                                T* __restrict__ y, int C, int d, int K) {
  __shared__ float g[(32 - 1 + MAXC) * 64];
  const int b = blockIdx.y, cl = threadIdx.x & 63, ph = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const int nv = min(max(nvalid[b], 0), C), K1 = K - 1;
  if (c < d)
    for (int r = nv + ph; r < C; r += 4) Num<T>::st(y + ((long)b * C + r) * d + c, 0.f);
  if (nv == 0) return;
  if (c < d) {
    for (int r = ph; r < K1; r += 4) g[r * 64 + cl] = Num<T>::ld(state + ((long)b * K1 + r) * d + c);
    for (int r = ph; r < nv; r += 4) {
      const T* row = a + ((long)b * C + r) * 2 * d;
      g[(K1 + r) * 64 + cl] = round_as<T>(Num<T>::ld(row + c) * sigmoidf_(Num<T>::ld(row + d + c)));
    }
  }
  __syncthreads();
  if (c >= d) return;
  for (int r = ph; r < nv; r += 4) {
    float acc = bias ? bias[c] : 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(g[(r + k) * 64 + cl], w[k * d + c], acc);
    Num<T>::st(y + ((long)b * C + r) * d + c, acc);
  }
  for (int r = ph; r < K1; r += 4) Num<T>::st(state + ((long)b * K1 + r) * d + c, g[(nv + r) * 64 + cl]);
}

}  // namespace

extern "C" int tfasr_stream_attn_fwd(const void* qkv, const float* ubias, const float* vbias, const void* pos, const void* kcache,
                                     const void* vcache, const int32_t* seen, const int32_t* nvalid, void* out, int B, int C, int H, int dh,
                                     int hist, float scale, int dtype, void* stream_) {
  if (!qkv || !ubias || !vbias || !pos || !seen || !nvalid || !out || B <= 0 || C <= 0 || H <= 0 || dh <= 0 || hist < 0)
    return TFASR_STATUS_INVALID_VALUE;
  if (hist > 0 && (!kcache || !vcache)) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (C > MAXC || (long)hist + C > MAXK || dh > MAXDH || B > 65535) return TFASR_STATUS_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream_;
  const bool vec = (dh % 8 == 0) && ((((uintptr_t)qkv | (uintptr_t)pos | (uintptr_t)kcache) & 15) == 0);
#define TFASR_SA(TT, VV) TFASR_KLAUNCH((stream_attn_kernel<TT, VV>), dim3(H, B), dim3(256), 0, s, (const TT*)qkv, ubias, vbias, (const TT*)pos, \
                                       (const TT*)kcache, (const TT*)vcache, seen, nvalid, (TT*)out, C, H, dh, hist, scale)
  if (dtype == TFASR_F32) { if (vec) TFASR_SA(float, true); else TFASR_SA(float, false); }
  else { if (vec) TFASR_SA(bf16_t, true); else TFASR_SA(bf16_t, false); }
#undef TFASR_SA
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_stream_kv_append(const void* qkv, void* kcache, void* vcache, const int32_t* seen, const int32_t* nvalid, int B, int C,
                                      int H, int dh, int hist, int dtype, void* stream_) {
  if (!qkv || !seen || !nvalid || B <= 0 || C <= 0 || H <= 0 || dh <= 0 || hist < 0) return TFASR_STATUS_INVALID_VALUE;
  if (hist > 0 && (!kcache || !vcache)) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (C > MAXC || (long)hist + C > MAXK || dh > MAXDH) return TFASR_STATUS_UNSUPPORTED;
  if (hist == 0) return TFASR_STATUS_SUCCESS;  // no ring to fill
  hipStream_t s = (hipStream_t)stream_;
  if (dtype == TFASR_F32)
    TFASR_KLAUNCH(stream_kv_append_kernel<float>, dim3(B), dim3(256), 0, s, (const float*)qkv, (float*)kcache, (float*)vcache, seen, nvalid, C, H * dh, hist);
  else
    TFASR_KLAUNCH(stream_kv_append_kernel<bf16_t>, dim3(B), dim3(256), 0, s, (const bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache, seen, nvalid, C, H * dh, hist);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_stream_glu_dwconv_fwd(const void* glu_x, void* state, const float* w, const float* bias, const int32_t* nvalid, void* y,
                                           int B, int C, int d, int K, int dtype, void* stream_) {
  if (!glu_x || !w || !nvalid || !y || B <= 0 || C <= 0 || d <= 0 || K <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (K > 1 && !state) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (C > MAXC || K > 32 || B > 65535) return TFASR_STATUS_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((d + 63) / 64, B);
  if (dtype == TFASR_F32)
    TFASR_KLAUNCH(stream_glu_dwconv_kernel<float>, grid, dim3(256), 0, s, (const float*)glu_x, (float*)state, w, bias, nvalid, (float*)y, C, d, K);
  else
    TFASR_KLAUNCH(stream_glu_dwconv_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)glu_x, (bf16_t*)state, w, bias, nvalid, (bf16_t*)y, C, d, K);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
