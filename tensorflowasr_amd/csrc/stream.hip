// Streaming (chunk-by-chunk) Conformer encoder for gfx950: the kernels that read or write state carried between chunks.
//
// One step processes B streams x at most C encoder frames (C = chunk_size of the streaming config, multihead_attention.py:104-143
// compute_streaming_mask: query chunk c sees keys [c C - hist, c C + C)).  The dense pieces of a block run on the forward kernels of
// training with T = C; what is here:
//   stream_attn_kernel       : the chunk's queries against (key / value ring of the last `hist` frames) ++ (the chunk's own keys)
//   stream_kv_append_kernel  : the chunk's keys / values into the ring (its own launch AFTER the attention: every head of the attention
//                              launch still reads the slots this overwrites - they lie inside the chunk's window)
//   stream_dwconv_kernel     : causal depthwise conv whose left context is a carried [K-1, d] state, updated in place: with the GLU in
//                              front (Conformer) or as DeepSpeech2's RowConv1D with the folded BatchNorm affine and the ReLU behind
// and for the streaming Transformer encoder (plain attention over absolute positions, no convolution module):
//   stream_attn_plain_kernel : the same chunk attention without the relative-position term, keys and values staged in LDS block by
//                              block (every ring or chunk row leaves global memory once per workgroup), optional causal mask inside the
//                              chunk, and the ring append in the SAME launch: a workgroup is the only reader and the only writer of its
//                              head's column slice of the rings, and it writes them only after its last ring read and a barrier
//   stream_add_pe_kernel     : x + pe[seen[b] + r] for the valid rows: the absolute position table at each stream's own offset
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

// Causal depthwise conv of one step over a carried [K-1, d] state, updated in place: ONE kernel for the Conformer's convolution module
// and for DeepSpeech2's RowConv1D, which differ only in how a row enters (Op::load) and in what is done with a tap sum (Op::init /
// Op::finish).  grid (ceil(d / 64), B), 256 threads = 64 channels x 4 row phases.  The K-1 state rows and the chunk's valid rows go to
// LDS first; outputs and the new state are computed from LDS only, so the state is updated in place; an idle stream returns before any
// barrier and nothing of its state is written.
//   GluBias   : a row is the GLU of a [2d] row (rounded to the storage type, as the offline GLU's output tensor is); sum from the bias
//   RowAffine : (encoders/deepspeech2.py:56-60: causal DepthwiseConv1D without bias -> BatchNormalization -> ReLU) a row as it lies; the
//               sum from 0, rounded to the storage type (the intermediate tensor of the offline pair tfasr_dwconv_fwd ->
//               tfasr_channel_affine_fwd), then a multiply and an add that stay TWO roundings (channel_affine_kernel's are: the empty
//               asm keeps the compiler from contracting them here), then the ReLU - the offline pair bit for bit
template <typename T> struct GluBias {
  const float* bias;
  static constexpr int IN = 2;  // input row width in units of d
  __device__ __forceinline__ float load(const T* row, int c, int d) const { return round_as<T>(Num<T>::ld(row + c) * sigmoidf_(Num<T>::ld(row + d + c))); }
  __device__ __forceinline__ float init(int c) const { return bias ? bias[c] : 0.f; }
  __device__ __forceinline__ float finish(float acc, int) const { return acc; }
};
template <typename T> struct RowAffine {
  const float *scale, *shift;
  static constexpr int IN = 1;
  __device__ __forceinline__ float load(const T* row, int c, int) const { return Num<T>::ld(row + c); }
  __device__ __forceinline__ float init(int) const { return 0.f; }
  __device__ __forceinline__ float finish(float acc, int c) const {
    float v = round_as<T>(acc) * scale[c];
    asm volatile("" : "+v"(v));
    v += shift[c];
    return fmaxf(v, 0.f);
  }
};

template <typename T, typename Op>
__global__ __launch_bounds__(256) void stream_dwconv_kernel(const T* __restrict__ a, T* __restrict__ state, const float* __restrict__ w, const Op op,
                                                            const int32_t* __restrict__ nvalid, T* __restrict__ y, int C, int d, int K) {
  __shared__ float g[(32 - 1 + MAXC) * 64];
  const int b = blockIdx.y, cl = threadIdx.x & 63, ph = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const int nv = min(max(nvalid[b], 0), C), K1 = K - 1;
  if (c < d)
    for (int r = nv + ph; r < C; r += 4) Num<T>::st(y + ((long)b * C + r) * d + c, 0.f);
  if (nv == 0) return;
  if (c < d) {
    for (int r = ph; r < K1; r += 4) g[r * 64 + cl] = Num<T>::ld(state + ((long)b * K1 + r) * d + c);
    for (int r = ph; r < nv; r += 4) g[(K1 + r) * 64 + cl] = op.load(a + ((long)b * C + r) * Op::IN * d, c, d);
  }
  __syncthreads();
  if (c >= d) return;
  for (int r = ph; r < nv; r += 4) {
    float acc = op.init(c);
    for (int k = 0; k < K; ++k) acc = fmaf(g[(r + k) * 64 + cl], w[k * d + c], acc);
    Num<T>::st(y + ((long)b * C + r) * d + c, op.finish(acc, c));
  }
  for (int r = ph; r < K1; r += 4) Num<T>::st(state + ((long)b * K1 + r) * d + c, g[(nv + r) * 64 + cl]);
}

// ------------------------------------------------------------------------------------------- plain chunk attention + ring append
constexpr int PKB = 32;           // keys per LDS block (>= MAXC: the chunk's own rows are one block, the LAST one)
constexpr int PLDK = MAXDH + 4;   // widest key row in LDS: + one 16-byte access, so that lanes reading consecutive rows hit different banks
constexpr int PROWS = 16;         // output rows per thread at most: 256 / dh >= 2 row groups, MAXC = 32 rows
static_assert(PKB == 32 && MAXC <= PKB && MAXC <= 2 * PROWS, "stream_attn_plain_kernel's blocking: a half-wave of keys per block");

template <bool VEC> __device__ __forceinline__ float dot_lds(const float* __restrict__ q, const float* __restrict__ k, int dh) {
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f;  // four chains: the products of one row are 128 dependent FMAs otherwise
  if (VEC) {
    for (int e = 0; e < dh; e += 8) {
      const float4 q0 = *reinterpret_cast<const float4*>(q + e), q1 = *reinterpret_cast<const float4*>(q + e + 4);
      const float4 k0 = *reinterpret_cast<const float4*>(k + e), k1 = *reinterpret_cast<const float4*>(k + e + 4);
      a = fmaf(q0.x, k0.x, a); b = fmaf(q0.y, k0.y, b); c = fmaf(q0.z, k0.z, c); d = fmaf(q0.w, k0.w, d);
      a = fmaf(q1.x, k1.x, a); b = fmaf(q1.y, k1.y, b); c = fmaf(q1.z, k1.z, c); d = fmaf(q1.w, k1.w, d);
    }
  } else {
    for (int e = 0; e < dh; ++e) a = fmaf(q[e], k[e], a);
  }
  return (a + b) + (c + d);
}

// all-reduce over the 32 lanes of a half-wave in the vector unit alone (DPP row rotations, then one permlane16 swap for lane ^ 16):
// wave_max / wave_sum go through ds_bpermute, an LDS round trip per step in a dependent chain
__device__ __forceinline__ float half_max(float v) { return xor16_max(row16_max(v)); }
__device__ __forceinline__ float half_sum(float v) { return xor16_sum(row16_sum(v)); }

// grid (H, B), 256 threads.  Keys in time order: nh = min(seen, hist) ring frames (slot (seen - nh + jj) % hist), then the chunk's own
// rows; they are walked in blocks of PKB with a running max / sum per query row (Ms / Ls) and the output rows in registers: thread t
// owns column t % dh of rows t / dh + k * (256 / dh).  The own rows are the last block, so after the loop they still stand in LDS
// (f32 copies of storage-type values: the conversion back is exact) and go from there into the ring.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void stream_attn_plain_kernel(const T* __restrict__ qkv, T* kc, T* vc, const int32_t* __restrict__ seen,
                                                                const int32_t* __restrict__ nvalid, T* __restrict__ out, int C, int H, int dh,
                                                                int hist, float scale, int causal) {
  __shared__ __attribute__((aligned(16))) float Qs[MAXC * MAXDH];
  __shared__ __attribute__((aligned(16))) float Ks[PKB * PLDK];
  __shared__ __attribute__((aligned(16))) float Vs[PKB * MAXDH];
  __shared__ __attribute__((aligned(16))) float Ps[MAXC * PKB];
  __shared__ float Ms[MAXC], Ls[MAXC], As[MAXC];
  const int h = blockIdx.x, b = blockIdx.y, HD = H * dh, t = threadIdx.x;
  const int nv = min(max(nvalid[b], 0), C), sn = max(seen[b], 0);
  T* ob = out + (long)b * C * HD + h * dh;
  for (int i = nv * dh + t; i < C * dh; i += 256) Num<T>::st(ob + (long)(i / dh) * HD + i % dh, 0.f);
  if (nv == 0) return;  // an idle stream: before any barrier, and nothing of its rings is written
  const int nh = min(sn, hist), ldk = dh + (VEC ? 4 : 1);
  const T* qb = qkv + (long)b * C * 3 * HD + h * dh;
  T* kcb = kc + (long)b * hist * HD + h * dh;
  T* vcb = vc + (long)b * hist * HD + h * dh;
  const int G = 256 / dh, e = t % dh, g = t / dh, nkr = (nv + G - 1) / G;  // rows g + k G, k < nkr, of column e
  const bool owner = g < G;
  float acc[PROWS];
#pragma unroll
  for (int k = 0; k < PROWS; ++k) acc[k] = 0.f;
  for (int i = t; i < nv * dh; i += 256) Qs[i] = Num<T>::ld(qb + (long)(i / dh) * 3 * HD + i % dh) * scale;
  if (t < nv) { Ms[t] = -INFINITY; Ls[t] = 0.f; }
  const int nring = (nh + PKB - 1) / PKB;
  for (int blk = 0; blk <= nring; ++blk) {
    const bool own = blk == nring;
    const int j0 = blk * PKB, kbn = own ? nv : min(PKB, nh - j0), kb4 = (kbn + 3) & ~3;
    if (blk) __syncthreads();  // the previous block's K / V / P are read no more
    // ---- K and V rows of the block into LDS as f32; rows kbn .. kb4 - 1 zero (the P V loop walks keys four at a time)
    if (VEC) {
      const int c8 = dh >> 3;
      for (int i = t; i < kb4 * c8; i += 256) {
        const int row = i / c8, c = (i % c8) * 8;
        float kk[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (row < kbn) {
          if (own) {
            ld8(qb + (long)row * 3 * HD + HD + c, kk);
            ld8(qb + (long)row * 3 * HD + 2 * HD + c, vv);
          } else {
            const long slot = (sn - nh + j0 + row) % hist;
            ld8(kcb + slot * HD + c, kk);
            ld8(vcb + slot * HD + c, vv);
          }
        }
        *reinterpret_cast<float4*>(Ks + row * ldk + c) = make_float4(kk[0], kk[1], kk[2], kk[3]);
        *reinterpret_cast<float4*>(Ks + row * ldk + c + 4) = make_float4(kk[4], kk[5], kk[6], kk[7]);
        *reinterpret_cast<float4*>(Vs + row * dh + c) = make_float4(vv[0], vv[1], vv[2], vv[3]);
        *reinterpret_cast<float4*>(Vs + row * dh + c + 4) = make_float4(vv[4], vv[5], vv[6], vv[7]);
      }
    } else {
      for (int i = t; i < kb4 * dh; i += 256) {
        const int row = i / dh, c = i % dh;
        float kk = 0.f, vv = 0.f;
        if (row < kbn) {
          if (own) {
            kk = Num<T>::ld(qb + (long)row * 3 * HD + HD + c);
            vv = Num<T>::ld(qb + (long)row * 3 * HD + 2 * HD + c);
          } else {
            const long slot = (sn - nh + j0 + row) % hist;
            kk = Num<T>::ld(kcb + slot * HD + c);
            vv = Num<T>::ld(vcb + slot * HD + c);
          }
        }
        Ks[row * ldk + c] = kk;
        Vs[row * dh + c] = vv;
      }
    }
    __syncthreads();
    // ---- scores and the running max / sum: a half-wave per query row (8 rows per pass), one key per lane, the score never leaves its
    // register.  With the causal flag own key j is hidden from the rows before it.  As = what the row's earlier blocks are scaled by
    for (int r0 = 0; r0 < nv; r0 += 8) {
      const int r = r0 + (t >> 5), j = t & 31;  // r <= 31 = MAXC - 1
      const bool row = r < nv, live = row && j < kbn && !(own && causal && j > r);
      const float s = live ? dot_lds<VEC>(Qs + r * dh, Ks + j * ldk, dh) : -INFINITY;
      const float mo = row ? Ms[r] : 0.f;
      const float mn = fmaxf(mo, half_max(s));  // finite from the first block on: a row sees every ring key and its own
      const float p = live ? expf(s - mn) : 0.f;
      const float sum = half_sum(p);
      if (row) {
        Ps[r * PKB + j] = p;  // (keys kbn .. 31: zero)
        if (j == 0) {
          const float a = expf(mo - mn);
          As[r] = a;
          Ls[r] = Ls[r] * a + sum;
          Ms[r] = mn;
        }
      }
    }
    __syncthreads();
    // ---- P V: one value read per key serves all rows of the thread
    if (owner) {
      int rc[PROWS];
#pragma unroll
      for (int k = 0; k < PROWS; ++k) {
        rc[k] = min(g + k * G, nv - 1);  // (a row past nv computes row nv - 1 again and is dropped at the end)
        if (k < nkr) acc[k] *= As[rc[k]];
      }
      for (int j = 0; j < kb4; j += 4) {
        const float v0 = Vs[j * dh + e], v1 = Vs[(j + 1) * dh + e], v2 = Vs[(j + 2) * dh + e], v3 = Vs[(j + 3) * dh + e];
#pragma unroll
        for (int k = 0; k < PROWS; ++k) {
          if (k < nkr) {
            const float4 p = *reinterpret_cast<const float4*>(Ps + rc[k] * PKB + j);
            acc[k] = fmaf(p.w, v3, fmaf(p.z, v2, fmaf(p.y, v1, fmaf(p.x, v0, acc[k]))));
          }
        }
      }
    }
  }
  if (owner) {
#pragma unroll
    for (int k = 0; k < PROWS; ++k) {
      const int r = g + k * G;
      if (k < nkr && r < nv) Num<T>::st(ob + (long)r * HD + e, acc[k] / Ls[r]);
    }
  }
  // ---- ring append from LDS (the own block's K / V): every ring read of this workgroup lies before the barriers above.  With more valid
  // rows than slots only the last `hist` rows go (no two rows share a slot)
  for (int i = max(0, nv - hist) * dh + t; i < nv * dh && hist > 0; i += 256) {
    const int r = i / dh, c = i % dh;
    const long dst = (long)((sn + r) % hist) * HD + c;
    Num<T>::st(kcb + dst, Ks[r * ldk + c]);
    Num<T>::st(vcb + dst, Vs[r * dh + c]);
  }
}

// grid flat over B * C * d (8 elements per thread when VEC): y = x + pe[seen[b] + r] for r < nvalid[b] in f32, one rounding; the other
// rows are copied; a position outside [0, Tcap) is never read and gives NaN
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void stream_add_pe_kernel(const T* __restrict__ x, const float* __restrict__ pe, const int32_t* __restrict__ seen,
                                                            const int32_t* __restrict__ nvalid, T* __restrict__ y, int B, int C, int d, int Tcap) {
  constexpr int W = VEC ? 8 : 1;
  const int dw = d / W;
  const long n = (long)B * C * dw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % dw) * W;
    const long row = i / dw;
    const int r = (int)(row % C), b = (int)(row / C);
    const bool valid = r < nvalid[b];
    const long pos = (long)seen[b] + r;
    const bool inside = pos >= 0 && pos < Tcap;
    if (VEC) {
      float v[8];
      ld8(x + row * d + c, v);
      if (valid && inside) {
        float p[8];
        ld8(pe + pos * d + c, p);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += p[k];
      } else if (valid) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = NAN;
      }
      st8(y + row * d + c, v);
    } else {
      float v = Num<T>::ld(x + row * d + c);
      if (valid) v = inside ? v + pe[pos * d + c] : NAN;
      Num<T>::st(y + row * d + c, v);
    }
  }
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
    TFASR_KLAUNCH((stream_dwconv_kernel<float, GluBias<float>>), grid, dim3(256), 0, s, (const float*)glu_x, (float*)state, w, GluBias<float>{bias},
                  nvalid, (float*)y, C, d, K);
  else
    TFASR_KLAUNCH((stream_dwconv_kernel<bf16_t, GluBias<bf16_t>>), grid, dim3(256), 0, s, (const bf16_t*)glu_x, (bf16_t*)state, w,
                  GluBias<bf16_t>{bias}, nvalid, (bf16_t*)y, C, d, K);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_stream_rowconv_fwd(const void* x, void* state, const float* w, const float* scale, const float* shift, const int32_t* nvalid,
                                        void* y, int B, int C, int d, int K, int dtype, void* stream_) {
  if (!x || !w || !scale || !shift || !nvalid || !y || B <= 0 || C <= 0 || d <= 0 || K <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (K > 1 && !state) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (C > MAXC || K > 32 || B > 65535) return TFASR_STATUS_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((d + 63) / 64, B);
  if (dtype == TFASR_F32)
    TFASR_KLAUNCH((stream_dwconv_kernel<float, RowAffine<float>>), grid, dim3(256), 0, s, (const float*)x, (float*)state, w,
                  RowAffine<float>{scale, shift}, nvalid, (float*)y, C, d, K);
  else
    TFASR_KLAUNCH((stream_dwconv_kernel<bf16_t, RowAffine<bf16_t>>), grid, dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)state, w,
                  RowAffine<bf16_t>{scale, shift}, nvalid, (bf16_t*)y, C, d, K);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_stream_attn_plain_fwd(const void* qkv, void* kcache, void* vcache, const int32_t* seen, const int32_t* nvalid, void* out,
                                           int B, int C, int H, int dh, int hist, float scale, int causal, int dtype, void* stream_) {
  if (!qkv || !seen || !nvalid || !out || B <= 0 || C <= 0 || H <= 0 || dh <= 0 || hist < 0) return TFASR_STATUS_INVALID_VALUE;
  if (hist > 0 && (!kcache || !vcache)) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (C > MAXC || (long)hist + C > MAXK || dh > MAXDH || B > 65535) return TFASR_STATUS_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream_;
  const bool vec = (dh % 8 == 0) && ((((uintptr_t)qkv | (uintptr_t)kcache | (uintptr_t)vcache) & 15) == 0);
#define TFASR_SP(TT, VV) TFASR_KLAUNCH((stream_attn_plain_kernel<TT, VV>), dim3(H, B), dim3(256), 0, s, (const TT*)qkv, (TT*)kcache, (TT*)vcache, \
                                       seen, nvalid, (TT*)out, C, H, dh, hist, scale, causal != 0)
  if (dtype == TFASR_F32) { if (vec) TFASR_SP(float, true); else TFASR_SP(float, false); }
  else { if (vec) TFASR_SP(bf16_t, true); else TFASR_SP(bf16_t, false); }
#undef TFASR_SP
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_stream_add_pe(const void* x, const float* pe, const int32_t* seen, const int32_t* nvalid, void* y, int B, int C, int d,
                                   int Tcap, int dtype, void* stream_) {
  if (!x || !pe || !seen || !nvalid || !y || B <= 0 || C <= 0 || d <= 0 || Tcap <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  const bool vec = (d % 8 == 0) && ((((uintptr_t)x | (uintptr_t)pe | (uintptr_t)y) & 15) == 0);
  const long n = (long)B * C * (vec ? d / 8 : d);
  const dim3 grid((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096));
#define TFASR_PE(TT, VV) TFASR_KLAUNCH((stream_add_pe_kernel<TT, VV>), grid, dim3(256), 0, s, (const TT*)x, pe, seen, nvalid, (TT*)y, B, C, d, Tcap)
  if (dtype == TFASR_F32) { if (vec) TFASR_PE(float, true); else TFASR_PE(float, false); }
  else { if (vec) TFASR_PE(bf16_t, true); else TFASR_PE(bf16_t, false); }
#undef TFASR_PE
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
