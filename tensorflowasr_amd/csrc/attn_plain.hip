// Fused plain (absolute-position) scaled dot-product attention, forward, for gfx950: the attention of the Transformer encoder
// (keras MultiHeadAttention as tensorflow_asr/models/layers/multihead_attention.py:216-423 configures it, `encoder_mha_type: mha`).
//
//   out[b,i,h,:] = softmax_j( masked_fill(scale * q_i.k_j, mask[b,i,j], -1e9) ) @ v        (general.py:25-41)
//   mask[b,i,j]  = (i < len_b) AND causal(i,j) AND window(i,j)                               (multihead_attention.py:146-213, 331-345)
// Only the QUERY carries a length mask (the layer strips the key / value masks, :368-373).  A masked score is REPLACED by -1e9, so
//   * a valid query row gives its masked keys exactly zero probability in f32 (it always sees itself, so its maximum is a real score);
//   * a padded query row (i >= len_b) has every score replaced: it attends uniformly over ALL T keys, whatever the causal or streaming
//     mask says.  Those rows are not dead - their keys and values feed the valid rows of the next layer - so they are computed, and key
//     blocks outside the windows of a query block are only skipped when no row of the block is padded.
// qkv [B*T, 3*H*dh] (q|k|v column blocks, the layout tfasr_relattn_fused_fwd reads), out [B*T, H*dh]; nothing of size T x T touches HBM.
// lse[b,h,i] = log sum_j exp(s_ij) over the visible keys; for a padded row the constant score is dropped: log T (as tfasr_relattn_fused_fwd).
//
// bf16 kernel (dh = 64 | 128).  The structure is relattn_fused_fwdT_kernel's (attn_fused.hip) without the position window: per
// (b, h, 64-query block) a 4-wave workgroup streams 64-key blocks of K and V through LDS (global_load_lds, 16-byte chunks XOR-swizzled by
// row so the fragment reads are free of bank conflicts), each wave owning 16 query rows.  The scores are computed TRANSPOSED,
// S^T = K Q^T with v_mfma_f32_16x16x32_bf16, so that in the C layout a lane owns ONE query row: the online-softmax state is a per-lane
// scalar, the row reductions are in-lane plus two permlane swaps, and P^T in C layout IS the B operand of O^T += V^T P^T (the key rows
// are dealt to the MFMA tiles so that a lane's eight probabilities of a 32-key group are eight consecutive keys; V^T fragments come from
// ds_read_b64_tr_b16).  A 256-byte row (dh = 128) is held as two 64-column images of 128-byte rows, so the loaders, the swizzle keys
// and the fragment readers are those of the 128-byte-row images of attn_fused.hip (restated here: that file's are file-local).
//
// Query block = 64 rows, not 128 or the 256 of an MFMA-bound prefill kernel: at the shipped configuration on 32 x 10 s (B H = 128,
// T' = 250) one layer is ~4 GFLOP - bound by launch and by not writing scores, not by the matrix cores.  64 rows give 4 x 128 = 512
// workgroups for the 256 CUs, at least two resident per CU (16 / 32 KB of LDS, 92 - 138 registers) so one's loads hide under the other's products;
// 128 rows would give exactly 256 workgroups of which every second one is the ragged 122-row tail, and one workgroup per CU with nothing to
// overlap its (unpipelined) loads with.  No inter-workgroup communication, no persistent loop.
//
// f32 twin (any dh % 16 == 0, dh <= 128): a plain FMA kernel (32 queries x 32 keys per step, scores and probabilities through LDS) for the
// token-exact decoding mode; same semantics, expf / f32 accumulation.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) short short4_t;

namespace {

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

constexpr int BI = 64, BJ = 64, IMG_BYTES = 64 * 128;  // one [64 rows][64 bf16] image
// chunk swizzle keys of the 128-byte-row images (attn_fused.hip: key_d for images read by rows, key_t64 for the transposed reads)
__device__ __forceinline__ int key_d(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }
__device__ __forceinline__ int key_t64(int k) { return (((k >> 1) & 1) | (((k >> 3) & 1) << 1)) << 1; }

// [64 rows][64] bf16 image of global rows row0 .. row0 + 63 (clamped to nrows - 1), columns g[0..63]; 4 waves, 2 pieces of 8 rows each
template <bool TRANS>
__device__ __forceinline__ void load_img(char* s, const bf16_t* g, long ld, int row0, int nrows, int w, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = w * 2 + i;
    const int row = q * 8 + (lane >> 3), p = lane & 7;
    const int gr = min(row0 + row, nrows - 1);
    const bf16_t* src = g + (long)gr * ld + ((p ^ (TRANS ? key_t64(row) : key_d(row))) << 3);
    __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(s + __builtin_amdgcn_readfirstlane(q * 1024)), 16, 0, 0);
  }
}
__device__ __forceinline__ short8_t frag_rows(const char* s, int row, int c) {
  return *reinterpret_cast<const short8_t*>(s + row * 128 + ((c ^ key_d(row)) << 4));
}
// A fragment of V^T: rows n = nbase + (lane & 15), k = keys kbase .. kbase + 7 (kbase already holds the lane group's 8 g)
__device__ __forceinline__ short8_t frag_v(const char* s, int nbase, int kbase, int r) {
  const int col = nbase + ((r & 3) << 2);
  const int chunk = col >> 3, half = (col >> 2) & 1;
  const int k0 = kbase + (r >> 2), k1 = k0 + 4;
  const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4_t*)(s + k0 * 128 + ((chunk ^ key_t64(k0)) << 4) + half * 8));
  const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4_t*)(s + k1 * 128 + ((chunk ^ key_t64(k1)) << 4) + half * 8));
  short8_t v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return v;
}

// visible keys [lo, hi) of VALID query row i: the streaming window (compute_streaming_mask) ANDed with the lower triangle
__device__ __forceinline__ void visible(int i, int T, int causal, int chunk, int hist, int& lo, int& hi) {
  lo = 0; hi = T;
  if (chunk > 0) {
    const int index = (i / chunk) * chunk;
    lo = hist < 0 ? 0 : max(0, index - hist);
    hi = min(T, index + chunk);
  }
  if (causal) hi = min(hi, i + 1);
}
// key blocks [jb_lo, jb_hi) (of `bj` keys) that some row of the query block i0 .. i0 + bi - 1 sees; every block when a row of it is padded
__device__ __forceinline__ void block_range(int i0, int bi, int bj, int T, int len, int use_mask, int causal, int chunk, int hist, int& jb_lo,
                                            int& jb_hi) {
  jb_lo = 0; jb_hi = (T + bj - 1) / bj;
  if ((causal || chunk > 0) && !(use_mask && i0 + bi > len)) {
    int lo, hi, lo2, hi2;
    visible(i0, T, causal, chunk, hist, lo, hi);
    visible(min(i0 + bi - 1, T - 1), T, causal, chunk, hist, lo2, hi2);  // lo and hi are non-decreasing in i
    jb_lo = lo / bj;
    jb_hi = (hi2 + bj - 1) / bj;
  }
}

template <int DHT, bool WINDOWED>
__global__ __launch_bounds__(256, 2) void attn_plain_bf16_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lengths,
                                                                 bf16_t* __restrict__ out, float* __restrict__ lse_out, int B, int H, int T,
                                                                 float scale, int use_mask, int causal, int chunk, int hist) {
  constexpr int NI = DHT / 64;   // 64-column images per K / V block
  constexpr int NKK = DHT / 32;  // k steps of the score product
  constexpr int NO = DHT / 16;   // 16-row tiles of O^T
  __shared__ __attribute__((aligned(1024))) char smem[2 * NI * IMG_BYTES];
  char* sK = smem;
  char* sV = smem + NI * IMG_BYTES;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * BI;
  const int HD = H * DHT, LDQ = 3 * HD;
  const int len = (use_mask && lengths) ? max(0, min(lengths[b], T)) : T;
  const bf16_t* qb = qkv + (long)b * T * LDQ + h * DHT;
  const bf16_t* kb = qb + HD;
  const bf16_t* vb = qb + 2 * HD;

  // this lane's query row = the B operand column
  const int i = i0 + w * 16 + r, irow = min(i, T - 1);
  short8_t bq[NKK];
#pragma unroll
  for (int kk = 0; kk < NKK; ++kk) bq[kk] = *reinterpret_cast<const short8_t*>(qb + (long)irow * LDQ + kk * 32 + g * 8);
  float m_run = -INFINITY, l_run = 0.f;
  float4_t acc_o[NO];  // O^T: rows = head dims n * 16 + g * 4 + e, column = this lane's query
#pragma unroll
  for (int n = 0; n < NO; ++n) acc_o[n] = float4_t{0.f, 0.f, 0.f, 0.f};

  const bool qm = i >= len;  // padded query row: constant scores over all T keys
  int klo = 0, khi = T;
  if (WINDOWED && !qm) visible(irow, T, causal, chunk, hist, klo, khi);
  const float scale2 = scale * 1.4426950408889634f;
  int jl0[4], krow[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    jl0[jt] = 32 * (jt >> 1) + g * 8 + (jt & 1) * 4;                    // first of this lane's four keys of tile jt (C rows g * 4 + e)
    krow[jt] = 32 * (jt >> 1) + (r >> 2) * 8 + (jt & 1) * 4 + (r & 3);  // key row that is MFMA row r of tile jt (A operand)
  }
  int jb_lo, jb_hi;
  block_range(i0, BI, BJ, T, len, use_mask, WINDOWED ? causal : 0, WINDOWED ? chunk : 0, hist, jb_lo, jb_hi);

  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    const int j0 = jb * BJ;
#pragma unroll
    for (int s = 0; s < NI; ++s) {
      load_img<false>(sK + s * IMG_BYTES, kb + s * 64, LDQ, j0, T, w, lane);
      load_img<true>(sV + s * IMG_BYTES, vb + s * 64, LDQ, j0, T, w, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // scores, transposed: tile jt = 16 keys x this wave's 16 queries
    float4_t acc_s[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      acc_s[jt] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk)
        acc_s[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(sK + (kk >> 1) * IMG_BYTES, krow[jt], (kk & 1) * 4 + g), bq[kk],
                                                            acc_s[jt], 0, 0, 0);
      if (qm) acc_s[jt] = float4_t{0.f, 0.f, 0.f, 0.f};
    }
    // keys outside [klo, khi): past the end of a ragged last block (the image rows are clamped copies), outside the window / triangle
    const bool edge = WINDOWED || j0 + BJ > T;
    float mx = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + jl0[jt] + e;
        mx = fmaxf(mx, (edge && (j < klo || j >= khi)) ? -INFINITY : acc_s[jt][e]);
      }
    mx = xor32_max(xor16_max(mx));
    // (the softmax scale is positive: the maximum commutes with it, and the exponent is one fused multiply-add per element)
    const float m_new = fmaxf(m_run, mx == -INFINITY ? -INFINITY : mx * scale2);
    const float m_ref = m_new == -INFINITY ? 0.f : m_new;  // no visible key so far: every probability below is set to zero
    const float corr = __builtin_amdgcn_exp2f(m_run - m_ref);
    float rs = 0.f;
    short8_t pf[2];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      float p[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + jl0[jt] + e;
        p[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(acc_s[jt][e], scale2, -m_ref));
        if (edge && (j < klo || j >= khi)) p[e] = 0.f;
      }
      rs += (p[0] + p[1]) + (p[2] + p[3]);
      const uint32_t lo = pack2_bf16(p[0], p[1]), hi = pack2_bf16(p[2], p[3]);
      const int o = (jt & 1) * 4;
      pf[jt >> 1][o + 0] = (short)(lo & 0xffffu); pf[jt >> 1][o + 1] = (short)(lo >> 16);
      pf[jt >> 1][o + 2] = (short)(hi & 0xffffu); pf[jt >> 1][o + 3] = (short)(hi >> 16);
    }
    rs = xor32_sum(xor16_sum(rs));
    l_run = l_run * corr + rs;
    m_run = m_new;
    // O^T = O^T * corr + V^T P^T: the probabilities are the B operand straight from registers
#pragma unroll
    for (int n = 0; n < NO; ++n) {
      acc_o[n] *= corr;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_v(sV + (n >> 2) * IMG_BYTES, (n & 3) * 16, q * 32 + g * 8, r), pf[q], acc_o[n],
                                                            0, 0, 0);
    }
    __syncthreads();  // every wave is done with this block's images
  }

  if (i < T) {
    const float inv = 1.f / l_run;
#pragma unroll
    for (int n = 0; n < NO; ++n) {
      uint2 v;
      v.x = pack2_bf16(acc_o[n][0] * inv, acc_o[n][1] * inv);
      v.y = pack2_bf16(acc_o[n][2] * inv, acc_o[n][3] * inv);
      *reinterpret_cast<uint2*>(out + ((long)b * T + i) * HD + h * DHT + n * 16 + g * 4) = v;
    }
    if (lse_out && g == 0) lse_out[((long)b * H + h) * T + i] = m_run * 0.6931471805599453f + logf(l_run);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// f32 twin: 32 queries x 32 keys per step, 256 threads.  Scores: thread (ty, tx) = (tid / 16, tid % 16) owns rows 2 ty + {0, 1}, keys
// 2 tx + {0, 1}; softmax: 8 threads per row, 4 keys each, the running maximum / sum replicated in the 8; P V: rows 2 ty + {0, 1},
// columns tx + 16 c.  Row strides dh + 1 / 33 floats keep the column walks on distinct banks.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int FI = 32, FJ = 32;

__global__ __launch_bounds__(256) void attn_plain_f32_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ lengths,
                                                             float* __restrict__ out, float* __restrict__ lse_out, int B, int H, int T, int dh,
                                                             float scale, int use_mask, int causal, int chunk, int hist) {
  extern __shared__ __attribute__((aligned(16))) char smem_f[];
  const int ldq = dh + 1;
  float* sQ = reinterpret_cast<float*>(smem_f);  // [32][dh + 1]
  float* sK = sQ + FI * ldq;                     // [32][dh + 1]
  float* sV = sK + FJ * ldq;                     // [32][dh]
  float* sS = sV + FJ * dh;                      // [32][33]
  float* sC = sS + FI * 33;                      // [32] rescale factor of the step, then 1 / l
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * FI;
  const int HD = H * dh, LDQ = 3 * HD, nc = dh >> 4;
  const int len = (use_mask && lengths) ? max(0, min(lengths[b], T)) : T;
  const float* qb = qkv + (long)b * T * LDQ + h * dh;
  const float* kb = qb + HD;
  const float* vb = qb + 2 * HD;
  for (int idx = tid; idx < FI * dh; idx += 256) {
    const int rr = idx / dh, c = idx - rr * dh;
    sQ[rr * ldq + c] = qb[(long)min(i0 + rr, T - 1) * LDQ + c] * scale;  // the reference scales the query first (keras _compute_attention)
  }
  // softmax role: row srow, keys 4 part .. 4 part + 3 of the step
  const int srow = tid >> 3, part = tid & 7;
  const int si = i0 + srow;
  const bool qm = si >= len;
  int klo = 0, khi = T;
  if (!qm) visible(min(si, T - 1), T, causal, chunk, hist, klo, khi);
  float m_run = -INFINITY, l_run = 0.f;
  float acc[2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[a][c] = 0.f;
  int jb_lo, jb_hi;
  block_range(i0, FI, FJ, T, len, use_mask, causal, chunk, hist, jb_lo, jb_hi);

  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    const int j0 = jb * FJ;
    __syncthreads();  // the last step's K, V and probabilities are dead (and Q is written, the first time)
    for (int idx = tid; idx < FJ * dh; idx += 256) {
      const int rr = idx / dh, c = idx - rr * dh;
      const long grow = (long)min(j0 + rr, T - 1) * LDQ + c;
      sK[rr * ldq + c] = kb[grow];
      sV[rr * dh + c] = vb[grow];
    }
    __syncthreads();
    {
      float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
      const float* q0 = sQ + (2 * ty) * ldq;
      const float* q1 = q0 + ldq;
      const float* k0 = sK + (2 * tx) * ldq;
      const float* k1 = k0 + ldq;
      for (int k = 0; k < dh; ++k) {
        const float a0 = q0[k], a1 = q1[k], b0 = k0[k], b1 = k1[k];
        s00 = fmaf(a0, b0, s00); s01 = fmaf(a0, b1, s01);
        s10 = fmaf(a1, b0, s10); s11 = fmaf(a1, b1, s11);
      }
      sS[(2 * ty) * 33 + 2 * tx] = s00; sS[(2 * ty) * 33 + 2 * tx + 1] = s01;
      sS[(2 * ty + 1) * 33 + 2 * tx] = s10; sS[(2 * ty + 1) * 33 + 2 * tx + 1] = s11;
    }
    __syncthreads();
    {
      float s[4];
      bool vis[4];
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + part * 4 + e;
        vis[e] = j >= klo && j < khi;
        s[e] = qm ? 0.f : sS[srow * 33 + part * 4 + e];
        if (vis[e]) mx = fmaxf(mx, s[e]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
      const float m_new = fmaxf(m_run, mx);
      const float m_ref = m_new == -INFINITY ? 0.f : m_new;
      const float corr = expf(m_run - m_ref);
      float rs = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = vis[e] ? expf(s[e] - m_ref) : 0.f;
        sS[srow * 33 + part * 4 + e] = p;
        rs += p;
      }
      rs += __shfl_xor(rs, 4, 64);
      rs += __shfl_xor(rs, 2, 64);
      rs += __shfl_xor(rs, 1, 64);
      l_run = l_run * corr + rs;
      m_run = m_new;
      if (part == 0) sC[srow] = corr;
    }
    __syncthreads();
    {
      const float c0 = sC[2 * ty], c1 = sC[2 * ty + 1];
#pragma unroll
      for (int c = 0; c < 8; ++c) { acc[0][c] *= c0; acc[1][c] *= c1; }
      const float* p0 = sS + (2 * ty) * 33;
      const float* p1 = p0 + 33;
      for (int j = 0; j < FJ; ++j) {
        const float a0 = p0[j], a1 = p1[j];
        const float* vr = sV + j * dh + tx;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < nc) {
            const float v = vr[16 * c];
            acc[0][c] = fmaf(a0, v, acc[0][c]);
            acc[1][c] = fmaf(a1, v, acc[1][c]);
          }
      }
    }
  }
  __syncthreads();
  if (part == 0) sC[srow] = 1.f / l_run;
  if (part == 0 && si < T && lse_out) lse_out[((long)b * H + h) * T + si] = m_run + logf(l_run);
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int i = i0 + 2 * ty + a;
    if (i < T) {
      const float inv = sC[2 * ty + a];
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < nc) out[((long)b * T + i) * HD + h * dh + tx + 16 * c] = acc[a][c] * inv;
    }
  }
}

}  // namespace

extern "C" int tfasr_attn_plain_fwd(const void* qkv, const int32_t* lengths, void* out, float* lse, int B, int H, int T, int dh, float scale,
                                    int use_mask, int causal, int chunk, int hist, int dtype, void* stream_) {
  if (!qkv || !out || B <= 0 || H <= 0 || T <= 0 || dh <= 0 || (use_mask && !lengths)) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (B > 65535 || H > 65535) return TFASR_STATUS_UNSUPPORTED;  // gridDim.y / z
  hipStream_t s = (hipStream_t)stream_;
  const int ck = chunk > 0 ? chunk : 0;
  const bool windowed = causal != 0 || ck > 0;
  if (dtype == TFASR_BF16) {
    if (dh != 64 && dh != 128) return TFASR_STATUS_UNSUPPORTED;
    if ((((uintptr_t)qkv | (uintptr_t)out) & 15) != 0) return TFASR_STATUS_INVALID_VALUE;
    const dim3 grid((T + BI - 1) / BI, H, B);
#define ATTN_PLAIN_LAUNCH(D, W)                                                                                                              \
  TFASR_KLAUNCH((attn_plain_bf16_kernel<D, W>), grid, dim3(256), 0, s, (const bf16_t*)qkv, lengths, (bf16_t*)out, lse, B, H, T, scale, use_mask, \
                causal ? 1 : 0, ck, hist)
    if (dh == 64) { if (windowed) ATTN_PLAIN_LAUNCH(64, true); else ATTN_PLAIN_LAUNCH(64, false); }
    else { if (windowed) ATTN_PLAIN_LAUNCH(128, true); else ATTN_PLAIN_LAUNCH(128, false); }
#undef ATTN_PLAIN_LAUNCH
  } else {
    if (dh % 16 != 0 || dh > 128) return TFASR_STATUS_UNSUPPORTED;
    const size_t smem = (size_t)(FI * (dh + 1) + FJ * (dh + 1) + FJ * dh + FI * 33 + FI) * sizeof(float);
    if (smem > 48 * 1024) tfasr_dynamic_lds<attn_plain_f32_kernel>((int)smem);
    const dim3 grid((T + FI - 1) / FI, H, B);
    TFASR_KLAUNCH(attn_plain_f32_kernel, grid, dim3(256), smem, s, (const float*)qkv, lengths, (float*)out, lse, B, H, T, dh, scale, use_mask,
                  causal ? 1 : 0, ck, hist);
  }
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
