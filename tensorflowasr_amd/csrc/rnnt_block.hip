// Tail of one RnnTransducerBlock (encoders/rnnt.py:27-82) in one launch: LayerNormalization over the LSTM's rnn_units, Dense(dmodel), and
// the bookkeeping of the TimeReduction that follows (the tf.pad rows, the reduced lengths, a streaming step's row offset).
//
//   out[b, off_b + t, :] = LN(m(y[b, t, :]); gamma, beta, eps) . W + bias     0 <= t < T,   m(row) = row if t < lengths[b] else 0
//   out[b, r, :]         = 0                                                  off_b + T <= r < Tpad
//   out_lengths[b]       = ceil((off_b + min(lengths[b], T)) / factor)
//
// A masked row is computed from zeros whatever y holds there (the masked LSTM emits zeros, LayerNorm of zeros is beta, so the row is
// beta . W + bias, as in the reference); rows in front of off_b are the caller's (a stream's carried rows) and are not touched; a row that
// would fall at or past Tpad is dropped.
//
// A workgroup owns BM consecutive OUTPUT rows of one stream.  It normalises them into LDS (one wave per row, f32 two-pass statistics
// summed in one fixed order) and runs the product from there over the whole reduction, k ascending: there is no split over k and no
// atomic, one tile shape per type, and a row's dot products never read another row - so the bits of an output row depend on its input row
// and the weights alone, not on T, B, off or the rows that share the launch.
//   bf16: BM 32, 4 waves; mfma_f32_16x16x32_bf16, A fragments (lane l: row l & 15, columns 8 (l >> 4) ..) are one ds_read_b128 from the
//         normalised rows (row pitch P + 8 elements: the 16 rows of a read start 4 dwords apart), B fragments 16 contiguous bytes of the
//         packed weight tfasr_conv1d_pack_weight writes for one tap ([chunk][N rounded up to 64][32] bf16, zero filled), loaded one chunk
//         ahead.  Wave w owns the 16-column tiles w, w + 4, ... (an even share for any N), four at a time for both 16-row halves.
//   f32:  BM 16, a plain FMA kernel (4 x 4 outputs per thread, W [P, N] f32 read through float4) - the token-exact twin, not a fast one.
#include "common.h"

namespace {

constexpr int MAX_P = 2048, MAX_N = 1024, VEC = MAX_P / 512;  // a lane holds VEC groups of 8 elements of a row

template <typename T>
__device__ __forceinline__ void load_row(const T* __restrict__ row, bool live, int P, int lane, float (&v)[VEC][8]) {
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    const int c = q * 512 + lane * 8;
    if (live && c < P) {
      ld8(row + c, v[q]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[q][e] = 0.f;
    }
  }
}

// the sum over the wave in every lane, without the LDS crossbar: rotations inside each row of 16 lanes, then the two row-group swaps
__device__ __forceinline__ float wave_sum_dpp(float v) { return xor32_sum(xor16_sum(row16_sum(v))); }

// (mean, rstd) of the P elements a wave holds; the same instruction sequence for every row
__device__ __forceinline__ void row_stats(const float (&v)[VEC][8], int P, int lane, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < VEC; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[q][e];
  mean = wave_sum_dpp(s) / (float)P;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < VEC; ++q) {
    if (q * 512 + lane * 8 < P) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[q][e] - mean;
        ss = fmaf(d, d, ss);
      }
    }
  }
  rstd = rsqrtf(wave_sum_dpp(ss) / (float)P + eps);
}

struct RowRange {
  int lo, hi, len;  // computed output rows [lo, hi); valid input frames
};

__device__ __forceinline__ RowRange row_range(const int32_t* __restrict__ lengths, const int32_t* __restrict__ off, int32_t* __restrict__ out_len,
                                              int b, int T, int Tpad, int factor) {
  RowRange r;
  r.lo = off ? min(max(off[b], 0), Tpad) : 0;
  r.len = lengths ? min(max(lengths[b], 0), T) : T;
  r.hi = min(r.lo + T, Tpad);
  if (out_len && blockIdx.x == 0 && threadIdx.x == 0) out_len[b] = (r.lo + r.len + factor - 1) / factor;
  return r;
}

// zero the tf.pad rows [hi, Tpad) of this tile; N % 16 == 0, so a row is a whole number of 16-byte stores in either type
template <typename T>
__device__ __forceinline__ void zero_pad_rows(T* __restrict__ out, int b, int r0, int BM, int hi, int Tpad, int N) {
  constexpr int E = 16 / (int)sizeof(T);
  const int per = N / E;
  for (int idx = threadIdx.x; idx < BM * per; idx += 256) {
    const int r = r0 + idx / per;
    if (r >= hi && r < Tpad) *reinterpret_cast<uint4*>(out + ((long)b * Tpad + r) * N + (idx % per) * E) = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ------------------------------------------------------------------------------------------------ bf16 (MFMA)
constexpr int BM = 32, CK = 32, PAD = 8;

__global__ __launch_bounds__(256) void tail_bf16_kernel(const bf16_t* __restrict__ y, long ld_y, const int32_t* __restrict__ lengths,
                                                        const int32_t* __restrict__ off, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const bf16_t* __restrict__ wp,
                                                        const float* __restrict__ bias, bf16_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                        int T, int Tpad, int P, int N, int Np, int factor, float eps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_[];
  bf16_t* rows = reinterpret_cast<bf16_t*>(smem_);
  const int b = blockIdx.y, r0 = blockIdx.x * BM, pitch = P + PAD;
  const RowRange rr = row_range(lengths, off, out_len, b, T, Tpad, factor);
  zero_pad_rows(out, b, r0, BM, rr.hi, Tpad, N);
  if (r0 + BM <= rr.lo || r0 >= rr.hi) return;  // (uniform) nothing to compute in this tile
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    float gm[VEC][8], bt[VEC][8];
    load_row(gamma, true, P, lane, gm);
    load_row(beta, true, P, lane, bt);
    for (int i = 0; i < BM / 4; ++i) {
      const int row = wv * (BM / 4) + i, r = r0 + row, t = r - rr.lo;
      const bool live = r >= rr.lo && r < rr.hi && t < rr.len;
      float v[VEC][8], mean, rstd;
      load_row(y + ((long)b * T + (live ? t : 0)) * ld_y, live, P, lane, v);
      row_stats(v, P, lane, eps, mean, rstd);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const int c = q * 512 + lane * 8;
        if (c < P) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = fmaf((v[q][e] - mean) * rstd, gm[q][e], bt[q][e]);
          st8(rows + row * pitch + c, o);
        }
      }
    }
  }
  __syncthreads();
  const int r16 = lane & 15, g = lane >> 4, nt = N / 16, nch = P / CK;
  const bf16_t* arow = rows + r16 * pitch + g * 8;
  // wave wv owns the 16-column tiles wv, wv + 4, wv + 8, ... (an even share for any N), four of them at a time for both 16-row halves
  for (int q0 = 0; wv + 4 * q0 < nt; q0 += 4) {
    float4_t acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    const bf16_t* wb[4];
    bool on[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tile = wv + 4 * (q0 + j);
      on[j] = tile < nt;  // (wave-uniform)
      wb[j] = wp + ((long)(on[j] ? tile : 0) * 16 + r16) * CK + g * 8;
    }
    short8_t bcur[4], bnxt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bcur[j] = *reinterpret_cast<const short8_t*>(wb[j]);
    for (int ch = 0; ch < nch; ++ch) {
      if (ch + 1 < nch) {  // the next chunk's fragments are in flight while this chunk's MFMAs run
#pragma unroll
        for (int j = 0; j < 4; ++j) bnxt[j] = *reinterpret_cast<const short8_t*>(wb[j] + (long)(ch + 1) * Np * CK);
      }
      short8_t a[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const short8_t*>(arow + i * 16 * pitch + ch * CK);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!on[j]) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bcur[j], acc[i][j], 0, 0, 0);
      }
      if (ch + 1 < nch) {
#pragma unroll
        for (int j = 0; j < 4; ++j) bcur[j] = bnxt[j];
      }
    }
    // C / D map of the 16x16 tile: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!on[j]) continue;
      const int n = (wv + 4 * (q0 + j)) * 16 + r16;
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = r0 + i * 16 + g * 4 + e;
          if (r >= rr.lo && r < rr.hi) out[((long)b * Tpad + r) * N + n] = f32_to_bf16(acc[i][j][e] + bv);
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------ f32 twin (plain FMA)
constexpr int FM = 16;

__global__ __launch_bounds__(256) void tail_f32_kernel(const float* __restrict__ y, long ld_y, const int32_t* __restrict__ lengths,
                                                       const int32_t* __restrict__ off, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int32_t* __restrict__ out_len, int T, int Tpad, int P, int N,
                                                       int factor, float eps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_[];
  float* rows = reinterpret_cast<float*>(smem_);
  const int b = blockIdx.y, r0 = blockIdx.x * FM, pitch = P + 4;  // (pitch % 4 == 0: the rows are written through float4)
  const RowRange rr = row_range(lengths, off, out_len, b, T, Tpad, factor);
  zero_pad_rows(out, b, r0, FM, rr.hi, Tpad, N);
  if (r0 + FM <= rr.lo || r0 >= rr.hi) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    float gm[VEC][8], bt[VEC][8];
    load_row(gamma, true, P, lane, gm);
    load_row(beta, true, P, lane, bt);
    for (int i = 0; i < FM / 4; ++i) {
      const int row = wv * (FM / 4) + i, r = r0 + row, t = r - rr.lo;
      const bool live = r >= rr.lo && r < rr.hi && t < rr.len;
      float v[VEC][8], mean, rstd;
      load_row(y + ((long)b * T + (live ? t : 0)) * ld_y, live, P, lane, v);
      row_stats(v, P, lane, eps, mean, rstd);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const int c = q * 512 + lane * 8;
        if (c < P) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = fmaf((v[q][e] - mean) * rstd, gm[q][e], bt[q][e]);
          st8(rows + row * pitch + c, o);
        }
      }
    }
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // rows ty * 4 .. + 3, column groups tx, tx + 64, ...
  const float* sa = rows + ty * 4 * pitch;
  for (int n = tx * 4; n < N; n += 256) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
#pragma unroll 4
    for (int k = 0; k < P; ++k) {
      const float4 wv4 = *reinterpret_cast<const float4*>(w + (long)k * N + n);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = sa[i * pitch + k];
        acc[i][0] = fmaf(a, wv4.x, acc[i][0]);
        acc[i][1] = fmaf(a, wv4.y, acc[i][1]);
        acc[i][2] = fmaf(a, wv4.z, acc[i][2]);
        acc[i][3] = fmaf(a, wv4.w, acc[i][3]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + ty * 4 + i;
      if (r < rr.lo || r >= rr.hi) continue;
      float4 o = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
      if (bias) {
        const float4 bv = *reinterpret_cast<const float4*>(bias + n);
        o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
      }
      *reinterpret_cast<float4*>(out + ((long)b * Tpad + r) * N + n) = o;
    }
  }
}

}  // namespace

extern "C" int tfasr_rnnt_block_tail_fwd(const void* y, long ld_y, const int32_t* lengths, const int32_t* off, const float* gamma,
                                         const float* beta, const void* W, const float* bias, void* out, int32_t* out_lengths, int B, int T,
                                         int Tpad, int P, int N, int factor, float eps, int dtype, void* stream_) {
  if (!y || !gamma || !beta || !W || !out) return TFASR_STATUS_INVALID_VALUE;
  if (B < 0 || T < 0 || Tpad < T || P <= 0 || N <= 0 || factor < 1 || Tpad % factor != 0 || ld_y < P || !(eps >= 0.f)) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (P % 32 != 0 || P > MAX_P || N % 16 != 0 || N > MAX_N || B > 65535 || (long)Tpad > 0x3fffffffL) return TFASR_STATUS_UNSUPPORTED;
  const size_t esz = dtype == TFASR_F32 ? 4 : 2;
  if ((((uintptr_t)y | (uintptr_t)W | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)bias) & 15) != 0 ||
      ((size_t)ld_y * esz) % 16 != 0)
    return TFASR_STATUS_INVALID_VALUE;
  if (B == 0 || Tpad == 0) return TFASR_STATUS_SUCCESS;
  hipStream_t s = (hipStream_t)stream_;
  if (dtype == TFASR_F32) {
    const int smem = FM * (P + 4) * (int)sizeof(float);
    tfasr_dynamic_lds<tail_f32_kernel>(smem);
    TFASR_KLAUNCH(tail_f32_kernel, dim3((Tpad + FM - 1) / FM, B), dim3(256), (size_t)smem, s, (const float*)y, ld_y, lengths, off, gamma, beta,
                  (const float*)W, bias, (float*)out, out_lengths, T, Tpad, P, N, factor, eps);
  } else {
    const int smem = BM * (P + PAD) * (int)sizeof(bf16_t), Np = (N + 63) / 64 * 64;
    tfasr_dynamic_lds<tail_bf16_kernel>(smem);
    TFASR_KLAUNCH(tail_bf16_kernel, dim3((Tpad + BM - 1) / BM, B), dim3(256), (size_t)smem, s, (const bf16_t*)y, ld_y, lengths, off, gamma, beta,
                  (const bf16_t*)W, bias, (bf16_t*)out, out_lengths, T, Tpad, P, N, Np, factor, eps);
  }
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
