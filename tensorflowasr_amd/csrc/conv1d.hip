// Causal dense Conv1D, channels-last, for gfx950: the encoder of the Jasper CTC model (encoders/jasper.py: Conv1D(padding="causal") ->
// BatchNormalization -> [+ residuals] -> ReLU), offline and streamed.
//
//   y[b, t, n] = epi( sum_k sum_c xin[b, lead + t * stride + (k - (K - 1)) * dilation, c] * w[k, c, n] ),  t < ceil(T / stride)
//
// x is [B, lead + T, Cin]: `lead` rows of REAL left context in front of the T rows the call convolves (a stream's carried tail; 0 offline).
// Input rows in front of the buffer are zeros - the causal padding - and so are rows past lead + T; no tile reads another batch row.
//
// Tiling.  Consecutive output rows share K - 1 of their K input rows, so a workgroup stages ONE slab of
// (BM - 1) * stride + (K - 1) * dilation + 1 input rows by a channel chunk in LDS and slides the K taps over it: every input element is
// fetched from HBM once per (row tile, Cout tile), not K times as a per-tap GEMM over shifted row views does.  Grid = (row tile inside one
// utterance, Cout tile, b): a tile never straddles utterances.
//   bf16: BM 128 x BN 64, 4 waves of 64 x 32, mfma_f32_16x16x32_bf16, chunk = 32 channels = one MFMA k-step per tap.  The A operand
//         (lane l: row l & 15, channels 8 (l >> 4) ..) is one ds_read_b128 per 16 rows from the slab, row pitch 80 B (20 dwords: the 16
//         rows of a stride-1 read start in 16 different 4-dword bank groups).  The B operand comes from a copy of the weight packed once
//         at load time as [K][chunk][Cout rounded up to 64][32 channels] bf16 (zero filled), so lane l's 8 channels of column l & 15 are 16
//         contiguous bytes: no transpose, no LDS; the next tap's fragments are loaded while the current tap's MFMAs run.
//   f32 : the parity twin (token-exact inference): BM 64 x BN 64, 4 x 4 outputs per thread, plain FMAs, weight in the Keras layout.
// Fixed order.  An output element is reduced over channel chunks in ascending order, inside a chunk over taps k = 0 .. K-1, inside a tap
// over the chunk's channels (one MFMA / a 16-step FMA chain); padding contributes exact zeros.  There is one tile shape per type and no
// split over the reduction, so the value does not depend on the row's place in a tile, on B, on T or on lead: a stream that supplies the
// (K - 1) * dilation rows in front of a chunk as real rows gets the bits the whole utterance gets.
// Epilogue (f32, before the store): v = (acc + bias[n]) * scale[n] + shift[n]  (inference BatchNorm folded to an affine pair);
// v += addend[b, t, n]; optional ReLU.
#include "common.h"

namespace {

constexpr int MAX_TAPS = 32, MAX_SPAN = 256;  // K, (K - 1) * dilation

__device__ __forceinline__ float epilogue(float v, int n, const float* __restrict__ bias, const float* __restrict__ scale,
                                          const float* __restrict__ shift) {
  if (bias) v += bias[n];
  if (scale) v *= scale[n];
  if (shift) v += shift[n];
  return v;
}

// ------------------------------------------------------------------------------------------------ bf16 (MFMA)
constexpr int BM = 128, BN = 64, CK = 32, PITCH = 40;  // PITCH in bf16 elements (80 B)

__global__ __launch_bounds__(256) void conv1d_bf16_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const bf16_t* __restrict__ addend,
                                                          bf16_t* __restrict__ y, int T, int Tout, int lead, int Cin, int Cout, int K,
                                                          int stride, int dil, int relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_[];
  bf16_t* slab = reinterpret_cast<bf16_t*>(smem_);
  const int t0 = blockIdx.x * BM, n0 = blockIdx.y * BN, b = blockIdx.z;
  const int Tin = lead + T, R = (BM - 1) * stride + (K - 1) * dil + 1;
  const int in0 = t0 * stride - (K - 1) * dil + lead;  // input row of slab row 0
  const int nch = (Cin + CK - 1) / CK, Np = gridDim.y * BN;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wm = wv & 1, wn = wv >> 1, r = lane & 15, g = lane >> 4;
  const bf16_t* xb = x + (long)b * Tin * Cin;
  float4_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
  const bf16_t* arow = slab + (wm * 64 + r) * stride * PITCH + g * 8;
  for (int ch = 0; ch < nch; ++ch) {
    const int c0 = ch * CK;
    __syncthreads();
    for (int idx = threadIdx.x; idx < R * 4; idx += 256) {
      const int rr = idx >> 2, q = idx & 3, row = in0 + rr, c = c0 + q * 8;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row >= 0 && row < Tin && c < Cin) v = *reinterpret_cast<const uint4*>(xb + (long)row * Cin + c);
      *reinterpret_cast<uint4*>(slab + rr * PITCH + q * 8) = v;
    }
    __syncthreads();
    const bf16_t* wb = wp + ((long)ch * Np + n0 + wn * 32 + r) * CK + g * 8;
    const long wstep = (long)nch * Np * CK;  // one tap
    short8_t bcur[2], bnxt[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bcur[j] = *reinterpret_cast<const short8_t*>(wb + j * 16 * CK);
    for (int k = 0; k < K; ++k) {
      if (k + 1 < K) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bnxt[j] = *reinterpret_cast<const short8_t*>(wb + (k + 1) * wstep + j * 16 * CK);
      }
      short8_t a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const short8_t*>(arow + (i * 16 * stride + k * dil) * PITCH);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bcur[j], acc[i][j], 0, 0, 0);
      if (k + 1 < K) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bcur[j] = bnxt[j];
      }
    }
  }
  // C / D map of the 16x16 tile: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 32 + j * 16 + r;
    if (n >= Cout) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = t0 + wm * 64 + i * 16 + g * 4 + e;
        if (t >= Tout) continue;
        const long o = ((long)b * Tout + t) * Cout + n;
        float v = epilogue(acc[i][j][e], n, bias, scale, shift);
        if (addend) v += bf16_to_f32(addend[o]);
        if (relu) v = fmaxf(v, 0.f);
        y[o] = f32_to_bf16(v);
      }
  }
}

// [K, Cin, Cout] f32 (Keras) -> [K][chunk][Np][32] bf16, zero filled past Cin / Cout
__global__ __launch_bounds__(256) void conv1d_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp, int K, int Cin, int Cout,
                                                          int nch, int Np) {
  const long total = (long)K * nch * Np * CK;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % CK);
    const long q = i / CK;
    const int n = (int)(q % Np);
    const long q2 = q / Np;
    const int ch = (int)(q2 % nch), k = (int)(q2 / nch), ci = ch * CK + c;
    wp[i] = (ci < Cin && n < Cout) ? f32_to_bf16(w[((long)k * Cin + ci) * Cout + n]) : (bf16_t)0;
  }
}

// ------------------------------------------------------------------------------------------------ f32 twin (FMA)
constexpr int FM = 64, FN = 64, FC = 16, FP = FC + 1;

__global__ __launch_bounds__(256) void conv1d_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, const float* __restrict__ addend,
                                                         float* __restrict__ y, int T, int Tout, int lead, int Cin, int Cout, int K, int stride,
                                                         int dil, int relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_[];
  float* slab = reinterpret_cast<float*>(smem_);
  const int t0 = blockIdx.x * FM, n0 = blockIdx.y * FN, b = blockIdx.z;
  const int Tin = lead + T, R = (FM - 1) * stride + (K - 1) * dil + 1;
  const int in0 = t0 * stride - (K - 1) * dil + lead;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, n = n0 + tx * 4;
  const bool ncol = n < Cout;  // Cout % 16 == 0: the four columns of a thread are in or out together
  const float* xb = x + (long)b * Tin * Cin;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int c0 = 0; c0 < Cin; c0 += FC) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < R * FC; idx += 256) {
      const int rr = idx >> 4, c = idx & 15, row = in0 + rr;
      slab[rr * FP + c] = (row >= 0 && row < Tin) ? xb[(long)row * Cin + c0 + c] : 0.f;
    }
    __syncthreads();
    if (!ncol) continue;
    for (int k = 0; k < K; ++k) {
      const float* sa = slab + (ty * 4 * stride + k * dil) * FP;
      const float* wk = w + ((long)k * Cin + c0) * Cout + n;
#pragma unroll 4
      for (int c = 0; c < FC; ++c) {
        const float4 wv = *reinterpret_cast<const float4*>(wk + (long)c * Cout);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float a = sa[i * stride * FP + c];
          acc[i][0] = fmaf(a, wv.x, acc[i][0]);
          acc[i][1] = fmaf(a, wv.y, acc[i][1]);
          acc[i][2] = fmaf(a, wv.z, acc[i][2]);
          acc[i][3] = fmaf(a, wv.w, acc[i][3]);
        }
      }
    }
  }
  if (!ncol) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = t0 + ty * 4 + i;
    if (t >= Tout) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long o = ((long)b * Tout + t) * Cout + n + j;
      float v = epilogue(acc[i][j], n + j, bias, scale, shift);
      if (addend) v += addend[o];
      if (relu) v = fmaxf(v, 0.f);
      y[o] = v;
    }
  }
}

// tail[b, r, :] = window[b, clamp(nvalid[b]) + r, :]: the last `tail_rows` valid rows of [old tail | new rows]; nvalid == 0 copies the old
// tail onto itself bit for bit.  grid (ceil(tail_rows * C / 256), B)
template <typename T>
__global__ __launch_bounds__(256) void conv1d_tail_kernel(const T* __restrict__ win, const int32_t* __restrict__ nvalid, T* __restrict__ tail,
                                                          int rows, int tail_rows, int C) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= tail_rows * C) return;
  const int nv = min(max(nvalid[b], 0), rows - tail_rows);
  tail[(long)b * tail_rows * C + i] = win[((long)b * rows + nv) * C + i];
}

int check_shape(int B, int T, int lead, int Cin, int Cout, int K, int stride, int dilation, int dtype) {
  if (B < 0 || T < 0 || lead < 0 || Cin <= 0 || Cout <= 0 || K <= 0 || stride <= 0 || dilation <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (K > MAX_TAPS || stride > 2 || Cin % 16 != 0 || Cout % 16 != 0 || (long)(K - 1) * dilation > MAX_SPAN) return TFASR_STATUS_UNSUPPORTED;
  if ((long)lead + T > 0x3fffffffL) return TFASR_STATUS_UNSUPPORTED;
  return TFASR_STATUS_SUCCESS;
}

}  // namespace

extern "C" int tfasr_conv1d_packed_weight_elems(int K, int Cin, int Cout, size_t* elems) {
  if (!elems) return TFASR_STATUS_INVALID_VALUE;
  const int st = check_shape(1, 1, 0, Cin, Cout, K, 1, 1, TFASR_BF16);
  if (st != TFASR_STATUS_SUCCESS) return st;
  *elems = (size_t)K * ((Cin + CK - 1) / CK) * ((Cout + BN - 1) / BN * BN) * CK;
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_conv1d_pack_weight(const float* w, void* packed, int K, int Cin, int Cout, void* stream_) {
  if (!w || !packed) return TFASR_STATUS_INVALID_VALUE;
  const int st = check_shape(1, 1, 0, Cin, Cout, K, 1, 1, TFASR_BF16);
  if (st != TFASR_STATUS_SUCCESS) return st;
  const int nch = (Cin + CK - 1) / CK, Np = (Cout + BN - 1) / BN * BN;
  const long total = (long)K * nch * Np * CK;
  TFASR_KLAUNCH(conv1d_pack_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0,
                (hipStream_t)stream_, w, (bf16_t*)packed, K, Cin, Cout, nch, Np);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_conv1d_workspace_size(int B, int T, int Cin, int Cout, int K, int stride, int dilation, int dtype, size_t* bytes) {
  if (!bytes) return TFASR_STATUS_INVALID_VALUE;
  const int st = check_shape(B, T, 0, Cin, Cout, K, stride, dilation, dtype);
  if (st != TFASR_STATUS_SUCCESS) return st;
  *bytes = 0;  // the slab lives in LDS and there is no split over the reduction: nothing to stage in HBM
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_conv1d_fwd(const void* x, const void* w, const float* bias, const float* scale, const float* shift, const void* addend,
                                void* y, int B, int T, int lead, int Cin, int Cout, int K, int stride, int dilation, int relu, int dtype,
                                void* workspace, size_t workspace_bytes, void* stream_) {
  (void)workspace;
  (void)workspace_bytes;
  if (!x || !w || !y) return TFASR_STATUS_INVALID_VALUE;
  const int st = check_shape(B, T, lead, Cin, Cout, K, stride, dilation, dtype);
  if (st != TFASR_STATUS_SUCCESS) return st;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)addend) & 15) != 0) return TFASR_STATUS_INVALID_VALUE;
  const int Tout = (T + stride - 1) / stride;
  if (B == 0 || Tout == 0) return TFASR_STATUS_SUCCESS;
  hipStream_t s = (hipStream_t)stream_;
  const size_t esz = dtype == TFASR_F32 ? 4 : 2;
  const long xrow = (long)(lead + T) * Cin, yrow = (long)Tout * Cout;
  for (int b0 = 0; b0 < B; b0 += 65535) {  // gridDim.z
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    const char* xp = (const char*)x + (size_t)b0 * xrow * esz;
    const char* ap = addend ? (const char*)addend + (size_t)b0 * yrow * esz : nullptr;
    char* yp = (char*)y + (size_t)b0 * yrow * esz;
    if (dtype == TFASR_F32) {
      const int R = (FM - 1) * stride + (K - 1) * dilation + 1;
      const dim3 grid((Tout + FM - 1) / FM, (Cout + FN - 1) / FN, nb);
      TFASR_KLAUNCH(conv1d_f32_kernel, grid, dim3(256), (size_t)R * FP * sizeof(float), s, (const float*)xp, (const float*)w, bias, scale, shift,
                    (const float*)ap, (float*)yp, T, Tout, lead, Cin, Cout, K, stride, dilation, relu);
    } else {
      const int R = (BM - 1) * stride + (K - 1) * dilation + 1;
      const dim3 grid((Tout + BM - 1) / BM, (Cout + BN - 1) / BN, nb);
      TFASR_KLAUNCH(conv1d_bf16_kernel, grid, dim3(256), (size_t)R * PITCH * sizeof(bf16_t), s, (const bf16_t*)xp, (const bf16_t*)w, bias, scale,
                    shift, (const bf16_t*)ap, (bf16_t*)yp, T, Tout, lead, Cin, Cout, K, stride, dilation, relu);
    }
  }
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_conv1d_tail_update(const void* window, const int32_t* nvalid, void* tail, int B, int rows, int tail_rows, int C, int dtype,
                                        void* stream_) {
  if (!window || !nvalid || !tail || B <= 0 || rows <= 0 || tail_rows <= 0 || C <= 0 || tail_rows > rows) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if (B > 65535 || (long)tail_rows * C > 0x3fffffffL) return TFASR_STATUS_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((tail_rows * C + 255) / 256, B);
  if (dtype == TFASR_F32)
    TFASR_KLAUNCH(conv1d_tail_kernel<float>, grid, dim3(256), 0, s, (const float*)window, nvalid, (float*)tail, rows, tail_rows, C);
  else
    TFASR_KLAUNCH(conv1d_tail_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)window, nvalid, (bf16_t*)tail, rows, tail_rows, C);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
