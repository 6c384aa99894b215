// General strided Conv2D forward, channels-last, for gfx950: the convolution blocks of the DeepSpeech2 encoder (encoders/deepspeech2.py:
// ConvBlock = Conv2D("same" | the reference's "causal") -> BatchNormalization -> ReLU, kernels 11x41 / 11x21, strides (2,2) / (1,2)).
//
//   x [B, T, F, Cin]   w keras [kh, kw, Cin, Cout]   y [B, T', F', Cout]
//   y[b,t,f,n] = epi( sum_i sum_j sum_c x[b, t*st + i - pad_t, f*sf + j - pad_f, c] * w[i,j,c,n] )      (reads outside the buffer are zero)
//   epi(v) = (v + bias[n]) * scale[n] + shift[n], ReLU when relu != 0: in f32 before the store, each vector may be NULL.
// pad_t, pad_f, T', F' are the caller's (the padding rule lives on the host).
//
// bf16 (MFMA).  In channels-last memory the (kw, Cin) window of ONE tap row i is one contiguous run of S = kw * Cin elements of input row
// t*st + i - pad_t, starting at frequency position f*sf - pad_f: the reduction over (j, c) is a dot product of two contiguous runs, cut in
// MFMA k-steps of 32.  The packed weight [kh][KS = ceil(S / 32)][Cout rounded up to 32][32] pads every tap row's run with zeros to a whole
// k-step, which is how Cin = 1 (S = kw) rides the same kernel.  Tile = 4 output rows t' x 16 output positions f' x 32 output channels, four
// waves = the four rows, mfma_f32_16x16x32_bf16 with M = the 16 positions.  Per tap row the workgroup stages the 4 input rows it needs, cut to
// the 15*sf + kw (+ the k-step overshoot) positions of the tile, in LDS - every staged row serves all kw taps and all 16 positions - and
// slides over it: lane l reads position (l & 15) * sf + e / Cin, channel e % Cin for e = 32 kk + 8 (l >> 4).  Each position's channel vector
// is padded by 16 bytes in LDS (positions sf apart would otherwise start in the same banks); Cin = 1 keeps the row dense and reads it
// with 2-byte loads (the 8-element run of a lane starts at any even or odd element there).
// The overshoot of the last k-step of a tap row reads staged (finite) neighbours against zero weights: exact zeros for finite inputs.
// f32 (FMA): the parity twin over the Keras kernel, no LDS: one thread = 4 positions f' x 4 channels of one output row, the operands come
// through the vector cache.  It is the token-exact path, not a fast one.
// Fixed order.  bf16: tap rows ascending, inside a row k-steps ascending (one MFMA each).  f32: per tap row one FMA chain over (j, c)
// ascending, the row sums added in ascending order.  One tile shape per type, no split reduction: a value does not depend on B, T, the
// tile its row falls in, or its place there.
#include "common.h"

namespace {

constexpr int MAX_KH = 16, MAX_KW = 48, MAX_COUT = 128, MAX_CIN = 128;
constexpr int TT = 4, FT = 16, BN = 32, CK = 32;  // bf16 tile: rows, positions, channels; MFMA k

__device__ __forceinline__ float epilogue(float v, int n, const float* __restrict__ bias, const float* __restrict__ scale,
                                          const float* __restrict__ shift, int relu) {
  if (bias) v += bias[n];
  if (scale) v *= scale[n];
  if (shift) v += shift[n];
  if (relu) v = fmaxf(v, 0.f);
  return v;
}

struct Shape { int T, F, Cin, Cout, kh, kw, st, sf, pad_t, pad_f, To, Fo; };

// staged positions per row / LDS elements per position
__host__ __device__ inline int staged_positions(int Cin, int kw, int sf) {
  const int KS = (kw * Cin + CK - 1) / CK;
  return (FT - 1) * sf + (Cin == 1 ? KS * CK : kw + 2);
}
__host__ __device__ inline int position_pitch(int Cin) { return Cin == 1 ? 1 : Cin + 8; }

template <bool ONE>  // ONE: Cin == 1
__global__ __launch_bounds__(256) void conv2d_bf16_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, bf16_t* __restrict__ y, Shape s, int relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_[];
  bf16_t* slab = reinterpret_cast<bf16_t*>(smem_);
  const int ftiles = (s.Fo + FT - 1) / FT;
  const int f0 = (blockIdx.x % ftiles) * FT, n0 = (blockIdx.x / ftiles) * BN, t0 = blockIdx.y * TT, b = blockIdx.z;
  const int Np = (s.Cout + BN - 1) / BN * BN, KS = (s.kw * s.Cin + CK - 1) / CK;
  const int WP = staged_positions(s.Cin, s.kw, s.sf), CP = position_pitch(s.Cin);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int p0 = f0 * s.sf - s.pad_f;  // frequency position of staged position 0
  const bf16_t* xb = x + (long)b * s.T * s.F * s.Cin;
  float4_t acc[2] = {float4_t{0.f, 0.f, 0.f, 0.f}, float4_t{0.f, 0.f, 0.f, 0.f}};
  const bf16_t* arow = slab + ((long)wv * WP + r * s.sf) * CP;
  for (int i = 0; i < s.kh; ++i) {
    __syncthreads();
    if (ONE) {
      for (int idx = threadIdx.x; idx < TT * WP; idx += 256) {
        const int tt = idx / WP, pl = idx - tt * WP, row = (t0 + tt) * s.st + i - s.pad_t, p = p0 + pl;
        slab[idx] = (row >= 0 && row < s.T && p >= 0 && p < s.F) ? xb[(long)row * s.F + p] : (bf16_t)0;
      }
    } else {
      const int c8n = s.Cin >> 3;
      for (int idx = threadIdx.x; idx < TT * WP * c8n; idx += 256) {
        const int c8 = idx % c8n, q = idx / c8n, tt = q / WP, pl = q - tt * WP, row = (t0 + tt) * s.st + i - s.pad_t, p = p0 + pl;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row >= 0 && row < s.T && p >= 0 && p < s.F) v = *reinterpret_cast<const uint4*>(xb + ((long)row * s.F + p) * s.Cin + c8 * 8);
        *reinterpret_cast<uint4*>(slab + (long)q * CP + c8 * 8) = v;
      }
    }
    __syncthreads();
    const bf16_t* wb = wp + (((long)i * KS) * Np + n0 + r) * CK + g * 8;
    short8_t bcur[2], bnxt[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bcur[j] = *reinterpret_cast<const short8_t*>(wb + j * 16 * CK);
    int pos = 0, c = g * 8;  // (position, channel) of element 32 kk + 8 g of the run
    if (!ONE) while (c >= s.Cin) { c -= s.Cin; ++pos; }
    for (int kk = 0; kk < KS; ++kk) {
      if (kk + 1 < KS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bnxt[j] = *reinterpret_cast<const short8_t*>(wb + ((long)(kk + 1) * Np + j * 16) * CK);
      }
      short8_t a;
      if (ONE) {
        const bf16_t* ap = arow + kk * CK + g * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (short)ap[e];
      } else {
        a = *reinterpret_cast<const short8_t*>(arow + pos * CP + c);
        c += CK;
        while (c >= s.Cin) { c -= s.Cin; ++pos; }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bcur[j], acc[j], 0, 0, 0);
      if (kk + 1 < KS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bcur[j] = bnxt[j];
      }
    }
  }
  // C / D map of the 16x16 tile: column (channel) = lane & 15, row (position) = 4 (lane >> 4) + register
  const int t = t0 + wv;
  if (t >= s.To) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + j * 16 + r;
    if (n >= s.Cout) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = f0 + g * 4 + e;
      if (f >= s.Fo) continue;
      y[(((long)b * s.To + t) * s.Fo + f) * s.Cout + n] = f32_to_bf16(epilogue(acc[j][e], n, bias, scale, shift, relu));
    }
  }
}

// [kh, kw, Cin, Cout] f32 (Keras) -> [kh][KS][Np][32] bf16, zero filled past kw * Cin / Cout
__global__ __launch_bounds__(256) void conv2d_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ wp, int kh, int S, int Cout, int KS,
                                                          int Np) {
  const long total = (long)kh * KS * Np * CK;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int e = (int)(idx % CK);
    const long q = idx / CK;
    const int n = (int)(q % Np);
    const long q2 = q / Np;
    const int kk = (int)(q2 % KS), i = (int)(q2 / KS), k = kk * CK + e;
    wp[idx] = (k < S && n < Cout) ? f32_to_bf16(w[((long)i * S + k) * Cout + n]) : (bf16_t)0;
  }
}

// ------------------------------------------------------------------------------------------------ f32 twin (FMA)
// thread = 4 positions x 4 channels of output row (b, t); a block = 256 such threads of ONE output row (grid.x covers its positions)
__global__ __launch_bounds__(256) void conv2d_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ y,
                                                         Shape s, int relu) {
  const int n4 = s.Cout >> 2, fq = (s.Fo + 3) >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n4 * fq) return;
  const int n = (idx % n4) * 4, f0 = (idx / n4) * 4, t = blockIdx.y, b = blockIdx.z;
  const float* xb = x + (long)b * s.T * s.F * s.Cin;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[a][j] = 0.f;
  for (int i = 0; i < s.kh; ++i) {
    const int row = t * s.st + i - s.pad_t;
    if (row < 0 || row >= s.T) continue;  // a row of zeros adds exact zeros
    const float* xr = xb + (long)row * s.F * s.Cin;
    float part[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) part[a][j] = 0.f;
    for (int j = 0; j < s.kw; ++j) {
      int p[4];
      bool in[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        p[a] = (f0 + a) * s.sf + j - s.pad_f;
        in[a] = p[a] >= 0 && p[a] < s.F;
      }
      const float* wk = w + ((long)(i * s.kw + j) * s.Cin) * s.Cout + n;
      for (int c = 0; c < s.Cin; ++c) {
        const float4 wv = *reinterpret_cast<const float4*>(wk + (long)c * s.Cout);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float v = in[a] ? xr[(long)p[a] * s.Cin + c] : 0.f;
          part[a][0] = fmaf(v, wv.x, part[a][0]);
          part[a][1] = fmaf(v, wv.y, part[a][1]);
          part[a][2] = fmaf(v, wv.z, part[a][2]);
          part[a][3] = fmaf(v, wv.w, part[a][3]);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[a][j] += part[a][j];
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int f = f0 + a;
    if (f >= s.Fo) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      y[(((long)b * s.To + t) * s.Fo + f) * s.Cout + n + j] = epilogue(acc[a][j], n + j, bias, scale, shift, relu);
  }
}

// y[r, c] = x[r, c] * scale[c] + shift[c], ReLU when relu != 0 (an inference BatchNorm + activation behind a layer without an epilogue)
template <typename T>
__global__ __launch_bounds__(256) void channel_affine_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, T* __restrict__ y, long n, int C, int relu) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    float v = Num<T>::ld(x + i);
    if (scale) v *= scale[c];
    if (shift) v += shift[c];
    if (relu) v = fmaxf(v, 0.f);
    Num<T>::st(y + i, v);
  }
}

int check_weight(int kh, int kw, int Cin, int Cout) {
  if (kh <= 0 || kw <= 0 || Cin <= 0 || Cout <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (kh > MAX_KH || kw > MAX_KW || (Cin != 1 && Cin % 16 != 0) || Cin > MAX_CIN || Cout % 16 != 0 || Cout > MAX_COUT) return TFASR_STATUS_UNSUPPORTED;
  return TFASR_STATUS_SUCCESS;
}

int check_shape(int B, int T, int F, int To, int Fo, int Cin, int Cout, int kh, int kw, int st, int sf, int pad_t, int pad_f, int dtype) {
  if (B <= 0 || T <= 0 || F <= 0 || To <= 0 || Fo <= 0 || st <= 0 || sf <= 0 || pad_t < 0 || pad_f < 0) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  const int cw = check_weight(kh, kw, Cin, Cout);
  if (cw != TFASR_STATUS_SUCCESS) return cw;
  if (st > 3 || sf > 2) return TFASR_STATUS_UNSUPPORTED;
  // the index arithmetic is 32-bit per batch row and the grid's y dimension counts output rows (f32) or tiles of them
  if ((long)T * F * Cin > 0x3fffffffL || (long)To * Fo * Cout > 0x3fffffffL || To > 65535 || (long)To * st > 0x3fffffffL ||
      (long)Fo * sf > 0x3fffffffL || pad_t > 0xffff || pad_f > 0xffff)
    return TFASR_STATUS_UNSUPPORTED;
  return TFASR_STATUS_SUCCESS;
}

}  // namespace

extern "C" int tfasr_conv2d_packed_weight_elems(int kh, int kw, int Cin, int Cout, size_t* elems) {
  if (!elems) return TFASR_STATUS_INVALID_VALUE;
  const int st = check_weight(kh, kw, Cin, Cout);
  if (st != TFASR_STATUS_SUCCESS) return st;
  *elems = (size_t)kh * ((kw * Cin + CK - 1) / CK) * ((Cout + BN - 1) / BN * BN) * CK;
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_conv2d_pack_weight(const float* w, void* packed, int kh, int kw, int Cin, int Cout, void* stream_) {
  if (!w || !packed) return TFASR_STATUS_INVALID_VALUE;
  const int st = check_weight(kh, kw, Cin, Cout);
  if (st != TFASR_STATUS_SUCCESS) return st;
  const int KS = (kw * Cin + CK - 1) / CK, Np = (Cout + BN - 1) / BN * BN;
  const long total = (long)kh * KS * Np * CK;
  TFASR_KLAUNCH(conv2d_pack_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0,
                (hipStream_t)stream_, w, (bf16_t*)packed, kh, kw * Cin, Cout, KS, Np);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_conv2d_workspace_size(int B, int T, int F, int To, int Fo, int Cin, int Cout, int kh, int kw, int st, int sf, int pad_t,
                                           int pad_f, int dtype, size_t* bytes) {
  if (!bytes) return TFASR_STATUS_INVALID_VALUE;
  const int s = check_shape(B, T, F, To, Fo, Cin, Cout, kh, kw, st, sf, pad_t, pad_f, dtype);
  if (s != TFASR_STATUS_SUCCESS) return s;
  *bytes = 0;  // the staged rows live in LDS and there is no split over the reduction
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_conv2d_fwd(const void* x, const void* w, const float* bias, const float* scale, const float* shift, void* y, int B, int T,
                                int F, int To, int Fo, int Cin, int Cout, int kh, int kw, int st, int sf, int pad_t, int pad_f, int relu,
                                int dtype, void* workspace, size_t workspace_bytes, void* stream_) {
  (void)workspace;
  (void)workspace_bytes;
  if (!x || !w || !y) return TFASR_STATUS_INVALID_VALUE;
  const int cs = check_shape(B, T, F, To, Fo, Cin, Cout, kh, kw, st, sf, pad_t, pad_f, dtype);
  if (cs != TFASR_STATUS_SUCCESS) return cs;
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) != 0) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  const Shape sh{T, F, Cin, Cout, kh, kw, st, sf, pad_t, pad_f, To, Fo};
  const size_t esz = dtype == TFASR_F32 ? 4 : 2;
  const long xrow = (long)T * F * Cin, yrow = (long)To * Fo * Cout;
  for (int b0 = 0; b0 < B; b0 += 65535) {  // gridDim.z
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    const char* xp = (const char*)x + (size_t)b0 * xrow * esz;
    char* yp = (char*)y + (size_t)b0 * yrow * esz;
    if (dtype == TFASR_F32) {
      const dim3 grid(((Cout / 4) * ((Fo + 3) / 4) + 255) / 256, To, nb);
      TFASR_KLAUNCH(conv2d_f32_kernel, grid, dim3(256), 0, s, (const float*)xp, (const float*)w, bias, scale, shift, (float*)yp, sh, relu);
    } else {
      const size_t smem = (size_t)TT * staged_positions(Cin, kw, sf) * position_pitch(Cin) * sizeof(bf16_t);
      const dim3 grid(((Fo + FT - 1) / FT) * ((Cout + BN - 1) / BN), (To + TT - 1) / TT, nb);
      if (Cin == 1) {
        TFASR_KLAUNCH(conv2d_bf16_kernel<true>, grid, dim3(256), smem, s, (const bf16_t*)xp, (const bf16_t*)w, bias, scale, shift, (bf16_t*)yp,
                      sh, relu);
      } else {
        if (smem > 48 * 1024) tfasr_dynamic_lds<conv2d_bf16_kernel<false>>((int)smem);
        TFASR_KLAUNCH(conv2d_bf16_kernel<false>, grid, dim3(256), smem, s, (const bf16_t*)xp, (const bf16_t*)w, bias, scale, shift, (bf16_t*)yp,
                      sh, relu);
      }
    }
  }
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_channel_affine_fwd(const void* x, const float* scale, const float* shift, void* y, long rows, int C, int relu, int dtype,
                                        void* stream_) {
  if (!x || !y || rows <= 0 || C <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  const long n = rows * C;
  const dim3 grid((unsigned)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192));
  if (dtype == TFASR_F32)
    TFASR_KLAUNCH(channel_affine_kernel<float>, grid, dim3(256), 0, s, (const float*)x, scale, shift, (float*)y, n, C, relu);
  else
    TFASR_KLAUNCH(channel_affine_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, scale, shift, (bf16_t*)y, n, C, relu);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
