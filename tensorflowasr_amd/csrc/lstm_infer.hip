// Inference LSTM recurrence over one or two directions for gfx950: the RnnBlock of the DeepSpeech2 encoder (encoders/deepspeech2.py:197-256:
// keras.layers.LSTM(return_sequences, zero_output_for_mask=True), alone or inside keras.layers.Bidirectional with the "concat" merge).
//
//   xg [B, T, ndir * 4P] (row stride ld_xg): x @ W_d + b_d of every direction side by side (one GEMM in front of this call)
//   rk [ndir, P, 4P]; gates i, f, c, o; zero initial state, or (tfasr_lstm_infer_fwd_state, one direction) h0 / c0 [B, P] f32: the
//   h_last / c_last of the launch that walked the frames in front of these
//   y  [B, T, ndir * P]  (row stride ld_y): direction d writes columns [d P, (d + 1) P) - already the concat merge
// Direction 0 walks t = 0 .. T-1, direction 1 walks t = T-1 .. 0.  A step with t >= lengths[b] carries h and c and emits zeros, so the
// reverse direction starts, in effect, at each utterance's last valid frame.  h_last / c_last [ndir, B, P] f32: the state after the last
// step walked.  Nothing else is kept: no gate or cell sequence (there is no backward).
//
// bf16, B <= 64, P % 32 == 0, P <= 1024, grid resident: ONE persistent launch of ndir * P/16 workgroups.  It is the forward kernel of
// lstm_persist.hip (workgroup = 16 hidden units, its slice of R in registers, h_{t-1} staged in LDS, z = h R on the matrix cores) with the
// training buffers removed and each direction a group of its own: own arrival counter, own abort word (two Sync records at the front of
// the workspace), own hand-off buffer for h_t ([ndir, B, T, P] bf16 behind the records: one slot per step, never reused inside a
// launch).  The hand-off protocol is lstm_handoff.h's: write-through stores of h_t drained by every storing wave, one agent-scope
// counter, one lane polling relaxed, one agent-scope acquire after the match, every spin bounded by the wall clock, a timed-out
// workgroup poisons what it owns of the remaining steps with NaN, and the launch is refused unless the whole grid can be resident.
// The two directions never wait for each other.
// With a state, step 0 stages h0 (rounded to bf16: exact for a carried value, h_last holds bf16-rounded numbers) where a stateless launch
// stages zeros, and c starts from c0; after that it is a step like any other - the same instructions in the same order as a middle step
// of one long launch, so a sequence walked in several launches gives the bits of one launch over all of it.  On the per-step route step 0
// runs the recurrent GEMM on h0 (cast to the activation type) and takes c0 as c_prev.
// Any other shape or type, and every call while tfasr_lstm_set_persist(0) / TFASR_LSTM_PERSIST=0 is in force: the per-step kernels
// (recurrent tfasr_gemm + tfasr_lstm_step_fwd), direction 0 queued ascending, then direction 1 descending.
#include "lstm_handoff.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------
template <int MT>  // MT = ceil(B / 16) batch row tiles
__global__ __launch_bounds__(256) void lstm_infer_kernel(const bf16_t* __restrict__ xg, long ld_xg, const bf16_t* __restrict__ rk,
                                                         const int32_t* __restrict__ lengths, bf16_t* __restrict__ y, long ld_y, bf16_t* hbuf,
                                                         const float* __restrict__ h0, const float* __restrict__ c0,
                                                         float* __restrict__ h_last, float* __restrict__ c_last, int B, int T, int P,
                                                         Sync* sync) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int nwg = P / PW;                       // workgroups of one direction
  const int d = blockIdx.x / nwg;               // direction = group
  const int u0 = (blockIdx.x - d * nwg) * PW;
  const int Bp = MT * 16;
  // this direction's operands
  xg += (long)d * 4 * P;
  rk += (long)d * P * 4 * P;
  y += (long)d * P;
  bf16_t* hseq = hbuf + (long)d * B * T * P;    // [B, T, P]: the carried h of every step (the hand-off buffer)
  sync += d;
  const int ldh = P * 2 + 16;                       // LDS row stride of the staged h tile in bytes (+16: rows land 4 banks apart)
  char* sH = smem;                                  // [Bp][P] bf16
  float* sZ = reinterpret_cast<float*>(smem + (long)Bp * ldh);  // [4 gates][Bp][16] f32
  const int ks = P / 32;

  // this wave's gate: B fragments of R[:, q*P + u0 + n], k = hidden index (strided 2-byte loads, once)
  short8_t bw[MAXKS];
#pragma unroll
  for (int k = 0; k < MAXKS; ++k) {
    if (k < ks) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bw[k][e] = (short)rk[(long)(k * 32 + g * 8 + e) * 4 * P + w * P + u0 + r];
    }
  }
  // owned items: (batch row b, unit pair up) -> units u0 + 2 up, u0 + 2 up + 1; item = threadIdx.x + 256 * i
  constexpr int NIT = (MT * 16 * (PW / 2) + 255) / 256;
  float c_st[NIT][2], h_st[NIT][2];
  int len_b[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int it = threadIdx.x + 256 * i, b = it / (PW / 2), u = (it % (PW / 2)) * 2;
    const bool in = it < Bp * (PW / 2) && b < B;
    c_st[i][0] = c_st[i][1] = h_st[i][0] = h_st[i][1] = 0.f;
    if (in && h0) {  // (a state belongs to direction 0 alone: the host refuses it with two)
      const float2 hv = *reinterpret_cast<const float2*>(h0 + (long)b * P + u0 + u), cv = *reinterpret_cast<const float2*>(c0 + (long)b * P + u0 + u);
      h_st[i][0] = bf16_to_f32(f32_to_bf16(hv.x)); h_st[i][1] = bf16_to_f32(f32_to_bf16(hv.y));  // what step 0 stages
      c_st[i][0] = cv.x; c_st[i][1] = cv.y;
    }
    len_b[i] = in ? (lengths ? lengths[b] : T) : 0;
  }

  if (h0) {
    // step 0's tile from the state: h0 [B, P] f32 rounded to bf16 (rows >= B: zeros).  Its own loop in front of the recurrence, four
    // 16-byte pieces a pass (their loads in flight together), so that the f32 values are never live beside the steps' staging registers
    const int chunks = P / 8;
#pragma unroll 1
    for (int cf = threadIdx.x; cf < Bp * chunks; cf += 4 * 256) {
      float4 lo[4], hi[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cf + 256 * q, b = c / chunks, ch = c % chunks;
        lo[q] = hi[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < Bp * chunks && b < B) {
          lo[q] = *reinterpret_cast<const float4*>(h0 + (long)b * P + ch * 8);
          hi[q] = *reinterpret_cast<const float4*>(h0 + (long)b * P + ch * 8 + 4);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = cf + 256 * q;
        if (c < Bp * chunks)
          *reinterpret_cast<uint4*>(sH + (long)(c / chunks) * ldh + (c % chunks) * 16) =
              make_uint4(pack2_bf16(lo[q].x, lo[q].y), pack2_bf16(lo[q].z, lo[q].w), pack2_bf16(hi[q].x, hi[q].y), pack2_bf16(hi[q].z, hi[q].w));
      }
    }
  }
  for (int s = 0; s < T; ++s) {
    const int t = d ? T - 1 - s : s, tp = d ? t + 1 : t - 1;  // this step's frame, the previous step's frame
    // input-projection terms of this step for the owned items (independent of the recurrence: in flight during the wait)
    float xz[NIT][4][2];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = threadIdx.x + 256 * i, b = it / (PW / 2), u = (it % (PW / 2)) * 2;
      const bool in = it < Bp * (PW / 2) && b < B;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xz[i][q][0] = xz[i][q][1] = 0.f;
        if (in) ld2(xg + ((long)b * T + t) * ld_xg + q * P + u0 + u, xz[i][q][0], xz[i][q][1]);
      }
    }
    if (s > 0 && !wait_count(sync, (unsigned)nwg * (unsigned)s)) {
      // the frames not walked yet: [t, T) forward, [0, t] backward
      const int lo = d ? 0 : t, hi = d ? t + 1 : T;
      poison_rows(hseq, (long)T * P, P, lo, hi, B, u0, PW);
      poison_rows(y, (long)T * ld_y, ld_y, lo, hi, B, u0, PW);
      return;
    }
    // stage h_{s-1} [Bp][P] (rows >= B: zeros): every load of the tile is issued before the first LDS store
    const int chunks = P / 8;  // 16-B chunks per row
    constexpr int NST = MT * 16 * (32 * MAXKS / 8) / 256;  // 16-B chunks per thread at P = 1024
    uint4 hv[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int c = threadIdx.x + 256 * i;
      hv[i] = make_uint4(0, 0, 0, 0);
      if (c < Bp * chunks) {
        const int b = c / chunks, ch = c % chunks;
        if (b < B && s > 0) hv[i] = *reinterpret_cast<const uint4*>(hseq + ((long)b * T + tp) * P + ch * 8);
      }
    }
    if (s > 0 || !h0) {  // (step 0 of a launch with a state: the tile was staged in front of the loop)
#pragma unroll
      for (int i = 0; i < NST; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < Bp * chunks) *reinterpret_cast<uint4*>(sH + (long)(c / chunks) * ldh + (c % chunks) * 16) = hv[i];
      }
    }
    __syncthreads();
    float4_t acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < MAXKS; ++k) {
      if (k < ks) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const short8_t a = *reinterpret_cast<const short8_t*>(sH + (long)(m * 16 + r) * ldh + (k * 32 + g * 8) * 2);
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bw[k], acc[m], 0, 0, 0);
        }
      }
    }
    // C layout: row = g*4+e (batch row within the tile), col = r (unit)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) sZ[(w * Bp + m * 16 + g * 4 + e) * PW + r] = acc[m][e];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = threadIdx.x + 256 * i, b = it / (PW / 2), u = (it % (PW / 2)) * 2;
      if (it < Bp * (PW / 2) && b < B) {
        float yv[2] = {0.f, 0.f};
        if (t < len_b[i]) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            float z[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) z[q] = xz[i][q][j] + sZ[(q * Bp + b) * PW + u + j];
            const float ig = sigmoidf_(z[0]), fg = sigmoidf_(z[1]), gg = tanh_fast(z[2]), og = sigmoidf_(z[3]);
            const float c = fg * c_st[i][j] + ig * gg;
            const float h = og * tanh_fast(c);
            c_st[i][j] = c;
            h_st[i][j] = bf16_to_f32(f32_to_bf16(h));  // the carried state is what the hand-off buffer holds
            yv[j] = h;
          }
        }
        *reinterpret_cast<unsigned*>(y + ((long)b * T + t) * ld_y + u0 + u) = pack2_bf16(yv[0], yv[1]);
        store_wt2(hseq + ((long)b * T + t) * P + u0 + u, h_st[i][0], h_st[i][1]);
      }
    }
    if (s + 1 < T) arrive(sync);
  }
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int it = threadIdx.x + 256 * i, b = it / (PW / 2), u = (it % (PW / 2)) * 2;
    if (it < Bp * (PW / 2) && b < B) {
      const long o = ((long)d * B + b) * P + u0 + u;
      if (h_last) *reinterpret_cast<float2*>(h_last + o) = make_float2(h_st[i][0], h_st[i][1]);
      if (c_last) *reinterpret_cast<float2*>(c_last + o) = make_float2(c_st[i][0], c_st[i][1]);
    }
  }
}

// the per-step route's final state [B, P] (h in the activation type, c f32) -> h_last / c_last rows of one direction
template <typename T>
__global__ __launch_bounds__(256) void state_out_kernel(const T* __restrict__ h, const float* __restrict__ c, float* __restrict__ h_last,
                                                        float* __restrict__ c_last, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (h_last) h_last[i] = Num<T>::ld(h + i);
  if (c_last) c_last[i] = c[i];
}

// the per-step route's initial h [B, P] f32 -> the activation type (exact for a carried value: it came out of that type)
template <typename T>
__global__ __launch_bounds__(256) void state_in_kernel(const float* __restrict__ h0, T* __restrict__ h, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) Num<T>::st(h + i, h0[i]);
}

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// workspace layout: [ndir Sync records | persistent: h hand-off [ndir, B, T, P] bf16 | step route: per direction hr [B, 4P] f32,
// h [2][B, P] (activation type), c [2][B, P] f32]
struct Layout { size_t sync, hbuf, step, total; };
Layout layout(int B, int T, int P, int ndir, int dtype) {
  Layout l;
  l.sync = 0;
  l.hbuf = align256((size_t)ndir * sizeof(Sync));
  const size_t hand = persist_ok(B, P, dtype) ? align256((size_t)ndir * B * T * P * 2) : 0;
  l.step = l.hbuf + hand;
  const size_t esz = dtype == TFASR_F32 ? 4 : 2;
  const size_t per_dir = align256((size_t)B * 4 * P * 4) + 2 * align256((size_t)B * P * esz) + 2 * align256((size_t)B * P * 4);
  l.total = l.step + per_dir;  // the directions of the step route run one after the other and share one set
  return l;
}

int check_args(int B, int T, int P, int ndir, int dtype) {
  if (B <= 0 || T <= 0 || P <= 0 || (ndir != 1 && ndir != 2)) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_F32 && dtype != TFASR_BF16) return TFASR_STATUS_INVALID_VALUE;
  if ((long)B * T * ndir * 4 * P > 0x7fffffffffL) return TFASR_STATUS_UNSUPPORTED;
  return TFASR_STATUS_SUCCESS;
}

// the rules of a call with a state (tfasr_lstm_infer_fwd_state), judged on the host before anything else about the call
bool state_ok(const float* h0, const float* c0, const float* h_last, const float* c_last, int B, int T, int P, int ndir) {
  if (B <= 0 || T <= 0 || P <= 0) return false;
  if (!h0 || !c0) return false;   // one half of a state alone
  if (ndir != 1) return false;    // a backward direction cannot be continued
  if ((((uintptr_t)h0 | (uintptr_t)c0) & 15) != 0) return false;         // the persistent launch reads them 16 bytes at a time
  if ((((uintptr_t)h_last | (uintptr_t)c_last) & 7) != 0) return false;  // ... and writes these 8 bytes at a time
  // every workgroup of the persistent launch stages ALL of h0 at step 0 while a finished one writes its slice of h_last, and with
  // T == 1 no hand-off lies between the two: the new state goes to other memory
  const size_t n = (size_t)B * P * sizeof(float);
  const auto overlap = [n](const float* a, const float* b) { return a && b && (uintptr_t)a < (uintptr_t)b + n && (uintptr_t)b < (uintptr_t)a + n; };
  return !(overlap(h0, h_last) || overlap(h0, c_last) || overlap(c0, h_last) || overlap(c0, c_last));
}

}  // namespace

extern "C" int tfasr_lstm_infer_workspace_size(int B, int T, int P, int ndir, int dtype, size_t* bytes) {
  if (!bytes) return TFASR_STATUS_INVALID_VALUE;
  const int st = check_args(B, T, P, ndir, dtype);
  if (st != TFASR_STATUS_SUCCESS) return st;
  *bytes = layout(B, T, P, ndir, dtype).total;
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_lstm_infer_fwd(const void* xg, long ld_xg, const void* rk, const int32_t* lengths, void* y, long ld_y, float* h_last,
                                    float* c_last, int B, int T, int P, int ndir, int dtype, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
  return tfasr_lstm_infer_fwd_state(xg, ld_xg, rk, lengths, y, ld_y, nullptr, nullptr, h_last, c_last, B, T, P, ndir, dtype, workspace,
                                    workspace_bytes, stream_);
}

extern "C" int tfasr_lstm_infer_fwd_state(const void* xg, long ld_xg, const void* rk, const int32_t* lengths, void* y, long ld_y, const float* h0,
                                          const float* c0, float* h_last, float* c_last, int B, int T, int P, int ndir, int dtype,
                                          void* workspace, size_t workspace_bytes, void* stream_) {
  if (!xg || !rk || !y || !workspace) return TFASR_STATUS_INVALID_VALUE;
  // a state that cannot be taken is an argument that is wrong: it wins over a shape that is merely too large (check_args' UNSUPPORTED)
  if ((h0 || c0) && !state_ok(h0, c0, h_last, c_last, B, T, P, ndir)) return TFASR_STATUS_INVALID_VALUE;
  const int ca = check_args(B, T, P, ndir, dtype);
  if (ca != TFASR_STATUS_SUCCESS) return ca;
  if (ld_xg < (long)ndir * 4 * P || ld_y < (long)ndir * P || (ld_xg & 1) || (ld_y & 1)) return TFASR_STATUS_INVALID_VALUE;
  if ((((uintptr_t)xg | (uintptr_t)y) & 3) != 0 || (((uintptr_t)rk | (uintptr_t)workspace) & 15) != 0) return TFASR_STATUS_INVALID_VALUE;
  const Layout l = layout(B, T, P, ndir, dtype);
  if (workspace_bytes < l.total) return TFASR_STATUS_INVALID_VALUE;
  hipStream_t s = (hipStream_t)stream_;
  char* ws = (char*)workspace;

  if (tfasr_lstm_persist_on() && persist_ok(B, P, dtype)) {
    const int MT = (B + 15) / 16, Bp = MT * 16;
    const size_t smem = (size_t)Bp * (P * 2 + 16) + (size_t)4 * Bp * PW * 4;
    const dim3 grid(ndir * (P / PW));
    const int st = with_mt(MT, [&](auto mt) -> int {
      auto kernel = lstm_infer_kernel<decltype(mt)::value>;
      if (!grid_fits(kernel, grid.x, smem)) { (void)hipGetLastError(); return TFASR_STATUS_UNSUPPORTED; }
      if (hipMemsetAsync(ws + l.sync, 0, (size_t)ndir * sizeof(Sync), s) != hipSuccess) return TFASR_STATUS_EXECUTION_FAILED;
      TFASR_KLAUNCH(kernel, grid, dim3(256), smem, s, (const bf16_t*)xg, ld_xg, (const bf16_t*)rk, lengths, (bf16_t*)y, ld_y, (bf16_t*)(ws + l.hbuf),
                    h0, c0, h_last, c_last, B, T, P, (Sync*)(ws + l.sync));
      TFASR_CHECK_LAUNCH();
      return TFASR_STATUS_SUCCESS;
    });
    if (st != TFASR_STATUS_UNSUPPORTED) return st;  // (the grid does not fit: the per-step route)
  }

  // per-step route: recurrent GEMM (f32 out) + the cell kernel per step; the state ping-pongs between two [B, P] buffers
  const long esz = dtype == TFASR_F32 ? 4 : 2;
  float* hr = (float*)(ws + l.step);
  char* hb[2];
  float* cb[2];
  size_t off = l.step + align256((size_t)B * 4 * P * 4);
  for (int i = 0; i < 2; ++i) { hb[i] = ws + off; off += align256((size_t)B * P * esz); }
  for (int i = 0; i < 2; ++i) { cb[i] = (float*)(ws + off); off += align256((size_t)B * P * 4); }
  if (h0) {  // (one direction) step 0's h_prev: the buffer step 0 would read had it a predecessor
    const long n = (long)B * P;
    if (dtype == TFASR_F32) TFASR_KLAUNCH(state_in_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h0, (float*)hb[1], n);
    else TFASR_KLAUNCH(state_in_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h0, (bf16_t*)hb[1], n);
    TFASR_CHECK_LAUNCH();
  }
  for (int d = 0; d < ndir; ++d) {
    const char* rkd = (const char*)rk + (size_t)d * P * 4 * P * esz;
    for (int step = 0; step < T; ++step) {
      const int t = d ? T - 1 - step : step;
      const int cur = step & 1, prv = cur ^ 1;
      const bool prev = step > 0 || h0;
      if (prev) {
        const tfasr_gemm_args a = recurrent_gemm_args(hb[prv], P, rkd, hr, B, P, dtype);
        const int st = tfasr_gemm(&a, stream_);
        if (st != TFASR_STATUS_SUCCESS) return st;
      }
      const int st = tfasr_lstm_step_fwd((const char*)xg + ((long)t * ld_xg + (long)d * 4 * P) * esz, (long)T * ld_xg, prev ? hr : nullptr,
                                         prev ? hb[prv] : nullptr, P, step > 0 ? cb[prv] : c0, P, lengths, t, nullptr, 0, cb[cur], P,
                                         hb[cur], P, (char*)y + ((long)t * ld_y + (long)d * P) * esz, (long)T * ld_y, B, P, dtype, stream_);
      if (st != TFASR_STATUS_SUCCESS) return st;
    }
    if (h_last || c_last) {
      const long n = (long)B * P;
      const int last = (T - 1) & 1;
      float* hl = h_last ? h_last + (long)d * n : nullptr;
      float* cl = c_last ? c_last + (long)d * n : nullptr;
      if (dtype == TFASR_F32)
        TFASR_KLAUNCH(state_out_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)hb[last], cb[last], hl, cl, n);
      else
        TFASR_KLAUNCH(state_out_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16_t*)hb[last], cb[last], hl, cl, n);
    }
  }
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}
