// Fused relative-position attention, forward (flash style) for gfx950, head size 64, bf16.
//
//   out[b,i,h,:] = softmax_j( scale*[(q_i+u).k_j + (q_i+v).p_{idx(i,j)}] ) @ v      (multihead_attention.py:543-582)
// with the relative shift (:27-77) and the per-sample roll/zero of the relative PE (positional_encoding.py:152-172) as
// index arithmetic:  idx(i,j) = r + (T-len_b) if r = T-1-i+j < 2*len_b-1 else R (the bias row), R = 2T-1
// (see attention.hip for the derivation; `pext` is the projected table [R+1, H*64]).
// Nothing of size T x T touches HBM: per (b, h, 64-query block) the kernel streams 64-key blocks of K, V and the
// 127-row window of `pext` that the block's (i,j) pairs need through LDS (global_load_lds), computes the content
// scores and the window scores G = (q+v) @ window^T with MFMA, reads G back skewed (col = 63-il+jl) from a per-wave LDS
// strip, runs an online softmax in registers and accumulates P@V.  Saves lse[b,h,i] = log sum_j exp(s_ij) for the backward.
// Auto-mask semantics as in attention.hip: padded QUERY rows give uniform attention over all T keys; keys are never masked.
#include "common.h"
#ifdef TFASR_ATTN_TIMING  // probe build (tools/build_probe_lib.sh attn_fused.hip -DTFASR_ATTN_TIMING): shader clocks per phase
__device__ long long g_attn_timing[8 * 8192];
#define ATT_TICK(k) { const long long t_ = __builtin_readcyclecounter(); ph[k] += t_ - tp; tp = t_; }
#else
#define ATT_TICK(k)
#endif
#include <algorithm>
#include <stdlib.h>

typedef __attribute__((ext_vector_type(4))) short short4_t;

namespace {

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

constexpr int DH = 64, BI = 64, BJ = 64, WIN = 128;
constexpr int SK_BYTES = BJ * DH * 2, SV_BYTES = BJ * DH * 2, SP_BYTES = WIN * DH * 2;
// chunk swizzle of the 128-byte-row images: bits 0, 1 and 3 of the row.  With it the three ways these images are read are all free of
// bank conflicts (tools/hwprobe/lds_sim.py): 16 consecutive rows per ds_read_b128 lane group, the key-dealt rows of the transposed kernels
// (32q + 8a + o + b: rows 0-3, 8-11, 16-19, 24-27 in one group), and the transposed ds_read_b64_tr_b16 fragments (rows k..k+3 and k+8..k+11
// in one 32-lane group).  The earlier (row >> 1) & 7 served only the first: 2-way conflicts on the other two, SQ_LDS_BANK_CONFLICT =
// 0.49 / 0.43 of the LDS cycles of the query-backward / forward kernels.
__device__ __forceinline__ int key_d(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }
__device__ __forceinline__ int key_t64(int k) { return (((k >> 1) & 1) | (((k >> 3) & 1) << 1)) << 1; }

// One LDS-DMA piece through inline asm (see glds16 in gemm_fast.hip): for the builtin the compiler puts s_waitcnt vmcnt(0) in front of the
// wave's next LDS read, which is what a DOUBLE-BUFFERED loop must not have (the next tile's pieces are meant to stay in flight).  Only the
// kernels whose waits are hand-counted for that use it; the single-buffered ones keep the builtin.
__device__ __forceinline__ void glds16_asm(const void* g, const char* lds_uniform) {
  const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)lds_uniform);  // generic LDS pointer: low half = offset
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(l) : "memory");
}
// [rows][64] bf16 image, 128-B rows, 16-B chunk ^= key_d(row); global rows clamped to [0, nrows-1]
// KEEP_LAST: image row ROWS-1 is not written (the lanes that would are switched off): it holds something the caller put there once
template <int ROWS, bool ASM = false, bool KEEP_LAST = false>
__device__ __forceinline__ void load_rows(char* s, const bf16_t* g, long ld, int row0, int nrows, int w, int lane) {
#pragma unroll
  for (int i = 0; i < ROWS / 32; ++i) {
    const int q = w * (ROWS / 32) + i;
    const int row = q * 8 + (lane >> 3), p = lane & 7;
    const int gr = min(max(row0 + row, 0), nrows - 1);
    const bf16_t* src = g + (long)gr * ld + ((p ^ key_d(row)) << 3);
    if (KEEP_LAST && row == ROWS - 1) continue;
    if constexpr (ASM) glds16_asm(src, s + __builtin_amdgcn_readfirstlane(q * 1024));
    else __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(s + __builtin_amdgcn_readfirstlane(q * 1024)), 16, 0, 0);
  }
}
// V block as [64 k=j][64 n=dh] "trans" image (128-B k-rows, chunk ^= key_t64(k)); k rows clamped to nrows-1
template <bool ASM = false>
__device__ __forceinline__ void load_v(char* s, const bf16_t* g, long ld, int j0, int nrows, int w, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = w * 2 + i;
    const int k = q * 8 + (lane >> 3), p = lane & 7;
    const int gr = min(j0 + k, nrows - 1);
    const bf16_t* src = g + (long)gr * ld + ((p ^ key_t64(k)) << 3);
    if constexpr (ASM) glds16_asm(src, s + __builtin_amdgcn_readfirstlane(q * 1024));
    else __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(s + __builtin_amdgcn_readfirstlane(q * 1024)), 16, 0, 0);
  }
}
__device__ __forceinline__ short8_t frag_rows(const char* s, int row, int c) {
  return *reinterpret_cast<const short8_t*>(s + row * 128 + ((c ^ key_d(row)) << 4));
}
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


// transposed fragment (k = image row) of a [64 rows][64] image swizzled with key_d (the row-major images above)
__device__ __forceinline__ short8_t frag_kt(const char* s, int nbase, int kbase, int r) {
  const int col = nbase + ((r & 3) << 2);
  const int chunk = col >> 3, half = (col >> 2) & 1;
  const int k0 = kbase + (r >> 2), k1 = k0 + 4;
  const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4_t*)(s + k0 * 128 + ((chunk ^ key_d(k0)) << 4) + half * 8));
  const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4_t*)(s + k1 * 128 + ((chunk ^ key_d(k1)) << 4) + half * 8));
  short8_t v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return v;
}

// (q + bias) rounded to bf16, as an MFMA A fragment: lane (r = row, g = k group) holds 8 consecutive k
__device__ __forceinline__ short8_t q_frag(const bf16_t* qrow, const float* bias, int k0) {
  float x[8];
  ld8(qrow + k0, x);
  short8_t f;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (short)f32_to_bf16(x[e] + bias[k0 + e]);
  return f;
}

// Workgroup -> (sample, head, 64-row block) for the kernels whose grid is (blocks, H, B).  The hardware deals consecutive workgroup ids
// round-robin over the 8 XCDs (own L2 each) and starts them in id order.  (i) Every block of one (sample, head) goes to ONE XCD, so its
// K / V / position window - re-read by every block - are fetched into one L2, not eight; (ii) ids are block-major inside an XCD: the
// low blocks of every sample (always real frames) start first and the high ones - padding for most samples, a fraction of the work -
// fill the tail, instead of a long-running block starting last.  Launch with a 1-D grid of attn_grid_size() workgroups.
struct BlockId { int b, h, blk; bool ok; };
// BLK_MAJOR = false (key-side backward: every workgroup of a sample runs equally long): the blocks of one (sample, head) are consecutive
// in their XCD's order instead, so they are also resident at the same TIME and share the query-side tiles they all walk.
// `lin`: the workgroup's id inside its role's range (the whole grid for the one-role kernels; the merged backward launch passes
// blockIdx.x minus the start of the role's range, a multiple of 8: lin & 7 stays the XCD).
template <bool BLK_MAJOR = true>
__device__ __forceinline__ BlockId attn_block_id(int B, int H, int nblk, int lin) {
  const int xcd = lin & 7, slot = lin >> 3;
  const int nbh = B * H, per = (nbh + 7) >> 3;
  const int blk = BLK_MAJOR ? slot / per : slot % nblk;
  const int bh = (BLK_MAJOR ? slot - blk * per : slot / nblk) * 8 + xcd;
  BlockId id;
  id.ok = bh < nbh && blk < nblk;
  id.b = bh / H; id.h = bh - id.b * H; id.blk = blk;
  return id;
}
template <bool BLK_MAJOR = true>
__device__ __forceinline__ BlockId attn_block_id(int B, int H, int nblk) { return attn_block_id<BLK_MAJOR>(B, H, nblk, (int)blockIdx.x); }
inline unsigned attn_grid_size(int B, int H, int nblk) { return (unsigned)(8 * ((B * H + 7) / 8) * nblk); }

// streaming window of query i (compute_streaming_mask, multihead_attention.py:104-143): keys [lo, hi) are visible; outside it the
// reference's score is -1e9 = probability exactly 0.  chunk <= 0: the whole utterance.  hist < 0: unlimited history.
__device__ __forceinline__ void stream_window(int i, int T, int chunk, int hist, int& lo, int& hi) {
  const int index = (i / chunk) * chunk;
  lo = hist < 0 ? 0 : max(0, index - hist);
  hi = min(T, index + chunk);
}



// ---------------------------------------------------------------------------------------------------------------------------------
// Forward, TRANSPOSED orientation (round 4): the scores are computed as S^T = K (Q+u)^T (rows = keys, columns = this wave's 16 query
// rows), so that in the MFMA C layout a lane owns ONE query row: the online-softmax state (running maximum, running sum, rescale factor)
// is a per-lane scalar, the row reductions are in-lane over the lane's 16 keys plus two cross-row-group shuffles (they were eight 4-step
// DPP chains), and P^T in C layout IS the B operand of O^T += V^T P^T - the probabilities never go through LDS (the row-oriented kernel
// writes a bf16 P image with 16 two-byte LDS stores per lane and reads it back as A fragments).  For that the key rows of a 32-key
// group are dealt to the two 16-row MFMA tiles so that a lane's eight probabilities of the group are eight CONSECUTIVE keys
// (tile 2q: keys 32q + 8g + e, tile 2q+1: keys 32q + 8g + 4 + e) = the k order of the V^T fragment (frag_v).  The window scores are
// G^T = window (Q+v)^T: a lane holds four consecutive window columns of its query row and stores them with one 16-byte LDS write
// (four 4-byte ones before); the skewed read-back (column 15 - il + jl of the wave's strip) is four consecutive floats per tile.
// Same LDS budget as the row-oriented kernel (three workgroups per CU).
// ---------------------------------------------------------------------------------------------------------------------------------
// LDS is allocated in 1280-byte granules on gfx950 (160 KB = 128 granules): THREE workgroups per CU need <= 42 granules = 53 760 bytes
// each.  Strip = [16 il][80 window columns] f32 + the 16 bias-row scores behind it = 5 184 bytes per wave, 53 504 per workgroup (with a
// row stride of 84 floats it was 54 272 -> 43 granules -> two workgroups per CU: 90 instead of 62 us at T' = 743).
constexpr int GLDT = 80, SGTT_BYTES = 16 * GLDT * 4 + 64;
// Strip column swizzle: the 16-byte chunk (4 window columns) of row il is stored at chunk ^ ((il >> 1) & 3).  With a row stride of 80 floats
// (what three workgroups per CU leave room for) the rows il and il + 2 start 160 dwords = 0 banks (mod 32) apart, so the eight lanes of a
// ds_write_b128 service group - eight rows, the same chunk - hit four banks-of-four twice over: 4-way conflicts on the five G^T writes of
// every key block, 0.41 of the forward's LDS cycles (profiles/r06_lds_conflicts.txt).  The key keeps a chunk inside its aligned group of
// four (20 chunks per row) and spreads the eight rows over all 32 banks (bank model of the guide, tools/hwprobe/lds_sim.py).
__device__ __forceinline__ int strip_col(int il, int x) { return (((x >> 2) ^ ((il >> 1) & 3)) << 2) | (x & 3); }
constexpr int SMEM_FWDT = SK_BYTES + SV_BYTES + SP_BYTES + 4 * SGTT_BYTES;
static_assert((SMEM_FWDT + 1279) / 1280 * 3 <= 128, "three workgroups per CU");

template <bool STREAM>
__global__ __launch_bounds__(256, 3) void relattn_fused_fwdT_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ ubias, const float* __restrict__ vbias,
    const bf16_t* __restrict__ pext, const int32_t* __restrict__ lengths, bf16_t* __restrict__ out, float* __restrict__ lse_out,
    int B, int H, int T, float scale, int use_mask, int chunk, int hist) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = sK + SK_BYTES;
  char* sP = sV + SV_BYTES;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* sG = reinterpret_cast<float*>(sP + SP_BYTES + w * SGTT_BYTES);  // [16 il][80]: window columns 48-16w .. 127-16w; then [16] bias-row scores
  float* sGb = sG + 16 * GLDT;
  const int r = lane & 15, g = lane >> 4;
  const BlockId bid = attn_block_id(B, H, (T + BI - 1) / BI);
  if (!bid.ok) return;
  const int b = bid.b, h = bid.h, i0 = bid.blk * BI;
  const int HD = H * DH, LDQ = 3 * HD, R1 = 2 * T;
  const int len = lengths ? min(lengths[b], T) : T;
  const int shift = T - len;
  const bf16_t* qb = qkv + (long)b * T * LDQ + h * DH;
  const bf16_t* kb = qb + HD;
  const bf16_t* vb = qb + 2 * HD;
  const bf16_t* pb = pext + h * DH;
  uint4 bias_row = make_uint4(0, 0, 0, 0);
  if ((threadIdx.x >> 6) == 0 && (threadIdx.x & 63) < 8) bias_row = *reinterpret_cast<const uint4*>(pb + (long)(2 * T - 1) * HD + (((threadIdx.x & 63) ^ key_d(127)) << 3));

  // this lane's query row (B operand column): Q + u, Q + v
  const int i = i0 + w * 16 + r, irow = min(i, T - 1);
  short8_t bqu[2], bqv[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    bqu[kk] = q_frag(qb + (long)irow * LDQ, ubias + h * DH, kk * 32 + g * 8);
    bqv[kk] = q_frag(qb + (long)irow * LDQ, vbias + h * DH, kk * 32 + g * 8);
  }
  float m_run = -INFINITY, l_run = 0.f;
  float4_t acc_o[4];  // O^T: rows = head dims n*16 + g*4 + e, column = this lane's query
#pragma unroll
  for (int n = 0; n < 4; ++n) acc_o[n] = float4_t{0.f, 0.f, 0.f, 0.f};

  const float scale2 = scale * 1.4426950408889634f;
  const int lim = 2 * len - 1;
  const bool qm = use_mask && (i >= len);
  const int jthr = lim - (T - 1 - i);  // keys j < jthr: relative position T-1-i+j inside the sample's 2 len - 1 encodings
  int klo = 0, khi = T;  // visible keys of this query row
  if constexpr (STREAM) { if (!qm) stream_window(min(i, T - 1), T, chunk, hist, klo, khi); }
  const float scale2q = qm ? 0.f : scale2;
  int jl0[4], krow[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    jl0[jt] = 32 * (jt >> 1) + g * 8 + (jt & 1) * 4;                      // first of this lane's four keys of tile jt (C rows g*4 + e)
    krow[jt] = 32 * (jt >> 1) + (r >> 2) * 8 + (jt & 1) * 4 + (r & 3);  // key row that is MFMA row r of tile jt (A operand)
  }
  int goff[4][4];  // strip offset of this lane's skewed score of key jl0[jt] + e: row il = r, window column 15 - r + jl (swizzled)
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int e = 0; e < 4; ++e) goff[jt][e] = r * GLDT + strip_col(r, 15 - r + jl0[jt] + e);
#ifdef TFASR_ATTN_TIMING
  long long ph[5] = {0, 0, 0, 0, 0};
#endif
  const int njb = (T + BJ - 1) / BJ;
  int jb_lo = 0, jb_hi = njb;
  if constexpr (STREAM) {
    if (!(use_mask && i0 + BI > len)) {
      int lo, hi, lo2, hi2;
      stream_window(i0, T, chunk, hist, lo, hi);
      stream_window(min(i0 + BI - 1, T - 1), T, chunk, hist, lo2, hi2);
      jb_lo = lo / BJ;
      jb_hi = (hi2 + BJ - 1) / BJ;
    }
  }
  // window row 127 <- the bias row R of the position table (the block loop's DMA leaves that row alone), and from it the bias-row score of
  // this lane's query, (q_i + v) . pext[R]: the same for every key block, so it is formed once - the product of window rows 112..127 with
  // the query fragments the loop used to repeat per key block (row 15 of it; the other rows are not loaded yet and are kept out)
  if (w == 0 && lane < 8) *reinterpret_cast<uint4*>(sP + 127 * 128 + lane * 16) = bias_row;
  __syncthreads();
  float gbias;
  {
    float4_t a = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      short8_t f = frag_rows(sP, 112 + r, kk * 4 + g);
      if (r != 15) f = short8_t{0, 0, 0, 0, 0, 0, 0, 0};
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, bqv[kk], a, 0, 0, 0);
    }
    if (g == 3) sGb[r] = a[3];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gbias = sGb[r];
    asm volatile("" : "+v"(gbias));
  }
  if (use_mask && i0 >= len) {
    // every query row of this block is padding: uniform attention over ALL T keys (see relattn_fused_fwd_kernel): out = mean_j v_j, lse = log T
    for (int jb = 0; jb < njb; ++jb) {
      const int j0 = jb * BJ;
      load_v(sV, vb, LDQ, j0, T, w, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        short8_t pf;
#pragma unroll
        for (int t = 0; t < 8; ++t) pf[t] = (j0 + 32 * q + g * 8 + t < T) ? (short)0x3F80 : (short)0;
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_v(sV, n * 16, q * 32 + g * 8, r), pf, acc_o[n], 0, 0, 0);
      }
      __syncthreads();
    }
    m_run = 0.f; l_run = (float)T;
  } else {
  // The loop is software pipelined without a second set of tiles: K and the window are dead behind the score products, V until the last
  // products.  So K / window of block jb+1 are fetched behind a barrier in the middle of block jb (under the softmax and the P V products),
  // V of block jb behind the barrier that opens it (under the score products): every DMA has half an iteration to land, three barriers
  // per key block instead of two, the same 53.5 KB.  (The DMA pieces go through inline asm: the compiler does not see them and places no
  // vmcnt wait of its own; the hand-counted ones below are 2 K + 4 window pieces per wave behind the 2 V pieces.)
  if (jb_lo < jb_hi) {
    load_rows<BJ, true>(sK, kb, LDQ, jb_lo * BJ, T, w, lane);
    load_rows<WIN, true, true>(sP, pb, HD, (T - 1 - (i0 + BI - 1) + jb_lo * BJ) + shift, R1, w, lane);
  }
  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    const int j0 = jb * BJ;
#ifdef TFASR_ATTN_TIMING
    long long tp = __builtin_readcyclecounter();
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // K and the window of this block
    __builtin_amdgcn_s_barrier();                       // ... of every wave; every wave is done with the last block's V
    load_v<true>(sV, vb, LDQ, j0, T, w, lane);
    ATT_TICK(0)

    // content scores, transposed: tile jt = 16 keys x this wave's 16 queries
    float4_t acc_s[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      acc_s[jt] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        acc_s[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(sK, krow[jt], kk * 4 + g), bqu[kk], acc_s[jt], 0, 0, 0);
    }
    // window scores, transposed: G^T[c][il] for the 80 window columns 48-16w .. 127-16w this wave's skew reads: five 16-row tiles from
    // window row 48-16w on (straight-line code: only the row offset depends on the wave)
    {
      const int grow = (3 - w) * 16 + r;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        float4_t a = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(sP, grow + t * 16, kk * 4 + g), bqv[kk], a, 0, 0, 0);
        *reinterpret_cast<float4_t*>(sG + r * GLDT + strip_col(r, t * 16 + g * 4)) = a;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();   // every wave has read K and the window: the next block's may land
    if (jb + 1 < jb_hi) {
      load_rows<BJ, true>(sK, kb, LDQ, j0 + BJ, T, w, lane);
      load_rows<WIN, true, true>(sP, pb, HD, (T - 1 - (i0 + BI - 1) + j0 + BJ) + shift, R1, w, lane);
    }
    ATT_TICK(1)

    // every skewed score is read unconditionally (the strip column 15 - il + jl exists for every key of the block), THEN selected against
    // the bias score: a conditional read compiles to an exec-mask branch per element
    float4_t gv[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[jt][e] = sG[goff[jt][e]];
    // t = content + position score, UNSCALED (the softmax scale is positive: the maximum commutes with it, and the exponent below is one
    // fused multiply-add per element).  The common key block - every key inside the sample's relative positions for every query of the
    // wave - needs no select against the bias score (wave-uniform ballot, as in the query-side backward)
    const int trb = jthr - j0;  // keys jl < trb of this block have a relative position inside the table
    if (__builtin_amdgcn_ballot_w64(trb >= BJ) == ~0ull) {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) acc_s[jt] += gv[jt];
    } else {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int tr = trb - jl0[jt];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc_s[jt][e] += (e < tr) ? gv[jt][e] : gbias;
      }
    }
    const bool edge = STREAM || j0 + BJ > T;  // keys outside [klo, khi): past the end of a ragged last block / outside the streaming window
    float mx;
    if (edge) {
      mx = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = j0 + jl0[jt] + e;
          mx = fmaxf(mx, (j < klo || j >= khi) ? -INFINITY : acc_s[jt][e]);
        }
    } else {
      float m4[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) m4[jt] = fmaxf(fmaxf(acc_s[jt][0], acc_s[jt][1]), fmaxf(acc_s[jt][2], acc_s[jt][3]));
      mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    }
    mx = xor32_max(xor16_max(mx));
    // (scale2q = 0 for a padded query row: constant scores; its keys are finite, so 0 * mx = 0)
    const float m_new = fmaxf(m_run, mx == -INFINITY ? -INFINITY : mx * scale2q);
    const float m_ref = (STREAM && m_new == -INFINITY) ? 0.f : m_new;
    const float corr = __builtin_amdgcn_exp2f(m_run - m_ref);
    float rs = 0.f;
    short8_t pf[2];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      float p[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) p[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(acc_s[jt][e], scale2q, -m_ref));
      if (edge) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = j0 + jl0[jt] + e;
          if (j < klo || j >= khi) p[e] = 0.f;
        }
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
#pragma unroll
    for (int n = 0; n < 4; ++n) acc_o[n] *= corr;
    ATT_TICK(2)
    // this block's V (2 pieces per wave, issued in front of the 6 of the next block's K / window) has landed, for every wave
    if (jb + 1 < jb_hi) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // O^T += V^T P^T: the probabilities are the B operand straight from registers
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc_o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_v(sV, n * 16, q * 32 + g * 8, r), pf[q], acc_o[n], 0, 0, 0);
    ATT_TICK(3)
    ATT_TICK(4)
  }
  }
#ifdef TFASR_ATTN_TIMING
  if (threadIdx.x == 0) {
    long long* o = g_attn_timing + 5L * blockIdx.x;
    for (int k = 0; k < 5; ++k) o[k] = ph[k];
  }
#endif

  if (i < T) {
    const float inv = 1.f / l_run;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      uint2 v;
      v.x = pack2_bf16(acc_o[n][0] * inv, acc_o[n][1] * inv);
      v.y = pack2_bf16(acc_o[n][2] * inv, acc_o[n][3] * inv);
      *reinterpret_cast<uint2*>(out + ((long)b * T + i) * HD + h * DH + n * 16 + g * 4) = v;
    }
    if (g == 0) lse_out[((long)b * H + h) * T + i] = m_run * 0.6931471805599453f + logf(l_run);
  }
}

// ======================================================================================================================
// Backward, part 1 in TRANSPOSED orientation (round 5; the query-gradient kernel of the default route, tfasr_relattn_fused_bwd_q3).
// Everything is computed as in relattn_fused_fwdT_kernel: S^T = K (Q+u)^T, dP^T = V dO^T (rows = keys, dealt to the MFMA tiles so that a
// lane's eight values of a 32-key group are eight CONSECUTIVE keys; column = the lane's ONE query row), so
//   * the per-row quantities (lse_i, D_i, the bias-row share of the score gradient, the validity thresholds) are per-lane scalars;
//   * dS^T in the C layout IS the B operand of dq_u^T += K^T dS^T - the dS A-image of the row-oriented kernel (16 two-byte LDS stores and
//     two fragment reads per lane and key block) is gone, and the unskewed dS leaves for HBM as two 16-byte stores straight from registers;
//   * the window scores G^T are written with one 16-byte LDS store per tile and read back as four consecutive floats (they were 24 + 16
//     four-byte accesses); only the SKEWED score gradient (dq_v^T += window^T dG^T needs dS against the window column, not the key) still
//     goes through a per-wave LDS image, and that image lies over the dead G^T strip: 53.5 KB of LDS per workgroup instead of 65.
// Per lane and key block: ~34 LDS instructions instead of ~84 of the row-oriented kernel it replaced (rounds 2-4; profiles/r05_attention_backward_investigation.md).
// ======================================================================================================================
constexpr int QT_IMG_LD = 272;                       // byte stride of a row of the skewed dS image: 128 bf16 columns + 16 B (bank spread, no swizzle)
constexpr int QT_IMG_BYTES = 16 * QT_IMG_LD;
// PIPELINED: the K block and the window are double buffered and the next key block's DMA is issued behind the barrier that opens the current
// one (V, dead after the first products, is refetched behind a second barrier): 32 + 24 KB of tiles, the image over the wave's G^T strip
// (cleared per key block): 76.7 KB, two workgroups per CU.  The single-buffered and the lean three-per-CU builds measured slower (97 vs 82 us;
// profiles/r05_attention_backward_investigation.md) and are gone; MODE stays a template constant of the one build.
static_assert(QT_IMG_BYTES <= 16 * GLDT * 4, "the skewed dS image fits under the bias scores of the strip");
constexpr int qt_tile_bytes(int mode) { return (mode == 1 ? 2 : 1) * (SK_BYTES + SP_BYTES) + SV_BYTES; }
constexpr int qt_smem(int mode) { return qt_tile_bytes(mode) + 4 * SGTT_BYTES + (mode == 0 ? 4 * QT_IMG_BYTES : 0); }

__device__ __forceinline__ short8_t row_frag(const bf16_t* row, int k0) {
  return *reinterpret_cast<const short8_t*>(row + k0);
}

typedef float float2_t __attribute__((ext_vector_type(2)));

// The prologue arithmetic of one query row, shared by the query-side body and relattn_bwd_prep_kernel so that both give the same bits:
// the q + u / q + v / dO fragments of lane (r, g) (head dims kk*32 + g*8 .. +7) and its share of D_i = rowsum(dO * o) ...
__device__ __forceinline__ float qrow_frags(const bf16_t* qrow, const float* ub, const float* vb, const bf16_t* dorow, const bf16_t* orow, int g,
                                            short8_t (&bqu)[2], short8_t (&bqv)[2], short8_t (&bdo)[2]) {
  float dpart = 0.f;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    bqu[kk] = q_frag(qrow, ub, kk * 32 + g * 8);
    bqv[kk] = q_frag(qrow, vb, kk * 32 + g * 8);
    bdo[kk] = row_frag(dorow + kk * 32 + g * 8, 0);
    float a[8], c[8];
    ld8(dorow + kk * 32 + g * 8, a);
    ld8(orow + kk * 32 + g * 8, c);
#pragma unroll
    for (int e = 0; e < 8; ++e) dpart += a[e] * c[e];
  }
  return dpart;
}
// ... and its share of the bias-row score (q_i + v) . pext[R] (`prow`: the bias row of this head); the caller sums both over the four g lanes
__device__ __forceinline__ float qrow_bias_part(const short8_t (&bqv)[2], const bf16_t* prow, int g) {
  float part = 0.f;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    float pr[8];
    ld8(prow + kk * 32 + g * 8, pr);
#pragma unroll
    for (int t = 0; t < 8; ++t) part += bf16_to_f32((bf16_t)bqv[kk][t]) * pr[t];
  }
  return part;
}

// PRE (the merged launch, relattn_fused_bwd_qk_kernel): q + u, q + v and both planes of dvec were written by relattn_bwd_prep_kernel - the
// body READS them (the same bits it would have formed) instead of forming and writing them.  `lin`: see attn_block_id.
template <bool STREAM, int MODE, bool PRE>
__device__ __forceinline__ void relattn_bwd_qT_body(
    char* const smem, const int lin,
    const bf16_t* __restrict__ qkv, const float* __restrict__ ubias, const float* __restrict__ vbias,
    const bf16_t* __restrict__ pext, const int32_t* __restrict__ lengths, const bf16_t* __restrict__ o,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse, bf16_t* __restrict__ dq, bf16_t* __restrict__ dpos,
    float* __restrict__ dvec, int B, int H, int T, int ldp, float scale, int use_mask, float* __restrict__ dpext,
    long lddq, float* __restrict__ du, float* __restrict__ dv, int chunk, int hist, bf16_t* qu_out, bf16_t* qv_out) {
  constexpr bool QT_PIPE = MODE == 1, QT_LEAN = MODE == 2, QT_ALIAS = MODE != 0;
  constexpr int QT_TILE_BYTES = qt_tile_bytes(MODE);
  static_assert(!PRE || MODE == 1, "the reading mode exists for the pipelined build only");
  // K block [64 j][64 dh] row-major: rows = A operand of S^T, transposed = A operand of dq_u^T; V block: rows = A operand of dP^T;
  // window rows: rows = A operand of G^T, transposed = A operand of dq_v^T.  QT_PIPE: K and the window twice.
  char* const sK0 = smem;
  char* const sV = sK0 + (QT_PIPE ? 2 : 1) * SK_BYTES;
  char* const sP0 = sV + SV_BYTES;
  char* const sStrips = smem + QT_TILE_BYTES;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* sG = reinterpret_cast<float*>(sStrips + w * SGTT_BYTES);  // [16 il][80]: window columns 48-16w .. 127-16w; then [16] bias-row scores
  float* sGb = sG + 16 * GLDT;
  // skewed dS image [16 il][128 c] bf16 of this wave, rows QT_IMG_LD bytes apart.  Row il is WRITTEN at columns 63-16w-il .. 126-16w-il
  // whatever the key block, so it is cleared once: the cells outside that range stay zero, the ones inside are rewritten every block.
  char* sAg = QT_ALIAS ? reinterpret_cast<char*>(sG) : sStrips + 4 * SGTT_BYTES + w * QT_IMG_BYTES;
  const int r = lane & 15, g = lane >> 4;
  const BlockId bid = attn_block_id(B, H, (T + BI - 1) / BI, lin);
  if (!bid.ok) return;
  const int b = bid.b, h = bid.h, i0 = bid.blk * BI;
  const int HD = H * DH, LDQ = 3 * HD, R = 2 * T - 1, R1 = 2 * T;
  const int len = lengths ? min(lengths[b], T) : T;
  const int shift = T - len;
  const bf16_t* qb = qkv + (long)b * T * LDQ + h * DH;
  const bf16_t* kb = qb + HD;
  const bf16_t* vb = qb + 2 * HD;
  const bf16_t* pb = pext + h * DH;
  uint4 bias_row = make_uint4(0, 0, 0, 0);
  if (MODE == 0 && (threadIdx.x >> 6) == 0 && (threadIdx.x & 63) < 8) bias_row = *reinterpret_cast<const uint4*>(pb + (long)(2 * T - 1) * HD + (((threadIdx.x & 63) ^ key_d(127)) << 3));

  const int i = i0 + w * 16 + r;  // this lane's query row
  if (use_mask && i0 >= len) {
    // a block of padded query rows: constant scores, dS = 0, zero query gradient (see relattn_fused_bwd_q_kernel)
    if (i < T) {
#pragma unroll
      for (int n = 0; n < 4; ++n) *reinterpret_cast<uint2*>(dq + ((long)b * T + i) * lddq + h * DH + n * 16 + g * 4) = make_uint2(0u, 0u);
    }
    return;
  }
  const int irow = min(i, T - 1);
  short8_t bqu[2], bqv[2], bdo[2];
  float dpart = 0.f;
  if constexpr (PRE) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bqu[kk] = row_frag(qu_out + ((long)b * T + irow) * HD + h * DH, kk * 32 + g * 8);
      bqv[kk] = row_frag(qv_out + ((long)b * T + irow) * HD + h * DH, kk * 32 + g * 8);
      bdo[kk] = row_frag(dout + ((long)b * T + irow) * HD + h * DH, kk * 32 + g * 8);
    }
  } else {
    dpart = qrow_frags(qb + (long)irow * LDQ, ubias + h * DH, vbias + h * DH, dout + ((long)b * T + irow) * HD + h * DH,
                       o + ((long)b * T + irow) * HD + h * DH, g, bqu, bqv, bdo);
  }
  if (!PRE && qu_out && i < T) {  // q + u / q + v of this block's rows for the key-side and table-gradient kernels (the fragments ARE those rows)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      *reinterpret_cast<short8_t*>(qu_out + ((long)b * T + irow) * HD + h * DH + kk * 32 + g * 8) = bqu[kk];
      *reinterpret_cast<short8_t*>(qv_out + ((long)b * T + irow) * HD + h * DH + kk * 32 + g * 8) = bqv[kk];
    }
  }
  if constexpr (PRE) {
    dpart = dvec[((long)b * H + h) * T + irow];
  } else {
    dpart = xor32_sum(xor16_sum(dpart));  // D_i of this lane's query, in all four lanes of its column
    if (g == 0 && i < T) dvec[((long)b * H + h) * T + i] = dpart;
  }
  const float Di = dpart;
  const float scale2 = scale * 1.4426950408889634f;
  const float lse2 = lse[((long)b * H + h) * T + irow] * 1.4426950408889634f;
  const int lim = 2 * len - 1;
  const bool inrow = i < T;
  const bool live = inrow && !(use_mask && i >= len);
  const int jthr = lim - (T - 1 - i);  // keys j < jthr: relative position T-1-i+j inside the sample's 2 len - 1 encodings
  int klo = 0, khi = T;
  if constexpr (STREAM) { if (live) stream_window(i, T, chunk, hist, klo, khi); }
  if (!live) khi = 0;  // (no visible key: dS = 0 everywhere in this row)
  int jl0[4], krow[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    jl0[jt] = 32 * (jt >> 1) + g * 8 + (jt & 1) * 4;
    krow[jt] = 32 * (jt >> 1) + (r >> 2) * 8 + (jt & 1) * 4 + (r & 3);
  }
  int goff[4][4];  // strip offset of this lane's skewed score of key jl0[jt] + e (swizzled column, see strip_col)
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int e = 0; e < 4; ++e) goff[jt][e] = r * GLDT + strip_col(r, 15 - r + jl0[jt] + e);
  // image cell of this lane's key 8g of the block: window column 63-16w-r+8g; the keys of tile jt, element e are 32(jt>>1)+4(jt&1)+e further
  char* const img = sAg + r * QT_IMG_LD + (63 - w * 16 - r + g * 8) * 2;
  float4_t acc_q[4], acc_v[4];  // dq_u^T / dq_v^T: rows = head dims n*16 + g*4 + e, column = this lane's query
#pragma unroll
  for (int n = 0; n < 4; ++n) { acc_q[n] = float4_t{0.f, 0.f, 0.f, 0.f}; acc_v[n] = float4_t{0.f, 0.f, 0.f, 0.f}; }
  float bias_acc = 0.f;
  bf16_t* dsrow = dpos + (((long)b * H + h) * T + irow) * ldp;
  const int kk_lo = w < 2 ? 1 : 0;  // this wave's skew touches window columns 48-16w .. 126-16w: three of the four 32-column groups

  const int njb = (T + BJ - 1) / BJ;
  // the bias-row score of this lane's query, (q_i + v) . pext[R]: the same for every key block, so it is formed once
  float gbias;
  if constexpr (PRE) {
    gbias = dvec[(long)B * H * T + ((long)b * H + h) * T + irow];
  } else if constexpr (QT_PIPE || QT_LEAN) {
    // ... as a plain dot product from the fragments (head dims kk*32 + g*8 + t of this lane, the other three quarters in lanes r + 16 m)
    gbias = xor32_sum(xor16_sum(qrow_bias_part(bqv, pb + (long)R * HD, g)));
  } else {
    char* const sP = sP0;
    if (w == 0 && lane < 8) *reinterpret_cast<uint4*>(sP + 127 * 128 + lane * 16) = bias_row;  // window row 127 <- the bias row
    if constexpr (!QT_ALIAS) {
      const uint4 z4 = make_uint4(0, 0, 0, 0);
      for (int q = lane; q < QT_IMG_BYTES / 16; q += 64) *reinterpret_cast<uint4*>(sAg + q * 16) = z4;
    }
    __syncthreads();
    // (row 15 of the product of window rows 112..127 with the query fragments; the other fifteen rows are not loaded yet and not looked at)
    float4_t a = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      short8_t f = frag_rows(sP, 112 + r, kk * 4 + g);
      if (r != 15) f = short8_t{0, 0, 0, 0, 0, 0, 0, 0};  // (stale LDS may hold NaN patterns: keep them out of the product)
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, bqv[kk], a, 0, 0, 0);
    }
    if (g == 3) sGb[r] = a[3];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gbias = sGb[r];
  }
  if (!PRE && g == 0 && i < T) dvec[(long)B * H * T + ((long)b * H + h) * T + i] = gbias;  // second plane of dvec: for the key-side kernel
  const float Dis = Di * scale;
  // the bias row of the table (this lane's 16 head dims n*16 + g*4 + e) for the epilogue: requested here, so that the epilogue has no
  // global load of its own to wait for (every workgroup pays its prologue and epilogue latencies once, and a launch is two rounds of them)
  uint2 prb[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) prb[n] = *reinterpret_cast<const uint2*>(pb + (long)R * HD + n * 16 + g * 4);
  // LEAN: where this lane's three B fragments are read back from at the top of every key block (q + u / q + v: what this lane itself
  // stored above - the stores are complete before the first read; rows past T: zeros)
  const bf16_t* const fr_qu = qu_out + ((long)b * T + irow) * HD + h * DH + g * 8;
  const bf16_t* const fr_qv = qv_out + ((long)b * T + irow) * HD + h * DH + g * 8;
  const bf16_t* const fr_do = dout + ((long)b * T + irow) * HD + h * DH + g * 8;
  if constexpr (QT_LEAN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (QT_PIPE) {
    // every value the prologue loaded is in its register before the first DMA is issued: a compiler-placed s_waitcnt vmcnt(0) for one of
    // them inside the loop would also wait for the prefetch the loop keeps in flight
    float l2 = lse2, gb = gbias, ds_ = Dis;
    asm volatile("" : "+v"(l2), "+v"(gb), "+v"(ds_));
    (void)l2; (void)gb; (void)ds_;
    if constexpr (PRE) {  // (here the fragments are plain loads, first used inside the loop: the same holds for them)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) asm volatile("" : "+v"(bqu[kk]), "+v"(bqv[kk]), "+v"(bdo[kk]));
    }
  }
#ifdef TFASR_ATTN_TIMING
  long long ph[5] = {0, 0, 0, 0, 0};
  const long long t_begin = __builtin_readcyclecounter();
#endif
  for (int jb = 0; jb < njb; ++jb) {
    const int j0 = jb * BJ;
    const int pw0 = (T - 1 - (i0 + BI - 1) + j0) + shift;
#ifdef TFASR_ATTN_TIMING
    long long tp = __builtin_readcyclecounter();
#endif
    char* sK = sK0;
    char* sP = sP0;
    if constexpr (QT_PIPE) {
      sK = sK0 + (jb & 1) * SK_BYTES;
      sP = sP0 + (jb & 1) * SP_BYTES;
      if (jb == 0) {
        load_rows<BJ, true>(sK, kb, LDQ, 0, T, w, lane);
        load_rows<BJ, true>(sV, vb, LDQ, 0, T, w, lane);
        load_rows<WIN, true>(sP, pb, HD, pw0, R1, w, lane);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this block's tiles (issued one block ago) and the last block's dS stores
      __builtin_amdgcn_s_barrier();                       // ... of every wave; every wave is also done with the other K / window buffer
      if (jb + 1 < njb) {
        load_rows<BJ, true>(sK0 + ((jb + 1) & 1) * SK_BYTES, kb, LDQ, j0 + BJ, T, w, lane);
        load_rows<WIN, true>(sP0 + ((jb + 1) & 1) * SP_BYTES, pb, HD, pw0 + BJ, R1, w, lane);
      }
    } else {
      if constexpr (QT_LEAN) {
        const short8_t z8 = short8_t{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          bqu[kk] = inrow ? *reinterpret_cast<const short8_t*>(fr_qu + kk * 32) : z8;
          bqv[kk] = inrow ? *reinterpret_cast<const short8_t*>(fr_qv + kk * 32) : z8;
          bdo[kk] = inrow ? *reinterpret_cast<const short8_t*>(fr_do + kk * 32) : z8;
        }
      }
      load_rows<BJ>(sK, kb, LDQ, j0, T, w, lane);
      load_rows<BJ>(sV, vb, LDQ, j0, T, w, lane);
      load_rows<WIN, false, MODE == 0>(sP, pb, HD, pw0, R1, w, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    ATT_TICK(0)

    float4_t acc_s[4], acc_p[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      acc_s[jt] = float4_t{0.f, 0.f, 0.f, 0.f};
      acc_p[jt] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        acc_s[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(sK, krow[jt], kk * 4 + g), bqu[kk], acc_s[jt], 0, 0, 0);
        acc_p[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(sV, krow[jt], kk * 4 + g), bdo[kk], acc_p[jt], 0, 0, 0);
      }
    }
    // window scores, transposed: G^T[c][il] for the 80 window columns 48-16w .. 127-16w this wave's skew reads (five 16-row tiles from
    // window row 48-16w on: straight-line code, nothing depends on the wave but the row offset)
    {
      const int grow = (3 - w) * 16 + r;
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        float4_t a = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(sP, grow + t * 16, kk * 4 + g), bqv[kk], a, 0, 0, 0);
        *reinterpret_cast<float4_t*>(sG + r * GLDT + strip_col(r, t * 16 + g * 4)) = a;
      }
    }
    if constexpr (QT_PIPE) {
      // V is dead for every wave behind this barrier: fetch the next block's
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (jb + 1 < njb) load_rows<BJ, true>(sV, vb, LDQ, j0 + BJ, T, w, lane);
    }
    // (no waits between the wave's own LDS writes and reads from here to the closing barrier: one wave's LDS operations execute in
    // order, and the compiler counts the returns it needs - explicit lgkmcnt(0) fences here cost 3 exposed LDS round trips per key block)
    ATT_TICK(1)
    float gv[4][4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[jt][e] = sG[goff[jt][e]];
    if constexpr (QT_ALIAS) {  // every score of the strip is in registers: clear the image that lies over it (4352 B = 4.25 x 64 lanes x 16 B)
      const uint4 z4 = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<uint4*>(sAg + (q * 64 + lane) * 16) = z4;
      if (lane < 16) *reinterpret_cast<uint4*>(sAg + (256 + lane) * 16) = z4;
    }
    // dS^T in C layout (rows = this lane's keys jl0[jt] + e, column = its query)
    short8_t pd[2];   // B fragments of dq_u^T: every visible pair
    uint4 pz[2];      // the same with the pairs outside the sample's relative positions zeroed (their gradient goes to the bias row)
    const int jhi = min(khi, T) - j0, jlo = klo - j0;  // visible keys of this row, block-relative
    const int trb = jthr - j0;                          // keys jl < trb of this block have a relative position inside the table
    // the common key block - every key of it visible to and inside the table for every query of the wave - needs none of the selects
    const bool plain = __builtin_amdgcn_ballot_w64(trb >= BJ && jlo <= 0 && jhi >= BJ) == ~0ull;
    if (plain) {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        uint32_t pk[2];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          const float2_t sc = float2_t{acc_s[jt][2 * h2], acc_s[jt][2 * h2 + 1]} + float2_t{gv[jt][2 * h2], gv[jt][2 * h2 + 1]};
          const float2_t ex = sc * scale2 - lse2;
          const float2_t pp = float2_t{__builtin_amdgcn_exp2f(ex[0]), __builtin_amdgcn_exp2f(ex[1])};
          const float2_t d2 = pp * (float2_t{acc_p[jt][2 * h2], acc_p[jt][2 * h2 + 1]} * scale - Dis);
          pk[h2] = pack2_bf16(d2[0], d2[1]);
        }
        const int o4 = (jt & 1) * 4;
        pd[jt >> 1][o4 + 0] = (short)(pk[0] & 0xffffu); pd[jt >> 1][o4 + 1] = (short)(pk[0] >> 16);
        pd[jt >> 1][o4 + 2] = (short)(pk[1] & 0xffffu); pd[jt >> 1][o4 + 3] = (short)(pk[1] >> 16);
        if (jt & 1) { pz[jt >> 1].z = pk[0]; pz[jt >> 1].w = pk[1]; } else { pz[jt >> 1].x = pk[0]; pz[jt >> 1].y = pk[1]; }
        char* const cell = img + (32 * (jt >> 1) + 4 * (jt & 1)) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) *reinterpret_cast<bf16_t*>(cell + e * 2) = (bf16_t)((pk[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
      }
    } else {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int tr = trb - jl0[jt];  // keys e < tr of this tile have a relative position inside the table
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int jl = jl0[jt] + e;
          const float pos = (e < tr) ? gv[jt][e] : gbias;
          const float p = __builtin_amdgcn_exp2f((acc_s[jt][e] + pos) * scale2 - lse2);
          const bool vis = jl >= jlo && jl < jhi;
          d[e] = vis ? p * (acc_p[jt][e] * scale - Dis) : 0.f;
          if (e >= tr) bias_acc += d[e];  // (d = 0 for pairs that do not exist / are not visible)
        }
        const uint32_t lo = pack2_bf16(d[0], d[1]), hi = pack2_bf16(d[2], d[3]);
        const uint32_t lz = pack2_bf16(0 < tr ? d[0] : 0.f, 1 < tr ? d[1] : 0.f), hz = pack2_bf16(2 < tr ? d[2] : 0.f, 3 < tr ? d[3] : 0.f);
        const int o4 = (jt & 1) * 4;
        pd[jt >> 1][o4 + 0] = (short)(lo & 0xffffu); pd[jt >> 1][o4 + 1] = (short)(lo >> 16);
        pd[jt >> 1][o4 + 2] = (short)(hi & 0xffffu); pd[jt >> 1][o4 + 3] = (short)(hi >> 16);
        if (jt & 1) { pz[jt >> 1].z = lz; pz[jt >> 1].w = hz; } else { pz[jt >> 1].x = lz; pz[jt >> 1].y = hz; }
        const uint32_t zz[2] = {lz, hz};
        char* const cell = img + (32 * (jt >> 1) + 4 * (jt & 1)) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) *reinterpret_cast<bf16_t*>(cell + e * 2) = (bf16_t)((zz[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
      }
    }
    // unskewed dS -> HBM straight from registers: 8 consecutive keys per 32-key group
    if (inrow) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int jc = j0 + 32 * q + g * 8;
#if !defined(TFASR_QT_NT) || TFASR_QT_NT
        // (non-temporal: 73 MB per launch that this kernel never reads again should not push K / V / window lines out of the L2;
        // 84.1 -> 82.4 us same box; -DTFASR_QT_NT=0: plain stores)
        if (jc < ldp) {
          typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
          const u32x4_t v = {pz[q].x, pz[q].y, pz[q].z, pz[q].w};
          __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t*>(dsrow + jc));
        }
#else
        if (jc < ldp) *reinterpret_cast<uint4*>(dsrow + jc) = pz[q];
#endif
      }
    }
    ATT_TICK(2)
    // dq_u^T += K^T dS^T (A: the K block read transposed, k = key; B: dS^T from registers)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc_q[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kt(sK, n * 16, q * 32 + g * 8, r), pd[q], acc_q[n], 0, 0, 0);
    // dq_v^T += window^T dG^T (A: the window rows read transposed, k = window column; B: the skewed image, k = window column)
#pragma unroll
    for (int k3 = 0; k3 < 3; ++k3) {
      const int kk = kk_lo + k3;
      const short8_t bfr = *reinterpret_cast<const short8_t*>(sAg + r * QT_IMG_LD + (kk * 4 + g) * 16);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc_v[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kt(sP, n * 16, kk * 32 + g * 8, r), bfr, acc_v[n], 0, 0, 0);
    }
    ATT_TICK(3)
    if constexpr (!QT_PIPE) __syncthreads();  // everyone is done with sK / sV / sP (and this wave with its strip) before the next block's DMA lands
    ATT_TICK(4)
  }
#ifdef TFASR_ATTN_TIMING
  const long long t_loop = __builtin_readcyclecounter();
#endif

  // epilogue: dq = dq_u + dq_v (+ the bias row's share), du / dv column sums, the bias row of the table gradient
  if constexpr (QT_LEAN) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) bqv[kk] = *reinterpret_cast<const short8_t*>(fr_qv + kk * 32);
  }
  float bsum = bias_acc;
  bsum = xor32_sum(xor16_sum(bsum));
  float su[4][4], sv[4][4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const uint2 pr = prb[n];  // the bias row of the table, this lane's 4 head dims
    const float pbias[4] = {__uint_as_float(pr.x << 16), __uint_as_float(pr.x & 0xffff0000u), __uint_as_float(pr.y << 16), __uint_as_float(pr.y & 0xffff0000u)};
    float gq[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gqv = acc_v[n][e] + bsum * pbias[e];
      gq[e] = acc_q[n][e] + gqv;
      su[n][e] = inrow ? acc_q[n][e] : 0.f;
      sv[n][e] = inrow ? gqv : 0.f;
    }
    if (inrow) {
      uint2 v;
      v.x = pack2_bf16(gq[0], gq[1]);
      v.y = pack2_bf16(gq[2], gq[3]);
      *reinterpret_cast<uint2*>(dq + ((long)b * T + i) * lddq + h * DH + n * 16 + g * 4) = v;
    }
  }
  // three column sums over the block's 64 rows: du = colsum(dq_u), dv = colsum(dq_v), and the bias row of the table gradient
  // dpext[R] += sum_i bsum_i (q_i + v).  Over the 16 queries of a wave by DPP, over the 4 waves through LDS (the staged tiles are dead),
  // then ONE 64-lane atomic instruction per sum and workgroup: the bias-row sum used to leave every wave as 16 four-lane atomics, and
  // those ~50 k requests per launch onto the same eight cache lines serialised in the L2 for ~110 us - longer than the key loop.
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);  // [4 waves][3][64]
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = row16_sum(su[n][e]), c = row16_sum(sv[n][e]);
      if (r == 0) { red[(w * 3 + 0) * 64 + n * 16 + g * 4 + e] = a; red[(w * 3 + 1) * 64 + n * 16 + g * 4 + e] = c; }
    }
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int t = 0; t < 8; ++t) {  // in the B-fragment indexing of bqv: head dim kk*32 + g*8 + t
      float v = inrow ? bsum * bf16_to_f32((bf16_t)bqv[kk][t]) : 0.f;
      v = row16_sum(v);
      if (r == 0) red[(w * 3 + 2) * 64 + kk * 32 + g * 8 + t] = v;
    }
  __syncthreads();
  if (threadIdx.x < 192) {
    const int which = threadIdx.x >> 6, col = threadIdx.x & 63;
    const float v = red[(0 * 3 + which) * 64 + col] + red[(1 * 3 + which) * 64 + col] + red[(2 * 3 + which) * 64 + col] + red[(3 * 3 + which) * 64 + col];
    float* dst = which == 0 ? du + h * DH : which == 1 ? dv + h * DH : dpext + (long)R * HD + h * DH;
    if (which < 2 || v != 0.f) atomicAdd(dst + col, v);
  }
#ifdef TFASR_ATTN_TIMING
  if (threadIdx.x == 0 && blockIdx.x < 8192) {  // [5 phase sums of wave 0][loop][epilogue][key blocks]
    long long* o = g_attn_timing + 8L * blockIdx.x;
    for (int kq = 0; kq < 5; ++kq) o[kq] = ph[kq];
    o[5] = t_loop - t_begin; o[6] = __builtin_readcyclecounter() - t_loop; o[7] = njb;
  }
#endif
}

template <bool STREAM, int MODE>
__global__ __launch_bounds__(256, MODE == 2 ? 3 : 2) void relattn_fused_bwd_qT_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ ubias, const float* __restrict__ vbias,
    const bf16_t* __restrict__ pext, const int32_t* __restrict__ lengths, const bf16_t* __restrict__ o,
    const bf16_t* __restrict__ dout, const float* __restrict__ lse, bf16_t* __restrict__ dq, bf16_t* __restrict__ dpos,
    float* __restrict__ dvec, int B, int H, int T, int ldp, float scale, int use_mask, float* __restrict__ dpext,
    long lddq, float* __restrict__ du, float* __restrict__ dv, int chunk, int hist, bf16_t* qu_out, bf16_t* qv_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  relattn_bwd_qT_body<STREAM, MODE, false>(smem, (int)blockIdx.x, qkv, ubias, vbias, pext, lengths, o, dout, lse, dq, dpos, dvec, B, H, T, ldp, scale,
                                           use_mask, dpext, lddq, du, dv, chunk, hist, qu_out, qv_out);
}


// Backward, part 3 (V2): the gradient of the projected position table,
//   dpext[c, :] += sum_b sum_i dS_b[i, j(i,c)] * (q_i + v),     j(i,c) = (c - shift_b) - (T-1-i),   valid iff 0 <= c - shift_b < 2 len_b - 1
// read from the UNSKEWED dS [B,H,T,lds].  Block = (128 table rows, head, group of samples); the 4 waves own 2 of the 8 16-row tiles
// each and keep them in registers over every sample of the group and every 64-query block that can reach them, so dpext receives
// one f32 atomic per (table row, column, group) instead of one per (sample, query block) pair.  The MFMA A operand (rows = c, k = i)
// is the diagonal of the raw dS tile: element (il, c) sits at column (c - shift - T + 1 + i0 + il) of row il.
// ======================================================================================================================
constexpr int DPX_TLD = 208;                              // raw tile row stride in elements (192 columns + alignment slack)
constexpr int DPX_CHUNKS = 64 * (DPX_TLD / 8);            // 1664 16-B chunks
constexpr int DPX_TILE_BYTES = 7 * 256 * 16;              // 7 DMA instructions per wave (the tail lanes land in the slack)
constexpr int DPX_BUF = DPX_TILE_BYTES + SK_BYTES;        // raw dS tile + (q+v) block
constexpr int SMEM_DPX = 2 * DPX_BUF;                     // double buffered

__global__ __launch_bounds__(256, 2) void relattn_dpext_kernel(
    const bf16_t* __restrict__ ds, const bf16_t* __restrict__ qv, const int32_t* __restrict__ lengths, float* __restrict__ dpext,
    int B, int H, int T, int lds, int use_mask, int bchunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * 128, h = blockIdx.y;
  const int HD = H * DH, R = 2 * T - 1;
  const int b_lo = blockIdx.z * bchunk, b_hi = min(B, b_lo + bchunk);
  float4_t acc[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[ct][n] = float4_t{0.f, 0.f, 0.f, 0.f};
  const int nib = (T + BI - 1) / BI;

  // (sample, 64-query block) tiles that can reach this block's table rows, in order; `it` = b * nib + ib (uniform over the block)
  struct Tl { int b, i0, shift, lim, jmin, jb0; };
  auto tile_at = [&](int it, Tl& t) -> bool {
    const int b = b_lo + it / nib, ib = it % nib;
    const int len = lengths ? min(lengths[b], T) : T;
    t.b = b; t.i0 = ib * BI; t.shift = T - len; t.lim = 2 * len - 1;
    if (c0 + 128 <= t.shift || c0 >= t.shift + t.lim) return false;   // no valid table row of this sample in the block
    if (use_mask && t.i0 >= len) return false;                          // masked query rows carry dS = 0
    t.jmin = c0 - t.shift - T + 1 + t.i0;                                // key index of (il = 0, c = c0); (il, c) -> jmin + (c - c0) + il
    if (t.jmin + 127 + 63 < 0 || t.jmin >= T) return false;
    t.jb0 = (t.jmin >= 0 ? t.jmin : t.jmin - 7) / 8 * 8;                  // aligned-down tile origin (may be negative)
    return true;
  };
  const int nit = (b_hi - b_lo) * nib;
  auto next_valid = [&](int it, Tl& t) -> int {
    while (it < nit && !tile_at(it, t)) ++it;
    return it;
  };
  // LDS-DMA of one tile: raw dS rows [64][208] (source columns clamped into the row: out-of-range pairs are masked at use) + qv block
  auto issue = [&](const Tl& t, char* buf) {
    const bf16_t* dsb = ds + ((long)t.b * H + h) * T * lds;
#pragma unroll
    for (int q7 = 0; q7 < 7; ++q7) {
      const int q = (w * 7 + q7) * 64 + lane;
      const int qq = min(q, DPX_CHUNKS - 1);
      const int il = qq / (DPX_TLD / 8), ch = qq % (DPX_TLD / 8);
      const int i = min(t.i0 + il, T - 1);
      const int j = min(max(t.jb0 + ch * 8, 0), lds - 8);
      glds16_asm(dsb + (long)i * lds + j, buf + __builtin_amdgcn_readfirstlane((w * 7 + q7) * 1024));
    }
    load_rows<BI, true>(buf + DPX_TILE_BYTES, qv + (long)t.b * T * HD + h * DH, HD, t.i0, T, w, lane);
  };

  Tl cur, nxt;
  int it = next_valid(0, cur);
  int buf = 0;
  if (it < nit) issue(cur, smem);
  while (it < nit) {
    const int itn = next_valid(it + 1, nxt);
    if (itn < nit) {
      issue(nxt, smem + (buf ^ 1) * DPX_BUF);
      asm volatile("s_waitcnt vmcnt(9)" ::: "memory");   // this tile's 9 DMA instructions have landed, the next tile's stay in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const bf16_t* sT = reinterpret_cast<const bf16_t*>(smem + buf * DPX_BUF);
    const char* sQ = smem + buf * DPX_BUF + DPX_TILE_BYTES;
    // Tile column of key j is j - jb0 whatever the sign of jb0: the DMA clamps the ORIGIN of a 16-byte chunk, not the row, so a chunk of
    // keys >= 0 (origin jb0 + 8 ch >= 0, jb0 a multiple of 8) lands unshifted; only chunks that lie wholly below key 0 (or from lds on)
    // hold other columns' values, and their pairs do not exist (j < 0 or j >= T: masked below).
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int c = c0 + (2 * w + ct) * 16 + r;           // this lane's table row (A row)
      const int rr = c - cur.shift;
      const bool cvalid = rr >= 0 && rr < cur.lim && c < R;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        short8_t a;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int il = kk * 32 + g * 8 + t;
          const int j = cur.jmin + (c - c0) + il;          // real key index: pairs outside [0, T) do not exist
          const bool ok = cvalid && j >= 0 && j < T && cur.i0 + il < T;
          const int col = j - cur.jb0;
          a[t] = ok ? (short)sT[il * DPX_TLD + col] : (short)0;
        }
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[ct][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, frag_kt(sQ, n * 16, kk * 32 + g * 8, r), acc[ct][n], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                          // everyone is done with this buffer before the tile after next lands in it
    cur = nxt;
    it = itn;
    buf ^= 1;
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + (2 * w + ct) * 16 + g * 4 + e;
      if (c < R) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const float v = acc[ct][n][e];
          if (v != 0.f) atomicAdd(dpext + (long)c * HD + h * DH + n * 16 + r, v);
        }
      }
    }
}


// ======================================================================================================================
// Backward, part 2 (key side): block = (b, h, 64 key rows), wave = 16 key rows, loop over 64-query blocks.  Everything is computed
// transposed (rows = keys) so dK / dV accumulate in registers:
//   sT[j,i] = k_j.qu_i + G[i, c(i,j)],  pT = exp(sT - lse_i),  dpT[j,i] = v_j.dO_i,  dsT = pT (dpT - D_i) scale
//   dv_j += sum_i pT[j,i] dO_i ;   dk_j += sum_i dsT[j,i] qu_i
// PIPELINED (round 6).  Against the kernel of rounds 2-5 (block-wide window scores through a 34 KB strip, single-buffered tiles, row-major
// images written with 2-byte stores: 88 us per layer, removed) four changes:
//  * the window scores are PRIVATE to a wave: for its 16 keys and the 16 queries of tile `it` the relative positions span 31 window rows =
//    two 16-row tiles (3 - it + w, 4 - it + w) of the block's window - 16 MFMAs per wave and query block, exactly what its share of the
//    block-wide 128 x 64 product was, but into a 2.3 KB strip of its own (two slots) instead of a 34 KB strip every wave waits for: one
//    workgroup barrier and 26 KB of LDS less;
//  * the freed LDS double-buffers the qu / dO blocks (live for the whole iteration: the next block's are requested at the top of the
//    current one) and lets the qv / window blocks (dead behind the score products) be refetched behind the barrier that ends those products,
//    under the exponentials and the dK / dV products (inline-asm DMA, one hand-placed vmcnt(0) per iteration) - 74 KB, two workgroups per CU;
//  * the P^T / dS^T operand images are stored TRANSPOSED with one 8-byte store per (query, image) and read back through the transposing
//    LDS read (img_store / img_frag): 8 instead of 32 LDS stores per lane and query block, no two lanes sharing a dword;
//  * the bias-row score (q_i + v) . pext[R] of a query comes from the query-side kernel (second plane of `dvec`) instead of from window
//    tile 7, which most waves do not compute any more.
// Two workgroup barriers per query block instead of three, no exposed DMA wait at the top of an iteration (104 clocks: tools/attn_timing.py);
// per live query block 8 400 -> 7 300 clocks of wave 0, 88 -> 80 us per layer, step -0.09 ms same box.
// ======================================================================================================================
constexpr int K2_GLD = 36, K2_SLOT = 16 * K2_GLD * 4, K2_WAVE = 2 * K2_SLOT;  // strip slots [16 il][36] f32; the 2 x 2 KB images lie over them
static_assert(K2_WAVE >= 4096, "the P^T and dS^T images fit over the strip slots");
constexpr int SMEM_BWD_K = 4 * SK_BYTES + SK_BYTES + SP_BYTES + 4 * K2_WAVE;  // (qu, dO) x 2 + qv + window + per-wave regions
static_assert((SMEM_BWD_K + 1279) / 1280 * 2 <= 128, "two workgroups per CU");

// A-operand images of the key-side kernel, TRANSPOSED: [64 k = il][16 rows = jl] bf16 (32-byte k-rows, 2 KB).  A lane's four values of a
// query (keys g*4 .. +3) are ONE 8-byte store (slot g ^ ((il >> 2) & 3): the 16 lanes of a ds_write_b64 group cover all 32 banks) - in the
// row-major [16 jl][64 il] image they were four 2-byte stores into four rows, 32 per lane and query block for the two images, two lanes
// sharing every dword.  The fragment (row jl = r, k = kbase .. +7) comes back through the transposing read, as frag_kt's.
__device__ __forceinline__ void img_store(char* s, int il, int g, float v0, float v1, float v2, float v3) {
  uint2 u;
  u.x = pack2_bf16(v0, v1);
  u.y = pack2_bf16(v2, v3);
  *reinterpret_cast<uint2*>(s + il * 32 + ((g ^ ((il >> 2) & 3)) << 3)) = u;
}
__device__ __forceinline__ short8_t img_frag(const char* s, int kbase, int r) {
  const int k0 = kbase + (r >> 2), k1 = k0 + 4, c = r & 3;
  const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4_t*)(s + k0 * 32 + ((c ^ ((k0 >> 2) & 3)) << 3)));
  const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4_t*)(s + k1 * 32 + ((c ^ ((k1 >> 2) & 3)) << 3)));
  short8_t v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return v;
}

// `order` (the merged launch; nullptr: sample rank = sample index): the samples by length, longest first (relattn_bwd_prep_kernel) - a
// workgroup runs as long as its sample is, and the hardware starts workgroups in id order.  dk / dv rows are owned by one workgroup each,
// so the order changes no bit.  `lin`: see attn_block_id.
template <bool STREAM>
__device__ __forceinline__ void relattn_bwd_k_body(
    char* const smem, const int lin, const int32_t* __restrict__ order,
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ qu, const bf16_t* __restrict__ qv,
    const bf16_t* __restrict__ pext, const int32_t* __restrict__ lengths, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ dvec, bf16_t* __restrict__ dqkv, int B, int H, int T, float scale,
    int use_mask, int chunk, int hist) {
  char* const sQu0 = smem;                    // [2] qu blocks
  char* const sdO0 = sQu0 + 2 * SK_BYTES;     // [2] dO blocks
  char* const sQv = sdO0 + 2 * SK_BYTES;
  char* const sP = sQv + SK_BYTES;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  char* const sW = sP + SP_BYTES + w * K2_WAVE;  // this wave's region: strip slots, then (over them) the two A images
  float* const sS = reinterpret_cast<float*>(sW);
  char* const sAp = sW;
  char* const sAs = sW + 2048;
  const int r = lane & 15, g = lane >> 4;
  const BlockId bid = attn_block_id<false>(B, H, (T + BJ - 1) / BJ, lin);
  if (!bid.ok) return;
  const int b = order ? order[bid.b] : bid.b, h = bid.h, j0 = bid.blk * BJ;
  const int HD = H * DH, LDQ = 3 * HD, R1 = 2 * T;
  const int len = lengths ? min(lengths[b], T) : T;
  const int shift = T - len;
  const bf16_t* kb = qkv + (long)b * T * LDQ + HD + h * DH;
  const bf16_t* vb = kb + HD;
  const bf16_t* qub = qu + (long)b * T * HD + h * DH;
  const bf16_t* qvb = qv + (long)b * T * HD + h * DH;
  const bf16_t* dob = dout + (long)b * T * HD + h * DH;
  const bf16_t* pb = pext + h * DH;
  uint4 bias_row = make_uint4(0, 0, 0, 0);
  if ((threadIdx.x >> 6) == 0 && (threadIdx.x & 63) < 8) bias_row = *reinterpret_cast<const uint4*>(pb + (long)(2 * T - 1) * HD + (((threadIdx.x & 63) ^ key_d(127)) << 3));

  const int jrow = min(j0 + w * 16 + r, T - 1);
  short8_t ak[2], av[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    ak[kk] = row_frag(kb + (long)jrow * LDQ, kk * 32 + g * 8);
    av[kk] = row_frag(vb + (long)jrow * LDQ, kk * 32 + g * 8);
  }
  float4_t acc_k[4], acc_v[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) { acc_k[n] = float4_t{0.f, 0.f, 0.f, 0.f}; acc_v[n] = float4_t{0.f, 0.f, 0.f, 0.f}; }

  const float scale2 = scale * 1.4426950408889634f;
  const int lim = 2 * len - 1;
  const long lrow = ((long)b * H + h) * T;
  const long plane = (long)B * H * T;  // second plane of dvec: the bias-row score of every query (relattn_fused_bwd_qT_kernel)
  int rrk[4];
  bool jin[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int jl = w * 16 + g * 4 + e;
    rrk[e] = T - 1 + j0 + jl;
    jin[e] = j0 + jl < T;
  }
  const int soff = r * K2_GLD + 15 - r + g * 4;  // + e: this lane's skewed score of key g*4 + e in a strip slot (window column 15 - il + jl of the pair of tiles)
  const int nib = (T + BI - 1) / BI;
  auto full_block = [&](int ib) { return !(use_mask && ib * BI >= len); };
  auto issue_a = [&](int ib) {  // qu / dO blocks of query block ib -> buffer ib & 1
    load_rows<BI, true>(sQu0 + (ib & 1) * SK_BYTES, qub, HD, ib * BI, T, w, lane);
    load_rows<BI, true>(sdO0 + (ib & 1) * SK_BYTES, dob, HD, ib * BI, T, w, lane);
  };
  auto issue_b = [&](int ib) {  // qv block and the window of (query block ib, this key block)
    load_rows<BI, true>(sQv, qvb, HD, ib * BI, T, w, lane);
    load_rows<WIN, true, true>(sP, pb, HD, (T - 1 - (ib * BI + BI - 1) + j0) + shift, R1, w, lane);  // (row 127 = the bias row, written once)
  };
  // per-query scalars of a block: log-sum-exp, D_i, bias-row score (plain loads: issued in FRONT of the DMA pieces they travel with)
  float lse_nx[4], Di_nx[4], gb_nx[4];
  auto load_scalars = [&](int ib) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int ic = min(ib * BI + it * 16 + r, T - 1);
      lse_nx[it] = lse[lrow + ic] * 1.4426950408889634f;
      Di_nx[it] = dvec[lrow + ic];
      gb_nx[it] = dvec[plane + lrow + ic];
    }
  };
  if (w == 0 && lane < 8) *reinterpret_cast<uint4*>(sP + 127 * 128 + lane * 16) = bias_row;  // (visible behind the first iteration's barrier)
  load_scalars(0);
  issue_a(0);
  if (full_block(0)) issue_b(0);
#ifdef TFASR_ATTN_TIMING
  long long ph[5] = {0, 0, 0, 0, 0};
  int nfull = 0;
  const long long t_begin = __builtin_readcyclecounter();
#endif
  for (int ib = 0; ib < nib; ++ib) {
    const int i0 = ib * BI;
    const bool full = full_block(ib);
#ifdef TFASR_ATTN_TIMING
    long long tp = __builtin_readcyclecounter();
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this block's tiles and scalars (requested one / half an iteration ago)
    __builtin_amdgcn_s_barrier();                      // ... of every wave; every wave is done with the other qu / dO buffer and with its images
    if (full) { ATT_TICK(0) }
    float lse2_it[4], Di_it[4], gb_it[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) { lse2_it[it] = lse_nx[it]; Di_it[it] = Di_nx[it]; gb_it[it] = gb_nx[it]; }
    if (ib + 1 < nib) issue_a(ib + 1);
    const char* sQu = sQu0 + (ib & 1) * SK_BYTES;
    const char* sdO = sdO0 + (ib & 1) * SK_BYTES;
    if (!full) {
      // a block of padded query rows: p = 1 / T for every key (exp2(0 - lse), lse = log T), dS = 0: only dv += P^T @ dO remains
      if (ib + 1 < nib) load_scalars(ib + 1);  // (padded query blocks are a suffix: the next one needs no qv / window either)
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int i = i0 + it * 16 + r;
        const float pv = i < T ? __builtin_amdgcn_exp2f(0.f - lse2_it[it]) : 0.f;
        img_store(sAp, it * 16 + r, g, jin[0] ? pv : 0.f, jin[1] ? pv : 0.f, jin[2] ? pv : 0.f, jin[3] ? pv : 0.f);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const short8_t ap = img_frag(sAp, kk * 32 + g * 8, r);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc_v[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kt(sdO, n * 16, kk * 32 + g * 8, r), ap, acc_v[n], 0, 0, 0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      continue;
    }
    // transposed content scores and dP (rows = this wave's 16 keys, columns = the 16 queries of tile it), and the wave's own window scores.
    // Staged so that nothing waits inside: all 32 products first (their fragment reads stream under them), THEN the strip round trips -
    // tiles 0 / 1 through the two slots, tiles 2 / 3 behind them (one wave's LDS operations execute in order: the second pair of writes
    // cannot pass the first pair of reads).  As one loop over `it` every tile's write -> read round trip sat between two groups of products:
    // 3 045 of a query block's 8 400 clocks (tools/attn_timing.py).
    float4_t acc_s[4], acc_p[4], ga[4][2];
    float gvv[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      acc_s[it] = float4_t{0.f, 0.f, 0.f, 0.f};
      acc_p[it] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        acc_s[it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ak[kk], frag_rows(sQu, it * 16 + r, kk * 4 + g), acc_s[it], 0, 0, 0);
        acc_p[it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[kk], frag_rows(sdO, it * 16 + r, kk * 4 + g), acc_p[it], 0, 0, 0);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      short8_t fq[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) fq[kk] = frag_rows(sQv, it * 16 + r, kk * 4 + g);
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int ct = 3 - it + w + cc;  // window tile: rows ct*16 .. +15 (0 <= ct <= 7)
        ga[it][cc] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          ga[it][cc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows(sP, ct * 16 + r, kk * 4 + g), fq[kk], ga[it][cc], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int hp = 0; hp < 2; ++hp) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int it = hp * 2 + q;
        float* slot = sS + q * (K2_SLOT / 4);
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) *reinterpret_cast<float4_t*>(slot + r * K2_GLD + cc * 16 + g * 4) = ga[it][cc];  // G[il = r][c_local = cc*16 + g*4 + e]
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int it = hp * 2 + q;
        const float* slot = sS + q * (K2_SLOT / 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) gvv[it][e] = slot[soff + e];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    ATT_TICK(1)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave has read the qv block and the window: the next block's may land (and the strips are in registers)
    if (ib + 1 < nib) {
      load_scalars(ib + 1);
      if (full_block(ib + 1)) issue_b(ib + 1);
    }
    ATT_TICK(2)
    // pT and dsT in C layout (row jl = g*4+e of this wave, col il = it*16+r) -> A-operand images [16 jl][64 k = il] over the strip slots
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int il = it * 16 + r, i = i0 + il;
      const int ic = min(i, T - 1);
      const float lse2 = lse2_it[it];
      const float D_i = Di_it[it];
      const bool qmask = use_mask && (i >= len);
      const bool iin = i < T;
      const float gbias = gb_it[it];
      int wlo = 0, whi = T;
      if constexpr (STREAM) { if (!qmask) stream_window(ic, T, chunk, hist, wlo, whi); }
      float pp[4], dd[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pos = (rrk[e] - i < lim) ? gvv[it][e] : gbias;
        float p = 0.f, d = 0.f;
        bool vis = iin && jin[e];
        if constexpr (STREAM) { const int j = j0 + w * 16 + g * 4 + e; vis = vis && j >= wlo && j < whi; }
        if (vis) {
          const float s2 = qmask ? 0.f : (acc_s[it][e] + pos) * scale2;
          p = __builtin_amdgcn_exp2f(s2 - lse2);
          d = qmask ? 0.f : p * (acc_p[it][e] - D_i) * scale;
        }
        pp[e] = p;
        dd[e] = d;
      }
      img_store(sAp, il, g, pp[0], pp[1], pp[2], pp[3]);
      img_store(sAs, il, g, dd[0], dd[1], dd[2], dd[3]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    ATT_TICK(3)
    // dv^T += dO^T @ p ; dk^T += qu^T @ ds   (A operands: the dO / qu blocks read transposed, k = i; B operands: the images)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const short8_t ap = img_frag(sAp, kk * 32 + g * 8, r);
      const short8_t as = img_frag(sAs, kk * 32 + g * 8, r);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        acc_v[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kt(sdO, n * 16, kk * 32 + g * 8, r), ap, acc_v[n], 0, 0, 0);
        acc_k[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_kt(sQu, n * 16, kk * 32 + g * 8, r), as, acc_k[n], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the fragments are in registers before the next iteration's barrier releases the buffers)
    ATT_TICK(4)
#ifdef TFASR_ATTN_TIMING
    ++nfull;
#endif
  }
#if defined(TFASR_ATTN_TIMING) && TFASR_ATTN_TIMING == 3  // (-DTFASR_ATTN_TIMING=3: this kernel owns the probe buffer; =1: the query-side backward)
  if (threadIdx.x == 0 && blockIdx.x < 8192) {  // [5 phase sums of wave 0 over the live query blocks][loop][0][live query blocks]
    long long* o = g_attn_timing + 8L * blockIdx.x;
    for (int kq = 0; kq < 5; ++kq) o[kq] = ph[kq];
    o[5] = __builtin_readcyclecounter() - t_begin; o[6] = 0; o[7] = nfull;
  }
#endif
  // dK^T / dV^T are accumulated TRANSPOSED (the operand slots of the two products swapped): lane (r, g) holds key j0 + w*16 + r, four
  // consecutive head dims n*16 + g*4 + e - eight 8-byte stores per lane (they were 32 two-byte ones)
  {
    const int j = j0 + w * 16 + r;
    if (j < T) {
      bf16_t* row = dqkv + ((long)b * T + j) * LDQ + h * DH;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        uint2 vk, vv;
        vk.x = pack2_bf16(acc_k[n][0], acc_k[n][1]); vk.y = pack2_bf16(acc_k[n][2], acc_k[n][3]);
        vv.x = pack2_bf16(acc_v[n][0], acc_v[n][1]); vv.y = pack2_bf16(acc_v[n][2], acc_v[n][3]);
        *reinterpret_cast<uint2*>(row + HD + n * 16 + g * 4) = vk;
        *reinterpret_cast<uint2*>(row + 2 * HD + n * 16 + g * 4) = vv;
      }
    }
  }
}

template <bool STREAM>
__global__ __launch_bounds__(256, 2) void relattn_fused_bwd_k_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ qu, const bf16_t* __restrict__ qv,
    const bf16_t* __restrict__ pext, const int32_t* __restrict__ lengths, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ dvec, bf16_t* __restrict__ dqkv, int B, int H, int T, float scale,
    int use_mask, int chunk, int hist) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  relattn_bwd_k_body<STREAM>(smem, (int)blockIdx.x, nullptr, qkv, qu, qv, pext, lengths, dout, lse, dvec, dqkv, B, H, T, scale, use_mask, chunk, hist);
}

// ======================================================================================================================
// Backward, both sides in ONE launch (tfasr_relattn_fused_bwd_qk).  As two launches each side leaves most of the chip empty for half of
// its time: the live query-side workgroups are equally long and come to 1.1 - 1.4 rounds of the 512 resident slots, run as two; a key-side
// workgroup is as long as its sample, and a long sample late in the batch starts when the rest is nearly done.  Here ids [0, nq) are the
// query side in its block-major order (live blocks - the longest workgroups of the launch - first; a wholly padded block exits at once and
// frees its slot) and ids [nq, nq + nk) the key side with the samples longest first (`order`), so the key side fills the slots the
// query side's second round leaves empty.  For that the key side must not depend on the query side: what it used to read from it
// (q + u, q + v, dvec) comes from relattn_bwd_prep_kernel, launched ahead, and the query side reads the same buffers (PRE).  No workgroup
// waits for another one: no flag, no counter, no spin.  nq is a multiple of 8: both roles keep id & 7 = XCD (attn_block_id).
// ======================================================================================================================
constexpr int SMEM_BWD_QK = qt_smem(1) > SMEM_BWD_K ? qt_smem(1) : SMEM_BWD_K;
static_assert((SMEM_BWD_QK + 1279) / 1280 * 2 <= 128, "two workgroups per CU");

template <bool STREAM>
__global__ __launch_bounds__(256, 2) void relattn_fused_bwd_qk_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ ubias, const float* __restrict__ vbias, const bf16_t* __restrict__ pext,
    const int32_t* __restrict__ lengths, const bf16_t* __restrict__ dout, const float* __restrict__ lse, const bf16_t* __restrict__ qu,
    const bf16_t* __restrict__ qv, const float* __restrict__ dvec, const int32_t* __restrict__ order, bf16_t* __restrict__ dqkv,
    bf16_t* __restrict__ dpos, float* __restrict__ dpext, float* __restrict__ du, float* __restrict__ dv, int B, int H, int T, int ldp,
    float scale, int use_mask, int chunk, int hist, int nq) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lin = (int)blockIdx.x;
  if (lin < nq) {
    relattn_bwd_qT_body<STREAM, 1, true>(smem, lin, qkv, ubias, vbias, pext, lengths, nullptr, dout, lse, dqkv, dpos, const_cast<float*>(dvec), B, H, T,
                                         ldp, scale, use_mask, dpext, 3L * H * DH, du, dv, chunk, hist, const_cast<bf16_t*>(qu), const_cast<bf16_t*>(qv));
  } else {
    relattn_bwd_k_body<STREAM>(smem, lin - nq, order, qkv, qu, qv, pext, lengths, dout, lse, dvec, dqkv, B, H, T, scale, use_mask, chunk, hist);
  }
}

// Preparation of the merged launch: one pass over q, o and dO that writes q + u, q + v and both planes of dvec (D_i = rowsum(dO * o) and the
// bias-row score (q_i + v) . pext[R]) with the arithmetic of the query-side body (qrow_frags / qrow_bias_part, the same lane layout and the
// same reduction order: the same bits), for the rows the query-side kernel writes them for (every row of a 64-query block that is not wholly
// padding).  Workgroup (0, 0, 0) also writes `order`: the samples by length, descending, ties by sample index - a permutation of 0 .. B-1.
__global__ __launch_bounds__(256) void relattn_bwd_prep_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ ubias, const float* __restrict__ vbias, const bf16_t* __restrict__ pext,
    const int32_t* __restrict__ lengths, const bf16_t* __restrict__ o, const bf16_t* __restrict__ dout, bf16_t* __restrict__ qu_out,
    bf16_t* __restrict__ qv_out, float* __restrict__ dvec, int32_t* __restrict__ order, int B, int H, int T, int use_mask) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
    for (int s = threadIdx.x; s < B; s += 256) {
      const int ls = lengths ? min(lengths[s], T) : T;
      int rank = 0;
      for (int t = 0; t < B; ++t) {
        const int lt = lengths ? min(lengths[t], T) : T;
        rank += (lt > ls || (lt == ls && t < s)) ? 1 : 0;
      }
      order[rank] = s;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * BI;
  const int HD = H * DH, LDQ = 3 * HD, R = 2 * T - 1;
  const int len = lengths ? min(lengths[b], T) : T;
  if (use_mask && i0 >= len) return;
  const int i = i0 + w * 16 + r;
  const int irow = min(i, T - 1);
  const long orow = ((long)b * T + irow) * HD + h * DH;
  short8_t bqu[2], bqv[2], bdo[2];
  float dpart = qrow_frags(qkv + ((long)b * T + irow) * LDQ + h * DH, ubias + h * DH, vbias + h * DH, dout + orow, o + orow, g, bqu, bqv, bdo);
  dpart = xor32_sum(xor16_sum(dpart));
  const float gbias = xor32_sum(xor16_sum(qrow_bias_part(bqv, pext + (long)R * HD + h * DH, g)));
  if (i < T) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      *reinterpret_cast<short8_t*>(qu_out + orow + kk * 32 + g * 8) = bqu[kk];
      *reinterpret_cast<short8_t*>(qv_out + orow + kk * 32 + g * 8) = bqv[kk];
    }
    if (g == 0) {
      dvec[((long)b * H + h) * T + i] = dpart;
      dvec[(long)B * H * T + ((long)b * H + h) * T + i] = gbias;
    }
  }
}

}  // namespace

extern "C" int tfasr_relattn_fused_fwd(const void* qkv, const float* ubias, const float* vbias, const void* pext,
                                       const int32_t* lengths, void* out, float* lse, int B, int H, int T, int dh, float scale,
                                       int use_mask, int chunk, int hist, int dtype, void* stream_) {
  if (!qkv || !ubias || !vbias || !pext || !out || !lse || B <= 0 || H <= 0 || T <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_BF16 || dh != DH) return TFASR_STATUS_UNSUPPORTED;
  const dim3 gridT(attn_grid_size(B, H, (T + BI - 1) / BI));
  if (chunk > 0) TFASR_KLAUNCH(relattn_fused_fwdT_kernel<true>, gridT, dim3(256), SMEM_FWDT, (hipStream_t)stream_, (const bf16_t*)qkv, ubias, vbias,
                                    (const bf16_t*)pext, lengths, (bf16_t*)out, lse, B, H, T, scale, use_mask, chunk, hist);
  else TFASR_KLAUNCH(relattn_fused_fwdT_kernel<false>, gridT, dim3(256), SMEM_FWDT, (hipStream_t)stream_, (const bf16_t*)qkv, ubias, vbias,
                          (const bf16_t*)pext, lengths, (bf16_t*)out, lse, B, H, T, scale, use_mask, chunk, hist);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_relattn_fused_bwd_q3(const void* qkv, const float* ubias, const float* vbias, const void* pext, const int32_t* lengths,
                                          const void* o, const void* dout, const float* lse, void* dq, long lddq, float* du, float* dv, void* ds,
                                          float* dvec, float* dpext, void* qu, void* qv, int B, int H, int T, int dh, int lds, float scale,
                                          int use_mask, int chunk, int hist, int dtype, void* stream_) {
  if (!qkv || !ubias || !vbias || !pext || !o || !dout || !lse || !dq || !du || !dv || !ds || !dvec || !dpext || B <= 0 || H <= 0 || T <= 0 || lds < T ||
      (lds & 7) || lddq < (long)H * dh || (lddq & 3) || ((qu == nullptr) != (qv == nullptr)) || (((uintptr_t)qu | (uintptr_t)qv) & 15))
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_BF16 || dh != DH) return TFASR_STATUS_UNSUPPORTED;
  const dim3 gq(attn_grid_size(B, H, (T + BI - 1) / BI));
#define TFASR_QT_LAUNCH(ST)                                                                                                                  \
  tfasr_dynamic_lds<relattn_fused_bwd_qT_kernel<ST, 1>>(qt_smem(1));                                                                        \
  TFASR_KLAUNCH((relattn_fused_bwd_qT_kernel<ST, 1>), gq, dim3(256), qt_smem(1), (hipStream_t)stream_, (const bf16_t*)qkv, ubias, vbias,   \
                     (const bf16_t*)pext, lengths, (const bf16_t*)o, (const bf16_t*)dout, lse, (bf16_t*)dq, (bf16_t*)ds, dvec, B, H, T, lds, scale, \
                     use_mask, dpext, lddq, du, dv, chunk > 0 ? chunk : 0, chunk > 0 ? hist : 0, (bf16_t*)qu, (bf16_t*)qv)
  if (chunk > 0) { TFASR_QT_LAUNCH(true); } else { TFASR_QT_LAUNCH(false); }
#undef TFASR_QT_LAUNCH
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_relattn_dpext(const void* ds, const void* qv, const int32_t* lengths, float* dpext, int B, int H, int T, int dh, int lds,
                                   int use_mask, int dtype, void* stream_) {
  if (!ds || !qv || !dpext || B <= 0 || H <= 0 || T <= 0 || lds < T || (lds & 7)) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_BF16 || dh != DH) return TFASR_STATUS_UNSUPPORTED;
  const int cblocks = (2 * T - 1 + 127) / 128;
  // sample groups: enough workgroups to fill the chip (4 per CU measured best: 512 -> +0.12 ms per step, 2048: no further gain) without
  // multiplying the atomics more than needed
  const int target = 1024;
  int groups = std::max(1, std::min(B, target / std::max(1, cblocks * H)));
  const int bchunk = (B + groups - 1) / groups;
  groups = (B + bchunk - 1) / bchunk;
  TFASR_KLAUNCH(relattn_dpext_kernel, dim3(cblocks, H, groups), dim3(256), SMEM_DPX, (hipStream_t)stream_, (const bf16_t*)ds, (const bf16_t*)qv,
                     lengths, dpext, B, H, T, lds, use_mask, bchunk);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_relattn_fused_bwd_k(const void* qkv, const void* qu, const void* qv, const void* pext, const int32_t* lengths,
                                         const void* dout, const float* lse, const float* dvec, void* dqkv, int B, int H, int T,
                                         int dh, float scale, int use_mask, int chunk, int hist, int dtype, void* stream_) {
  if (!qkv || !qu || !qv || !pext || !dout || !lse || !dvec || !dqkv || B <= 0 || H <= 0 || T <= 0) return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_BF16 || dh != DH) return TFASR_STATUS_UNSUPPORTED;
  const dim3 gk(attn_grid_size(B, H, (T + BJ - 1) / BJ));
#define TFASR_BK_LAUNCH(KERN, SMEM, ST, CH, HI)                                                                                         \
  tfasr_dynamic_lds<KERN<ST>>(SMEM);                                                                                                    \
  TFASR_KLAUNCH((KERN<ST>), gk, dim3(256), SMEM, (hipStream_t)stream_, (const bf16_t*)qkv, (const bf16_t*)qu, (const bf16_t*)qv,        \
                (const bf16_t*)pext, lengths, (const bf16_t*)dout, lse, dvec, (bf16_t*)dqkv, B, H, T, scale, use_mask, CH, HI)
  if (chunk > 0) { TFASR_BK_LAUNCH(relattn_fused_bwd_k_kernel, SMEM_BWD_K, true, chunk, hist); } else { TFASR_BK_LAUNCH(relattn_fused_bwd_k_kernel, SMEM_BWD_K, false, 0, 0); }
#undef TFASR_BK_LAUNCH
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_relattn_bwd_prep(const void* qkv, const float* ubias, const float* vbias, const void* pext, const int32_t* lengths,
                                      const void* o, const void* dout, void* qu, void* qv, float* dvec, int32_t* order, int B, int H, int T,
                                      int dh, int use_mask, int dtype, void* stream_) {
  if (!qkv || !ubias || !vbias || !pext || !o || !dout || !qu || !qv || !dvec || !order || B <= 0 || H <= 0 || T <= 0 || B > 65535 || H > 65535 ||
      (((uintptr_t)qu | (uintptr_t)qv) & 15))
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_BF16 || dh != DH) return TFASR_STATUS_UNSUPPORTED;
  TFASR_KLAUNCH(relattn_bwd_prep_kernel, dim3((T + BI - 1) / BI, H, B), dim3(256), 0, (hipStream_t)stream_, (const bf16_t*)qkv, ubias, vbias,
                (const bf16_t*)pext, lengths, (const bf16_t*)o, (const bf16_t*)dout, (bf16_t*)qu, (bf16_t*)qv, dvec, order, B, H, T, use_mask);
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

extern "C" int tfasr_relattn_fused_bwd_qk(const void* qkv, const float* ubias, const float* vbias, const void* pext, const int32_t* lengths,
                                          const void* dout, const float* lse, const void* qu, const void* qv, const float* dvec,
                                          const int32_t* order, void* dqkv, float* du, float* dv, void* ds, float* dpext, int B, int H, int T, int dh,
                                          int lds, float scale, int use_mask, int chunk, int hist, int dtype, void* stream_) {
  if (!qkv || !ubias || !vbias || !pext || !dout || !lse || !qu || !qv || !dvec || !order || !dqkv || !du || !dv || !ds || !dpext || B <= 0 || H <= 0 ||
      T <= 0 || lds < T || (lds & 7) || (((uintptr_t)qu | (uintptr_t)qv) & 15))
    return TFASR_STATUS_INVALID_VALUE;
  if (dtype != TFASR_BF16 || dh != DH) return TFASR_STATUS_UNSUPPORTED;
  const unsigned nq = attn_grid_size(B, H, (T + BI - 1) / BI), nk = attn_grid_size(B, H, (T + BJ - 1) / BJ);
#define TFASR_QK_LAUNCH(ST, CH, HI)                                                                                                          \
  tfasr_dynamic_lds<relattn_fused_bwd_qk_kernel<ST>>(SMEM_BWD_QK);                                                                          \
  TFASR_KLAUNCH((relattn_fused_bwd_qk_kernel<ST>), dim3(nq + nk), dim3(256), SMEM_BWD_QK, (hipStream_t)stream_, (const bf16_t*)qkv, ubias, vbias, \
                (const bf16_t*)pext, lengths, (const bf16_t*)dout, lse, (const bf16_t*)qu, (const bf16_t*)qv, dvec, order, (bf16_t*)dqkv,   \
                (bf16_t*)ds, dpext, du, dv, B, H, T, lds, scale, use_mask, CH, HI, (int)nq)
  if (chunk > 0) { TFASR_QK_LAUNCH(true, chunk, hist); } else { TFASR_QK_LAUNCH(false, 0, 0); }
#undef TFASR_QK_LAUNCH
  TFASR_CHECK_LAUNCH();
  return TFASR_STATUS_SUCCESS;
}

#ifdef TFASR_ATTN_TIMING
// probe build only (tools/attn_timing.sh): per-workgroup phase clocks of the last instrumented attention launch
extern "C" int tfasr_attn_timing_read(long long* out, int n) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_timing), sizeof(long long) * n) == hipSuccess ? 0 : 1;
}
#endif
