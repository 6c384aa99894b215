// Which kernel tfasr_gemm / tfasr_gemm_group take for a call: THE statement of the dispatch rules of the GEMM family.
//
// Pure host arithmetic over the argument struct and the CU count: no HIP, nothing launched, no data pointer dereferenced (only
// null-ness and alignment are looked at), so the file also compiles with a plain C++ compiler (tests/test_gemm_route.py reaches it
// through tfasr_gemm_route / tfasr_gemm_group_route).  The launch side (gemm.hip, gemm_fast.hip) computes the route and maps it to a
// kernel instantiation through the tables below; it decides nothing.
//
//   gemm_route()       one product:  status, kernel family, layout, tile width, compiled epilogue, grid, dynamic LDS, launch count
//   gemm_group_plan()  up to GEMM_GROUP_MAX weight gradients in one launch: k-split per product and the (product, k-slice) units per XCD
//
// The compiled instantiations are written down once, as X-macro lists: TFASR_GEMM_FAST_TABLE (128-row tiles, the persistent and the
// one-tile kernel) and TFASR_GEMM_BIG_TABLE (256-row tiles).  gemm_route() asks the first whether a lean epilogue exists; the launcher
// expands both into its `switch`, so a route outside the lists ends in that switch's default (TFASR_STATUS_EXECUTION_FAILED).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/tfasr_hip.h"

// EPI selects which epilogue terms are COMPILED IN.  The fully generic epilogue (every term behind a runtime branch, tanh /
// sigmoid / f32 outputs included) is ~20k instructions and thrashes the instruction cache: a plain bias epilogue took 1700
// cycles per 16-row strip.  The step's common combinations get lean instantiations; anything else falls back to E_GEN.
enum : int {
  E_ACT = TFASR_GEMM_E_ACT /* swish(+prez) */, E_DACT = TFASR_GEMM_E_DACT /* * swish'(dact_z) */, E_DROP = TFASR_GEMM_E_DROP, E_RES = TFASR_GEMM_E_RES,
  E_WS = TFASR_GEMM_E_WS /* split-K partial -> workspace */, E_CSUM = TFASR_GEMM_E_CSUM /* + column sums of B (bias gradient) */,
  E_LSE = TFASR_GEMM_E_LSE /* + log-softmax statistics of the output rows */, E_RGRAD = TFASR_GEMM_E_RGRAD /* re-computed logits -> RNN-T loss gradient */,
  E_GEN = TFASR_GEMM_E_GEN, E_BNS = TFASR_GEMM_E_BNS /* + BatchNorm backward statistics of the output */,
  E_MUL = TFASR_GEMM_E_MUL /* * dact_z (the stored derivative factor) */
};

typedef tfasr_gemm_route_info GemmRoute;

// ---- the compiled instantiations --------------------------------------------------------------------------------------------------
// X(TA, TB, BN, EPI): gemm_fast_kernel<TA, TB, BN, EPI>; every 64-column entry without E_CSUM also exists as gemm_fast_one_kernel<TA, TB, EPI>.
#define TFASR_GEMM_FAST_LAYOUTS(X, BN, EPI) X(false, false, BN, EPI) X(false, true, BN, EPI) X(true, false, BN, EPI) X(true, true, BN, EPI)
#define TFASR_GEMM_FAST_WIDTH(X, BN)                                                                                              \
  TFASR_GEMM_FAST_LAYOUTS(X, BN, 0)                                                                                               \
  TFASR_GEMM_FAST_LAYOUTS(X, BN, E_GEN)                                                                                           \
  X(false, false, BN, E_RES) X(false, false, BN, E_RES | E_DROP) X(false, false, BN, E_ACT) X(false, false, BN, E_ACT | E_DROP) /* forward Dense layers */ \
  X(false, true, BN, E_DACT) X(false, true, BN, E_DACT | E_DROP) X(false, true, BN, E_MUL)                /* data gradients (dy @ W^T) */ \
  X(true, false, BN, E_CSUM)                                                                              /* weight gradient + bias gradient */
#define TFASR_GEMM_FAST_TABLE(X)                                                                          \
  TFASR_GEMM_FAST_WIDTH(X, 64)                                                                            \
  TFASR_GEMM_FAST_WIDTH(X, 128)                                                                           \
  X(false, true, 64, E_BNS)                                                                               \
  TFASR_GEMM_FAST_LAYOUTS(X, 128, E_WS)                                                                   \
  X(false, false, 128, E_LSE)
// X(TB, BN, EPI, SEG, TR): gemm_big_kernel<TB, BN, EPI, SEG, TR>
#define TFASR_GEMM_BIG_TABLE(X)                                                                                                   \
  X(false, 256, 0, false, false) X(false, 256, 0, false, true) X(false, 256, 0, true, false) X(false, 256, 0, true, true)          \
  X(true, 256, 0, false, false) X(true, 256, 0, false, true) X(true, 256, 0, true, false) X(true, 256, 0, true, true)              \
  X(true, 320, 0, false, false)                                                                                                   \
  X(true, 256, E_DACT, false, false) X(true, 256, E_DACT, false, true) X(true, 320, E_DACT, false, false)                          \
  X(false, 256, E_LSE, false, false) X(false, 256, E_LSE, false, true)                                                             \
  X(false, 256, E_RGRAD, false, false)

// one integer per instantiation: what the launcher switches on
constexpr int gemm_fast_key(bool ta, bool tb, int bn, int epi) { return (epi << 4) | ((bn == 64 ? 0 : 1) << 2) | ((ta ? 1 : 0) << 1) | (tb ? 1 : 0); }
constexpr int gemm_big_key(bool tb, int bn, int epi, bool seg, bool tr) { return (epi << 4) | ((bn == 320 ? 1 : 0) << 3) | ((seg ? 1 : 0) << 2) | ((tr ? 1 : 0) << 1) | (tb ? 1 : 0); }
inline bool gemm_fast_compiled(bool ta, bool tb, int bn, int epi) {
  switch (gemm_fast_key(ta, tb, bn, epi)) {
#define TFASR_X(TA, TB, BN, EPI) case gemm_fast_key(TA, TB, BN, EPI):
    TFASR_GEMM_FAST_TABLE(TFASR_X)
#undef TFASR_X
    return true;
    default: return false;
  }
}

// ---- launch geometry ----------------------------------------------------------------------------------------------------------------
constexpr int GEMM_BM = 128, GEMM_BK = 64;  // rows per tile of the 128-row kernels; k per slab of every bf16 kernel
// dynamic LDS: two stages of (128 x 64 A + BN x 64 B) bf16 + the four waves' epilogue strips; the one-tile kernel lays its strips over the
// dead stages; the 256-row kernels hold two 64 / 72 KiB stages (+ eight waves' strips at 256 columns)
constexpr int gemm_fast_lds(int bn) { return 2 * (GEMM_BM * GEMM_BK * 2 + bn * GEMM_BK * 2) + 4 * (64 / (bn / 16)) * (bn / 2 + 4) * 4; }
constexpr int GEMM_ONE_LDS = 2 * (GEMM_BM * GEMM_BK * 2 + 64 * GEMM_BK * 2);
constexpr int GEMM_GROUP_LDS = 2 * (GEMM_BM * GEMM_BK * 2 + 128 * GEMM_BK * 2);  // accumulate epilogue: atomics from the fragments, no strips
constexpr int gemm_big_lds(int bn) { return bn == 320 ? 2 * (256 * GEMM_BK * 2 + 320 * GEMM_BK * 2) : 2 * (256 * GEMM_BK * 2 + 256 * GEMM_BK * 2) + 8 * 8 * 68 * 4; }

// persistent workgroups on `slots` resident slots: every tile its own workgroup below that, else the slots rounded down to whole XCD rounds
inline int gemm_persistent_grid(long ntiles, int slots) { return ntiles < slots ? (int)ntiles : (slots & ~7); }

inline bool gemm_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline long gemm_ceil(long a, long b) { return (a + b - 1) / b; }
inline long gemm_up8(long n) { return (n + 7) & ~7L; }
// tiles of an x * y * z grid; beyond what a grid can hold the count saturates (far above everything it is compared with) instead of overflowing
inline long gemm_tile_count(long x, long y, long z) { return (x * y > 0x7fffffffL || z > 0x7fffffffL) ? (1L << 62) : x * y * z; }

// what a product with a K-block table must be (tfasr_gemm_args.k_tiles); nb = its batch count
inline bool gemm_ktab_eligible(const tfasr_gemm_args& a, long nb) {
  return a.dtype == TFASR_BF16 && a.trans_a && !a.trans_b && a.accumulate && nb <= 1 && !a.ws && !a.seg_a_off && !a.row_tiles && !a.lse_part &&
         !a.rgrad_coef && !a.bns_out && a.n_k_tiles > 0 && a.n_k_tiles <= gemm_ceil(a.K, 256);
}

// ---- one product ----------------------------------------------------------------------------------------------------------------------
// `ncu`: compute units of the device; allow_big = false keeps the 256-row kernels out (probes: g_gemm_big_mode = 0).
inline GemmRoute gemm_route(const tfasr_gemm_args& a, int ncu, bool allow_big = true) {
  GemmRoute r;
  memset(&r, 0, sizeof(r));
  auto end = [&r](int status) { r.status = status; return r; };
  auto tiles = [&r](long x, long y, long z) { r.tiles_x = (int)x; r.tiles_y = (int)y; r.tiles_z = (int)std::min(z, 0x7fffffffL); return gemm_tile_count(x, y, z); };
  r.launches = 1;
  r.trans_a = a.trans_a != 0;
  r.trans_b = a.trans_b != 0;
  // ---- what tfasr_gemm refuses
  if (!a.A || !a.B || (!a.D && !a.lse_part)) return end(TFASR_STATUS_INVALID_VALUE);
  if (a.rgrad_coef && (!a.row_label || !a.D || a.lse_part)) return end(TFASR_STATUS_INVALID_VALUE);
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return end(TFASR_STATUS_INVALID_VALUE);
  const int split = std::max(a.split_k, 1);
  const long nb = (long)std::max(a.nb1, 1) * std::max(a.nb2, 1), slices = nb > 0x7fffffffL ? nb : nb * split;  // batches; batches x k-slices = the grid's z
  if (a.accumulate && !a.out_f32) return end(TFASR_STATUS_INVALID_VALUE);
  if (split > 1 && !a.accumulate) return end(TFASR_STATUS_INVALID_VALUE);
  if (split > 1 && (a.res || a.dact_z || a.prez || a.act != TFASR_ACT_NONE || a.drop_p > 0.f)) return end(TFASR_STATUS_INVALID_VALUE);
  if (a.drop_p < 0.f || a.drop_p >= 1.f) return end(TFASR_STATUS_INVALID_VALUE);
  if (a.colsum && !(a.accumulate && a.trans_a && !a.trans_b && nb == 1)) return end(TFASR_STATUS_INVALID_VALUE);
  if (a.row_tiles) {  // row-tile table: the K-segmented NN / NT products only, every entry count the tile grid can hold
    if (a.n_row_tiles <= 0 || a.n_row_tiles > gemm_ceil(a.M, 256)) return end(TFASR_STATUS_INVALID_VALUE);
    if (!a.seg_a_off || a.trans_a || a.accumulate || split > 1 || nb != 1 || a.dtype != TFASR_BF16) return end(TFASR_STATUS_UNSUPPORTED);
  }
  if (a.k_tiles) {  // K-block table: the bf16 transposed-A weight gradient only, every entry count the K range can hold
    if (a.n_k_tiles <= 0 || a.n_k_tiles > gemm_ceil(a.K, 256)) return end(TFASR_STATUS_INVALID_VALUE);
    if (!a.trans_a || a.trans_b || !a.accumulate || nb != 1 || a.dtype != TFASR_BF16 || a.seg_a_off || a.row_tiles || a.ws) return end(TFASR_STATUS_UNSUPPORTED);
  }
  const bool ta = r.trans_a, tb = r.trans_b;
  const long m128 = gemm_ceil(a.M, GEMM_BM);

  // ---- the bf16 LDS-DMA kernels (gemm_fast.hip, gemm_big.h).  They need A, B 16-byte aligned, lda / ldb and the batch strides multiples of
  // 8, a k-strided operand's row extent rounded up to 8 inside its row stride (16-byte chunks must stay inside the row) and K >= 8;
  // `break` = the call is left to the generic kernels below
  if (a.dtype == TFASR_BF16 && gemm_al16(a.A) && gemm_al16(a.B) && !(a.lda & 7) && !(a.ldb & 7) && !(a.sA1 & 7) && !(a.sA2 & 7) && !(a.sB1 & 7) && !(a.sB2 & 7) &&
      !(ta && gemm_up8(a.M) > a.lda) && !(!tb && gemm_up8(a.N) > a.ldb) && a.K >= 8) do {
    if (a.k_tiles) {  // K-block table: the accumulating x^T dy product on 128-wide tiles, or nothing at all
      if (!(ta && !tb && gemm_ktab_eligible(a, nb) && a.out_f32)) break;
      const long nt = tiles(gemm_ceil(a.N, 128), m128, split);
      if (nt > 0x7fffffffL) return end(TFASR_STATUS_INVALID_VALUE);
      r.family = TFASR_GEMM_FAST_KTAB; r.tile_n = 128; r.epi = E_CSUM;
      r.workgroups = gemm_persistent_grid(nt, 2 * ncu); r.lds_bytes = gemm_fast_lds(128);
      return end(TFASR_STATUS_SUCCESS);
    }
    // 128x64 tiles: per-head attention products (N = head size: halves the wasted B tile) and every product whose 128x128 tiling
    // would leave at most one workgroup per CU (the N = 256 Dense layers of a Conformer block: 190 tiles): with a single resident
    // workgroup the DMA issue, the fragment reads and the MFMAs of a slab serialise (1530 cycles / slab measured); two 128x64
    // workgroups per CU overlap them (14.2 vs 16.9 us on [12096,256,1024]).
    // Round 4: every product the one-tile kernel takes (no split-K, no accumulation / column sums) with K <= 256 or N <= 256 (the
    // Conformer's d = 256 layers: four slabs per tile, or two 128-wide column tiles) runs as 64-column tiles, ONE per workgroup, three
    // workgroups per CU (gemm_fast_one_kernel), whatever its size: 744 128-wide tiles on 512 persistent slots are two rounds with half
    // the chip idle in the second, 1 488 narrow tiles on 768 dynamic slots are 1.94.  Same-box A/B: [rows,256]x[256,768|512] 17.8 -> 17.0 us,
    // the FFN data gradient with its swish' + dropout epilogue 38.6 -> 34.3, N = 256 products 17.0 -> 16.3 / 16.2 -> 13.0; M 23.23 -> 23.01
    // ms/step, S 12.17 -> 12.01.  With both K and N >= 512 (ContextNet's 512 - 1280-channel layers) the 128-wide persistent kernel amortises
    // a tile better (cross-tile prefetch, half the operand bytes per flop): 33.3 vs 35.5 us per launch there, ContextNet-L 45.0 vs 45.4
    // ms/step - those, and everything that accumulates, take 64 columns only up to one 128-wide tile per CU.
    const long t128 = gemm_tile_count(gemm_ceil(a.N, 128), m128, slices);
    const bool any_size = split <= 1 && !a.accumulate && !a.colsum && std::min(a.K, a.N) <= 256;
    const bool narrow = !a.lse_part && !a.seg_a_off && (a.N <= 64 || ((any_size || t128 <= ncu) && !(a.accumulate && a.ws)));
    const int bn = narrow ? 64 : 128;
    const long ntiles = tiles(gemm_ceil(a.N, bn), m128, slices);
    if (ntiles > 0x7fffffffL) return end(TFASR_STATUS_INVALID_VALUE);
    // epilogue terms this call needs; accumulate (atomics from fragments) needs none of them
    int need = 0;
    bool generic = false;
    if (!a.accumulate) {
      if (a.out_f32) generic = true;
      if (a.act != TFASR_ACT_NONE || a.prez) { if (a.act == TFASR_ACT_SWISH) need |= E_ACT; else generic = true; }
      if (a.dact_z) { if (a.dact == TFASR_ACT_SWISH) need |= E_DACT; else if (a.dact == TFASR_ACT_FACTOR) need |= E_MUL; else generic = true; }
      if (a.drop_p > 0.f) need |= E_DROP;
      if (a.res) need |= E_RES;
    }
    const bool plain = !generic && need == 0;
    // 128-row tiles: one tile per workgroup, three workgroups per CU, when a 64-column tile list does not fit two per CU at once (never for
    // split-K, the column sums, the workspace and the statistics epilogues); else persistent workgroups, two per CU
    auto fast = [&](int epi) {
      r.tile_n = bn; r.epi = epi;
      if (bn == 64 && !(epi & (E_WS | E_CSUM | E_LSE)) && a.split_k <= 1 && ntiles > 2L * ncu) {
        r.family = TFASR_GEMM_FAST_ONE; r.workgroups = (int)ntiles; r.lds_bytes = GEMM_ONE_LDS;
      } else {
        r.family = TFASR_GEMM_FAST_PERSISTENT; r.workgroups = gemm_persistent_grid(ntiles, 2 * ncu); r.lds_bytes = gemm_fast_lds(bn);
      }
      return end(TFASR_STATUS_SUCCESS);
    };
    if (a.bns_out) {  // BatchNorm backward statistics in the epilogue: the plain NT product on 64-column tiles, or nothing at all
      if (!ta && tb && narrow && plain && !a.accumulate && !a.bias && split == 1 && nb == 1 && a.bns_x && a.bns_fin && (a.N & 7) == 0 && (a.ldd & 7) == 0 &&
          (a.bns_c == 0 || (a.bns_c > 0 && (a.bns_c & 7) == 0 && a.N % a.bns_c == 0)) && (((uintptr_t)a.D | (uintptr_t)a.bns_x) & 15) == 0 &&
          !a.colsum && !a.lse_part && !a.seg_a_off && !a.rgrad_coef)
        return fast(E_BNS);
      break;
    }
    // thousands of tiles: 256-row tiles, one 8-wave workgroup per CU (gemm_big.h).  A k-contiguous: [M, K] row major, M >= 256; B
    // k-contiguous (N a multiple of 8) or k-strided (256 columns only).  Epilogues: bias, and the tanh-out factor / the log-softmax
    // statistics / the loss gradient.
    const bool tanh_out = !a.accumulate && a.dact_z && a.dact == TFASR_ACT_TANH_OUT;  // the only epilogue term gemm_big knows beyond bias
    const bool other = a.out_f32 || a.act != TFASR_ACT_NONE || a.prez || (a.dact_z && !tanh_out);
    const bool seg = a.seg_a_off != nullptr;
    if (allow_big && !ta && !other && need == 0 && !a.accumulate && split == 1 && nb == 1 && !a.colsum && a.K >= 2 * GEMM_BK && !(a.K & 7) && a.M >= 256 &&
        !(tb && (a.N & 7)) && !(seg && !(a.seg_k > 0 && (a.seg_k % GEMM_BK) == 0 && (a.K % a.seg_k) == 0 && a.K / GEMM_BK <= 64))) do {
      // BN: 320 for N = 320 / 640 / ... (k-contiguous B only: the joint's data gradient, joint_dim 320 or 640), else 256 when the last
      // column tile is at least 3/4 full
      int big = 0;
      if (tb && !seg && !a.lse_part && (a.N % 320) == 0) big = 320;
      else if (a.N >= (tb ? 256 : 192) && ((a.N % 256) == 0 || (a.N % 256) >= 192)) big = 256;
      if (!big) break;
      const long gx = gemm_ceil(a.N, big), full = gx * gemm_ceil(a.M, 256);
      if (full < 2L * ncu || full > 0x7fffffffL) break;
      if (tanh_out && (!tb || seg || a.lse_part)) break;
      if (a.lse_part && !(!tb && a.row_label && a.pick && big == 256 && a.lse_parts == gemm_ceil(a.N, 128) * 2)) break;
      if (a.rgrad_coef && (tb || seg || tanh_out || big != 256 || !a.row_label)) break;
      if (!a.D && !a.lse_part) break;
      // a row-tile table never changes WHICH kernel runs (the rule above counts the full product's tiles): a listed 256-row block is
      // computed exactly as the full product computes it
      const long nt = tiles(gx, a.row_tiles ? a.n_row_tiles : gemm_ceil(a.M, 256), 1);
      r.family = TFASR_GEMM_BIG; r.tile_n = big;
      r.epi = tanh_out ? E_DACT : a.lse_part ? E_LSE : a.rgrad_coef ? E_RGRAD : 0;
      r.seg = seg && r.epi == 0;  // (the statistics epilogue has no K-segment variant: it reads a contiguous K)
      // transposed accumulators (16-byte stores straight from the accumulators): every variant whose output rows allow them (ldd % 8 == 0,
      // N % 8 == 0, 16-byte aligned D; a statistics-only projection stores nothing).  Not the 320-column kernels (the 160 accumulators leave
      // no register for the transposed epilogue - seen at compile time, also with the tanh-out operand requested only two fragments ahead:
      // two spill reloads land INSIDE the slab loop, each followed by a vmcnt(0) that drains the DMA prefetch; tests/test_isa_guard.py
      // watches for scratch traffic) and not the loss-gradient epilogue.
      r.tr = big == 256 && r.epi != E_RGRAD && (((a.ldd & 7) == 0 && (a.N & 7) == 0 && gemm_al16(a.D)) || (a.lse_part && !a.D));
      r.workgroups = gemm_persistent_grid(nt, ncu); r.lds_bytes = gemm_big_lds(big);
      return end(TFASR_STATUS_SUCCESS);
    } while (0);
    if (a.rgrad_coef || !a.D) break;  // gradient epilogue / statistics-only projection: 256-row kernel only
    // workspace split-K: the k-slices store their partial tiles and a second launch sums them into D.  (Measured: NOT faster than the
    // atomics - 34.8 vs 33.0 us on the [256,1024,19040] weight gradient, +5 ms on the step from the extra workspace traffic - so callers
    // only pass a workspace when TFASR_SPLITK_WS=1; kept as the deterministic option.)
    if (a.accumulate && split > 1 && nb == 1 && a.ws && a.ws_elems / split / a.M >= a.N /* ws_elems >= split M N */ && !narrow && !a.colsum) {
      r.launches = 2;
      return fast(E_WS);
    }
    if (a.colsum) {  // the bias gradient as one more MFMA row of the weight gradient; anything else: a separate column-sum pass below
      if (ta && !tb && a.accumulate && a.N > 64) return fast(E_CSUM);
      break;
    }
    if (a.seg_a_off) {  // K-segmented operands: conv2 forward (NN) / data gradient (NT) over the haloed space-to-depth layout
      if (!(!ta && plain && !a.accumulate && split == 1 && nb == 1 && a.seg_k > 0 && (a.seg_k % GEMM_BK) == 0 && (a.K % a.seg_k) == 0 && a.K / GEMM_BK <= 64 && !a.lse_part)) break;
      const long nt = tiles(gemm_ceil(a.N, 128), a.row_tiles ? 2L * a.n_row_tiles : m128, 1);
      r.family = TFASR_GEMM_FAST_SEG; r.tile_n = 128; r.epi = 0; r.seg = 1;
      r.workgroups = gemm_persistent_grid(nt, 2 * ncu); r.lds_bytes = gemm_fast_lds(128);
      return end(TFASR_STATUS_SUCCESS);
    }
    if (a.lse_part) {  // joint vocabulary projection with fused log-softmax statistics
      if (!ta && !tb && plain && !a.accumulate && nb == 1 && a.row_label && a.pick && a.lse_parts == gemm_ceil(a.N, 128) * 2) return fast(E_LSE);
      break;
    }
    // a lean epilogue where one is compiled, else the generic one.  On 64-column tiles the swish / swish' / factor epilogues serve only
    // layers of MORE than one 128-wide tile per CU (what they were compiled for); smaller products take E_GEN there.
    const bool lean = !generic && gemm_fast_compiled(ta, tb, bn, need) && !(narrow && (need & (E_ACT | E_DACT | E_MUL)) && !(t128 > ncu && a.N > 64));
    return fast(lean ? need : E_GEN);
  } while (0);

  // ---- the generic kernels (gemm.hip): any alignment, f32
  if (a.k_tiles) return end(TFASR_STATUS_UNSUPPORTED);  // only the bf16 fast path reads the table
  if (a.lse_part || a.rgrad_coef || a.bns_out) return end(TFASR_STATUS_UNSUPPORTED);  // only the bf16 fast path's epilogues produce the row statistics / the loss gradient / the BatchNorm sums
  if (a.seg_a_off) return end(TFASR_STATUS_UNSUPPORTED);  // K-segments: bf16 fast path only (the f32 host path issues one product per segment)
  if (a.dtype != TFASR_BF16 && a.dtype != TFASR_F32) return end(TFASR_STATUS_INVALID_VALUE);
  if (a.colsum) r.launches = 2;  // the generic kernels do not fuse the bias gradient: one extra pass over B = dy (tfasr_colsum) first
  r.family = TFASR_GEMM_GENERIC; r.tile_n = 128; r.epi = E_GEN; r.seg = 0; r.lds_bytes = 0;
  long nt = tiles(gemm_ceil(a.N, 128), m128, slices);
  if (r.tiles_y > 65535 || slices > 65535) return end(TFASR_STATUS_INVALID_VALUE);
  // f32: 128 x 64 tiles while the 128-wide tiling leaves CUs without a workgroup of their own (N = 256 at 8 000 rows: 126 tiles for 256
  // CUs) - same slabs, same k order per element: bitwise the same results
  if (a.dtype == TFASR_F32 && a.N > 64 && nt < 2L * ncu) { r.tile_n = 64; nt = tiles(gemm_ceil(a.N, 64), m128, slices); }
  r.workgroups = (int)nt;
  return end(TFASR_STATUS_SUCCESS);
}

// ---- grouped weight gradients -----------------------------------------------------------------------------------------------------------
constexpr int GEMM_GROUP_MAX = 10;
constexpr int GEMM_GROUP_UNITS = 20;  // (product, k-slice) units per XCD
// the launch tables of wgrad_group_kernel (its argument struct holds the products in front of them)
struct GemmGroupTables {
  int gx[GEMM_GROUP_MAX], gy[GEMM_GROUP_MAX];
  // XCD x (= blockIdx.x & 7) runs nunit[x] units; unit u covers slots [j0[x][u], j0[x][u+1]) of that XCD (slot = blockIdx.x >> 3)
  short uq[8][GEMM_GROUP_UNITS], uks[8][GEMM_GROUP_UNITS];
  int j0[8][GEMM_GROUP_UNITS + 1];
  int nunit[8];
};
struct GemmGroupPlan {
  int status;  // SUCCESS: one launch; UNSUPPORTED: the caller launches the products one by one
  int ktab;    // every product carries a K-block table
  int workgroups, lds_bytes;
  int split[GEMM_GROUP_MAX];
  GemmGroupTables t;
};

inline bool gemm_group_eligible(const tfasr_gemm_args& a) {
  return a.dtype == TFASR_BF16 && a.trans_a && !a.trans_b && a.accumulate && a.out_f32 && (long)a.nb1 * a.nb2 <= 1 && !a.ws && !a.bias && !a.res &&
         !a.dact_z && !a.prez && a.act == TFASR_ACT_NONE && a.drop_p == 0.f && gemm_al16(a.A) && gemm_al16(a.B) && !(a.lda & 7) && !(a.ldb & 7) &&
         gemm_up8(a.M) <= a.lda && gemm_up8(a.N) <= a.ldb && a.K >= 8 && a.N > 64 && a.M > 0 && (!a.k_tiles || gemm_ktab_eligible(a, (long)a.nb1 * a.nb2));
}

// One launch for n <= GEMM_GROUP_MAX weight-gradient products (wgrad_group_kernel, 128-column tiles).  `beside`: the launch shares the
// chip with another stream's dependent chain (g_tfasr_group_beside).
inline GemmGroupPlan gemm_group_plan(const tfasr_gemm_args* a, int n, int ncu, bool beside) {
  GemmGroupPlan g;
  memset(&g, 0, sizeof(g));
  g.status = TFASR_STATUS_UNSUPPORTED;
  if (n < 2 || n > GEMM_GROUP_MAX) return g;
  for (int i = 0; i < n; ++i)
    if (!gemm_group_eligible(a[i]) || (a[i].k_tiles != nullptr) != (a[0].k_tiles != nullptr)) return g;
  g.ktab = a[0].k_tiles != nullptr;
  // K the k loop runs over: the compacted block list of a product with a K-block table
  auto keff = [](const tfasr_gemm_args& p) -> long { return p.k_tiles ? 256L * p.n_k_tiles : (long)p.K; };
  long total = 0, kmax = 0;
  for (int i = 0; i < n; ++i) {
    g.t.gx[i] = (int)gemm_ceil(a[i].N, 128);
    g.t.gy[i] = (int)gemm_ceil(a[i].M, GEMM_BM);
    total += (long)g.t.gx[i] * g.t.gy[i];
    kmax = std::max(kmax, keff(a[i]));
  }
  if (total > 0x7fffffffL / 8) return g;  // more tiles than a grid holds
  // k-split shared by the group: fill the resident slots (2 workgroups per CU) once.
  // A group that runs BESIDE another stream's dependent chain (the block executor's weight-gradient stream) takes 1.25 slots per CU
  // (256 / 320 / 512 slots for those groups alone: -0.04 / -0.09 / 0 ms per step).
  // A group of LONG products in line (the nine shifted conv2 weight gradients: K = B T2 F2 = 500 k rows, 36 tiles) also wants about one
  // workgroup per CU: with 512 slots its 14 k-slices per tile were 8 M atomics and the slices' workgroups drifted apart in L2 - 256 / 320
  // slots for every group of the step: -0.28 / -0.33 ms per step against 512, of which the block groups beside the chain are 0.04.
  const long slots = (beside || kmax >= 131072) ? ncu * 5L / 4 : 2L * ncu;
  const long split = std::max(1L, slots / std::max(total, 1L));
  // units (product, k-slice), largest first, each onto the XCD with the fewest slots taken so far
  struct U { int q, ks, tiles; };
  U units[GEMM_GROUP_MAX * 64];
  int nu = 0;
  for (int i = 0; i < n; ++i) {
    g.split[i] = (int)std::min(64L, std::max(1L, std::min(split, keff(a[i]) / 512)));
    for (int k2 = 0; k2 < g.split[i]; ++k2) units[nu++] = U{i, k2, g.t.gx[i] * g.t.gy[i]};
  }
  for (int i = 1; i < nu; ++i) {  // insertion sort by tiles, descending
    const U v = units[i];
    int j = i - 1;
    while (j >= 0 && units[j].tiles < v.tiles) { units[j + 1] = units[j]; --j; }
    units[j + 1] = v;
  }
  int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < nu; ++i) {
    int best = 0;
    for (int x = 1; x < 8; ++x)
      if (load[x] < load[best]) best = x;
    const int c = g.t.nunit[best];
    if (c >= GEMM_GROUP_UNITS) return g;  // more units than an XCD's list holds: one by one
    g.t.uq[best][c] = (short)units[i].q;
    g.t.uks[best][c] = (short)units[i].ks;
    g.t.j0[best][c] = load[best];
    load[best] += units[i].tiles;
    g.t.j0[best][c + 1] = load[best];
    g.t.nunit[best] = c + 1;
  }
  g.workgroups = 8 * *std::max_element(load, load + 8);
  g.lds_bytes = GEMM_GROUP_LDS;
  g.status = TFASR_STATUS_SUCCESS;
  return g;
}

// tfasr_gemm_group: chunks of GEMM_GROUP_MAX, each one launch or one by one.  Returns the status of the whole call; *launches = its launch count.
inline int gemm_group_route(const tfasr_gemm_args* a, int n, int ncu, bool beside, bool allow_big, int* launches) {
  *launches = 0;
  if (!a || n <= 0) return TFASR_STATUS_INVALID_VALUE;
  for (int i = 0; i < n; i += GEMM_GROUP_MAX) {
    const int m = std::min(n - i, GEMM_GROUP_MAX);
    if (gemm_group_plan(a + i, m, ncu, beside).status == TFASR_STATUS_SUCCESS) { *launches += 1; continue; }
    for (int j = 0; j < m; ++j) {
      const GemmRoute r = gemm_route(a[i + j], ncu, allow_big);
      if (r.status != TFASR_STATUS_SUCCESS) return r.status;
      *launches += r.launches;
    }
  }
  return TFASR_STATUS_SUCCESS;
}
