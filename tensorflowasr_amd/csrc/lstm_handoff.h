// The hand-off protocol of the persistent, whole-grid LSTM kernels (lstm_persist.hip: training forward / backward of the prediction
// network; lstm_infer.hip: the one- or two-direction inference recurrence), and the host side they share: the shape rule, the residency
// check, the MT dispatch and the argument block of the per-step recurrent product.  Everything here is file-local.
//
// The workgroups of such a launch wait for each other across the device.  Per step a workgroup waits until every workgroup of its group
// has published the previous step's vector (one monotonic device-scope counter, relaxed polling by one lane, then ONE agent-scope
// acquire), computes, stores what it owns of this step's vector WRITE-THROUGH (sc1), drains, and adds 1 to the counter.
// Every spin is bounded by the wall clock; a timeout raises a flag (second word of the caller's 64-byte `Sync` record) that makes every
// workgroup leave - after overwriting what it owns of the remaining steps with NaN (no hang, and no silently wrong result: the step's loss /
// gradients are NaN); the caller can also check the word after a stream synchronisation.  The launch itself is refused unless the whole
// grid can be resident at once (`grid_fits`).
#pragma once
#include "common.h"
#include <string.h>
#include <type_traits>

bool tfasr_lstm_persist_on();  // lstm.hip: tfasr_lstm_set_persist / TFASR_LSTM_PERSIST

namespace {

typedef __attribute__((address_space(1))) unsigned int gu32;
#define AGENT_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

constexpr int PW = 16;          // hidden units per workgroup
constexpr int MAXKS = 32;       // k-steps of 32 per wave: P <= 1024
constexpr long long SPIN_TICKS = 100000000LL;  // 1 s of the 100 MHz wall clock

struct Sync { unsigned int count; unsigned int abort; unsigned int pad[14]; };

// wait until *count >= target (one lane polls, relaxed); false on timeout / abort
__device__ __forceinline__ bool wait_count(Sync* s, unsigned target) {
  bool ok = true;
  if (threadIdx.x == 0) {
    const long long t0 = wall_clock64();
    unsigned spins = 0;
    gu32* cnt = (gu32*)&s->count;
    gu32* abt = (gu32*)&s->abort;
    while (__hip_atomic_load(cnt, AGENT_RLX) < target) {
      __builtin_amdgcn_s_sleep(2);
      if ((++spins & 255u) == 0) {
        if (__hip_atomic_load(abt, AGENT_RLX) != 0u || wall_clock64() - t0 > SPIN_TICKS) {
          __hip_atomic_store(abt, 1u, AGENT_RLX);
          ok = false;
          break;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // ONE buffer_inv sc1 after the match: drops this CU's stale L1 lines
  }
  return __syncthreads_and(ok ? 1 : 0) != 0;
}

// every storing wave has drained its write-through stores -> one arrival
__device__ __forceinline__ void arrive(Sync* s) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add((gu32*)&s->count, 1u, AGENT_RLX);
}

// write-through (sc1) store of two adjacent bf16 values: visible at device scope once the storing wave has drained its stores
__device__ __forceinline__ void store_wt2(bf16_t* p, float lo, float hi) {
  __hip_atomic_store((gu32*)p, pack2_bf16(lo, hi), AGENT_RLX);
}
__device__ __forceinline__ void ld2(const bf16_t* p, float& lo, float& hi) {
  const unsigned v = *reinterpret_cast<const unsigned*>(p);
  lo = __uint_as_float(v << 16);
  hi = __uint_as_float(v & 0xffff0000u);
}

// A timed-out / aborted launch must not pass for a result: the leaving workgroup overwrites what it owns of the REMAINING
// steps with NaN, so the loss / the gradients of that step are NaN (what the reference's TerminateOnNaN watches) - no host read needed.
__device__ __forceinline__ void poison_rows(bf16_t* base, long row_stride, long step_stride, int t_lo, int t_hi, int B, int col0, int width) {
  for (int t = t_lo; t < t_hi; ++t)
    for (int i = threadIdx.x; i < B * width; i += blockDim.x)
      base[(long)(i / width) * row_stride + (long)t * step_stride + col0 + i % width] = (bf16_t)0x7FC0;
}

bool persist_ok(int B, int P, int dtype) { return dtype == TFASR_BF16 && B >= 1 && B <= 64 && P % 32 == 0 && P >= 32 && P <= 32 * MAXKS; }

// The workgroups of a launch wait for each other, so ALL of them must be resident at once (an ordinary launch gives no such promise):
// the launch is refused (UNSUPPORTED -> the caller's per-step kernels) unless resident-blocks-per-CU x CUs covers the grid.
// NECESSARY, NOT SUFFICIENT: the occupancy query knows nothing about kernels of OTHER streams that hold CUs when the launch starts (the
// encoder beside the prediction network); a workgroup that is not scheduled in time is caught by the kernels' wall-clock bound and abort
// flag (results poisoned, `sync` word 1 set), never by a hang.
// The answer depends on the kernel INSTANCE (the MT variants differ in registers, hence in blocks per CU), the device, the LDS size and the
// grid: a small per-thread table keyed on all four (the function-pointer type is the same for every MT, so a function-local static would
// be ONE entry shared by all instantiations - ADVICE r04).
template <typename KERNEL>
bool grid_fits(KERNEL kernel, int grid, size_t smem) {
  struct Entry { const void* fn; int dev; size_t smem; int grid; int ok; };
  static thread_local Entry cache[16];
  static thread_local int used = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const void* fn = reinterpret_cast<const void*>(kernel);
  for (int i = 0; i < used; ++i)
    if (cache[i].fn == fn && cache[i].dev == dev && cache[i].smem == smem && cache[i].grid == grid) return cache[i].ok != 0;
  int cus = 0, per_cu = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, smem) != hipSuccess) return false;
  const int ok = (long)per_cu * cus >= grid ? 1 : 0;
  Entry& e = cache[used < 16 ? used++ : (used = 1, 0)];  // (full: start over - 16 distinct launch shapes per thread do not occur in one model)
  e.fn = fn; e.dev = dev; e.smem = smem; e.grid = grid; e.ok = ok;
  return ok != 0;
}

// MT = ceil(B / 16) batch row tiles, 1 .. 4 (persist_ok caps B at 64), as a compile-time constant: f(std::integral_constant<int, MT>),
// so that an entry point names its kernel template once - `kernel<decltype(mt)::value>` - for the residency check and the launch
template <typename F>
int with_mt(int MT, F&& f) {
  switch (MT) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// the per-step routes' recurrent product h_prev [B, P] (row stride ld_h) @ R [P, 4P] -> hr [B, 4P] f32
inline tfasr_gemm_args recurrent_gemm_args(const void* h_prev, long ld_h, const void* rk, float* hr, int B, int P, int dtype) {
  tfasr_gemm_args a;
  memset(&a, 0, sizeof(a));
  a.A = h_prev; a.B = rk; a.D = hr; a.M = B; a.N = 4 * P; a.K = P; a.lda = ld_h; a.ldb = 4 * P; a.ldd = 4 * P;
  a.nb1 = a.nb2 = 1; a.alpha = 1.f; a.beta = 1.f; a.dtype = dtype; a.out_f32 = 1; a.split_k = 1;
  return a;
}

}  // namespace
