// Log-probability passes shared by the losses and the forced alignment (csrc/align.hip).  Library-internal: not part of the C ABI.
#pragma once
#include "common.h"

namespace tfasr_detail {

// lse / blank / truth log-probabilities of every lattice node, dense [B,T,U1] (cell_off == nullptr) or packed, into three arrays of
// `nrows` floats: from the logits (f32 | bf16), or, with lse_part / pick, from the vocabulary GEMM's statistics epilogue (csrc/rnnt_loss.hip).
__attribute__((visibility("hidden"))) int rnnt_lattice_logprobs(const void* logits, const int32_t* labels, const int32_t* label_len,
                                                                const int32_t* logit_len, const long* cell_off, long nrows, int B, int T, int U1,
                                                                int V, int dtype, const float* lse_part, int lse_parts, const float* pick,
                                                                float* lse, float* blank_lp, float* truth_lp, hipStream_t stream);

// log-sum-exp of every row of logits [rows, V] (csrc/ctc.hip)
__attribute__((visibility("hidden"))) int ctc_row_lse(const void* logits, float* lse, long rows, int V, int dtype, hipStream_t stream);

// the same lse (bit for bit) with the entropy of every row, by the greedy detail decoder's frame function (csrc/ctc.hip)
__attribute__((visibility("hidden"))) int ctc_row_lse_entropy(const void* logits, float* lse, float* entropy, long rows, int V, int dtype,
                                                              hipStream_t stream);

}  // namespace tfasr_detail
