// Step processors of on-device decoding (fairseq2's NGramRepeatBlockProcessor / BannedSequenceProcessor): the ids a row
// may not take next, formed from the row's sequence so far (prompt included) by the workgroup that selects its token.
// Used by vocab_select_banned_kernel (decoder.hip) and sample_rows_kernel<true> (sampling.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace smi {

// Every banned id of the sequence s[0 .. L) (in LDS), handed to ban(id); the threads tid = 0 .. nthr-1 of the workgroup share
// the windows and the banned sequences.  An id may be handed over more than once.
//   n-gram (n >= 1): for every window start i in [0, L - n] with s[i, i + n - 1) == s[L - n + 1, L), ban s[i + n - 1]
//   banned sequence b: ban b[-1] when the last len(b) - 1 tokens of s equal b[:-1] (a prefix longer than s never matches)
template <class F>
__device__ __forceinline__ void step_proc_bans(const StepProcDev& p, const int32_t* s, int L, int tid, int nthr, F&& ban) {
  const int n = p.ngram;
  if (n > 0) {
    for (int i = tid; i <= L - n; i += nthr) {
      bool eq = true;
      for (int j = 0; j < n - 1 && eq; ++j) eq = s[i + j] == s[L - n + 1 + j];
      if (eq) ban(s[i + n - 1]);
    }
  }
  for (int q = tid; q < p.num_banned; q += nthr) {
    const int b0 = p.offsets[q], pl = p.offsets[q + 1] - b0 - 1;  // prefix length
    if (pl > L) continue;
    bool eq = true;
    for (int j = 0; j < pl && eq; ++j) eq = s[L - pl + j] == p.tokens[b0 + j];
    if (eq) ban(p.tokens[b0 + pl]);
  }
}

}  // namespace smi
