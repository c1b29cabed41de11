// The stop-sequence test of the generation bookkeeping kernels (lmod_gen_push_stop / _rows in logits.hip, lmod_batch_lookup_first /
// _round in batch_lookup.hip): one statement of the rule, shared.  A table of token sequences is `stop_flat` (all tokens back to
// back) and `stop_off` [n + 1] (sequence e is stop_flat[stop_off[e] .. stop_off[e+1])).
#pragma once

// does the history h[first .. n) of generated tokens end with one of the table's sequences [e0, e1)?
__device__ __forceinline__ bool stop_match(const int* h, int n, int first, const int* __restrict__ stop_flat,
                                           const int* __restrict__ stop_off, int e0, int e1) {
  bool fin = false;
  for (int e = e0; e < e1 && !fin; ++e) {
    const int o = stop_off[e], len = stop_off[e + 1] - o;
    if (len < 1 || n - len < first) continue;
    bool same = true;
    for (int q = 0; q < len && same; ++q) same = h[n - len + q] == stop_flat[o + q];
    fin = same;
  }
  return fin;
}
