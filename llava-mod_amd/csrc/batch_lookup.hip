// Prompt-lookup decoding under continuous batching (generate_batch(prompt_lookup_num_tokens=k)): the round bookkeeping of a batch
// whose slots are admitted, run and ended independently.  The draft is lmod_ngram_draft's (lookup.hip), the verification pass the
// assisted loop's (lmod_attn_append, lmod_row_argmax_bf16); what generate()'s lookup loop leaves to the host - a slot that ends in
// the middle of an accepted run (its own budget, EOS, a stop sequence), an idle slot that must not creep forward in the cache, a
// freshly admitted slot without a pending token - happens here, so a round has one read-back and no host -> device copy.
//   lmod_batch_lookup_first - the first token of freshly admitted slots (done == 0 && n_gen == 0): it becomes the pending token;
//   lmod_batch_lookup_round - acceptance, emission into the history, every end condition, the cache length, the [B, k+6] block.
// Both: int32 and exact, one thread per slot, no atomics, no workspace.  Every index is checked, none is clamped: a slot whose
// history row is full is left as it is and marked done.  The arrays are those of lmod_slot_admit / lmod_gen_push_stop.
#include "common.h"
#include "stop_match.h"

#define BLOOKUP_THREADS 256
#define BLOOKUP_T_MAX 16                     // APPEND_T_MAX of csrc/append.hip: the verification chunk holds k + 1 <= 16 tokens

struct BatchLookupArgs {
  int* done; int* hist; int ld_hist; int* n_hist; const int* n_prompt; int* n_gen; const int* budget;
  int eos; int pad; const int* stop_flat; const int* stop_off; int n_stop; int B;
};

// is the slot finished by the token that has just been appended (h[0 .. n) is its history, g its generated count)?
__device__ __forceinline__ bool blookup_ends(const BatchLookupArgs& a, int s, const int* h, int n, int t, int g) {
  if (a.eos >= 0 && t == a.eos) return true;
  if (stop_match(h, n, max(a.n_prompt[s], 0), a.stop_flat, a.stop_off, 0, a.n_stop)) return true;
  return g >= a.budget[s];
}

__global__ __launch_bounds__(BLOOKUP_THREADS) void batch_lookup_first_kernel(BatchLookupArgs a, const int* __restrict__ tokens,
                                                                              int* __restrict__ first_tok) {
  const int s = blockIdx.x * BLOOKUP_THREADS + threadIdx.x;
  if (s >= a.B) return;
  first_tok[s] = -1;
  if (a.done[s] != 0 || a.n_gen[s] != 0) return;          // not fresh: nothing else is touched
  const int n = a.n_hist[s];
  if (n < 0 || n >= a.ld_hist) { a.done[s] = 1; return; }  // a full history row: left as it is, the slot ends
  int* h = a.hist + (long long)s * a.ld_hist;
  const int t = tokens[s];
  h[n] = t;
  a.n_hist[s] = n + 1;
  a.n_gen[s] = 1;
  first_tok[s] = t;
  if (blookup_ends(a, s, h, n + 1, t, 1)) a.done[s] = 1;
}

// block row: columns 0..k emitted tokens then pad | k+1 n_acc | k+2 n_emit | k+3 next pending token (pad when fin) | k+4 fin |
// k+5 first_tok.  cache_lens[s] arrives as L0 + k + 1 (the verification pass appended k + 1 positions to every row).
__global__ __launch_bounds__(BLOOKUP_THREADS) void batch_lookup_round_kernel(BatchLookupArgs a, const int* __restrict__ draft,
                                                                              const int* __restrict__ target,
                                                                              const int* __restrict__ first_tok, int k,
                                                                              int* __restrict__ cache_lens, int* __restrict__ block) {
  const int s = blockIdx.x * BLOOKUP_THREADS + threadIdx.x;
  if (s >= a.B) return;
  int* b = block + (long long)s * (k + 6);
  const int L0 = cache_lens[s] - (k + 1);
  b[k + 5] = first_tok[s];
  if (a.done[s] != 0 || L0 < 0) {                          // an idle slot (or lens that no verification pass left: the slot ends)
    for (int j = 0; j <= k; ++j) b[j] = a.pad;
    b[k + 1] = 0; b[k + 2] = 0; b[k + 3] = a.pad; b[k + 4] = 1;
    a.done[s] = 1;
    if (L0 >= 0) cache_lens[s] = L0;                       // it stays where it is however long the call lasts
    return;
  }
  const int* d = draft + (long long)s * k;
  const int* t = target + (long long)s * (k + 1);
  int n_acc = 0;
  while (n_acc < k && d[n_acc] == t[n_acc]) ++n_acc;
  int* h = a.hist + (long long)s * a.ld_hist;
  int n = a.n_hist[s], g = a.n_gen[s], n_emit = 0, last = a.pad;
  bool fin = false;
  for (int j = 0; j <= n_acc && !fin; ++j) {
    if (n < 0 || n >= a.ld_hist) { fin = true; break; }   // a full history row: nothing more is written, the slot ends
    const int c = j < n_acc ? d[j] : t[n_acc];
    h[n++] = c;
    ++g;
    b[n_emit++] = c;
    last = c;
    fin = blookup_ends(a, s, h, n, c, g);
  }
  for (int j = n_emit; j <= k; ++j) b[j] = a.pad;
  b[k + 1] = n_acc; b[k + 2] = n_emit; b[k + 3] = fin ? a.pad : last; b[k + 4] = fin ? 1 : 0;
  if (n_emit > 0) { a.n_hist[s] = n; a.n_gen[s] = g; }
  a.done[s] = fin ? 1 : 0;
  cache_lens[s] = L0 + n_emit;                             // the prompt and every emitted token but the last: plain greedy's invariant
}

static int blookup_args(BatchLookupArgs& a, int* done, int* hist, int ld_hist, int* n_hist, const int* n_prompt, int* n_gen,
                        const int* budget, int eos, int pad, const int* stop_flat, const int* stop_off, int n_stop, int B) {
  if (B < 0 || ld_hist < 0 || n_stop < 0) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!done || !hist || !n_hist || !n_prompt || !n_gen || !budget || (n_stop > 0 && (!stop_flat || !stop_off))) return LMOD_EINVAL;
  a.done = done; a.hist = hist; a.ld_hist = ld_hist; a.n_hist = n_hist; a.n_prompt = n_prompt; a.n_gen = n_gen; a.budget = budget;
  a.eos = eos; a.pad = pad; a.stop_flat = stop_flat; a.stop_off = stop_off; a.n_stop = n_stop; a.B = B;
  return LMOD_OK;
}

extern "C" {

int lmod_batch_lookup_first(const int* tokens, int* done, int* hist, int ld_hist, int* n_hist, const int* n_prompt, int* n_gen,
                            const int* budget, int eos, const int* stop_flat, const int* stop_off, int n_stop, int* first_tok, int B,
                            hipStream_t stream) {
  BatchLookupArgs a;
  const int rc = blookup_args(a, done, hist, ld_hist, n_hist, n_prompt, n_gen, budget, eos, 0, stop_flat, stop_off, n_stop, B);
  if (rc != LMOD_OK || B == 0) return rc;
  if (!tokens || !first_tok) return LMOD_EINVAL;
  hipLaunchKernelGGL(batch_lookup_first_kernel, dim3((B + BLOOKUP_THREADS - 1) / BLOOKUP_THREADS), dim3(BLOOKUP_THREADS), 0, stream, a,
                     tokens, first_tok);
  return lmod_launch_status();
}

int lmod_batch_lookup_round(const int* draft, const int* target, const int* first_tok, int k, int* done, int* hist, int ld_hist,
                            int* n_hist, const int* n_prompt, int* n_gen, const int* budget, int* cache_lens, int eos, int pad,
                            const int* stop_flat, const int* stop_off, int n_stop, int* block, int B, hipStream_t stream) {
  if (k < 1 || k >= BLOOKUP_T_MAX) return LMOD_EINVAL;
  BatchLookupArgs a;
  const int rc = blookup_args(a, done, hist, ld_hist, n_hist, n_prompt, n_gen, budget, eos, pad, stop_flat, stop_off, n_stop, B);
  if (rc != LMOD_OK || B == 0) return rc;
  if (!draft || !target || !first_tok || !cache_lens || !block) return LMOD_EINVAL;
  hipLaunchKernelGGL(batch_lookup_round_kernel, dim3((B + BLOOKUP_THREADS - 1) / BLOOKUP_THREADS), dim3(BLOOKUP_THREADS), 0, stream, a,
                     draft, target, first_tok, k, cache_lens, block);
  return lmod_launch_status();
}

}  // extern "C"
