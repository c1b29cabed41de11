// Logits processors and stop sequences of generate() on the device (HF GenerationMixin semantics, transformers 5.x).
//
// lmod_logits_process_bf16 edits one step's bf16 logits [R, V] in place from the row's token history, one workgroup per row, in HF's
// processor order; the phases of a row are separated by barriers, so a ban always lands on top of a penalised value:
//   1. repetition penalty (penalty != 1, history not empty): every DISTINCT history token t in [0, V) gets x = x < 0 ? x * p : x / p
//      once, however often it occurs.  A V-bit bitmap in LDS decides: the thread whose atomic-or first sets t's bit applies the
//      penalty.  fp32 on the bf16 value with IEEE multiply / divide, one round-to-nearest-even back to bf16 (f2bf).
//   2. no-repeat n-gram (ngram = n > 0, history of at least n tokens): for every window hist[j .. j+n-1] whose first n-1 tokens
//      equal the last n-1 tokens of the history, ban the window's last token.  n = 1 bans every token seen.
//   3. bad words (a table of n_bad sequences): a one-token entry is always banned; a longer entry's last token is banned when the
//      history holds at least as many tokens as the entry and ends with the entry's other tokens.
//   4. min new tokens: ban eos while n_gen < min_new (eos < 0: no such token).
// A ban stores bf16 -inf (lmod_sample_bf16 gives it weight 0; lmod_row_argmax_bf16 never prefers it to a finite logit).  History
// ids are compared as plain integers (the negative image placeholder included); an id outside [0, V) is never penalised or banned.
// Elements that no processor touches are not written.
//
// lmod_gen_push_stop is the per-step bookkeeping of the same loop: one thread per row appends the step's token to the history and
// decides whether the row is done (EOS or a stop sequence over the GENERATED tokens only).
#include "common.h"
#include "stop_match.h"

#define LOGITS_THREADS 256
#define LOGITS_LDS_MAX 65536
#define BF16_NEG_INF ((bf16_t)0xff80u)

struct LogitsArgs {
  bf16_t* x; long long ld; int V;
  const int* hist; int ld_hist; const int* n_hist; const int* n_gen;
  float penalty; int ngram;
  const int* bad_flat; const int* bad_off; int n_bad;
  int min_new, eos, use_bitmap;
};

// One row by its workgroup.  penalty / ngram / min_new: the row's own; use_bitmap: the launch has the V-bit LDS bitmap and this row's
// penalty differs from 1.  Everything a branch around a barrier depends on is uniform over the workgroup.
__device__ __forceinline__ void logits_process_row(const LogitsArgs& a, int r, float penalty, int ngram, int min_new, int use_bitmap,
                                                   uint32_t* seen) {
  const int tid = threadIdx.x;
  bf16_t* row = a.x + (long long)r * a.ld;
  const int* h = a.hist + (long long)r * a.ld_hist;
  const int n = min(max(a.n_hist[r], 0), a.ld_hist);
  const int V = a.V;
  // 1. repetition penalty, once per distinct token
  if (use_bitmap && n > 0) {
    const int words = (V + 31) >> 5;
    for (int i = tid; i < words; i += LOGITS_THREADS) seen[i] = 0u;
    __syncthreads();
    const float p = penalty;
    for (int i = tid; i < n; i += LOGITS_THREADS) {
      const int t = h[i];
      if (t < 0 || t >= V) continue;
      const uint32_t bit = 1u << (t & 31);
      if (atomicOr(&seen[t >> 5], bit) & bit) continue;
      const float v = bf2f(row[t]);
      row[t] = f2bf(v < 0.f ? v * p : v / p);
    }
  }
  __syncthreads();
  // 2. no-repeat n-gram: windows that start with the history's last n-1 tokens ban their last token
  const int g = ngram;
  if (g > 0 && n >= g) {
    const int* suffix = h + n - (g - 1);
    for (int j = tid; j + g <= n; j += LOGITS_THREADS) {
      bool same = true;
      for (int q = 0; q < g - 1 && same; ++q) same = h[j + q] == suffix[q];
      const int t = h[j + g - 1];
      if (same && t >= 0 && t < V) row[t] = BF16_NEG_INF;
    }
  }
  __syncthreads();
  // 3. bad words / suppressed tokens
  for (int e = tid; e < a.n_bad; e += LOGITS_THREADS) {
    const int o = a.bad_off[e], len = a.bad_off[e + 1] - o;
    if (len < 1 || (len > 1 && len > n)) continue;
    bool same = true;
    for (int q = 0; q < len - 1 && same; ++q) same = h[n - (len - 1) + q] == a.bad_flat[o + q];
    const int t = a.bad_flat[o + len - 1];
    if (same && t >= 0 && t < V) row[t] = BF16_NEG_INF;
  }
  __syncthreads();
  // 4. min new tokens
  if (tid == 0 && a.eos >= 0 && a.eos < V && a.n_gen[r] < min_new) row[a.eos] = BF16_NEG_INF;
}

__global__ __launch_bounds__(LOGITS_THREADS) void logits_process_kernel(LogitsArgs a) {
  extern __shared__ uint32_t seen[];                  // V bits: tokens the penalty phase has already handled
  logits_process_row(a, blockIdx.x, a.penalty, a.ngram, a.min_new, a.use_bitmap, seen);
}

// lmod_logits_process_rows_bf16: penalty / ngram / min_new of row r from device arrays.  a.use_bitmap: the host's "some penalty != 1"
// (the bitmap is allocated); a row whose own penalty is 1 skips the penalty phase, as the scalar kernel does for penalty == 1.
__global__ __launch_bounds__(LOGITS_THREADS) void logits_process_rows_kernel(LogitsArgs a, const float* __restrict__ penalty,
                                                                              const int* __restrict__ ngram,
                                                                              const int* __restrict__ min_new) {
  extern __shared__ uint32_t seen[];
  const int r = blockIdx.x;
  const float p = penalty[r];
  logits_process_row(a, r, p, ngram[r], min_new[r], a.use_bitmap && p != 1.0f, seen);
}

// One row by one thread: sequences [0, n_stop) of the table, then [own_first, own_first + own_count).
__device__ __forceinline__ void gen_push_stop_row(int r, int* __restrict__ tokens, int* __restrict__ done, int* __restrict__ hist,
                                                  int ld_hist, int* __restrict__ n_hist, const int* __restrict__ n_prompt,
                                                  int* __restrict__ n_gen, int eos, int pad, const int* __restrict__ stop_flat,
                                                  const int* __restrict__ stop_off, int n_stop, int own_first, int own_count) {
  if (done[r]) { tokens[r] = pad; return; }
  int* h = hist + (long long)r * ld_hist;
  const int t = tokens[r];
  int n = n_hist[r];
  if (n < 0 || n >= ld_hist) return;                      // the caller sizes the history; a full row is left as it is, never overrun
  h[n++] = t;
  n_hist[r] = n;
  n_gen[r] += 1;
  const int first = max(n_prompt[r], 0);                  // generated tokens are h[first .. n)
  bool fin = eos >= 0 && t == eos;
  if (!fin) fin = stop_match(h, n, first, stop_flat, stop_off, 0, n_stop);
  if (!fin && own_count > 0) fin = stop_match(h, n, first, stop_flat, stop_off, own_first, own_first + own_count);
  if (fin) done[r] = 1;
}

__global__ __launch_bounds__(LOGITS_THREADS) void gen_push_stop_kernel(int* __restrict__ tokens, int* __restrict__ done,
                                                                        int* __restrict__ hist, int ld_hist, int* __restrict__ n_hist,
                                                                        const int* __restrict__ n_prompt, int* __restrict__ n_gen,
                                                                        int eos, int pad, const int* __restrict__ stop_flat,
                                                                        const int* __restrict__ stop_off, int n_stop, int R) {
  const int r = blockIdx.x * LOGITS_THREADS + threadIdx.x;
  if (r >= R) return;
  gen_push_stop_row(r, tokens, done, hist, ld_hist, n_hist, n_prompt, n_gen, eos, pad, stop_flat, stop_off, n_stop, 0, 0);
}

// lmod_gen_push_stop_rows: row r also tests its own range of the table.  A range that leaves [0, n_table) is not tested at all: no
// index is clamped.
__global__ __launch_bounds__(LOGITS_THREADS) void gen_push_stop_rows_kernel(int* __restrict__ tokens, int* __restrict__ done,
                                                                             int* __restrict__ hist, int ld_hist,
                                                                             int* __restrict__ n_hist, const int* __restrict__ n_prompt,
                                                                             int* __restrict__ n_gen, int eos, int pad,
                                                                             const int* __restrict__ stop_flat,
                                                                             const int* __restrict__ stop_off, int n_call, int n_table,
                                                                             const int* __restrict__ stop_first,
                                                                             const int* __restrict__ stop_count, int R) {
  const int r = blockIdx.x * LOGITS_THREADS + threadIdx.x;
  if (r >= R) return;
  const int f = stop_first[r];
  int c = stop_count[r];
  if (f < 0 || c < 0 || f > n_table || c > n_table - f) c = 0;
  gen_push_stop_row(r, tokens, done, hist, ld_hist, n_hist, n_prompt, n_gen, eos, pad, stop_flat, stop_off, n_call, f, c);
}

extern "C" {

int lmod_logits_process_bf16(void* logits, long long ld, int V, int R, const int* hist, int ld_hist, const int* n_hist,
                             const int* n_gen, float penalty, int ngram, const int* bad_flat, const int* bad_off, int n_bad,
                             int min_new, int eos, hipStream_t stream) {
  if (R < 0 || V < 1 || ld < V || ld_hist < 0 || ngram < 0 || n_bad < 0 || !(penalty > 0.f)) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!logits || !hist || !n_hist || !n_gen || (n_bad > 0 && (!bad_flat || !bad_off))) return LMOD_EINVAL;
  LogitsArgs a;
  a.x = (bf16_t*)logits; a.ld = ld; a.V = V;
  a.hist = hist; a.ld_hist = ld_hist; a.n_hist = n_hist; a.n_gen = n_gen;
  a.penalty = penalty; a.ngram = ngram;
  a.bad_flat = bad_flat; a.bad_off = bad_off; a.n_bad = n_bad;
  a.min_new = min_new; a.eos = eos;
  a.use_bitmap = penalty != 1.0f;
  const long long lds = a.use_bitmap ? 4LL * ((V + 31) >> 5) : 0;
  if (lds > LOGITS_LDS_MAX) return LMOD_EUNSUPPORTED;
  hipLaunchKernelGGL(logits_process_kernel, dim3(R), dim3(LOGITS_THREADS), (size_t)lds, stream, a);
  return lmod_launch_status();
}

int lmod_logits_process_rows_bf16(void* logits, long long ld, int V, int R, const int* hist, int ld_hist, const int* n_hist,
                                  const int* n_gen, const float* penalty, const int* ngram, const int* min_new, int any_penalty,
                                  const int* bad_flat, const int* bad_off, int n_bad, int eos, hipStream_t stream) {
  if (R < 0 || V < 1 || ld < V || ld_hist < 0 || n_bad < 0) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!logits || !hist || !n_hist || !n_gen || !penalty || !ngram || !min_new || (n_bad > 0 && (!bad_flat || !bad_off)))
    return LMOD_EINVAL;
  LogitsArgs a;
  a.x = (bf16_t*)logits; a.ld = ld; a.V = V;
  a.hist = hist; a.ld_hist = ld_hist; a.n_hist = n_hist; a.n_gen = n_gen;
  a.penalty = 1.0f; a.ngram = 0;
  a.bad_flat = bad_flat; a.bad_off = bad_off; a.n_bad = n_bad;
  a.min_new = 0; a.eos = eos;
  a.use_bitmap = any_penalty != 0;
  const long long lds = a.use_bitmap ? 4LL * ((V + 31) >> 5) : 0;
  if (lds > LOGITS_LDS_MAX) return LMOD_EUNSUPPORTED;
  hipLaunchKernelGGL(logits_process_rows_kernel, dim3(R), dim3(LOGITS_THREADS), (size_t)lds, stream, a, penalty, ngram, min_new);
  return lmod_launch_status();
}

int lmod_gen_push_stop(int* tokens, int* done, int* hist, int ld_hist, int* n_hist, const int* n_prompt, int* n_gen, int eos,
                       int pad, const int* stop_flat, const int* stop_off, int n_stop, int R, hipStream_t stream) {
  if (R < 0 || ld_hist < 0 || n_stop < 0) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!tokens || !done || !hist || !n_hist || !n_prompt || !n_gen || (n_stop > 0 && (!stop_flat || !stop_off))) return LMOD_EINVAL;
  hipLaunchKernelGGL(gen_push_stop_kernel, dim3((R + LOGITS_THREADS - 1) / LOGITS_THREADS), dim3(LOGITS_THREADS), 0, stream, tokens,
                     done, hist, ld_hist, n_hist, n_prompt, n_gen, eos, pad, stop_flat, stop_off, n_stop, R);
  return lmod_launch_status();
}

int lmod_gen_push_stop_rows(int* tokens, int* done, int* hist, int ld_hist, int* n_hist, const int* n_prompt, int* n_gen, int eos,
                            int pad, const int* stop_flat, const int* stop_off, int n_call, int n_table, const int* stop_first,
                            const int* stop_count, int R, hipStream_t stream) {
  if (R < 0 || ld_hist < 0 || n_call < 0 || n_table < n_call) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!tokens || !done || !hist || !n_hist || !n_prompt || !n_gen || !stop_first || !stop_count ||
      (n_table > 0 && (!stop_flat || !stop_off))) return LMOD_EINVAL;
  hipLaunchKernelGGL(gen_push_stop_rows_kernel, dim3((R + LOGITS_THREADS - 1) / LOGITS_THREADS), dim3(LOGITS_THREADS), 0, stream,
                     tokens, done, hist, ld_hist, n_hist, n_prompt, n_gen, eos, pad, stop_flat, stop_off, n_call, n_table, stop_first,
                     stop_count, R);
  return lmod_launch_status();
}

}  // extern "C"
