// Prompt-lookup decoding (HF generate(prompt_lookup_num_tokens=k), PromptLookupCandidateGenerator): the drafter that needs no second
// model.  The draft of a round is the continuation of an earlier occurrence of the row's trailing n-gram in the row's own token
// history, found on the device; the verification half is the assisted loop's (lmod_attn_append, lmod_row_argmax_bf16,
// lmod_spec_accept).  Two entry points, both int32 and exact, no atomics, no workspace:
//   lmod_ngram_draft     - one workgroup per row: the match, the draft and the verification chunk;
//   lmod_hist_push_block - one thread per row: the round's emitted tokens (lmod_spec_accept's block) appended to the history.
//
// ---------------------------------------------------------------------------- lmod_ngram_draft: one pass for every n
// L = n_hist[r], tail_j = hist[L-1-j].  For an END position e in [1, L-1] let m(e) = the number of j < min(nmax, e) with
// hist[e-1-j] == tail_j for all smaller j too (the common suffix of hist[0:e] and hist[0:L], capped at nmax = min(max_ngram, L-1)).
// A window of n tokens starting at i equals the trailing n-gram iff m(i+n) >= n, and e = i+n <= L-1 is the "continuation is not
// empty" condition, so the smallest matching start for n is (the smallest e with m(e) >= n) - n: ONE strided pass over e keeps, per
// thread, the smallest such e for every n = 1..8 (e ascends within a thread: the first hit is its minimum), a wave min over the
// 8 values (shuffles) and a min over the 4 waves through LDS give the block-wide minima over ALL strides, and the largest n that
// has one wins.  Most positions fail on their first token, so the pass costs about one history read.  The continuation starts at e.
#include "common.h"

#define LOOKUP_THREADS 256
#define LOOKUP_WAVES (LOOKUP_THREADS / 64)
#define LOOKUP_NGRAM_MAX 8
#define LOOKUP_T_MAX 16                      // APPEND_T_MAX of csrc/append.hip: the verification chunk holds k + 1 <= 16 tokens
#define LOOKUP_NONE 0x7fffffff

__global__ __launch_bounds__(LOOKUP_THREADS) void ngram_draft_kernel(const int* __restrict__ hist, int ld_hist,
                                                                     const int* __restrict__ n_hist, const int* __restrict__ done,
                                                                     int k, int max_ngram, int V, int* __restrict__ draft,
                                                                     int* __restrict__ chunk, int* __restrict__ n_draft) {
  __shared__ int s_best[LOOKUP_WAVES][LOOKUP_NGRAM_MAX];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int* h = hist + (long long)r * ld_hist;
  int* dr = draft + (long long)r * k;
  int* ch = chunk + (long long)r * (k + 1);
  const int L = n_hist[r];
  // all of these are functions of the row alone: the early exit is workgroup-uniform and comes before the only barrier
  if (L < 2 || L > ld_hist || done[r] != 0) {
    const int pending = (L >= 1 && L <= ld_hist) ? h[L - 1] : 0;
    for (int j = tid; j < k; j += LOOKUP_THREADS) dr[j] = -1;
    for (int j = tid; j <= k; j += LOOKUP_THREADS) ch[j] = pending;
    if (tid == 0) n_draft[r] = 0;
    return;
  }
  const int nmax = min(max_ngram, L - 1);
  int tail[LOOKUP_NGRAM_MAX], best[LOOKUP_NGRAM_MAX];
#pragma unroll
  for (int j = 0; j < LOOKUP_NGRAM_MAX; ++j) {
    tail[j] = j < nmax ? h[L - 1 - j] : 0;
    best[j] = LOOKUP_NONE;
  }
  for (int e = 1 + tid; e < L; e += LOOKUP_THREADS) {
    if (h[e - 1] != tail[0]) continue;
    int m = 1;
#pragma unroll
    for (int j = 1; j < LOOKUP_NGRAM_MAX; ++j)
      if (m == j && j < nmax && j < e && h[e - 1 - j] == tail[j]) m = j + 1;
#pragma unroll
    for (int j = 0; j < LOOKUP_NGRAM_MAX; ++j)
      if (j < m) best[j] = min(best[j], e);
  }
#pragma unroll
  for (int j = 0; j < LOOKUP_NGRAM_MAX; ++j) {
    int v = best[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    if ((tid & 63) == 0) s_best[tid >> 6][j] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  int start = LOOKUP_NONE;                     // where the continuation of the winning window begins
  for (int n = nmax; n >= 1 && start == LOOKUP_NONE; --n) {
    int v = s_best[0][n - 1];
#pragma unroll
    for (int w = 1; w < LOOKUP_WAVES; ++w) v = min(v, s_best[w][n - 1]);
    start = v;
  }
  const int pending = h[L - 1];
  int nd = 0;
  if (start != LOOKUP_NONE) {
    const int avail = min(k, L - start);
    while (nd < avail && (unsigned)h[start + nd] < (unsigned)V) ++nd;     // cut before the first id outside [0, V)
  }
  for (int j = 0; j < k; ++j) {
    const int t = j < nd ? h[start + j] : -1;
    dr[j] = t;
    ch[j + 1] = j < nd ? t : pending;
  }
  ch[0] = pending;
  n_draft[r] = nd;
}

// block [R, k+5] is lmod_spec_accept's output: columns 0..k the emitted tokens, k+2 their count.  A row whose emission would pass
// ld_hist (or whose count is outside [0, k+1]: not a block of this k) is left as it is.
__global__ __launch_bounds__(LOOKUP_THREADS) void hist_push_block_kernel(const int* __restrict__ block, int k, int* __restrict__ hist,
                                                                         int ld_hist, int* __restrict__ n_hist, int R) {
  const int r = blockIdx.x * LOOKUP_THREADS + threadIdx.x;
  if (r >= R) return;
  const int* b = block + (long long)r * (k + 5);
  const int ne = b[k + 2], L = n_hist[r];
  if (ne < 1 || ne > k + 1 || L < 0 || L > ld_hist - ne) return;
  int* h = hist + (long long)r * ld_hist + L;
  for (int j = 0; j < ne; ++j) h[j] = b[j];
  n_hist[r] = L + ne;
}

extern "C" {

int lmod_ngram_draft(const int* hist, int ld_hist, const int* n_hist, const int* done, int R, int k, int max_ngram, int V, int* draft,
                     int* chunk, int* n_draft, hipStream_t stream) {
  if (R < 0 || k < 1 || k >= LOOKUP_T_MAX || max_ngram < 1 || max_ngram > LOOKUP_NGRAM_MAX || ld_hist < 0 || V < 1) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!hist || !n_hist || !done || !draft || !chunk || !n_draft) return LMOD_EINVAL;
  hipLaunchKernelGGL(ngram_draft_kernel, dim3(R), dim3(LOOKUP_THREADS), 0, stream, hist, ld_hist, n_hist, done, k, max_ngram, V, draft,
                     chunk, n_draft);
  return lmod_launch_status();
}

int lmod_hist_push_block(const int* block, int k, int* hist, int ld_hist, int* n_hist, int R, hipStream_t stream) {
  if (R < 0 || k < 1 || k >= LOOKUP_T_MAX || ld_hist < 0) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!block || !hist || !n_hist) return LMOD_EINVAL;
  hipLaunchKernelGGL(hist_push_block_kernel, dim3((R + LOOKUP_THREADS - 1) / LOOKUP_THREADS), dim3(LOOKUP_THREADS), 0, stream, block, k,
                     hist, ld_hist, n_hist, R);
  return lmod_launch_status();
}

}  // extern "C"
