// Continuous batching of generate_batch() on the device: a request that has just been prefilled enters a slot of the running batch
// while the other slots keep decoding.
//   lmod_kv_admit_rows    - one launch over every K/V cache tensor of a model: dst[t][dst_row[r], 0:lens[r]] = src[t][r, 0:lens[r]]
//                           (the scatter that lmod_kv_gather_rows is not: the admission prefill's temporary cache into the slot cache);
//   lmod_slot_admit       - one launch that re-arms the admitted slots' generation state (token history, counters, done flag, cache
//                           length, request id): the arrays lmod_logits_process_bf16 / lmod_gen_push_stop work on;
//   lmod_request_uniform  - u[s] in [0, 1) as a pure function of (seed, req_id[s], n_gen[s]) (Philox4x32-10): a request's draws do
//                           not depend on its slot, its neighbours or the step it was admitted at;
//   lmod_request_uniform_rows - the same with the key and the counter's first word per slot (generate_batch with per-request
//                           parameters: a request with its own seed draws the same numbers in every call and at every list index).
#include "common.h"
#include "philox.h"

#define BATCH_THREADS 256

// ---------------------------------------------------------------------------------------------- cache row scatter
// grid (position blocks of P, R rows, ntensor tensors): the P positions of one row are one contiguous span of P * width bf16.
// A row whose length exceeds the bound the host vouched for, or whose slot is outside [0, B), is skipped: no position is clamped.
__global__ __launch_bounds__(BATCH_THREADS) void kv_admit_rows_kernel(void* const* __restrict__ dst, const void* const* __restrict__ src,
                                                                      const int* __restrict__ dst_row, const int* __restrict__ lens,
                                                                      int B, int smax_dst, int smax_src, int width, int max_len,
                                                                      int P) {
  const int t = blockIdx.z, r = blockIdx.y, p0 = blockIdx.x * P;
  const int n = lens[r];
  if (n > max_len || p0 >= n) return;
  const int dr = dst_row[r];
  if (dr < 0 || dr >= B) return;
  const int p1 = min(p0 + P, n);
  const u32x4* s = (const u32x4*)((const bf16_t*)src[t] + ((long long)r * smax_src + p0) * width);
  u32x4* d = (u32x4*)((bf16_t*)dst[t] + ((long long)dr * smax_dst + p0) * width);
  const int nv = (p1 - p0) * (width >> 3);
  int q = threadIdx.x;
  for (; q + 3 * BATCH_THREADS < nv; q += 4 * BATCH_THREADS) {             // four 16-byte loads in flight per lane
    const u32x4 a0 = s[q], a1 = s[q + BATCH_THREADS], a2 = s[q + 2 * BATCH_THREADS], a3 = s[q + 3 * BATCH_THREADS];
    d[q] = a0; d[q + BATCH_THREADS] = a1; d[q + 2 * BATCH_THREADS] = a2; d[q + 3 * BATCH_THREADS] = a3;
  }
  for (; q < nv; q += BATCH_THREADS) d[q] = s[q];
}

// ---------------------------------------------------------------------------------------------- slot state
// One workgroup per admitted request: the prompt ids go into the slot's history row (16-byte vectors when both rows are 16-byte
// aligned, int by int otherwise), thread 0 writes the slot's scalars.  A request whose prompt does not fit either row, or whose
// slot is outside [0, B), is skipped as a whole.
struct SlotAdmitArgs {
  const int* dst_row; const int* prompt_ids; int ld_prompt; const int* n_prompt_new; const int* lens_new; const int* req_new;
  int B;
  int* hist; int ld_hist; int* n_prompt; int* n_hist; int* n_gen; int* done; int* cache_lens; int* req_id;
  int vec;
};

__global__ __launch_bounds__(BATCH_THREADS) void slot_admit_kernel(SlotAdmitArgs a) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int s = a.dst_row[r], n = a.n_prompt_new[r];
  if (s < 0 || s >= a.B || n < 0 || n > a.ld_hist || n > a.ld_prompt) return;
  const int* p = a.prompt_ids + (long long)r * a.ld_prompt;
  int* h = a.hist + (long long)s * a.ld_hist;
  int done_ints = 0;
  if (a.vec) {
    const int nv = n >> 2;
    for (int q = tid; q < nv; q += BATCH_THREADS) ((u32x4*)h)[q] = ((const u32x4*)p)[q];
    done_ints = nv << 2;
  }
  for (int i = done_ints + tid; i < n; i += BATCH_THREADS) h[i] = p[i];
  if (tid == 0) {
    a.n_prompt[s] = n; a.n_hist[s] = n; a.n_gen[s] = 0; a.done[s] = 0;
    a.cache_lens[s] = a.lens_new[r]; a.req_id[s] = a.req_new[r];
  }
}

// ---------------------------------------------------------------------------------------------- per-request uniforms
// counter (req_id, n_gen, 0, 0), key = seed; u = (word 0 >> 8) * 2^-24: 24 bits, exact in fp32, never 1.
__global__ __launch_bounds__(BATCH_THREADS) void request_uniform_kernel(unsigned long long seed, const int* __restrict__ req_id,
                                                                        const int* __restrict__ n_gen, float* __restrict__ u, int B) {
  const int s = blockIdx.x * BATCH_THREADS + threadIdx.x;
  if (s >= B) return;
  uint32_t c[4] = {(uint32_t)req_id[s], (uint32_t)n_gen[s], 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  u[s] = (float)(c[0] >> 8) * 5.9604644775390625e-08f;
}

// lmod_request_uniform_rows: key and counter word 0 per slot (a request with a seed of its own: its seed and 0, wherever it stands in
// the list; one without: the call's seed and its request index).  The same mapping to 24 bits.
__global__ __launch_bounds__(BATCH_THREADS) void request_uniform_rows_kernel(const unsigned long long* __restrict__ seed,
                                                                             const int* __restrict__ ctr0, const int* __restrict__ n_gen,
                                                                             float* __restrict__ u, int B) {
  const int s = blockIdx.x * BATCH_THREADS + threadIdx.x;
  if (s >= B) return;
  const unsigned long long k = seed[s];
  uint32_t c[4] = {(uint32_t)ctr0[s], (uint32_t)n_gen[s], 0u, 0u};
  philox4x32_10(c, (uint32_t)k, (uint32_t)(k >> 32));
  u[s] = (float)(c[0] >> 8) * 5.9604644775390625e-08f;
}

extern "C" {

int lmod_kv_admit_rows(void* const* dst, const void* const* src, int ntensor, const int* dst_row, const int* lens, int R, int B,
                       int smax_dst, int smax_src, int width, int max_len, hipStream_t stream) {
  if (R < 0 || ntensor < 0 || ntensor > 65535 || R > 65535 || B < 1 || smax_dst < 1 || smax_src < 1 || width < 8 || (width & 7) ||
      max_len < 0) return LMOD_EINVAL;
  if (max_len > smax_dst || max_len > smax_src) return LMOD_EINVAL;      // a prompt would run past a cache: grow it first
  if (R == 0 || ntensor == 0 || max_len == 0) return LMOD_OK;
  if (!dst || !src || !dst_row || !lens) return LMOD_EINVAL;
  const int P = width >= 32768 ? 1 : 32768 / width;     // 64 KiB per workgroup
  const dim3 grid((max_len + P - 1) / P, R, ntensor);
  hipLaunchKernelGGL(kv_admit_rows_kernel, grid, dim3(BATCH_THREADS), 0, stream, dst, src, dst_row, lens, B, smax_dst, smax_src, width,
                     max_len, P);
  return lmod_launch_status();
}

int lmod_slot_admit(const int* dst_row, const int* prompt_ids, int ld_prompt, const int* n_prompt_new, const int* lens_new,
                    const int* req_new, int R, int B, int* hist, int ld_hist, int* n_prompt, int* n_hist, int* n_gen, int* done,
                    int* cache_lens, int* req_id, hipStream_t stream) {
  if (R < 0 || R > 65535 || B < 1 || ld_prompt < 0 || ld_hist < 0) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!dst_row || !prompt_ids || !n_prompt_new || !lens_new || !req_new || !hist || !n_prompt || !n_hist || !n_gen || !done ||
      !cache_lens || !req_id) return LMOD_EINVAL;
  SlotAdmitArgs a;
  a.dst_row = dst_row; a.prompt_ids = prompt_ids; a.ld_prompt = ld_prompt; a.n_prompt_new = n_prompt_new; a.lens_new = lens_new;
  a.req_new = req_new; a.B = B;
  a.hist = hist; a.ld_hist = ld_hist; a.n_prompt = n_prompt; a.n_hist = n_hist; a.n_gen = n_gen; a.done = done;
  a.cache_lens = cache_lens; a.req_id = req_id;
  a.vec = !((ld_prompt | ld_hist) & 3) && !(((uintptr_t)prompt_ids | (uintptr_t)hist) & 15);
  hipLaunchKernelGGL(slot_admit_kernel, dim3(R), dim3(BATCH_THREADS), 0, stream, a);
  return lmod_launch_status();
}

int lmod_request_uniform(unsigned long long seed, const int* req_id, const int* n_gen, float* u, int B, hipStream_t stream) {
  if (B < 0) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!req_id || !n_gen || !u) return LMOD_EINVAL;
  hipLaunchKernelGGL(request_uniform_kernel, dim3((B + BATCH_THREADS - 1) / BATCH_THREADS), dim3(BATCH_THREADS), 0, stream, seed,
                     req_id, n_gen, u, B);
  return lmod_launch_status();
}

int lmod_request_uniform_rows(const unsigned long long* seed, const int* ctr0, const int* n_gen, float* u, int B, hipStream_t stream) {
  if (B < 0) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!seed || !ctr0 || !n_gen || !u || ((uintptr_t)seed & 7)) return LMOD_EINVAL;
  hipLaunchKernelGGL(request_uniform_rows_kernel, dim3((B + BATCH_THREADS - 1) / BATCH_THREADS), dim3(BATCH_THREADS), 0, stream, seed,
                     ctr0, n_gen, u, B);
  return lmod_launch_status();
}

}  // extern "C"
