// lmod_sample_rows_bf16: lmod_sample_bf16 with the parameters of every row read from device arrays (generate_batch with per-request
// parameters: a greedy request and a temperature / top-k / top-p request decode in one batch).  The contract of a sampled row, the
// method and the reasons are in sample.hip's header comment; this file only routes per-row parameters into the same device
// functions (sample_common.h).
//
// Row r with greedy[r] == 0 is lmod_sample_bf16 on that row alone with temperature[r], top_k[r], top_p[r], bit for bit in the token
// and the stats: every pass computes a weight with the shared expression and sums integers, so neither the neighbours, the row's
// position nor the workspace layout can change a result.  Row r with greedy[r] != 0 returns the first maximum (lmod_row_argmax_bf16's
// token; +0 and -0 are one value) and the stats {logsumexp(x) at T = 1, 1, V, -inf}: it runs as an unfiltered row at T = 1 (chunk
// maxima and chunk masses give the maximum and the logsumexp) and replaces the inverse-CDF draw by the argmax search.
//
// Launches: always the six of the both-filters case (chunk max, high-byte histogram, top-k low byte, top-p low byte, kept mass,
// draw), whatever the mix of parameters, grid chunks x rows (the draw: rows).  A workgroup whose row does not take part in a pass
// (the high-byte histogram without a filter, a low-byte pass without its filter) returns before its first barrier; the test depends
// on blockIdx.y alone, so the exit is workgroup-uniform.
//
// Workspace: the nh = 3 layout of lmod_sample_bf16 for every row, ws_bytes >= R * (64 + 3072 * 3 + 16 * C), C = ceil(V / chunk).  A
// row with top-p alone uses histogram 1 for its low-byte pass, as lmod_sample_bf16 does.
#include "sample_common.h"

struct SampleRowsArgs {
  SampleArgs base;                 // shape, workspace (nh = 3) and the alignment flag; T / top_k / use_p / top_p are filled per row
  const float* temperature; const int* top_k; const float* top_p; const int* greedy;
};

// the SampleArgs lmod_sample_bf16's sample_args_init builds for row r alone (same normalisation), on the nh = 3 layout
__device__ __forceinline__ SampleArgs sample_row_args(const SampleRowsArgs& ra, int r, bool& greedy) {
  SampleArgs a = ra.base;
  greedy = ra.greedy[r] != 0;
  const int k = ra.top_k[r];
  const float p = ra.top_p[r];
  const bool use_k = !greedy && k > 0 && k < a.V, use_p = !greedy && p < 1.f;
  a.T = greedy ? 1.f : fmaxf(ra.temperature[r], 1e-6f);
  a.top_k = use_k ? k : 0; a.use_p = use_p; a.top_p = p;
  return a;
}

__global__ __launch_bounds__(256) void sample_rows_max_kernel(SampleRowsArgs ra) {
  __shared__ SampleSmem s;
  bool g;
  const SampleArgs a = sample_row_args(ra, blockIdx.y, g);
  sample_pass_max(a, blockIdx.x, blockIdx.y, &s);
}

__global__ __launch_bounds__(256) void sample_rows_hist_kernel(SampleRowsArgs ra, int mode) {
  __shared__ SampleSmem s;
  __shared__ u64 hm[256];
  __shared__ uint32_t hc[256];
  bool g;
  const SampleArgs a = sample_row_args(ra, blockIdx.y, g);
  // workgroup-uniform: a function of blockIdx.y
  if (mode == 0 ? !(a.use_p || a.top_k > 0) : mode == 1 ? a.top_k <= 0 : !a.use_p) return;
  sample_pass_hist(a, blockIdx.x, blockIdx.y, mode, mode == 2 ? (a.top_k > 0 ? 2 : 1) : mode, &s, hm, hc);
}

__global__ __launch_bounds__(256) void sample_rows_mass_kernel(SampleRowsArgs ra) {
  __shared__ SampleSmem s;
  bool g;
  const SampleArgs a = sample_row_args(ra, blockIdx.y, g);
  sample_pass_mass(a, blockIdx.x, blockIdx.y, &s);
}

// The first maximum of a row by its whole workgroup, from the chunk maxima: the first chunk that holds the maximum key, then the
// first token of that chunk with that key.  Every thread returns the token.
__device__ __forceinline__ int sample_argmax_row(const SampleArgs& a, int r, SampleSmem* s) {
  const int tid = threadIdx.x;
  const int* cmax = s_cmax(a, r);
  int k = 0;
  for (int c = tid; c < a.C; c += 256) k = max(k, cmax[c]);
  const int kmax = block_max_int(k, s);
  int first = -a.C;                                       // block_max_int of the negated index = the smallest index
  for (int c = tid; c < a.C; c += 256) if (cmax[c] == kmax) first = max(first, -c);
  const int cs = min(-block_max_int(first, s), a.C - 1);
  const bf16_t* row = s_row(a, r);
  const int lo = cs * a.chunk, hi = min(a.V, lo + a.chunk);
  int tok = -a.V;
  for_tokens(row, lo, hi, a.vec, tid, [&](uint32_t b, int e) { if ((int)skey(b) == kmax) tok = max(tok, -e); });
  const int t = -block_max_int(tok, s);
  return t < a.V ? max(t, 0) : 0;                        // no token carries the key (NaN logits only): token 0
}

__global__ __launch_bounds__(256) void sample_rows_draw_kernel(SampleRowsArgs ra, const float* __restrict__ u, int* __restrict__ out_token,
                                                               float* __restrict__ out_stats) {
  __shared__ SampleSmem s;
  const int r = blockIdx.x;
  bool g;
  const SampleArgs a = sample_row_args(ra, r, g);
  float m;
  u64 kept;
  uint32_t cut, n_kept;
  int tok = sample_draw_row(a, r, g ? 0.f : u[r], &s, m, kept, cut, n_kept);     // greedy: its m and kept (= total mass at T = 1)
  if (g) tok = sample_argmax_row(a, r, &s);
  if (threadIdx.x == 0) {
    out_token[r] = tok;
    if (out_stats) {
      float* st = out_stats + 4 * (long long)r;
      sample_write_stats(a, r, st, m, kept, cut, n_kept);
      if (g) st[1] = 1.f;                                   // nothing is filtered, also on a row without a finite logit
    }
  }
}

extern "C" {

int lmod_sample_rows_bf16(const void* logits, long long ld, int V, const float* u, int R, const float* temperature, const int* top_k,
                          const float* top_p, const int* greedy, int chunk, void* ws, long long ws_bytes, int* out_token,
                          float* out_stats, hipStream_t stream) {
  SampleRowsArgs ra;
  // the shape checks of lmod_sample_bf16; both filters on fixes the nh = 3 layout
  if (sample_args_init(ra.base, logits, ld, V, R, 1.f, 1, 0.5f, chunk, ws)) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!logits || !u || !temperature || !top_k || !top_p || !greedy || !ws || !out_token || ((uintptr_t)ws & 7)) return LMOD_EINVAL;
  if (ra.base.C > 65535) return LMOD_EINVAL;
  if (ws_bytes < ra.base.row_bytes * R) return LMOD_EINVAL;
  ra.temperature = temperature; ra.top_k = top_k; ra.top_p = top_p; ra.greedy = greedy;
  const dim3 grid(ra.base.C, R), block(256);
  hipLaunchKernelGGL(sample_rows_max_kernel, grid, block, 0, stream, ra);
  hipLaunchKernelGGL(sample_rows_hist_kernel, grid, block, 0, stream, ra, 0);
  hipLaunchKernelGGL(sample_rows_hist_kernel, grid, block, 0, stream, ra, 1);
  hipLaunchKernelGGL(sample_rows_hist_kernel, grid, block, 0, stream, ra, 2);
  hipLaunchKernelGGL(sample_rows_mass_kernel, grid, block, 0, stream, ra);
  hipLaunchKernelGGL(sample_rows_draw_kernel, dim3(R), block, 0, stream, ra, u, out_token, out_stats);
  return lmod_launch_status();
}

}  // extern "C"
