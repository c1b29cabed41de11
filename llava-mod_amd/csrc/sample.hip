// Sampling on the device (generate(do_sample=True)): lmod_sample_bf16 draws one token per row of bf16 logits from the temperature /
// top-k / top-p (nucleus) warped distribution, HF's warper order, with one caller-supplied uniform per row.
//
// Semantics.  x = logit / max(temperature, 1e-6).  top-k (0 < top_k < V) keeps x >= the k-th largest x, every tie at that value
// included.  top-p (top_p < 1) orders the top-k survivors by logit descending (equal logits by the smaller token id, beam.hip's
// beats()), takes the shortest prefix whose renormalised mass reaches top_p (a token stays while the mass before it is <= top_p)
// and keeps every token with x >= the logit of the prefix's last token: the kept set is a pure threshold on the logit, so a tie
// group that the prefix cuts is kept whole.  That is at most part of one tie group more than a sort-based sampler keeps, which cuts
// inside the group in the sort's unspecified order.  At least the maximum is always kept (top_p <= 0 keeps the maximum's tie group).
// The draw is the inverse CDF over the kept tokens in token-id order: the first kept token whose cumulative kept mass exceeds
// u * kept_mass.
//
// No sort.  bf16 has 65536 values and x -> x / T is monotone, so both cutoffs are thresholds on the 16-bit order-preserving key of
// the logit (-0 folded onto +0).  They are found by radix selection: a 256-bin count + mass histogram over the key's high byte,
// then one over the low byte inside the selected high bin (one low-byte pass per active filter: the top-p cutoff needs the mass of
// the finished top-k set).  Histograms are built in LDS and added to the row's histogram in `ws` with integer atomics.
//
// Determinism.  Masses are fixed-point integers: round(exp((logit - rowmax) / T) * 2^40) in 64 bits (V * 2^40 < 2^58).  Integer
// sums do not depend on the reduction shape or the arrival order of atomics, the cutoff search and the inverse-CDF search are exact
// integer arithmetic, and every pass computes a token's weight with the same expression: the same inputs give the same token and
// the same stats bit for bit.  A weight below 2^-41 of the maximum's rounds to 0: such a token is never drawn.
//
// Launches (fixed per call, no host read-back, no allocation): chunk max (+ zeroing of the row's histograms), [high-byte histogram,
// low-byte histogram per active filter], per-chunk kept mass, draw: 3 without a filter, 5 with one, 6 with both.  Rows are cut
// into `chunk`-token pieces (grid = chunks x rows) so that one row still covers the chip; the draw runs one workgroup per row and
// rescans only the chunk that holds the drawn token.
//
// Workspace, per row (8-byte aligned): 64 B header, nh x 3072 B histograms (256 x u64 mass + 256 x u32 count; nh = 0 without a
// filter, 2 with one, 3 with both), C x u64 chunk masses, C x int chunk maxima: ws_bytes >= R * (64 + 3072 * nh + 16 * C),
// C = ceil(V / chunk).
//
// Edge cases: -inf logits weigh 0 and are never drawn; a row without a finite logit returns token 0, lse = -inf and kept fraction
// 0 (no NaN); NaN logits are unspecified (as in beam.hip) but the token stays in [0, V).
//
// The device functions (key, weight, scans, selection, the passes' bodies, the draw of one row) live in sample_common.h:
// specsample.hip and sample_rows.hip (per-row parameters) share them.
#include "sample_common.h"

// Pass 1: grid (C, R).  Chunk maximum (as a key); the chunk's workgroups also zero the row's header and histograms.
__global__ __launch_bounds__(256) void sample_max_kernel(SampleArgs a) {
  __shared__ SampleSmem s;
  sample_pass_max(a, blockIdx.x, blockIdx.y, &s);
}

// Pass 2: grid (C, R).  mode 0: histogram of the key's high byte over every token -> hist 0.  mode 1: low byte of the tokens in
// the top-k high bin -> hist 1.  mode 2: low byte of the tokens in the top-p high bin -> hist `hidx`.
__global__ __launch_bounds__(256) void sample_hist_kernel(SampleArgs a, int mode, int hidx) {
  __shared__ SampleSmem s;
  __shared__ u64 hm[256];
  __shared__ uint32_t hc[256];
  sample_pass_hist(a, blockIdx.x, blockIdx.y, mode, hidx, &s, hm, hc);
}

// Pass 3: grid (C, R).  The final cutoff key, then the chunk's kept mass.
__global__ __launch_bounds__(256) void sample_mass_kernel(SampleArgs a) {
  __shared__ SampleSmem s;
  sample_pass_mass(a, blockIdx.x, blockIdx.y, &s);
}

// Pass 4: one workgroup per row: the draw (sample_common.h) and the stats.
__global__ __launch_bounds__(256) void sample_draw_kernel(SampleArgs a, const float* __restrict__ u, int* __restrict__ out_token,
                                                          float* __restrict__ out_stats) {
  __shared__ SampleSmem s;
  const int r = blockIdx.x;
  float m;
  u64 kept;
  uint32_t cut, n_kept;
  const int tok = sample_draw_row(a, r, u[r], &s, m, kept, cut, n_kept);
  if (threadIdx.x == 0) {
    out_token[r] = tok;
    if (out_stats) sample_write_stats(a, r, out_stats + 4 * (long long)r, m, kept, cut, n_kept);
  }
}

int sample_args_init(SampleArgs& a, const void* logits, long long ld, int V, int R, float temperature, int top_k, float top_p, int chunk,
                     void* ws) {
  if (R < 0 || R > 65535 || V < 2 || ld < V || chunk < 8 || (chunk & 7)) return LMOD_EINVAL;
  const int C = (V + chunk - 1) / chunk;
  const int use_k = top_k > 0 && top_k < V, use_p = top_p < 1.f;
  a.x = (const bf16_t*)logits; a.ld = ld; a.V = V; a.chunk = chunk; a.C = C;
  a.vec = (ld % 8 == 0) && ((uintptr_t)logits % 16 == 0);
  a.nh = (use_k || use_p) ? 1 + use_k + use_p : 0;
  a.T = fmaxf(temperature, 1e-6f);
  a.top_k = use_k ? top_k : 0; a.use_p = use_p; a.top_p = top_p;
  a.ws = (unsigned char*)ws;
  a.row_bytes = SAMPLE_HDR_BYTES + (long long)SAMPLE_HIST_BYTES * a.nh + 16LL * C;
  a.x2 = nullptr; a.ld2 = 0; a.R1 = R;
  return LMOD_OK;
}

void sample_launch_filter(const SampleArgs& a, int R, hipStream_t stream) {
  const dim3 grid(a.C, R), block(256);
  hipLaunchKernelGGL(sample_max_kernel, grid, block, 0, stream, a);
  if (a.nh) {
    hipLaunchKernelGGL(sample_hist_kernel, grid, block, 0, stream, a, 0, 0);
    if (a.top_k > 0) hipLaunchKernelGGL(sample_hist_kernel, grid, block, 0, stream, a, 1, 1);
    if (a.use_p) hipLaunchKernelGGL(sample_hist_kernel, grid, block, 0, stream, a, 2, a.top_k > 0 ? 2 : 1);
  }
  hipLaunchKernelGGL(sample_mass_kernel, grid, block, 0, stream, a);
}

extern "C" {

int lmod_sample_bf16(const void* logits, long long ld, int V, const float* u, int R, float temperature, int top_k, float top_p,
                     int chunk, void* ws, long long ws_bytes, int* out_token, float* out_stats, hipStream_t stream) {
  SampleArgs a;
  if (sample_args_init(a, logits, ld, V, R, temperature, top_k, top_p, chunk, ws)) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!logits || !u || !ws || !out_token || ((uintptr_t)ws & 7)) return LMOD_EINVAL;
  if (a.C > 65535) return LMOD_EINVAL;
  if (ws_bytes < a.row_bytes * R) return LMOD_EINVAL;
  sample_launch_filter(a, R, stream);
  hipLaunchKernelGGL(sample_draw_kernel, dim3(R), dim3(256), 0, stream, a, u, out_token, out_stats);
  return lmod_launch_status();
}

}  // extern "C"
