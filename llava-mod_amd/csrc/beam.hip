// Beam search on the device (generate(num_beams > 1), HF GenerationMixin._beam_search semantics):
//   lmod_beam_topk_bf16  - per sample the top K = 2*nb candidates of log_softmax(logits) + beam score over nb*V;
//   lmod_kv_gather_rows  - one launch over every K/V cache tensor of a model: dst[t][r, 0:lens[r]] = src[t][src_row[r], 0:lens[r]]
//                          (replicate the prefill cache into the beam rows; reorder the beams into the second buffer).
#include "common.h"
#include <limits.h>

// ---------------------------------------------------------------------------------------------- top-K candidate lists
// Order: value descending, equal values by the smaller index (token in stage 1, flattened beam*V + token in stage 2).  Every
// index is unique, so this is a strict total order and the result does not depend on the reduction shape.  NaN never enters.
__device__ __forceinline__ bool beats(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

template <int L>
__device__ __forceinline__ void list_init(float (&v)[L], int (&ix)[L]) {
#pragma unroll
  for (int k = 0; k < L; ++k) { v[k] = -INFINITY; ix[k] = INT_MAX; }
}

// sorted insertion into a register list (constant indices only: no scratch)
template <int L>
__device__ __forceinline__ void list_push(float (&v)[L], int (&ix)[L], float x, int i) {
  if (!beats(x, i, v[L - 1], ix[L - 1])) return;
  v[L - 1] = x; ix[L - 1] = i;
#pragma unroll
  for (int k = L - 1; k > 0; --k) {
    if (beats(v[k], ix[k], v[k - 1], ix[k - 1])) {
      const float tv = v[k]; v[k] = v[k - 1]; v[k - 1] = tv;
      const int ti = ix[k]; ix[k] = ix[k - 1]; ix[k - 1] = ti;
    }
  }
}

// Merge the 64 sorted lane lists of a wave into its top KC: KC rounds of a butterfly arg-max over the list heads, the winning lane
// pops its head.  Every lane ends with the same (ov, oi).
template <int L, int KC>
__device__ __forceinline__ void wave_merge(float (&v)[L], int (&ix)[L], float (&ov)[KC], int (&oi)[KC]) {
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    float bv = v[0]; int bi = ix[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float tv = __shfl_xor(bv, o, 64); const int ti = __shfl_xor(bi, o, 64);
      if (beats(tv, ti, bv, bi)) { bv = tv; bi = ti; }
    }
    ov[k] = bv; oi[k] = bi;
    if (ix[0] == bi) {
#pragma unroll
      for (int j = 0; j + 1 < L; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
      v[L - 1] = -INFINITY; ix[L - 1] = INT_MAX;
    }
  }
}

// Workgroup (4 waves) top KC of the per-lane lists: wave merge, then wave 0 merges the 4 x KC survivors from LDS (one per lane).
// The result is valid in wave 0 (every lane).
template <int L, int KC>
__device__ __forceinline__ void block_merge(float (&v)[L], int (&ix)[L], float (&ov)[KC], int (&oi)[KC], float* sv, int* si) {
  static_assert(4 * KC <= 64, "one survivor per lane");
  wave_merge<L, KC>(v, ix, ov, oi);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < KC; ++k) { sv[w * KC + k] = ov[k]; si[w * KC + k] = oi[k]; }
  }
  __syncthreads();
  if (w == 0) {
    float v1[1]; int i1[1];
    v1[0] = lane < 4 * KC ? sv[lane] : -INFINITY;
    i1[0] = lane < 4 * KC ? si[lane] : INT_MAX;
    wave_merge<1, KC>(v1, i1, ov, oi);
  }
}

// online (max, sum exp(x - max)) pair, merged across lanes / chunks
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  if (nm == -INFINITY) return;
  s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
  m = nm;
}

// Workspace entry of one (row, chunk): [0] max, [1] sum exp(x - max), [2, 2+KC) the chunk's top KC logits (fp32),
// [2+KC, 2+2KC) their token ids (int bits; INT_MAX = empty).
template <int KC>
constexpr int ws_words() { return 2 + 2 * KC; }

// Stage 1: grid (C chunks, R rows), 256 threads.  Chunk c of row r covers tokens [c*chunk, min(V, (c+1)*chunk)), chunk % 8 == 0.
template <int KC>
__global__ __launch_bounds__(256) void beam_topk_stage1_kernel(const bf16_t* __restrict__ x, long long ld, int V, int chunk,
                                                               int C, int vec, float* __restrict__ ws) {
  __shared__ float sv[4 * KC];
  __shared__ int si[4 * KC];
  __shared__ float sm[4], ss[4];
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const bf16_t* row = x + (long long)r * ld;
  const int lo = c * chunk, hi = min(V, lo + chunk);
  float m = -INFINITY, s = 0.f;
  float v[KC]; int ix[KC];
  list_init<KC>(v, ix);
  int tail = lo;
  if (vec) {
    const int nv = (hi - lo) >> 3;
    for (int q = tid; q < nv; q += 256) {
      const int base = lo + (q << 3);
      const u32x4 w = *(const u32x4*)(row + base);
      float f[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { f[2 * j] = bflo(w[j]); f[2 * j + 1] = bfhi(w[j]); }
      float mx = f[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) mx = fmaxf(mx, f[j]);
      if (mx > m) { s = (m == -INFINITY) ? 0.f : s * __expf(m - mx); m = mx; }
      if (m != -INFINITY) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s += __expf(f[j] - m);
      }
      if (mx >= v[KC - 1]) {                            // rare after the first few vectors: one copy of the insertion code
#pragma unroll 1
        for (int j = 0; j < 8; ++j) {
          const uint32_t wj = j < 2 ? w[0] : j < 4 ? w[1] : j < 6 ? w[2] : w[3];
          list_push<KC>(v, ix, (j & 1) ? bfhi(wj) : bflo(wj), base + j);
        }
      }
    }
    tail = lo + (nv << 3);
  }
  for (int e = tail + tid; e < hi; e += 256) {        // scalar tail (V % 8) or the unaligned form
    const float f = bf2f(row[e]);
    if (f > m) { s = (m == -INFINITY) ? 0.f : s * __expf(m - f); m = f; }
    if (m != -INFINITY) s += __expf(f - m);
    list_push<KC>(v, ix, f, e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    lse_merge(m, s, om, os);
  }
  if ((tid & 63) == 0) { sm[tid >> 6] = m; ss[tid >> 6] = s; }
  float ov[KC]; int oi[KC];
  block_merge<KC, KC>(v, ix, ov, oi, sv, si);            // its __syncthreads also publishes sm / ss
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) lse_merge(m, s, sm[w], ss[w]);
    float* e = ws + ((long long)r * C + c) * ws_words<KC>();
    e[0] = m; e[1] = s;
#pragma unroll
    for (int k = 0; k < KC; ++k) { e[2 + k] = ov[k]; ((int*)e)[2 + KC + k] = oi[k]; }
  }
}

// Stage 2: one workgroup per sample.  lse of each of its nb rows from the chunk pairs, then the top K of
// (logit - max) - log(sum) + beam_score over the nb * C * KC chunk survivors (the same form as torch.log_softmax).
template <int KC>
__global__ __launch_bounds__(256) void beam_topk_stage2_kernel(const float* __restrict__ ws, const float* __restrict__ bscore,
                                                               int V, int nb, int C, int K, float* __restrict__ out_score,
                                                               int* __restrict__ out_beam, int* __restrict__ out_token) {
  __shared__ float sv[4 * KC];
  __shared__ int si[4 * KC];
  __shared__ float rmax[8], rlog[8], rbs[8];
  const int b = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  for (int j = w; j < nb; j += 4) {
    const float* base = ws + (long long)(b * nb + j) * C * ws_words<KC>();
    float m = -INFINITY, s = 0.f;
    for (int c = lane; c < C; c += 64) lse_merge(m, s, base[c * ws_words<KC>()], base[c * ws_words<KC>() + 1]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
      lse_merge(m, s, om, os);
    }
    if (lane == 0) { rmax[j] = m; rlog[j] = logf(s); rbs[j] = bscore[b * nb + j]; }
  }
  __syncthreads();
  float v[KC]; int ix[KC];
  list_init<KC>(v, ix);
  const int per_row = C * KC, n = nb * per_row;
  for (int e = tid; e < n; e += 256) {
    const int j = e / per_row, rem = e - j * per_row, c = rem / KC, k = rem - c * KC;
    const float* ent = ws + ((long long)(b * nb + j) * C + c) * ws_words<KC>();
    const int tok = ((const int*)ent)[2 + KC + k];
    if (tok >= V) continue;                             // empty slot of a short chunk
    const float sc = ((ent[2 + k] - rmax[j]) - rlog[j]) + rbs[j];
    list_push<KC>(v, ix, sc, j * V + tok);
  }
  float ov[KC]; int oi[KC];
  block_merge<KC, KC>(v, ix, ov, oi, sv, si);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      if (k < K) {
        const int f = oi[k] == INT_MAX ? 0 : oi[k];
        out_score[b * K + k] = ov[k]; out_beam[b * K + k] = f / V; out_token[b * K + k] = f - (f / V) * V;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- cache row gather
// grid (position blocks of P, R rows, ntensor tensors): the P positions of one row are one contiguous span of P * width bf16.
__global__ __launch_bounds__(256) void kv_gather_rows_kernel(void* const* __restrict__ dst, const void* const* __restrict__ src,
                                                             const int* __restrict__ src_row, const int* __restrict__ lens,
                                                             int R_src, int smax_dst, int smax_src, int width, int P) {
  const int t = blockIdx.z, r = blockIdx.y, p0 = blockIdx.x * P;
  const int n = min(lens[r], min(smax_dst, smax_src));
  if (p0 >= n) return;
  const int sr = src_row[r];
  if (sr < 0 || sr >= R_src) return;
  const int p1 = min(p0 + P, n);
  const u32x4* s = (const u32x4*)((const bf16_t*)src[t] + ((long long)sr * smax_src + p0) * width);
  u32x4* d = (u32x4*)((bf16_t*)dst[t] + ((long long)r * smax_dst + p0) * width);
  const int nv = (p1 - p0) * (width >> 3);
  int q = threadIdx.x;
  for (; q + 3 * 256 < nv; q += 4 * 256) {             // four 16-byte loads in flight per lane
    const u32x4 a0 = s[q], a1 = s[q + 256], a2 = s[q + 512], a3 = s[q + 768];
    d[q] = a0; d[q + 256] = a1; d[q + 512] = a2; d[q + 768] = a3;
  }
  for (; q < nv; q += 256) d[q] = s[q];
}

extern "C" {

int lmod_beam_topk_bf16(const void* logits, long long ld, int V, const float* beam_scores, int B, int nb, int chunk, float* ws,
                        long long ws_bytes, float* out_score, int* out_beam, int* out_token, hipStream_t stream) {
  if (B < 0 || nb < 1 || nb > 8 || V < 2 || ld < V || chunk < 8 || (chunk & 7)) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!logits || !beam_scores || !ws || !out_score || !out_beam || !out_token) return LMOD_EINVAL;
  if ((long long)nb * V > INT_MAX) return LMOD_EUNSUPPORTED;
  const int K = 2 * nb, R = B * nb, C = (V + chunk - 1) / chunk;
  const int KC = K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16;
  if (ws_bytes < (long long)R * C * (2 + 2 * KC) * 4 || C > 65535 || R > 65535) return LMOD_EINVAL;
  const int vec = (ld % 8 == 0) && ((uintptr_t)logits % 16 == 0);
  const dim3 g1(C, R);
#define LMOD_BEAM_LAUNCH(KCV)                                                                                               \
  hipLaunchKernelGGL(beam_topk_stage1_kernel<KCV>, g1, dim3(256), 0, stream, (const bf16_t*)logits, ld, V, chunk, C, vec, ws); \
  hipLaunchKernelGGL(beam_topk_stage2_kernel<KCV>, dim3(B), dim3(256), 0, stream, (const float*)ws, beam_scores, V, nb, C, K, \
                     out_score, out_beam, out_token);
  switch (KC) {
    case 2: LMOD_BEAM_LAUNCH(2) break;
    case 4: LMOD_BEAM_LAUNCH(4) break;
    case 8: LMOD_BEAM_LAUNCH(8) break;
    default: LMOD_BEAM_LAUNCH(16) break;
  }
#undef LMOD_BEAM_LAUNCH
  return lmod_launch_status();
}

int lmod_kv_gather_rows(void* const* dst, const void* const* src, int ntensor, const int* src_row, const int* lens, int R, int R_src,
                        int smax_dst, int smax_src, int width, hipStream_t stream) {
  if (R < 0 || ntensor < 0 || ntensor > 65535 || R > 65535 || R_src < 1 || smax_dst < 1 || smax_src < 1 || width < 8 ||
      (width & 7)) return LMOD_EINVAL;
  if (R == 0 || ntensor == 0) return LMOD_OK;
  if (!dst || !src || !src_row || !lens) return LMOD_EINVAL;
  const int P = width >= 32768 ? 1 : 32768 / width;     // 64 KiB per workgroup
  const dim3 grid((smax_dst + P - 1) / P, R, ntensor);
  hipLaunchKernelGGL(kv_gather_rows_kernel, grid, dim3(256), 0, stream, dst, src, src_row, lens, R_src, smax_dst, smax_src, width, P);
  return lmod_launch_status();
}

}  // extern "C"
