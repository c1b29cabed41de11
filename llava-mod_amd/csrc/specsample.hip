// Speculative sampling (generate(assistant_model=..., speculative_sampling=True)): lmod_spec_sample_bf16 verifies k draft tokens per
// sample against the target's k+1 verification rows with the rule of Leviathan et al. ("Fast inference from transformers via
// speculative decoding", ICML'23; HF `_speculative_sampling`), so that the emitted tokens are distributed exactly as plain sampling
// from the target's warped distribution.
//
// Semantics.  p_i / q_i: the temperature -> top-k -> top-p warped distributions of the target's row b*(k+1)+i and the draft's row
// b*k+i, with lmod_sample_bf16's kept-set rule, fixed-point weight w = round(exp((x - rowmax) / T) * 2^40) (0 outside the kept set)
// and kept mass M (sample_common.h): p_i(x) = w_p(x) / M_p.  Position i is accepted iff u_acc[b,i] * q_i(d_i) < p_i(d_i); n_acc is
// the number of accepted positions before the first rejection (0 for a sample already done).  n_acc < k: next_token is the
// inverse-CDF draw with u_draw[b], in token-id order, from r(x) = max(0, p_n(x) - q_n(x)), n = n_acc (from p_n when r is zero
// everywhere).  n_acc == k: the bonus draw from p_k - the very code lmod_sample_bf16 runs on that row (sample_draw_row), so the same
// token for the same u.  The block, done, EOS cut, pad and both lens follow lmod_spec_accept with target[n_acc] = next_token.
//
// Arithmetic: integers only, so the result is bit-for-bit reproducible.  U = floor(u * 2^24) (u is clamped to [0, 1]; 24-bit uniforms
// are exact).  Accept iff U * w_q(d) * M_p < 2^24 * w_p(d) * M_q: w <= 2^40, M < 2^58, both sides < 2^122 in unsigned __int128
// (multiply, shift, compare, subtract; no 128-bit division).  Residual weight r(x) = max(0, w_p(x) * M_q - w_q(x) * M_p) >> 24: at most
// 2^74 per token, a row sum at most 2^92, U * sum at most 2^116; a token with p(x) - q(x) >= 2^-40 has w_p M_q - w_q M_p >= 2^-40 M_p M_q
// >= 2^40 (a kept maximum weighs 2^40, so M >= 2^40) and never gets weight 0.  Per-chunk residual masses are written as two u64 by one
// workgroup each (integer sums are order-independent: no 128-bit atomics); the draw workgroup scans them: target = (U * sum) >> 24.
//
// Launches (fixed for a filter set, no host read-back, no allocation): the filter passes of sample.hip over all B * (2k+1) rows in
// one grid each (2 without a filter, 4 with one, 5 with both), accept (one workgroup per sample: the 2k+1 rows' maxima and kept
// masses from their chunk records, the 2k weights at the draft tokens, n_acc; also the stats), residual mass (grid chunks x B, reads
// only rows n_acc[b] of p and q, the index taken from device memory), draw (one workgroup per sample; writes the block).
//
// Workspace (8-byte aligned): the B*(2k+1) row records of lmod_sample_bf16 (p rows first, then q rows), then per sample 32 B
// {n_acc, max key of p_n, max key of q_n, -, M_p, M_q} and C x 16 B residual chunk masses (low, high word):
// ws_bytes >= B * (2k+1) * (64 + 3072 * nh + 16 * C) + B * (32 + 16 * C), C = ceil(V / chunk).
//
// Edge cases: a draft token outside [0, V) or outside the target's kept set is rejected; a row without a finite logit on either side
// rejects its position and the residual falls back to p_n (token 0 when p_n has no finite logit either); nothing is NaN.
//
// lmod_spec_uniform: the uniforms of the speculative loop, u = (word 0 >> 8) * 2^-24 of Philox4x32-10 at counter (row, round, position,
// purpose) under the key `seed`: a pure function of its coordinates (purpose 0: the draft's own draw, 1: accept test, 2: residual /
// bonus draw).
#include "sample_common.h"
#include "philox.h"

typedef unsigned __int128 u128;

#define SPEC_K_MAX 15            // k < APPEND_T_MAX = 16 (append.hip): the verification chunk holds k + 1 tokens
#define SPEC_HDR_BYTES 32

struct SpecHdr { int n_acc, kmax_p, kmax_q, pad; u64 Mp, Mq; };

struct SpecArgs {
  SampleArgs a;
  int B, k, eos, pad;
  const int* draft; const float* u_acc; const float* u_draw;
  int* done; int* lens_target; int* lens_draft; int* out; int* next_token; float* out_stats;
  unsigned char* spec; long long spec_bytes;       // per-sample records behind the row records
};

struct SpecSmem { u64 lo[4], hi[4]; u64 v0[2], v1[2]; int i0, found; };

__device__ __forceinline__ SpecHdr* sp_hdr(const SpecArgs& s, int b) { return (SpecHdr*)(s.spec + b * s.spec_bytes); }
__device__ __forceinline__ u64* sp_cmass(const SpecArgs& s, int b) { return (u64*)(s.spec + b * s.spec_bytes + SPEC_HDR_BYTES); }
__device__ __forceinline__ u128 mk128(u64 lo, u64 hi) { return ((u128)hi << 64) | lo; }
__device__ __forceinline__ int row_p(const SpecArgs& s, int b, int i) { return b * (s.k + 1) + i; }
__device__ __forceinline__ int row_q(const SpecArgs& s, int b, int i) { return s.a.R1 + b * s.k + i; }
__device__ __forceinline__ uint32_t row_cut(const SampleArgs& a, int r) {
  return (a.use_p || a.top_k > 0) ? (uint32_t)(s_hdr(a, r)[H_CUT] & 0xffff) : 0u;
}
__device__ __forceinline__ uint32_t u24(float u) { return min((uint32_t)(fminf(fmaxf(u, 0.f), 1.f) * 16777216.f), 16777215u); }

// the residual weight of a token; the one expression every pass uses
__device__ __forceinline__ u128 rweight(u64 wp, u64 wq, u64 Mp, u64 Mq) {
  const u128 x = (u128)wp * Mq, y = (u128)wq * Mp;
  return x > y ? (x - y) >> 24 : (u128)0;
}

// one side (target or draft) of a position: the row, its maximum, cutoff key and kept mass
struct Side { const bf16_t* row; float m; uint32_t cut; u64 M; };
__device__ __forceinline__ u64 side_weight(const Side& s, uint32_t bits, float T) {
  return skey(bits) >= s.cut ? sweight(bf2f((bf16_t)bits), s.m, T) : 0ull;
}

__device__ __forceinline__ u128 block_sum_u128(u128 v, SpecSmem* s) {
  u64 lo = (u64)v, hi = (u64)(v >> 64);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u128 t = mk128(__shfl_xor(lo, o, 64), __shfl_xor(hi, o, 64)) + mk128(lo, hi);
    lo = (u64)t; hi = (u64)(t >> 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s->lo[threadIdx.x >> 6] = lo; s->hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  return mk128(s->lo[0], s->hi[0]) + mk128(s->lo[1], s->hi[1]) + mk128(s->lo[2], s->hi[2]) + mk128(s->lo[3], s->hi[3]);
}

// inclusive scan of v over the 256 threads in thread order
__device__ __forceinline__ u128 scan256_u128(u128 v, SpecSmem* s) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 lo = (u64)v, hi = (u64)(v >> 64);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 tl = __shfl_up(lo, o, 64), th = __shfl_up(hi, o, 64);
    if (lane >= o) {
      const u128 t = mk128(lo, hi) + mk128(tl, th);
      lo = (u64)t; hi = (u64)(t >> 64);
    }
  }
  __syncthreads();
  if (lane == 63) { s->lo[w] = lo; s->hi[w] = hi; }
  __syncthreads();
  u128 r = mk128(lo, hi);
  for (int j = 0; j < w; ++j) r += mk128(s->lo[j], s->hi[j]);
  return r;
}

// Accept: one workgroup per sample.  Each wave reduces the chunk records of some of the sample's 2k+1 rows to the row's maximum key
// and kept mass (and writes the row's stats); thread i < k tests position i; thread 0 finds the first rejection and publishes n_acc
// with the maxima and kept masses of rows n_acc in the sample's record for the later launches.
__global__ __launch_bounds__(256) void spec_sample_accept_kernel(SpecArgs sa) {
  __shared__ int s_kmax[2 * SPEC_K_MAX + 1];
  __shared__ u64 s_M[2 * SPEC_K_MAX + 1];
  __shared__ int s_acc[SPEC_K_MAX];
  const SampleArgs& a = sa.a;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, k = sa.k;
  for (int j = tid >> 6; j < 2 * k + 1; j += 4) {
    const int r = j <= k ? row_p(sa, b, j) : row_q(sa, b, j - k - 1);
    const int* cmax = s_cmax(a, r);
    const u64* cmass = s_cmass(a, r);
    int km = 0;
    u64 M = 0;
    for (int c = lane; c < a.C; c += 64) { km = max(km, cmax[c]); M += cmass[c]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { km = max(km, __shfl_xor(km, o, 64)); M += __shfl_xor(M, o, 64); }
    if (lane == 0) {
      s_kmax[j] = km; s_M[j] = M;
      if (sa.out_stats) {
        const bool filt = a.use_p || a.top_k > 0;
        sample_write_stats(a, r, sa.out_stats + 4 * (long long)r, skey_value((uint32_t)km), M, row_cut(a, r),
                           filt ? (uint32_t)(s_hdr(a, r)[H_CUT] >> 32) : (uint32_t)a.V);
      }
    }
  }
  __syncthreads();
  if (tid < k) {
    const int i = tid, d = sa.draft[(long long)b * k + i];
    int ok = 0;
    if (d >= 0 && d < a.V) {
      const int rp = row_p(sa, b, i), rq = row_q(sa, b, i);
      const Side P{s_row(a, rp), skey_value((uint32_t)s_kmax[i]), row_cut(a, rp), s_M[i]};
      const Side Q{s_row(a, rq), skey_value((uint32_t)s_kmax[k + 1 + i]), row_cut(a, rq), s_M[k + 1 + i]};
      const u64 wp = side_weight(P, (uint32_t)P.row[d], a.T), wq = side_weight(Q, (uint32_t)Q.row[d], a.T);
      const u64 U = u24(sa.u_acc[(long long)b * k + i]);
      ok = (u128)(U * wq) * P.M < ((u128)wp * Q.M) << 24;
    }
    s_acc[i] = ok;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    if (!sa.done[b])
      while (n < k && s_acc[n]) ++n;
    SpecHdr* h = sp_hdr(sa, b);
    h->n_acc = n; h->kmax_p = s_kmax[n]; h->Mp = s_M[n];
    h->kmax_q = n < k ? s_kmax[k + 1 + n] : 0; h->Mq = n < k ? s_M[k + 1 + n] : 0ull;
    h->pad = 0;
  }
}

__device__ __forceinline__ void spec_sides(const SpecArgs& sa, int b, const SpecHdr* h, Side& P, Side& Q) {
  const int rp = row_p(sa, b, h->n_acc), rq = row_q(sa, b, h->n_acc);
  P = Side{s_row(sa.a, rp), skey_value((uint32_t)h->kmax_p), row_cut(sa.a, rp), h->Mp};
  Q = Side{s_row(sa.a, rq), skey_value((uint32_t)h->kmax_q), row_cut(sa.a, rq), h->Mq};
}

// the residual weights of the 8 tokens e0 .. e0 + 7 (0 at and past `hi`)
__device__ __forceinline__ void rweights8(const SampleArgs& a, const Side& P, const Side& Q, int e0, int hi, u128 (&w)[8]) {
  if (a.vec && e0 + 8 <= hi) {
    const u32x4 vp = *(const u32x4*)(P.row + e0), vq = *(const u32x4*)(Q.row + e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[2 * j] = rweight(side_weight(P, vp[j] & 0xffffu, a.T), side_weight(Q, vq[j] & 0xffffu, a.T), P.M, Q.M);
      w[2 * j + 1] = rweight(side_weight(P, vp[j] >> 16, a.T), side_weight(Q, vq[j] >> 16, a.T), P.M, Q.M);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      w[j] = e0 + j < hi ? rweight(side_weight(P, (uint32_t)P.row[e0 + j], a.T), side_weight(Q, (uint32_t)Q.row[e0 + j], a.T), P.M, Q.M)
                         : (u128)0;
  }
}

// Residual mass: grid (C, B).  The chunk's sum of r(x) over rows n_acc[b] of p and q; nothing to do for a sample that accepted all
// k drafts (bonus draw) or is done.
__global__ __launch_bounds__(256) void spec_sample_residual_kernel(SpecArgs sa) {
  __shared__ SpecSmem s;
  const SampleArgs& a = sa.a;
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const SpecHdr* h = sp_hdr(sa, b);
  if (h->n_acc >= sa.k || sa.done[b]) return;
  Side P, Q;
  spec_sides(sa, b, h, P, Q);
  const int lo = c * a.chunk, hi = min(a.V, lo + a.chunk);
  u128 sum = 0;
  for (int e0 = lo + tid * 8; e0 < hi; e0 += 2048) {
    u128 w[8];
    rweights8(a, P, Q, e0, hi, w);
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += w[j];
  }
  sum = block_sum_u128(sum, &s);
  if (tid == 0) {
    u64* o = sp_cmass(sa, b) + 2 * c;
    o[0] = (u64)sum; o[1] = (u64)(sum >> 64);
  }
}

// Draw: one workgroup per sample.  next_token from the residual (n_acc < k and a positive residual mass) or from p_n with the
// sampler's own draw; thread 0 writes the block.
__global__ __launch_bounds__(256) void spec_sample_draw_kernel(SpecArgs sa) {
  __shared__ SampleSmem ss;
  __shared__ SpecSmem s;
  const SampleArgs& a = sa.a;
  const int b = blockIdx.x, tid = threadIdx.x, k = sa.k;
  const SpecHdr* h = sp_hdr(sa, b);
  const int n = h->n_acc, was_done = sa.done[b] != 0;
  int tok = 0;
  if (!was_done) {
    const u64* cm = sp_cmass(sa, b);
    u128 total = 0;
    if (n < k) {
      u128 part = 0;
      for (int c = tid; c < a.C; c += 256) part += mk128(cm[2 * c], cm[2 * c + 1]);
      total = block_sum_u128(part, &s);
    }
    if (total == 0) {
      float m;
      u64 kept;
      uint32_t cut, n_kept;
      tok = sample_draw_row(a, row_p(sa, b, n), sa.u_draw[b], &ss, m, kept, cut, n_kept);
    } else {
      Side P, Q;
      spec_sides(sa, b, h, P, Q);
      const u128 target = ((u128)u24(sa.u_draw[b]) * total) >> 24;          // < total
      // the chunk that holds the target
      u128 run = 0;
      __syncthreads();
      if (tid == 0) { s.i0 = a.C - 1; s.v1[0] = 0; s.v1[1] = 0; }
      for (int c0 = 0; c0 < a.C; c0 += 256) {
        const int c = c0 + tid;
        const u128 v = c < a.C ? mk128(cm[2 * c], cm[2 * c + 1]) : (u128)0;
        const u128 iv = scan256_u128(v, &s);
        if (tid == 255) { s.v0[0] = (u64)iv; s.v0[1] = (u64)(iv >> 64); }
        if (v > 0 && run + (iv - v) <= target && target < run + iv) {
          const u128 rem = target - (run + (iv - v));
          s.i0 = c; s.v1[0] = (u64)rem; s.v1[1] = (u64)(rem >> 64);
        }
        __syncthreads();
        const u128 tile = mk128(s.v0[0], s.v0[1]);
        if (target < run + tile) break;
        run += tile;
        __syncthreads();
      }
      __syncthreads();
      const int cs = s.i0;
      const u128 rem = mk128(s.v1[0], s.v1[1]);
      const int lo = cs * a.chunk, hi = min(a.V, lo + a.chunk);
      if (tid == 0) s.found = -1;
      __syncthreads();
      u128 run2 = 0;
      int lastk = -1;
      for (int base = lo; base < hi; base += 2048) {
        const int e0 = base + tid * 8;
        u128 w[8];
        rweights8(a, P, Q, e0, hi, w);
        u128 sum = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          sum += w[j];
          if (w[j] > 0) lastk = e0 + j;
        }
        const u128 iv = scan256_u128(sum, &s);
        if (tid == 255) { s.v0[0] = (u64)iv; s.v0[1] = (u64)(iv >> 64); }
        const u128 ex = run2 + (iv - sum);
        if (sum > 0 && ex <= rem && rem < ex + sum) {
          u128 cum = ex;
          int pick = -1;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            cum += w[j];
            if (pick < 0 && cum > rem) pick = e0 + j;
          }
          s.found = pick;
        }
        __syncthreads();
        if (s.found >= 0) break;
        run2 += mk128(s.v0[0], s.v0[1]);
        __syncthreads();
      }
      tok = s.found;
      if (tok < 0) tok = block_max_int(lastk, &ss);
      tok = min(max(tok, 0), a.V - 1);
    }
  }
  if (tid == 0) {                                       // lmod_spec_accept's block with target[n_acc] = tok
    const int* dr = sa.draft + (long long)b * k;
    int* o = sa.out + (long long)b * (k + 5);
    sa.lens_target[b] += n - k;
    sa.lens_draft[b] += min(n + 1, k) - k;
    int n_emit = 0, fin = was_done;
    if (!was_done) {
      n_emit = n + 1;
      for (int i = 0; i <= n; ++i) {
        const int t = i < n ? dr[i] : tok;
        if (sa.eos >= 0 && t == sa.eos) { n_emit = i + 1; fin = 1; break; }
      }
    }
    for (int i = 0; i <= k; ++i) o[i] = i < n_emit ? (i < n ? dr[i] : tok) : sa.pad;
    const int nxt = fin ? sa.pad : tok;
    o[k + 1] = n; o[k + 2] = n_emit; o[k + 3] = nxt; o[k + 4] = fin;
    sa.next_token[b] = nxt;
    sa.done[b] = fin;
  }
}

// u[b * n_pos + i] of counter (row0 + b, round, i, purpose)
__global__ __launch_bounds__(256) void spec_uniform_kernel(unsigned long long seed, int row0, int round, int purpose, int n_pos,
                                                           float* __restrict__ u, long long n) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  uint32_t c[4] = {(uint32_t)(row0 + (int)(t / n_pos)), (uint32_t)round, (uint32_t)(t % n_pos), (uint32_t)purpose};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  u[t] = (float)(c[0] >> 8) * 5.9604644775390625e-08f;
}

extern "C" {

int lmod_spec_sample_bf16(const void* p_logits, long long ld_p, const void* q_logits, long long ld_q, int V, const int* draft,
                          const float* u_acc, const float* u_draw, int B, int k, float temperature, int top_k, float top_p, int chunk,
                          void* ws, long long ws_bytes, int* done, int eos, int pad, int* lens_target, int* lens_draft, int* out,
                          int* next_token, float* out_stats, hipStream_t stream) {
  if (B < 0 || k < 1 || k > SPEC_K_MAX || (long long)B * (2 * k + 1) > 65535 || ld_q < V) return LMOD_EINVAL;
  const int R = B * (2 * k + 1);
  SpecArgs sa;
  if (sample_args_init(sa.a, p_logits, ld_p, V, R, temperature, top_k, top_p, chunk, ws)) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!p_logits || !q_logits || !draft || !u_acc || !u_draw || !ws || ((uintptr_t)ws & 7) || !done || !lens_target || !lens_draft ||
      !out || !next_token)
    return LMOD_EINVAL;
  SampleArgs& a = sa.a;
  if (a.C > 65535) return LMOD_EINVAL;
  a.x2 = (const bf16_t*)q_logits; a.ld2 = ld_q; a.R1 = B * (k + 1);
  a.vec = a.vec && (ld_q % 8 == 0) && ((uintptr_t)q_logits % 16 == 0);
  sa.spec_bytes = SPEC_HDR_BYTES + 16LL * a.C;
  if (ws_bytes < a.row_bytes * R + sa.spec_bytes * B) return LMOD_EINVAL;
  sa.spec = a.ws + a.row_bytes * R;
  sa.B = B; sa.k = k; sa.eos = eos; sa.pad = pad;
  sa.draft = draft; sa.u_acc = u_acc; sa.u_draw = u_draw;
  sa.done = done; sa.lens_target = lens_target; sa.lens_draft = lens_draft; sa.out = out; sa.next_token = next_token;
  sa.out_stats = out_stats;
  sample_launch_filter(a, R, stream);
  hipLaunchKernelGGL(spec_sample_accept_kernel, dim3(B), dim3(256), 0, stream, sa);
  hipLaunchKernelGGL(spec_sample_residual_kernel, dim3(a.C, B), dim3(256), 0, stream, sa);
  hipLaunchKernelGGL(spec_sample_draw_kernel, dim3(B), dim3(256), 0, stream, sa);
  return lmod_launch_status();
}

int lmod_spec_uniform(unsigned long long seed, int row0, int round, int purpose, int n_pos, float* u, int B, hipStream_t stream) {
  if (B < 0 || n_pos < 1 || purpose < 0 || purpose > 2 || round < 0 || row0 < 0) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!u) return LMOD_EINVAL;
  const long long n = (long long)B * n_pos;
  hipLaunchKernelGGL(spec_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, row0, round, purpose, n_pos, u,
                     n);
  return lmod_launch_status();
}

}  // extern "C"
