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
#include "common.h"

typedef unsigned long long u64;

#define SAMPLE_HDR_BYTES 64
#define SAMPLE_HIST_BYTES 3072
#define SAMPLE_FIX 1099511627776.f   // 2^40

struct SampleArgs {
  const bf16_t* x; long long ld; int V, chunk, C, vec, nh; float T; int top_k, use_p; float top_p;
  unsigned char* ws; long long row_bytes;
};

// header words of a row (u64): written by workgroup 0 of the pass that derives them, read by later launches
enum { H_KSEL = 0,    // top-k high bin | count above it << 32
       H_KMASS = 1,   // mass above the top-k high bin
       H_PSEL = 2,    // top-k cutoff key | top-p high bin << 16 | count above that bin << 32
       H_P = 3,       // floor(top_p * mass of the top-k set)
       H_PMASS = 4,   // mass above the top-p high bin
       H_CUT = 5,     // final cutoff key | number of kept tokens << 32
       H_TOTAL = 6 }; // mass of all V tokens

struct Sel { int bin; uint32_t c_above, c_incl; u64 m_above, m_incl, total, P; };
struct SampleSmem { u64 sm[4]; uint32_t sc[4]; int red[4]; Sel sel; u64 v0, v1; int i0; };

__device__ __forceinline__ u64* s_hdr(const SampleArgs& a, int r) { return (u64*)(a.ws + r * a.row_bytes); }
__device__ __forceinline__ u64* s_hmass(const SampleArgs& a, int r, int h) {
  return (u64*)(a.ws + r * a.row_bytes + SAMPLE_HDR_BYTES + h * SAMPLE_HIST_BYTES);
}
__device__ __forceinline__ uint32_t* s_hcnt(const SampleArgs& a, int r, int h) { return (uint32_t*)(s_hmass(a, r, h) + 256); }
__device__ __forceinline__ u64* s_cmass(const SampleArgs& a, int r) {
  return (u64*)(a.ws + r * a.row_bytes + SAMPLE_HDR_BYTES + a.nh * SAMPLE_HIST_BYTES);
}
__device__ __forceinline__ int* s_cmax(const SampleArgs& a, int r) { return (int*)(s_cmass(a, r) + a.C); }

// 16-bit key of a bf16 bit pattern: a larger value has a larger key; -0 shares +0's key
__device__ __forceinline__ uint32_t skey(uint32_t b) {
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float skey_value(uint32_t k) { return bf2f((bf16_t)((k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu))); }

// fixed-point weight of a logit; the one expression every pass uses.  NaN (inf - inf, NaN logits) and -inf weigh 0.
__device__ __forceinline__ u64 sweight(float f, float m, float T) {
  const float w = expf((f - m) / T);
  return w > 0.f ? __float2ull_rn(w * SAMPLE_FIX) : 0ull;
}

// f(bits, token) over tokens [lo, hi) of a row: 16-byte vector path plus a scalar tail (or all scalar when the row is unaligned)
template <class F>
__device__ __forceinline__ void for_tokens(const bf16_t* row, int lo, int hi, int vec, int tid, F f) {
  int tail = lo;
  if (vec) {
    const int nv = (hi - lo) >> 3;
    for (int q = tid; q < nv; q += 256) {
      const int base = lo + (q << 3);
      const u32x4 w = *(const u32x4*)(row + base);
#pragma unroll
      for (int j = 0; j < 4; ++j) { f(w[j] & 0xffffu, base + 2 * j); f(w[j] >> 16, base + 2 * j + 1); }
    }
    tail = lo + (nv << 3);
  }
  for (int e = tail + tid; e < hi; e += 256) f((uint32_t)row[e], e);
}

// inclusive scan of (c, m) over the 256 threads in thread order
__device__ __forceinline__ void scan256(uint32_t& c, u64& m, SampleSmem* s) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t tc = __shfl_up(c, o, 64);
    const u64 tm = __shfl_up(m, o, 64);
    if (lane >= o) { c += tc; m += tm; }
  }
  __syncthreads();
  if (lane == 63) { s->sc[w] = c; s->sm[w] = m; }
  __syncthreads();
  for (int j = 0; j < w; ++j) { c += s->sc[j]; m += s->sm[j]; }
}

__device__ __forceinline__ u64 block_sum_u64(u64 v, SampleSmem* s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s->sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return s->sm[0] + s->sm[1] + s->sm[2] + s->sm[3];
}

__device__ __forceinline__ int block_max_int(int v, SampleSmem* s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s->red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(s->red[0], s->red[1]), max(s->red[2], s->red[3]));
}

// the row's maximum logit from the chunk maxima
__device__ __forceinline__ float row_max_value(const int* cmax, int C, SampleSmem* s) {
  int k = 0;
  for (int c = threadIdx.x; c < C; c += 256) k = max(k, cmax[c]);
  return skey_value((uint32_t)block_max_int(k, s));
}

// Walk the 256 bins from the top (thread t holds bin 255 - t).  sel_count: the bin in which the descending count reaches k
// (1 <= k <= total count).  Every thread gets the result.
__device__ __forceinline__ Sel sel_count(const uint32_t* cnt, const u64* mass, uint32_t k, SampleSmem* s) {
  const int g = 255 - threadIdx.x;
  const uint32_t c = cnt[g];
  const u64 mm = mass[g];
  uint32_t ic = c;
  u64 im = mm;
  __syncthreads();
  if (threadIdx.x == 0) s->sel = Sel{0, 0, 0, 0, 0, 0, 0};
  scan256(ic, im, s);
  if (ic >= k && ic - c < k) { s->sel.bin = g; s->sel.c_above = ic - c; s->sel.c_incl = ic; s->sel.m_above = im - mm; s->sel.m_incl = im; }
  if (threadIdx.x == 255) s->sel.total = im;
  __syncthreads();
  return s->sel;
}

// sel_mass: the lowest non-empty bin >= lb whose mass above it (base + the bins above) is <= P.  derive: P = floor(top_p * total
// of these bins) instead of the argument.  The top non-empty bin always qualifies when base <= P.
__device__ __forceinline__ Sel sel_mass(const uint32_t* cnt, const u64* mass, bool derive, double top_p, u64 P, u64 base, int lb,
                                        SampleSmem* s) {
  const int g = 255 - threadIdx.x;
  const uint32_t c = cnt[g];
  const u64 mm = mass[g];
  uint32_t ic = c;
  u64 im = mm;
  __syncthreads();
  if (threadIdx.x == 0) { s->sel = Sel{0, 0, 0, 0, 0, 0, 0}; s->sel.bin = 256; }
  scan256(ic, im, s);
  if (threadIdx.x == 255) s->sel.total = im;
  __syncthreads();
  if (derive) P = (u64)(top_p * (double)s->sel.total);
  if (c > 0 && base + (im - mm) <= P && g >= lb) atomicMin(&s->sel.bin, g);
  __syncthreads();
  const int b = min(s->sel.bin, 255);
  __syncthreads();
  if (g == b) { s->sel.bin = b; s->sel.c_above = ic - c; s->sel.c_incl = ic; s->sel.m_above = im - mm; s->sel.m_incl = im; s->sel.P = P; }
  __syncthreads();
  return s->sel;
}

// the top-k cutoff from the published high-byte selection and the low-byte histogram (hist 1): key, tokens kept, their mass
__device__ __forceinline__ void resolve_topk(const SampleArgs& a, int r, SampleSmem* s, uint32_t& key, uint32_t& n_kept, u64& mass) {
  const u64* h = s_hdr(a, r);
  const uint32_t hi = (uint32_t)(h[H_KSEL] & 0xff), above = (uint32_t)(h[H_KSEL] >> 32);
  const Sel lo = sel_count(s_hcnt(a, r, 1), s_hmass(a, r, 1), (uint32_t)a.top_k - above, s);
  key = (hi << 8) | (uint32_t)lo.bin;
  n_kept = above + lo.c_incl;
  mass = h[H_KMASS] + lo.m_incl;
}

// Pass 1: grid (C, R).  Chunk maximum (as a key); the chunk's workgroups also zero the row's header and histograms.
__global__ __launch_bounds__(256) void sample_max_kernel(SampleArgs a) {
  __shared__ SampleSmem s;
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const bf16_t* row = a.x + (long long)r * a.ld;
  const int lo = c * a.chunk, hi = min(a.V, lo + a.chunk);
  int k = 0;
  for_tokens(row, lo, hi, a.vec, tid, [&](uint32_t b, int) { k = max(k, (int)skey(b)); });
  k = block_max_int(k, &s);
  if (tid == 0) s_cmax(a, r)[c] = k;
  const int words = (SAMPLE_HDR_BYTES + a.nh * SAMPLE_HIST_BYTES) / 4, per = (words + a.C - 1) / a.C;
  uint32_t* z = (uint32_t*)s_hdr(a, r);
  for (int i = c * per + tid; i < min(words, (c + 1) * per); i += 256) z[i] = 0;
}

// Pass 2: grid (C, R).  mode 0: histogram of the key's high byte over every token -> hist 0.  mode 1: low byte of the tokens in
// the top-k high bin -> hist 1.  mode 2: low byte of the tokens in the top-p high bin -> hist `hidx`.
__global__ __launch_bounds__(256) void sample_hist_kernel(SampleArgs a, int mode, int hidx) {
  __shared__ SampleSmem s;
  __shared__ u64 hm[256];
  __shared__ uint32_t hc[256];
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const bf16_t* row = a.x + (long long)r * a.ld;
  const int lo = c * a.chunk, hi = min(a.V, lo + a.chunk);
  hm[tid] = 0;
  hc[tid] = 0;
  const float m = row_max_value(s_cmax(a, r), a.C, &s);
  int sel = -1;
  if (mode == 1) {
    const Sel k = sel_count(s_hcnt(a, r, 0), s_hmass(a, r, 0), (uint32_t)a.top_k, &s);
    sel = k.bin;
    if (c == 0 && tid == 0) {
      u64* h = s_hdr(a, r);
      h[H_KSEL] = (u64)k.bin | ((u64)k.c_above << 32); h[H_KMASS] = k.m_above; h[H_TOTAL] = k.total;
    }
  } else if (mode == 2) {
    uint32_t kk = 0, nk = 0;
    u64 mk = 0;
    if (a.top_k > 0) resolve_topk(a, r, &s, kk, nk, mk);
    const double tp = fmin(fmax((double)a.top_p, 0.0), 1.0);
    const Sel p = sel_mass(s_hcnt(a, r, 0), s_hmass(a, r, 0), a.top_k <= 0, tp, (u64)(tp * (double)mk), 0, (int)(kk >> 8), &s);
    sel = p.bin;
    if (c == 0 && tid == 0) {
      u64* h = s_hdr(a, r);
      h[H_PSEL] = (u64)kk | ((u64)p.bin << 16) | ((u64)p.c_above << 32); h[H_P] = p.P; h[H_PMASS] = p.m_above;
      if (a.top_k <= 0) h[H_TOTAL] = p.total;
    }
  }
  __syncthreads();
  const float T = a.T;
  for_tokens(row, lo, hi, a.vec, tid, [&](uint32_t b, int) {
    const uint32_t key = skey(b);
    uint32_t bin = key >> 8;
    if (mode != 0) {
      if ((int)bin != sel) return;
      bin = key & 255u;
    }
    const u64 w = sweight(bf2f((bf16_t)b), m, T);
    atomicAdd(&hc[bin], 1u);
    if (w) atomicAdd(&hm[bin], w);
  });
  __syncthreads();
  if (hc[tid]) {
    atomicAdd(&s_hcnt(a, r, hidx)[tid], hc[tid]);
    if (hm[tid]) atomicAdd(&s_hmass(a, r, hidx)[tid], hm[tid]);
  }
}

// Pass 3: grid (C, R).  The final cutoff key, then the chunk's kept mass.
__global__ __launch_bounds__(256) void sample_mass_kernel(SampleArgs a) {
  __shared__ SampleSmem s;
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const bf16_t* row = a.x + (long long)r * a.ld;
  const int lo = c * a.chunk, hi = min(a.V, lo + a.chunk);
  const float m = row_max_value(s_cmax(a, r), a.C, &s);
  uint32_t cut = 0, n_kept = (uint32_t)a.V;
  if (a.use_p) {
    const u64* h = s_hdr(a, r);
    const uint32_t kk = (uint32_t)(h[H_PSEL] & 0xffff), B = (uint32_t)((h[H_PSEL] >> 16) & 0xff), above = (uint32_t)(h[H_PSEL] >> 32);
    const int hidx = a.top_k > 0 ? 2 : 1;
    const int lb = (a.top_k > 0 && B == (kk >> 8)) ? (int)(kk & 255u) : 0;
    const Sel p = sel_mass(s_hcnt(a, r, hidx), s_hmass(a, r, hidx), false, 0.0, h[H_P], h[H_PMASS], lb, &s);
    cut = (B << 8) | (uint32_t)p.bin;
    n_kept = above + p.c_incl;
  } else if (a.top_k > 0) {
    u64 mk;
    resolve_topk(a, r, &s, cut, n_kept, mk);
  }
  if ((a.use_p || a.top_k > 0) && c == 0 && tid == 0) s_hdr(a, r)[H_CUT] = (u64)cut | ((u64)n_kept << 32);
  const float T = a.T;
  u64 sum = 0;
  for_tokens(row, lo, hi, a.vec, tid, [&](uint32_t b, int) {
    if (skey(b) >= cut) sum += sweight(bf2f((bf16_t)b), m, T);
  });
  sum = block_sum_u64(sum, &s);
  if (tid == 0) s_cmass(a, r)[c] = sum;
}

// Pass 4: one workgroup per row.  target = floor(u * kept mass); the chunk, then the token, at which the running kept mass in
// token order first exceeds it; the stats.
__global__ __launch_bounds__(256) void sample_draw_kernel(SampleArgs a, const float* __restrict__ u, int* __restrict__ out_token,
                                                          float* __restrict__ out_stats) {
  __shared__ SampleSmem s;
  __shared__ int s_found;
  const int r = blockIdx.x, tid = threadIdx.x;
  const bf16_t* row = a.x + (long long)r * a.ld;
  const float m = row_max_value(s_cmax(a, r), a.C, &s);
  const bool filt = a.use_p || a.top_k > 0;
  const u64* h = s_hdr(a, r);
  const uint32_t cut = filt ? (uint32_t)(h[H_CUT] & 0xffff) : 0u;
  const uint32_t n_kept = filt ? (uint32_t)(h[H_CUT] >> 32) : (uint32_t)a.V;
  const u64* cmass = s_cmass(a, r);
  u64 part = 0;
  for (int c = tid; c < a.C; c += 256) part += cmass[c];
  const u64 kept = block_sum_u64(part, &s);
  const u64 total = filt ? h[H_TOTAL] : kept;
  int tok = 0;
  if (kept > 0) {
    const u64 want = (u64)((double)u[r] * (double)kept);
    const u64 target = want < kept ? want : kept - 1;
    // the chunk that holds the target
    u64 run = 0;
    __syncthreads();
    if (tid == 0) { s.i0 = a.C - 1; s.v1 = 0; }
    for (int c0 = 0; c0 < a.C; c0 += 256) {
      const int c = c0 + tid;
      const u64 v = c < a.C ? cmass[c] : 0ull;
      u64 iv = v;
      uint32_t one = 0;
      scan256(one, iv, &s);
      if (tid == 255) s.v0 = iv;
      if (v > 0 && run + (iv - v) <= target && target < run + iv) { s.i0 = c; s.v1 = target - (run + (iv - v)); }
      __syncthreads();
      const u64 tile = s.v0;
      if (target < run + tile) break;
      run += tile;
      __syncthreads();
    }
    __syncthreads();
    const int cs = s.i0;
    const u64 rem = s.v1;
    const int lo = cs * a.chunk, hi = min(a.V, lo + a.chunk);
    if (tid == 0) s_found = -1;
    __syncthreads();
    const float T = a.T;
    u64 run2 = 0;
    int lastk = -1;
    for (int base = lo; base < hi; base += 2048) {
      const int e0 = base + tid * 8;
      u64 w[8];
      if (a.vec && e0 + 8 <= hi) {
        const u32x4 q = *(const u32x4*)(row + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t b0 = q[j] & 0xffffu, b1 = q[j] >> 16;
          w[2 * j] = skey(b0) >= cut ? sweight(bf2f((bf16_t)b0), m, T) : 0ull;
          w[2 * j + 1] = skey(b1) >= cut ? sweight(bf2f((bf16_t)b1), m, T) : 0ull;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t b = e0 + j < hi ? (uint32_t)row[e0 + j] : 0xff80u;      // -inf past the end
          w[j] = (e0 + j < hi && skey(b) >= cut) ? sweight(bf2f((bf16_t)b), m, T) : 0ull;
        }
      }
      u64 sum = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sum += w[j];
        if (w[j]) lastk = e0 + j;
      }
      u64 iv = sum;
      uint32_t one = 0;
      scan256(one, iv, &s);
      if (tid == 255) s.v0 = iv;
      const u64 ex = run2 + (iv - sum);
      if (sum > 0 && ex <= rem && rem < ex + sum) {
        u64 cum = ex;
        int pick = -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          cum += w[j];
          if (pick < 0 && cum > rem) pick = e0 + j;
        }
        s_found = pick;
      }
      __syncthreads();
      if (s_found >= 0) break;
      run2 += s.v0;
      __syncthreads();
    }
    tok = s_found;
    if (tok < 0) tok = block_max_int(lastk, &s);          // rounding ran past the end: the last kept token
    tok = min(max(tok, 0), a.V - 1);
  }
  if (tid == 0) {
    out_token[r] = tok;
    if (out_stats) {
      float* st = out_stats + 4 * (long long)r;
      st[0] = total > 0 ? (float)((double)m / (double)a.T + log((double)total) - 40.0 * 0.6931471805599453) : -INFINITY;
      st[1] = total > 0 ? (float)((double)kept / (double)total) : 0.f;
      st[2] = (float)n_kept;
      st[3] = filt ? skey_value(cut) : -INFINITY;
    }
  }
}

extern "C" {

int lmod_sample_bf16(const void* logits, long long ld, int V, const float* u, int R, float temperature, int top_k, float top_p,
                     int chunk, void* ws, long long ws_bytes, int* out_token, float* out_stats, hipStream_t stream) {
  if (R < 0 || R > 65535 || V < 2 || ld < V || chunk < 8 || (chunk & 7)) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!logits || !u || !ws || !out_token || ((uintptr_t)ws & 7)) return LMOD_EINVAL;
  const int C = (V + chunk - 1) / chunk;
  if (C > 65535) return LMOD_EINVAL;
  const int use_k = top_k > 0 && top_k < V, use_p = top_p < 1.f;
  SampleArgs a;
  a.x = (const bf16_t*)logits; a.ld = ld; a.V = V; a.chunk = chunk; a.C = C;
  a.vec = (ld % 8 == 0) && ((uintptr_t)logits % 16 == 0);
  a.nh = (use_k || use_p) ? 1 + use_k + use_p : 0;
  a.T = fmaxf(temperature, 1e-6f);
  a.top_k = use_k ? top_k : 0; a.use_p = use_p; a.top_p = top_p;
  a.ws = (unsigned char*)ws;
  a.row_bytes = SAMPLE_HDR_BYTES + (long long)SAMPLE_HIST_BYTES * a.nh + 16LL * C;
  if (ws_bytes < a.row_bytes * R) return LMOD_EINVAL;
  const dim3 grid(C, R), block(256);
  hipLaunchKernelGGL(sample_max_kernel, grid, block, 0, stream, a);
  if (a.nh) {
    hipLaunchKernelGGL(sample_hist_kernel, grid, block, 0, stream, a, 0, 0);
    if (use_k) hipLaunchKernelGGL(sample_hist_kernel, grid, block, 0, stream, a, 1, 1);
    if (use_p) hipLaunchKernelGGL(sample_hist_kernel, grid, block, 0, stream, a, 2, use_k ? 2 : 1);
  }
  hipLaunchKernelGGL(sample_mass_kernel, grid, block, 0, stream, a);
  hipLaunchKernelGGL(sample_draw_kernel, dim3(R), block, 0, stream, a, u, out_token, out_stats);
  return lmod_launch_status();
}

}  // extern "C"
