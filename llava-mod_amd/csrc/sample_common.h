// What lmod_sample_bf16 (sample.hip), lmod_spec_sample_bf16 (specsample.hip) and lmod_sample_rows_bf16 (sample_rows.hip) share: the 16-bit key of a bf16 logit, the fixed-point
// weight, the token loops, the 256-thread scans, the radix selection over the row histograms in `ws`, the inverse-CDF draw of one row
// and the stats record.  The contract, the workspace layout and the reasons are in sample.hip's header comment.  The filter passes
// themselves (chunk max, histograms, kept mass) are device functions here too (sample_pass_*): sample.hip wraps them in its kernels,
// which specsample.hip launches through sample_launch_filter; sample_rows.hip calls them with per-row arguments.
#pragma once
#include "common.h"

typedef unsigned long long u64;

#define SAMPLE_HDR_BYTES 64
#define SAMPLE_HIST_BYTES 3072
#define SAMPLE_FIX 1099511627776.f   // 2^40

// rows [0, R1) are x + r * ld; rows >= R1 (lmod_spec_sample_bf16's draft rows; lmod_sample_bf16 has none) x2 + (r - R1) * ld2
struct SampleArgs {
  const bf16_t* x; long long ld; int V, chunk, C, vec, nh; float T; int top_k, use_p; float top_p;
  unsigned char* ws; long long row_bytes;
  const bf16_t* x2; long long ld2; int R1;
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
struct SampleSmem { u64 sm[4]; uint32_t sc[4]; int red[4]; Sel sel; u64 v0, v1; int i0, found; };

__device__ __forceinline__ const bf16_t* s_row(const SampleArgs& a, int r) {
  return r < a.R1 ? a.x + (long long)r * a.ld : a.x2 + (long long)(r - a.R1) * a.ld2;
}
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

// ---------------------------------------------------------------------------------------------- the filter passes of one workgroup
// The bodies of sample.hip's kernels as device functions of (a, chunk c, row r): lmod_sample_bf16 / lmod_spec_sample_bf16 call them
// with the launch's SampleArgs, lmod_sample_rows_bf16 (sample_rows.hip) with a per-row copy.  Every thread of the workgroup calls.

// Pass 1.  Chunk maximum (as a key); the chunk's workgroups also zero the row's header and histograms.
__device__ __forceinline__ void sample_pass_max(const SampleArgs& a, int c, int r, SampleSmem* sp) {
  const int tid = threadIdx.x;
  const bf16_t* row = s_row(a, r);
  const int lo = c * a.chunk, hi = min(a.V, lo + a.chunk);
  int k = 0;
  for_tokens(row, lo, hi, a.vec, tid, [&](uint32_t b, int) { k = max(k, (int)skey(b)); });
  k = block_max_int(k, sp);
  if (tid == 0) s_cmax(a, r)[c] = k;
  const int words = (SAMPLE_HDR_BYTES + a.nh * SAMPLE_HIST_BYTES) / 4, per = (words + a.C - 1) / a.C;
  uint32_t* z = (uint32_t*)s_hdr(a, r);
  for (int i = c * per + tid; i < min(words, (c + 1) * per); i += 256) z[i] = 0;
}

// Pass 2.  mode 0: histogram of the key's high byte over every token -> hist 0.  mode 1: low byte of the tokens in the top-k high
// bin -> hist 1.  mode 2: low byte of the tokens in the top-p high bin -> hist `hidx`.  hm / hc: 256-entry LDS histograms.
__device__ __forceinline__ void sample_pass_hist(const SampleArgs& a, int c, int r, int mode, int hidx, SampleSmem* sp, u64* hm,
                                                 uint32_t* hc) {
  SampleSmem& s = *sp;
  const int tid = threadIdx.x;
  const bf16_t* row = s_row(a, r);
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

// Pass 3.  The final cutoff key, then the chunk's kept mass.
__device__ __forceinline__ void sample_pass_mass(const SampleArgs& a, int c, int r, SampleSmem* sp) {
  SampleSmem& s = *sp;
  const int tid = threadIdx.x;
  const bf16_t* row = s_row(a, r);
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

// The draw of one row by its whole workgroup (256 threads, every thread calls): target = floor(u * kept mass); the chunk, then the
// token, at which the running kept mass in token order first exceeds it.  Needs the row's finished filter passes.  Every thread
// returns the token (0 when the kept mass is 0) and the row's maximum logit, kept mass, cutoff key and kept count.
__device__ __forceinline__ int sample_draw_row(const SampleArgs& a, int r, float u, SampleSmem* sp, float& m_out, u64& kept_out,
                                               uint32_t& cut_out, uint32_t& n_kept_out) {
  SampleSmem& s = *sp;
  const int tid = threadIdx.x;
  const bf16_t* row = s_row(a, r);
  const float m = row_max_value(s_cmax(a, r), a.C, &s);
  const bool filt = a.use_p || a.top_k > 0;
  const u64* h = s_hdr(a, r);
  const uint32_t cut = filt ? (uint32_t)(h[H_CUT] & 0xffff) : 0u;
  n_kept_out = filt ? (uint32_t)(h[H_CUT] >> 32) : (uint32_t)a.V;
  const u64* cmass = s_cmass(a, r);
  u64 part = 0;
  for (int c = tid; c < a.C; c += 256) part += cmass[c];
  const u64 kept = block_sum_u64(part, &s);
  m_out = m; kept_out = kept; cut_out = cut;
  int tok = 0;
  if (kept > 0) {
    const u64 want = (u64)((double)u * (double)kept);
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
    if (tid == 0) s.found = -1;
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
        s.found = pick;
      }
      __syncthreads();
      if (s.found >= 0) break;
      run2 += s.v0;
      __syncthreads();
    }
    tok = s.found;
    if (tok < 0) tok = block_max_int(lastk, &s);          // rounding ran past the end: the last kept token
    tok = min(max(tok, 0), a.V - 1);
  }
  return tok;
}

// out_stats record of a row: {logsumexp of x over all V, kept mass / total mass, number of kept tokens, cutoff logit}
__device__ __forceinline__ void sample_write_stats(const SampleArgs& a, int r, float* st, float m, u64 kept, uint32_t cut,
                                                   uint32_t n_kept) {
  const bool filt = a.use_p || a.top_k > 0;
  const u64 total = filt ? s_hdr(a, r)[H_TOTAL] : kept;
  st[0] = total > 0 ? (float)((double)m / (double)a.T + log((double)total) - 40.0 * 0.6931471805599453) : -INFINITY;
  st[1] = total > 0 ? (float)((double)kept / (double)total) : 0.f;
  st[2] = (float)n_kept;
  st[3] = filt ? skey_value(cut) : -INFINITY;
}

// Host side, defined in sample.hip.  sample_args_init: checks the shape / filter arguments both entry points share (all but the chunk
// count, which each entry point checks behind its own no-op and pointer checks) and fills `a` for one row block (a.R1 = R, no second
// block; a.vec from `logits` and `ld` alone: lmod_spec_sample_bf16 adds its second block and ANDs its alignment in); LMOD_OK or
// LMOD_EINVAL.  sample_launch_filter: the filter passes over R rows (grid chunks x rows): chunk max, [high-byte histogram, low-byte
// histogram per active filter], kept mass: 2 launches without a filter, 4 with one, 5 with both.
int sample_args_init(SampleArgs& a, const void* logits, long long ld, int V, int R, float temperature, int top_k, float top_p, int chunk,
                     void* ws);
void sample_launch_filter(const SampleArgs& a, int R, hipStream_t stream);
