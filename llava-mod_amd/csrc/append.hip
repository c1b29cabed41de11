// Multi-token extension of a KV cache on gfx950 (lmod_attn_append / lmod_attn_append_nsplit / lmod_kv_append_rows /
// lmod_spec_accept): a chunk of T > 1 new tokens per sample against an existing cache in one pass — chunked continuation of a
// conversation and the verification step of greedy assisted (speculative) decoding (HF generate(assistant_model=...)).
//
// ---------------------------------------------------------------------------- lmod_attn_append: the arithmetic
// Sample b brings n_b <= T new tokens whose keys / values are ALREADY in the cache (positions lens[b] - n_b .. lens[b] - 1).  Query
// t sees the keys k <= lens[b] - n_b + t.  A kv head's group x n_b query rows (row r = t * group + g, at most APPEND_R_MAX = 128)
// are handled together, so a cached K / V row is fetched from HBM once per (sample, kv head) for all of them.
//
// Grid (key split s, kv head, sample), 256 threads.  The sample's 64-key chunks are dealt to the `nsplit` workgroups in
// contiguous runs of ceil(nchunks / nsplit).  Per chunk:
//   phase 1  lane <-> key, wave w <-> rows w, w + 4, ...: the lane's K row goes from global memory straight to registers (fp32, the
//            next chunk's row is prefetched during phase 2); score = sum_d (q_d * scale) * k_d, fp32 FMAs in ascending d, the
//            query pre-multiplied by `scale` in fp32 and broadcast from LDS; masked scores are -inf.  Online softmax per row over
//            the wave: m' = max(m, chunk max), alpha = exp(m - m'), p = exp(score - m') (fp32, NOT rounded to bf16),
//            l = l * alpha + sum p.  exp(x) is __expf: exp2 of the fp32 product x * log2(e).
//   phase 2  lane <-> feature (hd 64) or feature pair (hd 128), wave w <-> the same rows: acc = acc * alpha + sum_k p_k v_k, fp32
//            FMAs in ascending key order, the chunk's V column in registers, p broadcast from LDS.
// The products run on the VALU: the kernel is bound by the K / V read and the rows (<= 128) x keys x hd products of a chunk cost a
// few microseconds per workgroup; an MFMA form would need P in bf16 — a rounding point this kernel does not have.
// nsplit == 1: out = bf16(acc / l) — the ONLY rounding to bf16.  nsplit > 1: every split stores (m, l, acc) in fp32 to the
// caller's workspace and attn_append_merge_kernel adds them in split order s = 0, 1, ...: M = max m_s, L = sum l_s exp(m_s - M),
// out = bf16(sum acc_s exp(m_s - M) / L) — fixed order, no atomics, so two calls give the same bits.  Splits without a visible
// key carry m = -inf and are skipped.  A row without any visible key (unit 0) is exactly 0.  Keys >= lens[b] are never loaded.
//
// T <= APPEND_T_MAX = 16 and group * T <= APPEND_R_MAX = 128 (LMOD_EUNSUPPORTED beyond); T = 1 is lmod_attn_decode's case with
// a different summation order (same bound, not the same bits).
#include "common.h"
#include <atomic>

#define APPEND_T_MAX 16
#define APPEND_R_MAX 128
#define APPEND_KC 64
#define APPEND_NSPLIT_MAX 32

// LDS floats for R rows: q [R][HD], p [R][64], m / l / alpha [R] each
static inline size_t append_lds_bytes(int R, int hd) { return (size_t)R * (hd + APPEND_KC + 3) * sizeof(float); }

template <int HD>
__device__ __forceinline__ void append_load_k(u32x4 (&kp)[HD / 8], const bf16_t* __restrict__ kb, int key, int len, int ldc) {
  if (key < len) {
    const u32x4* kr = (const u32x4*)(kb + (long long)key * ldc);
#pragma unroll
    for (int j = 0; j < HD / 8; ++j) kp[j] = kr[j];
  } else {
#pragma unroll
    for (int j = 0; j < HD / 8; ++j) kp[j] = u32x4{0u, 0u, 0u, 0u};
  }
}

template <int HD, int RPT>
__global__ __launch_bounds__(256) void attn_append_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                                         const bf16_t* __restrict__ vc, const int* __restrict__ lens,
                                                         const int* __restrict__ cu, bf16_t* __restrict__ out,
                                                         float* __restrict__ ws, int group, int T, int smax, int ldq, int ldc,
                                                         int ldo, float scale, int nsplit) {
  extern __shared__ float smem[];
  constexpr int FPT = HD / 64;                                   // features per lane in phase 2
  const int s = blockIdx.x, hk = blockIdx.y, b = blockIdx.z, nkv = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = min(cu ? cu[b + 1] - cu[b] : T, T);
  if (n <= 0) return;
  const long long row0 = cu ? cu[b] : (long long)b * T;
  const int len = max(0, min(lens[b], smax));
  const int R = group * n, Rws = group * T;
  float* sq = smem;                                              // [R][HD] scaled queries
  float* sp = sq + (size_t)Rws * HD;                             // [R][64] probabilities of the current chunk
  float* sm = sp + (size_t)Rws * APPEND_KC;                      // [R] running max
  float* sl = sm + Rws;                                          // [R] running sum
  float* sa = sl + Rws;                                          // [R] rescale factor of the current chunk
  for (int i = tid; i < R * HD; i += 256) {
    const int r = i / HD, d = i - r * HD, t = r / group, g = r - t * group;
    sq[i] = bf2f(q[(row0 + t) * ldq + (hk * group + g) * HD + d]) * scale;
  }
  for (int r = tid; r < R; r += 256) { sm[r] = -INFINITY; sl[r] = 0.f; }
  const bf16_t* kb = kc + (long long)b * smax * ldc + hk * HD;
  const bf16_t* vb = vc + (long long)b * smax * ldc + hk * HD + lane * FPT;
  const int nchunks = (len + APPEND_KC - 1) / APPEND_KC, cps = (nchunks + nsplit - 1) / nsplit;
  const int c_begin = s * cps, c_end = min(nchunks, c_begin + cps);
  float acc[RPT][FPT];
#pragma unroll
  for (int i = 0; i < RPT; ++i)
#pragma unroll
    for (int f = 0; f < FPT; ++f) acc[i][f] = 0.f;
  u32x4 kp[HD / 8];
  if (c_begin < c_end) append_load_k<HD>(kp, kb, c_begin * APPEND_KC + lane, len, ldc);
  __syncthreads();
  for (int c = c_begin; c < c_end; ++c) {
    const int key = c * APPEND_KC + lane;
    // ---- phase 1: scores and the online softmax of rows w, w + 4, ...
    {
      float kf[HD];
#pragma unroll
      for (int j = 0; j < HD / 8; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { kf[j * 8 + 2 * e] = bflo(kp[j][e]); kf[j * 8 + 2 * e + 1] = bfhi(kp[j][e]); }
      for (int i = 0; i < RPT; ++i) {
        const int r = w + 4 * i;
        if (r >= R) break;
        const int t = r / group;
        const f32x4* qr = (const f32x4*)(sq + (size_t)r * HD);
        float a = 0.f;
#pragma unroll
        for (int d4 = 0; d4 < HD / 4; ++d4) {
          const f32x4 qv = qr[d4];
          a = fmaf(qv[0], kf[4 * d4], a); a = fmaf(qv[1], kf[4 * d4 + 1], a);
          a = fmaf(qv[2], kf[4 * d4 + 2], a); a = fmaf(qv[3], kf[4 * d4 + 3], a);
        }
        const float sc = (key <= len - n + t && key < len) ? a : -INFINITY;
        const float mold = sm[r];
        const float mnew = fmaxf(mold, wave_max(sc));
        const float alpha = (mnew == -INFINITY) ? 1.f : __expf(mold - mnew);
        const float p = (sc == -INFINITY) ? 0.f : __expf(sc - mnew);
        const float ps = wave_sum(p);
        sp[r * APPEND_KC + lane] = p;
        if (lane == 0) { sm[r] = mnew; sl[r] = sl[r] * alpha + ps; sa[r] = alpha; }
      }
    }
    __syncthreads();
    // ---- phase 2: rescale, prefetch the next chunk's K row, then the p-weighted sums in two halves of 32 keys (the half's V column
    //      of this lane's feature(s) in registers)
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int r = w + 4 * i;
      if (r < R) {
        const float alpha = sa[r];
#pragma unroll
        for (int f = 0; f < FPT; ++f) acc[i][f] *= alpha;
      }
    }
    if (c + 1 < c_end) append_load_k<HD>(kp, kb, key + APPEND_KC, len, ldc);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      constexpr int KH = APPEND_KC / 2;
      float vf[KH][FPT];
#pragma unroll
      for (int kk = 0; kk < KH; ++kk) {
        const int k2 = c * APPEND_KC + half * KH + kk;
        if (k2 < len) {
          if constexpr (FPT == 2) {
            const uint32_t x = *(const uint32_t*)(vb + (long long)k2 * ldc);
            vf[kk][0] = bflo(x); vf[kk][1] = bfhi(x);
          } else {
            vf[kk][0] = bf2f(vb[(long long)k2 * ldc]);
          }
        } else {
#pragma unroll
          for (int f = 0; f < FPT; ++f) vf[kk][f] = 0.f;
        }
      }
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int r = w + 4 * i;
        if (r < R) {
          const f32x4* pr = (const f32x4*)(sp + r * APPEND_KC + half * KH);
#pragma unroll
          for (int k4 = 0; k4 < KH / 4; ++k4) {
            const f32x4 pv = pr[k4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int f = 0; f < FPT; ++f) acc[i][f] = fmaf(pv[e], vf[4 * k4 + e][f], acc[i][f]);
          }
        }
      }
    }
    __syncthreads();
  }
  // ---- epilogue: the output rows (one split) or this split's fp32 partials
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int r = w + 4 * i;
    if (r >= R) continue;
    const int t = r / group, g = r - t * group;
    if (nsplit == 1) {
      const float l = sl[r], inv = l > 0.f ? 1.f / l : 0.f;
      bf16_t* o = out + (row0 + t) * ldo + (hk * group + g) * HD + lane * FPT;
      if constexpr (FPT == 2) *(uint32_t*)o = pack2bf(acc[i][0] * inv, acc[i][1] * inv);
      else *o = f2bf(acc[i][0] * inv);
    } else {
      const long long slot = (((long long)b * nkv + hk) * nsplit + s) * Rws + r;
      float* po = ws + slot * (HD + 2);
#pragma unroll
      for (int f = 0; f < FPT; ++f) po[lane * FPT + f] = acc[i][f];
      if (lane == 0) { po[HD] = sm[r]; po[HD + 1] = sl[r]; }
    }
  }
}

// One thread per (sample, chunk position, query head, feature): the splits' partials in index order.
__global__ __launch_bounds__(256) void attn_append_merge_kernel(const float* __restrict__ ws, const int* __restrict__ cu,
                                                               bf16_t* __restrict__ out, int B, int T, int nh, int group, int HD,
                                                               int ldo, int nsplit) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)B * T * nh * HD) return;
  const int d = (int)(id % HD);
  const int h = (int)(id / HD % nh);
  const int t = (int)(id / ((long long)HD * nh) % T);
  const int b = (int)(id / ((long long)HD * nh * T));
  const int n = min(cu ? cu[b + 1] - cu[b] : T, T);
  if (t >= n) return;
  const long long row = (cu ? cu[b] : (long long)b * T) + t;
  const int hk = h / group, r = t * group + (h - hk * group), nkv = nh / group, Rws = group * T;
  const float* base = ws + ((((long long)b * nkv + hk) * nsplit) * Rws + r) * (HD + 2);
  const long long stride = (long long)Rws * (HD + 2);
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, base[s * stride + HD]);
  float L = 0.f, O = 0.f;
  if (M > -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float m = base[s * stride + HD];
      if (m == -INFINITY) continue;
      const float e = __expf(m - M);
      L = fmaf(base[s * stride + HD + 1], e, L);
      O = fmaf(base[s * stride + d], e, O);
    }
  }
  out[row * ldo + h * HD + d] = f2bf(L > 0.f ? O / L : 0.f);
}

// grid (chunk position t, sample b): K and V columns of packed row cu[b] + t of the fused QKV buffer to cache position lens_before[b] + t
__global__ __launch_bounds__(256) void kv_append_rows_kernel(const bf16_t* __restrict__ qkv, int ldqkv, int kcol, int vcol, int width,
                                                            const int* __restrict__ cu, const int* __restrict__ lens_before,
                                                            bf16_t* __restrict__ kcache, bf16_t* __restrict__ vcache, int T, int smax,
                                                            int ldc) {
  const int t = blockIdx.x, b = blockIdx.y;
  const int n = min(cu ? cu[b + 1] - cu[b] : T, T);
  if (t >= n) return;
  const long long row = (cu ? cu[b] : (long long)b * T) + t;
  const int pos = lens_before[b] + t;
  if (pos < 0 || pos >= smax) return;                 // never writes outside the cache; the host wrapper rejects such a call
  const int nv = width >> 3;
  const long long dst = ((long long)b * smax + pos) * ldc;
  for (int i = threadIdx.x; i < 2 * nv; i += 256) {
    const int which = i >= nv, j = which ? i - nv : i;
    const u32x4 x = *(const u32x4*)(qkv + row * ldqkv + (which ? vcol : kcol) + j * 8);
    *(u32x4*)((which ? vcache : kcache) + dst + j * 8) = x;
  }
}

// One thread per sample: the acceptance rule of greedy assisted decoding (see include/lmod_hip.h).
__global__ __launch_bounds__(256) void spec_accept_kernel(const int* __restrict__ draft, const int* __restrict__ target, int k,
                                                         int* __restrict__ done, int eos, int pad, int* __restrict__ lens_target,
                                                         int* __restrict__ lens_draft, int* __restrict__ out,
                                                         int* __restrict__ next_token, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int* dr = draft + (long long)b * k;
  const int* tg = target + (long long)b * (k + 1);
  int* o = out + (long long)b * (k + 5);
  const int was_done = done[b] != 0;
  int n_acc = 0;
  if (!was_done)
    while (n_acc < k && dr[n_acc] == tg[n_acc]) ++n_acc;
  lens_target[b] += n_acc - k;                        // the verification pass appended k + 1; next_token + n_acc drafts stay
  lens_draft[b] += min(n_acc + 1, k) - k;             // the k draft steps appended next_token and drafts 1 .. k - 1
  int n_emit = 0, fin = was_done;
  if (!was_done) {
    n_emit = n_acc + 1;
    for (int i = 0; i <= n_acc; ++i) {
      const int tok = i < n_acc ? dr[i] : tg[n_acc];
      if (eos >= 0 && tok == eos) { n_emit = i + 1; fin = 1; break; }
    }
  }
  for (int i = 0; i <= k; ++i) o[i] = i < n_emit ? (i < n_acc ? dr[i] : tg[n_acc]) : pad;
  const int nxt = fin ? pad : tg[n_acc];
  o[k + 1] = n_acc; o[k + 2] = n_emit; o[k + 3] = nxt; o[k + 4] = fin;
  next_token[b] = nxt;
  done[b] = fin;
}

#define APPEND_MAX_DEVICES 64
static int append_device() {                          // the current device's slot in the per-device tables below
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  return dev % APPEND_MAX_DEVICES;
}

static int append_cus() {                             // CU count of the CURRENT device (a process may drive several)
  static std::atomic<int> cus[APPEND_MAX_DEVICES];
  const int dev = append_device();
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n <= 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

template <int HD, int RPT>
static int append_launch(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const int* lens, const int* cu, bf16_t* out, float* ws,
                         int B, int T, int nkv, int group, int smax, int ldq, int ldc, int ldo, float scale, int nsplit,
                         hipStream_t stream) {
  const size_t lds = append_lds_bytes(group * T, HD);
  // per instantiation AND device: the largest dynamic LDS size opted into so far (setting it twice from two threads is harmless)
  static std::atomic<size_t> lds_set[APPEND_MAX_DEVICES];
  const int dev = append_device();
  if (lds > lds_set[dev].load(std::memory_order_relaxed)) {
    if (hipFuncSetAttribute((const void*)attn_append_kernel<HD, RPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return LMOD_ELAUNCH;
    lds_set[dev].store(lds, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL((attn_append_kernel<HD, RPT>), dim3(nsplit, nkv, B), dim3(256), lds, stream, q, kc, vc, lens, cu, out, ws, group,
                     T, smax, ldq, ldc, ldo, scale, nsplit);
  return LMOD_OK;
}

extern "C" {

// The key-split count lmod_attn_append picks by itself (nsplit = 0) for B samples, nkv kv heads and caches of smax positions:
// enough workgroups for the chip, at most one per 64-key chunk and APPEND_NSPLIT_MAX.  Host-side query, no device work.
int lmod_attn_append_nsplit(int B, int nkv, int smax) {
  if (B < 1 || nkv < 1 || smax < 1) return 1;
  const long long wgs = (long long)B * nkv;
  long long n = (append_cus() + wgs - 1) / wgs;
  const int chunks = (smax + APPEND_KC - 1) / APPEND_KC;
  if (n > chunks) n = chunks;
  if (n > APPEND_NSPLIT_MAX) n = APPEND_NSPLIT_MAX;
  return n < 1 ? 1 : (int)n;
}

int lmod_attn_append(const void* q, const void* kcache, const void* vcache, const int* lens, const int* cu_new, void* out, int B, int T,
                     int nh, int nkv, int hd, int smax, int ldq, int ld_cache, int ldo, float scale, int nsplit, void* ws,
                     long long ws_bytes, hipStream_t stream) {
  if (B < 0 || T < 1 || nh <= 0 || nkv <= 0 || nh % nkv || smax <= 0 || nsplit < 0) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!q || !kcache || !vcache || !lens || !out) return LMOD_EINVAL;
  if (hd != 64 && hd != 128) return LMOD_EUNSUPPORTED;
  const int group = nh / nkv;
  if (T > APPEND_T_MAX || group * T > APPEND_R_MAX || nsplit > APPEND_NSPLIT_MAX || B > 65535 || nkv > 65535) return LMOD_EUNSUPPORTED;
  if ((ld_cache & 7) || ld_cache < nkv * hd || ldq < nh * hd || ldo < nh * hd || (ldo & 1) || ((uintptr_t)kcache & 15) ||
      ((uintptr_t)vcache & 15) || ((uintptr_t)out & 3))
    return LMOD_EINVAL;
  const long long need1 = (long long)B * nh * T * (hd + 2) * 4;          // workspace bytes per split
  if (nsplit == 0) {
    nsplit = lmod_attn_append_nsplit(B, nkv, smax);
    if (!ws || ws_bytes < need1 * nsplit) nsplit = (ws && ws_bytes >= 2 * need1) ? (int)(ws_bytes / need1) : 1;
  }
  if (nsplit > 1 && (!ws || ws_bytes < need1 * nsplit || ((uintptr_t)ws & 15))) return LMOD_EINVAL;
  const int rpt = (group * T + 3) / 4;
  int rc;
#define LMOD_APPEND_GO(HDV, RPTV)                                                                                                  \
  rc = append_launch<HDV, RPTV>((const bf16_t*)q, (const bf16_t*)kcache, (const bf16_t*)vcache, lens, cu_new, (bf16_t*)out, (float*)ws, B, \
                                T, nkv, group, smax, ldq, ld_cache, ldo, scale, nsplit, stream)
#define LMOD_APPEND_HD(HDV)                                                                                                        \
  if (rpt <= 2) LMOD_APPEND_GO(HDV, 2); else if (rpt <= 8) LMOD_APPEND_GO(HDV, 8); else if (rpt <= 16) LMOD_APPEND_GO(HDV, 16);     \
  else LMOD_APPEND_GO(HDV, 32)
  if (hd == 128) { LMOD_APPEND_HD(128); } else { LMOD_APPEND_HD(64); }
#undef LMOD_APPEND_HD
#undef LMOD_APPEND_GO
  if (rc) return rc;
  if (nsplit > 1) {
    const long long thr = (long long)B * T * nh * hd;
    hipLaunchKernelGGL(attn_append_merge_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, stream, (const float*)ws, cu_new,
                       (bf16_t*)out, B, T, nh, group, hd, ldo, nsplit);
  }
  return lmod_launch_status();
}

int lmod_kv_append_rows(const void* qkv, int ldqkv, int kcol, int vcol, int width, const int* cu_new, const int* lens_before,
                        void* kcache, void* vcache, int B, int T, int smax, int ld_cache, int max_len_after, hipStream_t stream) {
  if (B < 0 || T < 1 || smax < 1 || width < 8 || (width & 7) || kcol < 0 || vcol < 0 || (kcol & 7) || (vcol & 7) || (ldqkv & 7) ||
      (ld_cache & 7) || ld_cache < width || ldqkv < kcol + width || ldqkv < vcol + width)
    return LMOD_EINVAL;
  if (max_len_after > smax) return LMOD_EINVAL;      // the chunk would run past the cache: grow it first
  if (B == 0) return LMOD_OK;
  if (!qkv || !lens_before || !kcache || !vcache || ((uintptr_t)qkv & 15) || ((uintptr_t)kcache & 15) || ((uintptr_t)vcache & 15))
    return LMOD_EINVAL;
  if (T > 65535 || B > 65535) return LMOD_EUNSUPPORTED;
  hipLaunchKernelGGL(kv_append_rows_kernel, dim3(T, B), dim3(256), 0, stream, (const bf16_t*)qkv, ldqkv, kcol, vcol, width, cu_new,
                     lens_before, (bf16_t*)kcache, (bf16_t*)vcache, T, smax, ld_cache);
  return lmod_launch_status();
}

int lmod_spec_accept(const int* draft, const int* target, int k, int* done, int eos, int pad, int* lens_target, int* lens_draft,
                     int* out, int* next_token, int B, hipStream_t stream) {
  if (B < 0 || k < 1 || k >= APPEND_T_MAX) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!draft || !target || !done || !lens_target || !lens_draft || !out || !next_token) return LMOD_EINVAL;
  hipLaunchKernelGGL(spec_accept_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, draft, target, k, done, eos, pad, lens_target,
                     lens_draft, out, next_token, B);
  return lmod_launch_status();
}

}  // extern "C"
