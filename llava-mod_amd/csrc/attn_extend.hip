// Long-chunk extension of a KV cache on gfx950 (lmod_attn_extend): causal flash attention of a ragged chunk of up to 65535 new
// queries per sample against a cache that already holds a prefix AND the chunk's own keys / values — a later turn of a
// conversation (hundreds of text tokens, an image's 576 rows) in ONE pass over the weights.  Same conventions as lmod_attn_append
// (append.hip), which keeps T <= 16 and stays the kernel of the short chunks.
//
// ---------------------------------------------------------------------------- the arithmetic
// Sample b brings n_b <= T new tokens whose keys / values are ALREADY in the cache (positions lens[b] - n_b .. lens[b] - 1).  Query
// t sees the keys k <= lens[b] - n_b + t (and k < lens[b]).
//   S    = Q K^T                      bf16 x bf16 MFMA products, fp32 accumulation over hd
//   m    = running row max of S over the 64-key tiles seen so far (raw score units); masked scores are -inf by a select
//   p    = exp2(S * c - m * c), c = scale * log2(e), fp32;  l = l * alpha + sum p (the fp32 p, BEFORE its rounding),
//          alpha = exp2((m_old - m_new) * c)
//   O    = O * alpha + p V            bf16 MFMA products, fp32 accumulation over the keys; p enters as THREE bf16 terms
//                                     hi = bf16(p), mid = bf16(p - hi), lo = bf16(p - hi - mid), which together hold the fp32 p
//                                     exactly (3 x 8 significand bits), added smallest term first: P is NOT rounded to bf16
//   out  = bf16(O * (1 / l))          the ONLY rounding to bf16
// Why three terms: with P rounded once to bf16 (as the prefill's kernel does) every output carries a relative error of about 2^-9,
// and the K / V rows the NEXT layer appends to the cache then differ from the decode path's in 20 % of their elements by more than
// one bf16 ulp (measured on the golden small models); a conversation continued by a chunk and one continued token by token would
// hold different caches.  With the fp32 p the two paths agree as lmod_attn_append and lmod_attn_decode do.  The two extra MFMAs per
// P V product are a small cost next to the pass over the weights that surrounds this kernel.
// A row without a visible key has l = 0 and is exactly 0.  K / V rows at positions >= lens[b] are never loaded: their LDS rows are
// zero, so stale or non-finite data behind lens cannot reach an MFMA.  No address at or beyond (b + 1) * smax rows is formed.
// One workgroup owns a query tile from the first key tile to the last: no key split, no atomics, two calls give the same bits.
//
// ---------------------------------------------------------------------------- geometry
// Grid (query tile of 128 rows, query head, sample), 256 threads = 4 waves x 32 queries (two 16-query MFMA tiles), key tiles of 64.
// A workgroup whose first row is >= n_b exits before any barrier; rows >= n_b of a partial tile are computed and not stored.  Key
// tiles entirely above the tile's last row are not visited; a wave skips the tiles above ITS last row; the per-element mask
// runs only on the tiles the diagonal or lens[b] crosses.  Query tiles are issued last-first (the longest key ranges start first).
//
// Lane algebra (MFMA 16x16x32; both operands share one register layout: index = lane & 15, reduction slots = (lane >> 4) * 8 + j;
// D[row = (lane >> 4) * 4 + r][col = lane & 15]):
//   S^T tile = mfma(first = K rows, second = Q rows): a lane holds 4 keys x ONE query (lane & 15), so row max / sum are in-lane plus
//   two xor-shuffles and m, l, alpha are lane-local.  The S^T accumulators ARE the second operand of the next MFMA (slots j < 4 <- key
//   tile 2s, j >= 4 <- tile 2s + 1): O^T = mfma(first = V^T rows (d), second = P).  V^T is never materialised: the row-major V tile in
//   LDS is read with ds_read_b64_tr_b16, addresses chosen so that a lane ends with 16 contiguous features of one query row.
// Q fragments are read once from global memory into registers.  K / V tiles go global -> registers -> LDS, double-buffered: the
// next tile's loads are issued before a tile's MFMAs and written to LDS after them, one barrier per tile.
#include "common.h"

#define EXT_NW 4
#define EXT_NTHR (EXT_NW * 64)
#define EXT_QB (EXT_NW * 32)
#define EXT_KT 64

typedef __attribute__((ext_vector_type(4))) short ext_s16x4;
template <bool V> struct ExtTag { static constexpr bool value = V; };

// ---- LDS tile image: [64 keys][HD bf16], 16-byte chunks XOR-swizzled per row.
//  K tiles (ds_read_b128 operand reads, rows = lane & 15): chunk ^= row & (HD / 8 - 1)
//  V tiles (tr reads only, hd 128): chunk ^= (row & 1) | ((row >> 1) & 1) << 3, the two 8-byte halves of a chunk swapped when
//  (row >> 2) & 1; hd 64: chunk ^= row & 7.
template <int HD, bool TR>
__device__ __forceinline__ int ext_swz_key(int row) {
  if constexpr (HD == 128 && TR) return (row & 1) | (((row >> 1) & 1) << 3);
  else return row & (HD / 8 - 1);
}
template <int HD, bool TR>
__device__ __forceinline__ int ext_swz_half(int row) {
  if constexpr (HD == 128 && TR) return (row >> 2) & 1;
  else return 0;
}

// One MFMA operand: 8 bf16 of key row `row`, logical 16-byte chunk `chunk`.
template <int HD>
__device__ __forceinline__ bf16x8 ext_read_rows(const char* tile, int row, int chunk) {
  return *(const bf16x8*)(tile + row * (HD * 2) + ((chunk ^ ext_swz_key<HD, false>(row)) << 4));
}

// Transposed operand from the row-major V tile: within each 16-lane group, lanes 4r .. 4r + 3 fetch 4 contiguous bf16 of "row r"
// from their own address and lane i receives column i.  Rows r are pointed at keys 32 st + 4 g + r (second read: + 16), the slot
// order of the S^T accumulators; the 4 lanes of a row at features c4 * 16 + dt * 4 + (0..3) of a 64-wide strip.
template <int HD>
__device__ __forceinline__ bf16x8 ext_read_tr(const char* tile, int dtile, int st, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int tok = st * 32 + g * 4 + (i >> 2);
  const int chunk = (dtile >> 2) * 8 + (i & 3) * 2 + ((dtile & 3) >> 1);
  const char* p = tile + tok * (HD * 2) + ((chunk ^ ext_swz_key<HD, true>(tok)) << 4) + (((dtile & 1) ^ ext_swz_half<HD, true>(tok)) << 3);
  const ext_s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ext_s16x4*)p);
  // key + 16 has the same swizzle key / half as key (they only look at row bits 0..3)
  const ext_s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ext_s16x4*)(p + 16 * HD * 2));
  return (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// [64 x HD] cache tile through registers.  Rows >= rows_valid are zero and their address is never formed.
template <int HD, bool TR>
struct ExtStage {
  static constexpr int NC = HD / 8, NL = EXT_KT * NC / EXT_NTHR;
  static_assert(NL >= 1 && NL * EXT_NTHR == EXT_KT * NC, "tile does not divide over the workgroup");
  u32x4 vr[NL];
  __device__ __forceinline__ void load(const bf16_t* base, int ld, int rows_valid, int tid) {
#pragma unroll
    for (int a = 0; a < NL; ++a) {
      const int id = tid + a * EXT_NTHR, row = id / NC, ch = id % NC;
      if (row < rows_valid) vr[a] = *(const u32x4*)(base + (long long)row * ld + ch * 8);
      else vr[a] = (u32x4){0u, 0u, 0u, 0u};
    }
  }
  __device__ __forceinline__ void write(char* tile, int tid) const {
#pragma unroll
    for (int a = 0; a < NL; ++a) {
      const int id = tid + a * EXT_NTHR, row = id / NC, ch = id % NC;
      u32x4 v = vr[a];
      if (ext_swz_half<HD, TR>(row)) v = (u32x4){v[2], v[3], v[0], v[1]};
      *(u32x4*)(tile + row * (HD * 2) + ((ch ^ ext_swz_key<HD, TR>(row)) << 4)) = v;
    }
  }
};

__device__ __forceinline__ bf16x8 ext_pack(const f32x4& lo, const f32x4& hi) {
  u32x4 r = {pack2bf(lo[0], lo[1]), pack2bf(lo[2], lo[3]), pack2bf(hi[0], hi[1]), pack2bf(hi[2], hi[3])};
  return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ float ext_xmax16(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); return fmaxf(v, __shfl_xor(v, 32, 64)); }
__device__ __forceinline__ float ext_xsum16(float v) { v += __shfl_xor(v, 16, 64); return v + __shfl_xor(v, 32, 64); }

template <int HD>
__global__ __launch_bounds__(EXT_NTHR) void attn_extend_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                                               const bf16_t* __restrict__ vc, const int* __restrict__ lens,
                                                               const int* __restrict__ cu, bf16_t* __restrict__ out, int T, int group,
                                                               int smax, int ldq, int ldc, int ldo, float scale) {
  constexpr int KS = HD / 32, DT = HD / 16;
  constexpr int TB = EXT_KT * HD * 2;                    // tile bytes; LDS layout: K[2], V[2]
  __shared__ __attribute__((aligned(16))) char smem[4 * TB];
  const int qb = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int n = max(0, min(cu ? cu[b + 1] - cu[b] : T, T));
  const int q0 = qb * EXT_QB;
  if (q0 >= n) return;                                   // before any barrier
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hk = h / group;
  const long long row0 = cu ? (long long)cu[b] : (long long)b * T;
  const int len = max(0, min(lens[b], smax));
  const int hist = len - n;                              // query t sees keys k <= hist + t; negative: the first rows see nothing
  const int qw0 = q0 + wave * 32;
  const float c = scale * 1.4426950408889634f;

  bf16x8 qf[2][KS];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int t = qw0 + qt * 16 + li;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (t < n) qf[qt][ks] = *(const bf16x8*)(q + (row0 + t) * ldq + h * HD + ks * 32 + g * 8);
      else qf[qt][ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  f32x4 o[2][DT];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int d = 0; d < DT; ++d) o[qt][d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float mrun[2] = {-INFINITY, -INFINITY}, lrun[2] = {0.f, 0.f};

  const bf16_t* Kb = kc + (long long)b * smax * ldc + hk * HD;
  const bf16_t* Vb = vc + (long long)b * smax * ldc + hk * HD;
  const int kv_end = min(len, hist + min(q0 + EXT_QB, n));          // one past the last key any stored row of this tile sees
  const int ntiles = kv_end > 0 ? (kv_end + EXT_KT - 1) / EXT_KT : 0;

  ExtStage<HD, false> kst;
  ExtStage<HD, true> vst;
  auto prefetch = [&](int j) {                                      // rows >= len stay zero and unaddressed
    kst.load(Kb + (long long)j * EXT_KT * ldc, ldc, len - j * EXT_KT, tid);
    vst.load(Vb + (long long)j * EXT_KT * ldc, ldc, len - j * EXT_KT, tid);
  };
  auto commit = [&](int j) {
    kst.write(smem + (j & 1) * TB, tid);
    vst.write(smem + 2 * TB + (j & 1) * TB, tid);
  };
  if (ntiles > 0) { prefetch(0); commit(0); }
  __syncthreads();

  for (int j = 0; j < ntiles; ++j) {
    const int kv0 = j * EXT_KT;
    const char* sK = smem + (j & 1) * TB;
    const char* sV = smem + 2 * TB + (j & 1) * TB;
    const bool more = j + 1 < ntiles;
    if (more) prefetch(j + 1);
    if (kv0 <= hist + qw0 + 31) {                                   // wave-uniform: some key of the tile is visible to this wave
      const bool need_mask = (kv0 + EXT_KT > len) || (kv0 + EXT_KT - 1 > hist + qw0);
      f32x4 s[2][4];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) s[qt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 kf = ext_read_rows<HD>(sK, nt * 16 + li, ks * 4 + g);
          s[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][ks], s[0][nt], 0, 0, 0);
          s[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][ks], s[1][nt], 0, 0, 0);
          if (nt == 3) __builtin_amdgcn_sched_barrier(0);          // keep the compiler from hoisting every operand read of the tile
        }
      bf16x8 pf[2][2][3];                                           // [query tile][key half][term of p]
      auto softmax = [&](auto masked, const int qt) {
        constexpr bool MASKED = decltype(masked)::value;
        const int lim = hist + qw0 + qt * 16 + li;                  // last visible key of this lane's query
        float mx = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = s[qt][nt][r];
            if constexpr (MASKED) {
              const int key = kv0 + nt * 16 + g * 4 + r;
              if (key > lim || key >= len) v = -INFINITY;
              s[qt][nt][r] = v;
            }
            mx = fmaxf(mx, v);
          }
        mx = ext_xmax16(mx);
        const float mnew = fmaxf(mrun[qt], mx);
        const float msafe = (mnew == -INFINITY) ? 0.f : mnew;
        const float alpha = (mnew == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f((mrun[qt] - mnew) * c);
        const float nmc = -msafe * c;
        float rs = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(s[qt][nt][r], c, nmc));
            s[qt][nt][r] = pv;
            rs += pv;
          }
        rs = ext_xsum16(rs);
        lrun[qt] = lrun[qt] * alpha + rs;
        mrun[qt] = mnew;
        if (!__all(alpha == 1.f)) {
#pragma unroll
          for (int d = 0; d < DT; ++d) o[qt][d] *= alpha;
        }
        // p = hi + mid + lo, three bf16 terms that together hold the fp32 p exactly
#pragma unroll
        for (int term = 0; term < 3; ++term) {
          pf[qt][0][term] = ext_pack(s[qt][0], s[qt][1]);
          pf[qt][1][term] = ext_pack(s[qt][2], s[qt][3]);
          if (term < 2) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
              for (int r = 0; r < 4; ++r) s[qt][nt][r] -= bfround(s[qt][nt][r]);
          }
        }
      };
      if (need_mask) { softmax(ExtTag<true>{}, 0); softmax(ExtTag<true>{}, 1); }
      else { softmax(ExtTag<false>{}, 0); softmax(ExtTag<false>{}, 1); }
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const bf16x8 vf = ext_read_tr<HD>(sV, d, st, lane);
#pragma unroll
          for (int term = 2; term >= 0; --term) {                   // smallest term first
            o[0][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0][st][term], o[0][d], 0, 0, 0);
            o[1][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1][st][term], o[1][d], 0, 0, 0);
          }
          if ((d & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (more) commit(j + 1);
    __syncthreads();
  }

  // epilogue: lane (li, g) owns, per 64-wide strip sp, the 16 contiguous features g * 16 + dt * 4 + r of query row li
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int t = qw0 + qt * 16 + li;
    if (t >= n) continue;
    const float inv = lrun[qt] > 0.f ? 1.f / lrun[qt] : 0.f;
    bf16_t* dst = out + (row0 + t) * ldo + h * HD + g * 16;
#pragma unroll
    for (int sp = 0; sp < HD / 64; ++sp) {
      u32x4 w0, w1;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        w0[k * 2] = pack2bf(o[qt][sp * 4 + k][0] * inv, o[qt][sp * 4 + k][1] * inv);
        w0[k * 2 + 1] = pack2bf(o[qt][sp * 4 + k][2] * inv, o[qt][sp * 4 + k][3] * inv);
        w1[k * 2] = pack2bf(o[qt][sp * 4 + 2 + k][0] * inv, o[qt][sp * 4 + 2 + k][1] * inv);
        w1[k * 2 + 1] = pack2bf(o[qt][sp * 4 + 2 + k][2] * inv, o[qt][sp * 4 + 2 + k][3] * inv);
      }
      *(u32x4*)(dst + sp * 64) = w0;
      *(u32x4*)(dst + sp * 64 + 8) = w1;
    }
  }
}

extern "C" int lmod_attn_extend(const void* q, const void* kcache, const void* vcache, const int* lens, const int* cu_new, void* out,
                                int B, int T, int nh, int nkv, int hd, int smax, int ldq, int ld_cache, int ldo, float scale,
                                hipStream_t stream) {
  if (B < 0 || T < 1 || nh <= 0 || nkv <= 0 || nh % nkv || smax <= 0) return LMOD_EINVAL;
  if (B == 0) return LMOD_OK;
  if (!q || !kcache || !vcache || !lens || !out) return LMOD_EINVAL;
  if (hd != 64 && hd != 128) return LMOD_EUNSUPPORTED;
  if (T > 65535 || B > 65535 || nh > 65535) return LMOD_EUNSUPPORTED;
  // every row is moved in 16-byte pieces: leading dimensions in multiples of 8 elements, 16-byte aligned bases
  if ((ld_cache & 7) || ld_cache < nkv * hd || (ldq & 7) || ldq < nh * hd || (ldo & 7) || ldo < nh * hd || ((uintptr_t)q & 15) ||
      ((uintptr_t)kcache & 15) || ((uintptr_t)vcache & 15) || ((uintptr_t)out & 15))
    return LMOD_EINVAL;
  const dim3 grid((T + EXT_QB - 1) / EXT_QB, nh, B);
  if (hd == 128)
    hipLaunchKernelGGL(attn_extend_kernel<128>, grid, dim3(EXT_NTHR), 0, stream, (const bf16_t*)q, (const bf16_t*)kcache,
                       (const bf16_t*)vcache, lens, cu_new, (bf16_t*)out, T, nh / nkv, smax, ldq, ld_cache, ldo, scale);
  else
    hipLaunchKernelGGL(attn_extend_kernel<64>, grid, dim3(EXT_NTHR), 0, stream, (const bf16_t*)q, (const bf16_t*)kcache,
                       (const bf16_t*)vcache, lens, cu_new, (bf16_t*)out, T, nh / nkv, smax, ldq, ld_cache, ldo, scale);
  return lmod_launch_status();
}
