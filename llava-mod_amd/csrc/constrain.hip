// Constrained decoding of generate() / generate_batch() on the device: a deterministic finite automaton over token ids says which
// tokens a row MAY emit (generation.TokenConstraint builds the tables, kernels.constraint_table copies them).
//
// Tables, all int32: edge_off [n_states + 1], edge_tok / edge_next [E] (CSR, tokens strictly ascending inside a state),
// default_next [n_states], flags [n_states] (bit 0 accept: EOS is allowed here; bit 1 terminal: a row that enters is finished).
// A state s is CLOSED when default_next[s] < 0 (only tokens with a listed edge whose next >= 0 are allowed) and OPEN otherwise
// (every token is allowed and an unlisted one leads to default_next[s]; a listed edge with next < 0 bans its token).
//
// lmod_constrain_mask_rows_bf16 edits one step's bf16 logits [R, V] in place, one workgroup per row, from the row's state:
//   state outside [0, n_states)  the row is not touched (-1 is "unconstrained"; the upper guard keeps a bad state out of the tables);
//   open state    every listed edge with next < 0 stores -inf at its token, and eos is banned unless the state accepts; no sweep;
//   closed state  a V-bit bitmap in LDS (the layout and the limit of logits.hip's penalty bitmap) collects the allowed tokens - the
//                 edges with next >= 0, and eos when the state accepts - then the row is swept: an element whose bit is clear becomes
//                 -inf.  A row whose address is 16-byte aligned is swept 8 elements at a time: a vector with no allowed element is
//                 stored without being read, one with some is read, patched and stored, one that is allowed as a whole is left alone;
//                 its last V % 8 elements, and every row that is not aligned (an odd row stride), go element by element.
// An allowed element keeps its bits (NaN, -inf and -0 included); tokens outside [0, V) are ignored.
//
// lmod_constrain_advance_rows is the per-step bookkeeping, one thread per row, after lmod_gen_push_stop: a live row in a valid
// state follows its token's edge (binary search; default_next when the token is not listed).  A token that leaves the automaton
// (next < 0: possible only when the row had no allowed token left) finishes the row and keeps its state; entering a terminal state
// finishes the row by that token, as a stop-sequence match does.
#include "common.h"

#define CONSTRAIN_THREADS 256
#define CONSTRAIN_LDS_MAX 65536                  // logits.hip's LOGITS_LDS_MAX: V <= 524288
#define BF16_NEG_INF ((bf16_t)0xff80u)
#define FLAG_ACCEPT 1
#define FLAG_TERMINAL 2

struct ConstrainTables {
  const int* edge_off; const int* edge_tok; const int* edge_next; const int* default_next; const int* flags;
  int n_states;
};

// Everything a branch around a barrier depends on (the row's state, its tables' entries, the row's address, has_bitmap) is uniform
// over the workgroup.
__global__ __launch_bounds__(CONSTRAIN_THREADS) void constrain_mask_rows_kernel(bf16_t* __restrict__ x, long long ld, int V,
                                                                                const int* __restrict__ state, ConstrainTables t,
                                                                                int eos, int has_bitmap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t allowed[];      // V bits: tokens the row may emit
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int s = state[r];
  if (s < 0 || s >= t.n_states) return;
  bf16_t* row = x + (long long)r * ld;
  const int e0 = t.edge_off[s], e1 = t.edge_off[s + 1];
  const bool accept = (t.flags[s] & FLAG_ACCEPT) != 0;
  const bool eos_inside = eos >= 0 && eos < V;
  if (t.default_next[s] >= 0) {                                          // open: the listed bans only
    for (int e = e0 + tid; e < e1; e += CONSTRAIN_THREADS) {
      const int tok = t.edge_tok[e];
      if (t.edge_next[e] < 0 && tok >= 0 && tok < V) row[tok] = BF16_NEG_INF;
    }
    if (tid == 0 && !accept && eos_inside) row[eos] = BF16_NEG_INF;
    return;
  }
  if (!has_bitmap) return;                                                // V over the bitmap: the caller refuses closed states
  const int words = (V + 31) >> 5;
  for (int i = tid; i < words; i += CONSTRAIN_THREADS) allowed[i] = 0u;
  __syncthreads();
  for (int e = e0 + tid; e < e1; e += CONSTRAIN_THREADS) {
    const int tok = t.edge_tok[e];
    if (t.edge_next[e] >= 0 && tok >= 0 && tok < V) atomicOr(&allowed[tok >> 5], 1u << (tok & 31));
  }
  if (tid == 0 && accept && eos_inside) atomicOr(&allowed[eos >> 5], 1u << (eos & 31));
  __syncthreads();
  int first = 0;                                                          // elements [0, first) are swept by vectors
  if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0) {
    const int nvec = V >> 3;
    uint4* rv = reinterpret_cast<uint4*>(row);
    const uint32_t ninf2 = 0xff80ff80u;
    for (int k = tid; k < nvec; k += CONSTRAIN_THREADS) {
      const int i = k << 3;                                               // 8 elements: one byte of the bitmap
      const uint32_t bits = (allowed[i >> 5] >> (i & 31)) & 0xffu;
      if (bits == 0xffu) continue;
      uint4 v = make_uint4(ninf2, ninf2, ninf2, ninf2);
      if (bits != 0u) {
        const uint4 old = rv[k];
        const uint32_t o[4] = {old.x, old.y, old.z, old.w};
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t lo = (bits >> (2 * j)) & 1u ? (o[j] & 0xffffu) : 0xff80u;
          const uint32_t hi = (bits >> (2 * j + 1)) & 1u ? (o[j] & 0xffff0000u) : 0xff800000u;
          w[j] = lo | hi;
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      rv[k] = v;
    }
    first = nvec << 3;
  }
  for (int i = first + tid; i < V; i += CONSTRAIN_THREADS)
    if (!((allowed[i >> 5] >> (i & 31)) & 1u)) row[i] = BF16_NEG_INF;
}

__global__ __launch_bounds__(CONSTRAIN_THREADS) void constrain_advance_rows_kernel(const int* __restrict__ tokens, int* __restrict__ done,
                                                                                   int* __restrict__ state, ConstrainTables t, int R) {
  const int r = blockIdx.x * CONSTRAIN_THREADS + threadIdx.x;
  if (r >= R) return;
  if (done[r]) return;                                                    // finished before, or by this step's push: the state stays
  const int s = state[r];
  if (s < 0 || s >= t.n_states) return;
  const int tok = tokens[r];
  int lo = t.edge_off[s], hi = t.edge_off[s + 1];                         // the first edge whose token is >= tok
  const int end = hi;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (t.edge_tok[mid] < tok) lo = mid + 1; else hi = mid;
  }
  const int ns = (lo < end && t.edge_tok[lo] == tok) ? t.edge_next[lo] : t.default_next[s];
  if (ns < 0 || ns >= t.n_states) { done[r] = 1; return; }                // the token left the automaton
  state[r] = ns;
  if (t.flags[ns] & FLAG_TERMINAL) done[r] = 1;
}

extern "C" {

int lmod_constrain_mask_rows_bf16(void* logits, long long ld, int V, int R, const int* state, const int* edge_off, const int* edge_tok,
                                  const int* edge_next, const int* default_next, const int* flags, int n_states, int eos,
                                  hipStream_t stream) {
  if (R < 0 || V < 1 || ld < V || n_states < 1) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!logits || !state || !edge_off || !default_next || !flags) return LMOD_EINVAL;   // edge_tok / edge_next: null when E == 0
  ConstrainTables t = {edge_off, edge_tok, edge_next, default_next, flags, n_states};
  const long long lds = 4LL * ((V + 31) >> 5);
  const int has_bitmap = lds <= CONSTRAIN_LDS_MAX;
  hipLaunchKernelGGL(constrain_mask_rows_kernel, dim3(R), dim3(CONSTRAIN_THREADS), (size_t)(has_bitmap ? lds : 0), stream,
                     (bf16_t*)logits, ld, V, state, t, eos, has_bitmap);
  return lmod_launch_status();
}

int lmod_constrain_advance_rows(const int* tokens, int* done, int* state, const int* edge_off, const int* edge_tok, const int* edge_next,
                                const int* default_next, const int* flags, int n_states, int R, hipStream_t stream) {
  if (R < 0 || n_states < 1) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!tokens || !done || !state || !edge_off || !default_next || !flags) return LMOD_EINVAL;
  ConstrainTables t = {edge_off, edge_tok, edge_next, default_next, flags, n_states};
  hipLaunchKernelGGL(constrain_advance_rows_kernel, dim3((R + CONSTRAIN_THREADS - 1) / CONSTRAIN_THREADS), dim3(CONSTRAIN_THREADS), 0,
                     stream, tokens, done, state, t, R);
  return lmod_launch_status();
}

}  // extern "C"
