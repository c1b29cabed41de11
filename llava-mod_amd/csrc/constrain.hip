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
//
// generate(constraint=, constraint_draft_tokens=k) drafts what the automaton FORCES.  A state is FORCED when it is closed, not
// terminal, and the set the mask would allow in it is one listed edge (t, ns) with t != eos: exactly one edge with next >= 0 and
// 0 <= tok < V, and no eos beside it (the state does not accept, or eos is outside [0, V)).  The masked distribution is then a point
// mass at t, so a run of forced states is a draft that needs no drafter.  Both kernels below: one thread per row, int32 and exact, no
// atomics, no workspace, every index checked and none clamped.
//   lmod_constrain_draft   walks the forced run from the row's state (at most k tokens; a linear scan of the state's edges that
//                          leaves at the second allowed one) and writes the draft, the verification chunk and the state that
//                          masks each verification row;
//   lmod_constrain_accept  lmod_spec_accept's rule and block with the automaton, EOS and the token budget applied to every emitted
//                          token on the device: the row's state, done flag, counter and cache length come out as plain
//                          constrained greedy would leave them.
#include "common.h"

#define CONSTRAIN_THREADS 256
#define CONSTRAIN_LDS_MAX 65536                  // logits.hip's LOGITS_LDS_MAX: V <= 524288
#define CONSTRAIN_T_MAX 16                       // APPEND_T_MAX of csrc/append.hip: the verification chunk holds k + 1 <= 16 tokens
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

// The single allowed edge of state s, when s is forced: true, and (*tok, *ns) is the edge.  s must be inside [0, n_states).
__device__ __forceinline__ bool constrain_forced(const ConstrainTables& t, int s, int eos, int V, int* tok, int* ns) {
  const int fl = t.flags[s];
  if (t.default_next[s] >= 0 || (fl & FLAG_TERMINAL)) return false;      // open, or nothing left to emit
  if ((fl & FLAG_ACCEPT) && eos >= 0 && eos < V) return false;           // eos is allowed beside whatever the edges allow
  int n = 0, ft = -1, fn = -1;
  for (int e = t.edge_off[s], e1 = t.edge_off[s + 1]; e < e1; ++e) {
    const int nx = t.edge_next[e], tk = t.edge_tok[e];
    if (nx < 0 || tk < 0 || tk >= V) continue;
    if (++n > 1) return false;
    ft = tk; fn = nx;
  }
  if (n != 1 || ft == eos || fn >= t.n_states) return false;
  *tok = ft; *ns = fn;
  return true;
}

__global__ __launch_bounds__(CONSTRAIN_THREADS) void constrain_draft_kernel(const int* __restrict__ pending, const int* __restrict__ state,
                                                                            const int* __restrict__ done, ConstrainTables t, int eos,
                                                                            int V, int k, int* __restrict__ draft, int* __restrict__ chunk,
                                                                            int* __restrict__ vstate, int* __restrict__ n_draft, int R) {
  const int r = blockIdx.x * CONSTRAIN_THREADS + threadIdx.x;
  if (r >= R) return;
  int* dr = draft + (long long)r * k;
  int* ch = chunk + (long long)r * (k + 1);
  int* vs = vstate + (long long)r * (k + 1);
  const int pend = pending[r];
  int s = state[r];
  const bool live = done[r] == 0 && s >= 0 && s < t.n_states;
  ch[0] = pend;
  int nd = 0;
  if (live) {
    int tok, ns;
    while (nd < k && constrain_forced(t, s, eos, V, &tok, &ns)) {
      vs[nd] = s;
      dr[nd] = tok;
      ch[nd + 1] = tok;
      s = ns;
      ++nd;
    }
    vs[nd] = (t.flags[s] & FLAG_TERMINAL) ? -1 : s;                       // the row behind the run: masked by where the run ended
  }
  for (int j = nd; j < k; ++j) { dr[j] = -1; ch[j + 1] = pend; }
  for (int j = live ? nd + 1 : 0; j <= k; ++j) vs[j] = -1;
  n_draft[r] = nd;
}

__global__ __launch_bounds__(CONSTRAIN_THREADS) void constrain_accept_kernel(const int* __restrict__ draft, const int* __restrict__ target,
                                                                             int k, int* __restrict__ done, int* __restrict__ state,
                                                                             ConstrainTables t, int eos, int pad, int* __restrict__ n_gen,
                                                                             int budget, int* __restrict__ lens_target,
                                                                             int* __restrict__ out, int* __restrict__ next_token, int R) {
  const int r = blockIdx.x * CONSTRAIN_THREADS + threadIdx.x;
  if (r >= R) return;
  const int* dr = draft + (long long)r * k;
  const int* tg = target + (long long)r * (k + 1);
  int* o = out + (long long)r * (k + 5);
  const int len0 = lens_target[r] - (k + 1);                              // the cache before the verification pass
  int n_acc = 0, n_emit = 0, fin = 1, last = pad;
  if (done[r] == 0) {
    while (n_acc < k && dr[n_acc] == tg[n_acc]) ++n_acc;
    int s = state[r], ng = n_gen[r];
    const bool inside = s >= 0 && s < t.n_states;                         // outside: an unconstrained row, eos and the budget only
    fin = 0;
    while (!fin && n_emit <= n_acc) {
      const int tok = n_emit < n_acc ? dr[n_emit] : tg[n_acc];
      o[n_emit++] = tok;
      last = tok;
      ++ng;
      if (eos >= 0 && tok == eos) { fin = 1; break; }                     // the state stays, as after lmod_gen_push_stop's EOS
      if (inside) {
        int lo = t.edge_off[s], hi = t.edge_off[s + 1];                   // the first edge whose token is >= tok
        const int end = hi;
        while (lo < hi) {
          const int mid = lo + ((hi - lo) >> 1);
          if (t.edge_tok[mid] < tok) lo = mid + 1; else hi = mid;
        }
        const int ns = (lo < end && t.edge_tok[lo] == tok) ? t.edge_next[lo] : t.default_next[s];
        if (ns < 0 || ns >= t.n_states) { fin = 1; break; }               // the token left the automaton: the state stays
        s = ns;
        if (t.flags[ns] & FLAG_TERMINAL) fin = 1;
      }
      if (ng >= budget) fin = 1;
    }
    state[r] = s;
    n_gen[r] = ng;
  }
  for (int i = n_emit; i <= k; ++i) o[i] = pad;
  const int nxt = fin ? pad : last;
  o[k + 1] = n_acc; o[k + 2] = n_emit; o[k + 3] = nxt; o[k + 4] = fin;
  next_token[r] = nxt;
  done[r] = fin;
  lens_target[r] = len0 + n_emit;
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

int lmod_constrain_draft(const int* pending, const int* state, const int* done, const int* edge_off, const int* edge_tok,
                         const int* edge_next, const int* default_next, const int* flags, int n_states, int eos, int V, int k, int* draft,
                         int* chunk, int* vstate, int* n_draft, int R, hipStream_t stream) {
  if (R < 0 || n_states < 1 || V < 1 || k < 1 || k >= CONSTRAIN_T_MAX) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!pending || !state || !done || !edge_off || !default_next || !flags || !draft || !chunk || !vstate || !n_draft) return LMOD_EINVAL;
  ConstrainTables t = {edge_off, edge_tok, edge_next, default_next, flags, n_states};
  hipLaunchKernelGGL(constrain_draft_kernel, dim3((R + CONSTRAIN_THREADS - 1) / CONSTRAIN_THREADS), dim3(CONSTRAIN_THREADS), 0, stream,
                     pending, state, done, t, eos, V, k, draft, chunk, vstate, n_draft, R);
  return lmod_launch_status();
}

int lmod_constrain_accept(const int* draft, const int* target, int k, int* done, int* state, const int* edge_off, const int* edge_tok,
                          const int* edge_next, const int* default_next, const int* flags, int n_states, int eos, int pad, int* n_gen,
                          int budget, int* lens_target, int* out, int* next_token, int R, hipStream_t stream) {
  if (R < 0 || n_states < 1 || k < 1 || k >= CONSTRAIN_T_MAX) return LMOD_EINVAL;
  if (R == 0) return LMOD_OK;
  if (!draft || !target || !done || !state || !edge_off || !default_next || !flags || !n_gen || !lens_target || !out || !next_token)
    return LMOD_EINVAL;
  ConstrainTables t = {edge_off, edge_tok, edge_next, default_next, flags, n_states};
  hipLaunchKernelGGL(constrain_accept_kernel, dim3((R + CONSTRAIN_THREADS - 1) / CONSTRAIN_THREADS), dim3(CONSTRAIN_THREADS), 0, stream,
                     draft, target, k, done, state, t, eos, pad, n_gen, budget, lens_target, out, next_token, R);
  return lmod_launch_status();
}

}  // extern "C"
