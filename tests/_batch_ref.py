"""Restatements of the continuous-batching kernels (csrc/batch.hip) for the tests: Philox4x32-10 in numpy with the per-request
uniform map of lmod_request_uniform, and lmod_kv_admit_rows / lmod_slot_admit in plain torch."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # Weyl key increments
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter uint32 [..., 4], key uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]: ten Philox4x32 rounds
    (Salmon et al., SC'11)."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                              # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def request_uniform(seed, req_id, n_gen):
    """u fp32 [N] = (word 0 >> 8) * 2^-24 of Philox4x32-10 at counter (req_id, n_gen, 0, 0) under the key (seed low, seed high)."""
    req = np.asarray(req_id, dtype=np.int64) & MASK            # an int32 id enters the counter as its 32-bit pattern
    gen = np.asarray(n_gen, dtype=np.int64) & MASK
    ctr = np.stack([req, gen, np.zeros_like(req), np.zeros_like(req)], -1).astype(np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.array([seed & MASK, seed >> 32], dtype=np.uint32)
    w = philox4x32_10(ctr, key)[..., 0]
    return ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def kv_admit_rows(dst, src, dst_row, lens):
    """New dst tensors with dst[t][dst_row[r], :lens[r]] = src[t][r, :lens[r]]; nothing else changes."""
    out = [d.clone() for d in dst]
    for d, s in zip(out, src):
        for r, row in enumerate(dst_row):
            n = int(lens[r])
            d[int(row), :n] = s[r, :n]
    return out


def slot_admit(dst_row, prompt_ids, n_prompt_new, lens_new, req_new, hist, n_prompt, n_hist, n_gen, done, cache_lens, req_id):
    """New (hist, n_prompt, n_hist, n_gen, done, cache_lens, req_id) after admitting request r into slot dst_row[r]."""
    hist, n_prompt, n_hist, n_gen, done, cache_lens, req_id = (t.clone() for t in (hist, n_prompt, n_hist, n_gen, done, cache_lens,
                                                                                   req_id))
    for r, s in enumerate(dst_row):
        s, n = int(s), int(n_prompt_new[r])
        hist[s, :n] = prompt_ids[r, :n]
        n_prompt[s] = n_hist[s] = n
        n_gen[s] = done[s] = 0
        cache_lens[s], req_id[s] = lens_new[r], req_new[r]
    return hist, n_prompt, n_hist, n_gen, done, cache_lens, req_id
