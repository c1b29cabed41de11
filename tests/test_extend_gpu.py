"""lmod_attn_extend (csrc/attn_extend.hip) against its fp64 statement, its agreement with lmod_attn_append, its argument envelope,
and the chunk path built on it: a 40-token continuation and a second turn that brings an image."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llava-mod_amd"))

import _append_ref as R  # noqa: E402
import _extend_ref as E  # noqa: E402
import _util as U  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16


def _run(case, T, nh, nkv, hd):
    from llavamod import kernels as K
    q, kc, vc, lens, cu, scale = case
    dev = lambda t: None if t is None else t.to(DEV)
    return K.attn_extend(dev(q), dev(kc), dev(vc), dev(lens), nh, nkv, hd, scale, T, cu_new=dev(cu))


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", list(E.CASES))
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("hd,nh,nkv", E.GEOMS)
def test_attn_extend_vs_fp64(hd, nh, nkv, kind, name):
    """Within LIMIT of the fp64 statement per element; elements of unit 0 exactly 0; two calls bit-identical; NaN behind lens (the
    `flush` case: smax = max(lens), the last sample ends flush with the allocation)."""
    case, (ref, unit) = E.case_and_ref(kind, name, hd, nh, nkv, poison=True)
    T = E.CASES[name]["T"]
    out = _run(case, T, nh, nkv, hd)
    again = _run(case, T, nh, nkv, hd)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))
    fig, idx, nonzero = E.err_units(out.float().cpu(), ref, unit)
    print(f"EXTEND-KERNEL {kind} hd {hd} nh {nh} nkv {nkv} case {name}: {fig:.3e} at {idx} (LIMIT {E.LIMIT:.3e})")
    assert nonzero == 0
    assert fig <= E.LIMIT, (kind, name, fig, idx)


def test_attn_extend_writes_nothing_for_an_empty_sample():
    """A sample with n_b = 0 owns no row: with it in the middle of the batch every row of the output still belongs to a neighbour and
    is checked above; here the rows of a batch whose ONLY live sample is the last one are compared with that sample alone."""
    from llavamod import kernels as K
    hd, nh, nkv = 64, 2, 2
    q, kc, vc, lens, cu, scale = R.make_append_case("diffuse", [40, 9, 70], [0, 0, 33], 33, nh, nkv, hd, seed=5, device=DEV, poison=True)
    out = K.attn_extend(q, kc, vc, lens, nh, nkv, hd, scale, 33, cu_new=cu)
    alone = K.attn_extend(q, kc[2:].contiguous(), vc[2:].contiguous(), lens[2:].contiguous(), nh, nkv, hd, scale, 33)
    assert out.shape[0] == 33 and torch.equal(out.view(torch.int16), alone.view(torch.int16))


@pytest.mark.parametrize("hd,nh,nkv,T", [(128, 28, 4, 16), (64, 14, 2, 9), (64, 2, 2, 1)])
def test_attn_extend_agrees_with_attn_append(hd, nh, nkv, T):
    """Where both kernels apply (T <= 16) they are interchangeable: on the same inputs each element differs by at most the sum of
    the two kernels' bounds (each: 1/2 ulp + its LIMIT x unit)."""
    from llavamod import kernels as K
    for kind in E.KINDS:
        ns = [T, max(1, T // 2), 0, T]
        lens = [700 + T, 64 + ns[1], 33, T]
        q, kc, vc, ln, cu, scale = R.make_append_case(kind, lens, ns, T, nh, nkv, hd, seed=7, poison=True)
        ref, unit = R.append_ref64(q, kc, vc, ln, cu, T, nh, nkv, hd, scale)
        d = lambda t: t.to(DEV)
        a = K.attn_append(d(q), d(kc), d(vc), d(ln), nh, nkv, hd, scale, T, cu_new=d(cu)).float().cpu().double()
        e = K.attn_extend(d(q), d(kc), d(vc), d(ln), nh, nkv, hd, scale, T, cu_new=d(cu)).float().cpu().double()
        bound = R.ulp_bf16(ref) + (R.LIMIT + E.LIMIT) * unit
        worst = float(((a - e).abs() - bound).max())
        print(f"EXTEND-VS-APPEND {kind} hd {hd} T {T}: max(|append - extend| - bound) = {worst:.3e}")
        assert bool(((a - e).abs() <= bound).all()), (kind, worst)


def test_attn_extend_envelope():
    from llavamod import kernels as K
    from llavamod import _hip
    hd, nh, nkv, T = 64, 4, 2, 20
    q, kc, vc, lens, cu, scale = R.make_append_case("diffuse", [50, 30], None, T, nh, nkv, hd, device=DEV)
    args = lambda **kw: {**dict(q=q, kc=kc, vc=vc, out=torch.empty_like(q), B=2, T=T, nh=nh, nkv=nkv, hd=hd, ldq=q.stride(0),
                                ldc=kc.stride(1), ldo=q.stride(0)), **kw}

    def rc(**kw):
        a = args(**kw)
        return _hip.call("lmod_attn_extend", a["q"].data_ptr(), a["kc"].data_ptr(), a["vc"].data_ptr(), lens.data_ptr(), None,
                         a["out"].data_ptr(), a["B"], a["T"], a["nh"], a["nkv"], a["hd"], kc.shape[1], a["ldq"], a["ldc"], a["ldo"],
                         float(scale), allow=(-1, -3))
    assert rc() == 0
    assert rc(hd=96) == -3                                     # LMOD_EUNSUPPORTED: head dim
    assert rc(T=65536) == -3                                   # beyond the grid
    assert rc(nh=3) == -1                                      # LMOD_EINVAL: nh % nkv
    assert rc(T=0) == -1
    assert rc(ldq=q.stride(0) + 4) == -1                       # leading dimensions: multiples of 8
    assert rc(ldo=q.stride(0) + 4) == -1
    assert rc(ldc=kc.stride(1) + 4) == -1
    assert rc(ldc=nkv * hd - 8) == -1                          # narrower than the heads
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        K.attn_extend(q[:-1], kc, vc, lens, nh, nkv, hd, scale, T)   # uniform rows must be B * T


# ------------------------------------------------------------------------------------------ the chunk path of the golden small models
def _helpers():
    from test_append_gpu import _pair, _prompt, ulp_bf16_of
    from test_step_parity_gpu import _bf16_batch, _bf16_twin, _oracle_pair_from, small_cfgs
    return _pair, _prompt, ulp_bf16_of, _bf16_batch, _bf16_twin, _oracle_pair_from, small_cfgs


def _concat(ids, mask, extra):
    B, n = extra.shape
    plen = mask.sum(1)
    ids = torch.cat([ids, torch.zeros(B, n, dtype=ids.dtype)], 1)
    mask = torch.cat([mask, torch.zeros(B, n, dtype=torch.bool)], 1)
    for b in range(B):
        ids[b, int(plen[b]):int(plen[b]) + n] = extra[b].cpu()
        mask[b, int(plen[b]):int(plen[b]) + n] = True
    return ids, mask


@pytest.mark.parametrize("which", ["teacher", "student"])
def test_long_chunk_vs_decode_steps_and_oracle(which):
    """test_chunk_forward_vs_decode_steps_and_oracle's three comparisons, same bounds, for ONE 40-token chunk through forward_extend:
    logits against the fp32 oracle over prompt + chunk (relerr <= max(2 x bf16-twin floor, 5e-3)), cache K against 40 decode steps
    within 1 bf16 ulp, greedy tokens equal to the decode path's up to the first sub-8-ulp top-2 gap (at least 6 steps).  With
    extend_min_tokens raised the same call returns the piece loop's bits."""
    _pair, _prompt, ulp_bf16_of, _bf16_batch, _bf16_twin, _oracle_pair_from, small_cfgs = _helpers()
    T = 40
    student, teacher = _pair()
    model = teacher if which == "teacher" else student
    vc, sc, tc = small_cfgs()
    if which == "student":
        for m in model.moe_layers():
            m.eval_capacity_factor = 64.0
        sc.eval_capacity_factor = 64.0
    model.eval()
    assert type(model).extend_min_tokens == 17
    pr = _prompt(which)
    B = pr["input_ids"].shape[0]
    toks = model.generate(**pr, max_new_tokens=T)
    cache_d, _ = model._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], T + 1)
    dec = torch.stack([model._decode_step(toks[:, i].to(torch.int32).contiguous(), cache_d).float() for i in range(T)], 1)
    # the extend path, with the launch observed
    from llavamod import _hip
    seen = []
    real = _hip.call
    cache_c, _ = model._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], T + 1)
    import llavamod.kernels as K
    K.call = lambda name, *a, **kw: (seen.append(name), real(name, *a, **kw))[1]
    try:
        chunk = model(input_ids=toks, past_key_values=cache_c).logits
        assert seen.count("lmod_attn_extend") == len(cache_c.k) and "lmod_attn_append" not in seen
        # the A/B arm: the piece loop, bit for bit what forward_append gives piece by piece
        del seen[:]
        cache_p, _ = model._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], T + 1)
        model.extend_min_tokens = 1 << 30
        pieces = model(input_ids=toks, past_key_values=cache_p).logits
        assert "lmod_attn_extend" not in seen and seen.count("lmod_attn_append") == 3 * len(cache_c.k)
    finally:
        K.call = real
        del model.extend_min_tokens
    cache_q, _ = model._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], T + 1)
    emb_w, manual = model.model.embed_tokens.weight, []
    from llavamod import ops
    for j0 in range(0, T, K.APPEND_T_MAX):
        Tp = min(K.APPEND_T_MAX, T - j0)
        tok = toks[:, j0:j0 + Tp].to(DEV).to(torch.int32).reshape(-1).contiguous()
        hid = model.model.forward_append(K.gather_rows(emb_w, None, tok, emb_w.shape[1]), cache_q, Tp)
        manual.append(ops.linear_fwd(hid, model.head()).float().view(B, Tp, -1))
    assert torch.equal(pieces, torch.cat(manual, 1))
    assert chunk.shape == dec.shape and chunk.dtype == torch.float32 and torch.equal(cache_c.lens, cache_d.lens)
    # the fp32 oracle over prompt + chunk, and its bf16 twin
    ssd, tsd = U.load_golden("gpusmall_student.safetensors"), U.load_golden("gpusmall_teacher.safetensors")
    o_student, o_teacher = _oracle_pair_from(ssd, tsd, sc, tc, vc)
    oracle = o_teacher if which == "teacher" else o_student
    oracle.eval()
    if which == "student":
        oracle.set_gate_noise([None])
    plen = pr["attention_mask"].sum(1)
    ids, mask = _concat(pr["input_ids"].clone(), pr["attention_mask"].clone(), toks)
    ob = dict(input_ids=ids, attention_mask=mask, images=pr["images"].float().cpu())
    with torch.no_grad():
        ref = oracle(**ob).logits.float()
        twin = _bf16_twin(oracle)(**_bf16_batch(ob)).logits.float()
    n_img = model.get_image_tower().num_patches - 1
    for b in range(B):
        p0 = int(plen[b]) + n_img
        r, tw = ref[b, p0:p0 + T], twin[b, p0:p0 + T]
        floor = U.relerr(tw, r)
        e_chunk, e_dec = U.relerr(chunk[b].cpu(), r), U.relerr(dec[b].cpu(), r)
        print(f"EXTEND-LOGITS {which} sample {b}: chunk {e_chunk:.3e} decode {e_dec:.3e} floor {floor:.3e}")
        assert e_chunk <= max(2.0 * floor, 5e-3), ("chunk", b, e_chunk, floor)
    for layer in range(len(cache_c.k)):
        for b in range(B):
            L = int(cache_c.lens[b])
            kc_, kd_ = cache_c.k[layer][b, :L].float(), cache_d.k[layer][b, :L].float()
            assert bool(((kc_ - kd_).abs() <= R.ulp_bf16(kd_.cpu()).to(DEV).float()).all()), (layer, b)
    top2 = dec.topk(2, -1).values
    for b in range(B):
        n_cmp = T
        for i in range(T):
            if float(top2[b, i, 0] - top2[b, i, 1]) < 8 * ulp_bf16_of(top2[b, i, 0]):
                n_cmp = i
                break
        assert n_cmp >= 6, (b, n_cmp)
        assert torch.equal(chunk[b, :n_cmp].argmax(-1), dec[b, :n_cmp].argmax(-1)), b


def test_second_turn_with_an_image():
    """Turn 1: the golden prompt, greedy, return_dict_in_generate.  Turn 2: [last turn-1 token, text, IMAGE_TOKEN_INDEX, text] and a
    second image per sample, passed with past_key_values (tests/golden/extend_turn2.json, tools/make_extend_fixture.py: token ids on
    which the fp32 oracle's continuation of the concatenated two-image prompt is tie-free).  The logits of the turn-2 rows follow the
    relerr rule against the oracle's single forward over the concatenation; the greedy tokens equal one generate() over the
    concatenation up to the first step whose top-2 gap is below 8 bf16 ulps (at least 6 steps)."""
    _pair, _prompt, ulp_bf16_of, _bf16_batch, _bf16_twin, _oracle_pair_from, small_cfgs = _helpers()
    fx = U.load_json("extend_turn2.json")
    _, teacher = _pair()
    teacher.eval()
    vc, sc, tc = small_cfgs()
    pr = _prompt()
    B = pr["input_ids"].shape[0]
    t1 = torch.tensor(fx["turn1_tokens"])
    T1, STEPS = t1.shape[1], len(fx["turn2_tokens"][0])
    first = teacher.generate(**pr, max_new_tokens=T1, return_dict_in_generate=True)
    assert torch.equal(first.sequences.cpu(), t1)                          # tie-free steps of the golden prompt
    text = torch.tensor(fx["turn2_text"])
    turn2 = torch.cat([t1[:, -1:], text], 1)                               # the cache holds every fed position: all but the last token
    img2 = torch.randn(B, 3, vc.image_size, vc.image_size, generator=torch.Generator().manual_seed(fx["image_seed"])).to(BF)
    # an image token in a chunk without its image still raises
    with pytest.raises(ValueError, match="image tokens"):
        teacher.generate(input_ids=turn2, past_key_values=first.past_key_values, max_new_tokens=1)
    # the concatenated two-image prompt: images sample-major, in the order the splice consumes them
    ids_cat, mask_cat = _concat(*_concat(pr["input_ids"].clone(), pr["attention_mask"].clone(), t1), text)
    images_cat = torch.stack([pr["images"].cpu(), img2], 1).reshape(2 * B, *img2.shape[1:])
    whole = teacher.generate(input_ids=ids_cat, attention_mask=mask_cat, images=images_cat.to(DEV), max_new_tokens=STEPS)
    # turn 2, logits of its rows (a copy of the cache: the forward appends to it)
    import copy
    cache_l = copy.copy(first.past_key_values)
    cache_l.k, cache_l.v = [t.clone() for t in cache_l.k], [t.clone() for t in cache_l.v]
    cache_l.lens, cache_l._alt = cache_l.lens.clone(), None
    lens_before = cache_l.lens.clone()
    n_img = teacher.get_image_tower().num_patches - 1
    S2 = turn2.shape[1] + n_img
    logits2 = teacher(input_ids=turn2, images=img2.to(DEV), past_key_values=cache_l).logits
    assert logits2.shape[:2] == (B, S2) and torch.equal(cache_l.lens, lens_before + S2)
    _, o_teacher = _oracle_pair_from(U.load_golden("gpusmall_student.safetensors"), U.load_golden("gpusmall_teacher.safetensors"), sc, tc, vc)
    o_teacher.eval()
    ob = dict(input_ids=ids_cat, attention_mask=mask_cat, images=images_cat.float())
    with torch.no_grad():
        ref = o_teacher(**ob).logits.float()
        twin = _bf16_twin(o_teacher)(**_bf16_batch(ob)).logits.float()
    for b in range(B):
        p0 = int(lens_before[b])                                           # turn 2 starts where the cache ended
        r, tw = ref[b, p0:p0 + S2], twin[b, p0:p0 + S2]
        floor, e = U.relerr(tw, r), U.relerr(logits2[b].cpu(), r)
        print(f"EXTEND-TURN2-LOGITS sample {b}: {e:.3e} floor {floor:.3e}")
        assert e <= max(2.0 * floor, 5e-3), (b, e, floor)
    # turn 2, greedy, against one generate() over the concatenation
    second = teacher.generate(input_ids=turn2, images=img2.to(DEV), past_key_values=first.past_key_values, max_new_tokens=STEPS)
    cache_w, lg = teacher._prefill(ids_cat, mask_cat, images_cat.to(DEV), STEPS + 1)
    rows = [lg.float()]
    for i in range(STEPS - 1):                                             # the one-prompt path's logits, step by step, for its top-2 gaps
        rows.append(teacher._decode_step(whole[:, i].to(DEV).to(torch.int32).contiguous(), cache_w).float())
    top2 = torch.stack(rows, 1).topk(2, -1).values
    for b in range(B):
        n_cmp = STEPS
        for i in range(STEPS):
            if float(top2[b, i, 0] - top2[b, i, 1]) < 8 * ulp_bf16_of(top2[b, i, 0]):
                n_cmp = i
                break
        assert n_cmp >= 6, (b, n_cmp)
        assert torch.equal(second[b, :n_cmp].cpu(), whole[b, :n_cmp].cpu()), (b, second[b], whole[b])
