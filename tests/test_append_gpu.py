"""Multi-token KV-cache extension on the GPU: lmod_attn_append against the fp64 reference within the limit tests/_append_ref.py derives
on the CPU, lmod_kv_append_rows against an indexed copy, and the chunk forward of the golden small models against T sequential decode
steps and the fp32 oracle."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _append_ref as R  # noqa: E402
import _util as U  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


def _run(case, T, nh, nkv, hd, nsplit):
    from llavamod import kernels as K
    q, kc, vc, lens, cu, scale = case
    return K.attn_append(q.to(DEV), kc.to(DEV), vc.to(DEV), lens.to(DEV), nh, nkv, hd, scale, T,
                         cu_new=None if cu is None else cu.to(DEV), nsplit=nsplit)


def _check(case, T, nh, nkv, hd, nsplit, what):
    q, kc, vc, lens, cu, scale = case
    out = _run(case, T, nh, nkv, hd, nsplit)
    again = _run(case, T, nh, nkv, hd, nsplit)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), f"{what}: two calls differ"       # deterministic merge
    clean_k, clean_v = torch.nan_to_num(kc.float()).to(BF), torch.nan_to_num(vc.float()).to(BF)
    ref, unit = R.append_ref64(q, clean_k, clean_v, lens, cu, T, nh, nkv, hd, scale)
    fig, idx, nz = R.err_units(out.cpu(), ref, unit)
    print(f"APPEND-GPU {what} nsplit {nsplit}: {fig:.3e} at {idx} (L = {R.LIMIT:.3e})")
    assert nz == 0, f"{what}: {nz} elements with unit 0 are not exactly 0"
    assert fig <= R.LIMIT, (what, nsplit, fig, idx)


# cache lengths of the issue: n_b (empty history), 1 + n_b, 255, 256, 257, 700, 2049 + n_b — as samples of one batch
def _lens(T):
    return [T, 1 + T, 255, 256, 257, 700, 2049 + T]


@pytest.mark.parametrize("hd,nh,nkv", [(128, 28, 4), (64, 14, 2), (128, 8, 2), (64, 8, 2), (128, 4, 4), (64, 2, 2)],
                         ids=["hd128-g7", "hd64-g7", "hd128-g4", "hd64-g4", "hd128-g1", "hd64-g1"])
@pytest.mark.parametrize("T", [1, 2, 5, R.T_MAX])
def test_attn_append_vs_fp64(hd, nh, nkv, T):
    from llavamod import kernels as K
    lens = _lens(T)
    auto = K.attn_append_nsplit(len(lens), nkv, max(lens) + 3)
    for kind in ("diffuse", "hot", "spike"):
        case = R.make_append_case(kind, lens, None, T, nh, nkv, hd, poison=True)
        for nsplit in sorted({1, 2, auto}):
            _check(case, T, nh, nkv, hd, nsplit, f"{kind} hd{hd} g{nh // nkv} T{T}")


@pytest.mark.parametrize("hd,nh,nkv", [(128, 28, 4), (64, 14, 2)])
def test_attn_append_ragged_every_split_count(hd, nh, nkv):
    """Ragged cu_new (1 <= n_b <= T) and every key-split count the launcher accepts, NaN behind lens."""
    T = 5
    ns = [5, 1, 3, 2, 4, 5, 1]
    lens = [5, 2, 255, 256, 257, 700, 2049 + 1]
    case = R.make_append_case("hot", lens, ns, T, nh, nkv, hd, poison=True)
    for nsplit in range(1, 33):
        _check(case, T, nh, nkv, hd, nsplit, f"ragged hd{hd}")


@pytest.mark.parametrize("hd,nh,nkv", [(128, 8, 2), (64, 2, 2)])
def test_attn_append_rows_without_a_visible_key_are_zero(hd, nh, nkv):
    """lens[b] < n_b and lens[b] = 0: query t sees k <= lens - n + t < 0 for the first rows — their unit is 0 and they must be exactly 0,
    with NaN in every position behind lens (for lens 0: the whole cache row)."""
    T, lens = 5, [0, 2, 3, 70]
    for kind in ("diffuse", "hot"):
        case = R.make_append_case(kind, lens, None, T, nh, nkv, hd, poison=True)
        q, kc, vc, lt, cu, scale = case
        _, unit = R.append_ref64(q, torch.nan_to_num(kc.float()).to(BF), torch.nan_to_num(vc.float()).to(BF), lt, cu, T, nh, nkv, hd, scale)
        assert int((unit == 0).all(-1).sum()) == 5 + 3 + 2            # rows without a visible key: all of sample 0, 3 of sample 1, 2 of sample 2
        for nsplit in (1, 2, 3):
            _check(case, T, nh, nkv, hd, nsplit, f"unit-0 {kind} hd{hd}")


def test_attn_append_T1_is_the_decode_case():
    """T = 1 against lmod_attn_decode's fp64 reference and bound (tests/_attn_ref.py): the same contract, not the same bits."""
    import _attn_ref as A
    from llavamod import kernels as K
    B, smax, nh, nkv, hd = 3, 700, 8, 2, 128
    lens = [700, 233, 1]
    q, kc, vc, scale = A.make_decode_case("hot", B, smax, lens, nh, nkv, hd)
    lt = torch.tensor(lens, dtype=torch.int32)
    ref, unit = A.decode_ref64(q, kc, vc, lt, nh, nkv, hd, scale)
    for nsplit in (0, 1, 3):
        out = K.attn_append(q.to(DEV), kc.to(DEV), vc.to(DEV), lt.to(DEV), nh, nkv, hd, scale, 1, nsplit=nsplit)
        fig, idx, nz = A.err_units(out.cpu(), ref, unit)
        assert nz == 0 and fig <= A.LIMITS["O"], (nsplit, fig, idx)
    dec = K.attn_decode(q.to(DEV), kc.to(DEV), vc.to(DEV), lt.to(DEV), nh, nkv, hd, scale)
    assert A.err_units(dec.cpu(), ref, unit)[0] <= A.LIMITS["O"]


def test_attn_append_envelope():
    from llavamod import _hip
    lib = _hip.load()
    z = torch.zeros(64 * 17 * 128, device=DEV, dtype=BF)
    lens = torch.ones(1, device=DEV, dtype=torch.int32)
    f = lambda T, nh=4, nkv=4, hd=128, nsplit=1: lib.lmod_attn_append(  # noqa: E731
        z.data_ptr(), z.data_ptr(), z.data_ptr(), lens.data_ptr(), None, z.data_ptr(), 1, T, nh, nkv, hd, 1, nh * hd, nkv * hd, nh * hd,
        0.1, nsplit, None, 0, None)
    assert f(R.T_MAX) == 0 and f(R.T_MAX + 1) == -3 and f(0) == -1
    assert f(16, nh=36, nkv=4) == -3 and f(2, hd=96) == -3 and f(2, nsplit=2) == -1 and f(2, nsplit=33) == -3
    torch.cuda.synchronize()


def test_kv_append_rows_exact():
    from llavamod import _hip
    from llavamod import kernels as K
    B, T, smax, nh, nkv, hd = 4, 5, 40, 6, 2, 64
    g = torch.Generator().manual_seed(5)
    ns = [5, 1, 3, 2]
    cu = torch.tensor([0, 5, 6, 9, 11], dtype=torch.int32, device=DEV)
    lens_before = torch.tensor([0, 35, 17, 38], dtype=torch.int32, device=DEV)
    width = nkv * hd
    for cu_t, rows in ((cu, 11), (None, B * T)):
        qkv = torch.randn(rows, (nh + 2 * nkv) * hd, generator=g).to(BF).to(DEV)
        kc = torch.randn(B, smax, width, generator=g).to(BF).to(DEV)
        vc = torch.randn(B, smax, width, generator=g).to(BF).to(DEV)
        ek, ev = kc.clone(), vc.clone()
        lb = lens_before if cu_t is not None else torch.tensor([0, 35, 17, 30], dtype=torch.int32, device=DEV)
        for b in range(B):
            n = ns[b] if cu_t is not None else T
            r0 = int(cu[b]) if cu_t is not None else b * T
            p0 = int(lb[b])
            ek[b, p0:p0 + n] = qkv[r0:r0 + n, nh * hd:nh * hd + width]
            ev[b, p0:p0 + n] = qkv[r0:r0 + n, nh * hd + width:]
        K.kv_append_rows(qkv, nh * hd, nh * hd + width, width, kc, vc, lb, T, 40, cu_new=cu_t)
        assert torch.equal(kc.view(torch.int16), ek.view(torch.int16)) and torch.equal(vc.view(torch.int16), ev.view(torch.int16))
        with pytest.raises(RuntimeError, match="LMOD_EINVAL"):                      # a chunk that would run past smax
            K.kv_append_rows(qkv, nh * hd, nh * hd + width, width, kc, vc, lb, T, 41, cu_new=cu_t)
    assert _hip.load().lmod_kv_append_rows(None, 8, 0, 0, 8, None, None, None, None, 0, 1, 1, 8, 0, None) == 0


def test_spec_accept_kernel_vs_torch():
    from llavamod import kernels as K
    from llavamod.generation import spec_accept
    g = torch.Generator().manual_seed(9)
    for k in (1, 3, 15):
        B = 300
        target = torch.randint(4, 10, (B, k + 1), generator=g, dtype=torch.int32)
        draft = torch.where(torch.rand(B, k, generator=g) < 0.75, target[:, :k], torch.randint(4, 10, (B, k), generator=g, dtype=torch.int32))
        done = (torch.rand(B, generator=g) < 0.2).to(torch.int32)
        lt = torch.randint(k + 1, 50, (B,), generator=g, dtype=torch.int32)
        ld = torch.randint(k, 50, (B,), generator=g, dtype=torch.int32)
        for eos in (7, None):
            eb, en, ed, elt, eld = spec_accept(draft, target, done, eos, 3, lt, ld)
            d_dev, lt_dev, ld_dev = done.to(DEV), lt.to(DEV), ld.to(DEV)
            block, nxt = K.spec_accept(draft.to(DEV), target.to(DEV), d_dev, eos, 3, lt_dev, ld_dev)
            assert torch.equal(block.cpu().long(), eb) and torch.equal(nxt.cpu().long(), en)
            assert torch.equal(d_dev.cpu().bool(), ed) and torch.equal(lt_dev.cpu().long(), elt) and torch.equal(ld_dev.cpu().long(), eld)


# ------------------------------------------------------------------------------------------ chunk forward of the golden small models
def _pair():
    from test_generate_gpu import _pair as pair
    return pair()


def _prompt(which="teacher"):
    """tests/golden/append_prompt.safetensors (tools/make_append_fixture.py): ragged right-padded prompts with images on which the fp32
    oracle's greedy continuation keeps every top-2 gap above 8 bf16 ulps — 9 steps of the teacher, 8 steps of the student (its own
    prompt: the small student's logits are flatter)."""
    g = U.load_golden("append_prompt.safetensors")
    pre = "student_" if which == "student" else ""
    return dict(input_ids=g[pre + "input_ids"], attention_mask=g[pre + "attention_mask"].bool(),
                images=g[pre + "images"].to(DEV).to(torch.bfloat16))


def ulp_bf16_of(x):
    return float(R.ulp_bf16(torch.tensor(float(x))))


@pytest.mark.parametrize("which", ["teacher", "student"])
def test_chunk_forward_vs_decode_steps_and_oracle(which):
    """One chunk forward of T tokens against T sequential decode steps (golden small models; the MoE student with drop-free capacity, as
    the greedy test).  Both paths' logits are held to tests/test_step_parity_gpu.py's rule against the fp32 oracle's full forward over
    prompt + chunk: relerr <= max(2 x bf16-twin floor, 5e-3).  Caches over [0, lens): K within 1 bf16 ulp per element, V of layer 0
    exact (same GEMM, same rows).  Greedy tokens of the chunk rows equal the decode path's up to the first step whose top-2 logit gap
    (decode path) is below 8 bf16 ulps of the top logit; at least 6 steps per sample must be compared.
    Each model runs its own oracle-checked tie-free prompt (tests/golden/append_prompt.safetensors)."""
    from test_step_parity_gpu import _bf16_batch, _bf16_twin, _oracle_pair_from, small_cfgs
    T = 8
    student, teacher = _pair()
    model = teacher if which == "teacher" else student
    vc, sc, tc = small_cfgs()
    if which == "student":
        for m in model.moe_layers():
            m.eval_capacity_factor = 64.0
        sc.eval_capacity_factor = 64.0
    model.eval()
    pr = _prompt(which)
    B = pr["input_ids"].shape[0]
    toks = model.generate(**pr, max_new_tokens=T)                                   # g_0 .. g_{T-1}: the chunk
    # decode path: T steps
    cache_d, lg0 = model._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], T + 1)
    dec = []
    for i in range(T):
        dec.append(model._decode_step(toks[:, i].to(torch.int32).contiguous(), cache_d).float())
    dec = torch.stack(dec, 1)                                                       # [B, T, V]
    # chunk path
    cache_c, _ = model._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], T + 1)
    out = model(input_ids=toks, past_key_values=cache_c)
    chunk = out.logits
    assert chunk.shape == dec.shape and chunk.dtype == torch.float32 and out.past_key_values is cache_c
    assert torch.equal(cache_c.lens, cache_d.lens)
    # the fp32 oracle over prompt + chunk, and its bf16 twin
    ssd, tsd = U.load_golden("gpusmall_student.safetensors"), U.load_golden("gpusmall_teacher.safetensors")
    o_student, o_teacher = _oracle_pair_from(ssd, tsd, sc, tc, vc)
    oracle = o_teacher if which == "teacher" else o_student
    oracle.eval()
    if which == "student":
        oracle.set_gate_noise([None])
    ids, mask = pr["input_ids"].clone(), pr["attention_mask"].clone()
    plen = mask.sum(1)
    ids = torch.cat([ids, torch.zeros(B, T, dtype=ids.dtype)], 1)
    mask = torch.cat([mask, torch.zeros(B, T, dtype=torch.bool)], 1)
    for b in range(B):
        ids[b, int(plen[b]):int(plen[b]) + T] = toks[b].cpu()
        mask[b, int(plen[b]):int(plen[b]) + T] = True
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
        print(f"CHUNK-LOGITS {which} sample {b}: chunk {e_chunk:.3e} decode {e_dec:.3e} floor {floor:.3e}")
        assert e_dec <= max(2.0 * floor, 5e-3), ("decode", b, e_dec, floor)
        assert e_chunk <= max(2.0 * floor, 5e-3), ("chunk", b, e_chunk, floor)
    # caches
    for layer in range(len(cache_c.k)):
        for b in range(B):
            L = int(cache_c.lens[b])
            kc_, kd_ = cache_c.k[layer][b, :L].float(), cache_d.k[layer][b, :L].float()
            assert bool(((kc_ - kd_).abs() <= R.ulp_bf16(kd_.cpu()).to(DEV).float()).all()), (layer, b)
            if layer == 0:
                assert torch.equal(cache_c.v[0][b, :L], cache_d.v[0][b, :L]), b
    # greedy tokens, away from ties
    top2 = dec.topk(2, -1).values
    for b in range(B):
        n_cmp = T
        for i in range(T):
            if float(top2[b, i, 0] - top2[b, i, 1]) < 8 * ulp_bf16_of(top2[b, i, 0]):
                n_cmp = i
                break
        assert n_cmp >= 6, (b, n_cmp)
        assert torch.equal(chunk[b, :n_cmp].argmax(-1), dec[b, :n_cmp].argmax(-1)), b


def test_chunk_forward_contract():
    """forward(T > 1, past_key_values=...): [B, T, V] with zero rows on padded positions of a right-padded chunk mask; a left-padded
    chunk mask and an image token in a chunk raise; a chunk longer than one kernel call and a cache that is too small both work."""
    _, teacher = _pair()
    teacher.eval()
    pr = _prompt()
    B = pr["input_ids"].shape[0]
    cache, _ = teacher._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], 1)        # room for ONE more token: must grow
    g = torch.Generator().manual_seed(3)
    T = 21                                                                                     # > T_MAX: two pieces
    ids = torch.randint(0, 500, (B, T), generator=g)
    am = torch.ones(B, T, dtype=torch.bool)
    am[0, 18:] = False
    if B > 1:
        am[1, 3:] = False
    before = cache.lens.clone()
    out = teacher(input_ids=ids, attention_mask=am, past_key_values=cache)
    assert out.logits.shape == (B, T, teacher.lm_head.weight.shape[0])
    assert torch.equal(cache.lens.cpu(), before.cpu() + am.sum(1).to(torch.int32))
    assert float(out.logits[0, 18:].abs().max()) == 0.0 and float(out.logits[0, :18].abs().max()) > 0
    # the same tokens one at a time give the same argmax-free statement: logits of the last live row agree with a decode walk
    cache2, _ = teacher._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], T)
    last = None
    for i in range(18):
        last = teacher._decode_step(ids[:, i].to(DEV).to(torch.int32).contiguous(), cache2)
    assert U.relerr(out.logits[0, 17].cpu(), last[0].float().cpu()) <= 2e-2
    bad = torch.ones(B, T, dtype=torch.bool)
    bad[0, :2] = False
    with pytest.raises(ValueError, match="RIGHT-padded"):
        teacher(input_ids=ids, attention_mask=bad, past_key_values=cache)
    ids2 = ids.clone()
    ids2[0, 1] = -200
    with pytest.raises(ValueError, match="image tokens"):
        teacher(input_ids=ids2, past_key_values=cache)
