"""The tests of the attention tests (CPU): tests/_attn_ref.py's fp64 restatement against torch autograd, its units, the rounding model
that fixes the limits, and the seeded faults the bounds must catch.

Prints `ATTN-MODEL <output> <kind> <max err / unit>` (the measurement behind _attn_ref.MODEL_MAX / LIMITS) and
`ATTN-FAULT <fault> <worst output> <err / unit> <x limit> | old close() on diffuse input: <count> elements`."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_ref as R  # noqa: E402

# B, S, nh, nkv, hd, causal, lens
GEOMS = [
    (1, 512, 4, 4, 128, True, None),
    (1, 577, 2, 2, 64, False, None),
    (3, 320, 4, 1, 128, True, [300, 65, 320]),
    (2, 333, 14, 2, 64, True, [333, 200]),
    (2, 256, 2, 2, 128, False, [255, 33]),
    (1, 1024, 2, 1, 128, True, None),
    (3, 64, 2, 2, 64, True, [0, 1, 31]),
    (1, 1, 2, 1, 128, True, None),
]
KINDS = ["diffuse", "hot", "spike", "creep"]
OUTS = ("O", "dQ", "dK", "dV")


def _dense_autograd(q, k, v, do, scale, causal, lens):
    B, S, nh, hd = q.shape
    group = nh // k.shape[2]
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    kk, vv = kd.repeat_interleave(group, 2), vd.repeat_interleave(group, 2)
    s = torch.einsum("bqhd,bkhd->bhqk", qd, kk) * scale
    ar = torch.arange(S)
    ln = torch.tensor([S] * B if lens is None else lens)
    vis = (ar[None, None, :] < ln[:, None, None]).expand(B, S, S)
    if causal:
        vis = vis & (ar[None, None, :] <= ar[None, :, None])
    vis = vis[:, None]
    live = vis.any(-1, keepdim=True)
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(torch.where(live, s, torch.zeros_like(s)), -1) * live          # rows without a visible key: P = 0
    o = torch.einsum("bhqk,bkhd->bqhd", p, vv)
    lse = torch.logsumexp(s, -1)
    o.backward(do.double())
    return o.detach(), lse.detach(), qd.grad, kd.grad, vd.grad, vis.expand(B, nh, S, S)


@pytest.mark.parametrize("geom", GEOMS[:5] + GEOMS[6:], ids=str)
def test_ref64_equals_fp64_autograd_and_units_dominate(geom):
    B, S, nh, nkv, hd, causal, lens = geom
    q, k, v, do, scale = R.make_case("hot" if S > 1 else "diffuse", B, S, nh, nkv, hd, causal, lens, seed=3)
    ref = R.attn_ref64(q, k, v, do, scale, causal, lens, keep=True)
    o, lse, dq, dk, dv, vis = _dense_autograd(q, k, v, do, scale, causal, lens)
    for name, t in (("O", o), ("dQ", dq), ("dK", dk), ("dV", dv)):
        u = ref["u_" + name]
        assert ((ref[name] - t).abs() <= 1e-12 * (1 + u)).all(), name
        assert (u >= ref[name].abs() * (1 - 1e-12)).all(), f"unit of {name} below its value"
    dead = torch.isinf(lse)
    assert torch.equal(torch.isinf(ref["lse"]), dead) and (ref["lse"][dead] < 0).all()
    assert ((ref["lse"] - lse)[~dead].abs() <= 1e-12 * ref["u_lse"][~dead]).all()
    assert (ref["u_lse"][~dead] >= ref["lse"][~dead].abs()).all()
    # zero-unit elements are exactly the masked ones: query rows without a visible key (O, dQ), keys no query sees (dK, dV)
    row_dead = ~vis.any(-1)                                                  # [B, nh, S]
    key_dead = ~vis.any(-2)                                                  # [B, nh, S]
    group = nh // nkv
    assert torch.equal(ref["u_O"] == 0, row_dead.permute(0, 2, 1)[..., None].expand(B, S, nh, hd))
    assert torch.equal(ref["u_dQ"] == 0, row_dead.permute(0, 2, 1)[..., None].expand(B, S, nh, hd))
    kd = key_dead.reshape(B, nkv, group, S).all(2).permute(0, 2, 1)[..., None].expand(B, S, nkv, hd)
    assert torch.equal(ref["u_dV"] == 0, kd) and torch.equal(ref["u_dK"] == 0, kd)
    assert (ref["P"].sum(-1)[~row_dead] - 1).abs().max() < 1e-12 if (~row_dead).any() else True


def test_padded_query_rows_are_ordinary_rows_and_carry_gradient():
    """A dO that is zero except on padded query rows (q >= len) still produces dK / dV on the valid keys and dQ on the padded rows: the
    contract the kernels are held to (padded rows attend keys < len)."""
    B, S, nh, nkv, hd, lens = 2, 128, 2, 1, 64, [100, 33]
    q, k, v, do, scale = R.make_case("diffuse", B, S, nh, nkv, hd, True, lens, seed=1, do_kind="pad_only")
    ref = R.attn_ref64(q, k, v, do, scale, True, lens)
    for b, L in enumerate(lens):
        assert ref["dQ"][b, :L].abs().max() == 0 and ref["dQ"][b, L:].abs().min() > 0
        assert ref["dV"][b, :L].abs().min() > 0 and ref["dV"][b, L:].abs().max() == 0
        assert ref["O"][b, L:].abs().min() > 0


def _model_errs(geom, kind, do_kind="normal", hooks=None, seed=0):
    B, S, nh, nkv, hd, causal, lens = geom
    q, k, v, do, scale = R.make_case(kind, B, S, nh, nkv, hd, causal, lens, seed=seed, do_kind=do_kind)
    ref = R.attn_ref64(q, k, v, do, scale, causal, lens)
    mod = R.attn_model(q, k, v, do, scale, causal, lens, hooks)
    errs = {}
    for name in OUTS:
        e, idx, nz = R.err_units(mod[name], ref[name], ref["u_" + name])
        errs[name] = float("inf") if nz else e
    e, idx, nz = R.err_units_lse(mod["lse"], ref["lse"], ref["u_lse"])
    errs["lse"] = float("inf") if nz else e
    return errs, ref, mod


def test_rounding_model_is_within_the_figures_the_limits_come_from():
    """L = 4 x the largest err / unit of the rounding model against fp64 (module docstring of _attn_ref): this is that measurement."""
    worst = {}
    for kind in KINDS:
        kmax = {}
        for geom in GEOMS:
            for do_kind in (("normal", "pad_only") if geom[6] and kind == "diffuse" else ("normal",)):
                errs, _, _ = _model_errs(geom, kind, do_kind)
                for n, e in errs.items():
                    kmax[n] = max(kmax.get(n, 0.0), e)
        for n, e in kmax.items():
            print(f"ATTN-MODEL {n} {kind} {e:.3g}")
            worst[n] = max(worst.get(n, 0.0), e)
    for n, e in worst.items():
        print(f"ATTN-MODEL {n} ALL {e:.3g}   MODEL_MAX {R.MODEL_MAX[n]:.3g}   limit {R.LIMITS[n]:.3g}")
    for n, e in worst.items():
        assert e <= R.MODEL_MAX[n], (n, e, R.MODEL_MAX[n])
        assert R.LIMITS[n] == 4.0 * R.MODEL_MAX[n]
        assert e >= R.MODEL_MAX[n] / 2, f"{n}: MODEL_MAX {R.MODEL_MAX[n]} is not the measured figure ({e:.3g})"


FAULT_GEOM = {
    "causal": (1, 512, 2, 2, 128, True, None),
    "ragged": (2, 320, 2, 2, 128, True, [257, 200]),
    "gqa": (1, 320, 4, 2, 64, True, None),
    "any": (1, 320, 2, 1, 128, False, None),
}
# where the old criterion is counted: the same kind of geometry at the largest CPU-sized S (a late row spreads its mass over ~S keys)
OLD_GEOM = dict(FAULT_GEOM, causal=(1, 1024, 1, 1, 128, True, None), ragged=(2, 1024, 1, 1, 128, True, [1000, 897]))
# the assertions of tests/test_kernels_gpu.py::test_attn_fwd_bwd (rtol, afrac of close())
OLD = {"O": (2 ** -6, 2 ** -7), "lse": (1e-3, 1e-3), "dQ": (2 ** -5, 2 ** -6), "dK": (2 ** -5, 2 ** -6), "dV": (2 ** -5, 2 ** -6)}


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if R.FAULTS[f][1] != "decode"])
def test_every_seeded_fault_exceeds_a_limit_by_8x_on_hot_inputs(fault):
    hooks, need = R.FAULTS[fault]
    geom = FAULT_GEOM[need]
    errs, _, _ = _model_errs(geom, "hot", hooks=hooks, seed=5)
    over = {n: e / R.LIMITS[n] for n, e in errs.items()}
    name = max(over, key=over.get)
    # what the old criterion sees of the same fault on the diffuse input
    _, ref, mod = _model_errs(OLD_GEOM[need], "diffuse", hooks=hooks, seed=5)
    old = {n: R.old_close_count(mod[n], ref[n], *OLD[n]) for n in OLD}
    print(f"ATTN-FAULT {fault} {name} {errs[name]:.3g} {over[name]:.1f}x limit (" + " ".join(f"{n} {o:.3g}x" for n, o in over.items())
          + f") | old close() on diffuse input: {sum(old.values())} elements {old}")
    assert over[name] >= 8.0, (fault, errs, over)


def test_clean_model_passes_where_the_faults_fail():
    for need, geom in FAULT_GEOM.items():
        errs, _, _ = _model_errs(geom, "hot", seed=5)
        for n, e in errs.items():
            assert e <= R.LIMITS[n] / 4, (need, n, e)


DEC = [(5, 700, [0, 1, 255, 257, 700], 4, 4, 128, "diffuse"), (4, 700, [513, 256, 707, 600], 8, 2, 64, "hot"),
       (2, 700, [600, 600], 14, 2, 64, "spike"), (3, 5, [5, 12, 0], 4, 4, 128, "hot")]


@pytest.mark.parametrize("case", DEC, ids=str)
def test_decode_ref_and_model(case):
    B, smax, lens, nh, nkv, hd, kind = case
    q, kc, vc, scale = R.make_decode_case(kind, B, smax, lens, nh, nkv, hd, seed=2)
    ref, unit = R.decode_ref64(q, kc, vc, lens, nh, nkv, hd, scale)
    for b in range(B):
        L = min(lens[b], smax)
        if L == 0:
            assert ref[b].abs().max() == 0 and unit[b].abs().max() == 0
            continue
        qq = q[b].double().reshape(nh, 1, hd)
        kk = kc[b, :L].double().reshape(L, nkv, hd).permute(1, 0, 2).repeat_interleave(nh // nkv, 0)
        vv = vc[b, :L].double().reshape(L, nkv, hd).permute(1, 0, 2).repeat_interleave(nh // nkv, 0)
        o = torch.softmax(qq @ kk.transpose(1, 2) * scale, -1) @ vv
        assert (o.reshape(-1) - ref[b]).abs().max() < 1e-12
    # decode equals the last causal row of the prefill reference
    b = max(range(B), key=lambda i: min(lens[i], smax))
    L = min(lens[b], smax)
    full = R.attn_ref64(q[b].reshape(1, 1, nh, hd).expand(1, L, nh, hd), kc[b, :L].reshape(1, L, nkv, hd), vc[b, :L].reshape(1, L, nkv, hd),
                        None, scale, True)
    assert (full["O"][0, L - 1].reshape(-1) - ref[b]).abs().max() < 1e-12
    mod = R.decode_model(q, kc, vc, lens, nh, nkv, hd, scale)
    e, idx, nz = R.err_units(mod, ref, unit)
    print(f"ATTN-MODEL dec {kind} {e:.3g}")
    assert nz == 0 and e <= R.MODEL_MAX["O"], (e, idx)
    if kind == "spike":
        hooks, _ = R.FAULTS["decode_skipped_rescale"]
        bad = R.decode_model(q, kc, vc, lens, nh, nkv, hd, scale, hooks)
        eb, _, _ = R.err_units(bad, ref, unit)
        lim = R.LIMITS["O"]
        print(f"ATTN-FAULT decode_skipped_rescale dec {eb:.3g} {eb / lim:.1f}x limit")
        assert eb >= 8 * R.LIMITS["O"], eb
