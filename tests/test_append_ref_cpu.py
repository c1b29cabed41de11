"""The fp32 model of lmod_attn_append (tests/_append_ref.py) against the fp64 reference: where the limit L of the GPU test comes from,
and that L is tight enough to catch seeded faults.  No GPU."""
import pytest
import torch

import _append_ref as R

# (hd, nh, nkv, T, lens after the append, n_b per sample or None, nsplit)
GEOMS = [
    (128, 28, 4, 8, [2049 + 8], None, 4),             # teacher geometry (group 7), long history
    (64, 14, 2, 5, [700, 257], [5, 3], 3),            # student geometry (hd 64, group 7), ragged chunk
    (128, 8, 2, 16, [256, 16, 17], None, 2),          # group 4, T_MAX; empty history (lens = n_b) and 1 + n_b
    (64, 4, 4, 2, [255, 3], [2, 1], 1),               # group 1, one split
    (128, 4, 1, 1, [700], None, 5),                   # T = 1: the decode case
]
KINDS = ["diffuse", "hot", "spike"]


def _figure(kind, geom, hooks=None):
    hd, nh, nkv, T, lens, ns, nsplit = geom
    q, kc, vc, lt, cu, scale = R.make_append_case(kind, lens, ns, T, nh, nkv, hd)
    ref, unit = R.append_ref64(q, kc, vc, lt, cu, T, nh, nkv, hd, scale)
    out = R.append_model(q, kc, vc, lt, cu, T, nh, nkv, hd, scale, nsplit=nsplit, hooks=hooks)
    return R.err_units(out, ref, unit)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"hd{g[0]}-g{g[1] // g[2]}-T{g[3]}-s{g[6]}")
@pytest.mark.parametrize("kind", KINDS)
def test_model_within_model_max(kind, geom):
    fig, idx, nz = _figure(kind, geom)
    print(f"APPEND-MODEL {kind} {geom}: {fig:.3e} at {idx}")
    assert nz == 0
    assert fig <= R.MODEL_MAX
    assert R.LIMIT == 4.0 * R.MODEL_MAX


def test_reference_masks_the_chunk_causally():
    """The reference itself against a dense softmax over prompt + chunk: query t of the chunk is row L - n + t of full causal attention."""
    hd, nh, nkv, T, L = 64, 4, 2, 3, 11
    q, kc, vc, lt, cu, scale = R.make_append_case("diffuse", [L], None, T, nh, nkv, hd)
    ref, _ = R.append_ref64(q, kc, vc, lt, cu, T, nh, nkv, hd, scale)
    for h in range(nh):
        hk = h // (nh // nkv)
        Kh, V = kc[0, :L, hk * hd:(hk + 1) * hd].double(), vc[0, :L, hk * hd:(hk + 1) * hd].double()
        for t in range(T):
            s = (Kh[:L - T + t + 1] @ q[t, h * hd:(h + 1) * hd].double()) * scale
            assert torch.allclose(ref[t, h * hd:(h + 1) * hd], torch.softmax(s, 0) @ V[:L - T + t + 1], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("fault", sorted(R.FAULTS))
def test_seeded_faults_exceed_the_limit(fault):
    hooks, _ = R.FAULTS[fault]
    worst = max(_figure("hot", g, hooks)[0] for g in (GEOMS[0], GEOMS[1]))
    print(f"APPEND-FAULT {fault}: {worst:.3e} (L = {R.LIMIT:.3e})")
    assert worst > R.LIMIT
