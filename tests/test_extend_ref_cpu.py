"""The fp32 model of lmod_attn_extend against its fp64 statement, on the CPU: where LIMIT in tests/_extend_ref.py comes from, and
that every seeded fault is caught by it."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _extend_ref as E  # noqa: E402


def _figure(kind, name, hd, nh, nkv, hooks=None):
    (q, kc, vc, lens, cu, scale), (ref, unit) = E.case_and_ref(kind, name, hd, nh, nkv)
    out = E.extend_model(q, kc, vc, lens, cu, E.CASES[name]["T"], nh, nkv, hd, scale, hooks=hooks)
    return E.err_units(out, ref, unit)


@pytest.mark.parametrize("name", list(E.CASES))
@pytest.mark.parametrize("hd,nh,nkv", E.GEOMS)
def test_extend_model_vs_fp64(hd, nh, nkv, name):
    """extend_model <= MODEL_MAX in err_units over every geometry, case and input kind; rows without a visible key exactly 0.  The
    largest printed figure is what MODEL_MAX records (LIMIT = 4 x MODEL_MAX)."""
    for kind in E.KINDS:
        fig, idx, nonzero = _figure(kind, name, hd, nh, nkv)
        print(f"EXTEND-MODEL {kind} hd {hd} nh {nh} nkv {nkv} case {name}: {fig:.3e} at {idx}")
        assert nonzero == 0
        assert fig <= E.MODEL_MAX, (kind, name, fig)


def test_limit_is_four_times_the_model():
    assert E.LIMIT == 4.0 * E.MODEL_MAX
    # P stays at fp32 precision as in append_model: the figure is of that model's order, far below a bf16 rounding of P (2^-9)
    from _append_ref import MODEL_MAX as APPEND_MODEL_MAX
    assert APPEND_MODEL_MAX <= E.MODEL_MAX <= 8.0 * APPEND_MODEL_MAX


@pytest.mark.parametrize("fault", list(E.FAULTS))
def test_seeded_fault_exceeds_limit(fault):
    """Every seeded fault pushes the model over LIMIT on the `hot` kind (ragged case: several query tiles, a partial last tile, GQA)."""
    hooks, _ = E.FAULTS[fault]
    hd, nh, nkv = 64, 14, 2
    fig, idx, nonzero = _figure("hot", "ragged", hd, nh, nkv, hooks=hooks)
    print(f"EXTEND-FAULT {fault}: {fig:.3e} at {idx} (LIMIT {E.LIMIT:.3e}), {nonzero} non-zero elements of unit 0")
    assert fig > E.LIMIT, (fault, fig)
