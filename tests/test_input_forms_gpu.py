"""GPU: every public device entry point with strided and retyped inputs (the contract and the case table: tests/input_forms.py).

One case per (function, argument, variant).  The canonical call runs once per function and its outputs are kept; every case then
snapshots the bytes of every argument's parent buffer, runs the call with the one argument in its variant form, and checks that the
outputs are the canonical outputs bit for bit (or that the call was refused with SfmiError, where the table says so) and that no byte
of any argument changed.  Every comparison is bit equality or an exception type.  The shapes are the table's: the smallest at which
each function's kernels all run.  A call that must be refused runs with the library's loader replaced by one that fails the test, so it
is refused before the library is touched, argument by argument, and a wrapper that stopped refusing launches nothing.  Every other
variant keeps a wrapper that ignored its strides or dtype inside the tensors built here (see input_forms.py).  A caller-provided
output buffer is handed over zeroed on every variant call, so the variant has to write the whole result itself."""
import pytest
import torch

import input_forms as IF
from shapeformer_amd import _lib as L

pytestmark = pytest.mark.gpu

PARAMS = IF.gpu_params()
_canonical, _own = {}, {}


@pytest.fixture(scope="module")
def model(dev):
    """the res = 16 hash-weight VQDIF of test_mcubes_gpu.py::test_mesh_of_a_reconstructed_shape"""
    from shapeformer_amd import weights as W
    from shapeformer_amd.vqdif import VQDIF
    return VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)


def _run(key, kw, model):
    """the call's outputs as fresh tensors (the model's methods return views of a workspace that the next call reuses)"""
    out = [t.clone() for t in IF.flatten(IF.invoke(key, kw, model))]
    torch.cuda.synchronize()
    return out


def _tensors_of(kw):
    """the caller's own tensors among the arguments (lists and tuples of tensors included)"""
    vals = [e for v in kw.values() for e in (v if isinstance(v, (list, tuple)) else [v])]
    return [t for t in vals if isinstance(t, torch.Tensor) and t.is_contiguous()]


def _canon(key, dev, model):
    if key not in _canonical:
        kw = IF.CASES[key].build(dev)
        _canonical[key] = (kw, _run(key, kw, model))
    return _canonical[key]


def test_case_count():
    print(f"\ninput forms: {len(PARAMS)} (function, argument, variant) cases over {len(IF.CASES)} argument sets of "
          f"{len({IF.base_name(k) for k in IF.CASES})} functions")
    assert len(PARAMS) == len(set(PARAMS)) > 0


@pytest.mark.parametrize("key,a,v", PARAMS, ids=[f"{k}-{a}-{v}" for k, a, v in PARAMS])
def test_form(dev, request, monkeypatch, key, a, v):
    arg = IF.CASES[key].roles[a]
    want = IF.expectation(arg, v)
    mdl = request.getfixturevalue("model") if key.startswith("VQDIF.") else None
    kw, ref = _canon(key, dev, mdl)                                                                 # 1. the canonical call
    if want == "own":                                                                               # hpr's f64 path: its own contiguous f64 result
        if (key, a) not in _own:
            _own[key, a] = _run(key, dict(kw, **{a: IF.canonical_f64(kw[a])}), None)
        ref = _own[key, a]
    value, parents = IF.make_variant(arg, v, kw[a], dev)
    outs = {b: torch.zeros_like(kw[b]) for b, r in IF.CASES[key].roles.items() if r.role == IF.OUT and b != a}    # fresh, zeroed outputs
    call = dict(kw, **outs, **{a: value})
    inputs = {b: t for b, t in kw.items() if b not in outs and not (b == a and arg.role == IF.OUT)}
    held = [p for p in parents if isinstance(p, torch.Tensor)] + _tensors_of(inputs) + (list(outs.values()) if want == "refuse" else [])
    before = [IF.raw_bytes(t) for t in held]                                                        # 2. the bytes of every parent buffer
    if want == "refuse":                                                                            # 3. the variant call
        with monkeypatch.context() as m:
            m.setattr(L, "lib", lambda: pytest.fail(f"{key}({a}: {v}) reached the library instead of being refused"))
            with pytest.raises(L.SfmiError):
                IF.invoke(key, call, mdl)
        torch.cuda.synchronize()
    else:
        got = _run(key, call, mdl)
        assert len(got) == len(ref) > 0                                                             # 4. the same bits
        for i, (g, r) in enumerate(zip(got, ref)):
            assert IF.same_bits(g, r), f"{key}({a}: {v}): output {i} differs from the {'f64' if want == 'own' else 'canonical'} call"
    for t, b in zip(held, before):                                                                  # 5. nothing the caller owns changed
        assert torch.equal(IF.raw_bytes(t), b), f"{key}({a}: {v}) changed a caller's tensor"
