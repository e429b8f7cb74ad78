"""No GPU: the case table of tests/input_forms.py is complete, HOST_ONLY holds only what binds nothing to a kernel, and what has to be
refused is refused on the host - a tensor that does not live on the device, a caller's output buffer of another dtype or layout, a
retyped table a function chooses not to convert - with SfmiError, before the library is touched.  The contract is input_forms.py's."""
import importlib
import inspect
import re

import pytest
import torch

import input_forms as IF
from shapeformer_amd import _lib as L

CPU = torch.device("cpu")
TOOL_KEYS = [k for k in IF.CASES if not k.startswith("VQDIF.")]


def _public(mod):
    M = importlib.import_module("shapeformer_amd." + mod)
    return {k: v for k, v in vars(M).items() if inspect.isfunction(v) and v.__module__ == M.__name__ and not k.startswith("_")}


def test_every_public_function_is_tabulated_or_host_only():
    tabulated = {IF.base_name(k) for k in IF.CASES}
    total = 0
    for mod in IF.MODULES:
        for name in _public(mod):
            key = f"{mod}.{name}"
            total += 1
            assert (key in tabulated) != (key in IF.HOST_ONLY), f"{key}: in the case table or in HOST_ONLY, never both, never neither"
    assert total == len([k for k in tabulated if not k.startswith("VQDIF.")]) + len(IF.HOST_ONLY), "an entry names no public function"
    for k in list(tabulated) + list(IF.HOST_ONLY):
        mod, name = k.split(".")
        assert mod == "VQDIF" or name in _public(mod), f"{k} is not a public function"


def test_the_vqdif_methods_are_tabulated():
    from shapeformer_amd.vqdif import VQDIF
    for m in IF.VQDIF_METHODS:
        assert callable(getattr(VQDIF, m)) and f"VQDIF.{m}" in IF.CASES
    assert {IF.base_name(k) for k in IF.CASES if k.startswith("VQDIF.")} == {f"VQDIF.{m}" for m in IF.VQDIF_METHODS}


def test_every_tensor_argument_has_a_role_and_a_variant():
    for key in IF.CASES:
        fn = None if key.startswith("VQDIF.") else IF.resolve(key)
        kw = IF.CASES[key].build(CPU) if fn is not None else None
        assert IF.tensor_args(key), key
        for a, arg in IF.tensor_args(key):
            assert len(IF.variant_names(arg)) >= 1
            assert kw is None or a in kw, f"{key}: the builder gives no {a}"
        if fn is not None and IF.CASES[key].call is None:
            # no tensor of the canonical call goes without a role
            for a, v in kw.items():
                assert a in inspect.signature(fn).parameters or any(p.kind == p.VAR_KEYWORD for p in inspect.signature(fn).parameters.values())
                holds = isinstance(v, torch.Tensor) or (isinstance(v, (list, tuple)) and any(isinstance(e, torch.Tensor) for e in v))
                roles = {r for k in IF.CASES if IF.base_name(k) == IF.base_name(key) for r in IF.CASES[k].roles}    # a "#form" adds to its base
                assert not holds or a in roles, f"{key}: tensor argument {a} has no role"


def test_a_parameter_that_has_a_role_somewhere_has_one_everywhere():
    """the builders pass only some optional arguments: a parameter whose name is a tensor's role in any row of the table (off, offs,
    pairs, up, viewpoint, idx, ...) must have a role in every tabulated function that takes it"""
    names = {r for k in IF.CASES for r in IF.CASES[k].roles}
    for base in {IF.base_name(k) for k in IF.CASES if not k.startswith("VQDIF.")}:
        fn = IF.resolve(base)
        if any(IF.CASES[k].call is not None for k in IF.CASES if IF.base_name(k) == base):
            continue
        roles = {r for k in IF.CASES if IF.base_name(k) == base for r in IF.CASES[k].roles}
        missing = (set(inspect.signature(fn).parameters) & names) - roles - IF.NOT_TENSORS.get(base, set())
        assert not missing, f"{base}: {sorted(missing)} have no role"


def test_host_only_functions_bind_nothing_to_a_kernel():
    """the cap on HOST_ONLY, mechanically: no L.ptr( in the function, nor in a private helper of its module that it names"""
    for key, reason in IF.HOST_ONLY.items():
        mod, name = key.split(".")
        M = importlib.import_module("shapeformer_amd." + mod)
        src = inspect.getsource(getattr(M, name))
        assert reason and "L.ptr(" not in src, f"{key} hands a pointer to the library"
        for helper in set(re.findall(r"\b(_[A-Za-z]\w*)\b", src)):
            h = getattr(M, helper, None)
            if inspect.isfunction(h) or inspect.isclass(h):
                assert "L.ptr(" not in inspect.getsource(h), f"{key} calls {helper}, which hands a pointer to the library"


@pytest.fixture
def no_library(monkeypatch):
    def fail():
        pytest.fail("the library was loaded before the arguments were checked")
    return lambda: monkeypatch.setattr(L, "lib", fail)


@pytest.mark.parametrize("key", [k for k in TOOL_KEYS if IF.CASES[k].refuses_cpu])
def test_cpu_tensors_are_refused_before_the_library_is_touched(key, no_library):
    """with no device here every tensor of the call is a CPU tensor; test_input_forms_gpu.py replaces one argument at a time (`cpu`)"""
    kw = IF.CASES[key].build(CPU)                    # the weight packs of the ops cases load the library: build first
    no_library()
    with pytest.raises(L.SfmiError):
        IF.invoke(key, kw)


def _host_refusals():
    out = []
    for key in TOOL_KEYS:
        for a, arg in IF.tensor_args(key):
            for v in IF.variant_names(arg):
                if v != "cpu" and IF.expectation(arg, v) == "refuse" and arg.role in IF.DEVICE_ROLES:
                    out.append((key, a, v))
    return out


@pytest.mark.parametrize("key,a,v", _host_refusals(), ids=lambda x: x)
def test_refused_forms_are_refused_for_what_they_are(key, a, v, no_library):
    """an output buffer of another dtype or layout, and every retyped or strided table a function refuses: the refusal names the
    argument (the device is checked last, and every tensor here is a CPU tensor), comes before the library and leaves the buffer alone"""
    kw = IF.CASES[key].build(CPU)
    value, parents = IF.make_variant(IF.CASES[key].roles[a], v, kw[a], CPU)
    before = [IF.raw_bytes(p) for p in parents]
    no_library()
    with pytest.raises(L.SfmiError) as e:
        IF.invoke(key, dict(kw, **{a: value}))
    msg = str(e.value)
    assert re.search(rf"\b{re.escape(a)}\b", msg), f"{key}({a}: {v}) was refused for another reason: {msg}"
    assert all(torch.equal(b, IF.raw_bytes(p)) for b, p in zip(before, parents))
