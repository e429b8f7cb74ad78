"""CPU side of the convolution harness (tests/conv_ref.py): the float64 references against torch's float64 conv3d / group_norm on
non-cubic inputs, the error bounds against deliberate mistakes ("teeth": a bound that a dropped chunk, a shifted tap, swapped axes,
padding before the affine, a misplaced parity or a lost fold block does not exceed would let those bugs pass), conv_form against the
source text of conv_dispatch and over the GPU case table, and the argument checks of the three entry points.  No GPU.

How much room the bounds leave (torch CPU fp32 as a stand-in for the kernel, printed by test_bounds_have_teeth with pytest -s): the
stand-in itself stays below 0.015 of the bound everywhere.  One dropped 16-channel chunk violates the bound on 29-55 % of the elements
at K = 256 .. 1296 (the ReLU zeroes about half of them in the mutant and in the reference alike) and on 17 % at K = 20736 with the
ACC2 depth (n = 438); a bound TEN times wider is still violated on 28-55 % and 11 % of them, so it would still fail these mutants for
the per-tap, x-reuse, sub-pixel, stride-2 and ACC2 forms.  With the un-blocked depth (n = 20736) the same mutant at K = 20736 violates
the bound on 1.2 % of the elements and a tenfold-wider one on none: per-element bounds cannot guard the accumulation depth of
UNet3D's deepest layers, which is why tests/test_conv_kernels_gpu.py gates their rms error against torch CPU fp32 as well."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import conv_ref as R                                   # noqa: E402
from test_conv_kernels_gpu import CASES, Case, GEMM_KS, GEMM_MS, GEMM_NS, KNOBS, _gemm_cases   # noqa: E402


def _lib():
    from shapeformer_amd import _lib as L
    return L.lib()


def _inputs(c, seed):
    g = torch.Generator().manual_seed(seed)
    ks = 3 if c.subpixel else c.KS
    x = torch.randn(c.B, *c.grid, c.Cin, generator=g)
    w = torch.randn(c.Cout, c.Cin, ks, ks, ks, generator=g) / (c.Cin * ks ** 3) ** 0.5
    bias = torch.randn(c.Cout, generator=g) if c.bias else None
    sc = torch.rand(c.B, c.Cin, generator=g) + 0.5 if c.aff else None
    sh = torch.randn(c.B, c.Cin, generator=g) if c.aff else None
    geom = (3, 1, 1, 1) if c.subpixel else (c.KS, c.stride, c.pad, c.up)
    return x, w, sc, sh, bias, geom


def _torch_conv(x, w, sc, sh, bias, geom, act, dtype):
    ks, stride, pad, up = geom
    xin = x.to(dtype)
    if sc is not None:
        xin = xin * sc.to(dtype)[:, None, None, None, :] + sh.to(dtype)[:, None, None, None, :]
    xin = xin.permute(0, 4, 1, 2, 3)
    if up:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    y = F.conv3d(xin, w.to(dtype), None if bias is None else bias.to(dtype), stride=stride, padding=pad)
    y = y if act == 0 else F.relu(y) if act == 1 else F.gelu(y)
    return y.permute(0, 2, 3, 4, 1)


# ---------------------------------------------------------------------------------------------------- references restate the model
@pytest.mark.parametrize("c", [Case("k3", 2, (3, 5, 8), 16, 32), Case("k3 up gelu", 2, (3, 2, 5), 16, 32, up=1, act=2),
                               Case("k2s2 odd", 2, (5, 7, 9), 16, 32, KS=2, stride=2, pad=0, act=0), Case("k1", 1, (2, 3, 4), 32, 32, KS=1, pad=0, aff=False),
                               Case("k3p0", 2, (5, 4, 7), 16, 64, pad=0, bias=False), Case("subpixel", 2, (3, 5, 4), 16, 32, subpixel=True)],
                         ids=lambda c: c.name)
def test_conv_ref_is_torch_float64_conv3d(c):
    x, w, sc, sh, bias, geom = _inputs(c, 1)
    p = R.conv_ref(x, w, sc, sh, bias, *geom, c.act, parts=True)
    want = _torch_conv(x, w, sc, sh, bias, geom, c.act, torch.float64)
    assert p["y"].shape == want.shape
    assert torch.allclose(p["y"], want, rtol=1e-12, atol=1e-12)
    assert bool((p["A"] >= p["pre"].abs() - (0 if bias is None else bias.double().abs()) - 1e-12).all())      # |w| conv |x| dominates
    assert bool((p["E"] >= 0).all()) and (sc is not None or float(p["E"].max()) == 0.0)


def test_subpixel_packer_is_the_direct_form_in_float64():
    """sfmi_conv_pack_weight_subpixel's layout and pads as the header states them: eight 2^3 convolutions of the low-resolution grid
    with the packed weights, parity p written to voxels 2 v + p, equal conv3(nearest_x2(x)) with the original weights."""
    lib = _lib()
    c = Case("sp", 2, (3, 5, 4), 16, 32, subpixel=True)
    x, w, sc, sh, bias, geom = _inputs(c, 2)
    ws = np.empty(64 * c.Cout * c.Cin, np.float32)
    assert lib.sfmi_conv_pack_weight_subpixel(np.ascontiguousarray(w.numpy()).ctypes.data, c.Cout, c.Cin, ws.ctypes.data) == 0
    ws = torch.from_numpy(ws).view(8, 8, c.Cout, c.Cin).double()
    want = R.conv_ref(x, w, sc, sh, bias, 3, 1, 1, 1, 0)
    got = torch.empty_like(want)
    xa, _ = R.affine_pad(x, sc, sh, 1, 0)
    D, H, W = c.grid
    for par in range(8):
        pz, py, px = par >> 2, (par >> 1) & 1, par & 1
        wp = ws[par].view(2, 2, 2, c.Cout, c.Cin).permute(3, 4, 0, 1, 2)
        win = xa[:, pz:pz + D + 1, py:py + H + 1, px:px + W + 1]                      # leading pad 1 - parity per axis
        got[:, pz::2, py::2, px::2] = R.correlate(win, wp, 2, 1, (D, H, W)) + bias.double()
    assert torch.allclose(got, want, rtol=0, atol=1e-6)                               # f32 weight sums: ~1e-7


def test_groupnorm_and_gemm_refs_restate_the_model():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3 * 5 * 7, 24, generator=g) * 3 + 1
    gam, bet = torch.rand(24, generator=g) + 0.5, torch.randn(24, generator=g)
    for groups in (1, 8):
        sc, sh, ds, dt = R.groupnorm_coeffs_ref(x, gam, bet, groups)
        want = F.group_norm(x.double().permute(0, 2, 1), groups, gam.double(), bet.double(), 1e-5).permute(0, 2, 1)
        assert torch.allclose(x.double() * sc[:, None] + sh[:, None], want, rtol=1e-11, atol=1e-11)
        assert bool((ds > 0).all()) and bool((dt > 0).all()) and float((ds / sc.abs()).max()) < 1e-6
    # a mean of 100 standard deviations: the one-pass variance has lost (mean / std)^2 = 1e4 of f64's digits, still far below f32's u
    _, _, ds, _ = R.groupnorm_coeffs_ref(torch.randn(1, 4099, 24, generator=g) + 100.0, gam, bet, 8)
    assert float(ds.max()) < 1e-6
    sums = R.chan_sums_ref(x)
    assert torch.allclose(sums[..., 0], x.double().sum(1)) and torch.allclose(sums[..., 1], (x.double() ** 2).sum(1))
    xm, W, b = torch.randn(7, 32, generator=g), torch.randn(64, 32, generator=g), torch.randn(64, generator=g)
    res = torch.randn(12, 64, generator=g)
    rows, y, pre, P, r = R.gemm_ref(xm, W, b, 2, res, 3, 5)
    assert rows.tolist() == [0, 1, 2, 5, 6, 7, 10]
    assert torch.allclose(y, F.gelu(xm.double() @ W.double().T + b.double()) + res.double()[rows], rtol=1e-12, atol=1e-12)
    y = torch.randn(2, 4, 8, 16, 32, generator=g)
    t = R.tile_sums_ref(y, 256)
    assert t.shape == (2, 2, 32, 3) and torch.allclose(t[1, 1, :, 0], y[1].reshape(-1, 32)[256:].double().sum(0))
    t = R.tile_sums_ref(y, 32, subpixel=True)                      # low-resolution lattice 2 x 4 x 8 = 64 voxels: 2 tiles per parity
    assert t.shape == (2, 16, 32, 3)
    assert torch.allclose(t[0, 2 * 5 + 1, :, 1], (y[0, 1::2, 0::2, 1::2].reshape(-1, 32)[32:].double() ** 2).sum(0))


# ---------------------------------------------------------------------------------------------------- the launcher mirror
def _source_instances():
    src = open(os.path.join(ROOT, "shapeformer_amd", "csrc", "conv3d.hip")).read()
    body = src[src.index("static int conv_dispatch("):src.index('extern "C"')]
    out = set()
    for m in re.finditer(r"conv3d_igemm_kernel<([^>]*)>", body):
        a = [s.strip() for s in m.group(1).split(",")]
        a += ["false", "2", "false"][len(a) - 4:]                  # template defaults: XR = false, J = 2, ST = false
        assert len(a) == 7, m.group(0)
        out.add(tuple(int({"true": 1, "false": 0}.get(v, v)) for v in a))
    return out


def test_instance_list_is_the_source_text_of_conv_dispatch():
    assert len(R.CONV_INSTANCES) == 14 == len(set(R.CONV_INSTANCES))
    assert sorted(_source_instances()) == R.CONV_INSTANCES


def test_conv_form_is_total_and_the_gpu_table_reaches_every_instance():
    seen, wos, couts, cins = set(), set(), set(), set()
    straddle = {}
    for c in CASES:
        forms = c.forms()
        assert forms[2] is not None, c.name                       # every row runs at the default knob
        for knob in KNOBS:
            f = forms[knob]
            if f is None:
                assert c.stats and knob < 2, (c.name, knob)       # only a *_stats launch without a statistics instance is refused
                continue
            assert f.instance in R.CONV_INSTANCES and f.blocks >= 1 and f.n >= 16
            if knob in c.knobs():
                seen.add(f.instance)
                straddle.setdefault(f.instance, set()).add((f.straddle, f.partial, f.blocks % 8 != 0))
        f = forms[2]
        wos.add(f.Wo)
        couts.add(c.Cout)
        cins.add(c.Cin)
    assert sorted(seen) == R.CONV_INSTANCES, sorted(set(R.CONV_INSTANCES) - seen)
    assert {1, 2, 4, 128, 256} <= wos and {32, 96, 64, 192, 128, 384} <= couts and {16, 48, 768} <= cins
    for inst in R.CONV_INSTANCES:                                  # every instance on a non-cubic grid
        assert any(len(set(c.grid)) == 3 and any(f is not None and f.instance == inst and k in c.knobs() for k, f in c.forms().items())
                   for c in CASES), inst
    # straddling tiles, partly empty last tiles and block counts that are no multiple of 8 on x-reuse and per-tap forms alike
    for inst in [(1, 1, 4, 0, 1, 2, 0), (2, 1, 4, 0, 1, 2, 0), (1, 2, 2, 0, 1, 2, 0), (2, 2, 2, 0, 1, 2, 0), (1, 1, 4, 0, 0, 2, 0), (2, 2, 2, 0, 0, 2, 0)]:
        got = straddle[inst]
        assert any(s for s, _, _ in got) and any(p for _, p, _ in got) and any(b for _, _, b in got), (inst, got)
    # the J = 4 instances are launched only where no tile straddles two shapes (conv3d.hip load_chunk)
    for inst in [(1, 1, 4, 0, 1, 4, 0), (1, 1, 4, 0, 1, 4, 1)]:
        assert all(not s and not p for s, p, _ in straddle[inst])
    for M, N, K, *_, og, ogs in _gemm_cases():
        for knob in KNOBS:
            assert R.gemm_form(M, N, K, knob, og, ogs).instance[3:] == (0, 0, 2, 0)
    assert {(m, n, k) for m in GEMM_MS for n in GEMM_NS for k in GEMM_KS} <= {(m, n, k) for m, n, k, *_ in _gemm_cases()}
    # depth of the blocked form: 384 products + one add per fold; un-blocked: every product
    assert R.chain_depth(R.ACC2_INSTANCE, 768, 3) == 384 + 54 and R.chain_depth((2, 2, 2, 0, 0, 2, 0), 768, 3) == 20736
    assert R.chain_depth(R.ACC2_INSTANCE, 48, 3) == 384 + 4 and R.chain_depth(R.ACC2_INSTANCE, 16, 2) == 128 + 1


# ---------------------------------------------------------------------------------------------------- teeth
TEETH = [("per-tap", Case("t", 2, (3, 5, 8), 32, 32), 0), ("x-reuse", Case("t", 2, (6, 4, 16), 32, 64), 2),
         ("ACC2", Case("t", 2, (3, 5, 8), 48, 128), 2), ("ACC2 K=20736", Case("t", 1, (2, 3, 4), 768, 128, bias=False), 2),
         ("un-blocked K=20736", Case("t", 1, (2, 3, 4), 768, 128, bias=False), 0),
         ("sub-pixel", Case("t", 2, (3, 5, 4), 32, 32, subpixel=True), 2), ("stride 2", Case("t", 2, (5, 7, 9), 32, 64, KS=2, stride=2, pad=0), 2)]


def _mutants(c, form, x, w, sc, sh, bias, geom, y):
    ks, stride, pad, up = geom
    run = lambda **kw: R.conv_ref(kw.pop("x", x), w, sc, sh, bias, *geom, c.act, **kw)
    tap = (0, min(1, ks - 1), ks - 1)

    def drop(dz, dy, dx, sl, wt):
        if (dz, dy, dx) == tap:
            wt = wt.clone()
            wt[:, 16:32] = 0
        return sl, wt
    out = [("one 16-channel chunk of one tap dropped", run(hook=drop))]
    for ax in (1, 2, 3):
        def shift(dz, dy, dx, sl, wt, ax=ax):
            return (torch.roll(sl, 1, dims=ax) if (dz, dy, dx) == tap else sl), wt
        out.append((f"one tap shifted by one voxel along axis {ax}", run(hook=shift)))
    B, D, H, W, C = x.shape
    out.append(("H and W swapped", run(x=x.reshape(B, D, W, H, C).transpose(2, 3))))
    if sc is not None and pad > 0:
        out.append(("zero padding before the affine", run(pad_first=True)))
    if c.subpixel:
        ym = y.clone()
        ym[:, 0::2, 0::2, 0::2] = y[:, 0::2, 0::2, 1::2]
        out.append(("one sub-pixel parity written to its neighbour", ym))
    if form.instance == R.ACC2_INSTANCE:
        cpt = c.Cin // 16
        chunks = ks * ks * cpt
        if chunks % R.FOLD:
            def lost(dz, dy, dx, sl, wt):
                wt = wt.clone()
                for cc in range(cpt):
                    if (dz * ks + dy) * cpt + cc >= chunks // R.FOLD * R.FOLD:
                        wt[:, 16 * cc:16 * cc + 16] = 0
                return sl, wt
            out.append(("the last partial fold block dropped", run(hook=lost)))
    return out


@pytest.mark.parametrize("name,c,knob", TEETH, ids=[t[0] for t in TEETH])
def test_bounds_have_teeth(name, c, knob):
    """Every mutant of the reference, evaluated in float64, exceeds the bound of the form on at least one element; torch fp32 (a
    correct implementation with another summation order) stays inside it.  See the module docstring for the tenfold statement."""
    form = c.forms()[knob]
    x, w, sc, sh, bias, geom = _inputs(c, 7)
    p = R.conv_ref(x, w, sc, sh, bias, *geom, c.act, parts=True)
    n = R.chain_depth(form.instance, c.Cin, 2 if c.subpixel else c.KS)
    bound = R.conv_bound(p, n, bias, c.act, c.subpixel)
    assert bool((bound > 0).all())
    stand_in = float(((_torch_conv(x, w, sc, sh, bias, geom, c.act, torch.float32).double() - p["y"]).abs() / bound).max())
    print(f"[teeth] {name} {form.instance} n {n}: torch fp32 at {stand_in:.3g} of the bound")
    assert stand_in < 0.1
    for what, ym in _mutants(c, form, x, w, sc, sh, bias, geom, p["y"]):
        d = (ym - p["y"]).abs()
        frac, frac10 = float((d > bound).double().mean()), float((d > 10 * bound).double().mean())
        print(f"[teeth] {name}: {what}: over the bound on {100 * frac:.1f} % of the elements, over 10 x the bound on {100 * frac10:.1f} %")
        assert frac > 0, (name, what)
        if what.startswith("one 16-channel chunk"):
            if name == "un-blocked K=20736":
                assert frac < 0.1 and frac10 == 0        # the depth of 20736 roundings hides a lost chunk from a tenfold-wider bound
            else:
                assert frac >= 0.1 and frac10 > 0        # every other form: a tenfold-wider bound still fails


def test_gemm_bound_has_teeth():
    g = torch.Generator().manual_seed(11)
    M, N, K, og, ogs = 300, 64, 1024, 100, 130
    x, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / 32, torch.randn(N, generator=g)
    rows_out = int(R.remap_rows(M, og, ogs)[-1]) + 2 + M // og
    res = torch.randn(rows_out, N, generator=g)
    rows, y, pre, P, r = R.gemm_ref(x, W, b, 2, res, og, ogs)
    bound = R.gemm_bound(pre, P, K, True, 2, r)
    y32 = F.gelu(x @ W.T + b) + res[rows]
    assert float(((y32.double() - y).abs() / bound).max()) < 0.1
    full, fb = torch.zeros(rows_out, N, dtype=torch.float64), torch.zeros(rows_out, N, dtype=torch.float64)
    full[rows], fb[rows] = y, bound
    # remap stride off by one row
    rows_m, y_m, *_ = R.gemm_ref(x, W, b, 2, res, og, ogs + 1)
    mut = torch.zeros_like(full)
    mut[rows_m] = y_m
    assert bool(((mut - full).abs() > fb).any())
    # residual read from the un-remapped row
    _, y_m, *_ = R.gemm_ref(x, W, b, 2, res, og, ogs, resid_unmapped=True)
    assert bool(((y_m - y).abs() > bound).any())
    assert bool(((y_m - y)[:og].abs() == 0).all())                 # (group 0 maps onto itself: only later groups can tell)


# ---------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_refuse_bad_geometry_before_launching():
    """The convolution, GEMM and GroupNorm entries return SFMI_EINVAL before they touch a pointer or launch anything (dummy non-null
    pointers, no GPU)."""
    lib = _lib()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    EINVAL = -1

    def conv(B=2, Di=4, Hi=5, Wi=6, Cin=16, Cout=32, KS=3, stride=1, pad=1, up=0, relu=1, x=p, w=p, sc=None, sh=None, y=p, partial=None, splits=None):
        return lib.sfmi_conv3d_cl_stats_f32(x, w, sc, sh, None, y, B, Di, Hi, Wi, Cin, Cout, KS, stride, pad, up, relu, partial, splits, None)

    bad = [dict(stride=0), dict(stride=-1), dict(pad=-1), dict(up=2), dict(up=-1), dict(Di=0), dict(Hi=0), dict(Wi=-3), dict(B=0),
           dict(KS=3, pad=0, Di=1), dict(KS=3, pad=0, Hi=2), dict(KS=2, pad=0, Wi=1), dict(Cin=24), dict(Cin=0), dict(Cout=48), dict(Cout=0),
           dict(KS=0), dict(KS=4), dict(sc=p), dict(sh=p), dict(partial=p), dict(splits=p), dict(x=None), dict(w=None), dict(y=None),
           dict(Di=1 << 21), dict(pad=1 << 21)]
    for kw in bad:
        assert conv(**kw) == EINVAL, kw
        if "partial" not in kw and "splits" not in kw:
            assert conv(**dict(kw, partial=p, splits=p)) == EINVAL, kw
            if not {"x", "w", "y"} & set(kw):                      # the mirror refuses what the entry refuses
                with pytest.raises(ValueError):
                    R.conv_form(kw.get("B", 2), kw.get("Di", 4), kw.get("Hi", 5), kw.get("Wi", 6), kw.get("Cin", 16), kw.get("Cout", 32),
                                kw.get("KS", 3), kw.get("stride", 1), kw.get("pad", 1), kw.get("up", 0), has_scale="sc" in kw, has_shift="sh" in kw)
    # the plain entry is the same function without the partials
    assert lib.sfmi_conv3d_cl_f32(p, p, None, None, None, p, 2, 4, 5, 6, 16, 32, 3, 0, 1, 0, 1, None) == EINVAL      # stride 0: was SIGFPE
    assert lib.sfmi_conv3d_cl_f32(p, p, None, None, None, p, 2, 1, 5, 6, 16, 32, 3, 1, 0, 0, 1, None) == EINVAL      # Do = -1
    # a statistics request for a geometry without a statistics instance is refused too (nothing launched)
    assert conv(partial=p, splits=p, Cout=128) == EINVAL

    def up2(B=2, Di=4, Hi=5, Wi=6, Cin=16, Cout=32, sc=None, sh=None, partial=None, splits=None, x=p):
        return lib.sfmi_conv3d_up2_cl_stats_f32(x, p, sc, sh, None, p, B, Di, Hi, Wi, Cin, Cout, 1, partial, splits, None)
    for kw in [dict(Di=0), dict(Hi=-1), dict(Wi=0), dict(B=0), dict(Cin=8), dict(Cin=0), dict(Cout=16), dict(Cout=0), dict(sc=p), dict(sh=p),
               dict(partial=p), dict(splits=p), dict(x=None), dict(Wi=1 << 21)]:
        assert up2(**kw) == EINVAL, kw
    assert lib.sfmi_conv3d_up2_cl_f32(p, p, None, None, None, p, 2, 0, 5, 6, 16, 32, 1, None) == EINVAL

    def gemm(M=100, N=64, K=32, og=0, ogs=0, x=p):
        return lib.sfmi_gemm_f32(x, p, None, None, p, M, N, K, 0, og, ogs, None)
    for kw in [dict(og=-1), dict(og=-5, ogs=10), dict(og=10, ogs=9), dict(og=10, ogs=0), dict(og=10, ogs=-20), dict(M=0), dict(M=1 << 31), dict(N=48),
               dict(N=0), dict(K=8), dict(K=0), dict(x=None)]:
        assert gemm(**kw) == EINVAL, kw
        if "x" not in kw:
            with pytest.raises(ValueError):
                R.gemm_form(kw.get("M", 100), kw.get("N", 64), kw.get("K", 32), 2, kw.get("og", 0), kw.get("ogs", 0))

    def gn(B=2, V=100, C=24, groups=8, x=p):
        return lib.sfmi_groupnorm_coeffs_f32(x, p, p, p, p, p, B, V, C, groups, 1e-5, None)

    def gnp(B=2, V=100, C=24, S=4, groups=8):
        return lib.sfmi_groupnorm_coeffs_partial_f32(p, p, p, p, p, B, V, C, S, groups, 1e-5, None)
    for kw in [dict(groups=0), dict(groups=-8), dict(groups=65, C=260), dict(groups=5), dict(B=0), dict(V=0), dict(C=0), dict(C=6, groups=1),
               dict(C=1028, groups=1)]:
        assert gn(**kw) == EINVAL, kw                              # groups = 0: was SIGFPE
        assert gnp(**kw) == EINVAL, kw
    assert gn(x=None) == EINVAL and gnp(S=0) == EINVAL
