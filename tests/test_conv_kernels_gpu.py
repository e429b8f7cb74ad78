"""The implicit-GEMM convolution family of csrc/conv3d.hip against float64 (tests/conv_ref.py: references, a mirror of the launcher rule
and derived per-element error bounds) at every instance conv_dispatch can launch:

* conv3d_igemm_kernel through sfmi_conv3d_cl_f32 / sfmi_conv3d_up2_cl_f32 and their *_stats forms: one case table (CASES), every row
  run at each conv_xreuse knob that changes its instance.  Non-cubic grids with three different extents, Wo 1 .. 256, tiles inside one
  shape and tiles that straddle shapes, partly empty last tiles, block counts that are no multiple of 8, Cout 32 .. 384, Cin 16 / 48 /
  768, k1, k2 s2 on odd extents, k3 p0, the address-folded up-sampling at 32 / 64 / 128 channels, every {affine} x {bias} x {relu}
  combination on a per-tap and on an x-reuse instance, UNet3D's real layer shapes (weights.vqdif_spec) and their transposes (the input
  gradients of training).  y sits between sentinel bands, every input between NaN bands.
* the statistics epilogue against float64 sums of the y the same launch wrote; chan_stats_kernel / gn_coeffs_kernel against float64.
* sfmi_gemm_f32 with activation, bias, residual and the output-row remap.
* the blocked-accumulation claim of DESIGN.md as an rms gate against torch CPU fp32 (test_unet3d_accumulation_rms_gate).

Every ratio is printed as a `[ratio] ...` line (pytest -s).  Measured on one MI355X (largest error / bound; DESIGN.md has the table):
convolutions 0.008 .. 0.072 over the fourteen instances (ACC2 0.025, sub-pixel parities 0.003 .. 0.030), statistics partials 0.26,
GroupNorm coefficients 0.62 (mean = 100 std: 0.47), GEMM 0.27; rms of ACC2 0.94 .. 1.57 x torch CPU fp32's, of the per-tap chain
2.78 .. 6.62 x.  No kernel bug was found at these margins; the file runs in 3.4 s (the rest of the -m gpu suite: 228 s)."""
import contextlib
import ctypes
import math
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import conv_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 0x7FC0DEAD          # NaN bit pattern of every "must stay untouched" float
GUARD = 1024               # band elements on either side of every buffer
KNOBS = (2, 0, 1, 3)       # conv_xreuse values, the default first
# (b) <= RMS_GATE_M * (a).  Measured on one MI355X over UNet3D's eight layer shapes ("fp32 noise of the decoder"): (b) / (a) =
# 0.94 .. 1.57 (largest: 128 -> 256 at 8^3, boundary shell), (c) / (a) = 2.78 .. 6.62; 1.57 x 1.5 = 2.36, rounded up to one decimal.  A
# multiple of torch CPU fp32's own error, never of the code under test; (c) fails it at every shape, by 2.6 x at K = 20736.
RMS_GATE_M = 2.4


class Case:
    def __init__(self, name, B, grid, Cin, Cout, KS=3, stride=1, pad=1, up=0, aff=True, bias=True, act=1, stats=False, subpixel=False):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def forms(self):
        """{knob: ConvForm or None (the entry refuses: a *_stats launch without a statistics instance)}"""
        out = {}
        for knob in KNOBS:
            try:
                out[knob] = R.conv_form(self.B, *self.grid, self.Cin, self.Cout, self.KS, self.stride, self.pad, self.up, knob=knob,
                                        stats=self.stats, subpixel=self.subpixel, has_scale=self.aff)
            except ValueError:
                out[knob] = None
        return out

    def knobs(self):
        """the knobs to run: the first of KNOBS that reaches each distinct instance"""
        seen, out = set(), []
        for knob, f in self.forms().items():
            if f is not None and f.instance not in seen:
                seen.add(f.instance)
                out.append(knob)
        return out


def unet3d_layers(res=16):
    """(Cin, Cout, D) of every 3^3 convolution of the res-16 decoder's UNet3D, read from weights.vqdif_spec (unet3d.py:361-474: levels
    at 16^3, 8^3, 4^3)."""
    from shapeformer_amd import weights as W
    level = {"encoders.0": 16, "encoders.1": 8, "encoders.2": 4, "decoders.0": 8, "decoders.1": 16}
    out = []
    for k, shp in W.vqdif_spec(res).items():
        if k.startswith("decoder.unet3d.") and k.endswith("conv.weight") and len(shp) == 5 and shp[2] == 3:
            t = (shp[1], shp[0], level[k.split(".")[2] + "." + k.split(".")[3]])
            if t not in out:
                out.append(t)
    return out


def _cases():
    c = []
    # every output-channel tiling on non-cubic grids: straddling and partly empty tiles, block counts that are no multiple of 8
    c += [Case("c32 3x5x8", 3, (3, 5, 8), 48, 32), Case("c64 6x4x16", 5, (6, 4, 16), 16, 64), Case("c96 3x5x8", 3, (3, 5, 8), 16, 96),
          Case("c192 5x3x4", 2, (5, 3, 4), 16, 192), Case("c128 3x5x8", 3, (3, 5, 8), 48, 128),
          Case("c384 3x5x8 x183", 183, (3, 5, 8), 16, 384), Case("c384 6x4x16 x57", 57, (6, 4, 16), 16, 384, aff=False, act=0),
          Case("c128 k2s2 odd", 2, (5, 7, 9), 32, 128, KS=2, stride=2, pad=0), Case("c64 k2s2 odd", 3, (5, 7, 9), 32, 64, KS=2, stride=2, pad=0),
          Case("c64 k1", 2, (3, 5, 7), 48, 64, KS=1, pad=0), Case("c32 k3p0", 2, (5, 4, 7), 16, 32, pad=0),
          Case("c128 k3p0", 2, (5, 4, 7), 16, 128, pad=0, act=2)]
    # nearest x2 folded into the address (the direct up-sampling form)
    c += [Case(f"c{co} up", 2, (3, 2, 5), 16, co, up=1) for co in (32, 64, 128)]
    # Wo 1 .. 256 with small D, H: framed x-rows that do and do not fit the LDS, one or two x-rows per tile
    for grid in ((3, 2, 1), (2, 3, 2), (3, 5, 4), (2, 3, 128), (1, 2, 256)):
        c += [Case(f"c{co} Wo{grid[2]}", 2, grid, 16, co) for co in (32, 64, 128)]
    # every epilogue / input combination on an x-reuse and on a per-tap instance
    for aff in (True, False):
        for bias in (True, False):
            for act in (0, 1):
                c.append(Case(f"c64 xr aff{int(aff)} bias{int(bias)} relu{act}", 2, (6, 4, 16), 32, 64, aff=aff, bias=bias, act=act))
                c.append(Case(f"c32 s2 aff{int(aff)} bias{int(bias)} relu{act}", 2, (5, 6, 7), 32, 32, KS=2, stride=2, pad=0, aff=aff, bias=bias, act=act))
    # >= 1024 tiles of 512 voxels: the four-tiles-per-wave instance (1026 blocks)
    c.append(Case("c96 4x8x32 x171", 171, (4, 8, 32), 16, 96))
    # UNet3D's layers and the transposed pairs training launches as input gradients (train_vqdif.py: no affine, no bias, no ReLU)
    for ci, co, d in unet3d_layers():
        c.append(Case(f"unet {ci}->{co} @{d}", 1, (d, d, d), ci, co, bias=False))
    for ci, co, d in unet3d_layers():
        if ci != co:
            c.append(Case(f"unet dgrad {co}->{ci} @{d}", 1, (d, d, d), co, ci, aff=False, bias=False, act=0))
    # sub-pixel up-sampling convolution on non-cubic low-resolution grids
    c += [Case("up2 c32 3x5x4", 3, (3, 5, 4), 48, 32, subpixel=True), Case("up2 c64 3x5x4", 3, (3, 5, 4), 16, 64, subpixel=True, act=0),
          Case("up2 c128 3x5x4", 3, (3, 5, 4), 16, 128, subpixel=True), Case("up2 c32 2x3x1", 2, (2, 3, 1), 16, 32, subpixel=True),
          Case("up2 c96 5x2x8", 2, (5, 2, 8), 16, 96, subpixel=True, bias=False)]
    # statistics epilogue, direct and sub-pixel, 64 channels (256-voxel tiles) and 32 channels (>= 1024 tiles of 512 voxels)
    c += [Case("st c64 4x8x16", 2, (4, 8, 16), 16, 64, stats=True), Case("st c32 16x32x64 x16", 16, (16, 32, 64), 16, 32, stats=True),
          Case("st up2 c64 4x8x16", 2, (4, 8, 16), 16, 64, stats=True, subpixel=True),
          Case("st up2 c32 16x32x64 x16", 16, (16, 32, 64), 16, 32, stats=True, subpixel=True)]
    return c


CASES = _cases()


def _L():
    from shapeformer_amd import _lib as L
    return L


@contextlib.contextmanager
def _knob(value):
    """conv_xreuse for the duration, restored in a finally."""
    L = _L()
    lib = L.lib()
    old = int(lib.sfmi_tune_get(b"conv_xreuse"))
    try:
        L.check(lib.sfmi_tune_set(b"conv_xreuse", int(value)), "tune")
        yield
    finally:
        L.check(lib.sfmi_tune_set(b"conv_xreuse", old), "tune")


def _banded(t, dev, dtype=torch.float32):
    """t on the device between two bands of NaN; returns (whole buffer, view of the data)."""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = t.reshape(-1).to(dev)
    return buf, buf[GUARD:GUARD + n].view(t.shape)


def _sentinel_out(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _check_out(buf, view, what):
    bits = buf.view(torch.int32)
    n = view.numel()
    assert bool((bits[:GUARD] == SENT).all()) and bool((bits[GUARD + n:] == SENT).all()), f"{what}: wrote outside y"
    assert not bool((bits[GUARD:GUARD + n] == SENT).any()), f"{what}: left part of y unwritten"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class _Conv:
    """Inputs, float64 reference parts and launches of one CASES row."""

    def __init__(self, c, dev, seed):
        L = _L()
        self.c, self.dev = c, dev
        g = torch.Generator().manual_seed(seed)
        B, (D, H, W) = c.B, c.grid
        ks = 3 if c.subpixel else c.KS
        x = torch.randn(B, D, H, W, c.Cin, generator=g)
        w = torch.randn(c.Cout, c.Cin, ks, ks, ks, generator=g) / math.sqrt(c.Cin * ks ** 3)
        self.keep = []
        self.x = self._in(x)
        self.bias = self._in(torch.randn(c.Cout, generator=g)) if c.bias else None
        self.sc = self._in(torch.rand(B, c.Cin, generator=g) + 0.5) if c.aff else None
        self.sh = self._in(torch.randn(B, c.Cin, generator=g)) if c.aff else None
        if c.subpixel:
            ws = np.empty(64 * c.Cout * c.Cin, np.float32)
            L.check(L.lib().sfmi_conv_pack_weight_subpixel(np.ascontiguousarray(w.numpy()).ctypes.data, c.Cout, c.Cin, ws.ctypes.data), "pack_subpixel")
            self.w = self._in(torch.from_numpy(ws))
            self.geom = (3, 1, 1, 1)
        else:
            self.w = self._in(R.pack_weight(w))
            self.geom = (c.KS, c.stride, c.pad, c.up)
        self.oshape = (B,) + tuple(R.out_extent(d, *self.geom) for d in c.grid) + (c.Cout,)
        # float64 reference and the ingredients of the bound, on the device, from the ORIGINAL weights
        self.p = R.conv_ref(self.x, w.to(dev), self.sc, self.sh, self.bias, *self.geom, c.act, parts=True)

    def _in(self, t):
        buf, view = _banded(t, self.dev)
        self.keep.append(buf)
        return view

    def launch(self, stats=False):
        """One launch under the current knob into a fresh sentinel-banded y; stats: through the *_stats entry -> (y, partial (B, S, Cout, 2))."""
        L, c = _L(), self.c
        lib = L.lib()
        ybuf, y = _sentinel_out(self.oshape, self.dev)
        args = [L.ptr(self.x), L.ptr(self.w), L.ptr(self.sc), L.ptr(self.sh), L.ptr(self.bias), L.ptr(y), c.B, *c.grid, c.Cin, c.Cout]
        args += [c.act] if c.subpixel else [c.KS, c.stride, c.pad, c.up, c.act]
        part = None
        if stats:
            S = ctypes.c_int(0)
            vs = self.oshape[1] * self.oshape[2] * self.oshape[3]
            cap = c.B * (vs // 256) * c.Cout * 2
            pbuf = torch.full((cap + 2 * GUARD,), float("nan"), dtype=torch.float64, device=self.dev)
            fn = lib.sfmi_conv3d_up2_cl_stats_f32 if c.subpixel else lib.sfmi_conv3d_cl_stats_f32
            L.check(fn(*args, pbuf[GUARD:].data_ptr(), ctypes.addressof(S), L.stream_ptr()), "conv stats")
            torch.cuda.synchronize()
            n = c.B * S.value * c.Cout * 2
            assert 0 < n <= cap
            assert bool(pbuf[:GUARD].isnan().all()) and bool(pbuf[GUARD + n:].isnan().all()), "partials written outside (B, S, Cout, 2)"
            part = pbuf[GUARD:GUARD + n].view(c.B, S.value, c.Cout, 2)
            assert bool(torch.isfinite(part).all()), "a (tile, channel) partial was not written"
        else:
            fn = lib.sfmi_conv3d_up2_cl_f32 if c.subpixel else lib.sfmi_conv3d_cl_f32
            L.check(fn(*args, L.stream_ptr()), "conv")
            torch.cuda.synchronize()
        _check_out(ybuf, y, c.name)
        return (y, part) if stats else y

    def ratio(self, y, form):
        """|y - y64| / bound per element (the bound of the instance `form` names)."""
        c = self.c
        bound = R.conv_bound(self.p, R.chain_depth(form.instance, c.Cin, 2 if c.subpixel else c.KS), self.bias, c.act, c.subpixel)
        assert bool(torch.isfinite(y).all()), f"{c.name}: non-finite output (a read outside a tensor reached the result)"
        return (y.double() - self.p["y"]).abs() / bound


def _parities(r):
    B, D, H, W, C = r.shape
    return r.view(B, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(2, 4, 6, 0, 1, 3, 5, 7).reshape(8, -1).max(1).values.tolist()


def test_case_table_reaches_every_instance():
    seen = {f.instance for c in CASES for k, f in c.forms().items() if f is not None and k in c.knobs()}
    assert sorted(seen) == R.CONV_INSTANCES, sorted(set(R.CONV_INSTANCES) - seen)


def test_conv_instances_against_float64(dev):
    """Every CASES row at every knob that changes its instance: |y - y64| <= bound element by element, bands untouched, no sentinel left,
    output finite; the statistics partials within [ST] of float64 sums of the written y, and that y bit-identical to the plain launch.
    Failures are collected so that the report always names every instance."""
    worst, fails, t0 = {}, [], time.time()
    for i, c in enumerate(CASES):
        cv = _Conv(c, dev, 100 + i)
        forms = c.forms()
        for knob in c.knobs():
            f = forms[knob]
            with _knob(knob):
                try:
                    if c.stats:
                        y, part = cv.launch(stats=True)
                        assert part.shape[1] == (8 if c.subpixel else 1) * (f.Do * f.Ho * f.Wo // f.M_T), (part.shape, f)
                        ref = R.tile_sums_ref(y, f.M_T, c.subpixel)
                        es, bs = (part - ref[..., :2]).abs(), R.tile_sums_bound(ref, f.instance[5])    # (a channel the ReLU zeroed: 0 <= 0)
                        rs = float((es / bs.clamp_min(1e-300)).max())
                        print(f"[ratio] stats {f.instance} {c.name}: {rs:.3g}")
                        assert bool((es <= bs).all()), f"{c.name}: statistics partials off by {rs:.3g} of their bound"
                        c2 = Case(**dict(c.__dict__, stats=False))
                        assert c2.forms()[knob].instance[:6] == f.instance[:6]
                        assert torch.equal(cv.launch(), y), f"{c.name}: the statistics launch wrote another y than the plain one"
                    else:
                        y = cv.launch()
                    r = cv.ratio(y, f)
                    rmax = float(r.max())
                    extra = ""
                    if c.subpixel:
                        extra = "  parities " + " ".join(f"{v:.3f}" for v in _parities(r))
                    print(f"[ratio] conv {f.instance} knob {knob} {c.name} (tiles {f.voxel_tiles} x {c.Cout // f.N_T}, straddle {int(f.straddle)}, "
                          f"partial {int(f.partial)}, n {f.n}): {rmax:.3g}{extra}")
                    worst[f.instance] = max(worst.get(f.instance, 0.0), rmax)
                    assert rmax <= 1.0, f"{c.name} knob {knob} {f.instance}: error {rmax:.3g} of the bound on {int((r > 1).sum())} elements"
                except AssertionError as e:
                    fails.append(str(e))
        del cv
    print(f"[time] conv case table {time.time() - t0:.1f} s")
    for inst in R.CONV_INSTANCES:
        print(f"[report] instance {inst}: largest error / bound {worst.get(inst, float('nan')):.3g}")
    assert not fails, "\n".join(fails)
    assert sorted(worst) == R.CONV_INSTANCES and max(worst.values()) < 1.0


def test_unet3d_accumulation_rms_gate(dev):
    """DESIGN.md's blocked-accumulation claim.  For every UNet3D layer shape (taps * Cin >= 3456), e = rms(y - y64) / rms(y64) of
    (a) torch CPU fp32 conv3d on the same f32 inputs (how the reference computes the layer), (b) the default form (conv_xreuse 2: ACC2),
    (c) the per-tap form (conv_xreuse 0: one un-blocked chain), on the boundary shell and on the interior of the grid separately.
    Gate: (b) <= RMS_GATE_M (a) on both; and the un-blocked form must FAIL that gate at K = 20736 - the proof that it sees a lost fold."""
    fails, seen_k = [], set()
    for i, (ci, co, d) in enumerate(unet3d_layers()):
        assert 27 * ci >= 3456
        c = Case(f"unet {ci}->{co} @{d}", 1, (d, d, d), ci, co, bias=False)
        cv = _Conv(c, dev, 500 + i)
        forms = c.forms()
        assert forms[2].instance == R.ACC2_INSTANCE and forms[0].instance == (2, 2, 2, 0, 0, 2, 0)
        y64 = cv.p["y"]
        xin = (cv.x.cpu() * cv.sc.cpu().view(1, 1, 1, 1, ci) + cv.sh.cpu().view(1, 1, 1, 1, ci)).permute(0, 4, 1, 2, 3).contiguous()
        w5 = cv.w.cpu().view(27, co, ci).permute(1, 2, 0).reshape(co, ci, 3, 3, 3).contiguous()
        ya = F.relu(F.conv3d(xin, w5, None, padding=1)).permute(0, 2, 3, 4, 1).to(dev)
        ys = {}
        for knob in (2, 0):
            with _knob(knob):
                ys[knob] = cv.launch()
        shell = R.boundary_mask(d, d, d, dev)[None].expand(1, d, d, d)
        for region, mask in (("shell", shell), ("interior", ~shell)):
            ea, eb, ec = (R.rel_rms(y, y64, mask) for y in (ya, ys[2], ys[0]))
            print(f"[rms] unet {ci}->{co} @{d} K={27 * ci} {region}: torch-cpu {ea:.3g}  ACC2 {eb:.3g} ({eb / ea:.2f} x)  per-tap {ec:.3g} ({ec / ea:.2f} x)")
            if eb > RMS_GATE_M * ea:
                fails.append(f"{c.name} {region}: ACC2 rms {eb:.3g} > {RMS_GATE_M} x torch-cpu {ea:.3g}")
            if 27 * ci == 20736:
                seen_k.add(region)
                if not ec > RMS_GATE_M * ea:
                    fails.append(f"{c.name} {region}: the un-blocked chain passes the gate ({ec:.3g} vs {ea:.3g}): the gate cannot see a lost fold")
        del cv
    assert seen_k == {"shell", "interior"}
    assert not fails, "\n".join(fails)


GN_CASES = [(V, C, G, 0.5) for V in (125, 515, 4099, 32771) for C, G in ((4, 1), (24, 8), (1024, 64))] + \
    [(515, 24, 1, 0.5), (515, 1024, 8, 0.5), (4099, 24, 8, 100.0), (32771, 24, 8, 100.0)]


def test_groupnorm_coefficients_against_float64(dev):
    """sfmi_groupnorm_coeffs_f32 at V that make 1 / 4 / 16 / 64 splits (V no multiple of the split count), C 4 .. 1024, 1 .. 64 groups
    and inputs whose mean is 100 x their standard deviation: the f64 partials against float64 sums, scale / shift within [GN]."""
    L = _L()
    lib = L.lib()
    worst = 0.0
    for i, (V, C, G, mean) in enumerate(GN_CASES):
        g = torch.Generator().manual_seed(900 + i)
        B, S = 2, int(lib.sfmi_gn_splits(V))
        assert S == R.gn_splits(V) and V % S != 0 or S == 1
        xb, x = _banded(torch.randn(B, V, C, generator=g) + mean, dev)
        gb, gam = _banded(torch.rand(C, generator=g) + 0.5, dev)
        bb, bet = _banded(torch.randn(C, generator=g), dev)
        sbuf, sc = _sentinel_out((B, C), dev)
        tbuf, sh = _sentinel_out((B, C), dev)
        pbuf = torch.full((B * S * C * 2 + 2 * GUARD,), float("nan"), dtype=torch.float64, device=dev)
        L.check(lib.sfmi_groupnorm_coeffs_f32(L.ptr(x), L.ptr(gam), L.ptr(bet), L.ptr(sc), L.ptr(sh), pbuf[GUARD:].data_ptr(), B, V, C, G, 1e-5,
                                              L.stream_ptr()), "groupnorm_coeffs")
        torch.cuda.synchronize()
        _check_out(sbuf, sc, "scale")
        _check_out(tbuf, sh, "shift")
        n = B * S * C * 2
        assert bool(pbuf[:GUARD].isnan().all()) and bool(pbuf[GUARD + n:].isnan().all())
        part = pbuf[GUARD:GUARD + n].view(B, S, C, 2).sum(1)
        sums = R.chan_sums_ref(x)
        x64 = x.double()
        tol = R.gamma64(-(-V // S) + 256 + S + 8) * torch.stack([x64.abs().sum(1), (x64 * x64).sum(1)], -1)
        rp = float(((part - sums).abs() / tol).max())
        s64, t64_, ds, dt = R.groupnorm_coeffs_ref(x, gam, bet, G, 1e-5, S)
        r1, r2 = float(((sc.double() - s64).abs() / ds).max()), float(((sh.double() - t64_).abs() / dt).max())
        print(f"[ratio] groupnorm V {V} (S {S}) C {C} groups {G} mean {mean}: partials {rp:.3g} scale {r1:.3g} shift {r2:.3g}")
        worst = max(worst, rp, r1, r2)
        assert rp <= 1.0 and r1 <= 1.0 and r2 <= 1.0, (V, C, G, mean, rp, r1, r2)
    print(f"[report] groupnorm: largest error / bound {worst:.3g}")


GEMM_MS, GEMM_NS, GEMM_KS = (1, 255, 256, 257, 700, 4097), (32, 96, 64, 192, 128, 384), (16, 1024)


def _gemm_cases():
    out, i = [], 0
    for K in GEMM_KS:
        for M in GEMM_MS:
            for N in GEMM_NS:
                out.append((M, N, K, i % 3, (i // 3) % 2 == 0, (i // 2) % 2 == 1, False, 0, 0))
                i += 1
    # output-row remap with gaps (gpt.py: prefill rows of a (B, P) rectangle), every activation, with and without the residual
    out += [(700, 96, 1024, 2, True, True, False, 100, 130), (257, 128, 16, 1, True, False, False, 64, 65),
            (4097, 64, 1024, 0, False, True, False, 1000, 1024), (256, 384, 1024, 0, True, True, False, 1, 3)]
    # the residual IS the output buffer (gpt.py prefill: proj / fc2 accumulate into the residual stream in place), with and without a remap
    out += [(700, 128, 1024, 0, True, True, True, 0, 0), (257, 96, 16, 2, True, True, True, 0, 0), (700, 192, 1024, 0, True, True, True, 100, 130)]
    return out


def test_gemm_against_float64(dev):
    """sfmi_gemm_f32: M around the tile sizes, every channel tiling, K 16 and 1024, act 0 / 1 / 2 x bias x residual (every combination
    occurs), the residual aliasing the output, and the out_group / out_group_stride remap: mapped rows within the bound, the gap rows and the bands keep their sentinel."""
    L = _L()
    lib = L.lib()
    cases = _gemm_cases()
    assert {(a, b, r) for _, _, _, a, b, r, _, _, _ in cases} == {(a, b, r) for a in (0, 1, 2) for b in (False, True) for r in (False, True)}
    worst = {}
    for i, (M, N, K, act, use_bias, use_res, alias, og, ogs) in enumerate(cases):
        g = torch.Generator().manual_seed(1300 + i)
        rows_out = M if not og else int(R.remap_rows(M, og, ogs)[-1]) + 1
        xb, x = _banded(torch.randn(M, K, generator=g), dev)
        wb, W = _banded(torch.randn(N, K, generator=g) / math.sqrt(K), dev)
        bias = _banded(torch.randn(N, generator=g), dev) if use_bias else (None, None)
        resid = _banded(torch.randn(rows_out, N, generator=g), dev) if use_res else (None, None)
        rows, y64, pre, P, r = R.gemm_ref(x, W, bias[1], act, resid[1], og, ogs)
        bound = R.gemm_bound(pre, P, K, use_bias, act, r)
        for knob in (2, 0) if N % 128 == 0 else (2,):
            f = R.gemm_form(M, N, K, knob, og, ogs)
            ybuf, y = _sentinel_out((rows_out, N), dev)
            if alias:
                y[rows.to(dev)] = resid[1][rows.to(dev)]
            with _knob(knob):
                L.check(lib.sfmi_gemm_f32(L.ptr(x), L.ptr(W), L.ptr(bias[1]), L.ptr(y if alias else resid[1]), L.ptr(y), M, N, K, act, og, ogs,
                                          L.stream_ptr()), "gemm")
                torch.cuda.synchronize()
            bits = ybuf.view(torch.int32)
            assert bool((bits[:GUARD] == SENT).all()) and bool((bits[GUARD + y.numel():] == SENT).all()), "wrote outside y"
            yc = y.cpu()
            written = torch.zeros(rows_out, dtype=torch.bool)
            written[rows] = True
            assert bool((yc[~written].view(torch.int32) == SENT).all()), "a gap row of the remap was written"
            got = yc[rows]
            assert bool(torch.isfinite(got).all())
            ratio = float(((got.double() - y64).abs() / bound).max())
            worst[f.instance] = max(worst.get(f.instance, 0.0), ratio)
            assert ratio <= 1.0, (M, N, K, act, use_bias, use_res, alias, og, ogs, knob, ratio)
    for inst, v in sorted(worst.items()):
        print(f"[report] gemm instance {inst}: largest error / bound {v:.3g}")
