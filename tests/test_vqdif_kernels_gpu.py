"""The VQDIF point path - csrc/encoder.hip (enc_* kernels, fused and staged), csrc/vq_argmin.hip and the value forms of
csrc/sdf_query.hip - against float64 (tests/vqdif_ref.py: references, float32 mirrors of the discrete decisions, a mirror of the fused
kernel's ownership rule, and derived per-element error bounds).

* Encoder through sfmi_encode_points_f32 / _down_f32 / _tap_f32 at enc_fused = 1 and 0 over ENC_CASES: T = 1, 31, 3 x 33 (tiles that
  straddle shapes), cells of exactly 1 / 31 / 32 / 33 / 64 / 65 / 128 points, a batch whose middle shape alone is declined by the fused
  kernel (cells of 129 and 300 points), the ownership rule's limits (n = 511 of EF_CAP, a cell starting at sorted position 255 / 256, a
  last workgroup with n = 0), points on cell faces and outside the box at R = 16 and 32, and a second point order of the same cloud.
  Cell ids and mask equal the mirror; the mean grid, the first Downsampler convolution and the per-point taps (EVERY point) are within
  their bounds; empty cells / parents are exactly +0.0; fused == staged bit for bit.
* vq_argmin_kernel<64 / 128> with dmin_out at K = 32 / 64 / 4096 and N = 1 .. 300 (ragged last waves, waves whose rows 32..63 all lie
  past N), the documented tie rule on bit-identical duplicate codes without any allowance, vq_gather_kernel bit-exact.
* sdf_query_kernel's point, lattice (plain / affine / slab) and keyed forms at G = 2, 3, 16, 64, with and without the sigmoid, at the
  default grid and with sdf_blocks = 1 (one workgroup walks every tile: bit-identical); sigmoid_kernel's scalar tail and in-place use.

Every output sits between 0x5A5A5A5A bands, every input between NaN bands, every launch is made twice and must repeat bit for bit,
every comparison prints `[ratio] name err/bound` (pytest -s).  The from-scratch bounds follow the float64 network's own linearisation
(vqdif_ref.py [JAC]; five blocks deep they stand at 1e-3); the ANCHORED comparisons feed one layer with the kernel's own taps and are
gated at that layer's rounding alone.  Measured on one MI355X (largest error / bound; DESIGN.md has the table): encoder from scratch
- stage 1 0.0052, stage 4 0.0017, c 0.0012, mean 0.0012, down0 0.0003; anchored - c 0.098, mean 0.997 (the bound IS the final f32
rounding), down0 0.014; VQ dmin 0.064, chosen code against the float64 minimum 0.000; decoder logits 0.0072, with the affine 0.0061,
sigmoid 0.0072; sigmoid_kernel 0.43.  The file runs in 10 s (37 tests).
Finding: case 3 (B = 3, T = 33) faulted in the staged form - with B * T odd the workspace's 64-bit per-cell sums sat 4 bytes off an
8-byte boundary and the first atomic on them was an illegal access; fixed in enc_pipeline (csrc/encoder.hip), the case stays."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import vqdif_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
BAND = 4096                # bytes (outputs) / elements (inputs) on either side of every buffer
PAT = 0x5A


# ---------------------------------------------------------------------------------------------------- encoder case table
class EncCase:
    """shapes: per shape a list of (cell id, point count) for R.build_cloud, or an (T,3) array; expect: what the case is built to reach,
    asserted through R.fused_ownership / R.fused_declines by check_reach (CPU test and GPU test alike)."""

    def __init__(self, name, shapes, R_=16, seed=0, shuffle_seed=None, **expect):
        self.name, self.shapes, self.R, self.seed, self.shuffle_seed, self.expect = name, shapes, R_, seed, shuffle_seed, expect

    def cloud(self):
        out = [s if isinstance(s, np.ndarray) else R.build_cloud(s, 1000 * self.seed + 17 * b, self.shuffle_seed) for b, s in enumerate(self.shapes)]
        return np.ascontiguousarray(np.stack(out))

    def check_reach(self, cell):
        """cell (B,T) from the mirror -> per shape (declined, ownership); asserts the limits the case names."""
        B, T = cell.shape
        info = []
        for b in range(B):
            sc = np.sort(cell[b])
            info.append((R.fused_declines(sc), R.fused_ownership(sc, T)))
        e = self.expect
        if "declined" in e:
            assert [d for d, _ in info] == e["declined"], (self.name, [d for d, _ in info])
        if "straddle" in e:
            assert all((T * (b + 1)) % 32 != 0 for b in range(B - 1)), self.name
        for b, own in e.get("own", {}).items():
            assert not info[b][0], (self.name, "a declined shape has no fused ownership")
            assert info[b][1] == own, (self.name, b, info[b][1])
        for b, pos in e.get("starts", {}).items():                   # a cell's first sorted position
            sc = np.sort(cell[b])
            st, _ = R.runs_of(sc)
            assert pos in set(st.tolist()) and (pos == 0 or sc[pos] != sc[pos - 1]), (self.name, b, pos)
        for b, sizes in e.get("sizes", {}).items():
            _, n = np.unique(cell[b], return_counts=True)
            assert set(sizes) <= set(n.tolist()), (self.name, sorted(set(n.tolist())))
        return info


def _sized_cells(sizes, first=20000, gap=3):
    """cells of the given sizes in ascending cell order, `gap` single-point cells before, between and after them"""
    out, c = [], first
    for n in list(sizes) + [None]:
        out += R.singles(c, gap, 5)
        c += 5 * gap
        if n is not None:
            out.append((c, n))
            c += 5
    return out


def _enc_cases():
    S = R.singles
    cap, limit, nom = R.EF_CAP, R.EF_LIMIT, R.EF_NOM
    c = [EncCase("1: B1 T1", [[(133000, 1)]], seed=1, own={0: [(0, 1)]}),
         EncCase("2: B1 T31", [S(9000, 20) + [(70000, 11)]], seed=2, own={0: [(0, 31)]}),
         EncCase("3: B3 T33", [S(4000, 33, 11), [(150000, 33)], [(777, 16), (200000, 17)]], seed=3, straddle=True, sizes={1: [33], 2: [16, 17]}),
         EncCase("4: cells of 1 31 32 33 64 65 128", [_sized_cells([1, 31, 32, 33, 64, 65, 128])], seed=4, declined=[False],
                 sizes={0: [1, 31, 32, 33, 64, 65, 128]}),
         # T = 500: 500 % 32 = 20 and 1000 % 32 = 8, so a 32-point tile straddles shapes 0 / 1 and 1 / 2
         EncCase("5: middle shape declined (129, 300)", [_sized_cells([100, 128, 60], gap=53), S(100, 30) + [(90000, 129), (90009, 300)] + S(180000, 41),
                                                        S(50, 372) + [(250000, 128)]], seed=5, declined=[False, True, False], straddle=True,
                 sizes={1: [129, 300]}),
         # 383 single-point cells, a cell of EF_LIMIT points at sorted position 383, the rest: workgroup 0 finishes the straddling run
         # (n = EF_NOM + EF_LIMIT - 1 = EF_CAP - 1), workgroup 1 skips its tail
         EncCase("6a: n = 511", [S(100, nom - 1) + [(100000, limit)] + S(150000, 200)], seed=6, declined=[False],
                 own={0: [(0, cap - 1), (cap - 1, nom + limit + 199)]}),
         EncCase("6b: cells starting at 255 / 256", [S(100, cap // 2 - 1) + [(100000, 5)] + S(150000, 140), S(100, cap // 2) + [(100000, 5)] + S(150000, 139)],
                 seed=7, declined=[False, False], starts={0: cap // 2 - 1, 1: cap // 2}),
         # T = EF_NOM + 10 with a 20-point cell over positions EF_NOM - 10 .. EF_NOM + 9: the second workgroup's range is empty
         EncCase("6c: last workgroup n = 0", [S(100, nom - 10) + [(200000, 20)]], seed=8, declined=[False], own={0: [(0, nom + 10), (nom + 10, nom + 10)]}),
         EncCase("7: faces and outside, R16", [R.face_cloud(600, 70), R.face_cloud(600, 71)], R_=16),
         EncCase("7: faces and outside, R32", [R.face_cloud(600, 70), R.face_cloud(600, 71)], R_=32),
         EncCase("8: case 4, second order", [_sized_cells([1, 31, 32, 33, 64, 65, 128])], seed=4, shuffle_seed=99, declined=[False])]
    return c


ENC_CASES = _enc_cases()


# ---------------------------------------------------------------------------------------------------- buffers
def _L():
    from shapeformer_amd import _lib as L
    return L


@contextlib.contextmanager
def _tune(name, value):
    """a libsfmi knob for the duration, restored in a finally"""
    L = _L()
    lib = L.lib()
    old = int(lib.sfmi_tune_get(name))
    try:
        L.check(lib.sfmi_tune_set(name, int(value)), "tune")
        yield
    finally:
        L.check(lib.sfmi_tune_set(name, old), "tune")


def _banded(t, dev):
    """an input on the device between two bands of NaN (float) / of the pattern (integer); returns the view (the buffer lives with it)"""
    t = torch.as_tensor(t)
    n = t.numel()
    if t.dtype.is_floating_point:
        buf = torch.full((n + 2 * BAND,), float("nan"), dtype=t.dtype, device=dev)
    else:
        buf = torch.full((n + 2 * BAND,), 0x5A5A5A5A, dtype=t.dtype, device=dev)
    buf[BAND:BAND + n] = t.reshape(-1).to(dev)
    return buf[BAND:BAND + n].view(t.shape)


class _Out:
    """an output of `shape` / `dtype` between two BAND-byte bands, everything pre-filled with 0x5A bytes"""

    def __init__(self, shape, dtype, dev):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((self.nbytes + 2 * BAND,), PAT, dtype=torch.uint8, device=dev)
        self.t = self.buf[BAND:BAND + self.nbytes].view(dtype).view(shape)

    def check(self, what, written=True):
        assert bool((self.buf[:BAND] == PAT).all()) and bool((self.buf[BAND + self.nbytes:] == PAT).all()), f"{what}: wrote outside its output"
        if written and self.nbytes % 4 == 0:
            w = self.buf[BAND:BAND + self.nbytes].view(torch.int32)
            assert not bool((w == 0x5A5A5A5A).any()), f"{what}: left part of its output unwritten"
        return self.t


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratio(name, got, ref, bound, worst=None):
    got = torch.as_tensor(got).detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    r = float(((got - ref).abs() / bound).max()) if got.numel() else 0.0
    print(f"[ratio] {name} {r:.4f}")
    if worst is not None:
        key = name.split(" | ")[0]
        worst[key] = max(worst.get(key, 0.0), r)
    return r


# ---------------------------------------------------------------------------------------------------- encoder
class _Enc:
    def __init__(self, sd, dev):
        L = _L()
        lib = L.lib()
        g = lambda k: np.ascontiguousarray(np.asarray(sd["encoder." + k], np.float32))              # noqa: E731
        cat = lambda fmt: np.ascontiguousarray(np.stack([g(fmt.format(i)) for i in range(5)]))       # noqa: E731
        enc = np.empty(lib.sfmi_enc_pack_floats(), np.float32)
        a = [g("fc_pos.weight"), g("fc_pos.bias"), cat("blocks.{}.fc_0.weight"), cat("blocks.{}.fc_0.bias"), cat("blocks.{}.fc_1.weight"),
             cat("blocks.{}.fc_1.bias"), cat("blocks.{}.shortcut.weight"), g("fc_c.weight"), g("fc_c.bias"), enc]
        L.check(lib.sfmi_enc_pack_weights(*[x.ctypes.data for x in a]), "sfmi_enc_pack_weights")
        w = g("downsampler.blocks.0.conv.weight")
        assert w.shape == (64, 32, 2, 2, 2)
        wp = np.empty(w.size, np.float32)
        L.check(lib.sfmi_conv_pack_weight(w.ctypes.data, 64, 32, 2, wp.ctypes.data), "conv_pack")
        self.dev, self.enc_w, self.w_down = dev, _banded(enc, dev), _banded(wp, dev)

    def launch(self, cloud, R_, entry, knob):
        """one launch -> dict of checked outputs"""
        L = _L()
        lib, dev = L.lib(), self.dev
        B, T, _ = cloud.shape
        G, H = R.ENC_G, R.ENC_G // 2
        ws = torch.full((lib.sfmi_enc_workspace_bytes(B, T),), PAT, dtype=torch.uint8, device=dev)
        o = {"mask": _Out((B, R_, R_, R_), torch.uint8, dev), "cell": _Out((B, T), torch.int32, dev)}
        with _tune(b"enc_fused", knob):
            if entry == "down":
                o["down"] = _Out((B, H, H, H, 64), torch.float32, dev)
                rc = lib.sfmi_encode_points_down_f32(L.ptr(cloud), L.ptr(self.enc_w), L.ptr(self.w_down), L.ptr(o["down"].t), L.ptr(o["mask"].t),
                                                     L.ptr(o["cell"].t), L.ptr(ws), B, T, R_, 1, L.stream_ptr())
            else:
                o["grid"] = _Out((B, G, G, G, 32), torch.float32, dev)
                if entry == "tap":
                    o["s1"], o["s4c"] = _Out((B, T, 32), torch.float32, dev), _Out((B, T, 64), torch.float32, dev)
                    rc = lib.sfmi_encode_points_tap_f32(L.ptr(cloud), L.ptr(self.enc_w), L.ptr(o["grid"].t), L.ptr(o["mask"].t), L.ptr(o["cell"].t),
                                                        L.ptr(ws), B, T, R_, L.ptr(o["s1"].t), L.ptr(o["s4c"].t), L.stream_ptr())
                else:
                    rc = lib.sfmi_encode_points_f32(L.ptr(cloud), L.ptr(self.enc_w), L.ptr(o["grid"].t), L.ptr(o["mask"].t), L.ptr(o["cell"].t),
                                                    L.ptr(ws), B, T, R_, L.stream_ptr())
            L.check(rc, "encode " + entry)
            torch.cuda.synchronize()
        return {k: v.check(f"{entry} {k}") for k, v in o.items()}


@pytest.fixture(scope="module")
def enc(vq16_sd, dev):
    return _Enc(vq16_sd, dev)


_ENC_REF = {}


def _enc_ref(sd, case, dev):
    if case.name not in _ENC_REF:
        cloud = case.cloud()
        _ENC_REF[case.name] = (cloud, R.encoder_ref(sd, cloud, case.R, device=dev))
    return _ENC_REF[case.name]


def _check_encoder_outputs(name, o, ref, dev, worst):
    B, T = ref.cell.shape
    assert np.array_equal(o["cell"].cpu().numpy(), ref.cell), f"{name}: cell ids differ from the float32 mirror"
    assert np.array_equal(o["mask"].cpu().numpy().astype(bool), ref.mask), f"{name}: mask differs from the float32 mirror"
    assert int(o["mask"].max()) <= 1
    if "grid" in o:
        g = o["grid"].view(B, -1, 32)
        ob, oc = ref.occ[:, 0].to(dev), ref.occ[:, 1].to(dev)
        assert _ratio(f"enc mean | {name}", g[ob, oc], ref.mean, ref.e_mean, worst) <= 1.0, name
        nz = (_bits(g) != 0).any(-1)
        nz[ob, oc] = False
        assert not bool(nz.any()), f"{name}: a cell without points is not exactly +0.0"
    if "down" in o:
        y = o["down"]
        idx = tuple(ref.par.to(dev).T)
        assert _ratio(f"enc down0 | {name}", y[idx], ref.down, ref.e_down, worst) <= 1.0, name
        nz = (_bits(y).view(y.shape) != 0).any(-1)
        nz[idx] = False
        assert not bool(nz.any()), f"{name}: a parent without points is not exactly +0.0"
    if "s1" in o:
        assert _ratio(f"enc stage1 | {name}", o["s1"], ref.stages[1], ref.e_stages[1], worst) <= 1.0, name
        assert _ratio(f"enc stage4 | {name}", o["s4c"][..., :32], ref.stages[4], ref.e_stages[4], worst) <= 1.0, name
        assert _ratio(f"enc c | {name}", o["s4c"][..., 32:], ref.c, ref.e_c, worst) <= 1.0, name


@pytest.mark.parametrize("case", ENC_CASES, ids=[c.name for c in ENC_CASES])
def test_encoder_against_float64(dev, vq16_sd, enc, case):
    cloud_np, ref = _enc_ref(vq16_sd, case, dev)
    case.check_reach(ref.cell)
    cloud = _banded(cloud_np, dev)
    worst, keep = {}, {}
    for entry in ("points", "down", "tap"):
        outs = {}
        for knob in (1, 0):
            a = enc.launch(cloud, case.R, entry, knob)
            b = enc.launch(cloud, case.R, entry, knob)
            for k in a:
                assert _same(a[k], b[k]), f"{case.name}: {entry} {k} differs between two launches (enc_fused = {knob})"
            _check_encoder_outputs(f"{case.name} {entry} fused{knob}", a, ref, dev, worst)
            outs[knob] = a
        for k in outs[1]:
            assert _same(outs[1][k], outs[0][k]), f"{case.name}: {entry} {k}: fused and staged forms differ"
        keep[entry] = outs[1]
    # anchored: the kernels' own taps as the inputs of one layer each (R.anchored_ref) - gates at the f32 noise itself
    assert _same(keep["points"]["grid"], keep["tap"]["grid"]), "the taps disturb the mean grid"
    B = cloud_np.shape[0]
    anc = R.anchored_ref(vq16_sd, ref.cell, keep["tap"]["s4c"].cpu())
    assert _ratio(f"enc c anchored | {case.name}", keep["tap"]["s4c"][..., 32:], anc.c_from_net, anc.e_c_from_net, worst) <= 1.0
    assert torch.equal(anc.occ, ref.occ) and torch.equal(anc.par, ref.par)
    g = keep["points"]["grid"].view(B, -1, 32)[ref.occ[:, 0].to(dev), ref.occ[:, 1].to(dev)]
    assert _ratio(f"enc mean anchored | {case.name}", g, anc.mean, anc.e_mean, worst) <= 1.0
    assert _ratio(f"enc down0 anchored | {case.name}", keep["down"]["down"][tuple(ref.par.to(dev).T)], anc.down, anc.e_down, worst) <= 1.0
    print("[worst]", case.name, {k: round(v, 4) for k, v in worst.items()})


def test_encoder_result_does_not_depend_on_the_point_order(dev, vq16_sd, enc):
    """Case 4 and the same points in another order (case 8): mean grid, mask and first Downsampler output bit for bit."""
    c4, c8 = [c for c in ENC_CASES if c.name.startswith("4:")][0], [c for c in ENC_CASES if c.name.startswith("8:")][0]
    a, b = c4.cloud(), c8.cloud()
    assert a.shape == b.shape and not np.array_equal(a, b)
    assert np.array_equal(np.sort(a.view([("", a.dtype)] * 3).ravel()), np.sort(b.view([("", b.dtype)] * 3).ravel())), "not the same points"
    for knob in (1, 0):
        for entry, key in (("points", "grid"), ("down", "down")):
            oa, ob = enc.launch(_banded(a, dev), 16, entry, knob), enc.launch(_banded(b, dev), 16, entry, knob)
            assert _same(oa[key], ob[key]) and _same(oa["mask"], ob["mask"]), (entry, knob)
            assert not _same(oa["cell"], ob["cell"])


# ---------------------------------------------------------------------------------------------------- VQ
VQ_NS = (1, 31, 33, 64, 65, 300)


def _vq_launch(W, x, dev):
    """pack + argmin (with dmin_out) + gather, each launched twice -> idx (N) int64 cpu, dmin (N) f64 cpu"""
    L = _L()
    lib = L.lib()
    K, D = W.shape
    N = x.shape[0]
    pk = np.empty(lib.sfmi_vq_pack_floats(K, D), np.float32)
    L.check(lib.sfmi_vq_pack_codebook(np.ascontiguousarray(W).ctypes.data, K, D, pk.ctypes.data), "vq_pack")
    pkd, xd, Wd = _banded(pk, dev), _banded(x, dev), _banded(W, dev)
    res = []
    for _ in range(2):
        idx, dmin = _Out((N,), torch.int32, dev), _Out((N,), torch.float32, dev)
        L.check(lib.sfmi_vq_argmin_f32(L.ptr(xd), L.ptr(pkd), L.ptr(idx.t), L.ptr(dmin.t), N, K, D, L.stream_ptr()), "vq_argmin")
        torch.cuda.synchronize()
        i2 = _Out((N,), torch.int32, dev)                 # dmin_out is optional: the same indices without it
        L.check(lib.sfmi_vq_argmin_f32(L.ptr(xd), L.ptr(pkd), L.ptr(i2.t), None, N, K, D, L.stream_ptr()), "vq_argmin")
        code = _Out((N, D), torch.float32, dev)
        L.check(lib.sfmi_vq_gather_f32(L.ptr(Wd), L.ptr(idx.t), L.ptr(code.t), N, D, L.stream_ptr()), "vq_gather")
        torch.cuda.synchronize()
        res.append((idx.check("vq idx"), dmin.check("vq dmin"), i2.check("vq idx (no dmin)"), code.check("vq gather")))
    for a, b in zip(*res):
        assert _same(a, b), "two launches differ"
    idx, dmin, i2, code = res[0]
    assert _same(idx, i2)
    assert bool((idx >= 0).all()) and bool((idx < K).all())
    assert _same(code, Wd[idx.long()]), "vq_gather is not W[idx] bit for bit"
    return idx.long().cpu(), dmin.double().cpu()


def _vq_value_checks(name, x, W, idx, dmin, worst, same=()):
    d, e = R.vq_ref(x, W, same)
    r = torch.arange(len(idx))
    r1 = _ratio(f"vq dmin | {name}", dmin, d[r, idx], e[r, idx], worst)
    m = torch.argmin(d, 1)
    # the kernel's computed d(idx) <= its computed d(m): d(idx) - e(idx) <= d(m) + e(m)
    r2 = _ratio(f"vq min | {name}", d[r, idx], d[r, m], e[r, idx] + e[r, m], worst)
    assert r1 <= 1.0 and r2 <= 1.0, name
    return d


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("K", [32, 64, 4096])
def test_vq_argmin_against_float64(dev, D, K):
    worst = {}
    for N in VQ_NS:
        g = torch.Generator().manual_seed(1000 * D + K + N)
        W = (torch.randn(K, D, generator=g) * 0.5).numpy()
        x = (torch.randn(N, D, generator=g) * 0.5).numpy()
        idx, dmin = _vq_launch(W, x, dev)
        _vq_value_checks(f"D{D} K{K} N{N}", x, W, idx, dmin, worst)
    print("[worst]", f"vq D{D} K{K}", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("K", [32, 64, 4096])
def test_vq_tie_rule_lowest_index(dev, D, K):
    """Bit-identical duplicate codes (4, 8) [the lower index in the upper half-wave], (3, 35) [different tiles], (0, K - 1): the rows
    nearest to a duplicated code must get the LOWER index, exactly - no allowance, no cap on mismatches."""
    W, pairs = R.tie_codebook(K, D, 7 * D + K)
    for N in VQ_NS:
        g = torch.Generator().manual_seed(D + K + N)
        target = torch.arange(N) % len(pairs)
        lo = torch.tensor([p[0] for p in pairs])[target]
        x = (torch.from_numpy(W)[lo] + 0.01 * torch.randn(N, D, generator=g)).numpy()
        idx, dmin = _vq_launch(W, x, dev)
        d = _vq_value_checks(f"ties D{D} K{K} N{N}", x, W, idx, dmin, {}, pairs)
        want = R.vq_argmin_ref(d)
        assert torch.equal(want, lo), "the test's own rows are not nearest to their duplicated code"
        hi = torch.tensor([p[1] for p in pairs])[target]
        assert torch.equal(d[torch.arange(N), lo], d[torch.arange(N), hi])
        assert torch.equal(idx, want), (D, K, N, torch.nonzero(idx != want).flatten().tolist()[:8], idx[idx != want][:8].tolist())


# ---------------------------------------------------------------------------------------------------- decoder query
SDF_NS = (1, 31, 32, 33, 1000)
_GRIDS = {}


def _grid(G, dev):
    """(3,32,G,G,G) f32 feature grid (cpu) and its banded channels-last device copy, once per G"""
    if G not in _GRIDS:
        grid = torch.randn(3, 32, G, G, G, generator=torch.Generator().manual_seed(40 + G))
        _GRIDS[G] = (grid, _banded(grid.permute(0, 2, 3, 4, 1).contiguous(), dev))
    return _GRIDS[G]


def _point_launches(ops, xyz, grid_cl, wp, dev):
    B, N, _ = xyz.shape
    out = {}
    for sig in (False, True):
        o = _Out((B, N, 1), torch.float32, dev)
        ops.sdf_query(xyz, grid_cl, wp, sigmoid=sig, out=o.t)
        torch.cuda.synchronize()
        out["sigmoid" if sig else "logit"] = o.check("sdf_query")[..., 0]
    return out


def _lattice_launches(ops, axis, grid_cl, wp, aff, slab, keys, koff, dev):
    L = _L()
    B, G, Q = grid_cl.shape[0], grid_cl.shape[1], axis.numel()
    out = {}
    for name, kw, n in (("grid", {}, Q ** 3), ("grid sigmoid", dict(sigmoid=True), Q ** 3), ("affine", dict(affine=aff), Q ** 3),
                        ("slab", dict(x_range=slab), (slab[1] - slab[0]) * Q * Q), ("affine slab", dict(affine=aff, x_range=slab), (slab[1] - slab[0]) * Q * Q)):
        o = _Out((B, n, 1), torch.float32, dev)
        ops.sdf_query_grid(axis, grid_cl, wp, out=o.t, **kw)
        torch.cuda.synchronize()
        out[name] = o.check("sdf_query_grid " + name)[..., 0]
    for sig in (False, True):
        o = _Out((keys.numel(),), torch.float32, dev)
        L.check(L.lib().sfmi_sdf_query_keys_f32(L.ptr(axis), Q, L.ptr(keys), L.ptr(koff), keys.numel(), L.ptr(grid_cl), L.ptr(wp), L.ptr(o.t), B, G,
                                                int(sig), L.stream_ptr()), "sdf_query_keys")
        torch.cuda.synchronize()
        out["keys sigmoid" if sig else "keys"] = o.check("sdf_query_keys")
        assert _same(out["keys sigmoid" if sig else "keys"], ops.sdf_query_keys(axis, keys, koff, grid_cl, wp, sigmoid=sig))
    return out


def _twice_and_one_block(fn):
    """fn() at the default grid, twice, and twice with sdf_blocks = 1 (one workgroup walks every tile through the persistent loop; the
    knob is documented as performance-only): all four bit-identical -> the first"""
    a, b = fn(), fn()
    with _tune(b"sdf_blocks", 1):
        c, d = fn(), fn()
    for k in a:
        assert _same(a[k], b[k]), f"{k}: two launches differ"
        assert _same(c[k], d[k]), f"{k}: two launches differ (sdf_blocks = 1)"
        assert _same(a[k], c[k]), f"{k}: sdf_blocks = 1 changes the result"
    return a


@pytest.mark.parametrize("G", [2, 3, 16, 64])
def test_sdf_query_point_form_against_float64(dev, vq16_sd, G):
    from shapeformer_amd import ops
    grid, grid_cl = _grid(G, dev)
    wp = _banded(ops.sdf_pack_weights(vq16_sd), dev)
    worst = {}
    for B in (1, 3):
        for N in SDF_NS:
            pts = R.query_points(B, N, G, 100 * G + 10 * B + N)
            ref, bound, _ = R.query_ref(vq16_sd, grid[:B], pts)
            sref, sbound = R.sigmoid_bound(ref, bound)
            xyz = _banded(pts, dev)
            o = _twice_and_one_block(lambda: _point_launches(ops, xyz, grid_cl[:B], wp, dev))
            name = f"G{G} B{B} N{N}"
            assert _ratio(f"sdf logit | point {name}", o["logit"], ref, bound, worst) <= 1.0, name
            assert _ratio(f"sdf sigmoid | point {name}", o["sigmoid"], sref, sbound, worst) <= 1.0, name
    print("[worst]", f"sdf point G{G}", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("G", [2, 3, 16, 64])
@pytest.mark.parametrize("Q", [5, 7])
def test_sdf_query_lattice_and_keyed_forms_against_float64(dev, vq16_sd, G, Q):
    """The lattice form (plain, with the in-kernel affine, a slab of planes) and the keyed form, B = 3, Q odd (Q^2 no multiple of 32:
    tiles straddle planes and, in the keyed form, shapes): values within the bound, and the bit-equalities of test_sdf_query_gpu.py /
    test_iso_sparse_gpu.py - lattice == point form, slab == the whole lattice's planes, keyed == lattice."""
    from shapeformer_amd import ops
    B, slab = 3, (2, 5)
    grid, grid_cl = _grid(G, dev)
    wp = _banded(ops.sdf_pack_weights(vq16_sd), dev)
    g = torch.Generator().manual_seed(G + Q)
    aff = (torch.rand(B, 32, generator=g) + 0.5, torch.randn(B, 32, generator=g) * 0.3)
    axis_np = np.linspace(-1.0, 1.0, Q).astype(np.float32)
    keys_np = [np.sort(np.random.default_rng(G * Q + b).choice(Q ** 3, n, replace=False)).astype(np.int32) for b, n in enumerate((37, 1, 90))]
    koff_np = np.cumsum([0] + [len(k) for k in keys_np]).astype(np.int32)
    axis, keys, koff = _banded(axis_np, dev), _banded(np.concatenate(keys_np), dev), _banded(koff_np, dev)
    affd = (_banded(aff[0], dev), _banded(aff[1], dev))
    o = _twice_and_one_block(lambda: _lattice_launches(ops, axis, grid_cl, wp, affd, slab, keys, koff, dev))
    pts = R.lattice_points(axis_np, B)
    xyz = _banded(pts, dev)
    p = _twice_and_one_block(lambda: _point_launches(ops, xyz, grid_cl, wp, dev))
    # bit-equalities
    assert _same(o["grid"], p["logit"]) and _same(o["grid sigmoid"], p["sigmoid"]), "lattice form != point form"
    s0, s1 = slab[0] * Q * Q, slab[1] * Q * Q
    assert _same(o["slab"], o["grid"][:, s0:s1]) and _same(o["affine slab"], o["affine"][:, s0:s1]), "a slab != the whole lattice's planes"
    for b in range(B):
        kk = torch.from_numpy(keys_np[b]).long().to(dev)
        for a, f in (("keys", "grid"), ("keys sigmoid", "grid sigmoid")):
            assert _same(o[a][koff_np[b]:koff_np[b + 1]], o[f][b, kk]), "keyed form != lattice form"
    # values
    worst = {}
    name = f"G{G} Q{Q}"
    ref, bound, _ = R.query_ref(vq16_sd, grid, pts)
    sref, sbound = R.sigmoid_bound(ref, bound)
    aref, abound, _ = R.query_ref(vq16_sd, grid, pts, affine=aff)
    assert _ratio(f"sdf logit | lattice {name}", o["grid"], ref, bound, worst) <= 1.0
    assert _ratio(f"sdf sigmoid | lattice {name}", o["grid sigmoid"], sref, sbound, worst) <= 1.0
    assert _ratio(f"sdf affine | lattice {name}", o["affine"], aref, abound, worst) <= 1.0
    print("[worst]", f"sdf lattice {name}", {k: round(v, 4) for k, v in worst.items()})


def test_sigmoid_kernel_tail_and_in_place(dev):
    from shapeformer_amd import ops
    for n in (1, 3, 4, 5, 1027):
        g = torch.Generator().manual_seed(n)
        x = torch.rand(n, generator=g) * 200.0 - 100.0
        x[0] = 0.0
        if n > 2:
            x[n - 1], x[1] = -0.0, 100.0
        if n > 4:
            x[n - 2], x[2] = -100.0, -20.0
        ref, bound = R.sigmoid_bound(x.double(), torch.zeros(n, dtype=torch.float64))
        res = []
        for _ in range(2):
            o = _Out((n,), torch.float32, dev)
            ops.sigmoid(_banded(x, dev), out=o.t)
            io = _Out((n,), torch.float32, dev)
            io.t.copy_(x)
            ops.sigmoid(io.t, out=io.t)
            torch.cuda.synchronize()
            res.append((o.check(f"sigmoid n{n}"), io.check(f"sigmoid in place n{n}")))
        assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1]) and _same(res[0][0], res[0][1]), n
        assert _ratio(f"sigmoid | n{n}", res[0][0], ref, bound) <= 1.0
        assert float(res[0][0][0]) == 0.5
