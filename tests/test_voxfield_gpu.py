"""GPU tests of the voxel fields (csrc/edt.hip, shapeformer_amd/voxfield.py) against the numpy / scipy restatement of
tests/voxfield_ref.py.  The distance transform is an integer problem and the solve a fixed-order f64 iteration: both are compared bit
for bit.  The Gaussian is compared within a derived bound."""
import functools

import numpy as np
import pytest
import torch

import voxfield_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _vox(g, dev):
    return _dev(np.asarray(g, bool).astype(np.uint8), dev)


def _np(t):
    return t.cpu().numpy()


def _same_bits(t, a):
    a = np.asarray(a)
    x = _np(t)
    return x.dtype == a.dtype and x.shape == a.shape and x.tobytes() == a.tobytes()


# ---- distance transform ------------------------------------------------------------------------------------------------------

def _random_grid(G, p, seed):
    return np.random.default_rng(seed).random((G, G, G)) < p


@functools.lru_cache(maxsize=None)
def _edt_case(name):
    """name -> tuple of grids (a batch)"""
    if name == "g5":
        return (_random_grid(5, 0.1, 1), _random_grid(5, 0.6, 2))
    if name in ("g32", "g33"):
        G = int(name[1:])
        return (_random_grid(G, 0.02, 3), R.sphere(G, 9.6, (13.2, 17.9, 15.1)))
    if name == "g65":
        return (R.sphere(65, 24.7, (30.1, 33.2, 31.7)), _random_grid(65, 0.01, 4), np.zeros((65, 65, 65), bool))
    if name == "g257":
        g = np.zeros((257, 257, 257), bool)
        idx = np.random.default_rng(6).integers(0, 257, (40, 3))
        g[idx[:, 0], idx[:, 1], idx[:, 2]] = True
        g[0, 0, 256] = g[256, 256, 0] = True                  # corners: the far distances run the whole line
        return (g,)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _edt_ref(name, invert):
    fn = R.edt_sq_brute if name == "g5" else R.edt_sq
    return tuple(fn(g, invert) for g in _edt_case(name))


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", ["g5", "g32", "g33", "g65", "g257"])
def test_edt_equals_the_integer_transform(dev, name, invert):
    from shapeformer_amd import voxfield as V
    grids = _edt_case(name)
    d2, status = V.edt_sq_dev(_vox(np.stack(grids), dev), invert=bool(invert))
    assert d2.dtype == torch.int32 and d2.shape == (len(grids),) + grids[0].shape
    for b, (g, ref) in enumerate(zip(grids, _edt_ref(name, invert))):
        assert _same_bits(d2[b], ref), (name, invert, b, int((_np(d2[b]) != ref).sum()))
    assert _np(status).tolist() == [R.edt_status(g, invert) for g in grids]
    if name == "g65" and not invert:
        assert _np(status).tolist() == [0, 0, 1] and (_np(d2[2]) == 3 * 65 * 65).all()


def test_edt_ignores_pad_bits(dev):
    """G = 33: Wz = 2 and 31 pad bits per row, all of them set in the input.  With invert they would otherwise read as clear voxels'
    complement; without, as set voxels beyond the lattice."""
    from shapeformer_amd import morph as M
    from shapeformer_amd import voxfield as V
    grids = _edt_case("g33")
    bits = M._pack(_vox(np.stack(grids), dev), 2, 33)
    dirty = bits.clone()
    dirty[..., 1] |= -2                                       # bits 1 .. 31 of every row's second word
    assert not torch.equal(dirty, bits)
    for invert in (0, 1):
        d2, status = V._edt_sq(dirty, 2, 33, invert)
        for b in range(2):
            assert _same_bits(d2[b], _edt_ref("g33", invert)[b]), (invert, b)
        assert _np(status).tolist() == [0, 0]
    d, status = V._signed(dirty, 2, 33)
    d_clean, _ = V._signed(bits, 2, 33)
    assert torch.equal(d, d_clean)
    w = V.gaussian_weights(1.0)
    assert torch.equal(V._gaussian(dirty, 2, 33, *w), V._gaussian(bits, 2, 33, *w))
    assert torch.equal(V._constrained(dirty, d, 2, 33, 4.0, 3), V._constrained(bits, d, 2, 33, 4.0, 3))


# ---- signed distance ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["g5", "g33", "g65"])
def test_signed_distance(dev, name):
    from shapeformer_amd import voxfield as V
    grids = _edt_case(name)
    d, status = V.signed_distance_dev(_vox(np.stack(grids), dev))
    assert d.dtype == torch.float64
    for b, g in enumerate(grids):
        x = _np(d[b])
        a, c = _edt_ref(name, 1)[b], _edt_ref(name, 0)[b]
        ref = R.signed_distance(g, a, c)
        if g.any() and not g.all():
            assert ((x > 0) == g).all()                      # the signs follow the bits
        d2 = np.where(g, a, c).astype(np.int64)
        square = np.rint(np.sqrt(d2)).astype(np.int64) ** 2 == d2
        assert np.array_equal(x[square], ref[square])
        assert (np.abs(x - ref) <= np.spacing(np.abs(ref) + 0.5)).all()       # 1 ulp of the square root
    assert _np(status).tolist() == [R.signed_status(g) for g in grids]
    if name == "g65":
        assert (_np(d[2]) == -np.sqrt(3.0 * 65 * 65) + 0.5).all()


def test_signed_distance_of_a_full_grid(dev):
    from shapeformer_amd import voxfield as V
    d, status = V.signed_distance_dev(torch.ones(9, 9, 9, device=dev, dtype=torch.bool))
    assert _np(status).tolist() == [1] and (_np(d) == np.sqrt(243.0) - 0.5).all()


# ---- Gaussian ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,sigma", [(33, 0.5), (33, 1.0), (33, 3.0), (5, 3.0)])
def test_gaussian_equals_scipy(dev, G, sigma):
    """Bound: three passes of at most 2 * 64 + 1 = 129 f64 terms, each of magnitude at most 0.5, the weights summing to 1: a rounding
    error of about 129 * 2^-53 * 0.5 = 1e-14 per pass whatever the order of the sum.  1e-12 is the margin.  G = 5 with sigma 3: the
    radius 12 exceeds the lattice and the reflection repeats."""
    from shapeformer_amd import voxfield as V
    grids = [R.sphere(G, G * 0.3, (G * 0.45, G * 0.5, G * 0.55)), _random_grid(G, 0.3, 7)]
    out = V.gaussian_smooth_dev(_vox(np.stack(grids), dev), sigma)
    assert out.dtype == torch.float64
    for b, g in enumerate(grids):
        err = np.abs(_np(out[b]) - R.gaussian(g, sigma)).max()
        print(f"G {G} sigma {sigma} grid {b}: max |device - scipy| = {err:.3e}")
        assert err <= 1e-12


# ---- constrained solve -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _solve_grids():
    return R.solve_grids()


@pytest.mark.parametrize("name", ["sphere17", "sphere33", "noise17", "slab17"])
def test_constrained_equals_the_iteration_bit_for_bit(dev, name):
    """the reference is fed the device's own d: the solve is tested apart from the square root"""
    from shapeformer_amd import morph as M
    from shapeformer_amd import voxfield as V
    g = _solve_grids()[name]
    G = g.shape[0]
    bits = M._pack(_vox(g[None], dev), 1, G)
    d, _ = V._signed(bits, 1, G)
    d_host = _np(d[0])
    band = R.band_of(d_host)
    ref, energies = d_host.copy(), {0: R.energy(d_host)}
    done = 0
    for iters in (0, 1, 8):
        while done < iters:
            ref = R.constrained_step(ref, d_host, g, band)
            done += 1
        u, ws = V._constrained(bits, d, 1, G, 4.0, iters, return_ws=True)
        assert _same_bits(u[0], ref), (name, iters, int((_np(u[0]) != ref).sum()))
        energies[iters] = R.energy(_np(u[0]))
    # the lists: ascending flat index, the band and its one-step support
    bl, sl = V._band_lists(ws, 1, G)
    assert np.array_equal(_np(bl), np.flatnonzero(band).astype(np.int32))
    assert np.array_equal(_np(sl), np.flatnonzero(R.support_of(band)).astype(np.int32))
    u200 = _np(V._constrained(bits, d, 1, G, 4.0, 200)[0])
    assert (u200[g] >= 0).all() and (u200[~g] <= 0).all()
    assert np.array_equal(u200[~band], d_host[~band])
    e200 = R.energy(u200)
    print(f"{name}: E_0 {energies[0]:.1f} E_8 {energies[8]:.1f} E_200 {e200:.1f} band {band.mean():.3f} of the lattice")
    assert e200 <= energies[8] <= energies[0]


def test_constrained_band_radius_zero_and_wide(dev):
    """band_radius 0: no voxel has |d| <= 0, the lists are empty and u = d; a radius beyond the lattice: every voxel is in the band"""
    from shapeformer_amd import morph as M
    from shapeformer_amd import voxfield as V
    g = _solve_grids()["noise17"]
    bits = M._pack(_vox(g[None], dev), 1, 17)
    d, _ = V._signed(bits, 1, 17)
    u, ws = V._constrained(bits, d, 1, 17, 0.0, 5, return_ws=True)
    bl, sl = V._band_lists(ws, 1, 17)
    assert torch.equal(u, d) and len(bl) == 0 and len(sl) == 0
    u, ws = V._constrained(bits, d, 1, 17, 100.0, 3, return_ws=True)
    bl, sl = V._band_lists(ws, 1, 17)
    assert len(bl) == 17 ** 3 and len(sl) == 17 ** 3
    assert _same_bits(u[0], R.constrained(g, _np(d[0]), 100.0, 3))


# ---- determinism and batching ------------------------------------------------------------------------------------------------

def _every_entry(V, vox):
    return [V.edt_sq_dev(vox)[0], V.edt_sq_dev(vox, invert=True)[0], V.signed_distance_dev(vox)[0], V.gaussian_smooth_dev(vox, 1.0),
            V.constrained_smooth_dev(vox, iters=6)[0], V.smooth_dev(vox, "gaussian", sigma=0.7), V.edt_sq_dev(vox)[1],
            V.signed_distance_dev(vox)[1]]


def test_batches_streams_and_runs_give_the_same_bits(dev):
    from shapeformer_amd import morph as M
    from shapeformer_amd import voxfield as V
    G = 21                                                     # 3 * 21^3 = 27783 voxels: seven chunks of the compaction, the grids
    grids = [R.sphere(G, 6.4, (9.3, 10.1, 11.2)), _random_grid(G, 0.4, 8), np.zeros((G, G, G), bool)]   # cut across chunk borders
    grids[2][:7] = True
    batch = _vox(np.stack(grids), dev)
    first = _every_entry(V, batch)
    for a, b in zip(first, _every_entry(V, batch)):            # two runs
        assert torch.equal(a, b)
    for i in range(3):                                         # a batch equals the single calls; (G,G,G) equals a batch of one
        one = _every_entry(V, batch[i:i + 1])
        bare = _every_entry(V, batch[i])
        for a, b, c in zip(first, one, bare):
            assert torch.equal(a[i:i + 1], b)
            assert torch.equal(b[0], c) if c.dim() == 3 else torch.equal(b, c)
    s = torch.cuda.Stream(device=dev)                          # a non-default stream
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        other = _every_entry(V, batch)
    s.synchronize()
    for a, b in zip(first, other):
        assert torch.equal(a, b)
    # the lists of one grid do not depend on its batch-mates
    bits = M._pack(batch, 3, G)
    d, _ = V._signed(bits, 3, G)
    _, ws = V._constrained(bits, d, 3, G, 4.0, 1, return_ws=True)
    bl, sl = (_np(x) for x in V._band_lists(ws, 3, G))
    assert (np.diff(bl) > 0).all() and (np.diff(sl) > 0).all()
    for i in range(3):
        _, ws1 = V._constrained(bits[i:i + 1].contiguous(), d[i:i + 1].contiguous(), 1, G, 4.0, 1, return_ws=True)
        b1, s1 = (_np(x) for x in V._band_lists(ws1, 1, G))
        lo, hi = i * G ** 3, (i + 1) * G ** 3
        assert np.array_equal(bl[(bl >= lo) & (bl < hi)] - lo, b1) and np.array_equal(sl[(sl >= lo) & (sl < hi)] - lo, s1)
        assert len(b1) > 0


def test_bool_and_nonzero_inputs_are_the_same_grid(dev):
    from shapeformer_amd import voxfield as V
    g = _random_grid(12, 0.3, 9)
    a = V.signed_distance_dev(_vox(g, dev))[0]
    assert torch.equal(a, V.signed_distance_dev(_dev(g, dev))[0])
    assert torch.equal(a, V.signed_distance_dev(_dev(g.astype(np.uint8) * 200, dev))[0])


# ---- mesh --------------------------------------------------------------------------------------------------------------------

def test_smooth_mesh_of_a_voxelised_sphere(dev):
    from shapeformer_amd import components as C
    from shapeformer_amd import mcubes as MC
    from shapeformer_amd import voxfield as V
    G, r, c = 33, 10.3, np.array([16.3, 15.8, 16.1])
    g = R.sphere(G, r, c)
    vox = _vox(g, dev)
    centre = -1.0 + 2.0 * c / (G - 1)                          # the lattice maps onto the box [-1, 1]^3

    def radius_std(v):
        return float(np.sqrt(((_np(v).astype(np.float64) - centre) ** 2).sum(1)).std())
    v0, f0, _, _ = MC.marching_cubes_dev(vox[None].float(), 0.5)
    v1, f1, voff, toff = V.voxels2mesh_dev(vox, method="constrained")
    s0, s1 = radius_std(v0), radius_std(v1)
    print(f"vertex radius std: binary {s0:.5f} constrained {s1:.5f} ratio {s1 / s0:.3f}")
    assert s1 < s0 / 3
    assert v1.dtype == torch.float32 and f1.dtype == torch.int32 and voff.tolist() == [0, len(v1)] and toff.tolist() == [0, len(f1)]
    coff = C.mesh_components_dev(v1, f1, voff, toff)[2]
    assert list(coff) == [0, 1]                                # one piece
    va, fa = MC.array2mesh(g.astype(np.float32), smooth="constrained", device=str(dev))
    assert np.array_equal(va, _np(v1).astype(np.float64)) and np.array_equal(fa, _np(f1).astype(int))
    va, fa = MC.array2mesh(g.astype(np.float32), gaussian_sigma=2.0, device=str(dev))          # the reference's keyword alone
    assert np.array_equal(va, _np(v1).astype(np.float64)) and np.array_equal(fa, _np(f1).astype(int))
    vg, fg = MC.array2mesh(g.astype(np.float32), smooth="gaussian", gaussian_sigma=1.0, device=str(dev))
    v2, f2, _, _ = V.voxels2mesh_dev(vox, method="gaussian", sigma=1.0)
    assert np.array_equal(vg, _np(v2).astype(np.float64)) and np.array_equal(fg, _np(f2).astype(int))
    assert radius_std(v2) < s0
    # both keywords None: today's mesh, bit for bit
    vd, fd = MC.array2mesh(g.astype(np.float32), device=str(dev))
    assert np.array_equal(vd, _np(v0).astype(np.float64)) and np.array_equal(fd, _np(f0).astype(int))


def test_batch_of_meshes_equals_single_meshes(dev):
    from shapeformer_amd import voxfield as V
    grids = [R.sphere(17, 5.3, (6.2, 8.9, 9.4)), _solve_grids()["noise17"]]
    v, f, voff, toff = V.voxels2mesh_dev(_vox(np.stack(grids), dev), iters=20, bbox=((0, 0, 0), (1, 2, 3)))
    for i, g in enumerate(grids):
        v1, f1, _, _ = V.voxels2mesh_dev(_vox(g, dev), iters=20, bbox=((0, 0, 0), (1, 2, 3)))
        assert torch.equal(v[voff[i]:voff[i + 1]], v1) and torch.equal(f[toff[i]:toff[i + 1]], f1)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------

def test_every_entry_refuses_bad_arguments(dev):
    from shapeformer_amd import _lib as L
    lib, P, E = L.lib(), L.ptr, L.SFMI_EINVAL
    B, G = 2, 6
    NV = B * G ** 3
    bits = torch.zeros(B, G, G, 1, device=dev, dtype=torch.int32)
    d2 = torch.zeros(NV, device=dev, dtype=torch.int32)
    st = torch.zeros(B, device=dev, dtype=torch.int32)
    d, u = torch.zeros(NV, device=dev, dtype=torch.float64), torch.zeros(NV, device=dev, dtype=torch.float64)
    w = torch.ones(129, device=dev, dtype=torch.float64)
    ws = torch.zeros(1 << 20, device=dev, dtype=torch.uint8)
    sizes = [(0, G), (-1, G), (B, 0), (B, -2), (B, 514), (16, 513), (2 ** 30, 2)]
    for b, g in sizes:
        assert lib.sfmi_edt_sq_u32(P(bits), b, g, 0, P(d2), P(st), P(ws), None) == E
        assert lib.sfmi_edt_signed_f64(P(bits), b, g, P(d), P(st), P(ws), None) == E
        assert lib.sfmi_vox_gaussian_f64(P(bits), b, g, P(w), 1, P(d), P(ws), None) == E
        assert lib.sfmi_vox_constrained_f64(P(bits), P(d), b, g, 4.0, 1, P(u), P(ws), None) == E
        assert lib.sfmi_vox_constrained_lists_i32(P(ws), b, g, P(d2), P(d2), P(st), None) == E
        assert lib.sfmi_edt_workspace_bytes(b, g, 0) == 0 and lib.sfmi_vox_constrained_workspace_bytes(b, g) == 0
        assert lib.sfmi_vox_gaussian_workspace_bytes(b, g) == 0
    for k in range(4):                                         # a NULL pointer in every position
        a = [P(bits), P(d2), P(st), P(ws)]
        a[k] = None
        assert lib.sfmi_edt_sq_u32(a[0], B, G, 0, a[1], a[2], a[3], None) == E
        a = [P(bits), P(d), P(st), P(ws)]
        a[k] = None
        assert lib.sfmi_edt_signed_f64(a[0], B, G, a[1], a[2], a[3], None) == E
        a = [P(bits), P(w), P(d), P(ws)]
        a[k] = None
        assert lib.sfmi_vox_gaussian_f64(a[0], B, G, a[1], 1, a[2], a[3], None) == E
        a = [P(bits), P(d), P(u), P(ws)]
        a[k] = None
        assert lib.sfmi_vox_constrained_f64(a[0], a[1], B, G, 4.0, 1, a[2], a[3], None) == E
        a = [P(ws), P(d2), P(d2), P(st)]
        a[k] = None
        assert lib.sfmi_vox_constrained_lists_i32(a[0], B, G, a[1], a[2], a[3], None) == E
    for radius in (-1, 65, 1000):
        assert lib.sfmi_vox_gaussian_f64(P(bits), B, G, P(w), radius, P(d), P(ws), None) == E
    assert lib.sfmi_vox_constrained_f64(P(bits), P(d), B, G, 4.0, -1, P(u), P(ws), None) == E
    for r in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert lib.sfmi_vox_constrained_f64(P(bits), P(d), B, G, r, 1, P(u), P(ws), None) == E
    assert lib.sfmi_vox_constrained_f64(P(bits), P(d), B, G, 4.0, 1, P(d), P(ws), None) == E          # u must not be d
    torch.cuda.synchronize()
    assert int(d2.abs().sum()) == 0 and float(u.abs().sum()) == 0.0 and int(ws.sum()) == 0             # nothing was launched
    # the controls: the same buffers with good arguments
    assert lib.sfmi_edt_sq_u32(P(bits), B, G, 0, P(d2), P(st), P(ws), L.stream_ptr()) == 0
    assert lib.sfmi_vox_gaussian_f64(P(bits), B, G, P(w), 64, P(d), P(ws), L.stream_ptr()) == 0
    assert lib.sfmi_vox_constrained_f64(P(bits), P(d), B, G, 4.0, 0, P(u), P(ws), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [1, 1] and (d2 == 3 * G * G).all() and torch.equal(u, d)
