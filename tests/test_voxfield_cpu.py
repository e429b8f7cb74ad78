"""CPU tests of the voxel-field contract: the numpy / scipy restatement of tests/voxfield_ref.py checked against
itself (brute force, energy, constraints, roughness), the envelope routine of csrc/sfmi_edt_line.h compiled for the host against the
double loop, the host-side argument checks of shapeformer_amd/voxfield.py (they raise before the library is loaded), array2mesh's
keyword parsing and the exported symbols."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import voxfield_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def test_scipy_edt_is_the_integer_transform():
    from scipy import ndimage
    g = np.random.default_rng(0).random((9, 9, 9)) < 0.08
    for invert in (False, True):
        brute = R.edt_sq_brute(g, invert)
        e = ndimage.distance_transform_edt(~(g ^ invert))
        assert np.array_equal(np.rint(e ** 2).astype(np.int32), brute)
        assert np.array_equal(e, np.sqrt(brute.astype(np.float64)))          # bitwise: scipy's distance is sqrt(integer)
        assert np.array_equal(R.edt_sq(g, invert), brute)
    empty = np.zeros((5, 5, 5), bool)
    assert (R.edt_sq(empty) == 75).all() and (R.edt_sq_brute(empty) == 75).all() and R.edt_status(empty) == 1
    assert (R.edt_sq(empty, True) == 0).all() and R.edt_status(empty, True) == 0


def test_signed_distance_signs_and_faces():
    g = R.sphere(17, 5.3, (6.2, 8.9, 9.4))
    d = R.signed_distance(g)
    assert ((d > 0) == g).all() and np.abs(d).min() == 0.5
    assert R.signed_status(g) == 0 and R.signed_status(np.ones((4, 4, 4), bool)) == 1 and R.signed_status(np.zeros((4, 4, 4), bool)) == 1
    full = R.signed_distance(np.ones((4, 4, 4), bool))
    assert (full == np.sqrt(48.0) - 0.5).all()


def test_laplacian_is_symmetric_and_kills_constants():
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((2, 6, 6, 6))
    assert abs((R.laplace(x) * y).sum() - (x * R.laplace(y)).sum()) < 1e-10
    assert np.abs(R.laplace(np.full((6, 6, 6), 3.25))).max() == 0.0


@pytest.mark.parametrize("name", ["sphere17", "sphere33", "noise17", "slab17"])
def test_energy_never_increases_and_signs_hold(name):
    g = R.solve_grids()[name]
    d = R.signed_distance(g)
    band = R.band_of(d)
    touches_face = band[0].any() or band[-1].any() or band[:, 0].any() or band[:, -1].any() or band[:, :, 0].any() or band[:, :, -1].any()
    assert touches_face == (name != "sphere33")
    trace = []
    u = R.constrained(g, d, 4.0, 200, trace)
    assert len(trace) == 201
    assert all(b <= a for a, b in zip(trace, trace[1:])), "E(u) increased"
    assert trace[200] <= trace[8] <= trace[0] and trace[200] < trace[0]
    assert (u[g] >= 0).all() and (u[~g] <= 0).all()
    assert np.array_equal(u[~band], d[~band])


def test_support_is_the_band_and_its_neighbours():
    g = R.solve_grids()["slab17"]
    band = R.band_of(R.signed_distance(g), 1.0)
    sup = R.support_of(band)
    assert band[4:6].all() and not band[:4].any() and not band[6:].any()          # d = .. 1.5, 0.5 | -0.5, -1.5 ..
    assert sup[3:7].all() and not sup[:3].any() and not sup[7:].any()


@pytest.mark.parametrize("G,r", [(33, 10.3), (65, 24.7)])
def test_constrained_field_is_three_times_smoother_than_the_voxels(G, r):
    """the radius of the zero crossings along the lattice lines of a voxelised sphere: its std for the binary field is 0.2 voxels,
    for the constrained field a sixth to a fifth of that"""
    c = [(G - 1) / 2.0 + 0.3, (G - 1) / 2.0 - 0.2, (G - 1) / 2.0 + 0.1]
    g = R.sphere(G, r, c)
    binary = R.radius_std(g.astype(np.float64) - 0.5, c)
    smooth = R.radius_std(R.constrained(g, iters=200), c)
    gauss = R.radius_std(R.gaussian(g, 1.0), c)
    print(f"G {G}: binary {binary:.4f} gaussian(1) {gauss:.4f} constrained {smooth:.4f} ratio {smooth / binary:.3f}")
    assert 0.1 < binary < 0.3
    assert smooth < binary / 3 and gauss < binary


# ---- the envelope routine, compiled for the host -----------------------------------------------------------------------------

_LINE_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "sfmi_edt_line.h"
int main() {
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  long bad = 0;
  for (int trial = 0; trial < 4000; ++trial) {
    const int m = 1 + rnd() % (trial % 50 == 0 ? 513 : 40), stride = 1 + rnd() % 3, mode = rnd() % 5;
    std::vector<int> f(m * stride, -7), out(m * stride, -7);
    std::vector<unsigned short> S(m * stride), T(m * stride);
    for (int y = 0; y < m; ++y) {
      int v;
      switch (mode) {
        case 0: v = (rnd() % 4 == 0) ? (int)(rnd() % 30) * (int)(rnd() % 30) : SFMI_EDT_INF; break;    // the j pass: squares and empty rows
        case 1: v = rnd() % 600000; break;
        case 2: v = SFMI_EDT_INF + rnd() % 500000; break;                                             // an empty grid in the i pass
        case 3: v = (rnd() % 8 == 0) ? 0 : SFMI_EDT_INF + (int)(rnd() % 3) * 263169; break;
        default: v = (rnd() % 3) ? (int)(rnd() % 9) : SFMI_EDT_INF; break;
      }
      f[y * stride] = v;
    }
    sfmi_edt_line(f.data(), out.data(), S.data(), T.data(), m, stride);
    for (int x = 0; x < m; ++x) {
      long best = 1l << 40;
      for (int y = 0; y < m; ++y) { const long c = (long)f[y * stride] + (long)(x - y) * (x - y); if (c < best) best = c; }
      if (best != out[x * stride]) ++bad;
    }
  }
  std::printf("bad %ld\n", bad);
  return bad != 0;
}
"""


def test_envelope_line_equals_the_double_loop(tmp_path):
    """csrc/sfmi_edt_line.h is host and device code: the lower envelope of one line against min_y f[y] + (x - y)^2, for lines of 1 to 513
    elements at strides 1 to 3 with finite values, the "no set voxel" value and mixtures, under the address and undefined-behaviour
    sanitizers (a stand-alone host program)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        from shapeformer_amd import build as B
        cxx = B._hipcc()
    src, exe = tmp_path / "line.cpp", tmp_path / "line"
    src.write_text(_LINE_PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "shapeformer_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "bad 0", out.stdout + out.stderr


# ---- the host argument checks: every one raises SfmiError before the library is loaded ----------------------------------------

@pytest.fixture()
def no_library(monkeypatch):
    from shapeformer_amd import _lib
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def _calls(V):
    return {"edt_sq_dev": V.edt_sq_dev, "signed_distance_dev": V.signed_distance_dev, "gaussian_smooth_dev": V.gaussian_smooth_dev,
            "constrained_smooth_dev": V.constrained_smooth_dev, "smooth_dev": V.smooth_dev, "voxels2mesh_dev": V.voxels2mesh_dev}


@pytest.mark.parametrize("name", ["edt_sq_dev", "signed_distance_dev", "gaussian_smooth_dev", "constrained_smooth_dev", "smooth_dev",
                                  "voxels2mesh_dev"])
def test_grid_argument_checks(no_library, name):
    from shapeformer_amd import voxfield as V
    from shapeformer_amd._lib import SfmiError
    fn = _calls(V)[name]
    with pytest.raises(SfmiError, match="torch tensor"):
        fn(np.zeros((4, 4, 4), np.uint8))
    for shape in [(4, 4), (2, 4, 4, 5), (4, 5, 4), (1, 2, 4, 4, 4), (2, 0, 0, 0)]:
        with pytest.raises(SfmiError, match=r"\(B,G,G,G\)"):
            fn(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(SfmiError, match="empty batch"):
        fn(torch.zeros(0, 4, 4, 4, dtype=torch.uint8))
    with pytest.raises(SfmiError, match="at most 513"):
        fn(torch.zeros(1, dtype=torch.uint8).expand(1, 514, 514, 514))          # a view of one byte: nothing this large is allocated
    with pytest.raises(SfmiError, match="2\\^31"):
        fn(torch.zeros(1, dtype=torch.uint8).expand(16, 513, 513, 513))
    with pytest.raises(SfmiError, match="HIP device"):               # all host checks pass: the device check is the last one
        fn(torch.zeros(4, 4, 4, dtype=torch.uint8))
    with pytest.raises(SfmiError, match="HIP device"):
        fn(torch.zeros(2, 4, 4, 4, dtype=torch.bool))


def test_method_argument_checks(no_library):
    from shapeformer_amd import voxfield as V
    from shapeformer_amd._lib import SfmiError
    vox = torch.zeros(4, 4, 4, dtype=torch.uint8)
    for sigma in (0, -1.0, float("nan"), float("inf"), "3", True, None):
        with pytest.raises(SfmiError, match="sigma"):
            V.gaussian_smooth_dev(vox, sigma)
        with pytest.raises(SfmiError, match="sigma"):
            V.smooth_dev(vox, "gaussian", sigma=sigma)
    with pytest.raises(SfmiError, match="radius of 65"):
        V.gaussian_smooth_dev(vox, 16.2)
    for r in (-0.5, float("nan"), float("inf"), "4", None, True):
        with pytest.raises(SfmiError, match="band_radius"):
            V.constrained_smooth_dev(vox, band_radius=r)
        with pytest.raises(SfmiError, match="band_radius"):
            V.voxels2mesh_dev(vox, band_radius=r)
    for n in (-1, 2.0, None, True):
        with pytest.raises(SfmiError, match="iters"):
            V.constrained_smooth_dev(vox, iters=n)
    for big in (torch.zeros(1, 1, 1, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8).expand(6, 513, 513, 513)):
        with pytest.raises(SfmiError, match="marching cubes needs"):
            V.voxels2mesh_dev(big)
    for fn in (V.smooth_dev, V.voxels2mesh_dev):
        with pytest.raises(SfmiError, match="method"):
            fn(vox, "laplacian")
        with pytest.raises(SfmiError, match="takes"):
            fn(vox, "constrained", sigma=1.0)
        with pytest.raises(SfmiError, match="takes"):
            fn(vox, "gaussian", iters=3)
        with pytest.raises(SfmiError, match="HIP device"):
            fn(vox, "gaussian", sigma=1.0)
        with pytest.raises(SfmiError, match="HIP device"):
            fn(vox, "constrained", band_radius=0, iters=0)


def test_gaussian_weights_are_scipys():
    from scipy.ndimage import _filters
    from shapeformer_amd import voxfield as V
    for sigma in (0.5, 1.0, 3.0, 16.1):
        radius, w = V.gaussian_weights(sigma)
        assert radius == int(4.0 * sigma + 0.5) and len(w) == 2 * radius + 1
        assert np.array_equal(w, _filters._gaussian_kernel1d(float(sigma), 0, radius))
    assert V.gaussian_weights(0.1)[0] == 0 and V.gaussian_weights(0.1)[1].tolist() == [1.0]


def test_array2mesh_keyword_parsing(no_library):
    from shapeformer_amd import mcubes as MC
    from shapeformer_amd._lib import SfmiError
    assert MC._smooth_choice(None, None) is None
    assert MC._smooth_choice(2.0, None) == ("constrained", {})           # the reference: any non-None value calls mcubes.smooth
    assert MC._smooth_choice(None, "constrained") == ("constrained", {})
    assert MC._smooth_choice(1.5, "constrained") == ("constrained", {})
    assert MC._smooth_choice(None, "gaussian") == ("gaussian", {})
    assert MC._smooth_choice(1.5, "gaussian") == ("gaussian", {"sigma": 1.5})
    with pytest.raises(SfmiError, match="smooth = "):
        MC._smooth_choice(None, "median")
    grid = np.zeros((4, 4, 4), np.float32)
    with pytest.raises(SfmiError, match="smooth = "):
        MC.array2mesh(grid, smooth=True, device="cpu")
    with pytest.raises(SfmiError, match="sigma"):
        MC.array2mesh(grid, smooth="gaussian", gaussian_sigma=-1.0, device="cpu")
    with pytest.raises(SfmiError, match="HIP device"):
        MC.array2mesh(grid, gaussian_sigma=1.0, device="cpu")
    import inspect
    sig = inspect.signature(MC.array2mesh)
    assert sig.parameters["gaussian_sigma"].default is None and sig.parameters["smooth"].default is None


def test_voxfield_is_outside_the_input_forms_census():
    """the new public functions live in a module of their own: none was added to a module that tests/input_forms.py lists"""
    import input_forms as IF
    assert "voxfield" not in IF.MODULES
    from shapeformer_amd import mcubes as MC
    import inspect
    public = {k for k, v in vars(MC).items() if inspect.isfunction(v) and v.__module__ == MC.__name__ and not k.startswith("_")}
    assert public == {"marching_cubes_dev", "array2mesh"}


def test_header_declares_the_entries():
    from shapeformer_amd import _lib as L
    for name in ("sfmi_edt_sq_u32", "sfmi_edt_signed_f64", "sfmi_edt_workspace_bytes", "sfmi_vox_gaussian_f64",
                 "sfmi_vox_gaussian_workspace_bytes", "sfmi_vox_constrained_f64", "sfmi_vox_constrained_workspace_bytes",
                 "sfmi_vox_constrained_lists_i32", "sfmi_vox_max_grid", "sfmi_vox_gaussian_max_radius"):
        assert name in L.PROTOTYPES, name
    text = open(L.HEADER).read()
    assert "geoutil.py:194-197" in text


def test_workspace_sizes_and_refusals_of_the_size_functions():
    """the size functions run without a device: 0 for sizes the entries refuse, and the stated layouts otherwise"""
    import ctypes
    from shapeformer_amd import _lib as L
    from shapeformer_amd import build as B
    B.build(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)

    def fn(name):
        f = getattr(lib, name)
        f.restype, f.argtypes = L.PROTOTYPES[name]
        return f
    a256 = lambda n: (n + 255) // 256 * 256
    assert fn("sfmi_vox_max_grid")() == 513 and fn("sfmi_vox_gaussian_max_radius")() == 64
    for Bn, G in [(1, 5), (3, 65), (1, 513), (8, 256)]:
        NV = Bn * G ** 3
        edt = a256(4 * NV) + 2 * a256(2 * NV)
        assert fn("sfmi_edt_workspace_bytes")(Bn, G, 0) == edt
        assert fn("sfmi_edt_workspace_bytes")(Bn, G, 1) == edt + 2 * a256(4 * NV) + a256(8 * Bn)
        assert fn("sfmi_vox_gaussian_workspace_bytes")(Bn, G) == a256(8 * NV)
        assert fn("sfmi_vox_constrained_workspace_bytes")(Bn, G) == a256(8 * NV) + 2 * a256(4 * NV) + a256(NV) + a256(8 * ((NV + 4095) // 4096)) + 256
    for Bn, G in [(0, 4), (-1, 4), (1, 0), (1, 514), (16, 513), (1, -3)]:
        assert fn("sfmi_edt_workspace_bytes")(Bn, G, 0) == 0 and fn("sfmi_edt_workspace_bytes")(Bn, G, 1) == 0
        assert fn("sfmi_vox_gaussian_workspace_bytes")(Bn, G) == 0 and fn("sfmi_vox_constrained_workspace_bytes")(Bn, G) == 0
