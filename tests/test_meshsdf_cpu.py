"""Mesh signed distance, CPU side: the f64 oracle (tests/meshsdf_ref.py) against analytic distances and winding numbers, the
OBJ / OFF readers, the IMNet2 store writer read back by Imnet2LowResDataset, and meshsdf's argument checks (they raise before
any launch, so they need no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import meshsdf_ref as R   # noqa: E402


def test_oracle_cube_equals_box_sdf():
    rs = np.random.RandomState(0)
    q = np.concatenate([rs.uniform(-2, 2, (400, 3)), rs.uniform(-0.99, 0.99, (100, 3))])
    o = R.brute(q, R.CUBE_V, R.CUBE_F)
    assert np.abs(o["S"] - R.box_sdf(q)).max() < 1e-12
    C = o["C"]
    assert np.abs(np.sqrt(((q - C) ** 2).sum(1)) - np.abs(o["S"])).max() < 1e-12


def test_oracle_winding_number_closed_and_open():
    rs = np.random.RandomState(1)
    inside, outside = rs.uniform(-0.9, 0.9, (50, 3)), rs.uniform(1.1, 3, (50, 3)) * rs.choice([-1, 1], (50, 3))
    W = R.brute(np.concatenate([inside, outside]), R.CUBE_V, R.CUBE_F)["W"]
    assert np.abs(np.abs(W[:50]) - 1).max() < 1e-12 and np.abs(W[50:]).max() < 1e-12
    # just off the middle of one large triangle (normal +z): -1/2 on the side its normal points to, +1/2 behind it, up to the
    # solid angle the triangle misses
    tri_v, tri_f = np.array([[-100, -100, 0], [100, -100, 0], [0, 100, 0.]]), np.array([[0, 1, 2]])
    W = R.brute(np.array([[0, 0, 1e-3], [0, 0, -1e-3]]), tri_v, tri_f)["W"]
    assert abs(W[0] + 0.5) < 1e-4 and abs(W[1] - 0.5) < 1e-4 and abs(W[0]) < 0.5 and W[0] == -W[1]


def test_oracle_degenerate_faces_are_segments():
    q = np.array([[0.5, 1.0, 0.0], [3.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0.]])             # collinear: the segment [0, 2] on the x axis
    o = R.brute(q, v, np.array([[0, 1, 2]]))
    assert np.allclose(np.abs(o["S"]), [1.0, 1.0, 1.0]) and np.isfinite(o["W"]).all()
    o = R.brute(q, v, np.array([[1, 1, 1]]))                     # a point
    assert np.allclose(np.abs(o["S"]), np.linalg.norm(q - v[1], axis=1))


def test_read_obj_and_off(tmp_path):
    from shapeformer_amd import meshio
    p = tmp_path / "m.obj"
    p.write_text("# cube side\nv 0 0 0\nv 1 0 0\nvt 0 0\nvn 0 0 1\nv 1 1 0\nv 0 1 0\ng side\nusemtl m\n"
                 "f 1/1/1 2/1/1 3/1/1 4/1/1\nv 0 0 1\nf -1 1//1 2\n")
    v, f = meshio.read_obj(str(p))
    assert v.shape == (5, 3) and np.array_equal(v[4], [0, 0, 1])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1]]
    p = tmp_path / "m.off"
    p.write_text("OFF\n# comment\n5 2 0\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n0 0 1\n4 0 1 2 3\n3 4 0 1\n")
    v2, f2 = meshio.read_off(str(p))
    assert np.array_equal(v2, v) and f2.tolist() == f.tolist()
    p = tmp_path / "glued.off"
    p.write_text("OFF3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")
    v3, f3 = meshio.read_off(str(p))
    assert v3.shape == (3, 3) and f3.tolist() == [[0, 1, 2]]
    meshio.write_ply(str(tmp_path / "m.ply"), v, f)
    v4, f4 = meshio.read_mesh(str(tmp_path / "m.ply"))
    assert np.array_equal(v4, v) and np.array_equal(f4, f)
    with pytest.raises(ValueError):
        meshio.read_mesh(str(tmp_path / "m.stl"))


def test_write_imnet_store_reads_back(tmp_path):
    from shapeformer_amd import data as D
    from shapeformer_amd.make_dataset import write_imnet_store
    rs = np.random.RandomState(3)
    G, n, m = 8, 3, 100
    occ = (rs.rand(n, G, G, G) > 0.6).astype(np.uint8)
    Xbd = rs.uniform(-1, 1, (n, m, 3)).astype(np.float32)
    write_imnet_store(str(tmp_path), "mine", "train", Xbd, occ, {"chair": [0, 2], "table": [1]})
    ds = D.Imnet2LowResDataset(dataset="mine", split="train", root=str(tmp_path), grid_dim=G, boundary_N=64, cate="chair",
                               Xbd_as_Xct=True)
    assert len(ds) == 2
    it = ds[1]                                                    # the second chair: shape 2
    assert np.array_equal(it["Ytg"][:, 0], occ[2].reshape(-1))
    assert np.array_equal(it["Xtg"], D.make_grid([-1, -1, -1.], [1., 1, 1], [G] * 3).astype(np.float32))
    assert it["Xbd"].shape == (64, 3) and np.isin(it["Xbd"].view("V12"), Xbd[2].view("V12")).all()
    assert np.array_equal(np.load(tmp_path / "mine" / "train" / "cate_table.npy"), [1])


def test_meshsdf_argument_checks_raise_before_launch():
    from shapeformer_amd import meshsdf as MS
    from shapeformer_amd._lib import SfmiError
    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    q = torch.zeros(10, 3)
    with pytest.raises(SfmiError, match="queries"):
        MS.signed_distance_dev(torch.zeros(10, 2), v, f)
    with pytest.raises(SfmiError, match=r"verts \(V,3\)"):
        MS.signed_distance_dev(q, torch.zeros(8, 4), f)
    with pytest.raises(SfmiError, match="integer"):
        MS.signed_distance_dev(q, v, f.float())
    with pytest.raises(SfmiError, match="end at 8"):
        MS.signed_distance_dev(q, v, f, qoff=[0, 5, 10], voff=[0, 4, 7], toff=[0, 2, 4])
    with pytest.raises(SfmiError, match="nondecreasing"):
        MS.signed_distance_dev(q, v, f, qoff=[0, 5, 10], voff=[0, 4, 8], toff=[0, 3, 2, 4])
    with pytest.raises(SfmiError, match="different batch sizes"):
        MS.signed_distance_dev(q, v, f, qoff=[0, 5, 10], voff=[0, 4, 8], toff=[0, 1, 2, 4])
    with pytest.raises(SfmiError, match="query sets"):
        MS.signed_distance_dev(q, v, f, qoff=[0, 10], voff=[0, 4, 8], toff=[0, 2, 4])
    with pytest.raises(SfmiError, match="no faces"):
        MS.signed_distance_dev(q, v, f, qoff=[0, 5, 10], voff=[0, 4, 8], toff=[0, 4, 4])
    with pytest.raises(SfmiError, match="no faces"):
        MS.mesh_occupancy_dev(v, f, [0, 4, 8], [0, 0, 4])
    with pytest.raises(SfmiError, match="grid_dim"):
        MS.mesh_occupancy_dev(v, f, [0, 8], [0, 4], grid_dim=0)
    with pytest.raises(SfmiError, match="HIP device"):           # all host checks pass: the device check is the last one
        MS.signed_distance_dev(q, v, f)


def test_normalize_point_set():
    from shapeformer_amd.meshsdf import normalize_point_set
    v = np.array([[0, 0, 0], [4, 2, 1], [2, 1, 3.]])
    n = normalize_point_set(v)
    assert np.allclose(n.max(0)[0], 1) and np.allclose(n.min(0)[0], -1) and np.allclose(n.max(0) + n.min(0), 0)
    assert np.allclose(normalize_point_set(v, no_scale=True), v - [2, 1, 1.5])
