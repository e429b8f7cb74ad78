"""GPU: the mesh tree (csrc/meshtree.hip, shapeformer_amd/meshtree.py).  The node table against tests/meshtree_ref.py's own build;
exact distance bit for bit against the brute route (meshsdf.signed_distance_dev); the tree-code winding number against meshtree_ref's
f64 traversal of the node table the device built; lattice occupancy against the brute route outside the band of test_meshtree_cpu.py;
determinism; status codes; the reference's signatures; volumetric IoU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import meshsdf_ref as R   # noqa: E402
import meshtree_ref as M   # noqa: E402
from test_meshsdf_gpu import _queries, _soup   # noqa: E402
from test_meshtree_cpu import RECORDED   # noqa: E402

pytestmark = pytest.mark.gpu

# f32 evaluation noise of W_tree against the f64 traversal that takes the same branches, measured on the sphere and bowl fixtures
# (beta = 2 and 3, 1 200 queries each: sphere 2.49e-6, bowl 3.59e-6 on an MI355X), times 4 because it is noise.  DESIGN.md §5.23
W_NOISE_MEASURED = 3.6e-6
W_TOL = 4 * W_NOISE_MEASURED


def _t(x, dev, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)


def _bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
    return x.view(np.int32) if x.dtype == np.float32 else x


def _mt():
    from shapeformer_amd import meshtree
    return meshtree


def _ms():
    from shapeformer_amd import meshsdf
    return meshsdf


def _batch(meshes, dev):
    from shapeformer_amd._ragged import batch_meshes
    return batch_meshes(meshes, dev)


_torus_cache = {}


def _mc_torus():
    if "m" not in _torus_cache:
        from oracle import mc_oracle as MO
        from test_mcubes_cpu import _torus
        v, f = MO.marching_cubes(_torus(24), 0.5)
        _torus_cache["m"] = (v.astype(np.float32), f.astype(np.int32))
    return _torus_cache["m"]


def _node_table(tree, b=0):
    n0, n1 = int(tree.noff[b]), int(tree.noff[b + 1])
    nd = tree.nodes.cpu().numpy().reshape(-1, 9, 4)[n0:n1]
    coef = np.concatenate([nd[:, 2, 3:], nd[:, 4], nd[:, 5], nd[:, 6], nd[:, 7], nd[:, 8, :3]], 1)      # meshtree_ref.coefficients' order
    return dict(lo=nd[:, 0, :3], hi=nd[:, 1, :3], r=nd[:, 0, 3], noprune=nd[:, 1, 3] != 0, p=nd[:, 2, :3], dip=nd[:, 3, :3], coef=coef,
                mom=tree.mom.cpu().numpy()[n0:n1])


def _ulp_equal(a, b):
    """equal, or one ulp apart"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a == b) | (np.nextafter(a, b) == b)).all())


# ---- the node table -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 64, 65, 513, 4100])
def test_node_table_is_the_references(dev, T):
    v, f = M.strip_mesh(T)
    rs = np.random.RandomState(T)
    v = (v + rs.randint(-8, 9, v.shape) / 64).astype(np.float32)         # off the plane: every moment is non-trivial
    tree = _mt().mesh_tree_dev(_t(v, dev), _t(f, dev, torch.int32))
    ref = M.build(v, f)
    assert tree.status.cpu().tolist() == [0]
    assert np.array_equal(tree.keys.cpu().numpy(), M.morton_keys(v, f))
    assert np.array_equal(tree.order.cpu().numpy(), ref["order"]) and np.array_equal(tree.orig.cpu().numpy(), ref["order"])
    assert int(tree.noff[1]) == sum(ref["levels"]) == _lib().sfmi_meshtree_nodes(T)
    got = _node_table(tree)
    assert np.array_equal(_bits(got["lo"]), _bits(ref["lo"])) and np.array_equal(_bits(got["hi"]), _bits(ref["hi"]))
    scale = np.abs(ref["mom"]).max(0) + 1e-300
    assert (np.abs(got["mom"] - ref["mom"]) <= 1e-12 * scale).all()
    assert _ulp_equal(got["p"], ref["p"]) and _ulp_equal(got["dip"], ref["dip"])
    # the second and third moments: the shift of the device's own f64 sums to the device's own centre, in the reference's order
    assert _ulp_equal(got["coef"], M.coefficients(got["mom"], got["p"]))
    # the radius: about the DEVICE's stored p~, 1e-12 relative before rounding, i.e. equal after rounding up to 1 ulp
    P, L0 = ref["P"].astype(np.float64), ref["levels"][0]
    for l, n in enumerate(ref["levels"]):
        for j in range(n):
            a0, a1 = M.leaf_range(l, j, L0)
            k = M.level_base(ref["levels"], l) + j
            d = np.sqrt(((P[a0 * 64:min(a1 * 64, T)].reshape(-1, 3) - got["p"][k].astype(np.float64)) ** 2).sum(1).max())
            assert float(got["r"][k]) >= d * (1 - 1e-12) and _ulp_equal(got["r"][k], M.round_up_f32(d))
    assert not got["noprune"].any()
    # the packed records are the brute route's, in sorted order: the same face routine packs them
    rec = tree.rec.cpu().numpy().reshape(T, 5, 4)
    assert np.array_equal(rec[:, 0, :3], ref["P"][:, 0]) and np.array_equal(rec[:, 3, :3], ref["P"][:, 1])


def _lib():
    from shapeformer_amd import _lib as L
    return L.lib()


def test_slivers_forbid_pruning_above_them(dev):
    v, f = M.strip_mesh(130)
    v[71, 1] = 2.0 ** -10                                                # face (70, 71, 72): base 1, height 2^-10, so (h / L)^2 = 2^-20 <= 2^-16
    tree = _mt().mesh_tree_dev(_t(v, dev), _t(f, dev, torch.int32))
    got, ref = _node_table(tree), M.build(v, f)
    assert np.array_equal(got["noprune"], ref["noprune"]) and got["noprune"].any() and not got["noprune"].all() and got["noprune"][-1]


# ---- exact distance -------------------------------------------------------------------------------------------------------------------------

def _same_as_brute(dev, q, v, f, qoff=None, voff=None, toff=None, beta=2.0):
    MS, MT = _ms(), _mt()
    qd, vd, fd = _t(q, dev), _t(v, dev), _t(f, dev, torch.int32)
    S0, I0, C0, W0, st0 = MS.signed_distance_dev(qd, vd, fd, qoff, voff, toff, return_winding=True)
    tree = MT.mesh_tree_dev(vd, fd, voff, toff)
    S1, I1, C1, W1, st1 = MT.signed_distance_tree_dev(qd, tree, qoff, beta=beta, return_winding=True)
    assert st0.cpu().tolist() == st1.cpu().tolist()
    assert np.array_equal(_bits(S0.abs()), _bits(S1.abs())), "sqrt(d2) differs from the brute route"
    assert np.array_equal(I0.cpu().numpy(), I1.cpu().numpy()), "the closest face differs from the brute route"
    assert np.array_equal(_bits(C0), _bits(C1)), "the closest point differs from the brute route"
    return (S0.cpu().numpy(), W0.cpu().numpy()), (S1.cpu().numpy(), W1.cpu().numpy()), tree


def test_exact_distance_random_soups(dev):
    rs = np.random.RandomState(0)
    for n_tri, n_q in [(40, 700), (333, 1500), (2100, 1000)]:           # 45 faces: one leaf that is the root; 700: not a multiple of 64
        v, f = _soup(rs, n_tri, scale=0.5)                               # duplicated and degenerate faces inside
        _same_as_brute(dev, _queries(rs, v, n_q), v, f)
        _same_as_brute(dev, v[rs.randint(0, len(v), 257)], v, f)         # queries on vertices: d = 0
        far = (rs.choice([-1.0, 1.0], (130, 3)) * rs.uniform(50, 100, (130, 3))).astype(np.float32)
        (S0, _), (S1, W1), _ = _same_as_brute(dev, far, v, f)            # far outside: the root is admissible
        assert (S1 > 0).all() and np.abs(W1).max() < 1e-3


def test_exact_distance_cube_ties_take_the_lowest_original_index(dev):
    c = R.CUBE_V.astype(np.float32)
    edges = np.array([(c[i] + c[j]) / 2 for i in range(8) for j in range(i) if np.abs(c[i] - c[j]).sum() == 2], np.float32)
    q = np.concatenate([np.zeros((1, 3), np.float32), edges, edges * 1.5, c, c * 2, np.eye(3, dtype=np.float32) * 0.5])
    _, _, tree = _same_as_brute(dev, q, c, R.CUBE_F)
    I = _mt().signed_distance_tree_dev(_t(q, dev), tree)[1].cpu().numpy()
    assert I[0] == 0                                                     # the centre is equally far from all 12 faces


def test_exact_distance_on_a_fixture_translated_by_64(dev):
    """the pruning margin under coarse rounding: at x ~ 64 an f32 ulp is 7.6e-6, the face routine's differences are that coarse"""
    rs = np.random.RandomState(5)
    v, f = M.sphere()
    v = (v + np.array([64, 0, 0], np.float32)).astype(np.float32)
    near = v[rs.randint(0, len(v), 1200)] + (rs.randn(1200, 3) * 0.01).astype(np.float32)
    mid = v[rs.randint(0, len(v), 400)] + (rs.randn(400, 3) * 0.3).astype(np.float32)
    _same_as_brute(dev, np.concatenate([near, mid]).astype(np.float32), v, f)
    v0, f0 = M.bowl()
    _same_as_brute(dev, (v0[rs.randint(0, len(v0), 900)] + (rs.randn(900, 3) * 0.02)).astype(np.float32), v0, f0)


# ---- winding ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sphere", "bowl"])
def test_winding_is_the_reference_traversal_of_the_device_table(dev, name):
    rs = np.random.RandomState(7)
    v, f = getattr(M, name)()
    q = np.concatenate([rs.uniform(-1, 1, (800, 3)), v[rs.randint(0, len(v), 400)] + rs.randn(400, 3) * 0.03]).astype(np.float32)
    tree = _mt().mesh_tree_dev(_t(v, dev), _t(f, dev, torch.int32))
    nt = _node_table(tree)
    order = tree.order.cpu().numpy()
    P = v[f[order]]
    wt = tree.rec.cpu().numpy().reshape(-1, 5, 4)[:, 3, 3]
    worst = 0.0
    for beta in (2.0, 3.0):
        cnt = torch.zeros(3, device=dev, dtype=torch.int64)
        W = _mt().signed_distance_tree_dev(_t(q, dev), tree, beta=beta, return_winding=True, counters=cnt)[3].cpu().numpy()
        c = {}
        want = M.winding(q, P, wt, M.level_nodes(len(f)), nt["p"], nt["r"], nt["dip"], nt["coef"], beta, c)
        err = np.abs(W - want).max()
        worst = max(worst, err)
        print(f"{name} beta {beta}: max |W_tree(device) - W_tree(f64)| = {err:.3e}")
        assert err <= W_TOL
        assert cnt[1].item() == c["approx"].sum() and cnt[2].item() == len(q)          # the same branches
    assert worst > 0


# ---- occupancy ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [17, 33])
def test_occupancy_is_the_brute_routes_outside_the_band(dev, G):
    MS, MT = _ms(), _mt()
    meshes = [M.sphere(), _mc_torus(), M.bowl()]
    names = ["sphere", "sphere", "bowl"]                                 # the torus takes the sphere's (larger) recorded error: it is closed
    v, f, voff, toff = _batch(meshes, dev)
    brute = MS.mesh_occupancy_dev(v, f, voff, toff, grid_dim=G).cpu().numpy()
    q = _t(np.tile(M.lattice(G), (3, 1)), dev)
    Wb = MS.signed_distance_dev(q, v, f, np.arange(4) * G ** 3, voff, toff, return_winding=True)[3].cpu().numpy().reshape(3, -1)
    tree = MT.mesh_tree_dev(v, f, voff, toff)
    for beta in (2.0, 3.0):
        occ, st = MT.mesh_occupancy_tree_dev(tree, grid_dim=G, beta=beta, return_status=True)
        assert st.cpu().tolist() == [0, 0, 0] and occ.shape == (3, G, G, G) and occ.dtype == torch.uint8
        occ = occ.cpu().numpy()
        for b in range(3):
            differs = (occ[b] != brute[b]).reshape(-1)
            if b < 2:
                assert not differs.any(), f"closed fixture {b}, beta {beta}: {differs.sum()} lattice points differ"
            else:
                band = np.abs(np.abs(Wb[b]) - 0.5) <= 4 * RECORDED[names[b], beta]
                assert not differs[~band].any()
            assert 0 < occ[b].sum() < G ** 3
        # the lattice form and the free-query form are one walk: the same W, so the same inside test
        S = MT.signed_distance_tree_dev(q, tree, np.arange(4) * G ** 3, beta=beta)[0].cpu().numpy()
        assert np.array_equal(S < 0, occ.reshape(-1).astype(bool))


# ---- determinism --------------------------------------------------------------------------------------------------------------------------------

def _run_all(dev, meshes, queries, G=9, beta=2.0):
    MT = _mt()
    v, f, voff, toff = _batch(meshes, dev)
    qoff = np.concatenate([[0], np.cumsum([len(x) for x in queries])])
    tree = MT.mesh_tree_dev(v, f, voff, toff)
    S, I, C, W, st = MT.signed_distance_tree_dev(_t(np.concatenate(queries), dev), tree, qoff, beta=beta, return_winding=True)
    occ = MT.mesh_occupancy_tree_dev(tree, grid_dim=G, beta=beta)
    cut = lambda x: [_bits(x)[qoff[b]:qoff[b + 1]] for b in range(len(meshes))]
    return dict(S=cut(S), I=cut(I), C=cut(C), W=cut(W), occ=[o for o in occ.cpu().numpy()], nodes=_bits(tree.nodes), mom=tree.mom.cpu().numpy())


def test_determinism_runs_batches_and_query_order(dev):
    rs = np.random.RandomState(11)
    meshes = [(R.CUBE_V.astype(np.float32) * 0.5, R.CUBE_F.astype(np.int32)), _mc_torus(), M.sphere()]       # depths 1, 3 and 4
    queries = [rs.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (70, 333, 200)]
    a, b = _run_all(dev, meshes, queries), _run_all(dev, meshes, queries)
    for k in ("S", "I", "C", "W", "occ"):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k          # run twice, bitwise
    assert np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["mom"].view(np.int64), b["mom"].view(np.int64))
    for i in range(3):                                                           # a batch equals per-shape calls
        one = _run_all(dev, [meshes[i]], [queries[i]])
        for k in ("S", "I", "C", "W", "occ"):
            assert np.array_equal(a[k][i], one[k][0]), (k, i)
    perm = [rs.permutation(len(x)) for x in queries]                             # two orders of the queries: the same bits per query
    c = _run_all(dev, meshes, [x[p] for x, p in zip(queries, perm)])
    for k in ("S", "I", "C", "W"):
        assert all(np.array_equal(a[k][i][perm[i]], c[k][i]) for i in range(3)), k


def test_wide_batch_of_261_sets_equals_per_set_calls(dev):
    import wide_batch as WB
    MT = _mt()
    layout = WB.LAYOUTS["wide"]
    members = WB.mesh_members()
    rs = np.random.RandomState(13)
    mq = [np.concatenate([v[rs.randint(0, len(v), 12)] + rs.randn(12, 3).astype(np.float32) * 0.05,
                          rs.uniform(-1, 1, (12, 3)).astype(np.float32)]).astype(np.float32) for v, _ in members]
    alone = []
    for (v, f), q in zip(members, mq):
        tree = MT.mesh_tree_dev(_t(v, dev), _t(f, dev, torch.int32))
        out = MT.signed_distance_tree_dev(_t(q, dev), tree, return_winding=True)
        alone.append([_bits(x) for x in out[:4]] + [MT.mesh_occupancy_tree_dev(tree, grid_dim=6).cpu().numpy()[0]])
    mem = layout.members()
    vs, fs, qs = [], [], []
    for m in mem:
        vs.append(members[m][0] if m >= 0 else np.zeros((0, 3), np.float32))
        fs.append(members[m][1] if m >= 0 else np.zeros((0, 3), np.int32))
        qs.append(mq[m] if m >= 0 else np.zeros((0, 3), np.float32))
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    voff, toff, qoff = off(vs), off(fs), off(qs)
    tree = MT.mesh_tree_dev(_t(np.concatenate(vs), dev), _t(np.concatenate(fs), dev, torch.int32), voff, toff)
    status = tree.status.cpu().numpy()
    assert np.array_equal(status, np.where(mem < 0, 1, 0))
    out = [_bits(x) for x in MT.signed_distance_tree_dev(_t(np.concatenate(qs), dev), tree, qoff, return_winding=True)[:4]]
    for b, m in enumerate(mem):
        for k in range(4):
            assert m < 0 or np.array_equal(out[k][qoff[b]:qoff[b + 1]], alone[m][k]), (b, k)
    full = np.nonzero(mem >= 0)[0]                                               # the occupancy form refuses empty shapes
    voff2, toff2 = off([vs[b] for b in full]), off([fs[b] for b in full])
    tree2 = MT.mesh_tree_dev(_t(np.concatenate(vs), dev), _t(np.concatenate(fs), dev, torch.int32), voff2, toff2)
    occ = MT.mesh_occupancy_tree_dev(tree2, grid_dim=6).cpu().numpy()
    for i, b in enumerate(full):
        assert np.array_equal(occ[i], alone[mem[b]][4]), b


# ---- status codes and the reference's signatures ------------------------------------------------------------------------------------------------

def test_status_codes(dev):
    MT = _mt()
    rs = np.random.RandomState(4)
    v0, f0 = R.CUBE_V.astype(np.float32), R.CUBE_F.copy()
    f_bad = R.CUBE_F.copy()
    f_bad[5, 1] = 8                                                              # outside the 8 vertices of its shape
    v_nan = v0.copy()
    v_nan[3, 1] = np.nan
    v = np.concatenate([v0, v0, v0, v_nan])
    f = np.concatenate([f0, f_bad, f0, f0])
    voff, toff = np.array([0, 8, 16, 24, 32]), np.array([0, 12, 24, 36, 48])
    q = rs.uniform(-2, 2, (400, 3)).astype(np.float32)
    qoff = np.array([0, 100, 200, 300, 400])
    tree = MT.mesh_tree_dev(_t(v, dev), _t(f, dev, torch.int32), voff, toff)
    S, I, C, W, st = MT.signed_distance_tree_dev(_t(q, dev), tree, qoff, return_winding=True)
    assert st.cpu().tolist() == [0, 2, 0, 3]
    S, I, C, W = S.cpu().numpy(), I.cpu().numpy(), C.cpu().numpy(), W.cpu().numpy()
    for s in (slice(100, 200), slice(300, 400)):
        assert np.isnan(S[s]).all() and (I[s] == -1).all() and np.isnan(C[s]).all() and (W[s] == 0).all()
    box = R.box_sdf(q.astype(np.float64))
    assert np.abs(S[:100] - box[:100]).max() < 1e-6 and np.abs(S[200:300] - box[200:300]).max() < 1e-6
    occ, st = MT.mesh_occupancy_tree_dev(tree, grid_dim=8, return_status=True)
    assert st.cpu().tolist() == [0, 2, 0, 3] and occ[1].sum().item() == 0 and occ[3].sum().item() == 0 and occ[0].sum().item() > 0
    # a shape without faces and without queries is admitted: status 1
    tree = MT.mesh_tree_dev(_t(np.concatenate([v0, v0]), dev), _t(f0, dev, torch.int32), [0, 8, 16], [0, 0, 12])
    S, _, _, st = MT.signed_distance_tree_dev(_t(q[:100], dev), tree, [0, 0, 100])
    assert st.cpu().tolist() == [1, 0] and np.abs(S.cpu().numpy() - box[:100]).max() < 1e-6


def test_strided_and_retyped_inputs_give_the_canonical_bits(dev):
    """_ragged.py's contract for a public entry point: a strided view, a float64 cloud, int64 faces and offsets in any integer form give
    the bits of the canonical call"""
    MT = _mt()
    rs = np.random.RandomState(9)
    v, f = _soup(rs, 150, scale=0.5)
    q = _queries(rs, v, 300)
    tree = MT.mesh_tree_dev(_t(v, dev), _t(f, dev, torch.int32), [0, len(v)], [0, len(f)])
    want = MT.signed_distance_tree_dev(_t(q, dev), tree, return_winding=True)
    wide = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.repeat(x, 2, axis=1))).to(dev, dt)[:, ::2]
    tree2 = MT.mesh_tree_dev(wide(v, torch.float64), wide(f, torch.int64), torch.tensor([0, len(v)], dtype=torch.int32), np.array([0, len(f)], np.int16))
    assert np.array_equal(_bits(tree.nodes), _bits(tree2.nodes)) and np.array_equal(_bits(tree.rec), _bits(tree2.rec))
    got = MT.signed_distance_tree_dev(wide(q, torch.float64), tree2, torch.tensor([0, len(q)]), beta=2, return_winding=True)
    for a, b in zip(want, got):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(MT.mesh_occupancy_tree_dev(tree, 9).cpu().numpy(), MT.mesh_occupancy_tree_dev(tree2, np.int64(9), beta=2).cpu().numpy())


def test_reference_signatures_take_method_tree(dev):
    MS = _ms()
    v, f = R.icosphere(3, r=0.7)
    rs = np.random.RandomState(3)
    q = rs.uniform(-1, 1, (999, 3))
    a, b = MS.signed_distance(q, v, f, method="brute"), MS.signed_distance(q, v, f, method="tree")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])          # a closed mesh: S bitwise
    a, b = MS.mesh2sdf(v, f, gridDim=12, method="brute"), MS.mesh2sdf(v, f, gridDim=12, method="tree")
    assert np.array_equal(a, b) and a.shape == (12 ** 3, 4) and (a[:, 3] < 0).any()


def test_make_dataset_winding_tree_writes_the_same_store(dev, tmp_path):
    from shapeformer_amd import make_dataset as MD, meshio
    v, f = R.icosphere(3, r=3.0)
    meshio.write_ply(str(tmp_path / "a.ply"), v, f)
    tv, tf = _mc_torus()
    meshio.write_ply(str(tmp_path / "b.ply"), tv.astype(np.float64), tf)
    paths = [str(tmp_path / "a.ply"), str(tmp_path / "b.ply")]
    for w in ("brute", "tree"):
        MD.main(paths + ["--out", str(tmp_path / w), "--dataset", "d", "--grid", "16", "--boundary-n", "512", "--winding", w, "--beta", "2"])
    a, b = (np.load(tmp_path / w / "d" / "train" / "Ytg.npy") for w in ("brute", "tree"))
    assert a.shape == (2, 16 ** 3 // 8) and np.array_equal(a, b) and np.unpackbits(a[1]).sum() > 0


# ---- IoU --------------------------------------------------------------------------------------------------------------------------------------------

def test_mesh_iou(dev):
    MT = _mt()
    G = 24
    big, small = R.icosphere(3, r=0.8), R.icosphere(3, r=0.5)
    shifted = (small[0] * 0.4 + np.array([0.7, 0.7, 0.7]), small[1])                # radius 0.2 about (0.7, 0.7, 0.7): outside r = 0.5
    A = _batch([big, big, small], dev)
    Bm = _batch([big, small, shifted], dev)
    for method in ("tree", "brute"):
        iou = MT.mesh_iou_dev(*A, *Bm, grid_dim=G, method=method).cpu().numpy()
        ob, osm = (_ms().mesh_occupancy_dev(*_batch([m], dev), grid_dim=G).cpu().numpy().astype(bool) for m in (big, small))
        assert iou.dtype == np.float64 and iou[0] == 1.0 and iou[2] == 0.0
        assert iou[1] == (ob & osm).sum() / (ob | osm).sum() and 0 < iou[1] < 1 and (osm <= ob).all()        # concentric: the ratio of the counts
    z = torch.zeros(2, G, G, G, device=dev, dtype=torch.uint8)
    assert torch.isnan(MT.volumetric_iou_dev(z, z)).all()                            # empty against empty
    tiny = (small[0] * 1e-3 + 0.03, small[1])                                        # between the lattice points: empty occupancy
    assert np.isnan(MT.mesh_iou_dev(*_batch([tiny], dev), *_batch([tiny], dev), grid_dim=G).cpu().numpy()).all()
