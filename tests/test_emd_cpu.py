"""CPU tests of the earth mover's distance: the exported symbols, tests/emd_ref.py against an exact solver on the f64
costs the kernel uses, the set-level metrics against hand-made matrices, and every argument refusal (raised before the library loads).

The bound of every comparison with an exact solver is Bertsekas' for epsilon-complementary slackness, 0 <= emd - emd_opt <= eps_final,
plus 1e-12 diag for the two f64 sums: derived, not measured."""
import itertools
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import emd_ref as R
from shapeformer_amd import _lib as L
from shapeformer_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sfmi_emd_resident_max", "sfmi_emd_max_points", "sfmi_emd_default_cap", "sfmi_emd_default_chunk", "sfmi_emd_workspace_bytes",
       "sfmi_emd_f32")


def test_symbols_exported_declared_bound():
    import ctypes
    from shapeformer_amd import build as B
    B.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    declared = set(re.findall(r"\b(sfmi_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.PROTOTYPES and hasattr(lib, name), name
    lib.sfmi_emd_workspace_bytes.restype = ctypes.c_size_t
    lib.sfmi_emd_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_longlong]
    assert lib.sfmi_emd_resident_max() == 2048 and lib.sfmi_emd_max_points() == R.N_MAX == M.EMD_MAX_POINTS
    assert lib.sfmi_emd_default_cap(257) == R.default_cap(257)
    assert lib.sfmi_emd_workspace_bytes(0, 10) == 0 and lib.sfmi_emd_workspace_bytes(3, 0) > 0
    assert lib.sfmi_emd_workspace_bytes(4, 8192) >= 28 * 8192        # owner, list, the bids and B's coordinates as three arrays
    for name in ("emd_dev", "emd", "pairwise_chamfer_dev", "pairwise_emd_dev", "set_metrics", "metrics_from_matrices"):
        assert callable(getattr(M, name))


def test_fmaf32_is_the_fused_operation():
    """against exact rational arithmetic on operands picked to make the f64 sum inexact"""
    from fractions import Fraction
    rs = np.random.RandomState(0)
    a = (rs.randn(2000) * 10.0 ** rs.randint(-12, 12, 2000)).astype(np.float32)
    b = (rs.randn(2000) * 10.0 ** rs.randint(-12, 12, 2000)).astype(np.float32)
    c = (rs.randn(2000) * 10.0 ** rs.randint(-12, 12, 2000)).astype(np.float32)
    got = R.fmaf32(a, b, c)
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
        assert abs(exact - Fraction(g)) <= abs(exact - Fraction(float(lo))) and abs(exact - Fraction(g)) <= abs(exact - Fraction(float(hi)))


def _cases():
    out = {f"shell_{n}": (R.shell(n, 10 + n), R.shell(n, 500 + n)) for n in (1, 2, 3, 63, 64, 65, 257)}
    out.update(R.families())
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_within_eps_of_exact_solver(name):
    A, B = CASES[name]
    n = len(A)
    C = R.cost_matrix(A, B)
    o = R.auction(A, B, C=C)
    r, c = linear_sum_assignment(C)
    opt = float(C[r, c].sum()) / n
    diag = R.diag_of(A, B)
    gap = o["emd"] - opt
    print(f"{name}: n {n} rounds {o['rounds']} ({o['rounds'] / n:.2f} n) bids {o['bids']} gap / eps_final {gap / o['eps_final']:.4f}")
    assert o["status"] == 0 and sorted(o["assign"].tolist()) == list(range(n))
    assert o["eps_final"] == 1e-4 * diag
    assert -1e-12 * diag <= gap <= o["eps_final"] + 1e-12 * diag
    assert o["rounds"] <= R.default_cap(n) // 16                   # the default cap keeps its factor of 16 over every family here


def test_exact_optimum_at_small_n():
    """n = 2..7, eps_rel = 1e-6: wherever n eps_final is below the gap between the best and the second best permutation, an assignment
    within n eps_final of the optimum (total cost) is the optimum itself"""
    rs = np.random.RandomState(7)
    decided = 0
    for n in range(2, 8):
        perms = np.array(list(itertools.permutations(range(n))))
        for _ in range(40):
            A, B = rs.rand(n, 3).astype(np.float32), rs.rand(n, 3).astype(np.float32)
            C = R.cost_matrix(A, B)
            tot = C[np.arange(n)[None, :], perms].sum(1)
            order = np.argsort(tot, kind="stable")
            gap = tot[order[1]] - tot[order[0]]
            o = R.auction(A, B, eps_rel=1e-6, C=C)
            assert o["status"] == 0
            if n * o["eps_final"] < gap:
                decided += 1
                assert o["assign"].tolist() == perms[order[0]].tolist()
    assert decided >= 200


def test_round_cap():
    A, B = CASES["shell_257"]
    o = R.auction(A, B, max_rounds=3)
    assert o["status"] == 1 and o["rounds"] == 3 and np.isnan(o["emd"])
    a = o["assign"]
    assert (a == -1).any() and (a >= -1).all()
    owned = a[a >= 0]
    assert len(set(owned.tolist())) == len(owned)                  # the partial assignment is still one to one


def test_degenerate_pairs():
    o = R.auction(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert o["status"] == 0 and np.isnan(o["emd"]) and len(o["assign"]) == 0
    same = np.tile(np.float32([[0.25, -1.0, 3.0]]), (5, 1))
    o = R.auction(same, same)
    assert o["status"] == 0 and o["emd"] == 0.0 and o["rounds"] == 0 and o["assign"].tolist() == list(range(5))
    bad = R.shell(9, 1)
    bad[4, 1] = np.nan
    o = R.auction(R.shell(9, 2), bad)
    assert o["status"] == 2 and np.isnan(o["emd"]) and (o["assign"] == -1).all()


def test_fixed_sum_is_a_sum():
    x = np.random.RandomState(3).rand(2500)
    assert abs(R.fixed_sum(x) - x.sum()) <= 2500 * 2.0 ** -52 * x.sum()
    assert R.fixed_sum([1.5]) == 1.5


# ---- set-level metrics ----------------------------------------------------------------------------------------------------------------

def test_set_metrics_by_hand_with_ties():
    # 3 generated, 4 reference.  Row 0 ties between references 1 and 2 (the lower wins), rows 1 and 2 both pick reference 0
    D_gr = np.array([[5.0, 1.0, 1.0, 9.0],
                     [2.0, 3.0, 4.0, 9.0],
                     [2.0, 8.0, 8.0, 7.0]])
    assert R.mmd(D_gr) == (2.0 + 1.0 + 1.0 + 7.0) / 4
    assert R.cov(D_gr) == 2 / 4
    D_gg = np.array([[0.0, 6.0, 6.0], [6.0, 0.0, 1.0], [6.0, 1.0, 0.0]])
    D_rr = np.array([[0.0, 2.0, 9.0, 9.0], [2.0, 0.0, 0.5, 9.0], [9.0, 0.5, 0.0, 9.0], [9.0, 9.0, 9.0, 0.0]])
    # nearest neighbours in the union (g0 g1 g2 r0 r1 r2 r3): g0 -> r1 (1.0, tie with r2: lower index), g1 -> g2, g2 -> g1,
    # r0 -> g1 (2.0, tie with g2 and r1: lowest index), r1 -> r2, r2 -> r1, r3 -> g2 (7.0)
    assert R.one_nna(D_gg, D_gr, D_rr) == 4 / 7
    t = lambda a: torch.from_numpy(a)
    got = M.metrics_from_matrices(t(D_gr), t(D_gg), t(D_rr))
    assert got == {"mmd": R.mmd(D_gr), "cov": 0.5, "1nna": 4 / 7}


def test_set_metrics_random_matrices_match_numpy():
    rs = np.random.RandomState(5)
    for G, Rn in ((1, 1), (5, 4), (7, 12)):
        D_gr = rs.randint(0, 6, (G, Rn)).astype(np.float64)         # small integers: many ties
        D_gg = rs.randint(1, 6, (G, G)).astype(np.float64)
        D_gg = np.triu(D_gg, 1) + np.triu(D_gg, 1).T
        D_rr = rs.randint(1, 6, (Rn, Rn)).astype(np.float64)
        D_rr = np.triu(D_rr, 1) + np.triu(D_rr, 1).T
        got = M.metrics_from_matrices(torch.from_numpy(D_gr), torch.from_numpy(D_gg), torch.from_numpy(D_rr))
        assert got["mmd"] == pytest.approx(R.mmd(D_gr), rel=1e-15)
        assert got["cov"] == R.cov(D_gr) and got["1nna"] == pytest.approx(R.one_nna(D_gg, D_gr, D_rr), rel=1e-15)


# ---- refusals: all on the host, before the library loads ------------------------------------------------------------------------------

def test_refusals(monkeypatch):
    monkeypatch.setattr(L, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    E = L.SfmiError
    a, b = torch.zeros(6, 3), torch.zeros(6, 3)
    with pytest.raises(E, match="equal sizes"):
        M.emd_dev(a, torch.zeros(5, 3))
    with pytest.raises(E, match="equal sizes"):
        M.emd_dev(a, b, [0, 2, 6], [0, 3, 6])
    with pytest.raises(E, match="need `pairs`"):
        M.emd_dev(a, b, [0, 2, 6], [0, 6])
    with pytest.raises(E, match="more than 8192"):
        M.emd_dev(torch.zeros(8193, 3), torch.zeros(8193, 3))
    for bad in (0.0, 1e-10, 1.5, float("nan"), True, "x"):
        with pytest.raises(E, match="eps_rel"):
            M.emd_dev(a, b, eps_rel=bad)
    for name in ("max_rounds", "chunk_rounds"):
        for bad in (0, -1, 2.5, True):
            with pytest.raises(E, match=name):
                M.emd_dev(a, b, **{name: bad})
    with pytest.raises(E, match=r"\(P,2\)"):
        M.emd_dev(a, b, pairs=[0, 0])
    with pytest.raises(E, match=r"\(P,2\)"):
        M.emd_dev(a, b, pairs=np.zeros((1, 2)))
    with pytest.raises(E, match="outside its collection"):
        M.emd_dev(a, b, pairs=[[0, 1]])
    with pytest.raises(E, match="outside its collection"):
        M.emd_dev(a, b, pairs=[[-1, 0]])
    with pytest.raises(E, match="offsets"):
        M.emd_dev(a, b, [0, 7], None)
    with pytest.raises(E, match="offsets go with"):
        M.emd_dev(torch.zeros(2, 3, 3), torch.zeros(2, 3, 3), [0, 6], None)
    with pytest.raises(E, match="offsets go with"):
        M.emd_dev([a], [b], [0, 6], None)
    with pytest.raises(E, match="list"):
        M.emd_dev([], [b])
    with pytest.raises(E, match=r"\(N,3\)"):
        M.emd_dev(torch.zeros(6, 2), b)
    with pytest.raises(E, match="torch tensor"):
        M.emd_dev(np.zeros((6, 3)), b)
    with pytest.raises(E, match="HIP device"):
        M.emd_dev(a, b)                                            # every host check passed: the device is the last one
    with pytest.raises(E, match="HIP device"):
        M.emd(a, b)
    with pytest.raises(E, match="HIP device"):
        M.pairwise_chamfer_dev([a, b])
    with pytest.raises(E, match="equal sizes"):
        M.pairwise_emd_dev([a, torch.zeros(5, 3)])
    with pytest.raises(E, match="HIP device"):
        M.pairwise_emd_dev([a, b], [a])
    with pytest.raises(E, match="metric"):
        M.set_metrics([a], [b], metric="l2")
    with pytest.raises(E, match="go with metric"):
        M.set_metrics([a], [b], metric="cd", eps_rel=1e-3)
    with pytest.raises(E, match="matrices"):
        M.metrics_from_matrices(torch.zeros(2, 3), torch.zeros(2, 2), torch.zeros(2, 2))
    with pytest.raises(E, match="emd_n"):
        M.evaluate(a, [b], Xbd=a, emd_n=0)
    with pytest.raises(E, match="emd_n"):
        M.evaluate(a, [b], Xbd=a, emd_n=8193)
    with pytest.raises(E, match="needs the full shape"):
        M.evaluate(a, [b], emd_n=4)
