"""Coarse-to-fine sparse iso-surface extraction, CPU side: the numpy reference of the contract (tests/iso_sparse_ref.py)
against the marching-cubes oracle, and the Python-side argument validation.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_sparse_ref as R   # noqa: E402


@pytest.mark.parametrize("name,margin", [("sphere", 0), ("sphere", 1), ("slab", 0), ("open", 1)])
def test_full_coverage_selection_reproduces_the_oracle_mesh(name, margin):
    """Where the hierarchy reaches every cut cell, selecting out of the oracle's dense mesh is the identity."""
    from oracle import mc_oracle as MO
    Q0, L = 5, 2
    F = R.field(name, 17)
    h = R.hierarchy(F, Q0, L, 0.5, margin)
    assert h["final"].sum() > 0 and np.array_equal(h["final"], R.dense_cut_cells(F, 0.5))
    assert len(h["S"][0]) == (Q0 - 1) ** 3 and h["points"][0] == Q0 ** 3
    for l in range(L + 1):
        assert np.all(np.diff(h["S"][l]) > 0) and np.isin(h["M"][l], h["S"][l]).all()
    v, f = MO.marching_cubes(F, 0.5)
    vs, ts, fn = R.select_mesh(F, 0.5, h["final"], len(v), f)
    assert np.array_equal(vs, np.arange(len(v))) and np.array_equal(ts, np.arange(len(f))) and np.array_equal(fn, f)


def test_restricted_selection_is_a_strict_subset_closed_under_its_cells():
    """`two` at (9,3), margin 0: the small sphere's cut cells are not all reached; margin 1 reaches them all."""
    from oracle import mc_oracle as MO
    F = R.field("two", 65)
    dense = R.dense_cut_cells(F, 0.5)
    h0, h1 = R.hierarchy(F, 9, 3, 0.5, 0), R.hierarchy(F, 9, 3, 0.5, 1)
    assert np.array_equal(h1["final"], dense)
    assert 0 < h0["final"].sum() < dense.sum() and not (h0["final"] & ~dense).any()
    assert sum(h0["points"]) < 65 ** 3 and sum(h1["points"]) < 65 ** 3
    v, f = MO.marching_cubes(F, 0.5)
    vs, ts, fn = R.select_mesh(F, 0.5, h0["final"], len(v), f)       # asserts closedness: selected faces use selected vertices only
    assert 0 < len(ts) < len(f) and 0 < len(vs) <= len(v)            # fewer triangles; a missed cell may share all its edges
    assert np.all(np.diff(vs) > 0) and np.all(np.diff(ts) > 0)
    assert np.array_equal(np.unique(fn), np.arange(len(vs)))         # and every selected vertex is used
    assert np.array_equal(v[vs][fn], v[f[ts]])                       # the same triangles, corner for corner


def test_python_side_argument_validation():
    from shapeformer_amd import iso_sparse as IS
    from shapeformer_amd._lib import SfmiError
    assert IS.lattice_levels(65, 17) == 2 and IS.lattice_levels(257, 33) == 3 and IS.lattice_levels(513, 33) == 4
    assert IS.lattice_levels(3, 2) == 1
    with pytest.raises(SfmiError, match="nearest valid res = 129"):
        IS.lattice_levels(128, 33)
    with pytest.raises(SfmiError, match="nearest valid res = 257"):
        IS.lattice_levels(256, 33)
    with pytest.raises(SfmiError, match="nearest valid res"):
        IS.lattice_levels(33, 33)                                    # L >= 1
    with pytest.raises(SfmiError, match="nearest valid res = 1033"):
        IS.lattice_levels(1291, 130)
    with pytest.raises(SfmiError, match=r"2\^31"):
        IS.lattice_levels(1291, 646)                                 # 1291 = 645 * 2 + 1 fits the rule, but 1291^3 >= 2^31
    with pytest.raises(SfmiError):
        IS.lattice_levels(9, 1)
    field = lambda keys, koff: None
    with pytest.raises(SfmiError, match="margin"):
        IS.extract_sparse_dev(field, 1, 5, 2, margin=2)
    with pytest.raises(SfmiError, match="margin"):
        IS.extract_sparse_dev(field, 1, 5, 2, margin=-1)
    with pytest.raises(SfmiError):
        IS.extract_sparse_dev(field, 1, 5, 0)
    with pytest.raises(SfmiError):
        IS.extract_sparse_dev(field, 1, 1, 2)
    with pytest.raises(SfmiError):
        IS.extract_sparse_dev(field, 1, 646, 1)                      # Q = 1291
