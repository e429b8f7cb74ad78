"""GPU tests of the earth mover's distance (shapeformer_amd/metrics.py emd_dev, csrc/emd.hip) against tests/emd_ref.py.
Parity is ==: assign, rounds, status, the prices, eps_final and emd bit for bit.  Comparisons with an exact solver or a known optimum use
Bertsekas' bound 0 <= emd - emd_opt <= eps_final, which is derived, not measured.  Every size is the smallest at which its mechanism can
fail; the references of the parity cases are computed once."""
import numpy as np
import pytest
import torch

import emd_ref as R
import wide_batch as W
from shapeformer_amd import _lib as L
from shapeformer_amd import metrics as M

pytestmark = pytest.mark.gpu

N_RES = 2048


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(A, B, dev, **kw):
    e, d = M.emd_dev(_t(A, dev), _t(B, dev), details=True, **kw)
    torch.cuda.synchronize()
    r = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    r["emd"] = e.cpu().numpy()
    return r


def _same(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_equals_ref(got, ref, k=0, lo=None, hi=None):
    lo = 0 if lo is None else lo
    hi = len(ref["assign"]) if hi is None else hi
    assert int(got["status"][k]) == ref["status"] and int(got["rounds"][k]) == ref["rounds"]
    assert _same(got["assign"][lo:hi], ref["assign"])
    assert _same(got["price"][lo:hi], np.asarray(ref["price"], np.float64))
    assert _same(got["eps_final"][k], np.float64(ref["eps_final"]))
    assert _same(got["emd"][k], np.float64(ref["emd"]))


def _parity_cases():
    out = {f"shell_{n}": (R.shell(n, 10 + n), R.shell(n, 500 + n)) for n in (1, 2, 63, 64, 65, 257, 1025)}
    fam = R.families()
    for name in ("lattice_reversed", "lattice_half_cell", "repeated_8x", "collinear_mirror"):
        out[name] = fam[name]
    return out


PARITY = _parity_cases()
_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = R.auction(*PARITY[name])
    return _REF[name]


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_with_reference(dev, name):
    """n = 1, 2; a wave and its edges; 257; 1025 starts above EMD_LANE_MIN (one lane per bidder), passes through one wave per bidder
    and ends in the shared scans of the tail.  The lattice, duplicate and collinear families (512 points) meet every tie rule."""
    A, B = PARITY[name]
    ref = _ref(name)
    assert ref["status"] == 0
    got = _run(A, B, dev)
    _assert_equals_ref(got, ref)
    assert sorted(got["assign"].tolist()) == list(range(len(A)))


def test_bound_against_exact_solver_2048(dev):
    from scipy.optimize import linear_sum_assignment
    A, B = R.shell(2048, 31), R.shell(2048, 32)
    C = R.cost_matrix(A, B)
    r, c = linear_sum_assignment(C)
    opt = float(C[r, c].sum()) / 2048
    got = _run(A, B, dev)
    diag = R.diag_of(A, B)
    gap = float(got["emd"][0]) - opt
    print(f"n 2048: rounds {int(got['rounds'][0])} gap / eps_final {gap / float(got['eps_final'][0]):.4f}")
    assert int(got["status"][0]) == 0 and sorted(got["assign"].tolist()) == list(range(2048))
    assert got["eps_final"][0] == 1e-4 * diag
    assert float(got["emd"][0]) == pytest.approx(float(C[np.arange(2048), got["assign"]].sum()) / 2048, rel=1e-13)
    assert -1e-12 * diag <= gap <= got["eps_final"][0] + 1e-12 * diag


@pytest.mark.parametrize("n", [N_RES, N_RES + 1, 8192])
def test_known_optimum_of_a_shifted_permutation(dev, n):
    """B = a permutation of A + t: a bijection's mean cost is at least |mean(b) - mean(a)| = |t| (triangle inequality) and the
    permutation attains it, so emd_opt = |t| without a solver.  Slack for f32: A + t is rounded per coordinate by at most half an ulp
    of a value below 2, 2^-24, so a point moves by at most sqrt(3) 2^-24; a cost (difference, square, two fmaf, sqrtf: five roundings)
    is off by at most 5 x 2^-24 relative, and the costs of a matching near the optimum are below 1."""
    assert L.lib().sfmi_emd_resident_max() == N_RES
    A = R.shell(n, 900 + n)
    t = np.float32([0.3, 0.4, 0.0])                                # |t| = 0.5 in f64 up to f32 rounding: half of the shell's diameter
    B = (A + t).astype(np.float32)[np.random.RandomState(n).permutation(n)]
    tn = float(np.linalg.norm(t.astype(np.float64)))
    slack = np.sqrt(3) * 2.0 ** -24 + 5 * 2.0 ** -24
    got = _run(A, B, dev)
    print(f"n {n}: rounds {int(got['rounds'][0])} emd - |t| {float(got['emd'][0]) - tn:.3e} eps_final {float(got['eps_final'][0]):.3e}")
    assert int(got["status"][0]) == 0
    assert sorted(got["assign"].tolist()) == list(range(n))
    assert tn - slack <= float(got["emd"][0]) <= tn + float(got["eps_final"][0]) + slack


def test_result_does_not_depend_on_chunk_rounds(dev):
    A, B = PARITY["shell_257"]
    base = _run(A, B, dev)
    _assert_equals_ref(base, _ref("shell_257"))
    for kw in (dict(chunk_rounds=1), dict(chunk_rounds=7), dict()):   # the last: a second run of the default
        got = _run(A, B, dev, **kw)
        for key in ("assign", "price", "rounds", "status", "eps_final", "emd"):
            assert _same(got[key], base[key]), (kw, key)
    A, B = R.shell(N_RES + 1, 41), R.shell(N_RES + 1, 42)           # the streaming form keeps its state in the workspace
    base = _run(A, B, dev)
    assert int(base["status"][0]) == 0
    got = _run(A, B, dev, chunk_rounds=997)
    for key in ("assign", "price", "rounds", "status", "eps_final", "emd"):
        assert _same(got[key], base[key]), key


def test_batch_equals_per_pair_calls(dev):
    """70 pairs drawn from two collections of 12 clouds with repeated members and mixed sizes; one empty pair, one pair with a NaN
    coordinate, and max_rounds = 1000 cuts off the 257-point pairs (1444 rounds alone) and nobody else"""
    sizes = [0, 1, 2, 33, 33, 64, 65, 65, 130, 130, 257, 40]
    XA = [R.shell(n, 60 + k) for k, n in enumerate(sizes)]
    XB = [R.shell(n, 80 + k) for k, n in enumerate(sizes)]
    XB[11][7, 2] = np.nan
    ok = [(i, j) for i in range(12) for j in range(12) if sizes[i] == sizes[j] and (i == 11) == (j == 11)]
    rs = np.random.RandomState(0)
    pairs = ok + [ok[k] for k in rs.randint(0, len(ok), 70 - len(ok))]
    pairs = [pairs[k] for k in rs.permutation(70)]
    ao = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    a, b = _t(np.concatenate(XA), dev), _t(np.concatenate(XB), dev)
    e, d = M.emd_dev(a, b, ao, ao, pairs=np.asarray(pairs), max_rounds=1000, details=True)
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    got["emd"] = e.cpu().numpy()
    po = got["offsets"]
    assert po.tolist() == np.concatenate([[0], np.cumsum([sizes[i] for i, _ in pairs])]).tolist()
    alone = {}
    for k, (i, j) in enumerate(pairs):
        if (i, j) not in alone:
            alone[(i, j)] = _run(XA[i], XB[j], dev, max_rounds=1000)
        one = alone[(i, j)]
        for key in ("rounds", "status", "eps_final", "emd"):
            assert _same(got[key][k], one[key][0]), (k, i, j, key)
        for key in ("assign", "price"):
            assert _same(got[key][po[k]:po[k + 1]], one[key]), (k, i, j, key)
        want = 2 if i == 11 else (1 if sizes[i] == 257 else 0)
        assert int(got["status"][k]) == want, (k, i, j)
        if want:
            assert np.isnan(got["emd"][k])
        if want == 2:
            assert (got["assign"][po[k]:po[k + 1]] == -1).all()
        if sizes[i] == 0:
            assert np.isnan(got["emd"][k]) and int(got["rounds"][k]) == 0
    capped = got["assign"][po[pairs.index((10, 10))]:po[pairs.index((10, 10)) + 1]]
    assert (capped == -1).any() and (capped >= -1).all() and int(got["rounds"][pairs.index((10, 10))]) == 1000
    # the one pair of the batch that the reference also runs to its cap
    ref = R.auction(XA[10], XB[10], max_rounds=1000)
    _assert_equals_ref(alone[(10, 10)], ref)


@pytest.mark.parametrize("layout", ["wide", "sparse"])
def test_wide_batch_of_261_pairs(dev, layout):
    """set b of a against set b of b over tests/wide_batch.py's layouts: runs of empty pairs, members astride pair 256, more pairs
    than points"""
    lay = W.LAYOUTS[layout]
    sizes = W.POINT_SIZES if layout == "wide" else W.SPARSE_POINT_SIZES
    mem = [(W.cloud(n, 100 + m), W.cloud(n, 120 + m)) for m, n in enumerate(sizes)]
    member = lay.members()
    off = lay.offsets(sizes)
    cat = lambda which: np.concatenate([mem[m][which] for m in member if m >= 0] or [np.zeros((0, 3), np.float32)])
    e, d = M.emd_dev(_t(cat(0), dev), _t(cat(1), dev), off, off, details=True)
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    got["emd"] = e.cpu().numpy()
    assert got["offsets"].tolist() == off.tolist() and e.shape == (W.B,)
    alone = [_run(x, y, dev) for x, y in mem]
    for b in range(W.B):
        m = int(member[b])
        if m < 0:
            assert np.isnan(got["emd"][b]) and got["status"][b] == 0 and got["rounds"][b] == 0
            continue
        for key in ("rounds", "status", "eps_final", "emd"):
            assert _same(got[key][b], alone[m][key][0]), (b, m, key)
        for key in ("assign", "price"):
            assert _same(got[key][off[b]:off[b + 1]], alone[m][key]), (b, m, key)
        assert got["status"][b] == 0


# ---- wiring ---------------------------------------------------------------------------------------------------------------------------

def _cd_numpy(X, Y):
    """CD in f64 from the f32 squared distances of the nearest-neighbour kernel's one expression order"""
    dx = [(X[:, None, c] - Y[None, :, c]).astype(np.float32) for c in range(3)]
    xx = (dx[0].astype(np.float64) * dx[0].astype(np.float64)).astype(np.float32)
    d2 = R.fmaf32(dx[2], dx[2], R.fmaf32(dx[1], dx[1], xx)).astype(np.float64)
    return d2.min(1).mean() + d2.min(0).mean()


def test_pairwise_matrices_and_set_metrics(dev):
    gen = [R.shell(128, 200 + i, r=0.5 + 0.02 * i) for i in range(5)]
    ref = [R.shell(128, 300 + j, r=0.5 + 0.03 * j) for j in range(4)]
    G, Rf = [_t(x, dev) for x in gen], [_t(x, dev) for x in ref]
    want = {"cd": (np.array([[_cd_numpy(x, y) for y in ref] for x in gen]),
                   np.array([[0.0 if i == j else _cd_numpy(gen[min(i, j)], gen[max(i, j)]) for j in range(5)] for i in range(5)]),
                   np.array([[0.0 if i == j else _cd_numpy(ref[min(i, j)], ref[max(i, j)]) for j in range(4)] for i in range(4)])),
            "emd": (np.array([[R.auction(x, y)["emd"] for y in ref] for x in gen]),
                    np.array([[0.0 if i == j else R.auction(gen[min(i, j)], gen[max(i, j)])["emd"] for j in range(5)] for i in range(5)]),
                    np.array([[0.0 if i == j else R.auction(ref[min(i, j)], ref[max(i, j)])["emd"] for j in range(4)] for i in range(4)]))}
    for metric, pw in (("cd", M.pairwise_chamfer_dev), ("emd", M.pairwise_emd_dev)):
        D_gr, D_gg, D_rr = (x.cpu().numpy() for x in (pw(G, Rf), pw(G), pw(torch.stack(Rf))))
        assert D_gr.shape == (5, 4) and D_gr.dtype == np.float64
        for got, exp in zip((D_gr, D_gg, D_rr), want[metric]):
            if metric == "emd":
                assert _same(got, exp)                             # the auction's bits
            else:
                np.testing.assert_allclose(got, exp, rtol=1e-13)   # the same f32 distances; only the order of the f64 means differs
        assert (D_gg == D_gg.T).all() and (np.diag(D_gg) == 0).all() and (D_rr == D_rr.T).all() and (np.diag(D_rr) == 0).all()
        out = M.set_metrics(G, Rf, metric=metric)
        assert sorted(out) == ["1nna", "D_gr", "cov", "mmd"] and _same(out["D_gr"].cpu().numpy(), D_gr)
        assert out["mmd"] == pytest.approx(R.mmd(D_gr), rel=1e-14)
        assert out["cov"] == R.cov(D_gr) and out["1nna"] == pytest.approx(R.one_nna(D_gg, D_gr, D_rr), rel=1e-14)
    with pytest.raises(L.SfmiError, match="empty"):
        M.pairwise_chamfer_dev([G[0], torch.zeros(0, 3, device=dev)])
    assert M.emd(G[0], Rf[0]) == want["emd"][0][0, 0]


def test_evaluate_with_and_without_emd_n(dev):
    Xct = _t(R.shell(300, 1)[:150], dev)
    comps = [_t(R.shell(400 + 10 * i, 2 + i), dev) for i in range(3)]
    Xbd = _t(R.shell(500, 9), dev)
    plain = M.evaluate(Xct, comps, Xbd)
    assert sorted(plain) == ["cd", "cd_per", "fscore", "fscore_per", "k", "tau", "tmd", "uhd", "uhd_per"]
    per, mean = M.uhd(Xct, comps)
    assert plain["uhd_per"] == per.tolist() and plain["uhd"] == mean and plain["tmd"] == M.tmd(comps) and plain["k"] == 3
    assert plain["cd_per"] == pytest.approx([M.chamfer(c, Xbd) for c in comps], rel=1e-14)
    assert plain["fscore_per"] == pytest.approx([M.fscore(c, Xbd, 0.01) for c in comps], rel=1e-14)
    assert sorted(M.evaluate(Xct, comps)) == ["k", "tmd", "uhd", "uhd_per"]
    full = M.evaluate(Xct, comps, Xbd, emd_n=256)
    assert sorted(set(full) - set(plain)) == ["emd", "emd_n", "emd_per"] and full["emd_n"] == 256
    assert {k: full[k] for k in plain} == plain
    from shapeformer_amd import scan
    sub = lambda x: x[scan.farthest_point_sample_dev(x, None, 256)[0][0].long()]
    want = [M.emd(sub(c), sub(Xbd)) for c in comps]
    assert full["emd_per"] == want and full["emd"] == float(np.mean(want)) and all(0 < e < 1 for e in want)
    with pytest.raises(L.SfmiError, match="fewer points"):
        M.evaluate(Xct, comps, Xbd, emd_n=450)
