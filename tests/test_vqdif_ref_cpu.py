"""CPU side of the VQDIF point-path harness (tests/vqdif_ref.py): the float32 mirrors against the oracle and the golden vectors, the
float64 references against the float32 oracle (an independent float32 implementation: the derived bounds must hold for it, and the
printed ratios show how much room they leave), the mirror of the fused kernel's ownership rule over the GPU case table, and seeded
faults - float64 against float64 under the bound of the unfaulted case - that the bounds must be tight enough to see.  No GPU.

Measured here (pytest -s): the float32 oracle sits at 0.018 of the first block's bound and 0.001 .. 0.004 of the later encoder bounds
(its own error on c: 1.1e-6 .. 1.6e-6 at scale 2.0 .. 2.5), at 0.002 .. 0.003 of the logit bound (its own error 1.4e-6 .. 2.1e-6 at
scale 5.0 .. 5.7 for G = 2 .. 64 once the coordinates' rounding is shared).  A count off by one in a cell of 128 points exceeds the
mean's bound 4.3-fold (the convolution behind it: 0.8, not seen there; cells of 33 and 1 points are), swapped weight rows exceed the
bounds 240- to 1700-fold, a gather a hundredth of a cell off 1700-fold, the second-nearest code is outside the VQ bound on every row."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import vqdif_ref as R                                   # noqa: E402
import sdf_grad_ref as SG                               # noqa: E402
from oracle import vqdif_oracle as O                    # noqa: E402
from test_vqdif_kernels_gpu import ENC_CASES            # noqa: E402

GOLD = os.path.join(HERE, "golden", "vqdif16_small.npz")


def _ratio(name, got, ref, bound):
    r = float(((torch.as_tensor(got).double() - ref).abs() / bound).max())
    print(f"[ratio] {name} {r:.4f}")
    return r


def _case(prefix):
    return [c for c in ENC_CASES if c.name.startswith(prefix)][0]


# ---------------------------------------------------------------------------------------------------- mirrors
@pytest.mark.parametrize("R_", [16, 32])
def test_cells_mirror_equals_the_oracle_on_faces_and_outside_the_box(R_):
    cloud = np.stack([R.face_cloud(600, 70), R.face_cloud(600, 71)])
    cell, mask = R.cells_f32(cloud, R_)
    u = O.normalize_3d(torch.from_numpy(cloud) / 2.0)
    assert np.array_equal(cell, O.cell_index(u).numpy())
    assert np.array_equal(mask, O.occupancy_mask(u, R_).numpy())
    # the cloud does what it is for: clamped points land in cell 63 / 0, and some face value falls on either side of its face
    c3 = R.cell_xyz(cell)
    assert (c3 == 63).any() and (c3 == 0).any()
    for v, want in ((1.3, 63), (1.101, 63), (-1.3, 0), (-1.101, 0)):
        assert (c3[cloud == np.float32(v)] == want).all()
    sides = set()
    for f in (1, 2, 4, 31, 32, 33, 36, 62, 63):
        face = np.float32(2.0 * R.NORM_DIV * (f / 64 - 0.5))
        for v in (face, np.nextafter(face, np.float32(2)), np.nextafter(face, np.float32(-2))):
            got = {int(c) - f for c in c3[cloud == v]}
            assert got and got <= {-1, 0}, (f, v, got)
            sides |= got
    assert sides == {-1, 0}


def test_cells_mirror_equals_the_golden_vectors():
    z = np.load(GOLD)
    cell, mask = R.cells_f32(z["cloud"], 16)
    assert np.array_equal(cell, z["cell"])
    assert np.array_equal(np.packbits(mask), z["grid_mask"])


@pytest.mark.parametrize("G", [2, 3, 16, 64])
def test_axis_mirror_stays_within_its_ulp_bound_of_float64(G):
    x = np.concatenate([R.query_points(3, 400, G, 5 + G).reshape(-1), np.linspace(-1.4, 1.4, 20001).astype(np.float32)])
    i0, i1, w0, w1, ix = R.axis_f32(x, G, with_ix=True)
    # normalize_3d jumps from 1 to 0.999 at u = 1: a coordinate whose u is within rounding of 1 has no float64 counterpart to compare with
    u64 = x.astype(np.float64) * 0.5 / R.NORM_DIV + 0.5
    ok = np.abs(u64 - 1.0) > 4.0 * R.U
    assert (~ok).sum() < 100 and ok.sum() > 20000
    d = np.abs(ix.astype(np.float64) - R.ix_f64(x, G))[ok]
    print(f"[ratio] axis G{G} {d.max() / R.ix_ulp_bound(G):.4f}")
    assert d.max() <= R.ix_ulp_bound(G)
    assert (i0 >= 0).all() and (i1 <= G - 1).all() and ((i1 == i0 + 1) | (i0 == G - 1)).all()
    assert np.array_equal(w0 + w1, np.ones_like(w0)) and (w1 >= 0).all() and (w1 < 1).all()
    assert (w1[i0 == G - 1] == 0).all()                                      # the border: i1 == i0 carries no weight


# ---------------------------------------------------------------------------------------------------- encoder
def _random_cloud(seed, B=2, T=3000):
    g = np.random.default_rng(seed)
    c = (g.random((B, T, 3)) * 1.6 - 0.8).astype(np.float32)
    c[:, : T // 3] = (c[:, : T // 3] * 0.05 + 0.3).astype(np.float32)          # a dense clump: cells of many points
    return c


@pytest.mark.parametrize("which", ["golden", "random"])
def test_encoder_reference_agrees_with_the_float32_oracle(vq16_sd, vq16_sd_t, which):
    cloud = np.load(GOLD)["cloud"] if which == "golden" else _random_cloud(3)
    ref = R.encoder_ref(vq16_sd, cloud, 16)
    c, cell, u, stages = O.encoder_points(vq16_sd_t, torch.from_numpy(cloud) / 2.0, return_stages=True)
    assert np.array_equal(cell.numpy(), ref.cell) and np.array_equal(O.occupancy_mask(u, 16).numpy(), ref.mask)
    for i in (0, 1, 4):
        assert _ratio(f"oracle enc stage{i} | {which}", stages[i], ref.stages[i], ref.e_stages[i]) <= 1.0
    assert _ratio(f"oracle enc c | {which}", c, ref.c, ref.e_c) <= 1.0
    print(f"oracle's own error on c: {float((c.double() - ref.c).abs().max()):.2e} at scale {float(ref.c.abs().max()):.2f}")
    # the oracle's mean is an f32 sum of n values and a division: gamma(n + 1) mean|c| on top of the bound (the kernels' sum is exact)
    dense = O.grid_mean(c, cell)
    m32 = dense.reshape(cloud.shape[0], 32, -1)[ref.occ[:, 0], :, ref.occ[:, 1]]
    absmean = O.grid_mean(ref.c.abs(), cell).reshape(cloud.shape[0], 32, -1)[ref.occ[:, 0], :, ref.occ[:, 1]]
    e_sum = R.gamma(ref.count.double() + 1)[:, None] * absmean
    assert _ratio(f"oracle enc mean | {which}", m32, ref.mean, ref.e_mean + e_sum) <= 1.0
    # the sparse down0 of the reference (value and bound) == dense float64 convolutions; the float32 convolution of the oracle's mean
    # grid within the same rule fed with the oracle's mean bound
    w = torch.as_tensor(vq16_sd_t["encoder.downsampler.blocks.0.conv.weight"]).double()
    B = cloud.shape[0]
    idx = (ref.par[:, 0], slice(None), ref.par[:, 1], ref.par[:, 2], ref.par[:, 3])

    def dense_of(rows):
        d = torch.zeros(B, 32, 64 ** 3, dtype=torch.float64)
        d[ref.occ[:, 0], :, ref.occ[:, 1]] = rows
        return d.reshape(B, 32, 64, 64, 64)
    y64 = F.relu(F.conv3d(dense_of(ref.mean), w, stride=2))
    assert float((y64[idx] - ref.down).abs().max()) < 1e-12
    pocc = torch.zeros(B, 32, 32, 32, dtype=torch.bool)
    pocc[tuple(ref.par.T)] = True
    assert float(y64.abs().amax(1)[~pocc].max()) == 0.0
    rnd = R.gamma(258) * F.conv3d(dense_of(ref.mean.abs()), w.abs(), stride=2)
    assert torch.allclose((F.conv3d(dense_of(ref.e_mean), w.abs(), stride=2) + rnd)[idx], ref.e_down, rtol=1e-9, atol=0)
    y32 = F.relu(F.conv3d(dense, w.float(), stride=2))
    assert _ratio(f"oracle enc down0 | {which}", y32[idx], ref.down, (F.conv3d(dense_of(ref.e_mean + e_sum), w.abs(), stride=2) + rnd)[idx]) <= 1.0


def test_fused_ownership_invariants_on_every_case():
    seen = set()
    for case in ENC_CASES:
        cell, _ = R.cells_f32(case.cloud(), case.R)
        info = case.check_reach(cell)
        T = cell.shape[1]
        for b, (declined, own) in enumerate(info):
            st, en = R.runs_of(np.sort(cell[b]))
            assert len(own) == (T + R.EF_NOM - 1) // R.EF_NOM
            assert own[0][0] == 0 and own[-1][1] == T and all(a[1] == c[0] for a, c in zip(own, own[1:])), (case.name, own)   # tile [0, T)
            assert all(p == T or st[p] == p for p0, p1 in own for p in (p0, p1)), (case.name, "a run is split")
            if not declined:
                assert all(0 <= p1 - p0 <= R.EF_CAP for p0, p1 in own), (case.name, own)
                seen |= {p1 - p0 for p0, p1 in own}
            else:
                seen.add("declined")
    assert {0, R.EF_CAP - 1, "declined"} <= seen, "the case table no longer reaches n = 0, n = EF_CAP - 1 or a declined shape"
    assert (R.EF_CAP, R.EF_LIMIT, R.EF_NOM) == (512, 128, 384)


# ---------------------------------------------------------------------------------------------------- decoder query
@pytest.mark.parametrize("G", [2, 3, 16, 64])
def test_decoder_reference_agrees_with_the_float32_oracle_and_with_grid_sample(vq16_sd, vq16_sd_t, G):
    B, N = 2, 300
    grid = torch.randn(B, 32, G, G, G, generator=torch.Generator().manual_seed(G))
    pts = R.query_points(B, N, G, 9 + G)
    ref, bound, slack = R.query_ref(vq16_sd, grid, pts)
    o32 = O.sdf_query(vq16_sd_t, grid, torch.from_numpy(pts))[..., 0]
    print(f"oracle's own error on the logits at G = {G}: {float((o32.double() - ref).abs().max()):.2e} at scale {float(ref.abs().max()):.2f}")
    assert _ratio(f"oracle sdf logit | G{G}", o32, ref, bound) <= 1.0
    # an independent float64 implementation (F.grid_sample + sdf_grad_ref.decoder) differs only through the coordinates' rounding: at most
    # ix_ulp_bound(G) per axis where the [IX] slack allows IX_SLACK_ULP ulp(ix) >= IX_SLACK_ULP 2^-23
    u64 = pts.astype(np.float64) * 0.5 / R.NORM_DIV + 0.5
    ok = torch.from_numpy((np.abs(u64 - 1.0) > 4.0 * R.U).all(-1))
    d64 = SG.decoder(SG.cast_sd(vq16_sd, torch.float64), grid.double(), torch.from_numpy(pts).double())[0][..., 0]
    factor = R.ix_ulp_bound(G) / (R.IX_SLACK_ULP * 2.0 ** -23)
    assert ok.sum() > 0.9 * ok.numel()
    assert _ratio(f"grid_sample float64 | G{G}", d64[ok], ref[ok], slack[ok] * factor + 1e-12) <= 1.0
    # with the affine applied in the gather == on the affined grid
    g = torch.Generator().manual_seed(1)
    sc, sh = torch.rand(B, 32, generator=g) + 0.5, torch.randn(B, 32, generator=g) * 0.3
    a, ab, _ = R.query_ref(vq16_sd, grid, pts, affine=(sc, sh))
    g2 = (grid.double() * sc[:, :, None, None, None] + sh[:, :, None, None, None]).float()
    b, bb, _ = R.query_ref(vq16_sd, g2, pts)
    assert _ratio(f"affine in the gather | G{G}", a, b, ab + bb) <= 1.0


# ---------------------------------------------------------------------------------------------------- seeded faults
def test_fault_cell_count_off_by_one_is_seen(vq16_sd):
    case = _case("4:")
    cloud = case.cloud()
    ref = R.encoder_ref(vq16_sd, cloud, 16)
    for n in (128, 33, 1):
        k = int(torch.nonzero(ref.count == n)[0])
        cell = int(ref.occ[k, 1])
        bad = R.EncRef()
        bad.cell, bad.c, bad.e_c = ref.cell, ref.c, ref.e_c
        R.mean_down(vq16_sd, bad, count_fault=(0, cell, 1))
        r = (bad.mean - ref.mean).abs() / ref.e_mean
        assert float(r[k].max()) > 1.0, (n, float(r[k].max()))
        assert float(torch.cat([r[:k], r[k + 1:]]).max()) == 0.0
        c3 = R.cell_xyz(cell) // 2
        q = int(torch.nonzero((ref.par[:, 1:] == torch.tensor([c3[2], c3[1], c3[0]])).all(1))[0])
        rd = (bad.down - ref.down).abs() / ref.e_down
        print(f"[fault] count {n} + 1: mean {float(r[k].max()):.1f} x bound, down0 {float(rd[q].max()):.1f} x bound")
        # (one point in 129 moves the mean by 0.8 %: the mean's own bound sees it, the convolution's - |W| e_mean over 8 x 32 inputs - not)
        assert n == 128 or float(rd[q].max()) > 1.0, (n, float(rd[q].max()))


def test_fault_swapped_weight_row_is_seen(vq16_sd):
    case = _case("3:")
    cloud = case.cloud()
    ref = R.encoder_ref(vq16_sd, cloud, 16)
    for key in ("encoder.blocks.0.fc_0.weight", "encoder.blocks.3.shortcut.weight", "encoder.fc_c.weight", "encoder.downsampler.blocks.0.conv.weight"):
        sd = dict(vq16_sd)
        w = np.array(sd[key], copy=True)
        w[[3, 4]] = w[[4, 3]]
        sd[key] = w
        bad = R.encoder_ref(sd, cloud, 16)
        r = max(float(((bad.c - ref.c).abs() / ref.e_c).max()), float(((bad.down - ref.down).abs() / ref.e_down).max()))
        print(f"[fault] rows 3 / 4 of {key} swapped: {r:.1f} x bound")
        assert r > 1.0, key
    grid = torch.randn(1, 32, 16, 16, 16, generator=torch.Generator().manual_seed(2))
    pts = R.query_points(1, 200, 16, 3)
    out, bound, _ = R.query_ref(vq16_sd, grid, pts)
    for key in ("decoder.fc_c.0.weight", "decoder.blocks.2.fc_0.weight", "decoder.blocks.4.fc_1.weight"):
        sd = dict(vq16_sd)
        w = np.array(sd[key], copy=True)
        w[[3, 4]] = w[[4, 3]]
        sd[key] = w
        bad, _, _ = R.query_ref(sd, grid, pts)
        r = (bad - out).abs() / bound
        print(f"[fault] rows 3 / 4 of {key} swapped: {float(r.max()):.1f} x bound, {float((r > 1).double().mean()):.2f} of the points")
        assert float((r > 1).double().mean()) > 0.5, key
    # a gather a hundredth of a feature cell off along x is seen in the features themselves
    c, e, s = R.gather_ref(grid, pts)
    shifted = pts.copy()
    shifted[..., 0] = pts[..., 0] + np.float32(2.0 * R.NORM_DIV / 15 * 0.01)
    c2, _, _ = R.gather_ref(grid, shifted)
    r = ((c2 - c).abs() / (e + s)).amax(-1)
    print(f"[fault] gather 0.01 cell off: {float(r.median()):.1f} x bound (median over the points)")
    assert float((r > 1).double().mean()) > 0.8


@pytest.mark.parametrize("K", [32, 64, 4096])
def test_fault_reversed_tie_rule_is_seen(K):
    D, N = 64, 65
    W, pairs = R.tie_codebook(K, D, 3)
    target = torch.arange(N) % len(pairs)
    lo = torch.tensor([p[0] for p in pairs])[target]
    hi = torch.tensor([p[1] for p in pairs])[target]
    x = (torch.from_numpy(W)[lo] + 0.01 * torch.randn(N, D, generator=torch.Generator().manual_seed(K))).numpy()
    d, e = R.vq_ref(x, W, pairs)
    assert torch.equal(R.vq_argmin_ref(d), lo)
    assert torch.equal(R.vq_argmin_ref(d, lowest=False), hi) and not torch.equal(lo, hi)
    # the value checks alone cannot see it (the two codes are equally near): only the exact index comparison does
    r = torch.arange(N)
    assert float(((d[r, hi] - d[r, lo]).abs() / e[r, lo]).max()) == 0.0
    # a distance bound with teeth: the nearest code replaced by the second nearest is outside e(a) + e(m) for random rows
    g = torch.Generator().manual_seed(5)
    Wr, xr = (torch.randn(K, D, generator=g) * 0.5).numpy(), (torch.randn(N, D, generator=g) * 0.5).numpy()
    d, e = R.vq_ref(xr, Wr)
    two = torch.topk(d, 2, dim=1, largest=False)
    gap = (two.values[:, 1] - two.values[:, 0]) / (e[r, two.indices[:, 1]] + e[r, two.indices[:, 0]])
    print(f"[fault] second-nearest code, K = {K}: {float((gap > 1).double().mean()):.2f} of the rows outside the bound")
    assert float((gap > 1).double().mean()) > 0.9
