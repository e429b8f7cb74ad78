"""Float64 statement of the gradient kernel's contract (include/sfmi.h) on top of oracle.vqdif_oracle.

The implicit decoder (dec.py:62-100) is restated with the oracle's own pieces - `trilinear_sample`, and the MLP of `sdf_mlp` written
out so that its 11 ReLU inputs (5 x `net`, 5 x `h`, the last `net`; 32 channels each: 352 per point) are visible - and differentiated
with torch.autograd.  The result is what the kernel must return: value, d value / d Xtg, and per point the smallest |pre-activation|,
the margin by which a float32 implementation may legitimately take another ReLU branch.  Also: the Newton step of the step
epilogue with the same clamp, the inputs the tests share, and the lattice-edge crossings that marching cubes turns into vertices.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vqdif_oracle as O

NORM_DIV = 1.0 + O.PAD + 10e-4          # 1.101
FLAT = 1e-24                            # |g|^2 below which the epilogues do not divide


def cast_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in O.to_torch_sd(sd).items() if k.startswith("decoder.fc") or k.startswith("decoder.blocks")}


def decoder(sd, grid, Xtg):
    """sd / grid (B,32,G,G,G) / Xtg (B,N,3) of one dtype -> logits (B,N,1) by the operations of O.sdf_query, in their order, and the
    list of the 11 pre-activations (B,N,32)."""
    p = Xtg / 2.0
    c = O.trilinear_sample(grid, p)
    net = F.linear(p, sd["decoder.fc_p.weight"], sd["decoder.fc_p.bias"])
    pre = []
    for i in range(5):
        net = net + F.linear(c, sd[f"decoder.fc_c.{i}.weight"], sd[f"decoder.fc_c.{i}.bias"])
        pre.append(net)
        h = F.linear(F.relu(net), sd[f"decoder.blocks.{i}.fc_0.weight"], sd[f"decoder.blocks.{i}.fc_0.bias"])
        pre.append(h)
        dx = F.linear(F.relu(h), sd[f"decoder.blocks.{i}.fc_1.weight"], sd[f"decoder.blocks.{i}.fc_1.bias"])
        net = net + dx
    pre.append(net)
    return F.linear(F.relu(net), sd["decoder.fc_out.weight"], sd["decoder.fc_out.bias"]), pre


def value_grad(sd, grid, Xtg, dtype=torch.float64):
    """-> val (B,N), grad (B,N,3) = d val / d Xtg by autograd, margin (B,N) = min |pre-activation| over the 352 ReLU inputs; all in
    `dtype` (float64: the truth; float32: the oracle's own arithmetic, whose error against float64 scales the test's gate)."""
    x = Xtg.detach().to(dtype).clone().requires_grad_(True)
    out, pre = decoder(cast_sd(sd, dtype), grid.to(dtype), x)
    grad, = torch.autograd.grad(out.sum(), x)                   # the points are independent: the sum's gradient is per point
    margin = torch.stack([a.detach().abs().amin(-1) for a in pre]).amin(0)
    return out.detach()[..., 0], grad, margin


def oracle_grad_f32(sd, grid, Xtg):
    """torch.autograd on oracle.vqdif_oracle.sdf_query itself, in float32."""
    x = Xtg.detach().float().clone().requires_grad_(True)
    out = O.sdf_query(O.to_torch_sd(sd), grid.float(), x)
    grad, = torch.autograd.grad(out.sum(), x)
    return out.detach()[..., 0], grad


def newton_step(x, val, grad, level, max_step):
    """The step epilogue: x' = x - s (val - level) g / |g|^2, s = min(1, max_step |g| / |val - level|); x where |g|^2 < 1e-24."""
    g2 = (grad * grad).sum(-1)
    d = val - level
    ok = g2 >= FLAT
    g2s = torch.where(ok, g2, torch.ones_like(g2))
    s = torch.minimum(torch.ones_like(d), max_step * g2s.sqrt() / d.abs().clamp_min(1e-300))
    k = torch.where(ok, s * d / g2s, torch.zeros_like(d))
    return x - k[..., None] * grad


def rand_grid(B, seed):
    """The feature grids of tests/test_sdf_query_gpu.py."""
    return torch.randn(B, 32, 64, 64, 64, generator=torch.Generator().manual_seed(seed))


def interior_points(B, N, seed, G=64):
    """Cell-interior points: ix = cell + frac per axis, cell in [0, G-1), frac in [0.1, 0.9], mapped back to the [-1,1] frame by
    x = 2 * 1.101 * (ix / (G-1) - 0.5); float32 (what the kernel is given; the float64 truth is evaluated at these same values).
    No point is near a feature-cell face in either precision."""
    g = torch.Generator().manual_seed(seed)
    cell = torch.randint(0, G - 1, (B, N, 3), generator=g).double()
    frac = 0.1 + 0.8 * torch.rand(B, N, 3, generator=g, dtype=torch.float64)
    return (2.0 * NORM_DIV * ((cell + frac) / (G - 1) - 0.5)).float()


def clamped_points(seed):
    """(68,3): the four named points of the clamped-axes test and 64 random ones with every coordinate in [1.0, 1.3] of either sign."""
    g = torch.Generator().manual_seed(seed)
    named = torch.tensor([[1.2, 0.0, 0.0], [-1.3, 0.3, 1.25], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])
    r = 1.0 + 0.3 * torch.rand(64, 3, generator=g)
    sign = torch.where(torch.rand(64, 3, generator=g) < 0.5, -1.0, 1.0)
    return torch.cat([named, r * sign])


def edge_crossings(field, level):
    """field (Q,Q,Q) on the makeGrid 'ij' lattice over [-1,1]^3 -> (V,3) float64: where marching cubes puts its vertices, the linear
    interpolation of `level` on every lattice edge whose ends lie on different sides."""
    f = np.asarray(field, np.float64)
    Q = f.shape[0]
    ax = np.linspace(-1.0, 1.0, Q)
    out = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, Q - 1), slice(1, Q)
        f0, f1 = f[tuple(lo)], f[tuple(hi)]
        idx = np.argwhere((f0 < level) != (f1 < level))
        t = (level - f0[tuple(idx.T)]) / (f1[tuple(idx.T)] - f0[tuple(idx.T)])
        p = ax[idx]
        p[:, a] = ax[idx[:, a]] + t * (ax[1] - ax[0])
        out.append(p)
    return np.concatenate(out)
