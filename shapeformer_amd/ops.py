"""Thin Python wrappers over the C ABI (one function per exported kernel launcher).

Tensors are torch CUDA tensors used purely as device-memory handles; every call
goes through libsfmi.so (shapeformer_amd/_lib.py).  No eager fallbacks.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


def _chk_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.SfmiError("libsfmi kernels need CUDA/HIP device tensors (no CPU fallback)")


def _c(t, dtype, name="tensor"):
    """a kernel's input in the dtype it reads, contiguous (the tensor itself when it already is); another dtype is refused"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise L.SfmiError(f"libsfmi: {name} must be a {dtype} torch tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    return t if t.is_contiguous() else t.contiguous()


def _need(cond, msg):
    if not cond:
        raise L.SfmiError(f"libsfmi: {msg}")


def _out(out, numel, like, name="out"):
    """a caller's output buffer goes to the kernel as it is: f32, contiguous, `numel` elements, on the inputs' device - converting it
    would lose the result, so every other form is refused"""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != numel:
        got = f"{out.dtype} {tuple(out.shape)}{'' if out.is_contiguous() else ' strided'}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise L.SfmiError(f"libsfmi: {name} must be a contiguous float32 tensor of {numel} elements, got {got}")
    _chk_cuda(out)
    _need(out.device == like.device, f"{name} is on {out.device}, the inputs on {like.device}")
    return out


# ---------------------------------------------------------------- SDF query
def sdf_pack_weights(sd, prefix="decoder.") -> np.ndarray:
    """Pack LocalDecoder MLP tensors (reference key names) into the kernel's fragment order."""
    g = lambda k: np.ascontiguousarray(np.asarray(sd[prefix + k], dtype=np.float32))
    cat = lambda fmt: np.ascontiguousarray(np.stack([g(fmt.format(i)) for i in range(5)]))
    out = np.empty(L.lib().sfmi_sdf_pack_floats(), np.float32)
    arrs = [g("fc_p.weight"), g("fc_p.bias"), cat("fc_c.{}.weight"), cat("fc_c.{}.bias"),
            cat("blocks.{}.fc_0.weight"), cat("blocks.{}.fc_0.bias"), cat("blocks.{}.fc_1.weight"),
            cat("blocks.{}.fc_1.bias"), g("fc_out.weight"), g("fc_out.bias"), out]
    L.check(L.lib().sfmi_sdf_pack_weights(*[a.ctypes.data for a in arrs]), "sfmi_sdf_pack_weights")
    return out


def sdf_query(xyz, grid_cl, wpack, sigmoid=False, out=None):
    """xyz (B,N,3) in [-1,1]; grid_cl (B,G,G,G,32) channels-last; -> (B,N,1) logits."""
    xyz, grid_cl, wpack = _c(xyz, torch.float32, "xyz"), _c(grid_cl, torch.float32, "grid_cl"), _c(wpack, torch.float32, "wpack")
    _need(xyz.dim() == 3 and xyz.shape[2] == 3 and grid_cl.dim() == 5, f"xyz (B,N,3) and grid_cl (B,G,G,G,32), got {tuple(xyz.shape)}, {tuple(grid_cl.shape)}")
    B, N, _ = xyz.shape
    G = grid_cl.shape[1]
    _need(grid_cl.shape == (B, G, G, G, 32), f"grid_cl must be ({B},G,G,G,32), got {tuple(grid_cl.shape)}")
    if out is not None:
        _out(out, B * N, xyz)
    _chk_cuda(xyz, grid_cl, wpack)
    if out is None:
        out = torch.empty(B, N, 1, device=xyz.device, dtype=torch.float32)
    L.check(L.lib().sfmi_sdf_query_f32(L.ptr(xyz), L.ptr(grid_cl), L.ptr(wpack), L.ptr(out), B, N, G,
                                       int(sigmoid), L.stream_ptr()), "sfmi_sdf_query_f32")
    return out


def sdf_query_keys(axis, keys, koff, grid_cl, wpack, sigmoid=False):
    """Keyed lattice points (csrc/sdf_query.hip KEYS): axis (Q) f32 table, keys (n) int32 shape-local fine indices (ix*Q+iy)*Q+iz ascending
    per shape, koff (B+1) int32 device offsets -> (n) values, each equal to sdf_query_grid's value at (shape, key) bit for bit."""
    axis, grid_cl, wpack = _c(axis, torch.float32, "axis"), _c(grid_cl, torch.float32, "grid_cl"), _c(wpack, torch.float32, "wpack")
    keys, koff = _c(keys, torch.int32, "keys"), _c(koff, torch.int32, "koff")
    _need(grid_cl.dim() == 5, f"grid_cl must be (B,G,G,G,32), got {tuple(grid_cl.shape)}")
    B, G = grid_cl.shape[0], grid_cl.shape[1]
    _need(grid_cl.shape == (B, G, G, G, 32) and koff.shape == (B + 1,) and keys.dim() == 1,
          f"grid_cl (B,G,G,G,32), koff (B+1,), keys (n,), got {tuple(grid_cl.shape)}, {tuple(koff.shape)}, {tuple(keys.shape)}")
    _chk_cuda(axis, keys, koff, grid_cl, wpack)
    out = torch.empty(keys.numel(), device=axis.device, dtype=torch.float32)
    L.check(L.lib().sfmi_sdf_query_keys_f32(L.ptr(axis), axis.numel(), L.ptr(keys), L.ptr(koff), keys.numel(), L.ptr(grid_cl), L.ptr(wpack),
                                            L.ptr(out), B, G, int(sigmoid), L.stream_ptr()), "sfmi_sdf_query_keys_f32")
    return out


def sigmoid(x, out=None):
    """nputil.sigmoid of a device logits tensor (in-tree kernel: the SDF query's own epilogue expression)."""
    x = _c(x, torch.float32, "x")
    if out is not None:
        _out(out, x.numel(), x)
        _need(out.data_ptr() % 16 == 0, "out must start on a 16-byte line (the kernel writes float4)")
    _chk_cuda(x)
    if x.data_ptr() % 16:          # a contiguous view that starts inside a 16-byte line: the kernel reads float4
        x = x.clone()
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().sfmi_sigmoid_f32(L.ptr(x), L.ptr(out), x.numel(), L.stream_ptr()), "sfmi_sigmoid_f32")
    return out


def sdf_query_grid(axis, grid_cl, wpack, sigmoid=False, out=None, x_range=None, affine=None):
    """Structured Q^3 'ij' query grid from a Q-entry f32 axis table -> (B,Q^3,1); x_range = (x0, x1): only the planes x0 <= ix < x1 of
    the slowest lattice index -> (B,(x1-x0) Q^2,1), the same values the whole-lattice call computes for them.  affine = (scale, shift)
    (B,32) each: grid_cl is the decoder grid BEFORE its last GroupNorm, whose affine the kernel applies to the interpolated features."""
    axis, grid_cl, wpack = _c(axis, torch.float32, "axis"), _c(grid_cl, torch.float32, "grid_cl"), _c(wpack, torch.float32, "wpack")
    Q = axis.numel()
    x0, x1 = (0, Q) if x_range is None else (int(x_range[0]), int(x_range[1]))
    _need(grid_cl.dim() == 5 and 0 <= x0 <= x1 <= Q, f"grid_cl (B,G,G,G,32) and 0 <= x0 <= x1 <= Q, got {tuple(grid_cl.shape)}, {(x0, x1)}")
    B, G = grid_cl.shape[0], grid_cl.shape[1]
    sc, sh = (None, None) if affine is None else (_c(affine[0], torch.float32, "affine scale"), _c(affine[1], torch.float32, "affine shift"))
    _need(affine is None or (sc.shape == (B, 32) and sh.shape == (B, 32)), f"affine = (scale, shift), ({B},32) each")
    if out is not None:
        _out(out, B * (x1 - x0) * Q * Q, axis)
    _chk_cuda(axis, grid_cl, wpack, sc, sh)
    if out is None:
        out = torch.empty(B, (x1 - x0) * Q * Q, 1, device=axis.device, dtype=torch.float32)
    L.check(L.lib().sfmi_sdf_query_grid_aff_f32(L.ptr(axis), Q, x0, x1, L.ptr(grid_cl), L.ptr(sc), L.ptr(sh), L.ptr(wpack), L.ptr(out), B, G,
                                                int(sigmoid), L.stream_ptr()), "sfmi_sdf_query_grid_aff_f32")
    return out


# ---------------------------------------------------------------- SDF value + gradient (csrc/sdf_query.hip sdf_grad_kernel)
def sdf_pack_weights_grad(sd, prefix="decoder.") -> np.ndarray:
    """The gradient kernel's weight image: the sdf_pack_weights image, the fragment image of the transposed matrices, fc_p^T."""
    g = lambda k: np.ascontiguousarray(np.asarray(sd[prefix + k], dtype=np.float32))
    cat = lambda fmt: np.ascontiguousarray(np.stack([g(fmt.format(i)) for i in range(5)]))
    out = np.empty(L.lib().sfmi_sdf_pack_grad_floats(), np.float32)
    arrs = [g("fc_p.weight"), g("fc_p.bias"), cat("fc_c.{}.weight"), cat("fc_c.{}.bias"),
            cat("blocks.{}.fc_0.weight"), cat("blocks.{}.fc_0.bias"), cat("blocks.{}.fc_1.weight"),
            cat("blocks.{}.fc_1.bias"), g("fc_out.weight"), g("fc_out.bias"), out]
    L.check(L.lib().sfmi_sdf_pack_weights_grad(*[a.ctypes.data for a in arrs]), "sfmi_sdf_pack_weights_grad")
    return out


def _sdf_grad_launch(xyz, grid_cl, wpack_grad, off, level=0.0, max_step=0.0, step=False, normals=False):
    """One launch of the gradient kernel.  xyz (B,N,3) with off None (equal offsets are built), or (N,3) with off (B+1) int32 device
    offsets (ragged).  -> val, grad, xyz_out or None, normal or None, shaped like the input."""
    xyz, grid_cl, wpack_grad = _c(xyz, torch.float32, "xyz"), _c(grid_cl, torch.float32, "grid_cl"), _c(wpack_grad, torch.float32, "wpack_grad")
    _need(grid_cl.dim() == 5, f"grid_cl must be (B,G,G,G,32), got {tuple(grid_cl.shape)}")
    B, G = grid_cl.shape[0], grid_cl.shape[1]
    _need(grid_cl.shape == (B, G, G, G, 32), f"grid_cl must be ({B},G,G,G,32), got {tuple(grid_cl.shape)}")
    if off is None:
        _need(xyz.dim() == 3 and xyz.shape[0] == B and xyz.shape[2] == 3, f"xyz must be ({B},N,3), got {tuple(xyz.shape)}")
        vshape = (B, xyz.shape[1], 1)
    else:
        off = _c(off, torch.int32, "off")
        _need(xyz.dim() == 2 and xyz.shape[1] == 3 and off.shape == (B + 1,), f"xyz (N,3) with off ({B + 1},), got {tuple(xyz.shape)}, {tuple(off.shape)}")
        vshape = (xyz.shape[0],)
    _chk_cuda(xyz, grid_cl, wpack_grad, off)
    _need(wpack_grad.numel() == L.lib().sfmi_sdf_pack_grad_floats(), "wpack_grad is not sdf_pack_weights_grad's image")
    if off is None:
        off = torch.arange(B + 1, device=xyz.device, dtype=torch.int32) * xyz.shape[1]
    n = xyz.numel() // 3
    val = torch.empty(vshape, device=xyz.device, dtype=torch.float32)
    grad = torch.empty_like(xyz)
    xo = torch.empty_like(xyz) if step else None
    no = torch.empty_like(xyz) if normals else None
    if n == 0:
        return val, grad, xo, no
    L.check(L.lib().sfmi_sdf_query_grad_f32(L.ptr(xyz), L.ptr(off), n, L.ptr(grid_cl), L.ptr(wpack_grad), L.ptr(val), val.numel(), L.ptr(grad),
                                            grad.numel(), float(level), float(max_step), L.ptr(xo), 0 if xo is None else xo.numel(), L.ptr(no),
                                            0 if no is None else no.numel(), B, G, L.stream_ptr()), "sfmi_sdf_query_grad_f32")
    return val, grad, xo, no


def sdf_query_grad(xyz, grid_cl, wpack_grad, off=None):
    """Logit and d logit / d xyz (the [-1,1] frame) of the fused implicit decoder.  xyz (B,N,3) -> val (B,N,1), grad (B,N,3); or ragged:
    xyz (N,3) with off (B+1) int32 device offsets -> val (N), grad (N,3).  val equals sdf_query's logit bit for bit."""
    return _sdf_grad_launch(xyz, grid_cl, wpack_grad, off)[:2]


def sdf_refine_step(xyz, grid_cl, wpack_grad, level, max_step, off=None):
    """One Newton step towards the iso-surface logit == level, the move clamped to max_step in length (fused step epilogue):
    x' = x - s (val - level) g / |g|^2, s = min(1, max_step |g| / |val - level|); x where |g|^2 < 1e-24.  -> x', val (at x)."""
    val, _, xo, _ = _sdf_grad_launch(xyz, grid_cl, wpack_grad, off, level=level, max_step=max_step, step=True)
    return xo, val


def sdf_normals(xyz, grid_cl, wpack_grad, off=None):
    """Unit normals -g/|g| of the decoder field at xyz (outward: occupancy rises inward), zero where |g|^2 < 1e-24 (fused normal
    epilogue).  Shapes as sdf_query_grad."""
    return _sdf_grad_launch(xyz, grid_cl, wpack_grad, off, normals=True)[3]
