"""Sparse (pos,code) token packing over libsfmi (mirrors shapeformer/models/common.py:84-189).

Device representation is ragged-in-a-padded-buffer: (B,Lpad,2) int32 + len (B,) int32 (see
csrc/tokens.hip).  The `*_ref` helpers return the reference's exact tensor shapes/dtypes
((B,L,2) int64 etc.) and therefore sync once to size the result, as the reference does.
"""
from __future__ import annotations

import torch

from . import _lib as L
from ._ragged import on_device


def _table(t, what, name):
    """an integer table a kernel reads -> int32 contiguous (the tensor itself when it already is)"""
    if not isinstance(t, torch.Tensor) or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise L.SfmiError(f"{what}: {name} must be an integer torch tensor on the HIP device (no CPU fallback)")
    return t.to(torch.int32).contiguous()


def _exact(t, numels, what, name):
    """a control tensor or a caller's output buffer, handed to the kernel as it is: int32, contiguous, one of `numels` elements.
    Converting an output would lose the result, so every other form is refused."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() not in numels:
        got = f"{t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ' strided'}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise L.SfmiError(f"{what}: {name} must be a contiguous int32 tensor of {' or '.join(str(n) for n in numels)} elements, got {got}")
    return t


def _on_device(what, *ts):
    """the last check (the layout of every argument is reported first): _ragged.on_device over the arguments that were given"""
    return on_device(what, *[t for t in ts if t is not None])


def mode_i32(idx, vocab, rows=1):
    """rows=1: whole-tensor mode (reference batch semantics); rows=B: one mode per shape.  idx: an integer tensor of any layout (an
    int32 contiguous one is used as it is)."""
    idx = _table(idx, "mode_i32", "idx")
    _on_device("mode_i32", idx)
    dev = idx.device
    hist = torch.empty(rows * vocab, device=dev, dtype=torch.int32)
    out = torch.empty(rows, device=dev, dtype=torch.int32)
    L.check(L.lib().sfmi_mode_i32(L.ptr(idx), idx.numel(), vocab, rows, L.ptr(hist), L.ptr(out), L.stream_ptr()), "sfmi_mode_i32")
    return out


def dense2sparse_dev(q, mode, max_length, end_tokens, Lpad=None, tokens=None, length=None):
    """q (B,R,R,R) integers on device (int32 contiguous: used as it is), mode (1,) or (B,) int32 -> tokens (B,Lpad,2) int32, len (B,)
    int32.  tokens / length: the caller's buffers, int32 and contiguous, else SfmiError."""
    what = "dense2sparse_dev"
    q = _table(q, what, "q")
    if q.dim() < 2 or q.numel() == 0:
        raise L.SfmiError(f"{what}: q must be a non-empty (B,R,R,R) grid, got {tuple(q.shape)}")
    B = q.shape[0]
    ncell = q.numel() // B
    Lpad = Lpad or max_length
    mode = _exact(mode, (1, B), what, "mode")
    if tokens is not None:
        _exact(tokens, (B * Lpad * 2,), what, "tokens")
    if length is not None:
        _exact(length, (B,), what, "length")
    _on_device(what, q, mode, tokens, length)
    tokens = tokens if tokens is not None else torch.empty(B, Lpad, 2, device=q.device, dtype=torch.int32)
    length = length if length is not None else torch.empty(B, device=q.device, dtype=torch.int32)
    L.check(L.lib().sfmi_dense2sparse_i32(L.ptr(q), L.ptr(mode), int(mode.numel() > 1), L.ptr(tokens), L.ptr(length), B, ncell, Lpad, max_length,
                                          int(end_tokens[0]), int(end_tokens[1]), L.stream_ptr()), "sfmi_dense2sparse_i32")
    return tokens, length


def sparse2dense_dev(tokens, length, empty, dense_res, end_tokens, dim=3, out=None, start=None):
    """tokens (B,Lpad,2) integers (int32 contiguous: used as it is), len (B,) or None, empty (1,) or (B,) int32, optional per-row start
    (B,) int32 -> dense (B,R,R,R) int32.  length / empty / start and the caller's `out` are int32 and contiguous, else SfmiError."""
    what = "sparse2dense_dev"
    tokens = _table(tokens, what, "tokens")
    if tokens.dim() != 3 or tokens.shape[2] != 2 or tokens.numel() == 0:
        raise L.SfmiError(f"{what}: tokens must be a non-empty (B,Lpad,2) tensor, got {tuple(tokens.shape)}")
    B, Lpad, _ = tokens.shape
    ncell = dense_res ** dim
    empty = _exact(empty, (1, B), what, "empty")
    if length is not None:
        _exact(length, (B,), what, "length")
    if start is not None:
        _exact(start, (B,), what, "start")
    if out is not None:
        _exact(out, (B * ncell,), what, "out")
    _on_device(what, tokens, length, empty, start, out)
    out = out if out is not None else torch.empty((B,) + (dense_res,) * dim, device=tokens.device, dtype=torch.int32)
    L.check(L.lib().sfmi_sparse2dense_i32(L.ptr(tokens), L.ptr(start), L.ptr(length), L.ptr(empty), int(empty.numel() > 1), L.ptr(out), B, ncell, Lpad,
                                          int(end_tokens[0]), int(end_tokens[1]), L.stream_ptr()), "sfmi_sparse2dense_i32")
    return out


def batch_dense2sparse(indices, max_length=None, end_tokens=(100, 200), vocab=4097):
    """common.py:151-168 (unpack=True): (B,R,R,R) -> ((B,L,2) int64 padded with end tokens, mode)."""
    q = indices.to(torch.int32).contiguous()
    B = q.shape[0]
    ncell = q.numel() // B
    mode = mode_i32(q, vocab)
    ml = max_length if max_length is not None else ncell + 1
    tok, ln = dense2sparse_dev(q, mode, ml, end_tokens, Lpad=min(ml, ncell + 1))
    Lmax = int(ln.max().item())  # the reference sizes its output the same way (host sync)
    return tok[:, :Lmax].long(), mode.long()[0]


def batch_sparse2dense_padded(sparse, empty_ind, dense_res, end_tokens):
    """pack_sparse + batch_sparse2dense (common.py:126-140,171-189) on a padded (B,L,2) tensor."""
    tok = sparse.to(torch.int32).contiguous()
    empty = torch.as_tensor([int(empty_ind)], device=tok.device, dtype=torch.int32)
    return sparse2dense_dev(tok, None, empty, dense_res, end_tokens).long()
