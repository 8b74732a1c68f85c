"""What gallery.py, pool.py, quality.py and tracker.py ask of their tensors before a pointer goes to the library: one place for
each coercion, and ONE rule for a pointer."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

DIM = 512


def ptr(t):
    """The device address of `t`; null for None AND for an empty tensor, whatever storage an empty view sits in.  Every entry
    point of these modules accepts null wherever the count that goes with the pointer is 0.  An entry that wants an address
    where nothing will be read is given a one-element tensor at its call site (``FaceGallery.cluster``'s empty neighbour list)."""
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def cuda_device(device, message: str) -> torch.device:
    """`device` (None: the current GPU) as a CUDA device with an index; ``ValueError(message)`` for any other kind."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError(message)
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _float32(x, device) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.array(x, np.float32))                 # (a copy: the caller's array may be read-only)
    return torch.as_tensor(x).detach().to(device, torch.float32)


def rows(x, device, keep_pitch: bool = False) -> torch.Tensor:
    """(n, 512) float32 on `device` (a host array or tensor is uploaded once), contiguous -- or, with `keep_pitch`, a view with
    unit stride along a row and rows at least 512 floats apart taken as it is (its row pitch is the kernel's ld_rows)."""
    x = _float32(x, device)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.shape[1] != DIM:
        raise ValueError(f"expected ({'m' if keep_pitch else 'n'}, {DIM}) embeddings, got {tuple(x.shape)}")      # (the pool counts m rows)
    if keep_pitch and x.shape[0] > 1 and x.stride(1) == 1 and x.stride(0) >= DIM:
        return x
    return x.contiguous()


def vector(v, m: int, dtype, device, name: str):
    """None, or `v` as (m,) `dtype` on `device`, contiguous."""
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.array(v))
    v = torch.as_tensor(v).detach().to(device, dtype).reshape(-1).contiguous()
    if v.shape[0] != m:
        raise ValueError(f"{name} must have {m} entries, not {v.shape[0]}")
    return v


def table(x, cols: int, device, name: str) -> torch.Tensor:
    """`x` as (m, cols) float32 on `device`, contiguous: boxes (m, 4), points (m, 10)."""
    x = _float32(x, device)
    if x.numel() % cols:
        raise ValueError(f"{name} must be (m, {cols}), got {tuple(x.shape)}")
    return x.reshape(-1, cols).contiguous()


def grown(old: torch.Tensor, rows: int, dim: int = 0, fill=0) -> torch.Tensor:
    """A tensor of `rows` rows (along `dim`) of `fill` with `old` copied into its prefix, on `old`'s device."""
    shape = list(old.shape)
    shape[dim] = rows
    new = torch.full(shape, fill, dtype=old.dtype, device=old.device)
    new.narrow(dim, 0, old.shape[dim]).copy_(old)
    return new
