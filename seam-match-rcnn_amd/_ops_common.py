"""What every launch wrapper shares: the two compute dtypes, the current HIP stream, the tensor checks and raw pointers.

torch is plumbing only -- device memory, the stream and ``data_ptr()`` values handed to ``libseam_hip.so``.  Every op requires
contiguous tensors on the HIP device and raises otherwise: there is no CPU / eager fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native

F32 = torch.float32
F16 = torch.float16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, dtype=F32, name: str = "tensor") -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _native.SeamNativeError(f"{name}: expected a tensor on the HIP device (no CPU path exists)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _req_fp(t: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    """fp32 or fp16 activation (the two precisions the library computes in)."""
    t = _req(t, None, name)
    if t.dtype not in (F32, F16):
        raise TypeError(f"{name}: expected float32 or float16, got {t.dtype}")
    return t


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _sfx(dtype) -> str:
    return "f32" if dtype == F32 else "f16"


def _mask_device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _native.SeamNativeError("masks are rasterised on the HIP device (no CPU path exists)")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _upload(ctypes_array, device) -> torch.Tensor:
    """A ctypes table as a uint8 device tensor (the caller keeps it alive while kernels read it)."""
    host = torch.frombuffer(bytearray(bytes(ctypes_array)), dtype=torch.uint8)
    return host.to(device)
