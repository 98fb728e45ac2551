"""Launch wrappers of the element-wise and layout kernels: pooling, the top-down add, NCHW <-> NHWC, row concatenation, RoIAlign."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _native
from ._ops_common import F32, _ptr, _req, _req_fp, _sfx, _stream

__all__ = ["maxpool2d", "upsample_add_", "nchw_to_nhwc", "nhwc_to_nchw", "avgpool", "cat_rows", "roi_align"]


def maxpool2d(x: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    x = _req_fp(x)
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
    fn = getattr(_native.lib(), "seam_maxpool2d_" + _sfx(x.dtype))
    _native.check(fn(_ptr(x), _ptr(y), n, h, w, c, k, stride, pad, _stream()), "seam_maxpool2d")
    return y


def upsample_add_(lat: torch.Tensor, top: torch.Tensor) -> torch.Tensor:
    lat, top = _req_fp(lat), _req(top, lat.dtype)
    n, h, w, c = lat.shape
    fn = getattr(_native.lib(), "seam_upsample_add_" + _sfx(lat.dtype))
    _native.check(fn(_ptr(lat), _ptr(top), n, h, w, top.shape[1], top.shape[2], c, _stream()), "seam_upsample_add")
    return lat


def nchw_to_nhwc(x: torch.Tensor, dtype=F32) -> torch.Tensor:
    """fp32 [B,C,*sp] (the reference's layout) -> [B,*sp,C] in the library's compute dtype."""
    x = _req(x)
    b, c = x.shape[0], x.shape[1]
    l = x[0, 0].numel() if b else 0
    y = torch.empty((b,) + tuple(x.shape[2:]) + (c,), dtype=dtype, device=x.device)
    if b:
        fn = _native.lib().seam_nchw_to_nhwc_f32 if dtype == F32 else _native.lib().seam_nchw_f32_to_nhwc_f16
        _native.check(fn(_ptr(x), _ptr(y), b, c, l, _stream()), "seam_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    """[B,*sp,C] fp32 / fp16 -> fp32 [B,C,*sp] (the reference's layout and dtype)."""
    x = _req_fp(x)
    b, c = x.shape[0], x.shape[-1]
    sp = tuple(x.shape[1:-1])
    l = 1
    for s in sp:
        l *= s
    y = torch.empty((b, c) + sp, dtype=F32, device=x.device)
    if b:
        fn = _native.lib().seam_nhwc_to_nchw_f32 if x.dtype == F32 else _native.lib().seam_nhwc_f16_to_nchw_f32
        _native.check(fn(_ptr(x), _ptr(y), b, l, c, _stream()), "seam_nhwc_to_nchw")
    return y


def avgpool(x: torch.Tensor) -> torch.Tensor:
    """NHWC [K,h,w,C] -> [K,C] mean over the spatial positions (fp32 accumulate)."""
    x = _req_fp(x)
    k, c = x.shape[0], x.shape[-1]
    l = x[0].numel() // c if k else 0
    y = torch.empty((k, c), dtype=x.dtype, device=x.device)
    if k:
        fn = getattr(_native.lib(), "seam_avgpool_" + _sfx(x.dtype))
        _native.check(fn(_ptr(x), _ptr(y), k, l, c, _stream()), "seam_avgpool")
    return y


def cat_rows(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    """``torch.cat(parts, 0)`` without the copy when the parts are consecutive dim-0 slices of one allocation with equal
    strides (the per-image ``roi_features`` / ``match_features`` views the model hands out are): returns the covering view."""
    parts = list(parts)
    if len(parts) == 1:
        return parts[0]
    p0 = parts[0]
    if p0.dim() >= 1 and p0.shape[0] > 0:
        st, es, ptr, rows, ok = p0.stride(), p0.element_size(), p0.data_ptr(), 0, True
        for p in parts:
            if (p.dtype != p0.dtype or p.device != p0.device or p.shape[1:] != p0.shape[1:] or p.shape[0] == 0 or p.stride() != st
                    or p.untyped_storage().data_ptr() != p0.untyped_storage().data_ptr() or p.data_ptr() != ptr + rows * st[0] * es):
                ok = False
                break
            rows += p.shape[0]
        if ok:
            return p0.as_strided((rows,) + tuple(p0.shape[1:]), st, p0.storage_offset())
    return torch.cat(parts, 0)


# ------------------------------------------------------------------------------ RoIAlign
def roi_align(feats: Sequence[torch.Tensor], rois: torch.Tensor, scales: Sequence[float], pooled: int,
              sampling_ratio: int = 2, k_min: int = 2, levels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feats: 4 NHWC maps (fp32 or fp16); rois fp32 [K,5] (batch_idx,x1,y1,x2,y2) -> NHWC [K,P,P,C]."""
    feats = [_req_fp(f) for f in feats]
    dt = feats[0].dtype
    rois = _req(rois, name="rois")
    k = rois.shape[0]
    c = feats[0].shape[-1]
    out = torch.empty((k, pooled, pooled, c), dtype=dt, device=rois.device)
    if k == 0:
        return out
    hw = (C.c_int * 8)(*[d for f in feats for d in (f.shape[1], f.shape[2])])
    if levels is not None:
        levels = _req(levels, torch.int32, "levels")
    fn = getattr(_native.lib(), "seam_roi_align_" + _sfx(dt))
    _native.check(fn(_ptr(feats[0]), _ptr(feats[1]), _ptr(feats[2]), _ptr(feats[3]), hw, c, scales[0], scales[1],
                     scales[2], scales[3], k_min, _ptr(rois), _ptr(levels), _ptr(out), k, pooled, sampling_ratio,
                     _stream()), "seam_roi_align")
    return out
