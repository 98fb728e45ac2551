"""Launch wrappers of the input kernels: preprocess, the uint8 batch paths with their noise, the MovingFashion frame path --
and the one pinned-staging routine through which a batch of host images crosses to the device."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _native
from ._ops_common import F16, F32, _mask_device, _ptr, _req, _stream

__all__ = ["preprocess", "preprocess_u8_flat", "stage_u8_batch", "preprocess_u8_batch", "noise_u8_batch", "frame_noise",
           "resize_bicubic_u8", "FRAME_AS_IS", "FRAME_RGB", "FRAME_NOISY_HALF", "frame_out_size", "frames_prepare_flat",
           "StagedFrames", "stage_frames", "launch_frames", "frames_prepare_batch"]


def preprocess(images: Sequence[torch.Tensor], sizes: Sequence[tuple], hp: int, wp: int, dtype=F32, s2d: bool = False,
               s2d_pad: tuple = (0, 0)) -> torch.Tensor:
    """normalise + resize + pad + CHW->NHWC for a list of fp32 images -> [N,hp,wp,4] fp32 / [N,hp,wp,8] fp16.
    ``s2d`` (fp32 [3,H,W] images only): the space-to-depth layout [N,hp/2,wp/2,12] of ``seam_preprocess_s2d_batch_f32``
    (fp16: [N,hp/2,wp/2,16], four zero channels, ``_f16``); ``s2d_pad`` = (lo, hi): zero cells before / after the frame in both
    directions -- [N, hp/2 + lo + hi, wp/2 + lo + hi, 12 | 16], the input of ``stem_s2d_sx`` / ``stem_s2d_f16`` with ``padded=True``."""
    lib = _native.lib()
    # device check FIRST, for every image and every branch below: a CPU tensor must raise SeamNativeError, never reach a
    # kernel as a raw host pointer (the one-launch batch branches take data_ptr() of the views directly)
    images = [_req(i, None, "image") for i in images]
    if not images:
        raise ValueError("preprocess: empty image list")
    if s2d:
        if dtype not in (F32, F16) or hp % 2 or wp % 2 or any(i.dtype != F32 or i.dim() != 3 or i.shape[0] != 3 for i in images):
            raise ValueError("preprocess(s2d=True): fp32 [3,H,W] images and an even padded size")
        n = len(images)
        plo, phi = int(s2d_pad[0]), int(s2d_pad[1])
        out = torch.empty((n, hp // 2 + plo + phi, wp // 2 + plo + phi, 12 if dtype == F32 else 16), dtype=dtype, device=images[0].device)
        if dtype == F32 and not (plo or phi):
            s2d_fn = lib.seam_preprocess_s2d_batch_f32
        else:
            pad_fn = lib.seam_preprocess_s2d_pad_batch_f32 if dtype == F32 else lib.seam_preprocess_s2d_pad_batch_f16

            def s2d_fn(src, stride, dst, cnt, ih, iw, oh, ow, hpp, wpp, st):
                return pad_fn(src, stride, dst, cnt, ih, iw, oh, ow, hpp, wpp, plo, phi, st)
        same = n <= 65535 and all(i.shape == images[0].shape and i.is_contiguous() for i in images) \
            and all(tuple(z) == tuple(sizes[0]) for z in sizes)
        p0 = images[0].data_ptr()
        step = (images[1].data_ptr() - p0) if n > 1 else 0
        if same and n > 1 and step > 0 and step % 4 == 0 and all(im.data_ptr() == p0 + k * step for k, im in enumerate(images)):
            _native.check(s2d_fn(C.c_void_p(p0), step // 4, _ptr(out), n, images[0].shape[1],
                                                            images[0].shape[2], sizes[0][0], sizes[0][1], hp, wp, _stream()),
                          "seam_preprocess_s2d_batch")
            return out
        for i, (img, (oh, ow)) in enumerate(zip(images, sizes)):
            img = _req(img, name="image")
            _native.check(s2d_fn(_ptr(img), 0, C.c_void_p(out[i].data_ptr()), 1, img.shape[1], img.shape[2],
                                                            oh, ow, hp, wp, _stream()), "seam_preprocess_s2d_batch")
        return out
    cs = 4 if dtype == F32 else 8
    out = torch.empty((len(images), hp, wp, cs), dtype=dtype, device=images[0].device)
    fn = lib.seam_preprocess_f32 if dtype == F32 else lib.seam_preprocess_f16
    # the frames of one clip tensor (a list of same-shape fp32 views at a constant stride): one launch for the batch
    n = len(images)
    if n > 1 and n <= 65535 and all(i.dtype == F32 and i.dim() == 3 and i.shape == images[0].shape and i.is_contiguous()
                                     and i.is_cuda for i in images) \
            and images[0].shape[0] == 3 and all(tuple(s) == tuple(sizes[0]) for s in sizes):
        p0 = images[0].data_ptr()
        step = images[1].data_ptr() - p0
        if step > 0 and step % 4 == 0 and all(im.data_ptr() == p0 + k * step for k, im in enumerate(images)):
            fb = lib.seam_preprocess_batch_f32 if dtype == F32 else lib.seam_preprocess_batch_f16
            _native.check(fb(C.c_void_p(p0), step // 4, _ptr(out), n, images[0].shape[1], images[0].shape[2], sizes[0][0],
                             sizes[0][1], hp, wp, _stream()), "seam_preprocess_batch")
            return out
    for i, (img, (oh, ow)) in enumerate(zip(images, sizes)):
        if img.dtype == torch.uint8:        # extension: raw HWC RGB frame, ToTensor fused (row f4)
            img = _req(img, torch.uint8, "image")
            if img.dim() != 3 or img.shape[2] != 3:
                raise ValueError("uint8 images must be [H,W,3]")
            _native.check(lib.seam_preprocess_u8(_ptr(img), C.c_void_p(out[i].data_ptr()), img.shape[0], img.shape[1], oh, ow,
                                                 hp, wp, 0 if dtype == F32 else 1, _stream()), "seam_preprocess_u8")
            continue
        img = _req(img, name="image")
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError("images must be [3,H,W]")
        _native.check(fn(_ptr(img), C.c_void_p(out[i].data_ptr()), img.shape[1], img.shape[2], oh, ow, hp, wp, _stream()),
                      "seam_preprocess")
    return out


def preprocess_u8_flat(flat: torch.Tensor, img_off: torch.Tensor, img_dims: torch.Tensor, hp: int, wp: int, s2d: bool,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``seam_preprocess_u8_batch_f32`` on device tables: ``flat`` uint8 [bytes] holds N HWC images, image i at byte
    ``img_off[i]`` (int64 [N]), ``img_dims`` int32 [N,5] = (in_h, in_w, out_h, out_w, flip) -> fp32 [N,hp,wp,4] or, ``s2d``,
    [N,hp/2,wp/2,12].  One launch; every cell of the result is written (``out``: a tensor of that shape to write into)."""
    flat, img_off, img_dims = _req(flat, torch.uint8, "flat"), _req(img_off, torch.int64, "img_off"), _req(img_dims, torch.int32, "img_dims")
    n = img_off.numel()
    hp, wp = int(hp), int(wp)
    if flat.dim() != 1 or img_off.dim() != 1 or tuple(img_dims.shape) != (n, 5):
        raise ValueError("preprocess_u8_flat: flat uint8 [bytes], img_off int64 [N] and img_dims int32 [N,5] are needed")
    if not 1 <= n <= 65535:
        raise ValueError(f"preprocess_u8_flat: 1 <= N <= 65535 images per launch, got {n}")
    if s2d and (hp % 2 or wp % 2):
        raise ValueError("preprocess_u8_flat(s2d=True): an even padded size is needed")
    shape = (n, hp // 2, wp // 2, 12) if s2d else (n, hp, wp, 4)
    if out is None:
        out = torch.empty(shape, dtype=F32, device=flat.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == F32 and tuple(out.shape) == shape and out.is_contiguous()
              and out.device == flat.device):
        raise ValueError(f"preprocess_u8_flat: out must be a contiguous fp32 {shape} tensor on {flat.device}")
    with torch.cuda.device(flat.device):
        _native.check(_native.lib().seam_preprocess_u8_batch_f32(_ptr(flat), flat.numel(), _ptr(img_off), _ptr(img_dims), _ptr(out), n,
                                                                 hp, wp, 1 if s2d else 0, _stream()), "seam_preprocess_u8_batch_f32")
    return out


_STAGING = {}      # (device, thread) -> (pinned uint8 buffer, event of the last copy out of it)


def _staging_key(device):
    import threading
    return (device, threading.get_ident())


def _staging(nbytes: int, device) -> torch.Tensor:
    """The calling thread's pinned staging buffer for ``device``, grown when needed; the copy that last read it has finished when
    this returns.  One buffer per device and thread: two threads that prepare batches at once never share bytes, and within a
    thread a buffer is written only after its last copy's event, whichever stream carried that copy."""
    key = _staging_key(device)
    buf, ev = _STAGING.get(key, (None, None))
    if ev is not None:
        ev.synchronize()
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty((max(nbytes, 1 << 20),), dtype=torch.uint8).pin_memory()
    _STAGING[key] = (buf, None)
    return buf


def _noise_tables(noise, n: int):
    """``(sigmas, seeds)`` of a batch -> the 16 * n table bytes the noise launch reads: float64 [n] sigmas, then uint64 [n] seeds."""
    import math
    import numpy as np
    sigmas, seeds = noise
    sigmas, seeds = [float(v) for v in sigmas], [int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds]
    if len(sigmas) != n or len(seeds) != n:
        raise ValueError("noise: one sigma and one seed per image are needed")
    if not all(math.isfinite(v) for v in sigmas):
        raise ValueError("noise: every sigma must be finite")
    return np.concatenate([np.asarray(sigmas, np.float64).view(np.uint8), np.asarray(seeds, np.uint64).view(np.uint8)])


def _check_u8_images(what: str, images) -> bool:
    """The checks every staged batch begins with -> whether the images lie on the device (all of them) or on the host."""
    # device check FIRST: no CPU path exists, and nothing below may run without a HIP device to write to
    if not torch.cuda.is_available() or not all(isinstance(i, torch.Tensor) for i in images):
        raise _native.SeamNativeError(f"{what}: expected uint8 tensors and a HIP device (no CPU path exists)")
    n = len(images)
    if not 1 <= n <= 65535:
        raise ValueError(f"{what}: 1 <= N <= 65535 images per launch, got {n}")
    on_dev = [i.is_cuda for i in images]
    if any(on_dev) and not all(on_dev):
        raise ValueError(f"{what}: the images must be all on the host or all on one HIP device")
    for i in images:
        if i.dtype != torch.uint8:
            raise TypeError(f"image: expected torch.uint8, got {i.dtype}")
        if i.dim() != 3 or i.shape[2] != 3 or i.shape[0] < 1 or i.shape[1] < 1:
            raise ValueError("uint8 images must be [H,W,3]")
    return all(on_dev)


def _batch_device(what: str, images, on_dev: bool, device):
    """The device a checked batch goes to: the one its images lie on, or ``device`` (default: the current HIP device)."""
    if not on_dev:
        return _mask_device(device if device is not None else "cuda")
    device = images[0].device
    if any(i.device != device for i in images):
        raise ValueError(f"{what}: the images must lie on one device")
    return device


def _pack_staging(tables, images, offsets, total: int, device, tail=None) -> torch.Tensor:
    """Host images into the pinned staging buffer of ``device`` -> the pinned uint8 view to copy: ``tables`` (uint8 bytes, padded
    to the header) from byte 0, image i from byte ``offsets[i]``, ``total`` bytes so far; ``tail``: further table bytes behind the
    last image, from the next multiple of 8 on, zeros in between."""
    at = (total + 7) // 8 * 8
    end = total if tail is None else at + tail.size
    stage = _staging(end, device)
    stage[:tables.size].copy_(torch.from_numpy(tables))
    for i, o in zip(images, offsets):
        stage[o:o + i.numel()].copy_(i.reshape(-1))
    if tail is not None:
        stage[total:at] = 0
        stage[at:end].copy_(torch.from_numpy(tail))
    return stage[:end]


def _to_device(tables, images, offsets, total: int, device, tail=None) -> torch.Tensor:
    """The transfer of a checked batch -> its flat uint8 device buffer.  Device images are joined behind the uploaded tables.  Host
    images (``tail``: theirs alone) are packed by ``_pack_staging`` and cross in ONE non-blocking copy, whose event is stored with
    the pinned buffer: ``_staging`` waits for it before the buffer is written again."""
    if images[0].is_cuda:
        return torch.cat([torch.from_numpy(tables).to(device)] + [i.contiguous().reshape(-1) for i in images])
    dev = _pack_staging(tables, images, offsets, total, device, tail).to(device, non_blocking=True)      # the batch's one host-to-device copy
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    _STAGING[_staging_key(device)] = (_STAGING[_staging_key(device)][0], ev)
    return dev


def _u8_tables(images_u8, sizes, hp: int, wp: int, flips):
    """The tables of ``seam_preprocess_u8_batch_f32`` -> (their bytes padded to the header: int64 [N] byte offsets, then int32 [N,5]
    dims; the offsets as a list; the bytes of header and images together)."""
    import numpy as np
    n = len(images_u8)
    dims = np.asarray([(int(i.shape[0]), int(i.shape[1]), int(s[0]), int(s[1]), int(f)) for i, s, f in zip(images_u8, sizes, flips)],
                      np.int32)
    if (dims[:, 2:4] < 1).any() or (dims[:, 2] > hp).any() or (dims[:, 3] > wp).any():
        raise ValueError("preprocess_u8_batch: every resized size must lie in [1, hp] x [1, wp]")
    nbytes = dims[:, 0].astype(np.int64) * dims[:, 1] * 3
    head = 32 * ((28 * n + 31) // 32)                     # tables first, the images from `head` on
    off = head + np.cumsum(nbytes) - nbytes
    tables = np.concatenate([off.astype(np.int64).view(np.uint8), dims.reshape(-1).view(np.uint8), np.zeros(head - 28 * n, np.uint8)])
    return tables, off.tolist(), int(head + nbytes.sum())


def stage_u8_batch(images_u8: Sequence[torch.Tensor], sizes: Sequence[tuple], hp: int, wp: int, flips, device, noise=None):
    """The host side of ``preprocess_u8_batch`` for host images: the tables (int64 byte offsets, then int32 [N,5] dims) and the
    images' bytes packed into the pinned staging buffer of ``device`` -> (the pinned uint8 view to copy, N).  ``noise`` =
    ``(sigmas, seeds)``: the view is 16 * N bytes longer at its end -- behind the last image, from the next multiple of 8 on, lie
    the float64 sigmas and the uint64 seeds of ``seam_noise_u8_batch``; everything before is what it is without ``noise``."""
    n = len(images_u8)
    tables, off, total = _u8_tables(images_u8, sizes, hp, wp, flips)
    if device is None:                                    # images that lie on the device already: the tables alone
        if noise is not None:
            raise ValueError("stage_u8_batch: the noise tables are staged with host images only")
        return torch.from_numpy(tables), n
    return _pack_staging(tables, images_u8, off, total, device, None if noise is None else _noise_tables(noise, n)), n


def _u8_batch_to_device(what: str, images_u8, sizes, hp: int, wp: int, flips, s2d: bool, device, noise):
    """The checks and the staging that ``preprocess_u8_batch`` and ``noise_u8_batch`` share -> (the flat device buffer: tables,
    images [, noise tables], its int64 offsets, its int32 [N,5] dims, the device float64 sigmas and uint64 seeds or None)."""
    on_dev = _check_u8_images(what, images_u8)
    n = len(images_u8)
    if len(sizes) != n or len(flips) != n:
        raise ValueError(f"{what}: one size and one flip per image are needed")
    if s2d and (int(hp) % 2 or int(wp) % 2):
        raise ValueError(f"{what}(s2d=True): an even padded size is needed")
    device = _batch_device(what, images_u8, on_dev, device)
    tables, off, total = _u8_tables(images_u8, sizes, hp, wp, flips)
    sig = seed = None
    if on_dev:
        dev = _to_device(tables, images_u8, off, total, device)
        if noise is not None:
            tail = torch.from_numpy(_noise_tables(noise, n)).to(device)
            sig, seed = tail[:8 * n].view(torch.float64), tail[8 * n:]
    else:
        dev = _to_device(tables, images_u8, off, total, device, None if noise is None else _noise_tables(noise, n))
        if noise is not None:
            at = dev.numel() - 16 * n
            sig, seed = dev[at:at + 8 * n].view(torch.float64), dev[at + 8 * n:]
    return dev, dev[:8 * n].view(torch.int64), dev[8 * n:28 * n].view(torch.int32).view(n, 5), sig, seed


def _launch_noise(dev, img_off, img_dims, sig, seed, draws=None, draws_off=None) -> None:
    with torch.cuda.device(dev.device):
        _native.check(_native.lib().seam_noise_u8_batch(_ptr(dev), dev.numel(), _ptr(img_off), _ptr(img_dims), _ptr(sig), _ptr(seed),
                                                        _ptr(draws), _ptr(draws_off), img_off.numel(), _stream()),
                      "seam_noise_u8_batch")


def preprocess_u8_batch(images_u8: Sequence[torch.Tensor], sizes: Sequence[tuple], hp: int, wp: int, flips: Optional[Sequence] = None,
                        s2d: bool = False, device=None, out: Optional[torch.Tensor] = None, noise=None) -> torch.Tensor:
    """ToTensor + horizontal flip + normalise + resize + pad + layout for a batch of uint8 [H,W,3] images of different sizes in ONE
    launch (``seam_preprocess_u8_batch_f32``): image i is resized to ``sizes[i]`` and flipped where ``flips[i]``; the result is
    what ``preprocess([to_tensor(img).flip(-1) if flip else to_tensor(img) ...], sizes, hp, wp, s2d=s2d)`` gives, bit for bit.
    The images are all host tensors -- packed with the tables into one pinned staging buffer, ONE host-to-device copy to
    ``device`` (default: the current HIP device) -- or all on one HIP device (``device`` is theirs).  ``noise`` =
    ``(sigmas, seeds)``, one each per image: ``seam_noise_u8_batch`` runs on the staged device buffer first, on the same stream
    (its tables travel in the same copy), so that the images preprocessed are the ones ``noise_u8_batch`` returns for these
    sigmas and seeds; the noise is keyed by the unflipped element index and the flip happens here, as the reference's dataset
    adds noise before its transform flips.  Without a HIP device: SeamNativeError, as every preprocess branch."""
    images_u8 = list(images_u8)
    flips = [False] * len(images_u8) if flips is None else [bool(f) for f in flips]
    dev, img_off, img_dims, sig, seed = _u8_batch_to_device("preprocess_u8_batch", images_u8, sizes, hp, wp, flips, s2d, device, noise)
    if noise is not None:
        _launch_noise(dev, img_off, img_dims, sig, seed)
    return preprocess_u8_flat(dev, img_off, img_dims, hp, wp, s2d, out)


def noise_u8_batch(images: Sequence[torch.Tensor], sigmas: Sequence[float], seeds: Sequence[int],
                   noise_values: Optional[Sequence[torch.Tensor]] = None, device=None) -> list:
    """The noise of the reference's ``MultiDeepFashion2Dataset.__getitem__`` for a batch of uint8 [H,W,3] RGB images of different
    sizes in ONE launch (``seam_noise_u8_batch``): image i becomes ``uint8(clip((img / 255.0 + n * sigmas[i]) * 255.0, 0, 255))`` in
    float64 with ``n`` = ``noise_values[i]`` (float64 [H,W,3] draws, e.g. ``np.random.randn``: the NumPy arithmetic bit for bit)
    or, without ``noise_values``, the counter-based draws of ``frame_noise`` for ``seeds[i]``; sigma 0 leaves an image as it is.
    Returns uint8 [H,W,3] device tensors, views of one buffer; the caller's tensors are never written.  The images are all host
    tensors (one pinned copy through the staging buffer) or all on one HIP device."""
    images = list(images)
    shapes = [tuple(i.shape) if isinstance(i, torch.Tensor) else None for i in images]
    if noise_values is not None:
        noise_values = list(noise_values)
        if len(noise_values) != len(images) or not all(isinstance(v, torch.Tensor) and v.dtype == torch.float64
                                                       and tuple(v.shape) == z for v, z in zip(noise_values, shapes)):
            raise ValueError("noise_u8_batch: noise_values must be one float64 tensor of the image's shape per image")
    own = [z[:2] if z is not None and len(z) == 3 else (1, 1) for z in shapes]     # a wrong image is refused below
    hp, wp = max((z[0] for z in own), default=1), max((z[1] for z in own), default=1)
    dev, img_off, img_dims, sig, seed = _u8_batch_to_device("noise_u8_batch", images, own, hp, wp, [False] * len(images), False,
                                                            device, (sigmas, seeds))
    draws = draws_off = None
    if noise_values is not None:
        draws = torch.cat([v.to(dev.device).reshape(-1) for v in noise_values])
        counts = [v.numel() for v in noise_values]
        draws_off = torch.tensor([sum(counts[:k]) for k in range(len(counts))], dtype=torch.int64).to(dev.device)
    _launch_noise(dev, img_off, img_dims, sig, seed, draws, draws_off)
    head, out = 32 * ((28 * len(images) + 31) // 32), []
    for h, w in own:
        out.append(dev[head:head + h * w * 3].view(h, w, 3))
        head += h * w * 3
    return out


# ------------------------------------------------------------------------------ input pipeline (row f4)
def frame_noise(bgr: torch.Tensor, sigma: float, noise: Optional[torch.Tensor] = None, seed: int = 0) -> torch.Tensor:
    """uint8 [H,W,3] BGR -> uint8 [H,W,3] RGB with additive noise (float64 maths, ref datasets/MFDataset.py:81-88).
    noise: float64 [H,W,3] standard-normal draws, or None for on-device counter-based draws keyed by ``seed``;
    sigma == 0 and noise None: channel flip only (the dataset's noise=False branch)."""
    bgr = _req(bgr, torch.uint8, "bgr")
    if bgr.dim() != 3 or bgr.shape[2] != 3:
        raise ValueError("frame must be uint8 [H,W,3]")
    if noise is not None:
        noise = _req(noise, torch.float64, "noise")
        if noise.shape != bgr.shape:
            raise ValueError("noise must have the frame's shape")
    out = torch.empty_like(bgr)
    _native.check(_native.lib().seam_frame_noise_u8(_ptr(bgr), _ptr(noise), _ptr(out), bgr.shape[0], bgr.shape[1], float(sigma),
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "seam_frame_noise_u8")
    return out


def resize_bicubic_u8(img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """``PIL.Image.resize((out_w, out_h))`` (BICUBIC, antialiased, 8-bit fixed point) on a uint8 [H,W,3] device image."""
    lib = _native.lib()
    img = _req(img, torch.uint8, "img")
    h, w = img.shape[0], img.shape[1]
    out = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=img.device)
    ws = torch.empty((int(lib.seam_resize_workspace_bytes(h, w, out_h, out_w)),), dtype=torch.uint8, device=img.device)
    _native.check(lib.seam_resize_bicubic_u8(_ptr(img), _ptr(out), h, w, out_h, out_w, _ptr(ws), _stream()), "seam_resize_bicubic_u8")
    return out


FRAME_AS_IS, FRAME_RGB, FRAME_NOISY_HALF = 0, 1, 2      # the modes of seam_frames_prepare_batch_u8


def frame_out_size(h: int, w: int, mode: int) -> tuple:
    """The size ``seam_frames_prepare_batch_u8`` writes an ``h`` x ``w`` image of ``mode`` at: halved for mode 2, else its own."""
    return (int(h) // 2, int(w) // 2) if int(mode) == FRAME_NOISY_HALF else (int(h), int(w))


def frames_prepare_flat(flat: torch.Tensor, in_off: torch.Tensor, dims: torch.Tensor, sigma: torch.Tensor, seed: torch.Tensor,
                        out: torch.Tensor, out_off: torch.Tensor, max_h: int, max_w: int, draws: Optional[torch.Tensor] = None,
                        draws_off: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``seam_frames_prepare_batch_u8`` on device tables: ``flat`` uint8 [bytes] holds N HWC images, image i at byte ``in_off[i]``
    (int64 [N]) with ``dims`` int32 [N,3] = (h, w, mode), ``sigma`` float64 [N], ``seed`` int64 [N] (the uint64 seeds' bits); the
    results go to ``out`` uint8 [bytes] at ``out_off`` (int64 [N]).  ``max_h`` / ``max_w``: the largest h and w.  ``draws`` float64
    [elements] + ``draws_off`` int64 [N]: given standard-normal draws instead of the generator's.  One launch; returns ``out``."""
    flat, out = _req(flat, torch.uint8, "flat"), _req(out, torch.uint8, "out")
    in_off, out_off = _req(in_off, torch.int64, "in_off"), _req(out_off, torch.int64, "out_off")
    dims, sigma, seed = _req(dims, torch.int32, "dims"), _req(sigma, torch.float64, "sigma"), _req(seed, torch.int64, "seed")
    n = in_off.numel()
    if flat.dim() != 1 or out.dim() != 1 or in_off.dim() != 1 or tuple(dims.shape) != (n, 3) \
            or any(tuple(t.shape) != (n,) for t in (out_off, sigma, seed)):
        raise ValueError("frames_prepare_flat: flat / out uint8 [bytes], in_off / out_off / seed int64 [N], sigma float64 [N] and "
                         "dims int32 [N,3] are needed")
    if not 1 <= n <= 65535:
        raise ValueError(f"frames_prepare_flat: 1 <= N <= 65535 images per launch, got {n}")
    if int(max_h) < 1 or int(max_w) < 1:
        raise ValueError("frames_prepare_flat: max_h and max_w must be positive")
    if (draws is None) != (draws_off is None):
        raise ValueError("frames_prepare_flat: draws and draws_off go together")
    if draws is not None:
        draws, draws_off = _req(draws, torch.float64, "draws"), _req(draws_off, torch.int64, "draws_off")
        if draws.dim() != 1 or tuple(draws_off.shape) != (n,):
            raise ValueError("frames_prepare_flat: draws float64 [elements] and draws_off int64 [N] are needed")
    if any(t.device != flat.device for t in (out, in_off, out_off, dims, sigma, seed, draws, draws_off) if t is not None):
        raise ValueError("frames_prepare_flat: every tensor must lie on one device")
    with torch.cuda.device(flat.device):
        _native.check(_native.lib().seam_frames_prepare_batch_u8(
            _ptr(flat), flat.numel(), _ptr(in_off), _ptr(dims), _ptr(sigma), _ptr(seed), _ptr(draws), _ptr(draws_off),
            0 if draws is None else draws.numel(), _ptr(out), out.numel(), _ptr(out_off), n, int(max_h), int(max_w), _stream()),
            "seam_frames_prepare_batch_u8")
    return out


class StagedFrames:
    """A frame batch on the device: ``dev`` (the flat buffer: tables, then the images' bytes) and views of its tables."""
    __slots__ = ("dev", "in_off", "out_off", "sigma", "seed", "dims", "pre_dims", "out_hw", "out_bytes", "max_h", "max_w")


def stage_frames(what: str, images, modes, sigmas, seeds, device, pre_dims=None) -> StagedFrames:
    """The checks and the staging of a frame batch.  Host images: the tables and the images' bytes are packed into the pinned
    staging buffer of ``device`` and cross in ONE copy; device images: the tables alone are uploaded and joined with the bytes
    there.  Tables, in this order from byte 0: int64 [N] input offsets (into the buffer itself), int64 [N] output offsets (packed
    from 0), float64 [N] sigmas, uint64 [N] seeds, int32 [N,3] (h, w, mode) and, with ``pre_dims`` (int32 [N,5] rows for
    ``seam_preprocess_u8_batch_f32``, which reads the output buffer with the output offsets), those."""
    import math
    import numpy as np
    on_dev = _check_u8_images(what, images)
    n = len(images)
    if len(modes) != n or len(sigmas) != n or len(seeds) != n:
        raise ValueError(f"{what}: one mode, one sigma and one seed per image are needed")
    modes, sigmas = [int(m) for m in modes], [float(s) for s in sigmas]
    if any(m not in (FRAME_AS_IS, FRAME_RGB, FRAME_NOISY_HALF) for m in modes):
        raise ValueError(f"{what}: a mode is 0 (as is), 1 (BGR -> RGB) or 2 (BGR -> RGB, noise, half resolution)")
    if not all(math.isfinite(s) for s in sigmas):
        raise ValueError(f"{what}: every sigma must be finite")
    if any(m == FRAME_NOISY_HALF and min(i.shape[0], i.shape[1]) < 2 for i, m in zip(images, modes)):
        raise ValueError(f"{what}: a frame that is halved needs at least 2 x 2 pixels")
    dims = np.asarray([(int(i.shape[0]), int(i.shape[1]), m) for i, m in zip(images, modes)], np.int32)
    out_hw = [frame_out_size(*d) for d in dims.tolist()]
    in_bytes = dims[:, 0].astype(np.int64) * dims[:, 1] * 3
    out_bytes = np.asarray([h * w * 3 for h, w in out_hw], np.int64)
    extra = None
    if pre_dims is not None:
        extra = np.ascontiguousarray(pre_dims, np.int32)
        if extra.shape != (n, 5) or [tuple(r) for r in extra[:, :2].tolist()] != out_hw:
            raise ValueError(f"{what}: pre_dims must be int32 [N,5] rows that start with the output sizes")
    size = 44 * n + (20 * n if extra is not None else 0)
    head = 32 * ((size + 31) // 32)
    in_off = head + np.cumsum(in_bytes) - in_bytes
    out_off = np.cumsum(out_bytes) - out_bytes
    parts = [in_off.astype(np.int64).view(np.uint8), out_off.astype(np.int64).view(np.uint8), np.asarray(sigmas, np.float64).view(np.uint8),
             np.asarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], np.uint64).view(np.uint8), dims.reshape(-1).view(np.uint8)]
    if extra is not None:
        parts.append(extra.reshape(-1).view(np.uint8))
    tables = np.concatenate(parts + [np.zeros(head - size, np.uint8)])
    total = int(head + in_bytes.sum())
    dev = _to_device(tables, images, in_off.tolist(), total, _batch_device(what, images, on_dev, device))
    st = StagedFrames()
    st.dev = dev
    st.in_off, st.out_off = dev[:8 * n].view(torch.int64), dev[8 * n:16 * n].view(torch.int64)
    st.sigma, st.seed = dev[16 * n:24 * n].view(torch.float64), dev[24 * n:32 * n].view(torch.int64)
    st.dims = dev[32 * n:44 * n].view(torch.int32).view(n, 3)
    st.pre_dims = dev[44 * n:64 * n].view(torch.int32).view(n, 5) if extra is not None else None
    st.out_hw, st.out_bytes = out_hw, int(out_bytes.sum())
    st.max_h, st.max_w = int(dims[:, 0].max()), int(dims[:, 1].max())
    return st


def launch_frames(st: StagedFrames, noise_values=None) -> torch.Tensor:
    """The frames launch on a staged batch -> the flat uint8 output buffer (image i at ``st.out_off[i]``, ``st.out_hw[i]``)."""
    draws = draws_off = None
    if noise_values is not None:
        device = st.dev.device
        given = [v.to(device).reshape(-1) for v in noise_values if v is not None]
        draws = torch.cat(given) if given else torch.zeros(1, dtype=torch.float64, device=device)
        offs, pos = [], 0
        for v in noise_values:
            offs.append(pos)
            pos += 0 if v is None else v.numel()
        draws_off = torch.tensor(offs, dtype=torch.int64).to(device)
    out = torch.empty((max(st.out_bytes, 1),), dtype=torch.uint8, device=st.dev.device)
    return frames_prepare_flat(st.dev, st.in_off, st.dims, st.sigma, st.seed, out, st.out_off, st.max_h, st.max_w, draws, draws_off)


def frames_prepare_batch(images: Sequence[torch.Tensor], modes: Sequence[int], sigmas: Sequence[float], seeds: Sequence[int],
                         noise_values: Optional[Sequence] = None, device=None) -> list:
    """The per-frame work of the reference's ``MovingFashionDataset.__getitem__`` for a batch of uint8 [H,W,3] images of different
    sizes in ONE launch (``seam_frames_prepare_batch_u8``).  ``modes[i]``: 0 -- the image as it is (the RGB shop image, the zero
    placeholder of an unreadable frame); 1 -- BGR -> RGB (``noise=False``); 2 -- BGR -> RGB, noise of ``sigmas[i]``, then Pillow's
    BICUBIC resize to ``(H // 2, W // 2)``: what ``resize_bicubic_u8(frame_noise(bgr, sigma, noise, seed), H // 2, W // 2)`` gives,
    bit for bit, with no full-resolution intermediate.  The draws are ``noise_values[i]`` (float64 [H,W,3], or None for an image
    that is not mode 2) or, without ``noise_values``, the counter-based ones of ``frame_noise`` for ``seeds[i]``.
    Returns uint8 [h,w,3] RGB device tensors, views of one buffer; the caller's tensors are never written.  The images are all
    host tensors (one pinned copy through the staging buffer, the tables in the same copy, to ``device``, default: the current
    HIP device) or all on one HIP device.  Without a HIP device: SeamNativeError."""
    images, modes = list(images), list(modes)
    if noise_values is not None:
        noise_values = list(noise_values)
        ok = len(noise_values) == len(images) == len(modes)
        for v, i, m in zip(noise_values, images, modes):
            if m == FRAME_NOISY_HALF or v is not None:
                ok = ok and isinstance(v, torch.Tensor) and isinstance(i, torch.Tensor) and v.dtype == torch.float64 \
                    and tuple(v.shape) == tuple(i.shape)
        if not ok:
            raise ValueError("frames_prepare_batch: noise_values must hold one float64 tensor of the image's shape per mode-2 image")
        noise_values = [v if m == FRAME_NOISY_HALF else None for v, m in zip(noise_values, modes)]
    st = stage_frames("frames_prepare_batch", images, modes, list(sigmas), list(seeds), device)
    flat = launch_frames(st, noise_values)
    out, pos = [], 0
    for h, w in st.out_hw:
        out.append(flat[pos:pos + h * w * 3].view(h, w, 3))
        pos += h * w * 3
    return out
