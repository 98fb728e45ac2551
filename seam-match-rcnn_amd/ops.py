"""Launch wrappers over the C ABI (``include/seam_hip.h``): torch tensors in, torch tensors out.

torch is plumbing only here -- device memory (``torch.empty``), the current HIP stream
and raw ``data_ptr()`` values handed to ``libseam_hip.so``.  Every op requires CUDA(HIP)
fp32 contiguous tensors and raises otherwise: there is no CPU / eager fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _native
from .models.packed import PackedWeights

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


# ------------------------------------------------------------------------------ conv
@dataclass
class PackedConv:
    """Weights of one conv/linear in the kernel's layout + its fused epilogue vectors."""
    w: torch.Tensor                 # [rows_padded, kred]
    scale: Optional[torch.Tensor]   # [K] or None
    shift: Optional[torch.Tensor]   # [K] or None
    K: int
    Cstore: int
    R: int
    S: int
    stride: int = 1
    pad: int = 0
    Cin: int = 0                    # real (unpadded) input channels: algorithmic FLOP accounting
    dtype: object = F32             # operand precision of the packed weights: torch.float32 | torch.float16 | BX3 | SX6 | SX9
    u: Optional[torch.Tensor] = None  # fp32 stride-1 3x3 layers: Winograd F(2x2,3x3) weights (seam_pack_conv_weight_wino_f32)
    u24: Optional[torch.Tensor] = None  # ... and F(2x4,3x3) weights (seam_pack_conv_weight_wino24_f32)
    wn: Optional[torch.Tensor] = None   # fp32 1x1 layers with <= 16 outputs: register-resident weights of seam_linear_narrow_f32
    ws: Optional[torch.Tensor] = None   # fp32 1x1 / stride-1 layers with C <= 256: row-major [K, C] weights (scale folded) of seam_conv1x1_sw_f32
    shift_sw: Optional[torch.Tensor] = None   # ... and its shift vector (zeros when the layer has none)
    wq: Optional[torch.Tensor] = None   # fp32 1x1 / stride-1 layers with C >= 256 (a multiple of 128), K % 128 == 0: fragment-order weights of seam_conv1x1_pc_f32
    wh: Optional[torch.Tensor] = None   # fp16 stride-1 3x3 layers (C, K multiples of 128, or C = K = 64): fragment-order weights of seam_conv3x3_f16pc
    wsh: Optional[torch.Tensor] = None  # fp16 1x1 / stride-1 layers (C multiple of 64, <= 512): row-major fp16 [K, C] weights of seam_conv1x1_swh_f16
    wph: Optional[torch.Tensor] = None  # fp16 1x1 / stride-1 layers with C >= 512 (a multiple of 256), K a multiple of 128: fragment-order weights of seam_conv1x1_f16pc
    wx: Optional[torch.Tensor] = None   # SX6 1x1 / stride-1 layers with C >= 256 (a multiple of 64), K a multiple of 128: three bf16 planes in fragment order (seam_conv1x1_sxpc)
    wxs: Optional[torch.Tensor] = None  # SX6 1x1 / stride-1 layers with C == 128, K a multiple of 128: the same planes (seam_conv1x1_sxpc_short, seam_conv1x1_sxpc_dual_short)
    u24x: Optional[torch.Tensor] = None  # SX6 stride-1 3x3 layers (C, K multiples of 64): F(2x4,3x3) weights as three bf16 planes (seam_pack_conv_weight_wino24_sx)
    wx64: Optional[torch.Tensor] = None  # SX6 1x1 / stride-1 layers with K == 64, C >= 128 (a multiple of 64): the same planes, two n-tiles (seam_conv1x1_sxpc64, seam_stem_sxpc)


BX3 = "bf16x3"      # fp32 activations, split-bf16 operands (3 bf16 MFMAs per product, fp32 accumulate)
# fp32 activations and results, each operand cut into three bf16 pieces that sum to it exactly (csrc/seam_conv.hip conv_igemm_sx):
# six piece products per fp32 product (what is dropped is below one fp32 rounding of it) or all nine (the exact product)
SX6 = "bf16x6"
SX9 = "bf16x9"
_SX_TERMS = {SX6: 6, SX9: 9}


# Exact-fp32 path: run the stride-1 3x3 layers through the Winograd F(2x2,3x3) kernel (csrc/seam_wino.hip).  All fp32
# arithmetic; SEAM_WINOGRAD=0 keeps every layer on the implicit-GEMM kernel.
import os as _os
WINOGRAD = _os.environ.get("SEAM_WINOGRAD", "1") != "0"
# fp16 path: the stride-1 3x3 layers with C, K multiples of 128 through the producer / consumer kernel (csrc/seam_f16pc.hip);
# SEAM_F16PC=0 keeps them on the implicit GEMM
F16PC = _os.environ.get("SEAM_F16PC", "1") != "0"
F16PC64 = _os.environ.get("SEAM_F16PC64", "1") != "0"      # the C = K = 64 form (layer1's 3x3 layers; A/B switch)
# exact-fp32 path: the long-reduction 1x1 layers (C >= 256, a multiple of 128; K a multiple of 128) through the producer / consumer
# pointwise kernel (csrc/seam_pwpc.hip); SEAM_PWPC=0 keeps them on the implicit GEMM.  Layers the weights-stationary kernel takes
# (C <= 256) stay there.
PWPC = _os.environ.get("SEAM_PWPC", "1") != "0"
# fp16 path: the 1x1 / stride-1 layers through the streaming weights-stationary kernel (csrc/seam_pwh.hip, round 6); SEAM_PWH=0 keeps
# them on the implicit GEMM.  Maps of >= SW_MIN_HW pixels only -- a function of the map, like the fp32 rule.
SWH = _os.environ.get("SEAM_PWH", "1") != "0"
PWHPC = _os.environ.get("SEAM_PWHPC", "1") != "0"       # conv1x1_f16pc: the long-reduction fp16 1x1 layers (csrc/seam_pwhpc.hip)
PWHPC_MIN_C = int(_os.environ.get("SEAM_PWHPC_MIN_C", "1024"))  # reductions from this length on take it (C = 512 stays on conv1x1_swh: 1.04-1.2x alone, nothing in the step)
# split-bf16 path (SX6): the long 1x1 / stride-1 layers through the producer / consumer kernel (csrc/seam_pwsx.hip); SEAM_SXPC=0 keeps
# them on conv_igemm_sx.  The two kernels give the same bits, so the choice may depend on the batch: launches of at least
# SXPC_MIN_TILES tiles of 128 pixels x 128 channels take it -- every shape of a step does (1.05-1.26x); with fewer tiles than CUs the
# persistent blocks' long tiles lose to the implicit GEMM's smaller ones (196 tiles: 1.16x, 100 tiles: 0.87x, 40 tiles: 0.66x;
# profiles/sxpc_layer_ab.txt).  SXPC_RULE = False: every supported shape (tests, tools/sxpc_ab.py).  The two-source form
# (conv1x1_sxpc_dual, ``conv2d_dual`` on an SX6 pack) has no tile rule: it wins from one image on (profiles/sxpc_dual_layer_ab.txt).
# The upsampled-residual form (conv1x1_sxpc_up, ``conv2d_topdown`` on an SX6 pack) follows the tile rule: below it the un-fused
# conv_igemm_sx + upsample_add_ gives the same bits (profiles/sxpc_up_layer_ab.txt: the losing shapes have 10-50 tiles).
SXPC = _os.environ.get("SEAM_SXPC", "1") != "0"
SXPC_MIN_TILES = int(_os.environ.get("SEAM_SXPC_MIN_TILES", "196"))
SXPC_RULE = True
# The 64-output-channel form (conv1x1_sxpc64) behind ``conv2d``: layer1's two 256 -> 64 reductions.  Off by default: at a step's
# shape the kernel is level with conv_igemm_sx on them (profiles/stem_sxpc_layer_ab.txt); the form serves the stem
# (``stem_s2d_sx``), which does not look at this knob.  SEAM_SXPC64=1 routes them (same bits; tile rule as above, 64-channel tiles).
SXPC64 = _os.environ.get("SEAM_SXPC64", "0") != "0"
# The two-chunk reductions (C == 128: layer2's 128 -> 512 expansions with their residual; 64 + 64: layer1.0's shortcut GEMM) on
# conv1x1_sxpc / conv1x1_sxpc_dual through the `short` entries.  These layers' alternative is the EXACT conv1x1_sw, which rounds
# differently, so the body picks their twin by the map alone (``sxpc_short_map_ok``: an image's result never depends on the batch it
# rides in); on a twin, ``conv2d`` / ``conv2d_dual`` take the kernel by the usual rules and conv_igemm_sx (the same bits) otherwise.
# SEAM_SXPC_SHORT=0: the exact kernels, as before the entries existed.
SXPC_SHORT = _os.environ.get("SEAM_SXPC_SHORT", "1") != "0"
# split-bf16 path (SX6): the stride-1 3x3 layers that run F(2x4,3x3) through conv3x3_wino24sx (csrc/seam_wino24sx.hip), the Winograd
# position GEMMs as six-term split-bf16 products.  Its bits differ from conv3x3_wino24's, so a layer takes it by the map geometry
# alone (``w24sx_map_ok``), at every batch size.  The rule: reductions from W24SX_MIN_C channels on (at C = 64 the kernel is level
# with conv3x3_wino24pc), and maps on which ONE image is at least W24SX_MIN_BLOCKS blocks -- the kernel runs one block per CU and
# wins from a single image on there (1 x 100^2 x 256 -> 256, 160 blocks: 1.32x; 1 x 200^2: 1.19x), while on smaller maps it wins at
# a step's batch (1.10-1.30x at 40 / 80 frames) and loses 9-18 % on one or two images (80 blocks and fewer), so those stay on
# the fp32 kernel unless the knob is lowered (profiles/w24sx_layer_ab.txt).  SEAM_W24SX=0 / W24SX = False: the fp32 kernels, as
# before the kernel existed.
W24SX = _os.environ.get("SEAM_W24SX", "1") != "0"
W24SX_MIN_C = int(_os.environ.get("SEAM_W24SX_MIN_C", "128"))
W24SX_MIN_BLOCKS = int(_os.environ.get("SEAM_W24SX_MIN_BLOCKS", "128"))
F16PC_RULE = True      # dispatch by seam_conv3x3_f16pc_pays (False: every supported shape -- tests, tools/f16pc_ab.py)


def _pack_wino(lib, weight: torch.Tensor, K: int, cin: int, cs: int, mode: int):
    """Winograd weights of a stride-1 3x3 fp32 layer -> (u of F(2x2,3x3), u24 of F(2x4,3x3)); (None, None) where unsupported."""
    if not lib.seam_wino_supported(cs, K, 3, 3, 1):
        return None, None
    u = torch.empty((int(lib.seam_wino_weight_floats(K, cs)),), dtype=F32, device=weight.device)
    _native.check(lib.seam_pack_conv_weight_wino_f32(_ptr(weight), _ptr(u), K, cin, cs, mode, _stream()),
                  "seam_pack_conv_weight_wino_f32")
    u24 = torch.empty((int(lib.seam_wino24_weight_floats(K, cs)),), dtype=F32, device=weight.device)
    _native.check(lib.seam_pack_conv_weight_wino24_f32(_ptr(weight), _ptr(u24), K, cin, cs, mode, _stream()),
                  "seam_pack_conv_weight_wino24_f32")
    return u, u24


# F(2x4,3x3) (csrc/seam_wino24.hip): 0 = never, 1 = where it issues fewer MFMAs than F(2x2,3x3) (x WINO24_MARGIN), 2 = always
WINOGRAD24 = int(_os.environ.get("SEAM_WINOGRAD24", "1"))
WINO24_MARGIN = float(_os.environ.get("SEAM_WINO24_MARGIN", "0.95"))
_WINO24 = {}


def _wino24_pays(lib, n, h, w, c, k, pad) -> bool:
    if WINOGRAD24 >= 2:
        return True
    # decided on the map geometry alone (a canonical batch of 256 images): an image's result must not depend on the batch it
    # rides in (the two forms round differently), and the stacked layouts of small maps would make the ratio vary with n
    key = (h, w, c, k, pad)
    f = _WINO24.get(key)
    if f is None:
        s24, s22 = int(lib.seam_wino24_issue_slots(256, h, w, c, k, pad)), int(lib.seam_wino_issue_slots(256, h, w, c, k, pad))
        f = _WINO24[key] = s24 > 0 and s24 <= WINO24_MARGIN * s22
    return f


# <= 16-output 1x1 layers (RPN logits / deltas, mask logits) on the row-stream kernel of csrc/seam_narrow.hip (SEAM_NARROW=0: implicit GEMM)
NARROW = _os.environ.get("SEAM_NARROW", "1") != "0"
WINO_MIN_FILL = int(_os.environ.get("SEAM_WINO_MIN_FILL", "55"))    # % of tile slots in use below which the implicit GEMM wins
_WINO_FILL = {}


def _wino_pays(lib, n, h, w, c, k, pad) -> bool:
    # decided on the map geometry alone (a canonical batch of 256 images), like _wino24_pays: batch-independent results
    key = (h, w, c, k, pad)
    f = _WINO_FILL.get(key)
    if f is None:
        f = _WINO_FILL[key] = int(lib.seam_wino_slot_fill_pct(256, h, w, c, k, pad))
    return f >= WINO_MIN_FILL


# Short-reduction pointwise layers (1x1, stride 1, C <= 256) on the weights-stationary kernel of csrc/seam_pw.hip (SEAM_PW=0: implicit
# GEMM).  Decided on the map geometry alone -- maps of >= SW_MIN_HW pixels, any batch -- so that an image's (or a ROI's) result never
# depends on the batch it rides in (the two kernels round differently: folded scale, different k order).
SW = _os.environ.get("SEAM_PW", "1") != "0"
SW_MIN_HW = int(_os.environ.get("SEAM_PW_MIN_HW", "196"))


# maps of >= 50 x 50 pixels (a function of the map alone, like SW_MIN_HW: an image's result never depends on the batch it rides in): on
# the 25 x 25 maps a step's 80 frames are 3-6 tiles per CU and the kernel is level with the implicit GEMM (profiles/r05_pwpc_ab.txt)
PWPC_MIN_HW = int(_os.environ.get("SEAM_PWPC_MIN_HW", "2500"))


def _sw_ok(pc: "PackedConv", h: int, w: int) -> bool:
    return SW and pc.ws is not None and h * w >= SW_MIN_HW


def _swh_ok(pc: "PackedConv", h: int, w: int) -> bool:
    return SWH and pc.wsh is not None and h * w >= SW_MIN_HW


def _wino_form(lib, pc: "PackedConv", n, h, w, c, pad) -> int:
    """Winograd form of a stride-1 3x3 fp32 layer on an h x w map: 0 = none (implicit GEMM), 1 = F(2x2,3x3), 2 = F(2x4,3x3)."""
    if pc.u is None or not WINOGRAD or not _wino_pays(lib, n, h, w, c, pc.K, pad):
        return 0
    return 2 if pc.u24 is not None and WINOGRAD24 and _wino24_pays(lib, n, h, w, c, pc.K, pad) else 1


def _sxpc_tiles_ok(m: int, tiles_n: int) -> bool:
    """The tile rule of the split 1x1 kernels: m pixels x ``tiles_n`` n-tiles are at least SXPC_MIN_TILES tiles of 128 pixels, or
    SXPC_RULE is off (both read now: tests and tools assign them)."""
    return -(-m // 128) * tiles_n >= SXPC_MIN_TILES or not SXPC_RULE


def sxpc_short_map_ok(h: int, w: int, k: int) -> bool:
    """A two-chunk expansion with K outputs on an h x w map runs its split twin: ONE image fills SXPC_MIN_TILES tiles."""
    return bool(SXPC_SHORT and _sxpc_tiles_ok(h * w, k // 128))


def w24sx_map_ok(h: int, w: int, c: int, k: int, pad: int) -> bool:
    """A stride-1 3x3 layer (c -> k channels, ``pad``) on an h x w map runs its split twin on conv3x3_wino24sx: the kernel serves
    the shape, the reduction is long enough and one image is enough blocks to win, and the exact pack would run F(2x4,3x3) there (``_wino_pays`` /
    ``_wino24_pays``: where F(2x2) or the implicit GEMM issues less work, the layer stays on it).  The map geometry alone -- an
    image's result never depends on the batch it rides in."""
    lib = _native.lib()
    return bool(W24SX and WINOGRAD and WINOGRAD24 and c >= W24SX_MIN_C and lib.seam_conv3x3_wino24sx_supported(1, h, w, c, k, pad, 1) == 1
                and lib.seam_conv3x3_wino24sx_blocks(1, h, w, c, k, pad) >= max(W24SX_MIN_BLOCKS, 1)
                and _wino_pays(lib, 1, h, w, c, k, pad) and _wino24_pays(lib, 1, h, w, c, k, pad))


def _conv_route(lib, pc: "PackedConv", n, h, w, relu, has_residual, cropped, out_f32) -> str:
    """The kernel one ``conv2d`` launch takes.  First match wins; this order IS the precedence.  Integers, bools, which pack fields
    exist, the knobs above (read now: tests and tools assign them) and the library's host predicates -- no tensor data, no stream."""
    c, k, dt = pc.Cstore, pc.K, pc.dtype
    if (dt == SX6 and pc.u24x is not None and not cropped and relu in (0, 1, False, True) and pc.stride == 1
            and w24sx_map_ok(h, w, c, k, pc.pad)):
        return "wino24sx"
    if (dt == SX6 and pc.wx is not None and SXPC and not cropped and relu in (0, 1, False, True)
            and _sxpc_tiles_ok(n * h * w, k // 128) and lib.seam_conv1x1_sxpc_supported(n * h * w, c, k) == 1):
        return "sxpc"
    if (dt == SX6 and pc.wx64 is not None and SXPC and SXPC64 and not cropped and relu in (0, 1, False, True)
            and _sxpc_tiles_ok(n * h * w, 1) and lib.seam_conv1x1_sxpc64_supported(n * h * w, c, k) == 1):
        return "sxpc64"
    if (dt == SX6 and pc.wxs is not None and SXPC and SXPC_SHORT and not cropped and relu in (0, 1, False, True)
            and _sxpc_tiles_ok(n * h * w, k // 128) and lib.seam_conv1x1_sxpc_short_supported(n * h * w, c, k) == 1):
        return "sxpc_short"
    f16k = dt == F16 and not out_f32 and relu in (0, 1, False, True)      # what the fp16 routes below need: fp16 out, ReLU a flag
    if f16k and not cropped:
        if (pc.wph is not None and PWHPC and not has_residual and c >= PWHPC_MIN_C and h * w >= SW_MIN_HW
                and lib.seam_conv1x1_f16pc_supported(n * h * w, c, k) == 1):
            return "pwhpc"
        if _swh_ok(pc, h, w):
            return "swh"
    if pc.wn is not None and NARROW and not has_residual and not cropped:
        return "narrow"
    if dt == F32 and not cropped:
        if _sw_ok(pc, h, w):
            return "sw"
        if pc.wq is not None and PWPC and h * w >= PWPC_MIN_HW and lib.seam_conv1x1_pc_supported(n * h * w, c, k) == 1:
            return "pwpc"
        form = _wino_form(lib, pc, n, h, w, c, pc.pad)
        if form:
            return "wino24" if form == 2 else "wino"
    if cropped:            # (fp32 or fp16: conv2d has checked)
        return "crop"
    if (f16k and pc.wh is not None and F16PC and not has_residual
            and (lib.seam_conv3x3_f16pc_pays if F16PC_RULE else lib.seam_conv3x3_f16pc_supported)(n, h, w, c, k, pc.pad) == 1):
        return "f16pc"
    return "igemm"          # (like "crop": the instantiation is the pack's dtype)


# routes of one instantiation: their CONV_TRACE labels
_ROUTE_LABEL = {"wino24sx": "conv3x3_wino24sx", "sxpc": "conv1x1_sxpc", "sxpc64": "conv1x1_sxpc64", "sxpc_short": "conv1x1_sxpc_short", "pwhpc": "conv1x1_f16pc", "narrow": "linear_narrow", "pwpc": "conv1x1_pc", "f16pc": "conv3x3_f16pc"}
# the split 1x1 routes of ``conv2d`` (one signature): their launch entry and the pack field it reads
_SXPC_ENTRY = {"sxpc": ("seam_conv1x1_sxpc", "wx"), "sxpc_short": ("seam_conv1x1_sxpc_short", "wxs"), "sxpc64": ("seam_conv1x1_sxpc64", "wx64")}


def _conv_variant(lib, route: str, pc: "PackedConv", n, h, w, ho, wo) -> str:
    """The kernel's name for ``CONV_TRACE``, template arguments included, from the route ``_conv_route`` chose."""
    c, k = pc.Cstore, pc.K
    if route in _ROUTE_LABEL:
        return _ROUTE_LABEL[route]
    if route in ("sw", "swh"):
        return _sw_variant(lib, route, n * h * w, c, k)
    if route == "wino24":
        return ("conv3x3_wino24pc" if lib.seam_wino24_form(n, h, w, c, k, pc.pad) == 1
                else f"conv3x3_wino24<{lib.seam_wino24_variant(n, h, w, c, k, pc.pad)}>")
    if route == "wino":
        return f"conv3x3_wino<{lib.seam_wino_tile_variant(n, h, w, c, k, pc.pad)}>"
    return _igemm_variant(lib, pc.dtype, n * ho * wo, k, pc.R * pc.S)      # "igemm" and "crop" (the crop kernels are its instantiations)


def _sw_launch(lib, x, x2, pc, residual, y, m, c1, c2, relu, res_mode=0, ho=0, wo=0, rh=0, rw=0):
    _native.check(lib.seam_conv1x1_sw_f32(_ptr(x), _ptr(x2), _ptr(pc.ws), _ptr(pc.shift_sw), _ptr(residual), _ptr(y), m, c1, c2, pc.K,
                                          int(relu), res_mode, ho, wo, rh, rw, _stream()), "seam_conv1x1_sw_f32")


def _sw_variant(lib, route: str, m, c, k) -> str:
    """Label of the weights-stationary pointwise kernel of route "sw" (fp32) / "swh" (fp16)."""
    cfg = int((lib.seam_conv1x1_sw_config if route == "sw" else lib.seam_conv1x1_swh_config)(m, c, 0, k))
    return f"conv1x1_{route}<{cfg // 100},{cfg % 100}>"


def _igemm_variant(lib, dt, m, k, taps: int = 1, dual: bool = False) -> str:
    """Label of the implicit GEMM of precision ``dt`` (``dual``: ``conv2d_dual`` lists 128 x 128 where the tile table says 256 rows)."""
    tile = lib.seam_conv_tile_taps(3 if dt in _SX_TERMS else 2 if dt == BX3 else 1 if dt == F16 else 0, m, k, taps)
    if dual and tile // 1000 == 256:
        tile = 128128
    if dt in _SX_TERMS:
        return f"conv_igemm_sx<{tile // 1000},{tile % 1000},{_SX_TERMS[dt]}>"
    if dt == BX3:
        return f"conv_igemm_bx3<{tile // 1000},{tile % 1000}>"
    return f"conv_igemm<{'float' if dt == F32 else '_Float16'},{tile // 1000},{tile % 1000}>"


# When set to a list, every conv launch is bracketed by HIP events on the launch stream and
# (variant, algorithmic_flops, start_event, end_event, (n, h, w, c, k, r, stride), bytes_moved) is appended (bench.py's roofline leg).
CONV_TRACE = None


def _trace_begin(variant: str, flops: float, shape: tuple, nbytes: float):
    """Open the event bracket of one traced launch.  A launch site calls this only when ``CONV_TRACE`` is set --
    ``tr = CONV_TRACE is not None and _trace_begin(...)`` -- so an untraced launch pays one global read and one comparison."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tr = (CONV_TRACE, (variant, flops, e0, e1, shape, nbytes))
    e0.record()
    return tr


def _trace_end(tr) -> None:
    tr[1][3].record()
    tr[0].append(tr[1])


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, bn=None, *, stride: int = 1,
              pad: int = 0, cstore: Optional[int] = None, transposed2x2: bool = False,
              bn_eps: float = 1e-5, dtype: torch.dtype = F32, wino: bool = True, w24sx: bool = False) -> PackedConv:
    """Pack a PyTorch-layout weight for ``conv2d``.

    weight: Conv2d [K,Cin,R,S] | Linear [K,Cin] | (transposed2x2) ConvTranspose2d [Cin,Cout,2,2]
    bn:     optional (weight, bias, running_mean, running_var) folded into the epilogue:
            FrozenBatchNorm2d [TV] / BatchNorm1d eval (ref models/match_head.py:62).
    wino:   also pack Winograd F(2x2,3x3) weights for fp32 stride-1 3x3 layers (the inference path); the grad-enabled
            pass of the heads (autograd.py) packs per step and keeps the bit-exact fp32 fma chain of the implicit GEMM.
    w24sx:  an SX6 pack of a stride-1 3x3 layer also gets the planes of conv3x3_wino24sx (``u24x``): the twin of a layer whose exact
            pack runs F(2x4,3x3); ``conv2d`` on it takes that kernel where ``w24sx_map_ok`` holds and conv_igemm_sx elsewhere.
    dtype:  a tuple yields a tuple of packs of the ONE source (an exact pack and its split twin: the same shift tensor)."""
    if isinstance(dtype, tuple):
        return tuple(pack_conv(weight, bias, bn, stride=stride, pad=pad, cstore=cstore, transposed2x2=transposed2x2, bn_eps=bn_eps,
                               dtype=d, wino=wino, w24sx=w24sx) for d in dtype)
    lib = _native.lib()
    weight = _req(weight.detach(), name="weight")
    is_linear = not transposed2x2 and weight.dim() == 2      # a Linear runs on 1x1 maps: no weight form of the map-sized pointwise kernels
    if transposed2x2:
        cin, cout = weight.shape[0], weight.shape[1]
        K, R, S, mode = 4 * cout, 1, 1, 1
    else:
        if is_linear:
            weight = weight[:, :, None, None]
        if weight.dim() == 3:
            weight = weight[:, :, :, None]
        weight = weight.contiguous()
        K, cin, R, S = weight.shape
        mode = 0
    epv = 8 if dtype == F16 else 4
    cs = cstore if cstore is not None else ((cin + epv - 1) // epv) * epv
    rows = lib.seam_conv_rows_padded(K)
    plain = R == 1 and S == 1 and stride == 1 and pad == 0 and cs == cin      # a plain 1x1 layer: what every pointwise form below needs
    conv1x1 = plain and mode == 0 and not is_linear
    # the weight as a row-major fp32 [K, Cin] matrix, made on first use; of a Conv2d / Linear weight it is a view: the SAME storage
    rows_kc = functools.cache(lambda: (weight.permute(2, 3, 1, 0).reshape(K, cin) if transposed2x2 else weight.reshape(K, cin)).to(F32).contiguous())
    u = u24 = u24x = wh = wn = ws = shift_sw = wq = wsh = wph = None      # the optional forms: each set below where the layer is eligible
    sxw = dict(wx=None, wxs=None, wx64=None)
    if dtype == F32:
        kred = lib.seam_conv_kred(cs, R, S)
        wp = torch.empty((rows, kred), dtype=F32, device=weight.device)
        _native.check(lib.seam_pack_conv_weight_f32(_ptr(weight), _ptr(wp), K, cin, R, S, cs, mode, _stream()),
                      "seam_pack_conv_weight_f32")
        if wino and mode == 0 and R == 3 and S == 3 and stride == 1:
            u, u24 = _pack_wino(lib, weight, K, cin, cs, 0)
    elif dtype == BX3:
        kred = lib.seam_conv_kred(cs, R, S)
        wp = torch.empty((rows, kred), dtype=F32, device=weight.device)      # opaque: [32 hi | 32 lo] bf16 per 128-byte row-chunk
        tmp = torch.empty((rows, kred), dtype=F32, device=weight.device)
        _native.check(lib.seam_pack_conv_weight_bx3(_ptr(weight), _ptr(wp), _ptr(tmp), K, cin, R, S, cs, mode, _stream()),
                      "seam_pack_conv_weight_bx3")
    elif dtype in _SX_TERMS:
        kred = lib.seam_conv_kred(cs, R, S)
        wp = torch.empty((rows, kred * 3), dtype=torch.bfloat16, device=weight.device)      # opaque: three bf16 planes per chunk
        tmp = torch.empty((rows, kred), dtype=F32, device=weight.device)
        _native.check(lib.seam_pack_conv_weight_sx(_ptr(weight), _ptr(wp), _ptr(tmp), K, cin, R, S, cs, mode, _stream()),
                      "seam_pack_conv_weight_sx")
        # the forms of csrc/seam_pwsx.hip: (field, the library's rule, pack entry, layers it takes besides the plain 1x1 convs -- a
        # 2x2 / stride-2 transposed conv is the 1x1 conv of its [4 Cout, Cin] matrix: the same form)
        for field, ok, entry, also in (("wx", lib.seam_conv1x1_sxpc_supported, "seam_pack_conv1x1_weight_sxpc", plain and transposed2x2),
                                       ("wxs", lib.seam_conv1x1_sxpc_short_supported, "seam_pack_conv1x1_weight_sxpc_short", False),
                                       ("wx64", lib.seam_conv1x1_sxpc64_supported, "seam_pack_conv1x1_weight_sxpc64", False)):
            if SXPC and dtype == SX6 and (conv1x1 or also) and ok(1 << 20, cs, K):
                sxw[field] = torch.empty((int(lib.seam_conv1x1_sxpc_weight_bytes(K, cs)),), dtype=torch.uint8, device=weight.device)
                _native.check(getattr(lib, entry)(_ptr(rows_kc()), _ptr(sxw[field]), K, cs, _stream()), entry)
        if (w24sx and W24SX and dtype == SX6 and mode == 0 and R == 3 and S == 3 and stride == 1 and cs == cin
                and lib.seam_conv3x3_wino24sx_supported(1, 16, 16, cs, K, 1, 1)):
            u24x = torch.empty((int(lib.seam_wino24sx_weight_bytes(K, cs)),), dtype=torch.uint8, device=weight.device)
            _native.check(lib.seam_pack_conv_weight_wino24_sx(_ptr(weight), _ptr(u24x), K, cin, cs, 0, _stream()), "seam_pack_conv_weight_wino24_sx")
    else:
        kred = lib.seam_conv_kred_f16(cs, R, S)
        wp = torch.empty((rows, kred), dtype=F16, device=weight.device)
        _native.check(lib.seam_pack_conv_weight_f16(_ptr(weight), _ptr(wp), K, cin, R, S, cs, mode, _stream()),
                      "seam_pack_conv_weight_f16")
        if F16PC and mode == 0 and R == 3 and S == 3 and stride == 1 and pad in (0, 1) and ((cs % 128 == 0 and K % 128 == 0) or (cs == 64 and K == 64 and F16PC64)):
            wh = torch.empty((int(lib.seam_f16pc_weight_halves(K, cs)),), dtype=F16, device=weight.device)
            _native.check(lib.seam_pack_conv_weight_f16pc(_ptr(weight), _ptr(wh), K, cin, cs, _stream()), "seam_pack_conv_weight_f16pc")
    scale = shift = None
    if bias is not None:
        bias = bias.detach().to(F32)
        if transposed2x2:
            bias = bias.repeat(4)
    if bn is not None:
        bw, bb, rm, rv = (t.detach().to(F32) for t in bn)
        scale = (bw * torch.rsqrt(rv + bn_eps)).contiguous()
        shift = bb - rm * scale
        if bias is not None:
            shift = shift + bias * scale
        shift = shift.contiguous()
    elif bias is not None:
        shift = bias.contiguous()
    # (fp32 only: the same kernel on fp16 rows -- 8-byte loads, widened -- measured 1.7 % SLOWER end to end than the 128x64 fp16 tile)
    if dtype == F32 and mode == 0 and plain and scale is None and lib.seam_linear_narrow_supported(cs, K):
        wn = torch.empty((64 * cs,), dtype=F32, device=weight.device)
        _native.check(lib.seam_pack_linear_narrow_f32(_ptr(weight), _ptr(wn), K, cs, _stream()), "seam_pack_linear_narrow_f32")
    if dtype == F32 and mode in (0, 1) and plain and lib.seam_conv1x1_sw_config(1 << 20, cs, 0, K):
        # weights-stationary pointwise kernel (csrc/seam_pw.hip): plain row-major [K, C], the per-channel scale folded in
        # (without a scale ``ws`` IS the weight's storage: PackPlan skips its job by comparing the two pointers)
        ws = (rows_kc() * scale[:, None]).contiguous() if scale is not None else rows_kc()
        shift_sw = shift if shift is not None else torch.zeros((K,), dtype=F32, device=weight.device)
    if PWPC and dtype == F32 and conv1x1 and ws is None and lib.seam_conv1x1_pc_supported(1 << 20, cs, K):
        wq = torch.empty((int(lib.seam_conv1x1_pc_weight_floats(K, cs)),), dtype=F32, device=weight.device)
        _native.check(lib.seam_pack_conv1x1_pc_f32(_ptr(rows_kc()), _ptr(wq), K, cs, _stream()), "seam_pack_conv1x1_pc_f32")
    if SWH and dtype == F16 and mode in (0, 1) and plain and not is_linear and lib.seam_conv1x1_swh_config(1 << 20, cs, 0, K):
        wsh = rows_kc().to(F16).contiguous()
    if PWHPC and dtype == F16 and conv1x1 and lib.seam_conv1x1_f16pc_supported(1 << 20, cs, K):
        wph = torch.empty((int(lib.seam_conv1x1_f16pc_weight_halves(K, cs)),), dtype=F16, device=weight.device)
        _native.check(lib.seam_pack_conv1x1_weight_f16pc(_ptr(rows_kc()), _ptr(wph), K, cs, _stream()), "seam_pack_conv1x1_weight_f16pc")
    pc = PackedConv(wp, scale, shift, K, cs, R, S, stride=stride, pad=pad, Cin=cin, dtype=dtype, u=u, u24=u24, wn=wn, ws=ws,
                    shift_sw=shift_sw, wq=wq, wh=wh, wsh=wsh, wph=wph, u24x=u24x, **sxw)
    if _PACK_RECORDER is not None:
        _PACK_RECORDER.records.append((weight, bias, bn, mode, pc))
    return pc


def pack_conv_dgrad(weight: torch.Tensor, pad_fwd: int = 0, wino: bool = True) -> PackedConv:
    """Weights of the INPUT-GRADIENT conv of a stride-1 Conv2d / Linear with OIHW weight [Cout,Cin,R,S]:
    dX = conv2d(dY, pack_conv_dgrad(W))  (taps rotated 180 degrees, channels swapped, pad R-1-pad_fwd)."""
    lib = _native.lib()
    weight = _req(weight.detach(), name="weight")
    if weight.dim() == 2:
        weight = weight[:, :, None, None]
    weight = weight.contiguous()
    cout, cin, R, S = weight.shape
    if cout % 32 or R != S:
        raise ValueError("pack_conv_dgrad: Cout must be a multiple of 32 and the kernel square")
    rows = lib.seam_conv_rows_padded(cin)
    kred = lib.seam_conv_kred(cout, R, S)
    wp = torch.empty((rows, kred), dtype=F32, device=weight.device)
    _native.check(lib.seam_pack_conv_weight_f32(_ptr(weight), _ptr(wp), cin, cout, R, S, cout, 2, _stream()),
                  "seam_pack_conv_weight_f32")
    u, u24 = _pack_wino(lib, weight, cin, cout, cout, 2) if (wino and R == 3) else (None, None)
    return PackedConv(wp, None, None, cin, cout, R, S, stride=1, pad=R - 1 - pad_fwd, Cin=cout, dtype=F32, u=u, u24=u24)


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, R: int, S: int, stride: int = 1, pad: int = 0,
               out_hw: Optional[Sequence[int]] = None) -> torch.Tensor:
    """x NHWC [N,H,W,C], dy NHWC [N,Ho,Wo,K] -> dW in PyTorch OIHW layout [K,C,R,S] (fp32 MFMA, split over pixels).
    ``out_hw``: dy belongs to a conv cropped to its first ``out_hw`` output positions (``conv2d(..., out_hw=)``); it is read as it
    lies (``seam_conv_wgrad_crop_f32``)."""
    lib = _native.lib()
    x, dy = _req(x, name="x"), _req(dy, name="dy")
    n, h, w, c = x.shape
    k = dy.shape[-1]
    m = dy.numel() // k
    if out_hw is not None:
        ho, wo = int(out_hw[0]), int(out_hw[1])
        if tuple(dy.shape[:3]) != (n, ho, wo) or ho > (h + 2 * pad - R) // stride + 1 or wo > (w + 2 * pad - S) // stride + 1:
            raise ValueError(f"conv_wgrad: dy {tuple(dy.shape)} is not the output of this conv on x {tuple(x.shape)} cropped to {ho} x {wo}")
    dw = torch.empty((k, c, R, S), dtype=F32, device=x.device)
    ws = torch.empty((int(lib.seam_conv_wgrad_workspace_floats(m, c, k, R, S)),), dtype=F32, device=x.device)
    if out_hw is not None:
        _native.check(lib.seam_conv_wgrad_crop_f32(_ptr(x), _ptr(dy), _ptr(dw), n, h, w, c, k, R, S, stride, pad, ho, wo, _ptr(ws),
                                                   _stream()), "seam_conv_wgrad_crop_f32")
        return dw
    _native.check(lib.seam_conv_wgrad_f32(_ptr(x), _ptr(dy), _ptr(dw), n, h, w, c, k, R, S, stride, pad, _ptr(ws), _stream()),
                  "seam_conv_wgrad_f32")
    return dw


# seam_conv_wgrad_f32 indexes an operand with 32 bits: one of 2^31 bytes or more is split over images (FPN level 0 at
# 800x1333 passes that at 32 images).  A module constant so that a test can lower it.
WGRAD_MAX_OPERAND_BYTES = (1 << 31) - 1


def conv_wgrad_chunked(x: torch.Tensor, dy: torch.Tensor, R: int, S: int, stride: int = 1, pad: int = 0,
                       out_hw: Optional[Sequence[int]] = None) -> torch.Tensor:
    """``conv_wgrad`` for operands of any size: the images are split into equal consecutive chunks (the last may be shorter) whose
    operands stay within ``WGRAD_MAX_OPERAND_BYTES``, and the partial dW are added in chunk order -- a fixed order, so two calls
    give the same bits.  One chunk is exactly ``conv_wgrad``."""
    x, dy = _req(x, name="x"), _req(dy, name="dy")
    n = x.shape[0]
    if dy.shape[0] != n or n == 0:
        raise ValueError("conv_wgrad_chunked: x and dy need the same, non-zero number of images")
    per = max(x[0].numel(), dy[0].numel()) * 4
    if per > WGRAD_MAX_OPERAND_BYTES:
        raise ValueError(f"conv_wgrad_chunked: one image's operand ({per} bytes) exceeds the limit of {WGRAD_MAX_OPERAND_BYTES}")
    step = max(1, min(n, WGRAD_MAX_OPERAND_BYTES // per))
    if step >= n:
        return conv_wgrad(x, dy, R, S, stride, pad, out_hw)
    dw = None
    for i in range(0, n, step):
        part = conv_wgrad(x[i:i + step], dy[i:i + step], R, S, stride, pad, out_hw)
        dw = part if dw is None else dw.add_(part)
    return dw


def colsum(x: torch.Tensor) -> torch.Tensor:
    """[..., K] -> [K] sum over all leading dims (bias gradients)."""
    x = _req(x)
    k = x.shape[-1]
    m = x.numel() // k
    lib = _native.lib()
    out = torch.empty((k,), dtype=F32, device=x.device)
    ws = torch.empty((int(lib.seam_colsum_workspace_floats(m, k)),), dtype=F32, device=x.device)
    _native.check(lib.seam_colsum_f32(_ptr(x), _ptr(out), m, k, _ptr(ws), _stream()), "seam_colsum_f32")
    return out


def avgpool_relu_bwd(dpool: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dpool [N,C], y NHWC [N,H,W,C] (post-ReLU conv output) -> dy [N,H,W,C]."""
    dpool, y = _req(dpool), _req(y)
    n, h, w, c = y.shape
    dy = torch.empty_like(y)
    _native.check(_native.lib().seam_avgpool_relu_bwd_f32(_ptr(dpool), _ptr(y), _ptr(dy), n, h * w, c, _stream()),
                  "seam_avgpool_relu_bwd_f32")
    return dy


def bn1d_train_fwd(x, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """BatchNorm1d with batch statistics; running buffers (or None) updated in place -> (y, save_mean, save_invstd)."""
    x = _req(x)
    m, f = x.shape
    if m < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size " + str(tuple(x.shape)))
    y = torch.empty_like(x)
    mean = torch.empty((f,), dtype=F32, device=x.device)
    inv = torch.empty((f,), dtype=F32, device=x.device)
    _native.check(_native.lib().seam_bn1d_train_fwd_f32(_ptr(x), _ptr(_req(gamma.detach())), _ptr(_req(beta.detach())), _ptr(y),
                                                        _ptr(mean), _ptr(inv), _ptr(running_mean), _ptr(running_var), m, f,
                                                        float(momentum), float(eps), _stream()), "seam_bn1d_train_fwd_f32")
    return y, mean, inv


def ce2_fwd_bwd(logits: torch.Tensor, target: torch.Tensor, weight: torch.Tensor):
    """Weighted 2-class cross entropy (mean): logits [n,2], target int64 [n], weight [2] -> (loss [], dlogits [n,2])."""
    logits = _req(logits)
    target = _req(target.to(logits.device), torch.int64, "target")
    weight = _req(weight.to(logits.device))
    loss = torch.empty((), dtype=F32, device=logits.device)
    dl = torch.empty_like(logits)
    _native.check(_native.lib().seam_ce2_fwd_bwd_f32(_ptr(logits), _ptr(target), _ptr(weight), _ptr(loss), _ptr(dl),
                                                     logits.shape[0], _stream()), "seam_ce2_fwd_bwd_f32")
    return loss, dl


def bn1d_bwd(dy, x, save_mean, save_invstd, gamma, frozen: bool = False):
    dy, x = _req(dy), _req(x)
    m, f = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty((f,), dtype=F32, device=x.device)
    db = torch.empty((f,), dtype=F32, device=x.device)
    _native.check(_native.lib().seam_bn1d_bwd_f32(_ptr(dy), _ptr(x), _ptr(save_mean), _ptr(save_invstd), _ptr(_req(gamma.detach())),
                                                  _ptr(dx), _ptr(dg), _ptr(db), m, f, int(frozen), _stream()), "seam_bn1d_bwd_f32")
    return dx, dg, db


def pair_logits_bwd(a, b, w, g):
    """Gradients of ``pair_logits``: g [Q,G,2] -> (da [Q,256], db [G,256], dw [2,256], dbias [2])."""
    a, b, w, g = _req(a), _req(b), _req(w.detach()), _req(g)
    q, gg, d = a.shape[0], b.shape[0], a.shape[1]
    da, db = torch.zeros_like(a), torch.zeros_like(b)
    dw = torch.zeros((2, d), dtype=F32, device=a.device)
    dbias = torch.zeros((2,), dtype=F32, device=a.device)
    if q and gg:
        _native.check(_native.lib().seam_pair_logits_bwd_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(g), _ptr(da), _ptr(db), _ptr(dw),
                                                             _ptr(dbias), q, gg, d, _stream()), "seam_pair_logits_bwd_f32")
    return da, db, dw, dbias


def nlb_attnpool_bwd(seq, t_stride, s_stride, lens, n_seq, t_max, pk: "PackedNLB", dout, use_nlb=1):
    """Gradients of ``nlb_attnpool``: dout [S,256] -> (dseq like seq, [11 parameter gradients in the reference's layouts:
    theta.w, theta.b, phi.w, phi.b, g.w, g.b, concat_project.w, W.w, W.b, attention_scorer.w, attention_scorer.b])."""
    lib = _native.lib()
    seq, dout = _req(seq, name="seq"), _req(dout, name="dout")
    dev = seq.device
    dseq = torch.zeros_like(seq)
    shapes = [(128, 256, 1), (128,), (128, 256, 1), (128,), (128, 256, 1), (128,), (1, 256, 1, 1), (256, 128, 1), (256,), (1, 256), (1,)]
    grads = [torch.zeros(sh, dtype=F32, device=dev) for sh in shapes]
    if n_seq:
        ws = torch.empty((int(lib.seam_nlb_bwd_workspace_floats(n_seq, t_max)),), dtype=F32, device=dev)
        arr = (C.c_void_p * 11)(*[g.data_ptr() for g in grads])
        _native.check(lib.seam_nlb_attnpool_bwd_f32(_ptr(seq), t_stride, s_stride, _ptr(_req(lens, torch.int32, "lens")), n_seq, t_max,
                                                    _ptr(pk.w_proj_t), _ptr(pk.b_proj), _ptr(pk.w_cat), _ptr(pk.w_out_t),
                                                    _ptr(pk.b_out), _ptr(pk.w_att), _ptr(pk.b_att), _ptr(dout), _ptr(dseq), arr,
                                                    _ptr(ws), int(use_nlb), _stream()), "seam_nlb_attnpool_bwd_f32")
    return dseq, grads


def nlb_block_bwd(seq, t_stride, s_stride, lens, n_seq, t_max, pk: "PackedNLB", dz, dz_t_stride, dz_s_stride, use_nlb=2):
    """Gradients of the non-local block alone (the ``z`` output of ``nlb_attnpool``): dz rows -> (dseq like seq, [9 parameter
    gradients: theta.w, theta.b, phi.w, phi.b, g.w, g.b, concat_project.w, W.w, W.b])."""
    lib = _native.lib()
    seq, dz = _req(seq, name="seq"), _req(dz, name="dz")
    dev = seq.device
    dseq = torch.zeros_like(seq)
    shapes = [(128, 256, 1), (128,), (128, 256, 1), (128,), (128, 256, 1), (128,), (1, 256, 1, 1), (256, 128, 1), (256,)]
    grads = [torch.zeros(sh, dtype=F32, device=dev) for sh in shapes]
    if n_seq:
        ws = torch.empty((int(lib.seam_nlb_bwd_workspace_floats(n_seq, t_max)),), dtype=F32, device=dev)
        arr = (C.c_void_p * 9)(*[g.data_ptr() for g in grads])
        _native.check(lib.seam_nlb_block_bwd_f32(_ptr(seq), t_stride, s_stride, _ptr(_req(lens, torch.int32, "lens")), n_seq, t_max,
                                                 _ptr(pk.w_proj_t), _ptr(pk.b_proj), _ptr(pk.w_cat), _ptr(pk.w_out_t), _ptr(pk.b_out),
                                                 _ptr(dz), dz_t_stride, dz_s_stride, _ptr(dseq), arr, _ptr(ws), int(use_nlb), _stream()),
                      "seam_nlb_block_bwd_f32")
    return dseq, grads


def conv2d(x: torch.Tensor, pc: PackedConv, relu: bool = False, residual: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, out_f32: bool = False, out_hw: Optional[tuple] = None) -> torch.Tensor:
    """NHWC implicit-GEMM conv (+scale/shift, +residual, +ReLU) -> NHWC [N,Ho,Wo,K].
    The precision (fp32 exact / fp16 MFMA with fp32 accumulate) is that of the packed weights;
    ``out_f32`` makes the fp16 kernel write fp32 (hand-off to the fp32 descriptor heads)."""
    x = _req(x, None, "x")             # device check first: CPU tensors fail loudly
    x = _req(x, F16 if pc.dtype == F16 else F32, "x")
    n, h, w, c = x.shape
    if c != pc.Cstore:
        raise ValueError(f"conv2d: input has {c} channels, weights packed for {pc.Cstore}")
    ho = (h + 2 * pc.pad - pc.R) // pc.stride + 1
    wo = (w + 2 * pc.pad - pc.S) // pc.stride + 1
    if out_hw is not None:      # top-left crop of the output grid (``seam_conv2d_crop_f32``: the space-to-depth stem)
        if pc.dtype not in (F32, F16) or out_f32 or residual is not None or out_hw[0] > ho or out_hw[1] > wo:
            raise ValueError("conv2d: out_hw needs fp32 or fp16 weights, no residual and a size inside the full output")
        ho, wo = int(out_hw[0]), int(out_hw[1])
    ydt = F32 if (pc.dtype != F16 or out_f32) else F16
    if out is not None:
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != x.device or tuple(out.shape) != (n, ho, wo, pc.K)
                or out.dtype != ydt or not out.is_contiguous()):
            raise ValueError(f"conv2d: out must be a contiguous {ydt} tensor of shape {(n, ho, wo, pc.K)} on {x.device}")
    y = out if out is not None else torch.empty((n, ho, wo, pc.K), dtype=ydt, device=x.device)
    if residual is not None:
        residual = _req(residual, F16 if pc.dtype == F16 else F32, "residual")
        if residual.shape != y.shape:
            raise ValueError("conv2d: residual shape mismatch")
    lib = _native.lib()
    route = _conv_route(lib, pc, n, h, w, relu, residual is not None, out_hw is not None, out_f32)
    tr = CONV_TRACE is not None and _trace_begin(
        _conv_variant(lib, route, pc, n, h, w, ho, wo), 2.0 * n * ho * wo * pc.K * pc.R * pc.S * (pc.Cin or pc.Cstore), (n, h, w, c, pc.K, pc.R, pc.stride),
        float(x.element_size() * (x.numel() + pc.w.numel()) + y.element_size() * y.numel()
              + (x.element_size() * y.numel() if residual is not None else 0)))
    if route in _SXPC_ENTRY:
        entry, field = _SXPC_ENTRY[route]
        _native.check(getattr(lib, entry)(_ptr(x), _ptr(getattr(pc, field)), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y), n * h * w, c,
                                          pc.K, 1 if relu else 0, _stream()), entry)
    elif route == "pwhpc":
        _native.check(lib.seam_conv1x1_f16pc(_ptr(x), _ptr(pc.wph), _ptr(pc.scale), _ptr(pc.shift), None, _ptr(y), n * h * w, c, pc.K,
                                             1 if relu else 0, _stream()), "seam_conv1x1_f16pc")
    elif route == "swh":
        _native.check(lib.seam_conv1x1_swh_f16(_ptr(x), None, _ptr(pc.wsh), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                               n * h * w, c, 0, pc.K, 1 if relu else 0, 1 if residual is not None else 0, 0, 0, 0, 0,
                                               _stream()), "seam_conv1x1_swh_f16")
    elif route == "narrow":
        _native.check(lib.seam_linear_narrow_f32(_ptr(x), _ptr(pc.wn), _ptr(pc.shift), _ptr(y), n * h * w, c, pc.K, int(relu), _stream()),
                      "seam_linear_narrow_f32")
    elif route == "sw":
        _sw_launch(lib, x, None, pc, residual, y, n * h * w, c, 0, relu, 1 if residual is not None else 0)
    elif route == "pwpc":
        _native.check(lib.seam_conv1x1_pc_f32(_ptr(x), _ptr(pc.wq), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                              n * h * w, c, pc.K, int(relu), _stream()), "seam_conv1x1_pc_f32")
    elif route == "wino24sx":
        _native.check(lib.seam_conv3x3_wino24sx_f32(_ptr(x), _ptr(pc.u24x), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                                    n, h, w, c, pc.K, pc.pad, 1, int(relu), _stream()), "seam_conv3x3_wino24sx_f32")
    elif route == "wino24":
        _native.check(lib.seam_conv3x3_wino24_f32(_ptr(x), _ptr(pc.u24), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                                  n, h, w, c, pc.K, pc.pad, int(relu), _stream()), "seam_conv3x3_wino24_f32")
    elif route == "wino":
        _native.check(lib.seam_conv3x3_wino_f32(_ptr(x), _ptr(pc.u), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                                n, h, w, c, pc.K, pc.pad, int(relu), _stream()), "seam_conv3x3_wino_f32")
    elif route == "crop":             # (fp32 or fp16: checked above)
        crop = lib.seam_conv2d_crop_f16 if pc.dtype == F16 else lib.seam_conv2d_crop_f32
        _native.check(crop(_ptr(x), _ptr(pc.w), _ptr(pc.scale), _ptr(pc.shift), _ptr(y), n, h, w, c, pc.K,
                           pc.R, pc.S, pc.stride, pc.pad, ho, wo, int(relu), _stream()), "seam_conv2d_crop")
    elif route == "f16pc":
        _native.check(lib.seam_conv3x3_f16pc(_ptr(x), _ptr(pc.wh), _ptr(pc.scale), _ptr(pc.shift), None, _ptr(y),
                                             n, h, w, c, pc.K, pc.pad, 1 if relu else 0, _stream()), "seam_conv3x3_f16pc")
    elif pc.dtype == F32:
        _native.check(lib.seam_conv2d_f32(_ptr(x), _ptr(pc.w), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                          n, h, w, c, pc.K, pc.R, pc.S, pc.stride, pc.pad, int(relu), _stream()),
                      "seam_conv2d_f32")
    elif pc.dtype in _SX_TERMS:
        _native.check(lib.seam_conv2d_sx(_ptr(x), _ptr(pc.w), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                         n, h, w, c, pc.K, pc.R, pc.S, pc.stride, pc.pad, int(relu), _SX_TERMS[pc.dtype], _stream()),
                      "seam_conv2d_sx")
    elif pc.dtype == BX3:
        _native.check(lib.seam_conv2d_bx3(_ptr(x), _ptr(pc.w), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                          n, h, w, c, pc.K, pc.R, pc.S, pc.stride, pc.pad, int(relu), _stream()),
                      "seam_conv2d_bx3")
    else:
        _native.check(lib.seam_conv2d_f16(_ptr(x), _ptr(pc.w), _ptr(pc.scale), _ptr(pc.shift), _ptr(residual), _ptr(y),
                                          n, h, w, c, pc.K, pc.R, pc.S, pc.stride, pc.pad, 1 if relu else 0,
                                          1 if out_f32 else 0, _stream()), "seam_conv2d_f16")
    if tr:
        _trace_end(tr)
    return y


def stem_s2d_f16(x: torch.Tensor, w_rows: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                 relu: bool = True, padded: bool = False) -> torch.Tensor:
    """ResNet stem of the fp16 path on the space-to-depth frame ``x`` [N,H2,W2,16] (``preprocess(..., s2d=True)``) through the streaming
    kernel (``seam_stem_s2d_swh_f16``): the frame is zero-padded (2 cells before, 1 after) so that a tap is a constant shift of the
    flattened cell index -- ``padded=True``: ``x`` is that frame already, [N,H2+3,W2+3,16] (``preprocess(..., s2d_pad=(2, 1))``), else
    one padding copy is made.  ``w_rows`` fp16 [64,256], k = (4 r + s) * 16 + channel.  -> NHWC [N,H2,W2,64] fp16."""
    x = _req(x, F16, "x")
    n, h2, w2, c = x.shape
    if padded:
        h2, w2 = h2 - 3, w2 - 3
    if c != 16 or h2 < 1 or w2 < 1 or tuple(w_rows.shape) != (64, 256) or w_rows.dtype != F16:
        raise ValueError("stem_s2d_f16: x must be [N,H2,W2,16] fp16 (padded: +3 cells per direction) and w_rows [64,256] fp16")
    xp = x if padded else torch.nn.functional.pad(x, (0, 0, 2, 1, 2, 1))
    y = torch.empty((n, h2, w2, 64), dtype=F16, device=x.device)
    tr = CONV_TRACE is not None and _trace_begin("stem_swh<4,2>", 2.0 * n * h2 * w2 * 64 * 16 * 12, (n, h2, w2, 16, 64, 4, 1),
                                                 float(2 * (xp.numel() + w_rows.numel() + y.numel())))
    _native.check(_native.lib().seam_stem_s2d_swh_f16(_ptr(xp), _ptr(w_rows), _ptr(scale), _ptr(shift), _ptr(y), n, h2, w2,
                                                      1 if relu else 0, _stream()), "seam_stem_s2d_swh_f16")
    if tr:
        _trace_end(tr)
    return y


def stem_sx_ok(lib, pc: Optional["PackedConv"], n: int, hs: int, ws: int) -> bool:
    """``stem_s2d_sx`` serves N frames of hs x ws space-to-depth cells on this pack: the twin of the [64, 192] rows with its
    ``wx64``, ops.SXPC, a map of at least 128 output pixels (a rule on the map alone: a frame's result never depends on the batch it
    rides in) and the library's geometry rule.  Integers, the knob and the host predicate only."""
    return bool(pc is not None and pc.wx64 is not None and SXPC and pc.K == 64 and pc.Cstore == 192 and hs * ws >= 128
                and lib.seam_stem_sxpc_supported(n, hs, ws) == 1)


def stem_s2d_sx(x: torch.Tensor, pc: "PackedConv", relu: bool = True, padded: bool = False) -> torch.Tensor:
    """ResNet stem of the fp32 path's split class ``stem`` on the space-to-depth frame ``x`` [N,Hs,Ws,12]: the 4x4 / stride-1
    convolution as six-term split-bf16 products on the gather form of conv1x1_sxpc64 (``seam_stem_sxpc``).  ``padded``: ``x`` is the
    frame with its zero cells already, [N,Hs+3,Ws+3,12] (``preprocess(..., s2d_pad=(2, 1))``), else one padding copy is made.
    ``pc``: the SX6 pack of the [64, 192] rows in (r, s, c) order (``wx64``, scale, shift).  -> NHWC [N,Hs,Ws,64] fp32."""
    x = _req(x, F32, "x")
    n, hs, ws, c = x.shape
    if padded:
        hs, ws = hs - 3, ws - 3
    lib = _native.lib()
    if c != 12 or hs < 1 or ws < 1 or not stem_sx_ok(lib, pc, n, hs, ws):
        raise ValueError("stem_s2d_sx: x must be [N,Hs,Ws,12] fp32 (padded: +3 cells per direction) on a served map, pc the twin of the [64,192] rows")
    xp = x if padded else torch.nn.functional.pad(x, (0, 0, 2, 1, 2, 1))
    y = torch.empty((n, hs, ws, 64), dtype=F32, device=x.device)
    tr = CONV_TRACE is not None and _trace_begin("stem_sxpc", 2.0 * n * hs * ws * 64 * 16 * 12, (n, hs, ws, 12, 64, 4, 1),
                                                 float(4 * (xp.numel() + y.numel()) + pc.wx64.numel()))
    _native.check(lib.seam_stem_sxpc(_ptr(xp), _ptr(pc.wx64), _ptr(pc.scale), _ptr(pc.shift), _ptr(y), n, hs, ws, 1 if relu else 0,
                                     _stream()), "seam_stem_sxpc")
    if tr:
        _trace_end(tr)
    return y


def _sxpc_up_ok(lib, pc: "PackedConv", n, h, w, c, tn, th, tw, tk) -> bool:
    """``conv2d_topdown`` on an SX6 pack with ``wx`` takes ``seam_conv1x1_sxpc_up``: integers, the knobs and the library's host
    predicate only -- no tensor data, no stream."""
    return bool(SXPC and c == pc.Cstore and pc.R == 1 and pc.S == 1 and pc.stride == 1 and pc.pad == 0 and tn == n and tk == pc.K
                and _sxpc_tiles_ok(n * h * w, pc.K // 128) and lib.seam_conv1x1_sxpc_up_supported(n * h * w, n, h, w, c, pc.K, th, tw) == 1)


def conv2d_topdown(x: torch.Tensor, pc: PackedConv, top: torch.Tensor) -> torch.Tensor:
    """FPN top-down merge [TV]: conv(x) + nearest-upsample(top) -> NHWC.  Exact-fp32 weights: ONE launch (the coarse map is
    added in the conv epilogue, ``seam_conv2d_upres_f32``); a split-bf16 (SX6) pack with ``wx``: ONE launch of
    ``seam_conv1x1_sxpc_up`` when the launch has at least ``SXPC_MIN_TILES`` tiles; other precisions: conv + ``upsample_add_``.
    The fused and un-fused forms round identically."""
    if (pc.dtype == F16 and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and _swh_ok(pc, x.shape[1], x.shape[2])
            and x.shape[1] * x.shape[2] >= 128 and top.dim() == 4 and top.shape[0] == x.shape[0] and top.shape[3] == pc.K):
        # fp16 path (round 6): the merge in the streaming pointwise kernel's epilogue -- the lateral is never written and re-read
        x, top = _req(x, F16, "x"), _req(top, F16, "top")
        n, h, w, c = x.shape
        if c != pc.Cstore:
            raise ValueError(f"conv2d_topdown: input has {c} channels, weights packed for {pc.Cstore}")
        y = torch.empty((n, h, w, pc.K), dtype=F16, device=x.device)
        lib = _native.lib()
        tr = CONV_TRACE is not None and _trace_begin(
            _sw_variant(lib, "swh", n * h * w, c, pc.K), 2.0 * n * h * w * pc.K * (pc.Cin or pc.Cstore), (n, h, w, c, pc.K, 1, 1),
            float(2 * (x.numel() + pc.w.numel() + y.numel() + top.numel())))
        _native.check(lib.seam_conv1x1_swh_f16(_ptr(x), None, _ptr(pc.wsh), _ptr(pc.scale), _ptr(pc.shift), _ptr(top), _ptr(y),
                                               n * h * w, c, 0, pc.K, 0, 2, h, w, top.shape[1], top.shape[2], _stream()),
                      "seam_conv1x1_swh_f16")
        if tr:
            _trace_end(tr)
        return y
    if pc.dtype == SX6 and pc.wx is not None and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and top.dim() == 4:
        # split-bf16 lateral: the merge in conv1x1_sxpc's epilogue (csrc/seam_pwsx.hip conv1x1_sxpc_up).  The un-fused form below
        # gives the same bits, so the rule may look at the batch.
        n, h, w, c = x.shape
        if _sxpc_up_ok(_native.lib(), pc, n, h, w, c, top.shape[0], top.shape[1], top.shape[2], top.shape[3]):
            x, top = _req(x, F32, "x"), _req(top, F32, "top")
            y = torch.empty((n, h, w, pc.K), dtype=F32, device=x.device)
            tr = CONV_TRACE is not None and _trace_begin(
                "conv1x1_sxpc_up", 2.0 * n * h * w * pc.K * (pc.Cin or pc.Cstore), (n, h, w, c, pc.K, 1, 1),
                float(4 * (x.numel() + pc.K * c + y.numel() + top.numel())))
            _native.check(_native.lib().seam_conv1x1_sxpc_up(_ptr(x), _ptr(pc.wx), _ptr(pc.scale), _ptr(pc.shift), _ptr(top), _ptr(y), n, h, w, c,
                                                             pc.K, top.shape[1], top.shape[2], 0, _stream()), "seam_conv1x1_sxpc_up")
            if tr:
                _trace_end(tr)
            return y
    if pc.dtype != F32 or pc.K % 4:
        return upsample_add_(conv2d(x, pc), top)
    x = _req(x, None, "x")
    x, top = _req(x, F32, "x"), _req(top, F32, "top")
    n, h, w, c = x.shape
    if c != pc.Cstore:
        raise ValueError(f"conv2d_topdown: input has {c} channels, weights packed for {pc.Cstore}")
    ho = (h + 2 * pc.pad - pc.R) // pc.stride + 1
    wo = (w + 2 * pc.pad - pc.S) // pc.stride + 1
    if top.dim() != 4 or top.shape[0] != n or top.shape[3] != pc.K:
        raise ValueError("conv2d_topdown: top must be NHWC [N,Ht,Wt,K]")
    y = torch.empty((n, ho, wo, pc.K), dtype=F32, device=x.device)
    lib = _native.lib()
    sw = _sw_ok(pc, h, w) and h * w >= 64
    tr = CONV_TRACE is not None and _trace_begin(
        _sw_variant(lib, "sw", n * h * w, c, pc.K) if sw else _igemm_variant(lib, F32, n * ho * wo, pc.K),
        2.0 * n * ho * wo * pc.K * pc.R * pc.S * (pc.Cin or pc.Cstore), (n, h, w, c, pc.K, pc.R, pc.stride),
        float(4 * (x.numel() + pc.w.numel() + y.numel() + top.numel())))
    if sw:
        _sw_launch(lib, x, None, pc, top, y, n * h * w, c, 0, False, 2, ho, wo, top.shape[1], top.shape[2])
    else:
        _native.check(lib.seam_conv2d_upres_f32(_ptr(x), _ptr(pc.w), _ptr(pc.scale), _ptr(pc.shift), _ptr(top), _ptr(y),
                                                n, h, w, c, pc.K, pc.R, pc.S, pc.stride, pc.pad, top.shape[1], top.shape[2], 0,
                                                _stream()), "seam_conv2d_upres_f32")
    if tr:
        _trace_end(tr)
    return y


def pack_conv_dual(w1: torch.Tensor, bn1, w2: torch.Tensor, bn2, bn_eps: float = 1e-5, dtype=F32) -> PackedConv:
    """Weights of ``conv2d_dual``: two 1x1 convs, each followed by its own (Frozen)BatchNorm, summed.
    The scales are folded into the weights (one fp32 rounding per weight) and the shifts added:
    bn_a(W_a . h) + bn_b(W_b . x) = [s_a W_a | s_b W_b] . [h ; x] + (t_a + t_b).
    ``dtype``: fp32 / fp16 / SX6 (an eligible layer then has ``wx``, the form of ``seam_conv1x1_sxpc_dual``, beside ``w``); a tuple of
    them yields a tuple of packs of ONE folded matrix and shift (one ``derived_source`` each, whatever the number of packs)."""
    def fold(w, bn):
        bw, bb, rm, rv = (t.detach().to(F32) for t in bn)
        sc = bw * torch.rsqrt(rv + bn_eps)
        return w.detach().to(F32).reshape(w.shape[0], -1) * sc[:, None], bb - rm * sc
    w = derived_source(lambda: torch.cat([fold(w1, bn1)[0], fold(w2, bn2)[0]], 1).contiguous(), (w1, w2))
    shift = derived_source(lambda: (fold(w1, bn1)[1] + fold(w2, bn2)[1]).contiguous(), ())      # the two BN shifts: no parameter in it
    if isinstance(dtype, tuple):
        return tuple(pack_conv(w[:, :, None, None], shift, wino=False, dtype=d) for d in dtype)
    return pack_conv(w[:, :, None, None], shift, wino=False, dtype=dtype)


def _sxpc_dual_map_ok(n, ho, wo, h2, w2, c2) -> bool:
    """The geometry rule of ``seam_conv1x1_sxpc_dual`` (csrc/seam_pwsx.hip sxpc_src_plan; integers only): the images of x2 one tile
    of 128 output pixels touches lie within 2 GiB, and the producers' division by Wo is exact for every pixel of a map."""
    return 4 * h2 * w2 * c2 * min(n, 126 // (ho * wo) + 2) <= 1 << 31 and ho * wo * wo < 1 << 32


def conv2d_dual(x1: torch.Tensor, x2: torch.Tensor, pc: PackedConv, stride2: int = 1, relu: bool = False) -> torch.Tensor:
    """y = act(W[:, :C1] . x1 + W[:, C1:] . x2[:, ::stride2, ::stride2] + shift) in ONE launch (``seam_conv2d_dual_f32`` / ``_f16``;
    an SX6 pack: ``seam_conv1x1_sxpc_dual``, six-term split-bf16 products):
    the residual block with a projection shortcut [TV Bottleneck.forward] without writing the shortcut branch to memory.
    x1 NHWC [N,Ho,Wo,C1], x2 NHWC [N,H2,W2,C2] -> NHWC [N,Ho,Wo,K]; the operands' precision is the packed weights'."""
    x1 = _req(x1, None, "x1")
    if pc.dtype not in (F32, F16, SX6) or pc.R != 1 or pc.S != 1:
        raise ValueError("conv2d_dual: needs fp32 / fp16 / split-bf16 (SX6) 1x1 weights from pack_conv_dual")
    dt = F32 if pc.dtype == SX6 else pc.dtype
    x1, x2 = _req(x1, dt, "x1"), _req(x2, dt, "x2")
    n, ho, wo, c1 = x1.shape
    n2, h2, w2, c2 = x2.shape
    cm = 32 if dt == F32 else 64
    if n2 != n or c1 + c2 != pc.Cstore or c1 % cm or c2 % cm:
        raise ValueError(f"conv2d_dual: channel / batch mismatch (C1, C2 must be multiples of {cm} and sum to the packed width)")
    if stride2 < 1 or (ho - 1) * stride2 >= h2 or (wo - 1) * stride2 >= w2:
        raise ValueError("conv2d_dual: x2 too small for the output grid")
    lib = _native.lib()
    if pc.dtype == SX6:
        # six-term split-bf16 products (csrc/seam_pwsx.hip conv1x1_sxpc_dual).  Without the kernel (ops.SXPC off, no ``wx``, a shape
        # or a map it does not take) the sampled shortcut input is gathered, concatenated and multiplied by ``conv2d`` on the same
        # pack: conv_igemm_sx / conv1x1_sxpc on the materialised rows -- the same bits, one more pass over memory.
        # The two candidates in their order of preference: (trace label = the entry without "seam_", its pack, its own condition, its
        # stride argument -- the `short` entry takes none).
        for label, wpk, own, st in (("conv1x1_sxpc_dual", pc.wx, True, (stride2,)),
                                    ("conv1x1_sxpc_dual_short", pc.wxs, SXPC_SHORT and stride2 == 1, ())):
            entry = "seam_" + label
            if (SXPC and own and wpk is not None and relu in (0, 1, False, True)
                    and getattr(lib, entry + "_supported")(n * ho * wo, c1, c2, pc.K) == 1 and _sxpc_dual_map_ok(n, ho, wo, h2, w2, c2)):
                y = torch.empty((n, ho, wo, pc.K), dtype=F32, device=x1.device)
                tr = CONV_TRACE is not None and _trace_begin(
                    label, 2.0 * n * ho * wo * pc.K * (c1 + c2), (n, ho, wo, c1 + c2, pc.K, 1, 1),
                    float(x1.element_size() * (x1.numel() + n * ho * wo * c2 + pc.K * (c1 + c2) + y.numel())))
                _native.check(getattr(lib, entry)(_ptr(x1), _ptr(x2), _ptr(wpk), _ptr(pc.scale), _ptr(pc.shift), _ptr(y), n, ho, wo, c1,
                                                  h2, w2, c2, *st, pc.K, 1 if relu else 0, _stream()), entry)
                if tr:
                    _trace_end(tr)
                return y
        return conv2d(torch.cat([x1, x2[:, :(ho - 1) * stride2 + 1:stride2, :(wo - 1) * stride2 + 1:stride2]], -1), pc, relu=relu)
    y = torch.empty((n, ho, wo, pc.K), dtype=dt, device=x1.device)
    same = stride2 == 1 and (h2, w2) == (ho, wo)      # the pointwise kernels read both inputs on the output grid
    sw = dt == F32 and same and _sw_ok(pc, ho, wo)
    swh = dt == F16 and same and _swh_ok(pc, ho, wo) and lib.seam_conv1x1_swh_config(n * ho * wo, c1, c2, pc.K) != 0
    tr = CONV_TRACE is not None and _trace_begin(
        _sw_variant(lib, "sw" if sw else "swh", n * ho * wo, c1 + c2, pc.K) if sw or swh else _igemm_variant(lib, dt, n * ho * wo, pc.K, dual=True),
        2.0 * n * ho * wo * pc.K * (c1 + c2), (n, ho, wo, c1 + c2, pc.K, 1, 1),
        float(x1.element_size() * (x1.numel() + n * ho * wo * c2 + pc.w.numel() + y.numel())))
    if sw:
        _sw_launch(lib, x1, x2, pc, None, y, n * ho * wo, c1, c2, relu)
    elif swh:
        _native.check(lib.seam_conv1x1_swh_f16(_ptr(x1), _ptr(x2), _ptr(pc.wsh), _ptr(pc.scale), _ptr(pc.shift), None, _ptr(y),
                                               n * ho * wo, c1, c2, pc.K, 1 if relu else 0, 0, 0, 0, 0, 0, _stream()), "seam_conv1x1_swh_f16")
    else:
        fn = lib.seam_conv2d_dual_f32 if dt == F32 else lib.seam_conv2d_dual_f16
        _native.check(fn(_ptr(x1), _ptr(x2), _ptr(pc.w), _ptr(pc.scale), _ptr(pc.shift), _ptr(y), n, ho, wo, c1,
                         h2, w2, c2, stride2, pc.K, int(relu), _stream()), "seam_conv2d_dual")
    if tr:
        _trace_end(tr)
    return y


def linear(x: torch.Tensor, pc: PackedConv, relu: bool = False, out_f32: bool = False) -> torch.Tensor:
    """[M,C] x packed [K,C] -> [M,K] through the conv kernel (1x1 on a 1x1 map)."""
    m, c = x.shape
    return conv2d(x.view(m, 1, 1, c), pc, relu, out_f32=out_f32).view(m, pc.K)


def match_trunk(x: torch.Tensor, convs: Sequence[PackedConv], lin: PackedConv) -> torch.Tensor:
    """The match trunk in ONE ABI call (seam_match_trunk_f32): x NHWC fp32 [K,14,14,256], the four packed 3x3 convs and the packed
    Linear + BatchNorm1d -> x3 [K,256].  The form of every conv is decided here, by the rule ``conv2d`` applies (so the Python
    knobs SEAM_WINOGRAD / SEAM_WINOGRAD24 / SEAM_WINO_MIN_FILL act on both paths alike) and handed down."""
    lib = _native.lib()
    x = _req(x, F32, "x")
    k = x.shape[0]
    if tuple(x.shape[1:]) != (14, 14, 256) or len(convs) != 4 or any(pc.dtype != F32 for pc in list(convs) + [lin]):
        raise ValueError("match_trunk: fp32 NHWC [K,14,14,256] input and fp32-packed layers expected")
    out = torch.empty((k, 256), dtype=F32, device=x.device)
    if k == 0:
        return out

    def layer(pc):
        return _native.TrunkLayer(*(None if t is None else t.data_ptr() for t in (pc.w, pc.u, pc.u24, pc.scale, pc.shift)))
    layers = (_native.TrunkLayer * 4)(*[layer(pc) for pc in convs])
    form = (C.c_int * 4)()
    for i, (pc, h) in enumerate(zip(convs, (14, 12, 10, 8))):
        form[i] = _wino_form(lib, pc, k, h, h, 256, 0)
    ws = torch.empty((int(lib.seam_match_trunk_workspace_floats(k)),), dtype=F32, device=x.device)
    _native.check(lib.seam_match_trunk_f32(_ptr(x), layers, C.byref(layer(lin)), _ptr(out), k, _ptr(ws), form, _stream()),
                  "seam_match_trunk_f32")
    return out


# ------------------------------------------------------------------------------ elementwise
def _sfx(dtype) -> str:
    return "f32" if dtype == F32 else "f16"


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


def stage_u8_batch(images_u8: Sequence[torch.Tensor], sizes: Sequence[tuple], hp: int, wp: int, flips, device, noise=None):
    """The host side of ``preprocess_u8_batch`` for host images: the tables (int64 byte offsets, then int32 [N,5] dims) and the
    images' bytes packed into the pinned staging buffer of ``device`` -> (the pinned uint8 view to copy, N).  ``noise`` =
    ``(sigmas, seeds)``: the view is 16 * N bytes longer at its end -- behind the last image, from the next multiple of 8 on, lie
    the float64 sigmas and the uint64 seeds of ``seam_noise_u8_batch``; everything before is what it is without ``noise``."""
    import numpy as np
    n = len(images_u8)
    dims = np.asarray([(int(i.shape[0]), int(i.shape[1]), int(s[0]), int(s[1]), int(f)) for i, s, f in zip(images_u8, sizes, flips)],
                      np.int32)
    if (dims[:, 2:4] < 1).any() or (dims[:, 2] > hp).any() or (dims[:, 3] > wp).any():
        raise ValueError("preprocess_u8_batch: every resized size must lie in [1, hp] x [1, wp]")
    nbytes = dims[:, 0].astype(np.int64) * dims[:, 1] * 3
    head = 32 * ((28 * n + 31) // 32)                     # tables first, the images from `head` on
    off = head + np.cumsum(nbytes) - nbytes
    total = int(head + nbytes.sum())
    tables = np.concatenate([off.astype(np.int64).view(np.uint8), dims.reshape(-1).view(np.uint8)])
    if device is None:                                    # images that lie on the device already: the tables alone
        if noise is not None:
            raise ValueError("stage_u8_batch: the noise tables are staged with host images only")
        return torch.from_numpy(np.concatenate([tables, np.zeros(head - tables.size, np.uint8)])), n
    tail = None if noise is None else _noise_tables(noise, n)
    at = (total + 7) // 8 * 8
    stage = _staging(total if tail is None else at + tail.size, device)
    stage[:tables.size].copy_(torch.from_numpy(tables))
    for i, o, b in zip(images_u8, off.tolist(), nbytes.tolist()):
        stage[o:o + b].copy_(i.reshape(-1))
    if tail is None:
        return stage[:total], n
    stage[total:at] = 0
    stage[at:at + tail.size].copy_(torch.from_numpy(tail))
    return stage[:at + tail.size], n


def _u8_batch_to_device(what: str, images_u8, sizes, hp: int, wp: int, flips, s2d: bool, device, noise):
    """The checks and the staging that ``preprocess_u8_batch`` and ``noise_u8_batch`` share -> (the flat device buffer: tables,
    images [, noise tables], its int64 offsets, its int32 [N,5] dims, the device float64 sigmas and uint64 seeds or None)."""
    # device check FIRST: no CPU path exists, and nothing below may run without a HIP device to write to
    if not torch.cuda.is_available() or not all(isinstance(i, torch.Tensor) for i in images_u8):
        raise _native.SeamNativeError(f"{what}: expected uint8 tensors and a HIP device (no CPU path exists)")
    on_dev = [i.is_cuda for i in images_u8]
    n = len(images_u8)
    if not 1 <= n <= 65535:
        raise ValueError(f"{what}: 1 <= N <= 65535 images per launch, got {n}")
    if any(on_dev) and not all(on_dev):
        raise ValueError(f"{what}: the images must be all on the host or all on one HIP device")
    for i in images_u8:
        if i.dtype != torch.uint8:
            raise TypeError(f"image: expected torch.uint8, got {i.dtype}")
        if i.dim() != 3 or i.shape[2] != 3 or i.shape[0] < 1 or i.shape[1] < 1:
            raise ValueError("uint8 images must be [H,W,3]")
    if len(sizes) != n or len(flips) != n:
        raise ValueError(f"{what}: one size and one flip per image are needed")
    if s2d and (int(hp) % 2 or int(wp) % 2):
        raise ValueError(f"{what}(s2d=True): an even padded size is needed")
    sig = seed = None
    if all(on_dev):
        device = images_u8[0].device
        if any(i.device != device for i in images_u8):
            raise ValueError(f"{what}: the images must lie on one device")
        tables, _ = stage_u8_batch(images_u8, sizes, hp, wp, flips, None)
        dev = torch.cat([tables.to(device)] + [i.contiguous().reshape(-1) for i in images_u8])
        if noise is not None:
            tail = torch.from_numpy(_noise_tables(noise, n)).to(device)
            sig, seed = tail[:8 * n].view(torch.float64), tail[8 * n:]
    else:
        device = _mask_device(device if device is not None else "cuda")
        stage, _ = stage_u8_batch(images_u8, sizes, hp, wp, flips, device, noise)
        dev = stage.to(device, non_blocking=True)                            # the batch's one host-to-device copy
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        _STAGING[_staging_key(device)] = (_STAGING[_staging_key(device)][0], ev)
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


# ------------------------------------------------------------------------------ SEAM heads
@dataclass
class PackedNLB:
    w_proj_t: torch.Tensor   # [256,384]
    b_proj: torch.Tensor     # [384]
    w_cat: torch.Tensor      # [256]
    w_out_t: torch.Tensor    # [128,256]
    b_out: torch.Tensor      # [256]
    w_att: torch.Tensor      # [256]
    b_att: torch.Tensor      # [1]


NLB_MFMA = _os.environ.get("SEAM_NLB_MFMA", "1") != "0"      # 0: the VALU form of the block for every sequence length


def _nlb_mfma_pack(pk: PackedNLB):
    """Weights of ``seam_nlb_attnpool_mfma_f32`` derived (once per PackedNLB) from the plain pack:
    MFMA B-fragment order of the g and W projections -- element e of lane (h = lane >> 5, n = lane & 31) of fragment
    [n_tile][k / 8] is W[k = 8 j + 4 h + e][32 n_tile + n] -- and the folded theta / phi projections: theta and phi enter the
    block only through a_i = theta_i . wc[:128], b_j = phi_j . wc[128:] (ref models/nlb.py:80-90), i.e. a_i = X_i . u + c with
    u = W_theta^T wc[:128] (folded in fp64, rounded once)."""
    m = getattr(pk, "_mfma", None)
    if m is None:
        wp, bp, wc = pk.w_proj_t.double(), pk.b_proj.double(), pk.w_cat.double()       # [256,384], [384], [256]
        u = (wp[:, :128] @ wc[:128]).float().contiguous()
        v = (wp[:, 128:256] @ wc[128:]).float().contiguous()
        cd = torch.stack([bp[:128] @ wc[:128], bp[128:256] @ wc[128:]]).float().contiguous()
        wg = pk.w_proj_t[:, 256:]                                                        # [256 k, 128 n]
        wg_frag = wg.reshape(32, 2, 4, 4, 32).permute(3, 0, 1, 4, 2).contiguous()       # [nt, j, h, n, e]
        wo_frag = pk.w_out_t.reshape(16, 2, 4, 8, 32).permute(3, 0, 1, 4, 2).contiguous()   # [128 k, 256 n] -> [nt, j, h, n, e]
        m = pk._mfma = (wg_frag, pk.b_proj[256:].contiguous(), u, v, cd, wo_frag)
    return m


def nlb_attnpool(seq: torch.Tensor, t_stride: int, s_stride: int, lens: torch.Tensor, n_seq: int, t_max: int,
                 pk: PackedNLB, use_nlb: bool = True, want_att: bool = False, want_z: bool = False):
    """Batched non-local block + attention pooling.
    Returns (out[S,256], att[S,Tmax] | None) and additionally z[S,Tmax,256] when want_z.
    Sequences of up to ``seam_nlb_mfma_max_len()`` (96) rows run the block's GEMMs on the matrix cores
    (``seam_nlb_attnpool_mfma_f32``); longer ones take the VALU kernel with its global scratch."""
    lib = _native.lib()
    seq = _req(seq, name="seq")
    lens = _req(lens, torch.int32, "lens")
    out = torch.empty((n_seq, 256), dtype=F32, device=seq.device)
    att = torch.zeros((n_seq, t_max), dtype=F32, device=seq.device) if want_att else None
    z = torch.zeros((n_seq, t_max, 256), dtype=F32, device=seq.device) if want_z else None
    if n_seq == 0:
        return (out, att, z) if want_z else (out, att)
    if (NLB_MFMA and t_max <= int(lib.seam_nlb_mfma_max_len()) and t_stride % 4 == 0 and s_stride % 4 == 0
            and seq.data_ptr() % 16 == 0):
        wg_frag, b_g, u, v, cd, wo_frag = _nlb_mfma_pack(pk)
        _native.check(lib.seam_nlb_attnpool_mfma_f32(_ptr(seq), t_stride, s_stride, _ptr(lens), n_seq, t_max, _ptr(wg_frag), _ptr(b_g),
                                                     _ptr(u), _ptr(v), _ptr(cd), _ptr(wo_frag), _ptr(pk.b_out), _ptr(pk.w_att),
                                                     _ptr(pk.b_att), _ptr(out), _ptr(att), _ptr(z), int(use_nlb), _stream()),
                      "seam_nlb_attnpool_mfma_f32")
        return (out, att, z) if want_z else (out, att)
    ws = torch.empty((int(lib.seam_nlb_workspace_floats(n_seq, t_max)),), dtype=F32, device=seq.device)
    _native.check(lib.seam_nlb_attnpool_f32(_ptr(seq), t_stride, s_stride, _ptr(lens), n_seq, t_max, _ptr(pk.w_proj_t),
                                            _ptr(pk.b_proj), _ptr(pk.w_cat), _ptr(pk.w_out_t), _ptr(pk.b_out),
                                            _ptr(pk.w_att), _ptr(pk.b_att), _ptr(out), _ptr(att), _ptr(z), _ptr(ws),
                                            int(use_nlb), _stream()), "seam_nlb_attnpool_f32")
    return (out, att, z) if want_z else (out, att)


def pair_logits(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """a[Q,D], b[G,D], w[2,D], bias[2] -> [Q,G,2]."""
    a, b, w, bias = _req(a), _req(b), _req(w.detach()), _req(bias.detach())
    q, g, d = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty((q, g, 2), dtype=F32, device=a.device)
    _native.check(_native.lib().seam_pair_logits_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(bias), _ptr(out), q, g, d,
                                                     _stream()), "seam_pair_logits_f32")
    return out


def _topk_k(k: int, g: int, what: str) -> int:
    """min(k, G), refused above the selection's capacity (``seam_rank_topk_max_k()``: the kernels keep their winners on chip).
    Raised before anything is allocated or launched; there is no silent clamp -- a full ranking is what ``rank_of`` gives."""
    k = min(int(k), int(g))
    cap = int(_native.lib().seam_rank_topk_max_k())
    if k > cap:
        raise ValueError(f"{what}: k = {k} exceeds the top-k capacity of {cap} (seam_rank_topk_max_k()); "
                         "use rank_of for positions in the full ranking")
    return k


def rank_topk(logits: torch.Tensor, k: int):
    """logits[Q,G,2] -> (idx int64 [Q,k], score [Q,k]) by descending softmax(x)[...,1].
    min(k, G) <= seam_rank_topk_max_k() (256), else ValueError."""
    k = _topk_k(k, logits.shape[1], "rank_topk")
    logits = _req(logits)
    q, g = logits.shape[0], logits.shape[1]
    idx = torch.empty((q, k), dtype=torch.int64, device=logits.device)
    sc = torch.empty((q, k), dtype=F32, device=logits.device)
    _native.check(_native.lib().seam_rank_topk_f32(_ptr(logits), _ptr(idx), _ptr(sc), q, g, k, _stream()),
                  "seam_rank_topk_f32")
    return idx, sc


def match_scores(logits: torch.Tensor) -> torch.Tensor:
    """logits [...,2] -> softmax(logits)[...,1]."""
    logits = _req(logits)
    out = torch.empty(logits.shape[:-1], dtype=F32, device=logits.device)
    _native.check(_native.lib().seam_match_scores_f32(_ptr(logits), _ptr(out), out.numel(), _stream()),
                  "seam_match_scores_f32")
    return out


def pair_scores_blockdiag(x: torch.Tensor, seg, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """Self-similarity of every group of rows of ``x`` [rows, D] (groups = consecutive row ranges, boundaries ``seg`` [n_seg + 1]):
    the flat concatenation of the n_s x n_s score blocks, softmax(W (x_i - x_j)^2 + b)[1].  One launch for all groups
    (``seam_pair_scores_blockdiag_f32``); bit-identical to ``match_scores(pair_logits(x_s, x_s))`` per group
    (ref evaluate_movingfashion.py:102-121 ``compute_selfdist``)."""
    import numpy as np
    x = _req(x, name="x")
    seg = np.asarray(seg, dtype=np.int64)
    n = np.diff(seg)
    if len(n) == 0 or int(n.max()) == 0:
        return torch.empty((0,), dtype=F32, device=x.device)
    if seg[0] != 0 or int(seg[-1]) > x.shape[0] or (n < 0).any():
        raise ValueError("pair_scores_blockdiag: seg must be non-decreasing row offsets inside x, starting at 0")
    off = np.concatenate([[0], np.cumsum(n * n)])
    out = torch.empty((int(off[-1]),), dtype=F32, device=x.device)
    seg_d = torch.as_tensor(seg, dtype=torch.int32, device=x.device)
    off_d = torch.as_tensor(off, dtype=torch.int64, device=x.device)
    _native.check(_native.lib().seam_pair_scores_blockdiag_f32(_ptr(x), _ptr(seg_d), _ptr(off_d), _ptr(_req(w, name="w")), _ptr(_req(bias, name="bias")),
                                                               _ptr(out), len(n), int(n.max()), x.shape[1], _stream()),
                  "seam_pair_scores_blockdiag_f32")
    return out


def blockdiag_offsets(seg, device):
    """The two offset tables ``seam_pair_scores_blockdiag_f32`` and ``seam_build_tracklets_f32`` share, from host row offsets
    ``seg`` [n_seg + 1]: (seg int32 [n_seg + 1], out_off int64 [n_seg + 1] = running sum of n_s^2) on ``device``."""
    import numpy as np
    seg = np.asarray(seg, dtype=np.int64)
    n = np.diff(seg)
    off = np.concatenate([[0], np.cumsum(n * n)])
    return torch.as_tensor(seg, dtype=torch.int32, device=device), torch.as_tensor(off, dtype=torch.int64, device=device)


def pair_scores_blockdiag_device(x: torch.Tensor, seg: torch.Tensor, out_off: torch.Tensor, n_out: int, max_rows: int,
                                 w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``pair_scores_blockdiag`` with the offset tables already on the device (int32 ``seg``, int64 ``out_off``, as
    ``blockdiag_offsets`` forms them) and nothing read back: ``n_out`` floats are allocated (>= out_off[-1]; what lies behind
    out_off[-1] is not written) and ``max_rows`` bounds every group from above."""
    x = _req(x, name="x")
    seg, out_off = _req(seg, torch.int32, "seg"), _req(out_off, torch.int64, "out_off")
    out = torch.empty((int(n_out),), dtype=F32, device=x.device)
    if seg.numel() > 1 and max_rows > 0:
        _native.check(_native.lib().seam_pair_scores_blockdiag_f32(_ptr(x), _ptr(seg), _ptr(out_off), _ptr(_req(w, name="w")),
                                                                   _ptr(_req(bias, name="bias")), _ptr(out), seg.numel() - 1,
                                                                   int(max_rows), x.shape[1], _stream()),
                      "seam_pair_scores_blockdiag_f32")
    return out


def build_tracklets_max_rows() -> int:
    return int(_native.lib().seam_build_tracklets_max_rows())


def build_tracklets(blocks: torch.Tensor, out_off, seg, imgs: torch.Tensor, scores: torch.Tensor, threshold: float,
                    max_rows: Optional[int] = None):
    """Greedy tracklet linking of every segment in one launch (``seam_build_tracklets_f32``; the device twin of
    ``evaluator.build_tracklets_batch``): ``blocks`` as ``pair_scores_blockdiag`` returns them, ``imgs`` int32 [rows] frame labels
    (compared for equality only), ``scores`` fp32 [rows] confidences, all on the device.
    -> (members, track_len, n_tracks, track_of) int32 device tensors in the host helper's layout ([rows], [rows], [n_seg], [rows]).

    ``seg`` / ``out_off``: the host row offsets ``pair_scores_blockdiag`` took (``out_off`` may then be None: it is their running
    sum of squares), or the device tables of ``blockdiag_offsets``.  With device tables nothing here knows the segment sizes, so
    ``max_rows`` (an upper bound of every segment) must be passed; a longer segment then comes back with n_tracks[s] = -1.  With
    host offsets an oversized segment raises ValueError before anything is launched.  No host synchronisation either way."""
    import numpy as np
    cap = build_tracklets_max_rows()
    blocks, imgs, scores = _req(blocks, name="blocks"), _req(imgs, torch.int32, "imgs"), _req(scores, name="scores")
    dev = blocks.device
    if isinstance(seg, torch.Tensor) and seg.is_cuda:
        if max_rows is None or not isinstance(out_off, torch.Tensor):
            raise ValueError("build_tracklets: device offset tables need out_off on the device and max_rows (reading the segment "
                             "sizes back would be a host synchronisation)")
        seg_d, off_d = _req(seg, torch.int32, "seg"), _req(out_off, torch.int64, "out_off")
        max_rows = int(max_rows)
    else:
        seg_h = np.asarray(seg.numpy() if isinstance(seg, torch.Tensor) else seg, dtype=np.int64)
        n = np.diff(seg_h)
        if len(seg_h) < 1 or (len(n) and (seg_h[0] != 0 or (n < 0).any())):
            raise ValueError("build_tracklets: seg must be non-decreasing row offsets starting at 0")
        if len(n) and int(seg_h[-1]) != imgs.numel():
            raise ValueError(f"build_tracklets: seg ends at {int(seg_h[-1])} but imgs holds {imgs.numel()} detections")
        max_rows = int(n.max()) if len(n) else 0
        seg_d, off_d = blockdiag_offsets(seg_h, dev)
        if isinstance(out_off, torch.Tensor) and out_off.is_cuda:
            off_d = _req(out_off, torch.int64, "out_off")
        if len(n) and blocks.numel() != int((n * n).sum()):
            raise ValueError(f"build_tracklets: blocks holds {blocks.numel()} scores, the segments need {int((n * n).sum())}")
    if max_rows > cap:
        raise ValueError(f"build_tracklets: a segment of {max_rows} detections exceeds the linker's cap of {cap} "
                         "(seam_build_tracklets_max_rows())")
    rows, n_seg = imgs.numel(), seg_d.numel() - 1
    if scores.numel() != rows:
        raise ValueError("build_tracklets: scores must hold one confidence per detection")
    out = torch.empty((3 * rows + max(n_seg, 0),), dtype=torch.int32, device=dev)
    members, track_len, track_of, n_tracks = out[:rows], out[rows:2 * rows], out[2 * rows:3 * rows], out[3 * rows:]
    if n_seg > 0:
        _native.check(_native.lib().seam_build_tracklets_f32(_ptr(blocks), _ptr(off_d), _ptr(seg_d), _ptr(imgs), _ptr(scores), n_seg,
                                                             max_rows, float(threshold), _ptr(members), _ptr(track_len), _ptr(n_tracks),
                                                             _ptr(track_of), _stream()), "seam_build_tracklets_f32")
    return members, track_len, n_tracks, track_of


def rank_of(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """logits [Q,G,2], target int64 [Q] -> rank int64 [Q] of the target product in each query's ranking."""
    logits, target = _req(logits), _req(target, torch.int64, "target")
    q, g = logits.shape[0], logits.shape[1]
    out = torch.empty((q,), dtype=torch.int64, device=logits.device)
    _native.check(_native.lib().seam_rank_of_f32(_ptr(logits), _ptr(target), _ptr(out), q, g, _stream()), "seam_rank_of_f32")
    return out


def score_reduce(score: torch.Tensor, mode: str) -> torch.Tensor:
    """score [n,G] -> [G]: column mean (``"mean"``) or max (``"max"``)."""
    score = _req(score)
    n, g = score.shape
    out = torch.empty((g,), dtype=F32, device=score.device)
    _native.check(_native.lib().seam_score_reduce_f32(_ptr(score), _ptr(out), n, g, {"mean": 0, "max": 1}[mode], _stream()),
                  "seam_score_reduce_f32")
    return out


def score_reduce_segments(score: torch.Tensor, seg: torch.Tensor, mode: str) -> torch.Tensor:
    """score [N,G], seg [P+1] int32 row offsets (device) -> [P,G]: ``score_reduce`` of the rows seg[p]:seg[p+1] of every segment in
    ONE launch (the same sequential row order per column: bit-identical to P separate calls)."""
    score = _req(score)
    seg = _req(seg, torch.int32, "seg")
    n, g = score.shape
    p = seg.numel() - 1
    out = torch.empty((p, g), dtype=F32, device=score.device)
    _native.check(_native.lib().seam_score_reduce_seg_f32(_ptr(score), _ptr(seg), _ptr(out), p, g, {"mean": 0, "max": 1}[mode], _stream()),
                  "seam_score_reduce_seg_f32")
    return out


def rank_of_scores(score: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """score [Q,G], target int64 [Q] -> rank int64 [Q] of the target in each row's descending order."""
    score, target = _req(score), _req(target, torch.int64, "target")
    q, g = score.shape
    out = torch.empty((q,), dtype=torch.int64, device=score.device)
    _native.check(_native.lib().seam_rank_of_scores_f32(_ptr(score), _ptr(target), _ptr(out), q, g, _stream()),
                  "seam_rank_of_scores_f32")
    return out


def box_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """xyxy boxes a [Na,4], b [Nb,4] -> IoU [Na,Nb]."""
    a, b = _req(a), _req(b)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=F32, device=a.device)
    _native.check(_native.lib().seam_box_iou_f32(_ptr(a), _ptr(b), _ptr(out), a.shape[0], b.shape[0], _stream()),
                  "seam_box_iou_f32")
    return out


def gt_select(det_boxes: torch.Tensor, det_scores: torch.Tensor, det_off, gt_boxes: torch.Tensor, gt_off, gt_row: torch.Tensor,
              score_threshold: float):
    """Multi-DF2 ground-truth selection for N images in one launch (``seam_gt_select_f32``; ref evaluate_multiDF2.py:43-57,75-89):
    detections det_boxes [Dtot,4] / det_scores [Dtot] and GT boxes gt_boxes [Gtot,4] (xyxy, the images concatenated, device),
    their boundaries det_off / gt_off [N+1] (host sequences, checked here and uploaded with the launch) and gt_row int32 [N]
    (device; negative = from the end) -> (sel_idx, sel_pos, status) int32 [N] on the device.  Per image: the kept detection
    (score >= threshold, compared in fp32 as torch compares) with the largest pycocotools bbIou against its GT row, first maximum,
    as an index into the image's detections and as a position in the kept subsequence (-1 / -1 when nothing is kept); status
    1 = no GT box, 2 = row out of range (the GT is consulted only when something is kept)."""
    import numpy as np
    det_boxes, det_scores = _req(det_boxes, name="det_boxes"), _req(det_scores, name="det_scores")
    gt_boxes, gt_row = _req(gt_boxes, name="gt_boxes"), _req(gt_row, torch.int32, "gt_row")
    n = gt_row.numel()
    if det_boxes.dim() != 2 or det_boxes.shape[1] != 4 or gt_boxes.dim() != 2 or gt_boxes.shape[1] != 4:
        raise ValueError("gt_select: det_boxes and gt_boxes must be [*,4]")
    if det_scores.numel() != det_boxes.shape[0]:
        raise ValueError("gt_select: det_scores must hold one score per detection")
    det_boxes = det_boxes if det_boxes.data_ptr() % 16 == 0 else det_boxes.clone()      # the kernel reads boxes as float4
    gt_boxes = gt_boxes if gt_boxes.data_ptr() % 16 == 0 else gt_boxes.clone()
    offs = []
    for o, total, what in ((det_off, det_boxes.shape[0], "det_off"), (gt_off, gt_boxes.shape[0], "gt_off")):
        o = np.asarray(o, dtype=np.int64).reshape(-1)
        if o.size != n + 1 or o[0] != 0 or (np.diff(o) < 0).any() or int(o[-1]) > total or total >= 2 ** 31:
            raise ValueError(f"gt_select: {what} must be N+1 non-decreasing int32 offsets from 0 inside the table")
        offs.append(o)
    offs_d = torch.as_tensor(np.concatenate(offs).astype(np.int32)).to(det_boxes.device, non_blocking=False)
    outs = torch.empty((3, n), dtype=torch.int32, device=det_boxes.device)
    _native.check(_native.lib().seam_gt_select_f32(_ptr(det_boxes), _ptr(det_scores), _ptr(offs_d[:n + 1]), _ptr(gt_boxes),
                                                   _ptr(offs_d[n + 1:]), _ptr(gt_row), float(score_threshold), _ptr(outs[0]),
                                                   _ptr(outs[1]), _ptr(outs[2]), n, _stream()),
                  "seam_gt_select_f32")
    return outs[0], outs[1], outs[2]


PAIR_MFMA = True       # large banks: candidates on the fp32 matrix cores (seam_pair_topk_mfma_f32); False: the chunked VALU path


def pair_topk(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, k: int, fused: bool = False,
              q_chunk: int = 64, mfma: Optional[bool] = None, stats: Optional[torch.Tensor] = None, force_exact: bool = False):
    """a13+a14 without materialising the full [Q,G,2] logits -> (idx int64 [Q,k], score [Q,k]).  Three implementations with
    bit-identical results:

    * ``mfma`` (default when the bank has >= seam_pair_topk_mfma_min_gallery() rows, D == 256, k <= 64): seam_pair_topk_mfma_f32 --
      the logit-difference GEMM on the fp32 matrix cores finds candidates, the winners are re-scored with the direct form and a
      per-query error bound proves the top k (``stats``: optional int32[4] device tensor that receives [queries redone with the
      direct form, largest candidate list, overflowed lists, 0]; ``force_exact``: test hook, every query takes the direct form);
    * query chunks of ``q_chunk`` through seam_pair_logits_f32 + seam_rank_topk_f32 with one reused logits buffer (small banks);
    * ``fused=True``: seam_pair_topk_f32, the single-pass VALU kernel.

    Every branch: min(k, G) <= seam_rank_topk_max_k() (256), else ValueError before anything is allocated or launched."""
    lib = _native.lib()
    k = _topk_k(k, b.shape[0], "pair_topk")
    a, b, w, bias = _req(a), _req(b), _req(w.detach()), _req(bias.detach())
    q, g, d = a.shape[0], b.shape[0], a.shape[1]
    idx = torch.empty((q, k), dtype=torch.int64, device=a.device)
    sc = torch.empty((q, k), dtype=F32, device=a.device)
    can_mfma = d == 256 and g >= lib.seam_pair_topk_mfma_min_gallery() and 0 < k <= lib.seam_pair_topk_mfma_max_k() and q > 0
    if mfma is None:
        mfma = PAIR_MFMA and can_mfma and not fused
    if mfma:
        if not can_mfma:
            raise ValueError(f"pair_topk(mfma=True) needs D == 256, G >= {lib.seam_pair_topk_mfma_min_gallery()} and "
                             f"k <= {lib.seam_pair_topk_mfma_max_k()} (got D={d}, G={g}, k={k})")
        ws = torch.empty((int(lib.seam_pair_topk_mfma_workspace_floats(q, g, k)),), dtype=F32, device=a.device)
        if stats is not None:
            stats = _req(stats, torch.int32, "stats")
        _native.check(lib.seam_pair_topk_mfma_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(bias), _ptr(idx), _ptr(sc), q, g, d, k, _ptr(ws),
                                                  1 if force_exact else 0, _ptr(stats) if stats is not None else None, _stream()),
                      "seam_pair_topk_mfma_f32")
        return idx, sc
    if fused:
        ws = torch.empty((int(lib.seam_pair_topk_workspace_floats(q, g, k)),), dtype=F32, device=a.device)
        _native.check(lib.seam_pair_topk_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(bias), _ptr(idx), _ptr(sc), q, g, d, k,
                                             _ptr(ws), _stream()), "seam_pair_topk_f32")
        return idx, sc
    buf = torch.empty((min(q, q_chunk), g, 2), dtype=F32, device=a.device)
    for s0 in range(0, q, q_chunk):
        n = min(q_chunk, q - s0)
        _native.check(lib.seam_pair_logits_f32(C.c_void_p(a[s0:].data_ptr()), _ptr(b), _ptr(w), _ptr(bias), _ptr(buf), n, g, d,
                                               _stream()), "seam_pair_logits_f32")
        _native.check(lib.seam_rank_topk_f32(_ptr(buf), C.c_void_p(idx[s0:].data_ptr()), C.c_void_p(sc[s0:].data_ptr()), n, g,
                                             k, _stream()), "seam_rank_topk_f32")
    return idx, sc


# ------------------------------------------------------------------------------ detection
def decode_boxes(deltas: torch.Tensor, boxes: torch.Tensor, weights, clip_hw=None) -> torch.Tensor:
    """deltas [N,ncls*4], boxes [N,4] -> [N,ncls*4]; optional clip to (h,w)."""
    deltas, boxes = _req(deltas), _req(boxes)
    n = boxes.shape[0]
    ncls = deltas.shape[1] // 4
    out = torch.empty_like(deltas)
    ch, cw = (float(clip_hw[0]), float(clip_hw[1])) if clip_hw is not None else (0.0, 0.0)
    _native.check(_native.lib().seam_decode_boxes_f32(_ptr(deltas), _ptr(boxes), _ptr(out), n, ncls, *map(float, weights),
                                                      ch, cw, _stream()), "seam_decode_boxes_f32")
    return out


def nms_sorted(boxes: torch.Tensor, thr: float, max_keep: int = 0) -> torch.Tensor:
    """boxes [N,4] or [B,N,4], already sorted by descending score (per image) -> keep mask int32 [N] / [B,N].
    max_keep > 0: only the first ``max_keep`` survivors of each image are marked (== the full result truncated; the scan stops
    there)."""
    boxes = _req(boxes)
    single = boxes.dim() == 2
    b3 = boxes[None] if single else boxes
    bsz, n = b3.shape[0], b3.shape[1]
    keep = torch.empty((bsz, n), dtype=torch.int32, device=boxes.device)
    if n and bsz:
        nb = (n + 63) // 64
        ws = torch.empty((bsz * n * nb,), dtype=torch.int64, device=boxes.device)
        _native.check(_native.lib().seam_nms_sorted_topn_f32(_ptr(b3), _ptr(keep), bsz, n, float(thr), int(max_keep), _ptr(ws),
                                                             _stream()), "seam_nms_sorted_topn_f32")
    return keep[0] if single else keep


def rpn_topk_max() -> int:
    return int(_native.lib().seam_rpn_topk_max())


def rpn_topk_decode(head: torch.Tensor, num_anchors: int, anchors: torch.Tensor, clip_hw: torch.Tensor, k: int,
                    boxes: torch.Tensor, scores: torch.Tensor, offset: int, index: Optional[torch.Tensor] = None) -> None:
    """One pyramid level of RPN ``filter_proposals`` [TV] in one launch (``seam_rpn_topk_decode_f32``).

    head    [N,H,W,A+4A] fp32: the fused RPN head output (objectness logits | deltas per pixel), read in place
    anchors [H*W*A,4]; clip_hw [N,2] (height, width of each resized image), both fp32 on the device
    Writes, for every image, the top-``k`` anchors by logit (descending; ties lowest anchor index first) as decoded + clipped
    boxes into ``boxes[:, offset:offset+k]`` ([N,Ktot,4]) and sigmoid scores into ``scores[:, offset:offset+k]`` ([N,Ktot]);
    ``index`` (int64 [N,Ktot], optional) receives the anchor indices."""
    lib = _native.lib()
    head, anchors, clip_hw = _req(head, name="head"), _req(anchors, name="anchors"), _req(clip_hw, name="clip_hw")
    n_img, h, w, c = head.shape
    a = int(num_anchors)
    if c != 5 * a or anchors.shape != (h * w * a, 4) or clip_hw.shape != (n_img, 2):
        raise ValueError("rpn_topk_decode: head must be [N,H,W,5A], anchors [H*W*A,4], clip_hw [N,2]")
    if (boxes.dtype != F32 or scores.dtype != F32 or not boxes.is_cuda or not boxes.is_contiguous() or not scores.is_contiguous()
            or boxes.dim() != 3 or boxes.shape[0] != n_img or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2])
            or offset < 0 or offset + k > boxes.shape[1]):
        raise ValueError("rpn_topk_decode: boxes [N,Ktot,4] / scores [N,Ktot] fp32 contiguous with room for k rows at offset")
    if index is not None and (index.dtype != torch.int64 or tuple(index.shape) != tuple(scores.shape) or not index.is_contiguous()):
        raise ValueError("rpn_topk_decode: index must be int64 [N,Ktot] contiguous")
    if k < 1 or k > h * w * a or k > int(lib.seam_rpn_topk_max()):
        raise ValueError(f"rpn_topk_decode: k = {k} outside 1..min(n, {int(lib.seam_rpn_topk_max())})")
    obj = C.c_void_p(head.data_ptr())
    dlt = C.c_void_p(head.data_ptr() + 4 * a)
    _native.check(lib.seam_rpn_topk_decode_f32(obj, dlt, _ptr(anchors), _ptr(clip_hw), _ptr(boxes), _ptr(scores), _ptr(index),
                                               n_img, h * w * a, a, k, h * w * c, c, h * w * c, c, boxes.shape[1], offset,
                                               _stream()), "seam_rpn_topk_decode_f32")


def paste_masks(masks: torch.Tensor, boxes: torch.Tensor, hw) -> torch.Tensor:
    """masks [K,1,28,28] prob, boxes [K,4] original-image px -> [K,1,H,W]."""
    masks, boxes = _req(masks), _req(boxes)
    k = masks.shape[0]
    out = torch.empty((k, 1, int(hw[0]), int(hw[1])), dtype=F32, device=masks.device)
    if k:
        _native.check(_native.lib().seam_paste_masks_f32(_ptr(masks), _ptr(boxes), _ptr(out), k, int(hw[0]), int(hw[1]),
                                                         _stream()), "seam_paste_masks_f32")
    return out


def mask_inter(probs: torch.Tensor, boxes: torch.Tensor, gt_masks: torch.Tensor):
    """probs [D,1,28,28] or [D,28,28] (``mask_select``'s output), boxes [D,4] original-image px, gt_masks uint8 [G,H,W]
    (set iff != 0) -> (inter int32 [D,G], det_area int32 [D]): pixel counts of ``paste_masks(probs, boxes, (H, W)) > 0.5``
    against every ground truth and on its own, bit for bit, without the [D,1,H,W] paste (``seam_mask_inter_f32``)."""
    probs, boxes = _req(probs, name="probs"), _req(boxes, name="boxes")
    gt_masks = _req(gt_masks, torch.uint8, "gt_masks")
    d = probs.shape[0]
    if tuple(probs.shape[1:]) not in ((1, 28, 28), (28, 28)) or tuple(boxes.shape) != (d, 4):
        raise ValueError("mask_inter: probs must be [D,1,28,28] or [D,28,28] and boxes [D,4]")
    if gt_masks.dim() != 3:
        raise ValueError("mask_inter: gt_masks must be uint8 [G,H,W]")
    g, h, w = (int(s) for s in gt_masks.shape)
    if h * w >= 2 ** 31:
        raise ValueError("mask_inter: H*W must stay below 2^31")
    inter = torch.empty((d, g), dtype=torch.int32, device=probs.device)
    area = torch.empty((d,), dtype=torch.int32, device=probs.device)
    if d:
        _native.check(_native.lib().seam_mask_inter_f32(_ptr(probs), _ptr(boxes), d, _ptr(gt_masks) if g else None, g, h, w,
                                                        _ptr(inter) if g else None, _ptr(area), _stream()),
                      "seam_mask_inter_f32")
    return inter, area


def mask_select(logits: torch.Tensor, labels: torch.Tensor, ncls: int) -> torch.Tensor:
    """logits [K,14,14,4*ncls] (sub-pixel groups) -> sigmoid prob of channel labels[k]: [K,1,28,28]."""
    logits = _req_fp(logits)
    labels = _req(labels, torch.int64, "labels")
    k = logits.shape[0]
    out = torch.empty((k, 1, 28, 28), dtype=F32, device=logits.device)
    fn = getattr(_native.lib(), "seam_mask_select_" + _sfx(logits.dtype))
    _native.check(fn(_ptr(logits), _ptr(labels), _ptr(out), k, ncls, _stream()), "seam_mask_select")
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
    if all(on_dev):
        device = images[0].device
        if any(i.device != device for i in images):
            raise ValueError(f"{what}: the images must lie on one device")
        dev = torch.cat([torch.from_numpy(tables).to(device)] + [i.contiguous().reshape(-1) for i in images])
    else:
        device = _mask_device(device if device is not None else "cuda")
        stage = _staging(total, device)
        stage[:head].copy_(torch.from_numpy(tables))
        for i, o, b in zip(images, in_off.tolist(), in_bytes.tolist()):
            stage[o:o + b].copy_(i.reshape(-1))
        dev = stage[:total].to(device, non_blocking=True)                     # the batch's one host-to-device copy
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        _STAGING[_staging_key(device)] = (_STAGING[_staging_key(device)][0], ev)
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


# ------------------------------------------------------------------------------ RoI heads training branch (csrc/seam_roi_train.hip)
SAMPLE_MAX_CANDIDATES = 16384      # per image: rpn_post_nms_top_n_train (8000) + the GT boxes fit


def roi_sample(cand: torch.Tensor, n_cand: torch.Tensor, keys: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
               n_gt: torch.Tensor, batch: int = 512, pos_max: int = 128, weights=(10.0, 10.0, 5.0, 5.0)):
    """select_training_samples [TV] on padded per-image arrays: cand [N,P,4] (proposals then GT boxes), n_cand int32 [N],
    keys [N,P], gt_boxes [N,G,4], gt_labels int64 [N,G], n_gt int32 [N] -> (idx, labels, matched int64 [N,batch],
    boxes, targets [N,batch,4], count int32 [N,2] = (sampled rows, positives)); rows past the count hold -1 / 0."""
    cand, keys, gt_boxes = _req(cand, name="cand"), _req(keys, name="keys"), _req(gt_boxes, name="gt_boxes")
    n_cand, n_gt = _req(n_cand, torch.int32, "n_cand"), _req(n_gt, torch.int32, "n_gt")
    gt_labels = _req(gt_labels, torch.int64, "gt_labels")
    n, p = cand.shape[0], cand.shape[1]
    g = gt_boxes.shape[1]
    if p > SAMPLE_MAX_CANDIDATES:
        raise ValueError(f"roi_sample: {p} candidates per image exceed the kernel's capacity of {SAMPLE_MAX_CANDIDATES}")
    if tuple(keys.shape) != (n, p) or tuple(gt_labels.shape) != (n, g) or n_cand.numel() != n or n_gt.numel() != n:
        raise ValueError("roi_sample: inconsistent shapes")
    dev = cand.device
    idx = torch.empty((n, batch), dtype=torch.int64, device=dev)
    labels = torch.empty_like(idx)
    matched = torch.empty_like(idx)
    boxes = torch.empty((n, batch, 4), dtype=F32, device=dev)
    targets = torch.empty_like(boxes)
    count = torch.empty((n, 2), dtype=torch.int32, device=dev)
    wx, wy, ww, wh = (float(w) for w in weights)
    _native.check(_native.lib().seam_roi_sample_f32(_ptr(cand), _ptr(n_cand), _ptr(keys), _ptr(gt_boxes), _ptr(gt_labels), _ptr(n_gt),
                                                    n, p, g, int(batch), int(pos_max), wx, wy, ww, wh, _ptr(idx), _ptr(labels),
                                                    _ptr(matched), _ptr(boxes), _ptr(targets), _ptr(count), _stream()),
                  "seam_roi_sample_f32")
    return idx, labels, matched, boxes, targets, count


def fastrcnn_loss_fwd_bwd(class_logits: torch.Tensor, box_regression: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor):
    """fastrcnn_loss [TV] -> (loss [2] = (classifier, box_reg), dclass_logits, dbox_regression) for a unit upstream gradient."""
    class_logits, box_regression = _req(class_logits, name="class_logits"), _req(box_regression, name="box_regression")
    labels, targets = _req(labels, torch.int64, "labels"), _req(targets, name="targets")
    r, ncls = class_logits.shape
    if tuple(box_regression.shape) != (r, 4 * ncls) or labels.numel() != r or tuple(targets.shape) != (r, 4):
        raise ValueError("fastrcnn_loss_fwd_bwd: inconsistent shapes")
    loss = torch.empty((2,), dtype=F32, device=class_logits.device)
    dcls, dbox = torch.empty_like(class_logits), torch.empty_like(box_regression)
    _native.check(_native.lib().seam_fastrcnn_loss_fwd_bwd_f32(_ptr(class_logits), _ptr(box_regression), _ptr(labels), _ptr(targets),
                                                               r, ncls, _ptr(loss), _ptr(dcls), _ptr(dbox), _stream()),
                  "seam_fastrcnn_loss_fwd_bwd_f32")
    return loss, dcls, dbox


def mask_loss_fwd_bwd(logits: torch.Tensor, labels: torch.Tensor, rois: torch.Tensor, masks: torch.Tensor, mask_off: torch.Tensor,
                      mask_hw: torch.Tensor):
    """maskrcnn_loss [TV] on the sub-pixel logits [P,14,14,4*ncls]: labels int64 [P], rois [P,4] in the masks' frame, masks a flat
    uint8 buffer holding each ROI's GT mask at byte mask_off[k] (int64 [P]) with size mask_hw[k] (int32 [P,2])
    -> (loss [], dlogits like logits) for a unit upstream gradient."""
    logits, rois = _req(logits, name="logits"), _req(rois, name="rois")
    labels, masks = _req(labels, torch.int64, "labels"), _req(masks, torch.uint8, "masks")
    mask_off, mask_hw = _req(mask_off, torch.int64, "mask_off"), _req(mask_hw, torch.int32, "mask_hw")
    p = logits.shape[0]
    ncls = logits.shape[-1] // 4
    if tuple(logits.shape) != (p, 14, 14, 4 * ncls) or labels.numel() != p or tuple(rois.shape) != (p, 4) or mask_off.numel() != p \
            or tuple(mask_hw.shape) != (p, 2):
        raise ValueError("mask_loss_fwd_bwd: inconsistent shapes")
    loss = torch.empty((), dtype=F32, device=logits.device)
    dl = torch.empty_like(logits)
    ws = torch.empty((max(p, 1),), dtype=F32, device=logits.device)
    _native.check(_native.lib().seam_mask_loss_fwd_bwd_f32(_ptr(logits), _ptr(labels), _ptr(rois), _ptr(masks), _ptr(mask_off),
                                                           _ptr(mask_hw), p, ncls, _ptr(loss), _ptr(dl), _ptr(ws), _stream()),
                  "seam_mask_loss_fwd_bwd_f32")
    return loss, dl


# ------------------------------------------------------------------------------ RPN training branch (csrc/seam_rpn_train.hip)
RPN_MAX_ANCHORS = 1 << 20          # per image


def rpn_max_gt() -> int:
    return int(_native.lib().seam_rpn_max_gt())


def rpn_match(anchors: torch.Tensor, gt_boxes: torch.Tensor, n_gt: torch.Tensor, fg_thresh: float = 0.7, bg_thresh: float = 0.3):
    """Matcher(fg, bg, allow_low_quality_matches=True) [TV]: anchors [A,4] (shared by the batch), gt_boxes [N,G,4], n_gt int32 [N]
    -> (labels int8 [N,A]: -1 ignored / 0 background / 1 foreground, matched int32 [N,A]: the argmax GT of a foreground anchor)."""
    anchors, gt_boxes = _req(anchors, name="anchors"), _req(gt_boxes, name="gt_boxes")
    n_gt = _req(n_gt, torch.int32, "n_gt")
    if anchors.dim() != 2 or anchors.shape[1] != 4 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4 or n_gt.numel() != gt_boxes.shape[0]:
        raise ValueError("rpn_match: inconsistent shapes")
    a, (n, g) = anchors.shape[0], gt_boxes.shape[:2]
    lib = _native.lib()
    nws = int(lib.seam_rpn_match_workspace_floats(n, a, g))
    if nws <= 0:
        raise ValueError(f"rpn_match: N = {n}, A = {a}, G = {g} outside the kernel's caps (A <= {RPN_MAX_ANCHORS}, G <= {rpn_max_gt()})")
    dev = anchors.device
    labels = torch.empty((n, a), dtype=torch.int8, device=dev)
    matched = torch.empty((n, a), dtype=torch.int32, device=dev)
    ws = torch.empty((nws,), dtype=F32, device=dev)
    _native.check(lib.seam_rpn_match_f32(_ptr(anchors), _ptr(gt_boxes), _ptr(n_gt), n, a, g, float(fg_thresh), float(bg_thresh),
                                         _ptr(labels), _ptr(matched), _ptr(ws), _stream()), "seam_rpn_match_f32")
    return labels, matched


def rpn_sample(labels: torch.Tensor, matched: torch.Tensor, keys: torch.Tensor, anchors: torch.Tensor, gt_boxes: torch.Tensor,
               batch: int = 256, pos_max: int = 128):
    """BalancedPositiveNegativeSampler [TV] with the key rule of ``roi_sample`` on ``rpn_match``'s outputs: keys [N,A]
    -> (idx, labels, matched int64 [N,batch] in ascending anchor order, -1 past the count; targets [N,batch,4] =
    BoxCoder((1,1,1,1)).encode on the foreground rows; count int32 [N,2] = (rows, foreground rows))."""
    labels, matched = _req(labels, torch.int8, "labels"), _req(matched, torch.int32, "matched")
    keys, anchors, gt_boxes = _req(keys, name="keys"), _req(anchors, name="anchors"), _req(gt_boxes, name="gt_boxes")
    n, a = labels.shape
    g = gt_boxes.shape[1]
    if tuple(matched.shape) != (n, a) or tuple(keys.shape) != (n, a) or tuple(anchors.shape) != (a, 4) or gt_boxes.shape[0] != n:
        raise ValueError("rpn_sample: inconsistent shapes")
    lib = _native.lib()
    nws = int(lib.seam_rpn_sample_workspace_bytes(n, int(batch)))
    if nws <= 0 or a > RPN_MAX_ANCHORS:
        raise ValueError(f"rpn_sample: N = {n}, A = {a}, batch = {batch} outside the kernel's caps")
    dev = labels.device
    idx = torch.empty((n, batch), dtype=torch.int64, device=dev)
    slab, smat = torch.empty_like(idx), torch.empty_like(idx)
    targets = torch.empty((n, batch, 4), dtype=F32, device=dev)
    count = torch.empty((n, 2), dtype=torch.int32, device=dev)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    _native.check(lib.seam_rpn_sample_f32(_ptr(labels), _ptr(matched), _ptr(keys), _ptr(anchors), _ptr(gt_boxes), n, a, g, int(batch),
                                          int(pos_max), _ptr(idx), _ptr(slab), _ptr(smat), _ptr(targets), _ptr(count), _ptr(ws),
                                          _stream()), "seam_rpn_sample_f32")
    return idx, slab, smat, targets, count


def rpn_gather_patches(feats: Sequence[torch.Tensor], rows: torch.Tensor) -> torch.Tensor:
    """feats: the NHWC fp32 pyramid maps [N,H_l,W_l,C]; rows int32 [M,4] = (image, level, y, x) -> [M,3,3,C], the 3x3 window of
    each row's pixel with the conv's zero padding."""
    feats = [_req(f, name="feats") for f in feats]
    rows = _req(rows, torch.int32, "rows")
    n, c = feats[0].shape[0], feats[0].shape[3]
    if rows.dim() != 2 or rows.shape[1] != 4 or any(f.dim() != 4 or f.shape[0] != n or f.shape[3] != c for f in feats):
        raise ValueError("rpn_gather_patches: inconsistent shapes")
    m, l = rows.shape[0], len(feats)
    out = torch.empty((m, 3, 3, c), dtype=F32, device=rows.device)
    maps = (C.c_void_p * l)(*[f.data_ptr() for f in feats])
    hw = (C.c_int * (2 * l))(*[int(v) for f in feats for v in f.shape[1:3]])
    _native.check(_native.lib().seam_rpn_gather_patches_f32(maps, hw, _ptr(rows), m, n, l, c, _ptr(out), _stream()),
                  "seam_rpn_gather_patches_f32")
    return out


def rpn_loss_fwd_bwd(head: torch.Tensor, slot: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor, num_anchors: int,
                     grad_cols: int = 32):
    """RegionProposalNetwork.compute_loss [TV] on the sampled rows: head [M,>=5A], slot int32 [M], labels int64 [M], targets [M,4]
    -> (loss [2] = (objectness, rpn_box_reg), grad [M,grad_cols]) for a unit upstream gradient."""
    head, targets = _req(head, name="head"), _req(targets, name="targets")
    slot, labels = _req(slot, torch.int32, "slot"), _req(labels, torch.int64, "labels")
    m = head.shape[0]
    if head.dim() != 2 or slot.numel() != m or labels.numel() != m or tuple(targets.shape) != (m, 4):
        raise ValueError("rpn_loss_fwd_bwd: inconsistent shapes")
    loss = torch.empty((2,), dtype=F32, device=head.device)
    grad = torch.empty((m, int(grad_cols)), dtype=F32, device=head.device)
    _native.check(_native.lib().seam_rpn_loss_fwd_bwd_f32(_ptr(head), _ptr(slot), _ptr(labels), _ptr(targets), m, int(num_anchors),
                                                          head.shape[1], int(grad_cols), _ptr(loss), _ptr(grad), _stream()),
                  "seam_rpn_loss_fwd_bwd_f32")
    return loss, grad


# ------------------------------------------------------------------------------ FPN training: the adjoints (csrc/seam_fpn_train.hip)
def roi_align_bwd(dout: torch.Tensor, rois: torch.Tensor, feat_hws: Sequence[Sequence[int]], n_images: int, scales: Sequence[float],
                  sampling_ratio: int = 2, k_min: int = 2, levels: Optional[torch.Tensor] = None) -> list:
    """Adjoint of ``roi_align``: dout NHWC fp32 [K,P,P,C], rois fp32 [K,5], feat_hws the four (H_l, W_l) -> the four gradient
    maps [N,H_l,W_l,C], written completely (zeros where no ROI reaches).  Fixed summation order: two calls give the same bits."""
    dout, rois = _req(dout, name="dout"), _req(rois, name="rois")
    if dout.dim() != 4 or dout.shape[1] != dout.shape[2] or rois.dim() != 2 or rois.shape[1] != 5 or rois.shape[0] != dout.shape[0]:
        raise ValueError("roi_align_bwd: dout must be [K,P,P,C] and rois [K,5]")
    if len(feat_hws) != 4 or len(scales) != 4:
        raise ValueError("roi_align_bwd: four levels are needed")
    k, p, c = dout.shape[0], dout.shape[1], dout.shape[3]
    n = int(n_images)
    if levels is not None:
        levels = _req(levels, torch.int32, "levels")
        if levels.numel() != k:
            raise ValueError("roi_align_bwd: one level per ROI is needed")
    lib = _native.lib()
    hws = [(int(h), int(w)) for h, w in feat_hws]
    nws = int(lib.seam_roi_align_bwd_workspace_bytes(n, k))
    if nws <= 0:
        raise ValueError(f"roi_align_bwd: {n} images / {k} ROIs are outside the kernel's caps")
    outs = [torch.empty((n, h, w, c), dtype=F32, device=dout.device) for h, w in hws]
    ws = torch.empty((nws,), dtype=torch.uint8, device=dout.device)
    hw = (C.c_int * 8)(*[d for s in hws for d in s])
    _native.check(lib.seam_roi_align_bwd_f32(_ptr(dout) if k else None, _ptr(rois) if k else None, _ptr(levels), hw, c,
                                             scales[0], scales[1], scales[2], scales[3], k_min, n, k, p, int(sampling_ratio),
                                             _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(ws), _stream()),
                  "seam_roi_align_bwd_f32")
    return outs


def rpn_scatter_patches(dpatch: torch.Tensor, rows: torch.Tensor, feat_hws: Sequence[Sequence[int]], n_images: int) -> list:
    """Adjoint of ``rpn_gather_patches``: dpatch fp32 [M,3,3,C], rows int32 [M,4] = (image, level, y, x), feat_hws the (H_l, W_l)
    of the levels -> the gradient maps [N,H_l,W_l,C] (zeros where no window reaches).  Rows are added in row order."""
    dpatch = _req(dpatch, name="dpatch")
    rows = _req(rows, torch.int32, "rows")
    if dpatch.dim() != 4 or tuple(dpatch.shape[1:3]) != (3, 3) or rows.dim() != 2 or rows.shape[1] != 4 or rows.shape[0] != dpatch.shape[0]:
        raise ValueError("rpn_scatter_patches: inconsistent shapes")
    m, c, n, l = dpatch.shape[0], dpatch.shape[3], int(n_images), len(feat_hws)
    hws = [(int(h), int(w)) for h, w in feat_hws]
    if m == 0:
        return [torch.zeros((n, h, w, c), dtype=F32, device=dpatch.device) for h, w in hws]
    outs = [torch.empty((n, h, w, c), dtype=F32, device=dpatch.device) for h, w in hws]
    maps = (C.c_void_p * l)(*[o.data_ptr() for o in outs])
    hw = (C.c_int * (2 * l))(*[d for s in hws for d in s])
    _native.check(_native.lib().seam_rpn_scatter_patches_f32(_ptr(dpatch), _ptr(rows), m, n, l, c, maps, hw, _stream()),
                  "seam_rpn_scatter_patches_f32")
    return outs


def upsample_add_bwd(dlat: torch.Tensor, top_hw: Sequence[int], base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adjoint of the nearest top-down merge (``upsample_add_`` / ``conv2d_topdown``): dlat [N,H,W,C] -> [N,Ht,Wt,C], each
    coarse pixel the sum of the fine pixels the forward mapped to it, plus ``base`` [N,Ht,Wt,C] when given."""
    dlat = _req(dlat, name="dlat")
    n, h, w, c = dlat.shape
    ht, wt = int(top_hw[0]), int(top_hw[1])
    if base is not None:
        base = _req(base, name="base")
        if tuple(base.shape) != (n, ht, wt, c):
            raise ValueError("upsample_add_bwd: base must be [N,Ht,Wt,C]")
    out = torch.empty((n, ht, wt, c), dtype=F32, device=dlat.device)
    _native.check(_native.lib().seam_upsample_add_bwd_f32(_ptr(dlat), _ptr(base), _ptr(out), n, h, w, ht, wt, c, _stream()),
                  "seam_upsample_add_bwd_f32")
    return out


def subsample_add_bwd_(d: torch.Tensor, dpool: torch.Tensor) -> torch.Tensor:
    """Adjoint of LastLevelMaxPool (k=1, s=2), in place: d[n,2i,2j,:] += dpool[n,i,j,:]; returns d."""
    if not d.is_contiguous():
        raise ValueError("subsample_add_bwd_: d is updated in place and must be contiguous")
    d, dpool = _req(d, name="d"), _req(dpool, name="dpool")
    n, h, w, c = d.shape
    if tuple(dpool.shape) != (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c):
        raise ValueError("subsample_add_bwd_: dpool must be [N,(H-1)//2+1,(W-1)//2+1,C]")
    _native.check(_native.lib().seam_subsample_add_bwd_f32(_ptr(d), _ptr(dpool), n, h, w, dpool.shape[1], dpool.shape[2], c, _stream()),
                  "seam_subsample_add_bwd_f32")
    return d


subsample_add_bwd = subsample_add_bwd_


# ---------------------------------------------------------------------------------------------------- ResNet body training
def relu_mask_add(y: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = y > 0 ? a + b : 0 over [..., C] (``seam_relu_mask_add_f32``): the ReLU at a bottleneck's output, whose gradient
    feeds both the residual branch and the shortcut; ``b`` (or None) is a second gradient arriving at the same map."""
    y, a = _req(y, name="y"), _req(a, name="a")
    if a.shape != y.shape or (b is not None and b.shape != y.shape):
        raise ValueError("relu_mask_add: y, a and b need one shape")
    if b is not None:
        b = _req(b, name="b")
    c = y.shape[-1]
    out = torch.empty_like(y)
    _native.check(_native.lib().seam_relu_mask_add_f32(_ptr(y), _ptr(a), _ptr(b), _ptr(out), y.numel() // c, c, _stream()),
                  "seam_relu_mask_add_f32")
    return out


def maxpool3s2_relu_bwd(y: torch.Tensor, dpool: torch.Tensor) -> torch.Tensor:
    """Adjoint of ``maxpool2d(y, 3, 2, 1)`` behind the ReLU that made ``y`` (``seam_maxpool3s2_relu_bwd_f32``): y NHWC
    [N,H,W,C], the pool's input; dpool NHWC [N,(H-1)//2+1,(W-1)//2+1,C] -> dy [N,H,W,C], each pixel the sum of the dpool of the
    windows whose argmax it is (torch's: the first maximum in row-major order), zero where y <= 0.  A batch whose y passes
    ``WGRAD_MAX_OPERAND_BYTES`` is split over images, as ``conv_wgrad_chunked`` splits: images are independent, no bit changes."""
    y, dpool = _req(y, name="y"), _req(dpool, name="dpool")
    if y.dim() != 4 or y.shape[0] == 0 or y.shape[-1] % 4:
        raise ValueError(f"maxpool3s2_relu_bwd: y must be a non-empty NHWC tensor with C % 4 == 0, got {tuple(y.shape)}")
    n, h, w, c = y.shape
    if tuple(dpool.shape) != (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c):
        raise ValueError(f"maxpool3s2_relu_bwd: dpool {tuple(dpool.shape)} must be [N,(H-1)//2+1,(W-1)//2+1,C] of y {tuple(y.shape)}")
    per = h * w * c * 4
    if per > WGRAD_MAX_OPERAND_BYTES:
        raise ValueError(f"maxpool3s2_relu_bwd: one image's y ({per} bytes) exceeds the limit of {WGRAD_MAX_OPERAND_BYTES}")
    step = max(1, min(n, WGRAD_MAX_OPERAND_BYTES // per))
    dy = torch.empty_like(y)
    lib = _native.lib()
    for i in range(0, n, step):
        m = min(step, n - i)
        _native.check(lib.seam_maxpool3s2_relu_bwd_f32(_ptr(y[i:i + m]), _ptr(dpool[i:i + m]), _ptr(dy[i:i + m]), m, h, w, c, _stream()),
                      "seam_maxpool3s2_relu_bwd_f32")
    return dy


@dataclass
class PackedS2Dgrad:
    """Weights of ``conv3x3s2_dgrad``: both forms are packed from the same scaled weight, so either selector value can run."""
    K: int
    C: int
    w: torch.Tensor                       # OIHW, scale folded (the composition packs its rotated form from it on first use)
    wp: torch.Tensor                      # [9][C][K] rows of seam_conv3x3s2_dgrad_f32
    pc: Optional[PackedConv] = None       # stride-1 dgrad weights of the composition (SEAM_S2_DGRAD=0)


def pack_conv3x3s2_dgrad(weight: torch.Tensor, scale: Optional[torch.Tensor] = None) -> PackedS2Dgrad:
    """OIHW weight [K,C,3,3] of a 3x3 / stride-2 / pad-1 conv, and the [K] scale of its FrozenBN epilogue (or None), for
    ``conv3x3s2_dgrad``: ``dy * scale`` is never materialised, the scale rides in the packed weights."""
    weight = _req(weight.detach(), name="weight")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("pack_conv3x3s2_dgrad: weight must be [K,C,3,3]")
    k, c = int(weight.shape[0]), int(weight.shape[1])
    if scale is not None:
        scale = _req(scale.detach(), name="scale")
        if tuple(scale.shape) != (k,):
            raise ValueError("pack_conv3x3s2_dgrad: scale must be [K]")
    wp = torch.empty((9, c, k), dtype=F32, device=weight.device)
    _native.check(_native.lib().seam_pack_conv3x3s2_dgrad_f32(_ptr(weight), _ptr(scale), _ptr(wp), k, c, _stream()),
                  "seam_pack_conv3x3s2_dgrad_f32")
    ws = weight if scale is None else (weight * scale[:, None, None, None]).contiguous()
    return PackedS2Dgrad(k, c, ws, wp)


def _conv3x3s2_dgrad_one(dy, pk, hw, mask, out=None):
    n, ho, wo, k = dy.shape
    h, w = hw
    if _native.get_option("SEAM_S2_DGRAD") != 0:
        dx = out if out is not None else torch.empty((n, h, w, pk.C), dtype=F32, device=dy.device)
        _native.check(_native.lib().seam_conv3x3s2_dgrad_f32(_ptr(dy), _ptr(pk.wp), _ptr(mask), _ptr(dx), n, h, w, pk.C, k, _stream()),
                      "seam_conv3x3s2_dgrad_f32")
        return dx
    # the composition: dy zero-stuffed onto the even pixels of an [H, W] grid (2Ho-1 stuffed rows + the H - (2Ho-1) zero rows the
    # forward's last tap never reached), then the stride-1 dgrad with one pixel of padding
    if pk.pc is None:
        pk.pc = pack_conv_dgrad(pk.w, pad_fwd=1)
    z = torch.zeros((n, h, w, k), dtype=F32, device=dy.device)
    z[:, 0:2 * ho - 1:2, 0:2 * wo - 1:2] = dy
    return conv2d(z, pk.pc, relu=2 if mask is not None else False, residual=mask, out=out)


def conv3x3s2_dgrad(dy: torch.Tensor, pk: PackedS2Dgrad, hw: Sequence[int], mask: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Input gradient of a 3x3 / stride-2 / pad-1 conv: dy NHWC [N,Ho,Wo,K] -> dx NHWC [N,H,W,C] for the forward input size
    ``hw`` (Ho = (H-1)//2+1), zeroed where ``mask`` [N,H,W,C] <= 0 (the ReLU of the producer, ``relu=2`` of ``conv2d``).
    SEAM_S2_DGRAD selects the gather kernel (``seam_conv3x3s2_dgrad_f32``) or the zero-stuffed composition.  A batch whose dy or
    dx reaches ``WGRAD_MAX_OPERAND_BYTES`` is split over images, as ``conv_wgrad_chunked`` does.  ``out``: a contiguous fp32
    [N,H,W,C] tensor to write into (every element is written exactly once)."""
    dy = _req(dy, name="dy")
    n, ho, wo, k = dy.shape
    h, w = int(hw[0]), int(hw[1])
    if n == 0 or k != pk.K or ho != (h - 1) // 2 + 1 or wo != (w - 1) // 2 + 1:
        raise ValueError(f"conv3x3s2_dgrad: dy {tuple(dy.shape)} does not belong to an input of {h} x {w} and {pk.K} output channels")
    if mask is not None:
        mask = _req(mask, name="mask")
        if tuple(mask.shape) != (n, h, w, pk.C):
            raise ValueError("conv3x3s2_dgrad: mask must be [N,H,W,C]")
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != dy.device or out.dtype != F32
                            or tuple(out.shape) != (n, h, w, pk.C) or not out.is_contiguous()):
        raise ValueError(f"conv3x3s2_dgrad: out must be a contiguous float32 tensor of shape {(n, h, w, pk.C)} on {dy.device}")
    per = max(h * w * pk.C, ho * wo * k) * 4
    if per > WGRAD_MAX_OPERAND_BYTES:
        raise ValueError(f"conv3x3s2_dgrad: one image's operand ({per} bytes) exceeds the limit of {WGRAD_MAX_OPERAND_BYTES}")
    step = max(1, min(n, WGRAD_MAX_OPERAND_BYTES // per))
    if step >= n:
        return _conv3x3s2_dgrad_one(dy, pk, (h, w), mask, out)
    if out is None:
        out = torch.empty((n, h, w, pk.C), dtype=F32, device=dy.device)
    for i in range(0, n, step):
        _conv3x3s2_dgrad_one(dy[i:i + step], pk, (h, w), None if mask is None else mask[i:i + step], out[i:i + step])
    return out


# ---------------------------------------------------------------------------------------------------- ground-truth masks (csrc/seam_masks.hip)
MASK_MAX_SIDE = 16384              # h, w of an image whose annotations are rasterised
MASK_MAX_POINTS = 2 ** 31          # boundary points of one poly_masks call (32-bit thread index), exclusive


@dataclass
class MaskLayout:
    """Where every object's [h,w] bytes lie in the flat uint8 buffer of a batch: image after image, an image's objects adjacent,
    so that image i's stack is the view ``flat[img_off[i]:img_off[i+1]].view(n_i, H_i, W_i)``."""
    counts: list                   # objects per image
    sizes: list                    # (h, w) per image
    obj_hw: object                 # int32 [n,2]
    obj_off: object                # int64 [n] byte offsets
    img_off: list                  # len(images) + 1 byte offsets

    @property
    def total(self) -> int:
        return self.img_off[-1]


def mask_layout(counts: Sequence[int], sizes: Sequence[Sequence[int]]) -> MaskLayout:
    import numpy as np
    if len(counts) != len(sizes):
        raise ValueError(f"masks: {len(counts)} images but {len(sizes)} sizes")
    hw, off, img_off, pos = [], [], [0], 0
    for i, (n, size) in enumerate(zip(counts, sizes)):
        h, w = (int(size[0]), int(size[1])) if len(size) == 2 else (0, 0)
        if len(size) != 2 or h != size[0] or w != size[1] or not (1 <= h <= MASK_MAX_SIDE and 1 <= w <= MASK_MAX_SIDE):
            raise ValueError(f"masks: image {i}: size {tuple(size)} must be (h, w) with 1 <= h, w <= {MASK_MAX_SIDE}")
        for _ in range(n):
            hw.append((h, w))
            off.append(pos)
            pos += h * w
        img_off.append(pos)
    return MaskLayout(list(counts), [(int(s[0]), int(s[1])) for s in sizes], np.asarray(hw, np.int32).reshape(-1, 2),
                      np.asarray(off, np.int64), img_off)


def mask_views(flat: torch.Tensor, lay: MaskLayout) -> list:
    return [flat[lay.img_off[i]:lay.img_off[i + 1]].view(n, h, w) for i, (n, (h, w)) in enumerate(zip(lay.counts, lay.sizes))]


def _selected(objs_per_image):
    """(image, object, flat object index, entry) of every entry that is not None."""
    out, k = [], 0
    for i, objs in enumerate(objs_per_image):
        for j, o in enumerate(objs):
            if o is not None:
                out.append((i, j, k, o))
            k += 1
    return out


def pack_poly_masks(polys: Sequence[Sequence], sizes: Sequence[Sequence[int]]):
    """Host packing of ``seam_poly_masks_u8``: ``polys[i][j]`` is object j of image i as a list of parts, each a flat
    ``[x0, y0, x1, y1, ...]`` sequence (an empty list: an object of zero parts, all zeros; None: not a polygon object, skipped).
    Returns (layout, tables): the int32 / int64 NumPy tables of include/seam_hip.h, the vertices upsampled in float64 as
    ``trunc(5*x + 0.5)``.  Raises ValueError, naming the object, for an odd-length or empty part, a coordinate that is not
    finite or with ``|5x + 0.5| >= 2^31``, and for ``MASK_MAX_POINTS`` boundary points or more."""
    import numpy as np
    lay = mask_layout([len(o) for o in polys], sizes)
    flat_xy, names, part_len, part_obj, part_words, sel_obj = [], [], [], [], [], []
    words_of = {}
    for i, j, k, parts in _selected(polys):
        h, w = lay.sizes[i]
        if (h, w) not in words_of:
            words_of[(h, w)] = int(_native.lib().seam_poly_masks_ws_bytes(h, w)) // 4
        for q, part in enumerate(parts):
            what = f"poly_masks: image {i} object {j} part {q}"
            try:
                xy = np.asarray(part, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{what}: not a sequence of numbers") from e
            if xy.ndim != 1 or xy.size == 0 or xy.size % 2:
                raise ValueError(f"{what}: expected a flat, non-empty [x0, y0, x1, y1, ...] of even length, got shape {xy.shape}")
            flat_xy.append(xy)
            names.append(what)
            part_len.append(xy.size // 2)
            part_obj.append(len(sel_obj))
            part_words.append(words_of[(h, w)])
        sel_obj.append(k)
    P = len(part_len)
    part_len = np.asarray(part_len, np.int64)
    part_off = np.zeros(P + 1, np.int64)
    np.cumsum(part_len, out=part_off[1:])
    V = int(part_off[-1])
    up = 5.0 * (np.concatenate(flat_xy) if P else np.zeros(0))
    up = up + 0.5                                               # the multiply and the add stay apart, as (int)(5*x + 0.5) has them
    bad = ~(np.abs(up) < 2.0 ** 31)                             # also true for NaN
    if bad.any():
        at = int(np.flatnonzero(bad)[0])
        who = names[int(np.searchsorted(part_off, at // 2, side="right")) - 1]
        raise ValueError(f"{who}: a coordinate is not finite" if not np.isfinite(up[at]) else f"{who}: |5x + 0.5| must stay below 2^31")
    allp = np.trunc(up).astype(np.int64).reshape(-1, 2)
    nxt = np.arange(V, dtype=np.int64) + 1                      # ring successor of every vertex
    nxt[part_off[1:] - 1] = part_off[:-1]
    step = np.abs(allp[nxt] - allp)
    edge_pts = np.maximum(step[:, 0], step[:, 1]) + 1
    edge_pt_off = np.zeros(V + 1, np.int64)
    np.cumsum(edge_pts, out=edge_pt_off[1:])
    T = int(edge_pt_off[-1])
    if T >= MASK_MAX_POINTS:
        raise ValueError(f"poly_masks: {T} boundary points in one call, the limit is {MASK_MAX_POINTS} (split the batch)")
    part_ws_off = np.zeros(P + 1, np.int64)
    np.cumsum(part_words, out=part_ws_off[1:])
    sel = np.asarray(sel_obj, np.int64)
    tables = dict(pts=allp.astype(np.int32), part_off=part_off.astype(np.int32), part_obj=np.asarray(part_obj, np.int32),
                  edge_pt_off=edge_pt_off.astype(np.int32), part_ws_off=part_ws_off, obj_hw=np.ascontiguousarray(lay.obj_hw[sel]),
                  obj_out_off=np.ascontiguousarray(lay.obj_off[sel]), P=P, V=V, T=T, n=len(sel_obj), sel=sel)
    return lay, tables


def pack_rle_masks(rles: Sequence[Sequence], sizes: Sequence[Sequence[int]]):
    """Host packing of ``seam_rle_masks_u8``: ``rles[i][j]`` is object j of image i as its uncompressed counts (runs of 0 and 1
    alternating in column-major order, the first a run of zeros; None: not an RLE object, skipped).  Raises ValueError, naming
    the object, for counts that are negative, not integers, or do not sum to h*w."""
    import numpy as np
    lay = mask_layout([len(o) for o in rles], sizes)
    starts, run_off, sel_obj = [], [0], []
    for i, j, k, counts in _selected(rles):
        what = f"image {i} object {j}"
        h, w = lay.sizes[i]
        try:
            raw = np.asarray(counts)
            c = raw.astype(np.int64)
        except (TypeError, ValueError, OverflowError) as e:
            raise ValueError(f"rle_masks: {what}: counts are not a sequence of integers") from e
        if c.ndim != 1 or c.size == 0 or not (raw == c).all():
            raise ValueError(f"rle_masks: {what}: counts must be a flat, non-empty sequence of integers")
        if (c < 0).any() or int(c.sum()) != h * w:
            raise ValueError(f"rle_masks: {what}: counts must be non-negative and sum to h*w = {h * w}, got sum {int(c.sum())}")
        starts.append(np.cumsum(c) - c)
        run_off.append(run_off[-1] + c.size)
        sel_obj.append(k)
    if run_off[-1] >= 2 ** 31:
        raise ValueError("rle_masks: 2^31 runs or more in one call (split the batch)")
    sel = np.asarray(sel_obj, np.int64)
    tables = dict(run_start=(np.concatenate(starts) if starts else np.zeros(0, np.int64)).astype(np.int32),
                  obj_run_off=np.asarray(run_off, np.int32), obj_hw=np.ascontiguousarray(lay.obj_hw[sel]),
                  obj_out_off=np.ascontiguousarray(lay.obj_off[sel]), n=len(sel_obj), sel=sel)
    return lay, tables


def _mask_device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _native.SeamNativeError("masks are rasterised on the HIP device (no CPU path exists)")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _upload_tables(tables: dict, names, device) -> dict:
    """One host-to-device copy for all tables of a call: the int64 ones first (8-byte alignment), everything as int32 words."""
    import numpy as np
    names = sorted(names, key=lambda k: -tables[k].dtype.itemsize)
    words = [np.ascontiguousarray(tables[k]).reshape(-1).view(np.int32) for k in names]
    dev = torch.from_numpy(np.concatenate(words)).to(device)
    out, pos = {}, 0
    for k, wd in zip(names, words):
        t = dev[pos:pos + wd.size]
        out[k] = t.view(torch.int64) if tables[k].dtype.itemsize == 8 else t
        pos += wd.size
    return out


def mask_flat(lay: MaskLayout, device, flat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The flat uint8 buffer of a batch's masks on ``device``: allocated (uninitialised), or ``flat`` checked against the layout."""
    device = _mask_device(device)
    if flat is None:
        return torch.empty((lay.total,), dtype=torch.uint8, device=device)
    flat = _req(flat, torch.uint8, "flat")
    if flat.dim() != 1 or flat.numel() != lay.total or flat.device != device:
        raise ValueError(f"masks: flat must be a uint8 [{lay.total}] tensor on {device}")
    return flat


def launch_poly_masks(lay: MaskLayout, t: dict, device, flat: Optional[torch.Tensor] = None) -> list:
    """``seam_poly_masks_u8`` over the tables of ``pack_poly_masks``: one upload, one launch sequence.  ``flat``: the batch's
    flat buffer when another producer fills the objects that were None in the packing; allocated here otherwise."""
    device = _mask_device(device)
    flat = mask_flat(lay, device, flat)
    if t["n"]:
        names = ("pts", "part_off", "part_obj", "edge_pt_off", "part_ws_off", "obj_hw", "obj_out_off")
        d = _upload_tables(t, names, device)
        ws_bytes = 4 * int(t["part_ws_off"][-1])
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        p = [_ptr(d[k]) if d[k].numel() else None for k in names]
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_poly_masks_u8(*p, _ptr(flat), _ptr(ws) if ws_bytes else None, ws_bytes, t["P"], t["V"],
                                                           t["T"], t["n"], _stream()), "seam_poly_masks_u8")
    return mask_views(flat, lay)


def launch_rle_masks(lay: MaskLayout, t: dict, device, flat: Optional[torch.Tensor] = None) -> list:
    """``seam_rle_masks_u8`` over the tables of ``pack_rle_masks`` (``flat`` as in ``launch_poly_masks``)."""
    device = _mask_device(device)
    flat = mask_flat(lay, device, flat)
    if t["n"]:
        names = ("run_start", "obj_run_off", "obj_hw", "obj_out_off")
        d = _upload_tables(t, names, device)
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_rle_masks_u8(*[_ptr(d[k]) for k in names], _ptr(flat), t["n"], _stream()),
                          "seam_rle_masks_u8")
    return mask_views(flat, lay)


def resized_mask_layout(lay: MaskLayout, out_sizes: Sequence[Sequence[int]], flips: Optional[Sequence] = None):
    """The output side of the resized expands (csrc/seam_input.hip) for a batch laid out as ``lay``: image i's objects are written
    at ``out_sizes[i]``, flipped where ``flips[i]``.  Returns (layout of the resized stacks, obj_out int32 [n,3] = (out_h, out_w,
    flip) per object of the batch)."""
    import numpy as np
    out_lay = mask_layout(lay.counts, out_sizes)
    flips = [False] * len(lay.counts) if flips is None else [bool(f) for f in flips]
    if len(flips) != len(lay.counts):
        raise ValueError(f"masks: {len(lay.counts)} images but {len(flips)} flips")
    flip = np.repeat(np.asarray(flips, np.int32), np.asarray(lay.counts, np.int64)).reshape(-1, 1)
    return out_lay, np.concatenate([out_lay.obj_hw, flip], axis=1).astype(np.int32)


def _resized_tables(t: dict, out_lay: MaskLayout, obj_out) -> dict:
    import numpy as np
    return dict(t, obj_out=np.ascontiguousarray(obj_out[t["sel"]]), obj_out_off=np.ascontiguousarray(out_lay.obj_off[t["sel"]]))


def launch_poly_masks_resized(lay: MaskLayout, t: dict, out_sizes, flips, device, flat: Optional[torch.Tensor] = None) -> list:
    """``launch_poly_masks`` with the expand of ``seam_poly_masks_resized_u8``: image i's stack comes out as uint8
    ``[n_i, *out_sizes[i]]`` = ``resize_masks_nearest(stack.flip(-1) if flips[i] else stack, out_sizes[i])`` bit for bit, and the
    original-size stack is never written.  ``flat``: the flat buffer of the RESIZED layout (``resized_mask_layout``)."""
    device = _mask_device(device)
    out_lay, obj_out = resized_mask_layout(lay, out_sizes, flips)
    flat = mask_flat(out_lay, device, flat)
    if t["n"]:
        t = _resized_tables(t, out_lay, obj_out)
        names = ("pts", "part_off", "part_obj", "edge_pt_off", "part_ws_off", "obj_hw", "obj_out", "obj_out_off")
        d = _upload_tables(t, names, device)
        ws_bytes = 4 * int(t["part_ws_off"][-1])
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        p = [_ptr(d[k]) if d[k].numel() else None for k in names]
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_poly_masks_resized_u8(*p, _ptr(flat), flat.numel(), _ptr(ws) if ws_bytes else None,
                                                                   ws_bytes, t["P"], t["V"], t["T"], t["n"], _stream()),
                          "seam_poly_masks_resized_u8")
    return mask_views(flat, out_lay)


def launch_rle_masks_resized(lay: MaskLayout, t: dict, out_sizes, flips, device, flat: Optional[torch.Tensor] = None) -> list:
    """``launch_rle_masks`` with the expand of ``seam_rle_masks_resized_u8`` (arguments as ``launch_poly_masks_resized``)."""
    device = _mask_device(device)
    out_lay, obj_out = resized_mask_layout(lay, out_sizes, flips)
    flat = mask_flat(out_lay, device, flat)
    if t["n"]:
        t = _resized_tables(t, out_lay, obj_out)
        names = ("run_start", "obj_run_off", "obj_hw", "obj_out", "obj_out_off")
        d = _upload_tables(t, names, device)
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_rle_masks_resized_u8(*[_ptr(d[k]) for k in names], _ptr(flat), flat.numel(), t["n"],
                                                                  _stream()), "seam_rle_masks_resized_u8")
    return mask_views(flat, out_lay)


def poly_masks(polys: Sequence[Sequence], sizes: Sequence[Sequence[int]], device) -> list:
    """Polygon annotations of a batch of images -> list of uint8 0/1 [n_i,H_i,W_i] device stacks (views of one flat buffer), one
    table upload and one launch sequence for the batch; arguments and errors as ``pack_poly_masks``, no object may be None."""
    if any(o is None for img in polys for o in img):
        raise ValueError("poly_masks: every object needs a list of parts")
    return launch_poly_masks(*pack_poly_masks(polys, sizes), device)


def rle_masks(rles: Sequence[Sequence], sizes: Sequence[Sequence[int]], device) -> list:
    """Uncompressed RLE annotations of a batch of images -> list of uint8 0/1 [n_i,H_i,W_i] device stacks; arguments and errors
    as ``pack_rle_masks``, no object may be None."""
    if any(o is None for img in rles for o in img):
        raise ValueError("rle_masks: every object needs its counts")
    return launch_rle_masks(*pack_rle_masks(rles, sizes), device)


# ---------------------------------------------------------------------------------------------------- masks to RLE (csrc/seam_rle.hip)
def _rle_cells(h: int, w: int) -> int:
    b = int(_native.lib().seam_rle_encode_ws_bytes(int(h), int(w)))
    if b == 0:
        raise ValueError(f"rle_encode: size ({h}, {w}) must be (h, w) with 1 <= h, w <= {MASK_MAX_SIDE} and h*w < 2^31")
    return b // 4


def _rle_finish(counts: torch.Tensor, last_cell: torch.Tensor, hws, positions_launch) -> list:
    """The second half of both encoders: prefix sum, the per-object ends to the host (copy 1), the positions kernel into a
    buffer of exactly that size, the positions to the host (copy 2), then ``diff([0, *positions, h*w])`` per object."""
    import numpy as np
    scan = torch.cumsum(counts, 0)                                   # int64, inclusive
    ends = scan[last_cell].cpu().numpy()                             # device-to-host copy 1 of 2: the totals
    total = int(ends[-1])
    pos = torch.empty((total,), dtype=torch.int32, device=counts.device)
    positions_launch(scan, pos, total)
    pos = pos.cpu().numpy().astype(np.int64) if total else np.zeros(0, np.int64)      # copy 2 of 2: the positions
    return rle_counts_from_positions(pos, ends, hws)


def rle_counts_from_positions(pos, ends, hws) -> list:
    """Host: the batch's run boundaries (object o's are ``pos[ends[o-1]:ends[o]]``, ascending) -> per object
    ``diff([0, *positions, h*w])``, all objects in one pass."""
    import numpy as np
    n = len(hws)
    ends = np.asarray(ends, dtype=np.int64)
    lens = np.diff(ends, prepend=0)
    first = np.cumsum(lens + 2) - (lens + 2)                         # each object's slot for its leading 0
    edges = np.zeros(int(ends[-1]) + 2 * n, np.int64)
    edges[np.arange(pos.size, dtype=np.int64) + 2 * np.repeat(np.arange(n, dtype=np.int64), lens) + 1] = pos
    edges[first + lens + 1] = [h * w for h, w in hws]
    runs = np.diff(edges)
    keep = np.ones(runs.size, dtype=bool)
    keep[first[1:] - 1] = False                                      # the step from one object's h*w to the next one's 0
    return np.split(runs[keep], np.cumsum(lens + 1)[:-1])


def rle_encode(flat: torch.Tensor, lay: MaskLayout) -> list:
    """The objects of a flat uint8 mask buffer (``mask_flat`` / ``mask_views``; a pixel is set iff its byte != 0) -> one NumPy
    int64 ``counts`` array per object, maskApi's ``rleEncode``: column-major runs of 0 and 1 alternating, the first a run of
    zeros (``[h*w]`` for an empty mask, ``[0, h*w]`` for a full one).  Two device-to-host copies whatever the number of objects:
    the per-object totals, then the run boundaries."""
    import numpy as np
    flat = _req(flat, torch.uint8, "flat")
    if flat.dim() != 1 or flat.numel() != lay.total or not flat.is_cuda:
        raise ValueError(f"rle_encode: flat must be a uint8 [{lay.total}] tensor on the HIP device")
    n = int(len(lay.obj_off))
    if n == 0:
        return []
    hw_host = np.ascontiguousarray(lay.obj_hw, dtype=np.int32).reshape(n, 2)
    cells_of = {}
    for h, w in {(int(h), int(w)) for h, w in hw_host}:
        cells_of[(h, w)] = _rle_cells(h, w)
    cell_off = np.zeros(n + 1, np.int64)
    np.cumsum([cells_of[(int(h), int(w))] for h, w in hw_host], out=cell_off[1:])
    cells = int(cell_off[-1])
    tables = dict(obj_hw=hw_host, obj_off=np.ascontiguousarray(lay.obj_off, dtype=np.int64), cell_off=cell_off)
    d = _upload_tables(tables, ("obj_hw", "obj_off", "cell_off"), flat.device)
    ws = torch.empty((cells,), dtype=torch.int32, device=flat.device)
    counts = torch.empty((cells,), dtype=torch.int32, device=flat.device)
    lib = _native.lib()
    hw_ptr = hw_host.ctypes.data_as(C.c_void_p)
    with torch.cuda.device(flat.device):
        _native.check(lib.seam_rle_encode_masks_u8(_ptr(flat), flat.numel(), hw_ptr, _ptr(d["obj_hw"]), _ptr(d["obj_off"]),
                                                   _ptr(d["cell_off"]), _ptr(ws), 4 * cells, _ptr(counts), n, _stream()),
                      "seam_rle_encode_masks_u8")

        def positions(scan, pos, total):
            _native.check(lib.seam_rle_positions_masks(hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * cells,
                                                       _ptr(scan), _ptr(pos) if total else None, total, n, _stream()),
                          "seam_rle_positions_masks")

        return _rle_finish(counts, d["cell_off"][1:] - 1, [(int(h), int(w)) for h, w in hw_host], positions)


def rle_encode_paste(probs: torch.Tensor, boxes: torch.Tensor, hw) -> list:
    """The detections of one image, probs [D,1,28,28] or [D,28,28] and boxes [D,4] in pixels of the ``hw = (H, W)`` image ->
    one NumPy int64 ``counts`` array per detection: the RLE of ``paste_masks(probs, boxes, hw) > 0.5`` bit for bit (the set
    ``mask_inter`` counts), without the [D,1,H,W] paste -- only each clipped integer box is evaluated, each pixel once.  Two
    device-to-host copies, as ``rle_encode``."""
    probs, boxes = _req(probs, name="probs"), _req(boxes, name="boxes")
    d = probs.shape[0]
    if tuple(probs.shape[1:]) not in ((1, 28, 28), (28, 28)) or tuple(boxes.shape) != (d, 4):
        raise ValueError("rle_encode_paste: probs must be [D,1,28,28] or [D,28,28] and boxes [D,4]")
    if not probs.is_cuda or boxes.device != probs.device:
        raise ValueError("rle_encode_paste: probs and boxes must be on one HIP device")
    if boxes.data_ptr() & 15:                                       # the kernel reads a box as one float4
        boxes = boxes.clone()
    h, w = int(hw[0]), int(hw[1])
    per = _rle_cells(h, w)
    if d == 0:
        return []
    cells = per * d
    ws = torch.empty((cells,), dtype=torch.int32, device=probs.device)
    counts = torch.empty((cells,), dtype=torch.int32, device=probs.device)
    lib = _native.lib()
    with torch.cuda.device(probs.device):
        _native.check(lib.seam_rle_encode_paste_f32(_ptr(probs), _ptr(boxes), d, h, w, _ptr(ws), 4 * cells, _ptr(counts),
                                                    _stream()), "seam_rle_encode_paste_f32")

        def positions(scan, pos, total):
            _native.check(lib.seam_rle_positions_paste(d, h, w, _ptr(ws), 4 * cells, _ptr(scan), _ptr(pos) if total else None,
                                                       total, _stream()), "seam_rle_positions_paste")

        last = torch.arange(1, d + 1, device=probs.device, dtype=torch.int64) * per - 1
        return _rle_finish(counts, last, [(h, w)] * d, positions)


# ---------------------------------------------------------------------------------------------------- RLE algebra on bitmaps (csrc/seam_rle.hip)
RLE_BITS_BUDGET_BYTES = 64 << 20   # bitmap words (and dense bytes packed into them) of one chunk of a merge / iou / scoring job


@dataclass
class BitsLayout:
    """The objects of one bitmap workspace (int32 words, ``[ceil(h/32)][w]`` per object): object o's words start at
    ``cell_off[o]``; the objects lie one after the other in index order."""
    hw: object                     # NumPy int32 [n,2], the launchers' host table
    cell_off: object               # NumPy int64 [n+1], running sum of the objects' cells
    dev: dict                      # device tables: obj_hw int32 [n,2], cell_off int64 [n+1]

    @property
    def n(self) -> int:
        return int(self.hw.shape[0])

    @property
    def cells(self) -> int:
        return int(self.cell_off[-1])

    @property
    def hw_ptr(self):
        return self.hw.ctypes.data_as(C.c_void_p)


def rle_bits_cells(sizes: Sequence[Sequence[int]]) -> list:
    """Words of each object's bitmap, ``w * ceil(h/32)``; ValueError for a size the kernels refuse."""
    memo = {}
    return [memo[s] if s in memo else memo.setdefault(s, _rle_cells(*s)) for s in ((int(h), int(w)) for h, w in sizes)]


def _bits_layout(sizes, device, extra: Optional[dict] = None):
    """-> (layout, device copies of ``extra``'s tables): one upload for everything a chunk needs."""
    import numpy as np
    hw = np.ascontiguousarray(np.asarray([(int(h), int(w)) for h, w in sizes], np.int32).reshape(-1, 2))
    cell_off = np.zeros(len(hw) + 1, np.int64)
    np.cumsum(rle_bits_cells(hw.tolist()), out=cell_off[1:])
    tables = dict(extra or {}, obj_hw=hw, cell_off=cell_off)
    d = _upload_tables(tables, tuple(tables), device)
    return BitsLayout(hw, cell_off, dict(obj_hw=d["obj_hw"], cell_off=d["cell_off"])), d


def rle_bits(counts_per_object: Sequence, sizes: Sequence[Sequence[int]], device=None, dense=None):
    """Uncompressed RLE counts -> bitmaps, one bit per pixel, without a dense mask (``seam_rle_bits_from_runs``).
    ``counts_per_object[o]``: object o's counts, ``sizes[o] = (h, w)`` (any mix of sizes).  ``dense``: optional
    ``(flat uint8 tensor, byte offsets, sizes)`` of further objects that lie as row-major masks on the device (the rasteriser's
    output); they follow the run-list objects in the workspace, packed by the encoder's values stage.
    -> (ws int32 [cells] device tensor, BitsLayout).  One table upload; errors as ``pack_rle_masks``."""
    import numpy as np
    device = _mask_device(device if device is not None else (dense[0].device if dense is not None else "cuda"))
    n_runs_obj = len(counts_per_object)
    if len(sizes) != n_runs_obj:
        raise ValueError(f"rle_bits: {n_runs_obj} objects but {len(sizes)} sizes")
    _, t = pack_rle_masks([[c] for c in counts_per_object], sizes)   # validates: integers, non-negative, sum h*w
    d_sizes = [(int(h), int(w)) for h, w in dense[2]] if dense is not None else []
    extra = dict(run_start=t["run_start"], obj_run_off=t["obj_run_off"])
    all_sizes = [(int(h), int(w)) for h, w in sizes] + d_sizes
    cells = rle_bits_cells(all_sizes)
    first_dense = int(sum(cells[:n_runs_obj]))
    if d_sizes:
        extra["dense_off"] = np.asarray(dense[1], np.int64).reshape(-1)
        if extra["dense_off"].size != len(d_sizes):
            raise ValueError("rle_bits: one byte offset per dense object is needed")
        extra["dense_cell_off"] = np.cumsum([0] + cells[n_runs_obj:-1], dtype=np.int64)      # from the dense objects' first word
    lay, d = _bits_layout(all_sizes, device, extra)
    ws = torch.empty((lay.cells,), dtype=torch.int32, device=device)
    lib = _native.lib()
    with torch.cuda.device(device):
        if n_runs_obj:
            _native.check(lib.seam_rle_bits_from_runs(_ptr(d["run_start"]) if d["run_start"].numel() else None, _ptr(d["obj_run_off"]),
                                                      int(t["obj_run_off"][-1]), lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]),
                                                      _ptr(ws), 4 * lay.cells, n_runs_obj, _stream()), "seam_rle_bits_from_runs")
        if d_sizes:
            flat = _req(dense[0], torch.uint8, "dense")
            if flat.dim() != 1 or flat.device != device:
                raise ValueError(f"rle_bits: the dense buffer must be a flat uint8 tensor on {device}")
            tail = ws[first_dense:]
            scratch = torch.empty_like(tail)                          # the encoder's count stage comes with its values stage
            hw_tail = np.ascontiguousarray(lay.hw[n_runs_obj:])
            _native.check(lib.seam_rle_encode_masks_u8(_ptr(flat), flat.numel(), hw_tail.ctypes.data_as(C.c_void_p),
                                                       _ptr(d["obj_hw"][2 * n_runs_obj:]), _ptr(d["dense_off"]),
                                                       _ptr(d["dense_cell_off"]), _ptr(tail), 4 * tail.numel(), _ptr(scratch),
                                                       len(d_sizes), _stream()), "seam_rle_encode_masks_u8")
    return ws, lay


def bits_combine(ws: torch.Tensor, lay: BitsLayout, groups: Sequence[Sequence[int]], intersect: bool = False):
    """``groups[g]``: indices of objects of ``(ws, lay)``, all of one size -> (ws2, lay2) with object g the union (``intersect``:
    the intersection) of its group (``seam_rle_bits_combine``).  ValueError for an empty group, an index out of range or a group
    of mixed sizes."""
    import numpy as np
    sizes = []
    for g, grp in enumerate(groups):
        idx = [int(i) for i in grp]
        if not idx or min(idx) < 0 or max(idx) >= lay.n:
            raise ValueError(f"bits_combine: group {g} must name at least one object of 0..{lay.n - 1}")
        shapes = {(int(lay.hw[i, 0]), int(lay.hw[i, 1])) for i in idx}
        if len(shapes) > 1:
            raise ValueError(f"bits_combine: group {g} mixes the sizes {sorted(shapes)}")
        sizes.append(shapes.pop())
    group_off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=group_off[1:])
    group_obj = np.asarray([int(i) for g in groups for i in g], np.int32)
    lay2, d = _bits_layout(sizes, ws.device, dict(group_off=group_off, group_obj=group_obj))
    ws2 = torch.empty((lay2.cells,), dtype=torch.int32, device=ws.device)
    if groups:
        with torch.cuda.device(ws.device):
            _native.check(_native.lib().seam_rle_bits_combine(
                _ptr(d["group_off"]), _ptr(d["group_obj"]), int(group_obj.size), _ptr(lay.dev["obj_hw"]), _ptr(lay.dev["cell_off"]),
                _ptr(ws), 4 * ws.numel(), lay.n, lay2.hw_ptr, _ptr(lay2.dev["obj_hw"]), _ptr(lay2.dev["cell_off"]), _ptr(ws2),
                4 * lay2.cells, lay2.n, int(bool(intersect)), _stream()), "seam_rle_bits_combine")
    return ws2, lay2


def bits_to_rle(ws: torch.Tensor, lay: BitsLayout) -> list:
    """Bitmaps -> one NumPy int64 canonical ``counts`` array per object (``seam_rle_count_bits``, the prefix sum,
    ``seam_rle_positions_masks``): what ``rle_encode`` gives for the same masks.  Two device-to-host copies, as ``rle_encode``."""
    if lay.n == 0:
        return []
    counts = torch.empty((lay.cells,), dtype=torch.int32, device=ws.device)
    lib = _native.lib()
    d = lay.dev
    with torch.cuda.device(ws.device):
        _native.check(lib.seam_rle_count_bits(lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * lay.cells,
                                              _ptr(counts), lay.n, _stream()), "seam_rle_count_bits")

        def positions(scan, pos, total):
            _native.check(lib.seam_rle_positions_masks(lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * lay.cells,
                                                       _ptr(scan), _ptr(pos) if total else None, total, lay.n, _stream()),
                          "seam_rle_positions_masks")

        return _rle_finish(counts, d["cell_off"][1:] - 1, [(int(h), int(w)) for h, w in lay.hw], positions)


def bits_inter(ws: torch.Tensor, lay: BitsLayout, pairs, areas: bool = True) -> torch.Tensor:
    """``pairs`` int [P,2] (object indices of one size each) -> device int64 ``[P (+ n)]``: the pairs' ``popcount(a & b)``
    (``seam_rle_bits_inter``) followed, with ``areas``, by every object's own popcount (``seam_rle_bits_area``), so that one
    host copy brings both.  ValueError for an index out of range or a pair of two sizes."""
    import numpy as np
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    if pairs.size and (pairs.min() < 0 or pairs.max() >= lay.n):
        raise ValueError(f"bits_inter: pairs must name objects of 0..{lay.n - 1}")
    if pairs.size and (lay.hw[pairs[:, 0]] != lay.hw[pairs[:, 1]]).any():
        raise ValueError("bits_inter: the two objects of a pair must share a size")
    P = int(pairs.shape[0])
    out = torch.empty((P + (lay.n if areas else 0),), dtype=torch.int64, device=ws.device)
    lib = _native.lib()
    d = lay.dev
    with torch.cuda.device(ws.device):
        if P:
            dp = torch.from_numpy(pairs.astype(np.int32)).to(ws.device)
            _native.check(lib.seam_rle_bits_inter(_ptr(dp), P, lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws),
                                                  4 * lay.cells, lay.n, _ptr(out), _stream()), "seam_rle_bits_inter")
        if areas and lay.n:
            _native.check(lib.seam_rle_bits_area(lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * lay.cells, lay.n,
                                                 _ptr(out[P:]), _stream()), "seam_rle_bits_area")
    return out


def budget_chunks(costs: Sequence[int], budget: int = None) -> list:
    """Consecutive index ranges ``(lo, hi)`` whose costs sum to at most ``budget`` (``RLE_BITS_BUDGET_BYTES``); an item that
    alone exceeds it gets a chunk of its own."""
    budget = RLE_BITS_BUDGET_BYTES if budget is None else int(budget)
    out, lo, acc = [], 0, 0
    for i, c in enumerate(costs):
        if i > lo and acc + c > budget:
            out.append((lo, i))
            lo, acc = i, 0
        acc += int(c)
    if len(costs) > lo:
        out.append((lo, len(costs)))
    return out


def rle_merge(groups: Sequence[Sequence], sizes: Sequence[Sequence[int]], intersect: bool = False) -> list:
    """``groups[g]``: the counts arrays of the RLEs to merge, all of ``sizes[g]`` -> one canonical counts array per group.  The
    groups are processed in chunks of ``RLE_BITS_BUDGET_BYTES`` of source and destination bitmaps."""
    cells = rle_bits_cells(sizes)
    out = []
    for lo, hi in budget_chunks([4 * c * (len(g) + 1) for c, g in zip(cells, groups)]):
        flat = [c for g in groups[lo:hi] for c in g]
        flat_sizes = [sizes[i] for i in range(lo, hi) for _ in groups[i]]
        ws, lay = rle_bits(flat, flat_sizes)
        idx, k = [], 0
        for g in groups[lo:hi]:
            idx.append(list(range(k, k + len(g))))
            k += len(g)
        out += bits_to_rle(*bits_combine(ws, lay, idx, intersect))
    return out


# ------------------------------------------------------------------------------ optimizer step + in-place pack refresh
def sgd_chunk_table(numels: Sequence[int], chunk: int):
    """Host logic of ``seam_sgd_step_f32``'s chunk table: (tensor, count, offset) rows that put every element of every tensor into
    exactly one chunk of at most ``chunk`` elements, offsets multiples of ``chunk``, no row for an empty tensor."""
    rows = []
    for t, n in enumerate(numels):
        n = int(n)
        if n < 0:
            raise ValueError("sgd_chunk_table: negative element count")
        for off in range(0, n, chunk):
            rows.append((t, min(chunk, n - off), off))
    return rows


def _upload(ctypes_array, device) -> torch.Tensor:
    """A ctypes table as a uint8 device tensor (the caller keeps it alive while kernels read it)."""
    host = torch.frombuffer(bytearray(bytes(ctypes_array)), dtype=torch.uint8)
    return host.to(device)


_PACK_RECORDER = None


class _PackRecorder:
    def __init__(self):
        self.records = []      # (weight handed to the pack kernels, bias argument, bn argument, mode, PackedConv)
        self.derived = []      # (tensor, fn, deps): pack sources / shifts computed from parameters by ``derived_source``


class record_packs:
    """While active, ``pack_conv`` / ``pack_conv_dual`` / ``derived_source`` note what they packed from what (``PackPlan``)."""

    def __enter__(self):
        global _PACK_RECORDER
        self._prev, _PACK_RECORDER = _PACK_RECORDER, _PackRecorder()
        return _PACK_RECORDER

    def __exit__(self, *exc):
        global _PACK_RECORDER
        _PACK_RECORDER = self._prev
        return False


def derived_source(fn, deps: Sequence[torch.Tensor]) -> torch.Tensor:
    """``fn()``: a tensor a module computes from the parameters ``deps`` and hands to ``pack_conv`` as weight or bias (the stem's
    space-to-depth weight, the RPN head's stacked logits / deltas rows, the folded shortcut pair).  Under ``record_packs`` the
    recipe is noted, so that ``PackPlan.refresh`` can recompute the tensor in place when a dependency moved."""
    t = fn()
    if _PACK_RECORDER is not None:
        _PACK_RECORDER.derived.append((t, fn, tuple(deps)))
    return t


class PackPlan:
    """The in-place refresh of the cached packs of ``backbone.body``, ``backbone.fpn`` and ``rpn.head`` after an optimizer step.

    Built once: every covered module repacks by its own ``packed()`` under ``record_packs``, which yields, per pack, the source (a
    parameter, or a ``derived_source``) and the destination buffers.  ``rebuilds`` counts every later build.  ``refresh(updated)``
      * checks on the host that the plan still describes the model, by the two parts of ``models.packed.PackedWeights._pack_key``
        (the same ``_pk`` objects; tensors: the same parameter / buffer pointers, versions that moved by exactly the optimizer's
        one bump and only on updated parameters; switches: equal); otherwise it drops everything and rebuilds by the modules' own
        route -- it never writes through a stale pointer;
      * recomputes the derived sources whose parameters moved (torch; counted in ``fallback_calls``);
      * rewrites every weight-dependent buffer of every pack whose source moved in ONE ``seam_repack_many_f32`` launch on the
        current stream (``launches_per_refresh``); epilogue vectors of a frozen BN and packs of frozen layers are not touched;
      * sets each module's ``_pk_key`` to what ``packed()`` now computes: the next ``packed()`` is a hit on the same tensors.
    fp32 compute only (the exact packs and their split-bf16 twins)."""

    COVERED = ("backbone.body", "backbone.fpn", "rpn.head")

    def __init__(self, model):
        self.modules = []
        for path in self.COVERED:
            m = model
            for part in path.split("."):
                m = getattr(m, part, None)
                if m is None:
                    break
            if isinstance(m, PackedWeights):
                self.modules.append((path, m))
        if not self.modules:
            raise ValueError("PackPlan: the model has none of " + ", ".join(self.COVERED))
        self.refreshes = self.rebuilds = self.table_uploads = 0
        self.launches_per_refresh = self.fallback_calls = 0
        self._built = self._ever_built = False

    # -- build
    def build(self):
        """Build the plan now (``optim.SGD`` does, when it is given the model): every covered module repacks once by its own route."""
        if not self._built:
            self._build()
        return self

    def rebuild_after_edit(self):
        """The last in-place refresh followed an edit of a parameter that no version counter showed (``optim.SGD`` found the
        parameters changed under it): treat it like any other edit -- drop the plan and rebuild by the modules' own route."""
        self.refreshes -= 1
        self._build()

    def _build(self):
        self._built = False
        self._pk, self._keys, self._entries, self._derived = [], [], [], []
        self._table_for, self._table = None, None
        for path, m in self.modules:
            m._pk_key = None
            with record_packs() as rec:
                pk = m.packed()
            params = {p.data_ptr(): p for p in m.parameters() if p.numel()}
            derived = {t.data_ptr(): (t, fn, deps) for t, fn, deps in rec.derived}
            self._derived += [d for d in rec.derived if d[2]]

            def deps_of(t, what):
                if t.data_ptr() in params:
                    return (params[t.data_ptr()],)
                if t.data_ptr() in derived:
                    return derived[t.data_ptr()][2]
                raise NotImplementedError(f"PackPlan: {path}: the {what} of a pack is neither a parameter nor a derived_source")

            for weight, bias, bn, mode, pc in rec.records:
                wdeps = deps_of(weight, "weight")
                if bias is not None:
                    if bn is not None or pc.shift is None or pc.shift.data_ptr() != bias.data_ptr():
                        raise NotImplementedError(f"PackPlan: {path}: a pack whose shift is computed from its bias is not covered")
                    deps_of(bias, "bias")           # a parameter (the shift aliases it) or a derived_source (refreshed with it)
                self._entries.append((wdeps, self._jobs_of(path, weight, mode, pc)))
            self._pk.append(pk)
            self._keys.append(m._pack_key())
        self.rebuilds += self._ever_built
        self._built = self._ever_built = True

    @staticmethod
    def _jobs_of(path, weight, mode, pc):
        N = _native

        def job(form, dst, R=1, S=1, cs=pc.Cstore, cin=pc.Cin, md=0, scale=None):
            return N.RepackJob(src=weight.data_ptr(), dst=dst.data_ptr(), scale=None if scale is None else scale.data_ptr(), form=form,
                               K=pc.K, Cin=cin, R=R, S=S, Cstore=cs, mode=md)

        if pc.dtype in _SX_TERMS:
            jobs = [job(N.REPACK_SPLIT3, pc.w, pc.R, pc.S, md=mode)]
            if pc.wx is not None:
                jobs.append(job(N.REPACK_SXPC, pc.wx))
            if pc.wxs is not None:
                jobs.append(job(N.REPACK_SXPC64, pc.wxs))
            if pc.wx64 is not None:
                jobs.append(job(N.REPACK_SXPC64, pc.wx64))
            if pc.u24x is not None:
                jobs.append(job(N.REPACK_W24SX, pc.u24x, 3, 3, md=mode))
            return jobs
        if pc.dtype != F32 or pc.wh is not None or pc.wsh is not None or pc.wph is not None:
            raise NotImplementedError(f"PackPlan: {path}: only fp32 packs are refreshed in place (pass refresh_packs=False)")
        jobs = [job(N.REPACK_IGEMM, pc.w, pc.R, pc.S, md=mode)]
        if pc.u is not None:
            jobs.append(job(N.REPACK_WINO, pc.u, 3, 3, md=mode))
        if pc.u24 is not None:
            jobs.append(job(N.REPACK_WINO24, pc.u24, 3, 3, md=mode))
        if (pc.wn is not None or pc.ws is not None or pc.wq is not None) and mode != 0:
            raise NotImplementedError(f"PackPlan: {path}: the pointwise forms of a transposed conv are not covered")
        if pc.wn is not None:
            jobs.append(job(N.REPACK_NARROW, pc.wn))
        if pc.ws is not None and pc.ws.data_ptr() != weight.data_ptr():      # (without a scale the rows ARE the weight: nothing to do)
            jobs.append(job(N.REPACK_SW, pc.ws, scale=pc.scale))
        if pc.wq is not None:
            jobs.append(job(N.REPACK_PC, pc.wq))
        return jobs

    # -- the host checks
    def _valid(self, updated) -> bool:
        for (path, m), pk, old in zip(self.modules, self._pk, self._keys):
            if m._pk is not pk:
                return False
            (old_tensors, old_switches), (new_tensors, new_switches) = old, m._pack_key()
            if new_switches != old_switches or len(new_tensors) != len(old_tensors):      # compute dtype, split twins, pack-time knobs
                return False
            for t, a, b in zip(m._pack_tensors(), old_tensors, new_tensors):
                bump = 1 if id(t) in updated else 0
                if a[0] != b[0] or a[1] + bump != b[1]:
                    return False
        return True

    @torch.no_grad()
    def refresh(self, updated: Sequence[torch.Tensor]) -> bool:
        """``updated``: the parameters the optimizer just changed, their versions bumped once.  True: refreshed in place; False:
        the plan was (re)built by the modules' own route."""
        ids = frozenset(id(p) for p in updated)
        if not self._built or not self._valid(ids):
            self._build()
            return False
        lib = _native.lib()
        calls = 0
        for t, fn, deps in self._derived:
            if any(id(d) in ids for d in deps):
                t.copy_(fn())
                calls += 1
        if self._table_for != ids:
            jobs = [j for deps, js in self._entries if any(id(d) in ids for d in deps) for j in js]
            arr = (_native.RepackJob * max(1, len(jobs)))(*jobs)
            blocks = int(lib.seam_repack_layout(arr, len(jobs)))
            if blocks < 0:
                raise _native.SeamNativeError(f"seam_repack_layout refused job {-1 - blocks}")
            dev = self.modules[0][1]._pack_tensors()[0].device
            self._table = (_upload(arr, dev) if jobs else None, len(jobs), blocks)
            self._table_for = ids
            self.table_uploads += 1
        table, n, blocks = self._table
        if n:
            _native.check(lib.seam_repack_many_f32(_ptr(table), n, blocks, _stream()), "seam_repack_many_f32")
        for i, (path, m) in enumerate(self.modules):
            m._pk_key = self._keys[i] = m._pack_key()
        self.refreshes += 1
        self.launches_per_refresh = 1 if n else 0
        self.fallback_calls = calls
        return True
