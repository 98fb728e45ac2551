"""The convolutions: packs, routes, knobs and launch wrappers over the C ABI (``include/seam_hip.h``) -- and the public namespace of
every launch wrapper: the other kernel families live in the ``ops_*`` modules beside this one and are re-exported at the end.

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

from . import _native, ops_train
from ._ops_common import F16, F32, _ptr, _req, _stream, _upload      # noqa: F401  (_upload: reached as ops._upload)
from .ops_elementwise import upsample_add_


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


# ------------------------------------------------------------------------------ stride-2 input gradient (it runs pack_conv_dgrad / conv2d)
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
    limit = ops_train.WGRAD_MAX_OPERAND_BYTES         # read where it is assigned: the knob lives beside conv_wgrad_chunked
    if per > limit:
        raise ValueError(f"conv3x3s2_dgrad: one image's operand ({per} bytes) exceeds the limit of {limit}")
    step = max(1, min(n, limit // per))
    if step >= n:
        return _conv3x3s2_dgrad_one(dy, pk, (h, w), mask, out)
    if out is None:
        out = torch.empty((n, h, w, pk.C), dtype=F32, device=dy.device)
    for i in range(0, n, step):
        _conv3x3s2_dgrad_one(dy[i:i + step], pk, (h, w), None if mask is None else mask[i:i + step], out[i:i + step])
    return out


# ------------------------------------------------------------------------------ what pack_conv records for pack_plan.PackPlan
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


# ------------------------------------------------------------------------------ the other kernel families
# (a star import leaves private names behind: the three that the package, a test or a tool reaches through ops, by name)
from .ops_heads import _topk_k                              # noqa: E402,F401
from .ops_input import _launch_noise                        # noqa: E402,F401
from .ops_masks import _resized_tables                      # noqa: E402,F401
from .ops_elementwise import *      # noqa: E402,F401,F403
from .ops_input import *            # noqa: E402,F401,F403
from .ops_heads import *            # noqa: E402,F401,F403
from .ops_detect import *           # noqa: E402,F401,F403
from .ops_train import *            # noqa: E402,F401,F403
from .ops_masks import *            # noqa: E402,F401,F403
