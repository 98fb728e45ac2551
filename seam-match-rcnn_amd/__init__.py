"""seam-match-rcnn_amd: MI355X-native (gfx950) forward hot path of SEAM Match-RCNN.

Layout (only what the path needs):
  csrc/      hand-written HIP kernels + the C ABI (``include/seam_hip.h``)
  _native.py ctypes loader for ``lib/libseam_hip.so`` (fails loudly when missing)
  ops.py     thin launch wrappers (raw device pointers + current HIP stream): the convolutions, and the public namespace of
             every wrapper -- ``ops.<name>`` reaches the kernel families beside it:
               ops_elementwise.py  pooling, top-down add, layouts, RoIAlign      ops_input.py  preprocess, uint8 batches, frames
               ops_heads.py        NLB, pair logits, top-k, tracklets            ops_detect.py IoU, decoding, NMS, mask paste
               ops_train.py        gradients, sampling and losses of training    ops_masks.py  polygon / RLE masks, bitmap algebra
             (they import ``_ops_common.py`` and each other, never ``ops``)
  pack_plan.py  the in-place refresh of the cached weight packs after an optimizer step (above ``ops``)
  models/    host-side mirror of the reference's ``models/`` interface
  retrieval.py  clip sharding + RCCL all-gather of the product bank + match
  optim.py   SGD: the optimizer step in one launch + the in-place refresh of the cached weight packs
  mask_utils.py  ground-truth masks from COCO-style annotations, rasterised on the device
  synth.py   deterministic synthetic weights / inputs
"""
__version__ = "0.1.0"
