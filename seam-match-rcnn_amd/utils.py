"""The two helpers of the reference's ``stuffs/utils.py`` that its phase-1 loop imports (``train_matchrcnn.py``,
``stuffs/engine.py``)."""
from __future__ import annotations

import torch


def collate_fn(batch):
    """A list of ``(image, target, image_id)`` samples -> ``(images, targets, image_ids)`` tuples: images of different sizes are
    never stacked."""
    return tuple(zip(*batch))


def warmup_lr_scheduler(optimizer, warmup_iters, warmup_factor):
    """A ``LambdaLR`` that scales the learning rate by a factor rising linearly from ``warmup_factor`` at step 0 to 1 at step
    ``warmup_iters``, and by 1 from there on."""

    def factor(step):
        if step >= warmup_iters:
            return 1.0
        done = step / warmup_iters
        return warmup_factor + (1.0 - warmup_factor) * done

    return torch.optim.lr_scheduler.LambdaLR(optimizer, factor)
