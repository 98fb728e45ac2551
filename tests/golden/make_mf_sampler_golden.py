#!/usr/bin/env python3
"""Golden batches of the MovingFashion batch sampler, captured by running the reference's own ``MFBatchSampler``
(datasets/MFDataset.py:137-192) over the cases of tests/mf_fixture.py with Python's ``random`` seeded per case.

Run:  python tests/golden/make_mf_sampler_golden.py <path of the reference checkout>

The reference module imports cv2 at its top, which the sampler never touches: an empty stand-in is put into ``sys.modules``, as
tests/golden/make_eval_golden.py does for the modules ``evaluate()`` never touches.  What is stored (outputs only, no reference
source text): per case the batches as lists ``[i, tag, t(, video_i)]`` and ``len(sampler)`` -> tests/golden/mf_sampler_golden.json.
"""
import json
import os
import random
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mf_fixture as MF                                      # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.modules["cv2"] = types.ModuleType("cv2")
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_mfdataset", os.path.join(sys.argv[1], "datasets", "MFDataset.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    MFBatchSampler = module.MFBatchSampler
    out = {}
    for name, (n, batch_size, drop_last, kw, seed) in MF.SAMPLER_CASES.items():
        sampler = MFBatchSampler(None, torch.utils.data.SequentialSampler(range(n)), batch_size, drop_last, **kw)
        random.seed(seed)
        out[name] = {"batches": MF.as_json(list(sampler)), "len": len(sampler)}
    path = os.path.join(HERE, "mf_sampler_golden.json")
    with open(path, "w") as fp:
        json.dump(out, fp, sort_keys=True)
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
