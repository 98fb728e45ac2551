"""GPU: ``optim.SGD(..., model=m)`` on the detector in the reference's configuration (layer2..layer4 + FPN + RPN + heads trainable):
after a step the cached packs of the body, the FPN and the RPN head are the same tensor objects, rewritten in place, and the model
computes what a fresh model built from its ``state_dict()`` computes -- the construction of
``test_gpu_body_train_model.py::test_sgd_step_refreshes_the_packed_body_weights``, whose builders are imported.

The pack objects are collected after the optimizer is constructed (it builds its ``PackPlan`` there, through the modules' own
``packed()``) and before ``step()``.

Counters of one refresh in this configuration: ONE launch (``launches_per_refresh``) and five torch re-derivations
(``fallback_calls``): the folded conv3 + shortcut pairs of layer2.0 / layer3.0 / layer4.0 and the RPN head's stacked logits + deltas
weight and bias.  Neither depends on the number of layers or blocks.

``test_a_manual_edit_...[data]``: ``p.data.mul_(0.5)`` leaves ``p._version`` where it was (``.data`` has its own version counter),
so neither ``packed()`` nor the plan's host checks can see it.  The optimizer sees it in the SGD kernel's fingerprint: the sum over
the parameters as the kernel read them is not the sum of what the previous step wrote.  The ``no_grad`` form of the same edit bumps
the version and is caught by the host checks."""
import dataclasses

import pytest
import torch

from test_gpu_body_train_model import SIX, make_model, make_model_batch, run_model, same_losses

pytestmark = pytest.mark.gpu


def SGD(m, **kw):
    from seam_match_rcnn_amd.optim import SGD as S
    return S([p for p in m.parameters() if p.requires_grad], lr=0.01, momentum=0.9, model=m, **kw)


def covered(m):
    return [m.backbone.body, m.backbone.fpn, m.rpn.head]


def pack_tensors(pk):
    """every tensor of a module's ``packed()`` structure, in a fixed order"""
    from seam_match_rcnn_amd.ops import PackedConv
    if isinstance(pk, PackedConv):
        return [v for v in (getattr(pk, f.name) for f in dataclasses.fields(pk)) if isinstance(v, torch.Tensor)]
    if isinstance(pk, dict):
        return [t for k in pk for t in pack_tensors(pk[k])]
    if isinstance(pk, (list, tuple)):
        return [t for v in pk for t in pack_tensors(v)]
    return [pk] if isinstance(pk, torch.Tensor) else []


def all_packs(m):
    return [t for mod in covered(m) for t in pack_tensors(mod.packed())]


@pytest.fixture(scope="module")
def batch():
    return make_model_batch()


def assert_matches_a_fresh_model(m, batch):
    """eval features and the next training step's six losses (same sampler seeds), bit for bit"""
    images, targets = batch
    from seam_match_rcnn_amd.models.detection import set_split_f32
    fresh = make_model(3)
    fresh.load_state_dict(m.state_dict())
    set_split_f32(fresh, getattr(m.backbone.body, "split_f32", True))
    with torch.no_grad():
        f1 = list(m.eval().extract_features(images)[0].values())
        f2 = list(fresh.eval().extract_features(images)[0].values())
    assert len(f1) == len(f2) and all(torch.equal(a, b) for a, b in zip(f1, f2)), "eval features differ from a fresh model's"
    m.train()
    fresh.train()
    l1, _ = run_model(m, images, targets)
    l2, _ = run_model(fresh, images, targets)
    assert same_losses(l1, l2), {k: (float(l1[k]), float(l2[k])) for k in SIX}
    return l1


def test_one_step_refreshes_the_packs_in_place(batch):
    images, targets = batch
    m = make_model(3)
    run_model(m, images, targets)
    opt = SGD(m)
    plan = opt.plan
    frozen = {k: v.detach().clone() for k, v in m.state_dict().items()
              if k.startswith(("backbone.body.conv1", "backbone.body.bn1", "backbone.body.layer1")) or ".bn" in k or "downsample.1" in k}
    before = all_packs(m)
    body_pk = m.backbone.body.packed()
    frozen_packs = [t for key in ("stem", "stem_s2d", (1, 0), (1, 1), (1, 2)) for t in pack_tensors(body_pk[key])]
    frozen_packs_before = [t.clone() for t in frozen_packs]
    WEIGHT_FORMS, EPILOGUE = ("w", "u", "u24", "wn", "ws", "wq"), ("scale", "shift")
    entry = body_pk[(3, 1)]                                        # layer3.1: exact forms and split twins of a trainable block
    moved_before = {(k, f): getattr(pc, f).clone() for k, pc in entry.items() for f in WEIGHT_FORMS + EPILOGUE if getattr(pc, f) is not None}
    opt.step()
    after = all_packs(m)
    assert len(after) == len(before) and all(a is b for a, b in zip(after, before)), "packed() reallocated after the step"
    assert (plan.refreshes, plan.rebuilds, plan.launches_per_refresh, plan.fallback_calls, plan.table_uploads) == (1, 0, 1, 5, 1)
    assert opt.table_uploads == 1
    assert len(frozen) > 100 and all(torch.equal(v, frozen[k]) for k, v in m.state_dict().items() if k in frozen)
    assert all(torch.equal(a, b) for a, b in zip(frozen_packs, frozen_packs_before))
    assert {"c1", "c2", "c3", "c1x", "c3x"} <= set(entry) and sum(f in WEIGHT_FORMS for _, f in moved_before) >= 9
    for (k, f), old in moved_before.items():                       # every weight form moved, a frozen BN's epilogue did not
        assert torch.equal(getattr(entry[k], f), old) == (f in EPILOGUE), (k, f)
    assert_matches_a_fresh_model(m, batch)
    # a second step: nothing is uploaded again, the packs stay where they are
    run_model(m, images, targets)
    opt.step()
    assert (plan.refreshes, plan.rebuilds, plan.table_uploads) == (2, 0, 1) and all(a is b for a, b in zip(all_packs(m), before))


def test_refresh_off_gives_the_same_parameters_and_losses(batch):
    images, targets = batch
    out, grads = [], None
    for refresh in (True, False):
        m = make_model(3)
        if grads is None:
            _, grads = run_model(m, images, targets)
        for k, p in m.named_parameters():                          # both take the step from the same gradients
            p.grad = grads[k].clone() if k in grads else None
        opt = SGD(m, refresh_packs=refresh)
        opt.step()
        assert (opt.plan.refreshes == 1) == refresh
        losses, _ = run_model(m, images, targets)
        out.append((losses, {k: v.detach().clone() for k, v in m.named_parameters()}))
    (la, sa), (lb, sb) = out
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert same_losses(la, lb)


def _load_perturbed(m):
    sd = {k: (v * 1.01 if v.is_floating_point() and "running_var" not in k else v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)


def _split_off(m):
    from seam_match_rcnn_amd.models.detection import set_split_f32
    set_split_f32(m, False)


def _edit_no_grad(m):
    with torch.no_grad():
        m.backbone.body.layer3[2].conv2.weight.mul_(0.5)


def _edit_data(m):
    m.backbone.body.layer3[2].conv2.weight.data.mul_(0.5)


@pytest.mark.parametrize("disturb", [_load_perturbed, _split_off, _edit_no_grad, _edit_data],
                         ids=["load_state_dict", "set_split_f32", "no_grad", "data"])
def test_a_manual_edit_between_two_steps_rebuilds_the_plan(batch, disturb):
    images, targets = batch
    m = make_model(3)
    opt = SGD(m)
    run_model(m, images, targets)
    opt.step()
    assert (opt.plan.refreshes, opt.plan.rebuilds) == (1, 0)
    disturb(m)
    run_model(m, images, targets)
    opt.step()
    print("rebuilds after the disturbed step:", opt.plan.rebuilds, "refreshes:", opt.plan.refreshes)
    assert_matches_a_fresh_model(m, batch)
    assert opt.plan.rebuilds == 1, "the step after the disturbance must rebuild the plan"
    run_model(m, images, targets)
    opt.step()                                                    # the rebuilt plan serves the next step in place
    assert (opt.plan.rebuilds, opt.plan.refreshes) == (1, 2)
