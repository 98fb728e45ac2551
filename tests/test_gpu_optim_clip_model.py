"""GPU: ``optim.SGD(model=m, max_norm=..., skip_nonfinite=True)`` on the detector of ``test_gpu_optim_model.py`` (the tiny-frame
configuration, layer2..layer4 + FPN + RPN + heads trainable), whose helpers are imported.

After a clipped step the refreshed packs are the same tensor objects and the model computes what a fresh model built from its
``state_dict()`` computes, bit for bit: the assertion of the unclipped model test.  After a step whose loss was multiplied by inf
every weight and every pack holds the bytes of before, the step is counted as skipped, and the next forward gives the previous
outputs' bits."""
import pytest
import torch

from test_gpu_body_train_model import DEV, make_model, make_model_batch, run_model
from test_gpu_optim_model import SGD, all_packs, assert_matches_a_fresh_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch():
    return make_model_batch()


def features(m, images):
    with torch.no_grad():
        out = [f.clone() for f in m.eval().extract_features(images)[0].values()]
    m.train()
    return out


def test_a_clipped_step_refreshes_the_packs_and_a_non_finite_one_changes_nothing(batch):
    images, targets = batch
    m = make_model(3)
    run_model(m, images, targets)
    opt = SGD(m, max_norm=0.5, skip_nonfinite=True)
    before = all_packs(m)
    weights0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    opt.step()
    total, coef = float(opt.total_norm), float(opt.clip_coef)
    print("total_norm", total, "clip_coef", coef)
    assert total > 0.5 and coef < 1.0 and opt.skipped_steps() == 0
    after = all_packs(m)
    assert len(after) == len(before) and all(a is b for a, b in zip(after, before)), "packed() reallocated after the step"
    assert (opt.plan.refreshes, opt.plan.rebuilds, opt.table_uploads) == (1, 0, 1)
    assert any(not torch.equal(p, weights0[k]) for k, p in m.named_parameters() if p.requires_grad)
    assert_matches_a_fresh_model(m, batch)

    # a loss multiplied by inf: the gradients are inf / NaN, the step is dropped on the device
    weights = {k: v.detach().clone() for k, v in m.named_parameters()}
    bufs = {k: opt.state[p]["momentum_buffer"].clone() for k, p in m.named_parameters() if p in opt.state}
    packs = [t.clone() for t in all_packs(m)]
    f0 = features(m, images)
    m.rpn.sample_generator = torch.Generator(device=DEV).manual_seed(1)
    m.roi_heads.sample_generator = torch.Generator(device=DEV).manual_seed(2)
    m.zero_grad(set_to_none=True)
    (sum(m(images, targets).values()) * float("inf")).backward()
    refreshes = opt.plan.refreshes
    opt.step()
    assert opt.skipped_steps() == 1 and not bool(torch.isfinite(opt.total_norm))
    assert opt.plan.refreshes == refreshes + 1 and opt.plan.rebuilds == 0, "a skipped step refreshes the packs like any other"
    assert all(torch.equal(p.detach(), weights[k]) for k, p in m.named_parameters()), "a skipped step wrote a weight"
    assert bufs and all(torch.equal(opt.state[p]["momentum_buffer"], bufs[k]) for k, p in m.named_parameters() if k in bufs)
    now = all_packs(m)
    assert all(a is b for a, b in zip(now, before)) and all(torch.equal(a, b) for a, b in zip(now, packs)), "a pack changed"
    f1 = features(m, images)
    assert len(f0) == len(f1) and all(torch.equal(a, b) for a, b in zip(f0, f1)), "the next forward differs"
