"""Multi-DeepFashion2 evaluator (seam-match-rcnn_amd/evaluator_df2.py), CPU side: the scenarios are the ones the golden file was
made from, the report prints and writes what the reference printed and wrote, the GT-row rules, argument checks."""
import io
import os

import numpy as np
import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def df2_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "eval_df2_golden.npz")))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_scenario_builder_reproduces_the_golden_loader(name, df2_golden):
    import eval_df2_scenarios as DS
    loader, canned, _ = DS.build(name)
    assert DS.loader_digest(loader, canned) == str(df2_golden[f"{name}_loader_sha256"])


COUNTS = {"frame": "k_accs", "max_per_image": "k_accs_avg", "avg_desc": "k_accs_avg_desc", "aggr_desc": "k_accs_aggr_desc",
          "avg_dist": "k_accs_avg_dist", "max_dist": "k_accs_max_dist", "max_score": "k_accs_max_score"}


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_report_prints_and_writes_the_reference_output(name, df2_golden, tmp_path):
    """DF2Report fed the reference's own counters prints its six tables + rank quartiles and writes its CSV byte for byte."""
    from seam_match_rcnn_amd.evaluator_df2 import DF2Report
    import eval_df2_scenarios as DS
    g = df2_golden
    fpp = DS.scenario(name)["params"]["frames_per_product"]
    rep = DF2Report(k_thresholds=(1, 5, 10, 20), counts={k: g[f"{name}_{v}"] for k, v in COUNTS.items()},
                    count_street=int(g[f"{name}_count_street"]), frames_per_product=fpp,
                    frame_ranks=g[f"{name}_all_ranks_list"].tolist())
    assert int(g[f"{name}_total_querys"]) == rep.count_street * fpp
    assert rep.tables_text() == str(g[f"{name}_stdout"])
    buf = io.StringIO()
    np.savetxt(buf, rep.perf_rows(), fmt="%02.2f", delimiter="\t")
    assert buf.getvalue() == str(g[f"{name}_perf_csv"])
    rep.save_artifacts(str(tmp_path))
    csvs = os.listdir(tmp_path / "logs_mdf2")
    assert len(csvs) == 1 and (tmp_path / "logs_mdf2" / csvs[0]).read_text() == str(g[f"{name}_perf_csv"])
    assert (tmp_path / "accs_per_product_10frame_df2.pth").exists()
    np.testing.assert_allclose(rep.summary(), g[f"{name}_ret"], rtol=0, atol=1e-12)


def test_golden_covers_the_scenario_features(df2_golden):
    """What the scenarios were built to exercise really happened in the reference's run."""
    g = df2_golden
    assert int(g["B_count_street"]) < int(g["B_count_products"])                        # gallery-only products
    assert 2 not in g["B_shop_prods"].tolist() and 9 not in g["B_shop_prods"].tolist()  # skipped at the shop image
    assert int(g["B_shop_maxind"][g["B_shop_prods"].tolist().index(4)]) == 1            # kept position read from the full list
    a = g["A_street_prods"].tolist()
    assert sum(1 for p, i in zip(a, g["A_street_imgs"].tolist()) if p == 6) == 2        # the empty street frame is skipped
    for k in ("k_accs",):
        for name in "ABC":
            total = int(g[f"{name}_total_querys"])
            hits = g[f"{name}_{k}"]
            assert (hits[:3] > 0).all() and (hits[:3] < total).all()


def test_gt_row_resolution_rules():
    from seam_match_rcnn_amd.evaluator_df2 import resolve_gt_row
    styles, pairs = torch.tensor([1, 3, 3]), torch.tensor([7, 8, 9])
    assert resolve_gt_row(styles, pairs, 3, 9, 3) == 2                 # found
    assert resolve_gt_row(styles, pairs, 3, 9, 2) == -1                # the scan is bounded by the image's own GT count
    assert resolve_gt_row(styles, pairs, 5, 5, 3) == -1                # not found: -1 = the image's last row
    assert resolve_gt_row([1, 3], [7, 8], 3, 8, 0) == -1               # no GT row at all
    with pytest.raises(ValueError, match="street frame 4"):            # the scan runs past the shop's lists (reference: IndexError)
        resolve_gt_row([1, 3], [7, 8], 5, 5, 3, where="product 2 ('5_5'), street frame 4")
    assert resolve_gt_row([1, 3], [7, 8], 3, 8, 3) == 1                # found before the shop's list ends


def test_strategy_is_validated():
    from seam_match_rcnn_amd import evaluator_df2 as EV
    assert EV.check_strategy("best_match") == "best_match" and EV.check_strategy("best_box_only") == "best_box_only"
    with pytest.raises(ValueError, match="strategy"):
        EV.evaluate(None, [], torch.device("cpu"), strategy="best_frame")


def test_gt_select_rejects_cpu_tensors():
    from seam_match_rcnn_amd import _native, ops
    boxes = torch.tensor([[0., 0., 10., 10.]])
    with pytest.raises(_native.SeamNativeError):
        ops.gt_select(boxes, torch.ones(1), [0, 1], boxes, [0, 1], torch.zeros(1, dtype=torch.int32), 0.1)
