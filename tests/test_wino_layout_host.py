"""CPU: the block-layout chooser the F(2x2) and F(2x4) Winograd planners share (csrc/seam_wino_layout.h).

1. tests/wino_layout_check.cpp -- the header alone, no library -- built by the host compiler with -fsanitize=address,undefined and
   run: for the three kernel forms, every tile grid up to 70 x 70 and N in {1, 3, 8}, a region layout tiles the grid exactly once
   with patches inside the form's budgets, a stacked layout holds the rows, images and patch rows its blocks touch and saves blocks;
   the grids up to 35 x 35 again with images near 2 GiB, where the images of a stacked block must fit one buffer descriptor.
2. The six layout-derived queries of the C ABI, pinned on the shapes the product and the GPU parity tests run.  The values were
   recorded from the library as it was BEFORE the two planners shared one chooser (each kernel file then carried its own copy), so
   they pin that no layout, tile variant or n-tile split moved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "seam-match-rcnn_amd", "csrc")


def test_header_invariants_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wino_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "wino_layout_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe, "70"], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0 and "70 x 70 tile grids, 3 forms, N in {1, 3, 8}: 0 failures" in run.stdout
    assert "the G x image-bytes rule was not exercised" not in run.stdout


QUERIES = ("seam_wino_slot_fill_pct", "seam_wino_issue_slots", "seam_wino_tile_variant",
           "seam_wino24_issue_slots", "seam_wino24_variant", "seam_wino24_form")

# (N, H, W, C, K, pad): the six queries, in the order of QUERIES
PINNED = {
    # the 17 shapes of WINO_CASES in tests/test_gpu_wino.py
    (2, 20, 24, 64, 64, 1): (93, 8192, 1, 6144, 1, 0),
    (1, 17, 19, 128, 128, 1): (93, 6144, 1, 6144, 1, 0),
    (2, 13, 13, 256, 256, 1): (76, 16384, 1, 12288, 1, 0),
    (1, 25, 32, 256, 256, 1): (92, 28672, 1, 24576, 1, 0),
    (3, 14, 14, 256, 256, 1): (76, 24576, 1, 18432, 1, 0),
    (3, 14, 14, 256, 256, 0): (84, 16384, 1, 12288, 1, 0),
    (2, 8, 8, 256, 1024, 0): (56, 16384, 1, 24576, 1, 0),
    (1, 7, 9, 512, 512, 1): (62, 8192, 1, 12288, 1, 0),
    (1, 5, 70, 8, 32, 1): (82, 2048, 1, 1536, 1, 0),
    (1, 3, 3, 64, 32, 0): (3, 512, 1, 768, 1, 0),
    (2, 37, 41, 24, 96, 1): (95, 39936, 1, 32256, 1, 0),
    (7, 10, 10, 256, 256, 0): (87, 16384, 1, 12288, 1, 0),
    (11, 8, 8, 256, 64, 0): (77, 4096, 1, 4608, 1, 0),
    (5, 12, 12, 64, 64, 0): (78, 5120, 1, 4608, 1, 0),
    (1, 200, 200, 32, 32, 1): (99, 160256, 1, 120576, 1, 0),
    (2, 100, 50, 16, 32, 1): (97, 40960, 1, 32256, 1, 0),
    (1, 51, 35, 8, 32, 0): (94, 7168, 1, 6144, 1, 0),
    # the maps of a step at 256 channels, pad 1, for one image, a step's 80 frames and 256
    (1, 200, 200, 256, 256, 1): (99, 1286144, 2, 964608, 1, 0),
    (80, 200, 200, 256, 256, 1): (99, 102891520, 2, 77168640, 2, 1),
    (256, 200, 200, 256, 256, 1): (99, 329252864, 2, 246939648, 2, 1),
    (1, 100, 100, 256, 256, 1): (98, 323584, 1, 245760, 1, 0),
    (80, 100, 100, 256, 256, 1): (97, 26214400, 2, 19660800, 2, 1),
    (256, 100, 100, 256, 256, 1): (97, 83886080, 2, 62914560, 2, 1),
    (1, 50, 50, 256, 256, 1): (97, 81920, 1, 67584, 1, 0),
    (80, 50, 50, 256, 256, 1): (97, 6553600, 1, 5406720, 2, 1),
    (256, 50, 50, 256, 256, 1): (97, 20971520, 1, 17301504, 2, 1),
    (1, 25, 25, 256, 256, 1): (88, 24576, 1, 24576, 1, 0),
    (80, 25, 25, 256, 256, 1): (88, 1966080, 2, 1597440, 2, 1),
    (256, 25, 25, 256, 256, 1): (88, 6291456, 2, 5111808, 2, 1),
    (1, 13, 13, 256, 256, 1): (76, 8192, 1, 6144, 1, 0),
    (80, 13, 13, 256, 256, 1): (87, 573440, 1, 430080, 1, 0),
    (256, 13, 13, 256, 256, 1): (98, 1638400, 2, 1376256, 1, 0),
    # the match trunk's valid convs on 256 ROIs: 14 -> 12, 12 -> 10, 10 -> 8, and 8 -> 6 x 1024, where F(2x2) splits the n-tiles
    (256, 14, 14, 256, 256, 0): (93, 1261568, 2, 946176, 1, 0),
    (256, 12, 12, 256, 256, 0): (93, 876544, 1, 786432, 1, 0),
    (256, 10, 10, 256, 256, 0): (100, 524288, 1, 454656, 1, 0),
    (256, 8, 8, 256, 1024, 0): (83, 1409024, 2, 1474560, 1, 0),
    # refused: C not a multiple of 8, K not of 32, no image, no output pixel (both ways) ...
    (1, 8, 8, 7, 32, 1): (0, 0, 0, 0, 0, -1),
    (1, 8, 8, 8, 48, 1): (0, 0, 0, 0, 0, -1),
    (0, 8, 8, 64, 64, 1): (0, 0, 0, 0, 0, -1),
    (1, 2, 2, 64, 64, 0): (0, 0, 0, 0, 0, -1),
    (1, 1, 9, 64, 64, 0): (0, 0, 0, 0, 0, -1),
    # ... and the two grid limits, which differ: 2^24 blocks for F(2x4) (F(2x2) plans this one), 2^31 - 1 for F(2x2)
    (70000, 200, 200, 8, 2048, 1): (99, 720240640000, 2, 0, 0, -1),
    (300000, 200, 200, 8, 2048, 1): (0, 0, 0, 0, 0, -1),
}


def test_layout_queries_are_where_they_were():
    from seam_match_rcnn_amd import _native
    lib = _native.lib()
    got = {shape: tuple(int(getattr(lib, q)(*shape)) for q in QUERIES) for shape in PINNED}
    assert got == PINNED, {s: (got[s], PINNED[s]) for s in PINNED if got[s] != PINNED[s]}
    # every query has a shape it refuses and the tile variants, n-tile forms and kernels all occur
    for i, refused in enumerate((0, 0, 0, 0, 0, -1)):
        assert any(v[i] == refused for v in PINNED.values())
    assert {v[2] for v in PINNED.values()} == {0, 1, 2} == {v[4] for v in PINNED.values()} and {v[5] for v in PINNED.values()} == {-1, 0, 1}
