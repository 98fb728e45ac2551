"""CPU: the forced n-tile split of conv3x3_wino24sx (``seam_conv3x3_wino24sx_set_nsplit`` / ``_get_nsplit``, csrc/seam_wino24sx.hip) --
it defaults to the rule, refuses values that are not the rule (0) or a divisor of the eight XCDs, and does not move the tile count
``ops.w24sx_map_ok`` compares with W24SX_MIN_BLOCKS, so no route depends on it.  The setting is the launcher's own entry point and not a
row of the ``seam_set_option`` table, whose length ``tests/test_abi_and_host.py`` pins at ten.  No GPU."""
import pytest


@pytest.fixture()
def lib():
    from seam_match_rcnn_amd import _native
    L = _native.lib()
    before = L.seam_conv3x3_wino24sx_get_nsplit()
    yield L
    assert L.seam_conv3x3_wino24sx_set_nsplit(before) == 0


def test_setting_is_exported_and_defaults_to_the_rule(lib):
    from seam_match_rcnn_amd import _native
    assert "seam_conv3x3_wino24sx_set_nsplit" in _native.SIGNATURES and "seam_conv3x3_wino24sx_get_nsplit" in _native.SIGNATURES
    assert lib.seam_conv3x3_wino24sx_get_nsplit() == 0
    # the selector table is as it was: the setting is not reachable through it
    names = [lib.seam_option_name(i).decode() for i in range(lib.seam_option_count())]
    assert not any("W24SX" in n for n in names) and lib.seam_set_option(b"SEAM_W24SX_NSPLIT", 2) != 0


def test_unknown_values_are_refused(lib):
    for v in (0, 1, 2, 4, 8):
        assert lib.seam_conv3x3_wino24sx_set_nsplit(v) == 0 and lib.seam_conv3x3_wino24sx_get_nsplit() == v
    for v in (-1, 3, 5, 6, 7, 16, 256):
        assert lib.seam_conv3x3_wino24sx_set_nsplit(v) != 0
        assert lib.seam_conv3x3_wino24sx_get_nsplit() == 8          # a refused value leaves the setting as it was


# (n, h, w, c, k, pad) -> tiles: one image of the routed maps (tests/test_w24sx_host.py), batches whose patch blocks do not divide
# by the partitions, one n-tile (k = 64), and an unsupported shape
SHAPES = [((1, 200, 200, 256, 256, 1), 628), ((1, 100, 100, 256, 256, 1), 160), ((1, 50, 50, 256, 256, 1), 44), ((1, 14, 14, 256, 256, 1), 4),
          ((1, 8, 8, 64, 256, 1), 4), ((3, 100, 100, 256, 256, 1), 480), ((5, 14, 14, 64, 256, 0), 12), ((2, 9, 11, 64, 64, 1), None),
          ((80, 200, 200, 256, 256, 1), 50240), ((1, 8, 8, 96, 64, 1), 0)]


def test_block_count_does_not_depend_on_the_setting(lib):
    for shape, want in SHAPES:
        assert lib.seam_conv3x3_wino24sx_set_nsplit(1) == 0
        base = lib.seam_conv3x3_wino24sx_blocks(*shape)
        assert want is None or base == want, (shape, base)
        for v in (0, 2, 4, 8):
            assert lib.seam_conv3x3_wino24sx_set_nsplit(v) == 0
            assert lib.seam_conv3x3_wino24sx_blocks(*shape) == base, (shape, v)
            assert lib.seam_conv3x3_wino24sx_supported(*shape, 1) == (1 if base else 0)


def test_no_route_moves(lib):
    import seam_match_rcnn_amd.ops as ops
    maps = [(200, 200, 256, 256, 1), (100, 100, 256, 256, 1), (50, 50, 256, 256, 1), (100, 100, 128, 128, 1), (14, 14, 256, 256, 0)]
    want = None
    for v in (1, 0, 2, 4, 8):
        assert lib.seam_conv3x3_wino24sx_set_nsplit(v) == 0
        ops._WINO24.clear()
        got = [ops.w24sx_map_ok(*m) for m in maps]
        want = got if want is None else want
        assert got == want, (v, got, want)
    ops._WINO24.clear()
