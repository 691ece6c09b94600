"""CPU: the numpy restatement of the overlay stage (tests/overlay_ref.py) against scipy.ndimage on
the masks the GPU tests use, and the argument validation of the new C-ABI entries (no launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as ref  # noqa: E402
from overlay_cases import mask_cases  # noqa: E402

from seg_amd import _lib  # noqa: E402
from seg_amd.build import build  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cases(lib):
    return mask_cases(lib.seg_cc_tile_h(), lib.seg_cc_tile_w())


def test_tile_queries(lib):
    assert lib.seg_cc_tile_h() > 0 and lib.seg_cc_tile_w() > 0


def test_close_matches_scipy(cases):
    ndi = pytest.importorskip("scipy.ndimage")
    k = np.ones((5, 5), bool)
    for name, m in cases:
        want = ndi.binary_erosion(ndi.binary_dilation(m.astype(bool), k, border_value=0), k, border_value=1)
        assert np.array_equal(ref.close5(m), want.astype(np.uint8)), name


def test_labels_areas_boxes_match_scipy(cases):
    ndi = pytest.importorskip("scipy.ndimage")
    for name, m in cases:
        H, W = m.shape
        lab, n = ndi.label(m, structure=np.ones((3, 3)))
        idx = np.arange(H * W).reshape(H, W)
        roots = ndi.minimum(idx, lab, np.arange(1, n + 1)).astype(np.int64) if n else np.zeros(0, np.int64)
        want = np.where(lab > 0, np.concatenate([[-1], roots])[lab], -1).astype(np.int32)
        got = ref.label8(m)
        assert np.array_equal(got, want), name
        areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        comps = ref.components(got)
        assert [c[0] for c in comps] == sorted(roots.tolist()), name
        by_root = {c[0]: c for c in comps}
        for i, sl in enumerate(ndi.find_objects(lab)):
            _, x, y, w, h, area = by_root[int(roots[i])]
            assert (x, y, w, h, area) == (sl[1].start, sl[0].start, sl[1].stop - sl[1].start,
                                          sl[0].stop - sl[0].start, int(areas[i])), name
        if n:
            # 1 + np.argmax(stats[1:, AREA]) under raster-ordered labels: the first maximum
            assert ref.largest(got) == (int(roots[int(np.argmax(areas))]), int(areas.max())), name
        else:
            assert ref.largest(got) == (-1, 0), name


def test_blend_values():
    a = np.array([5, 0, 255, 10, 0], np.uint8)
    b = np.array([5, 255, 255, 0, 0], np.uint8)
    assert ref.blend(a, b).tolist() == [5, 102, 255, 6, 0]
    # every sum of the two float32 products stays within 0..255 after rounding
    aa, bb = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    s = aa.astype(np.float32) * np.float32(0.6) + bb.astype(np.float32) * np.float32(0.4)
    assert 0 <= np.rint(s).min() and np.rint(s).max() <= 255


def test_new_entries_reject_bad_arguments(lib):
    """hipErrorInvalidValue (1) before any launch: runs without a GPU."""
    H, W, MB = 8, 16, 4
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    p += -p % 16
    need = lib.seg_overlay_workspace_bytes(H, W, MB)
    assert 0 < need < (1 << 16) - 16
    # null buffers with non-zero sizes
    assert lib.seg_morph_close5(None, H, W, 1, None, None) == 1
    assert lib.seg_cc_label8(None, H, W, None, None) == 1
    assert lib.seg_cc_largest(None, H, W, None, None, need, None) == 1
    assert lib.seg_cc_boxes(None, H, W, 0, MB, None, None, None, need, None) == 1
    assert lib.seg_overlay_blend(None, None, H, W, None, 10, None, None) == 1
    assert lib.seg_overlay_outline(None, H, W, None, None, MB, None, None) == 1
    assert lib.seg_overlay_frame(None, None, H, W, None, 10, 300, MB, 1, None, None, None, None, None, need, None) == 1
    # max_boxes <= 0
    for mb in (0, -1):
        assert lib.seg_overlay_workspace_bytes(H, W, mb) == 0
        assert lib.seg_cc_boxes(p, H, W, 0, mb, p, p, p, need, None) == 1
        assert lib.seg_overlay_outline(p, H, W, p, p, mb, p, None) == 1
        assert lib.seg_overlay_frame(p, p, H, W, p, 10, 300, mb, 1, p, p, p, p, p, need, None) == 1
    # a workspace smaller than the query
    assert lib.seg_cc_largest(p, H, W, p, p, need - 1, None) == 1
    assert lib.seg_cc_boxes(p, H, W, 0, MB, p, p, p, need - 1, None) == 1
    assert lib.seg_overlay_frame(p, p, H, W, p, 10, 300, MB, 1, p, p, p, p, p, need - 1, None) == 1
    # Hf * Wf >= 2^31, and empty images
    for h, w in ((65536, 32768), (0, 16), (8, -1)):
        assert lib.seg_overlay_workspace_bytes(h, w, MB) == 0
        assert lib.seg_morph_close5(p, h, w, 1, p, None) == 1
        assert lib.seg_cc_label8(p, h, w, p, None) == 1
        assert lib.seg_cc_largest(p, h, w, p, p, 1 << 40, None) == 1
        assert lib.seg_cc_boxes(p, h, w, 0, MB, p, p, p, 1 << 40, None) == 1
        assert lib.seg_overlay_blend(p, p, h, w, p, 10, p, None) == 1
        assert lib.seg_overlay_outline(p, h, w, p, p, MB, p, None) == 1
        assert lib.seg_overlay_frame(p, p, h, w, p, 10, 300, MB, 1, p, p, p, p, p, 1 << 40, None) == 1
    # a class id or a colour count outside a byte
    assert lib.seg_morph_close5(p, H, W, 256, p, None) == 1
    assert lib.seg_overlay_blend(p, p, H, W, p, 257, p, None) == 1


def test_overlay_predictions_needs_cuda_logits():
    import torch
    from seg_amd import overlay_predictions
    with pytest.raises(RuntimeError, match="HIP path only"):
        overlay_predictions(np.zeros((8, 8, 3), np.uint8), torch.zeros(1, 10, 4, 4))


def test_color_table():
    from seg_amd.overlay import COLOR_MAP, color_table
    assert COLOR_MAP == ref.COLOR_MAP
    t = color_table({0: [1, 2, 3], 2: [4, 5, 6]})
    assert t.tolist() == [[1, 2, 3, 1], [0, 0, 0, 0], [4, 5, 6, 1]]
    with pytest.raises(ValueError):
        color_table({256: [0, 0, 0]})
