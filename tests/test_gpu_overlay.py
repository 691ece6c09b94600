"""GPU: the overlay post-processing stage (csrc/overlay.hip, seg_amd/overlay.py) against its numpy
restatement (tests/overlay_ref.py), bit for bit: the 5x5 close, the 8-connected labels (smallest linear
index), the largest component, the ordered box list, the blend and outlines, `Overlay`, the `Predictor`
option and `overlay_predictions`.  Nothing here has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as ref  # noqa: E402
from overlay_cases import border_masks, class_mask, frame, mask_cases, random_masks  # noqa: E402

from oracle import cvresize  # noqa: E402
from seg_amd import Overlay, UNet, deterministic_init, overlay_predictions  # noqa: E402
from seg_amd.infer import Predictor  # noqa: E402
from seg_amd._lib import call, query  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
# host functions of the library (built by __graft_entry__.build())
TH, TW = query("seg_cc_tile_h"), query("seg_cc_tile_w")
_REF_LABELS = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def ref_labels(name, m):
    """The helper's labels of a case, computed once and shared (read-only)."""
    if name not in _REF_LABELS:
        lab = ref.label8(m)
        lab.setflags(write=False)
        _REF_LABELS[name] = lab
    return _REF_LABELS[name]


def gpu_close(cls, class_id):
    d = torch.from_numpy(cls).to(DEV)
    out = torch.full(cls.shape, 77, device=DEV, dtype=torch.uint8)
    call("seg_morph_close5", d.data_ptr(), cls.shape[0], cls.shape[1], class_id, out.data_ptr(), stream())
    return out.cpu().numpy()


def gpu_labels(m):
    d = torch.from_numpy(np.ascontiguousarray(m)).to(DEV)
    lab = torch.full(m.shape, -7, device=DEV, dtype=torch.int32)
    call("seg_cc_label8", d.data_ptr(), m.shape[0], m.shape[1], lab.data_ptr(), stream())
    return lab


def gpu_largest(lab):
    H, W = lab.shape
    n = query("seg_overlay_workspace_bytes", H, W, 1)
    work = torch.full((n,), 0x5A, device=DEV, dtype=torch.uint8)  # the workspace needs no clearing
    out = torch.full((2,), -9, device=DEV, dtype=torch.int32)
    call("seg_cc_largest", lab.data_ptr(), H, W, out.data_ptr(), work.data_ptr(), n, stream())
    return tuple(out.cpu().tolist())


def gpu_boxes(lab, min_area, max_boxes):
    H, W = lab.shape
    n = query("seg_overlay_workspace_bytes", H, W, max_boxes)
    work = torch.full((n,), 0x5A, device=DEV, dtype=torch.uint8)
    boxes = torch.full((max_boxes, 5), -9, device=DEV, dtype=torch.int32)
    count = torch.full((2,), -9, device=DEV, dtype=torch.int32)
    call("seg_cc_boxes", lab.data_ptr(), H, W, min_area, max_boxes, boxes.data_ptr(), count.data_ptr(),
         work.data_ptr(), n, stream())
    stored, passed = count.cpu().tolist()
    rows = boxes.cpu().numpy()
    assert np.all(rows[stored:] == -9)  # nothing written past the stored boxes
    return rows[:stored].tolist(), (stored, passed)


CLOSE_CASES = random_masks(TH, TW) + border_masks(TH, TW)


@pytest.mark.parametrize("name,m", CLOSE_CASES, ids=[c[0] for c in CLOSE_CASES])
def test_close(name, m):
    # class 1 where the mask is set, other class ids elsewhere: the kernel compares with the class id
    g = np.random.Generator(np.random.PCG64(5))
    cls = np.where(m == 1, 1, g.choice(np.array([0, 2, 3, 255], np.uint8), size=m.shape)).astype(np.uint8)
    np.testing.assert_array_equal(gpu_close(cls, 1), ref.close5(m))


def test_close_other_class_id():
    _, m = CLOSE_CASES[10]
    cls = np.where(m == 1, 7, 1).astype(np.uint8)
    np.testing.assert_array_equal(gpu_close(cls, 7), ref.close5(m))


LABEL_CASES = mask_cases(TH, TW)


@pytest.mark.parametrize("name,m", LABEL_CASES, ids=[c[0] for c in LABEL_CASES])
def test_labels_largest_boxes(name, m):
    want = ref_labels(name, m)
    lab = gpu_labels(m * 3)  # any non-zero value is foreground
    np.testing.assert_array_equal(lab.cpu().numpy(), want)
    assert gpu_largest(lab) == ref.largest(want)
    for min_area, max_boxes in ((0, 64), (2, 5)):
        rows, count = gpu_boxes(lab, min_area, max_boxes)
        wrows, wcount = ref.boxes(want, min_area, max_boxes)
        assert count == wcount
        assert rows == wrows


def blobs(H, W, rects):
    m = np.zeros((H, W), np.uint8)
    for y, x, h, w in rects:
        m[y:y + h, x:x + w] = 1
    return m


def test_largest_tie_goes_to_the_raster_first():
    # two 3x4 blobs: the second starts on an earlier column but a later row -> the first wins
    m = blobs(TH + 9, TW + 9, [(2, TW - 2, 3, 4), (TH + 1, 1, 4, 3)])
    lab = gpu_labels(m)
    assert gpu_largest(lab) == (2 * (TW + 9) + TW - 2, 12) == ref.largest(ref.label8(m))
    # and the other way round in memory order: a larger blob later still beats an earlier smaller one
    m = blobs(TH + 9, TW + 9, [(2, TW - 2, 3, 4), (TH + 1, 1, 4, 4)])
    assert gpu_largest(gpu_labels(m)) == ((TH + 1) * (TW + 9) + 1, 16)


def test_no_foreground():
    m = np.zeros((TH + 3, TW + 5), np.uint8)
    lab = gpu_labels(m)
    assert np.all(lab.cpu().numpy() == -1)
    assert gpu_largest(lab) == (-1, 0)
    assert gpu_boxes(lab, 0, 8) == ([], (0, 0))


def test_box_cap_keeps_the_first_by_label():
    rects = [(1 + 4 * (i // 5), 2 + 14 * (i % 5), 2, 3 + i % 3) for i in range(10)]
    m = blobs(TH + 9, TW + 9, rects)
    want = ref.label8(m)
    rows, count = gpu_boxes(gpu_labels(m), 0, 4)
    assert count == (4, 10)
    assert rows == ref.boxes(want, 0, 4)[0] == [[x, y, w, h, w * h] for y, x, h, w in rects[:4]]


def test_min_area_is_exclusive():
    m = blobs(TH + 9, TW + 20, [(1, 1, 3, 4), (TH, TW - 1, 1, 13)])  # areas 12 and 13
    lab = gpu_labels(m)
    assert gpu_boxes(lab, 12, 8) == ([[TW - 1, TH, 13, 1, 13]], (1, 1))
    assert gpu_boxes(lab, 11, 8)[1] == (2, 2)
    assert gpu_boxes(lab, 13, 8) == ([], (0, 0))


def test_boxes_over_many_blocks():
    """More than 1024 blocks of 256 pixels: the one-block scan of the box list walks several counts per
    thread (a 720x1280 frame has 3600).  Sparse blobs keep the helper's flood fill quick."""
    H, W = 600, 520
    g = np.random.Generator(np.random.PCG64(8))
    rects = [(int(g.integers(0, H - 12)), int(g.integers(0, W - 12)), int(g.integers(1, 12)), int(g.integers(1, 12)))
             for _ in range(90)] + [(H - 3, W - 5, 3, 5), (0, 0, 2, 2)]
    m = blobs(H, W, rects)
    want = ref.label8(m)
    lab = gpu_labels(m)
    np.testing.assert_array_equal(lab.cpu().numpy(), want)
    assert gpu_largest(lab) == ref.largest(want)
    for min_area, max_boxes in ((0, 128), (20, 16)):
        assert gpu_boxes(lab, min_area, max_boxes) == ref.boxes(want, min_area, max_boxes)
    np.testing.assert_array_equal(gpu_close(m, 1), ref.close5(m))


def run_overlay(ov, f, cls):
    ov.launch(torch.from_numpy(f).to(DEV), torch.from_numpy(cls).to(DEV))
    return ov.result.cpu().numpy(), ov.cleaned.cpu().numpy(), ov.boxes(), ov.detected_objects()


def check_overlay(got, want):
    np.testing.assert_array_equal(got[1], want[1])  # cleaned
    assert got[2] == want[2]                        # boxes
    assert got[3] == want[3]                        # detected_objects
    np.testing.assert_array_equal(got[0], want[0])  # result


CUSTOM_MAP = {0: [1, 2, 3], 1: [9, 200, 9], 2: [200, 100, 50], 5: [7, 7, 7]}


@pytest.mark.parametrize("hw", [(90, 160), (72, 131)])
@pytest.mark.parametrize("kwargs", [{}, {"draw_boxes": False}, {"color_map": CUSTOM_MAP}, {"min_area": 30},
                                    {"min_area": 0, "max_boxes": 2}])
def test_overlay_stage(hw, kwargs):
    H, W = hw
    f, cls = frame(H, W, seed=H), class_mask(H, W, seed=W)
    want = ref.overlay(f, cls, **kwargs)
    got = run_overlay(Overlay(hw, **kwargs), f, cls)
    check_overlay(got, want)
    if not kwargs:
        # the scene is what the test is about: the fill joined the two road pieces over the cars in the gap,
        # the second road blob is not part of it, two cars pass, one box touches the frame's corner
        assert (cls == 2).sum() > (want[1] == 2).sum() and want[3] == {"cars": 2}
        assert any(b["x"] + b["w"] == W and b["y"] + b["h"] == H for b in want[2])
        assert not np.array_equal(want[0], ref.overlay(f, cls, draw_boxes=False)[0])
        assert (want[1] == 11).any()


def test_overlay_reuses_its_buffers_across_frames():
    """A second, different frame through the same Overlay gives its own answer (no stale workspace state),
    and a frame without road or cars gives none."""
    H, W = 72, 131
    ov = Overlay((H, W), min_area=30)
    for seed in (1, 2, 1):
        f, cls = frame(H, W, seed), class_mask(H, W, seed)
        if seed == 2:
            cls = np.roll(cls, 17, axis=1)
        check_overlay(run_overlay(ov, f, cls), ref.overlay(f, cls, min_area=30))
    f, cls = frame(H, W, 3), np.full((H, W), 4, np.uint8)
    got = run_overlay(ov, f, cls)
    check_overlay(got, ref.overlay(f, cls, min_area=30))
    assert got[2] == [] and got[3] == {"cars": 0}


def test_predictor_overlay():
    size, (fh, fw) = (64, 32), (22, 40)
    model = deterministic_init(UNet(10, 16), seed=11, random_running_stats=True).to(DEV)
    kw = dict(min_area=3, max_boxes=8)
    g = Predictor(model, frame_hw=(fh, fw), target_size=size, graph=True, overlay=Overlay((fh, fw), **kw))
    e = Predictor(model, frame_hw=(fh, fw), target_size=size, graph=False, overlay=Overlay((fh, fw), **kw))
    plain = Predictor(model, frame_hw=(fh, fw), target_size=size, graph=True)
    answers = []
    for seed in (3, 4):
        f = frame(fh, fw, seed)
        res, det = g.annotate(f)
        res = res.cpu().numpy()
        mask = g.mask.cpu().numpy()
        want = ref.overlay(f, mask, **kw)
        check_overlay((res, g.overlay.cleaned.cpu().numpy(), g.overlay.boxes(), det), want)
        # the eager launch sequence agrees bitwise with the graph
        res_e, det_e = e.annotate(f)
        assert np.array_equal(res_e.cpu().numpy(), res) and det_e == det
        assert torch.equal(e.overlay.cleaned, g.overlay.cleaned) and e.overlay.boxes() == g.overlay.boxes()
        # a second replay on the same frame agrees bitwise
        g.step()
        assert np.array_equal(g.overlay.result.cpu().numpy(), res) and g.overlay.detected_objects() == det
        # without the overlay the mask is bitwise the same, and __call__ still returns the mask
        assert np.array_equal(plain(f).cpu().numpy(), mask)
        assert g(f) is g.mask
        answers.append(res)
    assert not np.array_equal(answers[0], answers[1])
    with pytest.raises(RuntimeError):
        plain.annotate(frame(fh, fw, 3))


def test_overlay_predictions_numpy_frame():
    fh, fw = 45, 80
    g = torch.Generator().manual_seed(0)
    # smooth logits so that road (1) and car (2) regions of some size exist
    logits = torch.nn.functional.interpolate(torch.randn(1, 4, 4, 8, generator=g), size=(32, 64), mode="bilinear")
    f = frame(fh, fw, 9)
    res, det = overlay_predictions(f, logits.to(DEV), min_area=20)
    assert isinstance(res, np.ndarray) and res.dtype == np.uint8
    mask = cvresize.class_mask(logits.numpy(), (fh, fw))
    want = ref.overlay(f, mask, min_area=20)
    np.testing.assert_array_equal(res, want[0])
    assert det == want[3]
    # a tensor frame gives a tensor on the GPU
    res_t, det_t = overlay_predictions(torch.from_numpy(f).to(DEV), logits.to(DEV), min_area=20)
    assert res_t.is_cuda and np.array_equal(res_t.cpu().numpy(), res) and det_t == det
