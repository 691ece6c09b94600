"""Time the overlay post-processing stage (seg_amd/overlay.py) on the GPU.

    python tools/overlay_time.py [--frame 720 1280] [--replays 500] [--rounds 7] [--out FILE.json]

Device-event timing over hipGraph replays, the two variants of a comparison alternated in one process:
  * the fp16 `Predictor` frame with overlay=False and overlay=True, and their difference;
  * the stage alone (`Overlay` in a graph of its own) on a synthetic road scene and on the model's own mask;
  * each op-level entry (seg_morph_close5, seg_cc_label8, ...) in a graph of its own on the scene: the split.
Prints one JSON document (and writes it to --out).  Needs an MI355X: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "team02-objectdetection_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from seg_amd import MobileNetV2UNet, Overlay, Predictor, deterministic_init  # noqa: E402
from seg_amd._lib import call, query  # noqa: E402

DEV = "cuda"
# launches of seg_overlay_frame (csrc/overlay.hip): close 1, labels 3, areas 1, largest 1, fill 1,
# car labels 3, car areas + boxes 1, box list 3, blend 1, outlines 1
STAGE_LAUNCHES = 16


def video_frame(h, w, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.meshgrid(np.linspace(0, 6, h), np.linspace(0, 9, w), indexing="ij")
    base = 127.5 + 100 * np.sin(yy)[..., None] * np.cos(xx[..., None] + np.arange(3))
    return np.clip(base + g.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def road_scene(h, w, seed):
    """A class mask like a driving frame: a road trapezoid with a 3-column gap, a detached road patch, six
    cars, sidewalks, and speckle of road / car pixels (thousands of one-pixel components)."""
    g = np.random.Generator(np.random.PCG64(seed))
    cls = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    t = (yy - h // 2) / (h / 2)
    road = (yy >= h // 2) & (xx > w / 2 - 0.1 * w - t * 0.35 * w) & (xx < w / 2 + 0.1 * w + t * 0.35 * w)
    cls[(yy >= h // 2) & ~road] = 6
    cls[road] = 1
    cls[h // 2:, w // 2:w // 2 + 3] = 0
    cls[h // 2 - 40:h // 2 - 20, w // 8:w // 8 + 90] = 1
    for i in range(6):
        y, x = h // 2 + 20 + 45 * i, w // 4 + 120 * i
        cls[y:y + 28 + 6 * i, x:x + 44 + 10 * i] = 2
    speck = g.random((h, w))
    cls[speck < 0.002] = 1
    cls[speck > 0.998] = 2
    return cls


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def time_alternating(replayers, replays, rounds):
    """{name: [ms per replay, one value per round]}: the variants alternate inside every round."""
    for fn in replayers.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in replayers}
    for _ in range(rounds):
        for name, fn in replayers.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / replays)
    return out


def summary(ms):
    return {"median_us": round(1e3 * statistics.median(ms), 2), "min_us": round(1e3 * min(ms), 2),
            "max_us": round(1e3 * max(ms), 2)}


def op_graphs(ov, frame, cls):
    """One graph per op-level entry, fed with the buffers the whole stage left behind."""
    H, W = ov.Hf, ov.Wf
    s = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    closed = torch.empty((H, W), device=DEV, dtype=torch.uint8)
    labels = torch.empty((H, W), device=DEV, dtype=torch.int32)
    car = (ov.cleaned == 2).to(torch.uint8)
    car_labels = torch.empty((H, W), device=DEV, dtype=torch.int32)
    out2 = torch.zeros(2, device=DEV, dtype=torch.int32)
    boxes = torch.zeros((ov.max_boxes, 5), device=DEV, dtype=torch.int32)
    count = torch.zeros(2, device=DEV, dtype=torch.int32)
    res = torch.empty_like(ov.result)
    wp, wn = ov.work.data_ptr(), ov.work.numel()
    ops = {
        "seg_morph_close5 (1 launch)": lambda: call("seg_morph_close5", cls.data_ptr(), H, W, 1, closed.data_ptr(), s()),
        "seg_cc_label8 road (3)": lambda: call("seg_cc_label8", closed.data_ptr(), H, W, labels.data_ptr(), s()),
        "seg_cc_largest (4: reset, areas, max, decode)": lambda: call("seg_cc_largest", labels.data_ptr(), H, W,
                                                                      out2.data_ptr(), wp, wn, s()),
        "seg_cc_label8 cars (3)": lambda: call("seg_cc_label8", car.data_ptr(), H, W, car_labels.data_ptr(), s()),
        "seg_cc_boxes (5: reset, areas + boxes, count, scan, write)": lambda: call(
            "seg_cc_boxes", car_labels.data_ptr(), H, W, ov.min_area, ov.max_boxes, boxes.data_ptr(), count.data_ptr(),
            wp, wn, s()),
        "seg_overlay_blend (1)": lambda: call("seg_overlay_blend", frame.data_ptr(), ov.cleaned.data_ptr(), H, W,
                                              ov.table.data_ptr(), ov.ncolors, res.data_ptr(), s()),
        "seg_overlay_outline (1)": lambda: call("seg_overlay_outline", frame.data_ptr(), H, W, boxes.data_ptr(),
                                                count.data_ptr(), ov.max_boxes, res.data_ptr(), s()),
    }
    graphs = {}
    for name, fn in ops.items():  # in order: each op's input is the previous op's output
        graphs[name] = graph_of(fn)
        graphs[name].replay()
    torch.cuda.synchronize()
    return graphs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, nargs=2, default=(720, 1280))
    ap.add_argument("--replays", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_time.py needs an MI355X")
    H, W = a.frame
    model = deterministic_init(MobileNetV2UNet(10), seed=11, random_running_stats=True).to(DEV)
    f = video_frame(H, W, 3)
    plain = Predictor(model, frame_hw=(H, W), math="f16")
    full = Predictor(model, frame_hw=(H, W), math="f16", overlay=True)
    plain(f)
    full(f)
    torch.cuda.synchronize()
    assert torch.equal(plain.mask, full.mask)
    doc = {"frame": [H, W], "math": "f16", "replays": a.replays, "rounds": a.rounds,
           "stage_launches": STAGE_LAUNCHES}
    t = time_alternating({"overlay=False": plain.step, "overlay=True": full.step}, a.replays, a.rounds)
    doc["predictor_frame"] = {k: summary(v) for k, v in t.items()}
    doc["predictor_frame"]["difference_of_medians_us"] = round(
        doc["predictor_frame"]["overlay=True"]["median_us"] - doc["predictor_frame"]["overlay=False"]["median_us"], 2)
    mask = full.mask.clone()
    doc["model_mask"] = {"road_pixels": int((mask == 1).sum()), "car_pixels": int((mask == 2).sum()),
                         "cars": full.overlay.detected_objects()["cars"]}

    fd = torch.from_numpy(f).to(DEV)
    scene = torch.from_numpy(road_scene(H, W, 5)).to(DEV)
    ov_scene, ov_model = Overlay((H, W)), Overlay((H, W))
    g_scene = graph_of(lambda: ov_scene.launch(fd, scene))
    g_model = graph_of(lambda: ov_model.launch(fd, mask))
    t = time_alternating({"road scene": g_scene.replay, "model's mask": g_model.replay}, a.replays, a.rounds)
    doc["stage_alone"] = {k: summary(v) for k, v in t.items()}
    doc["road_scene"] = {"road_pixels": int((scene == 1).sum()), "car_pixels": int((scene == 2).sum()),
                         "cars": ov_scene.detected_objects()["cars"], "boxes_stored": len(ov_scene.boxes())}

    graphs = op_graphs(ov_scene, fd, scene)
    t = time_alternating({k: g.replay for k, g in graphs.items()}, a.replays, a.rounds)
    doc["ops_on_road_scene"] = {k: summary(v) for k, v in t.items()}
    doc["ops_on_road_scene"]["sum_of_medians_us"] = round(sum(summary(v)["median_us"] for v in t.values()), 2)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
