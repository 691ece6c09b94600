"""GPU replacement for the post-processing of the reference's overlay_predictions
(inference.py:72-146): everything the reference does with OpenCV between the class
mask and the frame it shows.

    road = (cls == 1)                      5x5 morphological close       seg_morph_close5
    8-connected components, keep largest   cleaned[largest] = 1          seg_cc_label8 / seg_cc_largest
    overlay = color_map[cleaned]           (a class outside the table keeps the frame's pixel)
    car blobs of cleaned == 2              boxes with area > min_area    seg_cc_boxes
    result = 0.6 * image + 0.4 * overlay   cv2.addWeighted, uint8        seg_overlay_blend
    2-pixel green box outlines                                           seg_overlay_outline

`Overlay` owns the static buffers and runs the stage as one chain of launches on one
stream (seg_overlay_frame), so `Predictor(..., overlay=True)` captures it into its
graph.  `overlay_predictions` mirrors the reference function.  Differences from the
reference: `area` is the blob's pixel count, not cv2.contourArea; a
blob inside a hole of another blob is kept; the outline is our own 2-pixel rule; the
distance text is not drawn (the distance is in `boxes()`).
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, query

# inference.py:50-61, applied as written to the BGR frame
COLOR_MAP = {
    0: [0, 0, 0],         # Background
    1: [0, 255, 0],       # Road
    2: [255, 0, 0],       # Car
    3: [250, 170, 30],    # Traffic Light
    4: [220, 220, 0],     # Traffic Sign
    5: [220, 20, 60],     # Person
    6: [244, 35, 232],    # Sidewalks
    7: [0, 0, 70],        # Truck
    8: [0, 60, 100],      # Bus
    9: [0, 0, 230],       # Motorcycle
}


def color_table(color_map) -> np.ndarray:
    """[n][4] uint8 rows (c0, c1, c2, listed) of a {class: colour} dict or a sequence of colours."""
    items = dict(color_map) if isinstance(color_map, dict) else dict(enumerate(color_map))
    if any(not 0 <= int(k) <= 255 for k in items):
        raise ValueError("color_map classes must lie in 0..255")
    n = max((int(k) for k in items), default=-1) + 1
    table = np.zeros((n, 4), np.uint8)
    for k, c in items.items():
        c = [int(v) for v in c]
        if len(c) != 3 or any(not 0 <= v <= 255 for v in c):
            raise ValueError(f"color_map[{k}] must be three values in 0..255, got {c}")
        table[int(k)] = (*c, 1)
    return table


class Overlay:
    """The overlay stage over static buffers.

    ov = Overlay((720, 1280))
    ov.launch(frame, mask)           # uint8 [Hf,Wf,3] BGR frame, uint8 [Hf,Wf] class mask, both on the GPU
    ov.result, ov.cleaned            # uint8 [Hf,Wf,3] blended frame, uint8 [Hf,Wf] cleaned mask
    ov.boxes()                       # [{x, y, w, h, area, distance}], one small D2H copy
    ov.detected_objects()            # {'cars': n}: every blob that passed min_area, stored or not
    """

    def __init__(self, frame_hw, color_map=COLOR_MAP, min_area: int = 300, max_boxes: int = 64,
                 draw_boxes: bool = True, device="cuda"):
        self.Hf, self.Wf = int(frame_hw[0]), int(frame_hw[1])
        self.min_area, self.max_boxes, self.draw_boxes = int(min_area), int(max_boxes), bool(draw_boxes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Overlay runs on the MI355X HIP path only; use device 'cuda'")
        nbytes = query("seg_overlay_workspace_bytes", self.Hf, self.Wf, self.max_boxes)
        if nbytes <= 0:
            raise ValueError(f"unsupported overlay size: frame {self.Hf}x{self.Wf}, max_boxes {self.max_boxes}")
        table = color_table(color_map)
        self.ncolors = table.shape[0]
        self.table = torch.from_numpy(table).to(self.device) if self.ncolors else None
        self.work = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        self.result = torch.zeros((self.Hf, self.Wf, 3), device=self.device, dtype=torch.uint8)
        self.cleaned = torch.zeros((self.Hf, self.Wf), device=self.device, dtype=torch.uint8)
        # count[2] (padded to 4) then boxes[max_boxes][5], so one copy fetches both
        self._out = torch.zeros(4 + 5 * self.max_boxes, device=self.device, dtype=torch.int32)

    def _check(self, t, shape, what):
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_cuda or \
                not t.is_contiguous():
            raise ValueError(f"expected a contiguous uint8 CUDA {what} of shape {shape}")

    def launch(self, frame, mask, stream=None):
        """Run the stage on `stream` (a raw stream handle; default: torch's current stream)."""
        self._check(frame, (self.Hf, self.Wf, 3), "frame")
        self._check(mask, (self.Hf, self.Wf), "class mask")
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        out = self._out.data_ptr()
        call("seg_overlay_frame", frame.data_ptr(), mask.data_ptr(), self.Hf, self.Wf,
             self.table.data_ptr() if self.table is not None else None, self.ncolors, self.min_area, self.max_boxes,
             int(self.draw_boxes), self.cleaned.data_ptr(), self.result.data_ptr(), out + 16, out, self.work.data_ptr(),
             self.work.numel(), stream)
        return self.result

    def _fetch(self):
        out = self._out.cpu().numpy()
        return int(out[0]), int(out[1]), out[4:].reshape(self.max_boxes, 5)

    def boxes(self):
        stored, _, rows = self._fetch()
        res = []
        for x, y, w, h, area in rows[:stored].tolist():
            # inference.py:133-135, in double
            res.append({"x": x, "y": y, "w": w, "h": h, "area": area,
                        "distance": int(50 * (1.0 - (y + h) / self.Hf))})
        return res

    def detected_objects(self):
        return {"cars": self._fetch()[1]}


def overlay_predictions(image, prediction, show_debug=True, **overlay_kwargs):
    """inference.py:48-146 on the GPU: (result, detected_objects) for a BGR frame and the
    model's [1, C, h, w] logits.  A numpy frame gives a numpy result, a tensor a CUDA tensor.
    `show_debug` is accepted for the reference's signature (it is unused there too)."""
    if not torch.is_tensor(prediction) or not prediction.is_cuda:
        raise RuntimeError("overlay_predictions runs on the MI355X HIP path only; move the logits to 'cuda' first")
    if prediction.dim() != 4 or prediction.shape[0] != 1:
        raise ValueError(f"expected [1, C, h, w] logits, got {tuple(prediction.shape)}")
    from .infer import _frame_tensor
    dev = prediction.device
    f = _frame_tensor(image, dev)
    Hf, Wf = f.shape[0], f.shape[1]
    _, cls = torch.max(prediction, dim=1)  # inference.py:64
    cls = cls[0].to(torch.uint8).contiguous()
    h, w = cls.shape
    mask = torch.empty((Hf, Wf), device=dev, dtype=torch.uint8)
    s = torch.cuda.current_stream(dev).cuda_stream
    call("seg_resize_u8", cls.data_ptr(), 1, h, w, w, mask.data_ptr(), Hf, Wf, 1, None, s)  # inference.py:68-70
    ov = Overlay((Hf, Wf), device=dev, **overlay_kwargs)
    result = ov.launch(f, mask, s)
    detected = ov.detected_objects()
    return (result.cpu().numpy() if isinstance(image, np.ndarray) else result), detected
