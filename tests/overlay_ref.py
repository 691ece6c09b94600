"""Pure-numpy restatement of the overlay stage (seg_amd/overlay.py, csrc/overlay.hip): the steps of
inference.py's overlay_predictions as the project defines them, for bit-for-bit comparison.

Small images only (the labelling is a stack flood fill).  Nothing here comes from oracle/ or from the
reference's code; test_overlay_ref.py checks the parts against scipy.ndimage.
"""
import numpy as np

COLOR_MAP = {0: [0, 0, 0], 1: [0, 255, 0], 2: [255, 0, 0], 3: [250, 170, 30], 4: [220, 220, 0], 5: [220, 20, 60],
             6: [244, 35, 232], 7: [0, 0, 70], 8: [0, 60, 100], 9: [0, 0, 230]}


def _window(mask, fill, op):
    """op over the 5x5 window of every pixel; positions outside the image hold `fill` (op's neutral)."""
    H, W = mask.shape
    pad = np.full((H + 4, W + 4), fill, bool)
    pad[2:-2, 2:-2] = mask
    out = np.full((H, W), fill, bool)
    for dy in range(5):
        for dx in range(5):
            out = op(out, pad[dy:dy + H, dx:dx + W])
    return out


def close5(mask):
    """5x5 all-ones close, constant border: pixels outside the image never decide."""
    dil = _window(mask.astype(bool), False, np.logical_or)
    return _window(dil, True, np.logical_and).astype(np.uint8)


def label8(mask):
    """int32 labels: the smallest linear index of the pixel's 8-connected component, background -1."""
    H, W = mask.shape
    m = mask.astype(bool)
    lab = np.full((H, W), -1, np.int32)
    for y0 in range(H):
        for x0 in range(W):
            if not m[y0, x0] or lab[y0, x0] >= 0:
                continue
            root = y0 * W + x0  # raster order: the first pixel met is the smallest index
            lab[y0, x0] = root
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for yy in range(max(y - 1, 0), min(y + 2, H)):
                    for xx in range(max(x - 1, 0), min(x + 2, W)):
                        if m[yy, xx] and lab[yy, xx] < 0:
                            lab[yy, xx] = root
                            stack.append((yy, xx))
    return lab


def components(lab):
    """[(root, x, y, w, h, area)] in ascending root order."""
    W = lab.shape[1]
    out = []
    for root in np.unique(lab[lab >= 0]):
        ys, xs = np.nonzero(lab == root)
        out.append((int(root), int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1),
                    int(ys.max() - ys.min() + 1), int(ys.size)))
    return out


def largest(lab):
    """(root, area) of the largest component, ties to the smaller root; (-1, 0) without foreground."""
    best = (-1, 0)
    for root, _, _, _, _, area in components(lab):
        if area > best[1]:
            best = (root, area)
    return best


def boxes(lab, min_area, max_boxes):
    """(stored rows [x, y, w, h, area], (stored, passed))."""
    rows = [[x, y, w, h, area] for _, x, y, w, h, area in components(lab) if area > min_area]
    return rows[:max_boxes], (min(len(rows), max_boxes), len(rows))


def blend(a, b):
    """cv2.addWeighted(a, 0.6, b, 0.4, 0) on uint8: float32 products, float32 sum, round half to even."""
    s = a.astype(np.float32) * np.float32(0.6) + b.astype(np.float32) * np.float32(0.4)
    return np.rint(s).astype(np.uint8)


def outline_mask(shape, rows):
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for x, y, w, h, _ in rows:
        rect = (xx >= x) & (xx <= x + w) & (yy >= y) & (yy <= y + h)
        inner = (xx >= x + 2) & (xx <= x + w - 2) & (yy >= y + 2) & (yy <= y + h - 2)
        m |= rect & ~inner
    return m


def overlay(image, cls, color_map=COLOR_MAP, min_area=300, max_boxes=64, draw_boxes=True):
    """Steps 1-9: (result, cleaned, box dicts, {'cars': n})."""
    Hf = image.shape[0]
    lab = label8(close5(cls == 1))
    root, _ = largest(lab)
    cleaned = cls.copy()
    if root >= 0:
        cleaned[lab == root] = 1
    items = color_map if isinstance(color_map, dict) else dict(enumerate(color_map))
    over = image.copy()
    for k, c in items.items():
        over[cleaned == k] = c
    rows, (_, passed) = boxes(label8(cleaned == 2), min_area, max_boxes)
    result = blend(image, over)
    if draw_boxes:
        m = outline_mask(cls.shape, rows)
        green = np.broadcast_to(np.array([0, 255, 0], np.uint8), image.shape)
        result[m] = blend(image, green)[m]
    out = [{"x": x, "y": y, "w": w, "h": h, "area": a, "distance": int(50 * (1.0 - (y + h) / Hf))}
           for x, y, w, h, a in rows]
    return result, cleaned, out, {"cars": passed}
