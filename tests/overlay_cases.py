"""The masks of the overlay tests (a helper, not a test module): seeded random masks at the sizes that
exercise every path of the close and labelling kernels, and the shapes that break a tiled union-find.
TH, TW: the labelling tile (seg_cc_tile_h / seg_cc_tile_w)."""
import numpy as np


def sizes(TH, TW):
    # (35, 300): wider than one block of the close kernel (256 columns), so its neighbour words are inside the image
    return [(1, 1), (3, 7), (5, 5), (TH + 1, TW + 1), (70, 131), (96, 160), (35, 300)]


def random_masks(TH, TW):
    out = []
    for H, W in sizes(TH, TW):
        for d in (0.05, 0.5, 0.95):
            g = np.random.Generator(np.random.PCG64(1000 * H + W + int(100 * d)))
            out.append((f"random {H}x{W} d{d}", (g.random((H, W)) < d).astype(np.uint8)))
    return out


def border_masks(TH, TW):
    out = []
    for H, W in ((5, 5), (TH + 1, TW + 1), (70, 131)):
        for name, rows, cols in (("top", [0], None), ("bottom", [H - 1], None), ("left", None, [0]),
                                 ("right", None, [W - 1])):
            m = np.zeros((H, W), np.uint8)
            if rows:
                m[rows, :] = 1
            if cols:
                m[:, cols] = 1
            out.append((f"border {name} {H}x{W}", m))
        m = np.zeros((H, W), np.uint8)
        m[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 1
        out.append((f"corners {H}x{W}", m))
        m = np.zeros((H, W), np.uint8)
        m[0, :] = m[H - 1, :] = m[:, 0] = m[:, W - 1] = 1
        out.append((f"frame {H}x{W}", m))
    return out


def shape_masks(TH, TW):
    out = []
    H, W = 2 * TH + 5, 2 * TW + 7
    # one-pixel serpentines: full lines on every second row (column), joined at alternating ends --
    # one component that crosses every tile border many times (long parent chains)
    m = np.zeros((H, W), np.uint8)
    m[0::2, :] = 1
    for i, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    out.append(("serpentine rows", m))
    m = np.zeros((H, W), np.uint8)
    m[:, 0::2] = 1
    for i, x in enumerate(range(1, W - 1, 2)):
        m[H - 1 if i % 2 == 0 else 0, x] = 1
    out.append(("serpentine columns", m))
    # the same lines without the joints: many components side by side
    m = np.zeros((H, W), np.uint8)
    m[0::2, :] = 1
    out.append(("stripes", m))
    yy, xx = np.mgrid[0:H, 0:W]
    out.append(("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8)))
    out.append(("checkerboard odd", ((yy + xx) % 2 == 1).astype(np.uint8)))
    # two pixels touching only diagonally across a tile corner
    for cy, cx in ((TH, TW), (2 * TH, TW), (TH, 2 * TW), (2 * TH, 2 * TW)):
        for name, pts in (("nw-se", [(cy - 1, cx - 1), (cy, cx)]), ("ne-sw", [(cy - 1, cx), (cy, cx - 1)])):
            m = np.zeros((H, W), np.uint8)
            for y, x in pts:
                m[y, x] = 1
            out.append((f"diagonal {name} at {cy},{cx}", m))
    # not touching: two apart across the corner
    m = np.zeros((H, W), np.uint8)
    m[TH - 2, TW - 2] = m[TH, TW] = 1
    out.append(("apart across a corner", m))
    # concentric rings: components inside the holes of others
    m = np.zeros((H, W), np.uint8)
    for k in range(0, min(H, W) // 2, 2):
        m[k, k:W - k] = m[H - 1 - k, k:W - k] = 1
        m[k:H - k, k] = m[k:H - k, W - 1 - k] = 1
    out.append(("concentric rings", m))
    out.append(("all ones", np.ones((H, W), np.uint8)))
    out.append(("all zeros", np.zeros((H, W), np.uint8)))
    m = np.zeros((H, W), np.uint8)
    m[H - 1, W - 1] = 1
    out.append(("last pixel", m))
    return out


def mask_cases(TH, TW):
    return random_masks(TH, TW) + border_masks(TH, TW) + shape_masks(TH, TW)


def frame(h, w, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8)


def class_mask(H, W, seed):
    """A synthetic class mask: noise of other classes (one id outside the colour table), a road in two
    pieces that the close joins (a 3-column gap), car pixels inside that gap, a second smaller road blob, a
    car blob > 300 pixels, one at the frame's corner (its outline is clipped) and a small one."""
    g = np.random.Generator(np.random.PCG64(seed))
    cls = g.choice(np.array([0, 3, 4, 5, 6, 7, 8, 9, 11], np.uint8), size=(H, W))
    cls[: H // 8, : W // 4] = 11                      # outside the table: keeps the frame's pixels
    r0, r1, gap = H // 2, H - H // 6, W // 2
    cls[r0:r1, W // 10:gap] = 1
    cls[r0:r1, gap + 3:W - W // 4] = 1
    cls[r0 + 3:r0 + 9, gap:gap + 3] = 2                 # cars inside the gap: overwritten by the fill
    cls[2:8, W - 30:W - 8] = 1                         # the smaller road blob stays class 1
    cls[H // 6:H // 6 + 18, W // 3:W // 3 + 20] = 2    # 360 pixels
    cls[H - 16:, W - 24:] = 2                          # 384 pixels, touches the bottom-right corner
    cls[H // 6:H // 6 + 5, 4:12] = 2                   # 40 pixels: below the default min_area
    return cls
