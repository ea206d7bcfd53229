"""NumPy restatement of the lane overlay's pixel rules D1-D5 (csrc/overlay_core.h), written from the STEPPING definitions: the
midpoint walk of the disc, the error-term loop of the line, the sorted crossings of the polygon -- not from the closed forms the
device uses.  Modelled on OpenCV 4.5's drawing.cpp / arithm; the definitions are the authority, parity with a real cv2 build is
unpinned, and lines are not clipped before they are walked.  Test scaffolding."""
import numpy as np

LANE_COLORS = [(255, 0, 0), (46, 139, 87), (50, 205, 50), (0, 255, 255)]
OFFSET_COLOR = (0, 0, 255)
AREA_COLOR = (255, 191, 0)
COLLISION_COLORS = [(0, 255, 255), (0, 255, 0), (0, 102, 255), (0, 0, 255)]   # UNKNOWN, NORMAL, PROMPT, WARNING
DIST_COLOR = (255, 255, 255)
OFFSET_UNKNOWN, OFFSET_RIGHT, OFFSET_LEFT, OFFSET_CENTER = 0, 1, 2, 3
LANES, AREA, DISTANCE, BIRD = 1, 2, 4, 8
POLY_RANGE = 1
COORD_MAX = 32767


# ------------------------------------------------------------------------------------------------------------- D1
def blend(a, alpha, b):
    """addWeighted(a, alpha, b, 1 - alpha, 0) on u8 (arrays or scalars): two fp32 products, one fp32 add, ties to even."""
    af = np.float32(alpha)
    bf = np.float32(1.0 - float(alpha))
    pa = np.asarray(a).astype(np.float32) * af
    pb = np.asarray(b).astype(np.float32) * bf
    s = (pa + pb).astype(np.float32)
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- D2
def disc_halfwidths(r):
    hw = [0] * (r + 1)
    dx, dy, err, plus, minus = r, 0, 0, 1, 2 * r - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def disc_rows(cx, cy, r, H, W):
    """(y, first column, last column) of every row of the disc that has a pixel inside the H x W image."""
    hw = disc_halfwidths(r)
    cx, cy = int(cx), int(cy)
    for j in range(-r, r + 1):
        y = cy + j
        if not 0 <= y < H:
            continue
        lo, hi = max(cx - hw[abs(j)], 0), min(cx + hw[abs(j)], W - 1)
        if lo <= hi:
            yield y, lo, hi


def disc_mask(cx, cy, r, H, W):
    m = np.zeros((H, W), bool)
    for y, lo, hi in disc_rows(cx, cy, r, H, W):
        m[y, lo:hi + 1] = True
    return m


# ------------------------------------------------------------------------------------------------------------- D3
def line_pixels(ax, ay, bx, by):
    """Every pixel of the 8-connected line, by the error-term loop."""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    if bx < ax:
        ax, ay, bx, by = bx, by, ax, ay
    dx, dy = bx - ax, by - ay
    M, m = max(abs(dx), abs(dy)), min(abs(dx), abs(dy))
    ymajor = abs(dy) > abs(dx)
    sx, sy = (1 if dx > 0 else 0), (1 if dy > 0 else (-1 if dy < 0 else 0))
    err = M - 2 * m
    x, y = ax, ay
    out = [(x, y)]
    for _ in range(M):
        diag = err < 0
        err += -2 * m + (2 * M if diag else 0)
        if ymajor:
            y += sy
            if diag:
                x += sx
        else:
            x += sx
            if diag:
                y += sy
        out.append((x, y))
    return out


def line_mask(ax, ay, bx, by, H, W):
    m = np.zeros((H, W), bool)
    for x, y in line_pixels(ax, ay, bx, by):
        if 0 <= x < W and 0 <= y < H:
            m[y, x] = True
    return m


# ------------------------------------------------------------------------------------------------------------- D4
def poly_mask(pts, H, W):
    """(coverage, flags) of fillPoly on one contour."""
    pts = [(int(x), int(y)) for x, y in np.asarray(pts, np.int64).reshape(-1, 2)]
    m = np.zeros((H, W), bool)
    n = len(pts)
    if n == 0:
        return m, 0
    if any(abs(x) > COORD_MAX or abs(y) > COORD_MAX for x, y in pts):
        return m, POLY_RANGE
    edges = [(pts[i], pts[(i + 1) % n]) for i in range(n)]
    for (ax, ay), (bx, by) in edges:
        for x, y in line_pixels(ax, ay, bx, by):
            if 0 <= x < W and 0 <= y < H:
                m[y, x] = True
    if n < 3:
        return m, 0
    a, b = np.array([e[0] for e in edges], np.int64), np.array([e[1] for e in edges], np.int64)
    keep = a[:, 1] != b[:, 1]                               # horizontal edges cross nothing
    a, b = a[keep], b[keep]
    up = a[:, 1] > b[:, 1]                                  # top (x0, y0) = the end with the smaller y
    x0, y0 = np.where(up, b[:, 0], a[:, 0]), np.where(up, b[:, 1], a[:, 1])
    x1, y1 = np.where(up, a[:, 0], b[:, 0]), np.where(up, a[:, 1], b[:, 1])
    num, den = (x1 - x0) << 16, y1 - y0
    D = np.where(num >= 0, 1, -1) * (np.abs(num) // den)    # int64 division truncated toward zero
    for y in range(H):
        act = (y0 <= y) & (y < y1)
        xs = np.sort((x0[act] << 16) + (y - y0[act]) * D[act])
        for k in range(0, len(xs) - 1, 2):
            lo = -((-int(xs[k])) // 65536)     # ceil
            hi = int(xs[k + 1]) // 65536       # floor
            lo, hi = max(lo, 0), min(hi, W - 1)
            if lo <= hi:
                m[y, lo:hi + 1] = True
    return m, 0


# ------------------------------------------------------------------------------------------------------------- D5
def lane_colors(offset_type=OFFSET_UNKNOWN, table=LANE_COLORS, offset_color=OFFSET_COLOR):
    t = [tuple(c) for c in table]
    if offset_type == OFFSET_RIGHT:
        t[1] = tuple(offset_color)
    if offset_type == OFFSET_LEFT:
        t[2] = tuple(offset_color)
    return t


def draw_lanes(img, lanes, offset_type=OFFSET_UNKNOWN, alpha=0.3, radius=3, direct=False, table=LANE_COLORS):
    """DrawDetectedOnFrame (direct=False) / DrawDetectedOnBirdView (direct=True, radius 10): lanes = 4 lists of (x, y)."""
    H, W = img.shape[:2]
    cols = lane_colors(offset_type, table)
    paint = np.zeros((H, W, 3), np.uint8)
    cover = np.zeros((H, W), bool)
    for l in range(4):
        for x, y in np.asarray(lanes[l], np.int64).reshape(-1, 2):
            for yy, lo, hi in disc_rows(x, y, radius, H, W):
                paint[yy, lo:hi + 1] = cols[l]          # the last disc drawn wins
                cover[yy, lo:hi + 1] = True
    out = img.copy()
    out[cover] = paint[cover] if direct else blend(paint[cover], alpha, img[cover])
    return out


def draw_area(img, poly, color=AREA_COLOR, alpha=0.85):
    """DrawAreaOnFrame's pixels: (image, flags)."""
    H, W = img.shape[:2]
    m, flags = poly_mask(poly, H, W)
    out = img.copy()
    out[m] = blend(img[m], alpha, np.array(color, np.uint8)[None, :])
    return out, flags


def draw_distance(img, points, radius=4, color=DIST_COLOR):
    H, W = img.shape[:2]
    out = img.copy()
    for x, y in np.asarray(points, np.int64).reshape(-1, 2):
        for yy, lo, hi in disc_rows(x, y, radius, H, W):
            out[yy, lo:hi + 1] = color
    return out


def compose(img, lanes=None, poly=None, area_status=False, dist=None, offset_type=OFFSET_UNKNOWN, area_color=AREA_COLOR, stages=7,
            lane_alpha=0.3, area_alpha=0.85, radii=(3, 4)):
    """One frame through stages 1-3 of D5: (frame_show, flags)."""
    out, flags = img.copy(), 0
    if stages & LANES and lanes is not None:
        out = draw_lanes(out, lanes, offset_type, lane_alpha, radii[0])
    if stages & AREA and poly is not None and area_status and len(poly):
        out, flags = draw_area(out, poly, area_color, area_alpha)
    if stages & DISTANCE and dist is not None:
        out = draw_distance(out, dist, radii[1])
    return out, flags
