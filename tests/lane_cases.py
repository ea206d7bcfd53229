"""Seeded lane-decoder heads and planted lanes for the device-only lane paths (NumPy only): tied grid maxima, tied existence logits,
valid counts on the edge of every count rule, heads of up to 16 lanes, UFLD v1 "no lane" ties, ego lanes of 0 .. 128 points on frames
of 256 .. 2397 rows, and the oracle's decoders restated with one tie rule changed.  tests/test_lane_cases_cpu.py shows on the CPU that
every case is sound and not vacuous; tests/test_gpu_lane_edges.py runs the same cases through the HIP kernels.

Two head families.  "exact": every logit is LOW or the column's hot value, so every softmax tap is exactly 0 or 1/k and the decoded
points are compared bit for bit.  "mixed": logits drawn from {-1000, 0, 8}; exp(-8) is inexact, so the project's +-1 px rule applies."""
import types

import numpy as np

LOW = -1000.0
FAMILIES = ("exact", "mixed")

# ------------------------------------------------------------------------------------------------ UFLD v2
V2_SHAPES = ((2, 1, 2, 1), (19, 6, 12, 8), (26, 5, 17, 9), (10, 7, 9, 4), (200, 128, 100, 128), (200, 72, 100, 81))    # (Gr, R, Gc, C)
V2_LANES = (4, 7, 16)
V2_WIDTHS = (0, 1, 2, 3)
V2_FRAME = {(2, 1, 2, 1): (333, 777), (19, 6, 12, 8): (1280, 720), (26, 5, 17, 9): (1640, 590), (10, 7, 9, 4): (1281, 721),
            (200, 128, 100, 128): (1920, 1080), (200, 72, 100, 81): (1280, 720)}
V2_CASES = [(s, nl, lw, fam) for s in V2_SHAPES for nl in V2_LANES for lw in V2_WIDTHS for fam in FAMILIES]
V2_BATCH_FAMILIES = (("exact", "exact", "mixed"), ("mixed", "exact", "exact"))      # of the frames of the two launches of a v2_batch
# (shape, num_lanes, local_width) of the B = 3 launches; the last one fills all four lanes of a slot to ADAS_UFLD_MAXPTS points
V2_BATCHES = (((26, 5, 17, 9), 7, 1), ((200, 72, 100, 81), 4, 2), ((10, 7, 9, 4), 16, 3), ((200, 128, 100, 128), 16, 0))


def v2_cfg(shape):
    """What oracle.ufld_decode.process_output reads of a ModelConfig, with R row and C column anchors."""
    _, R, _, C = shape
    return types.SimpleNamespace(row_anchor=np.linspace(0.42, 1, R), col_anchor=np.linspace(0, 1, C), num_lanes=4)


def v2_counts(shape, variant):
    """Valid-anchor counts (lane 0, 1, 2, 3) on the edges of the count rules: rows floor(R/2) | floor(R/2)+1 (`cnt > R/2`), columns
    floor(C/4) | floor(C/4)+1 (`cnt > C/4`); variants 2 and 3 put 2 | 3 on the column lanes where both pass the count rule (C < 8), the
    edge of `n > 2`.  Odd variants swap which lane of a pair sits below its edge."""
    _, R, _, C = shape
    r, c = (R // 2, R // 2 + 1), (C // 4, C // 4 + 1)
    if variant >= 2 and 3 <= C < 8:
        c = (2, 3)
    if variant % 2:
        r, c = r[::-1], c[::-1]
    return (c[0], r[0], r[1], c[1])


def v2_variant(nl, lw):
    return (V2_LANES.index(nl) + lw) % 4


def _hot_cells(rng, G, lw, n):
    """Hot cells of one column, first cell by kind n % 9: cell 0, 1, G-2, G-1, the last cell 8j of an unrolled group of the argmax scan
    (its body covers g = 1 .. 8*floor((G-1)/8)), the first cell 8j+1 of the next group or of the tail, a cell inside the tail, any cell,
    and no hot cell at all (a flat column: argmax 0, the window clamped at 0).  Further hot cells follow more than 2*lw cells apart, so
    the windows round the first and the last maximum share no cell."""
    body = 8 * ((G - 1) // 8)
    j = int(rng.integers(1, body // 8 + 1)) if body else 0
    kind = n % 9
    if kind == 8:
        return []
    first = (0, 1, G - 2, G - 1, 8 * j, 8 * j + 1, int(rng.integers(body + 1, G)) if body + 1 < G else G - 1, int(rng.integers(0, G)))[kind]
    first = min(max(first, 0), G - 1)
    d = 2 * lw + 1 + int(rng.integers(0, 3))
    if first + d >= G:
        d = 2 * lw + 1
    cells = [c for c in (first, first + d, first + 2 * d)[:int(rng.integers(2, 4))] if c < G]
    if len(cells) == 1 and first + 1 < G and rng.integers(2):
        cells.append(first + 1)            # a neighbour inside the window: taps of exactly 1/2
    return cells


def _v2_exist(rng, K, NL, want):
    """Existence logits [2][K][NL] on small integers: every (k, lane) present, except that decoded lane i has exactly want[i] present
    anchors; of its absent anchors about half are exact ties (at least one), the others have the larger logit in plane 0."""
    a = rng.integers(-2, 3, (K, NL))
    d = rng.integers(1, 3, (K, NL))
    ex = np.stack([a, a + d]).astype(np.float32)
    valid = {}
    for i, n in want.items():
        v = np.zeros(K, bool)
        v[rng.choice(K, n, replace=False)] = True
        tie = rng.random(K) < 0.5
        absent = np.nonzero(~v)[0]
        if len(absent):
            tie[absent[0]] = True
        for k in absent:
            ex[:, k, i] = (a[k, i], a[k, i]) if tie[k] else (a[k, i] + d[k, i], a[k, i])
        valid[i] = v
    return ex, valid


def _v2_grid(rng, G, K, NL, lw, family, valid):
    """Location logits [G][K][NL].  exact: every lane carries one hot cell per column; the decoded lanes (keys of `valid`) get _hot_cells,
    the n-th valid anchor of a lane taking kind n, so every kind is decoded.  mixed: {-1000, 0, 8} with probabilities 0.8, 0.1, 0.1."""
    if family == "mixed":
        return rng.choice(np.float32([LOW, 0, 8]), (G, K, NL), p=[0.8, 0.1, 0.1])
    g = np.full((G, K, NL), LOW, np.float32)
    hot = (2 * rng.integers(0, 4, (K, NL)) - 1).astype(np.float32)
    kk, ll = np.meshgrid(np.arange(K), np.arange(NL), indexing="ij")
    g[rng.integers(0, G, (K, NL)), kk, ll] = hot
    for i, v in valid.items():
        n = int(rng.integers(0, 9)) if K < 9 else 0
        for k in range(K):
            g[:, k, i] = LOW
            cells = _hot_cells(rng, G, lw, n if v[k] else int(rng.integers(0, 9)))
            n += int(v[k])
            g[cells, k, i] = hot[k, i]
    if len(valid) and K < 9:                      # few anchors: the first valid anchor of every lane has two maxima from cell 0 on
        for i, v in valid.items():
            if v.any():
                k = int(np.argmax(v))
                g[:, k, i] = LOW
                g[[c for c in (0, 2 * lw + 1) if c < G], k, i] = hot[k, i]
    return g


def v2_frame(shape, nl, lw, family, seed, counts):
    """One frame's [loc_row (Gr,R,NL), loc_col (Gc,C,NL), exist_row (2,R,NL), exist_col (2,C,NL)] with `counts` valid anchors on lanes 0..3."""
    Gr, R, Gc, C = shape
    rng = np.random.default_rng(seed)
    er, vr = _v2_exist(rng, R, nl, {1: counts[1], 2: counts[2]})
    ec, vc = _v2_exist(rng, C, nl, {0: counts[0], 3: counts[3]})
    return [_v2_grid(rng, Gr, R, nl, lw, family, vr), _v2_grid(rng, Gc, C, nl, lw, family, vc), er, ec]


def v2_seed(shape, nl, lw, family):
    return 100000 * V2_SHAPES.index(shape) + 1000 * nl + 10 * lw + FAMILIES.index(family)


def v2_case(shape, nl, lw, family):
    """(outs with a leading batch axis of 1, cfg, (W, H), counts)."""
    counts = v2_counts(shape, v2_variant(nl, lw))
    outs = [o[None] for o in v2_frame(shape, nl, lw, family, v2_seed(shape, nl, lw, family), counts)]
    return outs, v2_cfg(shape), V2_FRAME[shape], counts


def v2_batch(shape, nl, lw):
    """Two launches of three frames on one handle: ([outs of launch 0, outs of launch 1], cfg, (W, H)), every tensor with a batch axis of
    3.  The frames of a launch differ in family and counts; frame 1 has every anchor valid in launch 0 and counts on the rule edges in
    launch 1, so the second launch leaves fewer points in a slot than the first."""
    _, R, _, C = shape
    s = v2_seed(shape, nl, lw, "exact") + 5
    full = (C, R, R, C)
    a = [v2_frame(shape, nl, lw, "exact", s, v2_counts(shape, 0)), v2_frame(shape, nl, lw, "exact", s + 1, full),
         v2_frame(shape, nl, lw, "mixed", s + 2, v2_counts(shape, 3))]
    b = [v2_frame(shape, nl, lw, "mixed", s + 3, full), v2_frame(shape, nl, lw, "exact", s + 4, v2_counts(shape, 1)),
         v2_frame(shape, nl, lw, "exact", s + 5, v2_counts(shape, 2))]
    return [[np.stack([f[t] for f in fr]) for t in range(4)] for fr in (a, b)], v2_cfg(shape), V2_FRAME[shape]


def frame_of(outs, b):
    """Frame b of batched tensors, with a batch axis of 1 (what the oracle takes)."""
    return [o[b:b + 1] for o in outs]


def restate_v2(outs, cfg, img_w, img_h, local_width=1, grid_rule="first", tie_present=False):
    """oracle.ufld_decode.process_output restated with its two tie rules as parameters: grid_rule "first" | "last" maximum of a column,
    tie_present: an anchor whose two existence logits are equal counts as present.  ("first", False) is the oracle
    (test_lane_cases_cpu checks that on every case).  Returns (lanes, detected, trace) with trace = [(lane, G, m)] of every decoded point."""
    loc_row, loc_col, exist_row, exist_col = [np.asarray(o, np.float32)[0] for o in outs]

    def amax(loc):
        first = loc.argmax(0)
        return first if grid_rule == "first" else loc.shape[0] - 1 - loc[::-1].argmax(0)

    def present(ex):
        return (ex[1] >= ex[0]) if tie_present else (ex[1] > ex[0])

    lanes, trace = [[], [], [], []], []
    for i, loc, ex, div in ((1, loc_row, exist_row, 2), (2, loc_row, exist_row, 2), (0, loc_col, exist_col, 4), (3, loc_col, exist_col, 4)):
        G, K = loc.shape[0], loc.shape[1]
        m_all, ok = amax(loc), present(ex)
        if ok[:, i].sum() > K / div:
            for k in np.nonzero(ok[:, i])[0]:
                m = int(m_all[k, i])
                ind = np.arange(max(0, m - local_width), min(G - 1, m + local_width) + 1)
                z = loc[ind, k, i]
                e = np.exp(z - z.max())
                o = ((e / e.sum()) * ind.astype(np.float64)).sum() + 0.5
                if div == 2:
                    lanes[i].append((int(o / (G - 1) * img_w), int(cfg.row_anchor[k] * img_h)))
                else:
                    lanes[i].append((int(cfg.col_anchor[k] * img_w), int(o / (G - 1) * img_h)))
                trace.append((i, G, m))
    return lanes, [len(l) > 2 for l in lanes], trace


# ------------------------------------------------------------------------------------------------ UFLD v1
V1_SHAPES = ((3, 3), (4, 3), (9, 5), (33, 64), (17, 65), (17, 128), (100, 56), (200, 18))       # (G, K)
V1_SOURCES = ((1280, 720), (1640, 590), (333, 777))
V1_INPUT = (800, 288)
V1_CASES = [(s, fam) for s in V1_SHAPES for fam in FAMILIES]
V1_BATCH = (17, 65)
V1_ROLES = ("tie", "two", "three", "half")


def v1_cfg(shape):
    G, K = shape
    w, h = ((1280, 720), (1640, 590))[V1_SHAPES.index(shape) % 2]
    return types.SimpleNamespace(img_w=w, img_h=h, griding_num=G, cls_num_per_lane=K, row_anchor=np.linspace(64, 284, K), num_lanes=4)


def v1_frame(shape, family, seed):
    """((G+1, K, 4) head, roles): lane l plays roles[l].
      tie    cell G ("no lane") equals the best real cell on every anchor: the real cell wins, K points
      two    cell G is greater on all but exactly 2 anchors: 2 non-zero locations, not detected, 0 points
      three  cell G is greater on all but exactly 3 anchors: detected, 3 points
      half   cell G is greater on the first K/2 anchors of the tensor, -1000 on the others
    On the anchors where cell G is not greater it alternates between the column maximum (a tie) and -1000."""
    G, K = shape
    rng = np.random.default_rng(seed)
    if family == "mixed":
        real = rng.choice(np.float32([LOW, 0, 8]), (G, K, 4), p=[0.8, 0.1, 0.1])
    else:
        real = np.full((G, K, 4), LOW, np.float32)
        hot = (2 * rng.integers(0, 4, (K, 4)) - 1).astype(np.float32)
        for l in range(4):
            for k in range(K):
                real[rng.choice(G, int(rng.integers(1, min(3, G) + 1)), replace=False), k, l] = hot[k, l]
    top = real.max(0)
    roles = [V1_ROLES[p] for p in rng.permutation(4)]
    last = np.empty((K, 4), np.float32)
    for l, role in enumerate(roles):
        if role == "tie":
            greater = np.zeros(K, bool)
        elif role == "half":
            greater = np.arange(K) < K // 2
        else:
            greater = np.ones(K, bool)
            greater[rng.choice(K, 2 if role == "two" else 3, replace=False)] = False
        calm = np.where(np.arange(K) % 2 == 0, top[:, l], np.float32(LOW)) if role != "tie" else top[:, l]
        last[:, l] = np.where(greater, top[:, l] + 1, calm)
    return np.concatenate([real, last[None]]), roles


def v1_seed(shape, family):
    return 7000 + 10 * V1_SHAPES.index(shape) + FAMILIES.index(family)


def v1_case(shape, family):
    """((1, G+1, K, 4) head, roles, cfg)."""
    head, roles = v1_frame(shape, family, v1_seed(shape, family))
    return head[None], roles, v1_cfg(shape)


def v1_batch():
    """((3, G+1, K, 4) heads, [roles per frame], cfg) at V1_BATCH: an exact, a mixed and another exact frame."""
    fr = [v1_frame(V1_BATCH, fam, 7900 + b) for b, fam in enumerate(("exact", "mixed", "exact"))]
    return np.stack([f[0] for f in fr]), [f[1] for f in fr], v1_cfg(V1_BATCH)


def restate_v1(head, cfg, input_w, input_h, src_w, src_h, nolane_wins_tie=False):
    """oracle.ufld_decode.process_output_v1 restated with its tie rule as a parameter: nolane_wins_tie=True lets cell G win against an
    equal real cell (`>=` where the device and np.argmax have `>`).  False is the oracle."""
    G, K = cfg.griding_num, cfg.cls_num_per_lane
    raw = np.asarray(head, np.float32).reshape(G + 1, K, -1)[:, ::-1, :]
    z = raw[:G]
    e = np.exp(z - z.max(axis=0, keepdims=True))
    loc = ((e / e.sum(axis=0, keepdims=True)) * np.arange(1, G + 1).reshape(-1, 1, 1)).sum(axis=0)
    top = z.max(axis=0)
    loc[(raw[G] >= top) if nolane_wins_tie else (raw[G] > top)] = 0
    col_w = np.linspace(0, input_w - 1, G)
    col_w = col_w[1] - col_w[0]
    lanes, detected = [], []
    for lane in range(loc.shape[1]):
        ok = int((loc[:, lane] != 0).sum()) > 2
        pts = []
        for k in range(K):
            if ok and loc[k, lane] > 0:
                x = loc[k, lane] * col_w * cfg.img_w / input_w - 1
                y = cfg.img_h * (cfg.row_anchor[K - 1 - k] / input_h) - 1
                pts.append((int(x * (src_w / cfg.img_w)), int(y * (src_h / cfg.img_h))))
        lanes.append(pts)
        detected.append(ok)
    return lanes, detected


# ------------------------------------------------------------------------------------------------ lane geometry
GEO_COUNTS = ((3, 3), (10, 11), (11, 10), (11, 11), (12, 64), (63, 64), (64, 65), (65, 20), (127, 128), (128, 128), (128, 3), (11, 128))
GEO_FRAMES = ((1280, 720), (1279, 719), (1281, 721), (456, 256), (455, 257), (1920, 1080), (4260, 2397))
GEO_STARTS = (0.2, 0.35, 0.42, 0.6)
GEO_CASES = [(wh, n) for wh in GEO_FRAMES for n in GEO_COUNTS]


def _rows(rng, H, n, start):
    """n distinct rows from int(start * H) (always the first) to H - 1, ascending, as a decoder orders them."""
    y0 = int(start * H)
    rest = rng.choice(np.arange(y0 + 1, H), n - 1, replace=False)
    return np.sort(np.concatenate([[y0], rest]))


def geo_lanes(wh, counts):
    """(lanes, status): the two ego lanes as integer points on noisy parabolas in y (noise -2 .. 2) with distinct rows.  The lanes start
    on different rows (two of GEO_STARTS that leave room for the lane's points); the left lane bends out of the image through x = 0
    before the bottom row, the right lane bends to the right.  The side lanes are short straight lines."""
    W, H = wh
    nL, nR = counts
    seed = GEO_FRAMES.index(wh) * 100 + GEO_COUNTS.index(counts)
    rng = np.random.default_rng(9000 + seed)
    fits = [[f for f in GEO_STARTS if H - int(f * H) >= n] for n in (nL, nR)]
    fL = fits[0][seed % len(fits[0])]
    fR = [f for f in fits[1] if f != fL][(seed // 4) % (len(fits[1]) - (fL in fits[1]))]
    yl, yr = _rows(rng, H, nL, fL), _rows(rng, H, nR, fR)
    tl, tr = (yl - yl[0]) / (H - 1 - yl[0]), (yr - yr[0]) / (H - 1 - yr[0])
    xl = np.rint(0.34 * W - 0.40 * W * tl ** 2).astype(np.int64) + rng.integers(-2, 3, nL)
    xr = np.rint(0.60 * W + 0.05 * W * tr + 0.22 * W * tr ** 2).astype(np.int64) + rng.integers(-2, 3, nR)
    side_y = np.linspace(0.5 * H, H - 1, 5).astype(np.int64)
    lanes = [[(int(0.05 * W + k), int(y)) for k, y in enumerate(side_y)], [(int(x), int(y)) for x, y in zip(xl, yl)],
             [(int(x), int(y)) for x, y in zip(xr, yr)], [(int(0.97 * W - k), int(y)) for k, y in enumerate(side_y)]]
    return lanes, [True, True, True, True]


def geo_matrix(wh, lanes=None):
    """The homography of a (W, H) frame onto a bird view of the same size: the default trapezoid of analysis.PerspectiveTransformation,
    or with `lanes` that trapezoid re-anchored on the two ego lanes (updateTransformParams "Default"), which keeps every lane point
    inside the bird view's rows whatever row the lane starts on."""
    import importlib
    from conftest import load_pkg
    load_pkg()
    tv = importlib.import_module("adas_amd.analysis").PerspectiveTransformation(wh)
    if lanes is not None:
        tv.updateTransformParams(lanes[1], lanes[2], "Default")
    return tv.M.copy()


# direction: identity homography, 1280 x 720, 72 points per lane from row 290 to 716
DIR_WH = (1280, 720)
DIR_CASES = {      # name -> (which lane bends, planted c0, x[0] - x[n/2], direction the reference must give, reason)
    "left-below-eq": ("L", -0.00019, 0, "L", "both conditions hold at equality"),
    "left-below-gt": ("L", -0.00019, 1, "F", "comparison"),
    "left-above-eq": ("L", -0.00012, 0, "F", "threshold"),
    "left-above-gt": ("L", -0.00012, 1, "F", "threshold"),
    "right-above-eq": ("R", 0.00019, 0, "R", "both conditions hold at equality"),
    "right-above-lt": ("R", 0.00019, -1, "F", "comparison"),
    "right-below-eq": ("R", 0.00012, 0, "F", "threshold"),
    "right-below-lt": ("R", 0.00012, -1, "F", "threshold"),
}


def dir_lanes(name):
    """(lanes, status) of a direction case: the bending lane is x = c0 (y - yv)^2 + x0 rounded to integers, its vertex yv midway between
    row 0 and row n/2 of the lane, so x[0] == x[n/2] up to rounding; x[0] is then set to x[n/2] + the case's difference.  The other lane
    bends the same way at |c0| = 0.00003 and decides nothing."""
    side, c0, diff, _, _ = DIR_CASES[name]
    y = np.arange(290, 720, 6)
    n = len(y)
    yv = (y[0] + y[n // 2]) / 2

    def lane(c, x0):
        x = np.rint(c * (y - yv) ** 2 + x0).astype(np.int64)
        return x

    xl = lane(c0 if side == "L" else np.sign(c0) * 0.00003, 420)
    xr = lane(c0 if side == "R" else np.sign(c0) * 0.00003, 860)
    bent = xl if side == "L" else xr
    bent[0] = bent[n // 2] + diff
    return [[], [(int(a), int(b)) for a, b in zip(xl, y)], [(int(a), int(b)) for a, b in zip(xr, y)], []], [False, True, True, False]


# fewer than three points on an ego lane: (nL, nR)
FEW_COUNTS = ((0, 40), (40, 0), (1, 40), (40, 1), (2, 40), (40, 2), (2, 2), (1, 2), (0, 0))


def few_lanes(counts):
    """(lanes, status, area): ego lanes of counts points on two straight lines of 1280 x 720; a lane without points is reported as not
    detected, every other lane as detected.  area: the polygon the device must write when both are detected (the points as they are,
    left then reversed right -- no lane has more than 10 points on both sides), else no points."""
    nL, nR = counts
    yl, yr = np.arange(700 - 9 * nL, 700, 9)[:nL], np.arange(705 - 9 * nR, 705, 9)[:nR]
    left = [(int(300 + 0.3 * (700 - y)), int(y)) for y in yl]
    right = [(int(980 - 0.3 * (705 - y)), int(y)) for y in yr]
    status = [False, nL > 0, nR > 0, False]
    area = left + right[::-1] if (nL > 0 and nR > 0) else []
    return [[], left, right, []], status, np.asarray(area, np.int64).reshape(-1, 2)


def geo_batch():
    """Two launches of three frames: ([(lanes, status) x 3] x 2, (W, H), [M x 3]).  The second launch differs in slot 1 only, whose lanes
    are shorter than before; the three homographies differ (the default trapezoid, the same re-anchored on the lanes of frame 0, and the
    identity)."""
    import importlib
    from conftest import load_pkg
    load_pkg()
    A = importlib.import_module("adas_amd.analysis")
    wh = (1280, 720)
    a = [geo_lanes(wh, (64, 65)), geo_lanes(wh, (128, 128)), geo_lanes(wh, (11, 128))]
    b = [a[0], geo_lanes(wh, (12, 64)), a[2]]
    tv = A.PerspectiveTransformation(wh)
    m0 = tv.M.copy()
    tv.updateTransformParams(a[0][0][1], a[0][0][2], "Default")
    return [a, b], wh, [m0, tv.M.copy(), np.eye(3)]
