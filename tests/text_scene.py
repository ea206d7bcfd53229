"""The synthetic fonts and the scenes of the overlay text's tests (the repository ships no font).  A font's coverage comes from a seeded
generator: values in {0, 255} for the even slots, the full 0..255 range for the odd ones; widths run 1..9, some bearings are negative, and
advances carry fractional 16.16 parts so that the pen's carry (T3) matters.  Glyph 'c' of a full-range font holds coverage 1, 127, 128, 254
in its first row."""
import numpy as np
import text_ref as R

LADDER = (10, 3)                      # slots 10, 11, 12 at scales 0.5, 0.75, 1.0: 1 / 1.6 = 0.625 ties 0.5 with 0.75
LINE_SLOT, LINE_SLOT_BINARY = 13, 14
STYLE = dict(dist_first=LADDER[0], dist_count=LADDER[1], id_first=LADDER[0], id_count=LADDER[1])
NAMES = ["car", "person", "traffic light", "a-class-name-of-31-bytes-long.."]
COLORS = [(255, 64, 0), (20, 200, 25), (0, 0, 255), (7, 8, 9)]


def make_font(seed, binary, cell_h=9, scale=1.0):
    rng = np.random.default_rng(1000 + seed)
    gw = 1 + (np.arange(95) * 7 + seed) % 9
    gw[0] = 0                                             # the space draws nothing
    gx = np.zeros(95, np.int64)
    x = 1
    for g in range(95):
        gx[g] = x
        x += gw[g] + 1
    atlas = rng.integers(0, 2, (cell_h, x)).astype(np.uint8) * 255 if binary else rng.integers(0, 256, (cell_h, x)).astype(np.uint8)
    if not binary:
        c = ord("c") - 32
        gw[c] = max(gw[c], 4)
        if gx[c] + gw[c] > x:
            gx[c] = x - gw[c]
        atlas[0, gx[c]:gx[c] + 4] = (1, 127, 128, 254)
    bearing = (np.arange(95) * 5 + seed) % 5 - 2          # -2 .. 2
    advance = ((gw + 1) << 16) + rng.integers(0, 1 << 16, 95)
    return dict(atlas=atlas, glyph_x=gx.astype(np.int32), glyph_w=gw.astype(np.int32), bearing_x=bearing.astype(np.int32), advance=advance.astype(np.int32),
                baseline_row=cell_h - 3, size_h=cell_h - 2, size_w_extra=int(rng.integers(0, 3 << 16)), scale=float(scale))


def fonts():
    """{slot: font} for every slot the default style and STYLE name."""
    f = {k: make_font(k, k % 2 == 0, cell_h=7 + k % 5, scale=(1.0, 0.75, 6e-4, 1.0, 1.0, 1.0, 1.0, 1.0, 0.7, 0.6)[k]) for k in range(10)}
    for i, s in enumerate((0.5, 0.75, 1.0)):
        f[LADDER[0] + i] = make_font(20 + i, i == 1, cell_h=6 + 2 * i, scale=s)
    f[LINE_SLOT] = make_font(31, False, cell_h=10)
    f[LINE_SLOT_BINARY] = make_font(32, True, cell_h=8)
    return f


def background(n, H, W, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3)).astype(np.uint8)


def empty_scene():
    return dict(det_xyxy=np.zeros((0, 4), np.int32), det_cls=np.zeros(0, np.int32), trk_tlwh=np.zeros((0, 4)), trk_cls=np.zeros(0, np.int32),
                trk_ids=np.zeros(0, np.int32), trk_last=np.zeros((0, 4)), traj_len=np.zeros(0, np.int32), dist_points=np.zeros((0, 2), np.int32),
                dist_d=np.zeros(0), offset=0, curvature=0, collision=0, det_names=NAMES, trk_names=NAMES, det_colors=COLORS, trk_colors=COLORS, lines=[])


def scene_edges(W, H):
    """Caller strings clipped at each of the four edges and wholly outside, an empty string, a '?' substitution, coverage 1, 127, 128, 254."""
    s = empty_scene()
    s["lines"] = [(-4, H // 2, LINE_SLOT, (10, 200, 90), "Left edge"), (W - 7, H // 2 + 3, LINE_SLOT_BINARY, (250, 0, 90), "Right edge"),
                  (W // 3, 2, LINE_SLOT, (1, 2, 3), "Top"), (W // 4, H + 4, LINE_SLOT_BINARY, (255, 255, 255), "Bottom"),
                  (W + 40, 5, LINE_SLOT, (9, 9, 9), "outside"), (W // 2, H // 2, LINE_SLOT, (0, 0, 0), ""),
                  (W // 2, H - 4, LINE_SLOT, (0, 255, 128), "a\x7fb\xe9\x1f"), (3, H - 2, LINE_SLOT, (255, 0, 255), "ccc")]
    return s, R.LINES


def scene_overlap(W, H, swap):
    s = empty_scene()
    a, b = (5, H // 2 + 2, LINE_SLOT, (255, 0, 0), "overlapping"), (8, H // 2 + 4, LINE_SLOT_BINARY, (0, 255, 0), "strings")
    s["lines"] = [b, a] if swap else [a, b]
    return s, R.LINES


def scene_labels(W, H):
    """A label with ymin = 0, an 'unknown' one, a rectangle under its label in the middle, one leaving through the right edge."""
    s = empty_scene()
    s["det_xyxy"] = np.array([[3, 0, 30, 12], [W // 2, H // 2, W // 2 + 9, H - 1], [W - 12, H - 3, W + 5, H + 9], [-6, 14, 4, 20]], np.int32)
    s["det_cls"] = np.array([0, 17, 3, 1], np.int32)
    return s, R.DETECTIONS


def scene_overflow(W, H, n_det=129):
    """129 detections are 258 items: the 257th and 258th are absent and the frame is flagged."""
    s = empty_scene()
    k = np.arange(n_det)
    s["det_xyxy"] = np.stack([(k * 5) % (W + 10) - 5, (k * 3) % (H + 8), (k * 5) % (W + 10) + 9, (k * 3) % (H + 8) + 6], 1).astype(np.int32)
    s["det_cls"] = (k % 5).astype(np.int32)
    return s, R.DETECTIONS


def scene_full(W, H, seed=0, n_det=24, n_trk=16, n_dist=8):
    """Every kind: the shapes of tools/bench_text.py's frame, with the numbers the fixture asks for -- d < 0, binary ties of '%.2f', 1 / d on
    both sides of 0.4 and of 1, the ladder's tie, d == 0, nan, a distance out of range."""
    rng = np.random.default_rng(100 + seed)
    s = empty_scene()
    x0, y0 = rng.integers(-20, max(W - 40, 1), n_det), rng.integers(-5, max(H - 30, 8), n_det)
    s["det_xyxy"] = np.stack([x0, y0, x0 + rng.integers(10, 200, n_det), y0 + rng.integers(10, 200, n_det)], 1).astype(np.int32)
    s["det_xyxy"][0, 1] = 0
    s["det_cls"] = rng.integers(-1, 6, n_det).astype(np.int32)
    s["trk_tlwh"] = np.stack([rng.uniform(-30, max(W - 50, 10), n_trk), rng.uniform(-30, max(H - 50, 10), n_trk), rng.uniform(0.5, 300, n_trk), rng.uniform(0.5, 300, n_trk)], 1)
    s["trk_tlwh"][1, 2:] = (2.0, 5.0)                     # area 10: not drawn
    s["trk_cls"] = rng.integers(-1, 6, n_trk).astype(np.int32)
    s["trk_ids"] = rng.integers(1, 5000, n_trk).astype(np.int32)
    s["trk_ids"][0] = 2147483647
    tl = s["trk_tlwh"]
    s["trk_last"] = np.stack([tl[:, 0], tl[:, 1], tl[:, 0] + tl[:, 2], tl[:, 1] + tl[:, 3]], 1) + rng.uniform(-2, 2, (n_trk, 4))
    s["traj_len"] = rng.integers(0, 31, n_trk).astype(np.int32)
    s["traj_len"][2] = 1
    s["dist_points"] = np.stack([rng.integers(0, W, n_dist), rng.integers(0, H, n_dist)], 1).astype(np.int32)
    d = [-1.0, 2.125, 0.375, 1.6, 0.5, 2.4, 2.6, 0.0, float("nan"), 2.0 ** 30, 0.9999, 1.0001, 12.345, 2.675][:n_dist]
    s["dist_d"] = np.array(d + list(rng.uniform(0.2, 60, n_dist - len(d))))
    s["offset"], s["curvature"], s["collision"] = int(rng.integers(0, 4)), int(rng.integers(0, 6)), int(rng.integers(0, 4))
    s["lines"] = [(10, 345, LINE_SLOT, (255, 255, 255), "FPS  : 31.42"), (W - 220, 300, LINE_SLOT_BINARY, (230, 230, 230), "object-infer : 0.01 s")]
    return s, 63


def pack_scenes(scenes):
    """[scene per frame] -> (dict of stacked arrays by the Arrays field names, det_cap, trk_cap, dist_cap)."""
    n = len(scenes)
    caps = [max(1, max(len(s[k]) for s in scenes)) for k in ("det_cls", "trk_cls", "dist_d")]
    a = dict(det_xyxy=np.zeros((n, caps[0], 4), np.int32), det_cls=np.zeros((n, caps[0]), np.int32), det_counts=np.zeros(n, np.int32),
             trk_tlwh=np.zeros((n, caps[1], 4)), trk_cls=np.zeros((n, caps[1]), np.int32), trk_ids=np.zeros((n, caps[1]), np.int32),
             trk_counts=np.zeros(n, np.int32), trk_last_tlbr=np.zeros((n, caps[1], 4)), traj_len=np.zeros((n, caps[1]), np.int32),
             dist_points=np.zeros((n, caps[2], 2), np.int32), dist_d=np.zeros((n, caps[2])), dist_counts=np.zeros(n, np.int32),
             offset_type=np.zeros(n, np.int32), curvature_type=np.zeros(n, np.int32), collision_type=np.zeros(n, np.int32))
    for q, s in enumerate(scenes):
        nd, nt, nn = len(s["det_cls"]), len(s["trk_cls"]), len(s["dist_d"])
        a["det_xyxy"][q, :nd], a["det_cls"][q, :nd], a["det_counts"][q] = s["det_xyxy"], s["det_cls"], nd
        a["trk_tlwh"][q, :nt], a["trk_cls"][q, :nt], a["trk_ids"][q, :nt], a["trk_counts"][q] = s["trk_tlwh"], s["trk_cls"], s["trk_ids"], nt
        a["trk_last_tlbr"][q, :nt], a["traj_len"][q, :nt] = s["trk_last"], s["traj_len"]
        a["dist_points"][q, :nn], a["dist_d"][q, :nn], a["dist_counts"][q] = s["dist_points"], s["dist_d"], nn
        a["offset_type"][q], a["curvature_type"][q], a["collision_type"][q] = s["offset"], s["curvature"], s["collision"]
    return a, caps


def item_tuple(it):
    """An item, from text_ref.layout or from the device / the host build, as one comparable tuple."""
    return (it["kind"], it["source"], it["x"], it["y"], it["x1"], it["y1"], tuple(it["box"]), it["slot"], tuple(it["color"]), it["text"])
