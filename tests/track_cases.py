"""Deterministic tracker cases for the code of csrc/track_core.h that only hipcc compiles (bt_lap_wave<1|2|4|8>, the block-wide bt_lap
with block_argmin_unused, the ballot bt_compact, the barriers of bytetrack_update).  Importable without a GPU: tests/test_track_cases_cpu.py
proves every case sound on the host build, tests/test_gpu_track_edges.py runs them through adas_bytetrack_*.

A case is a dict(name, steps); a step is a frame dict(boxes, scores, ids) or the string "reset".  expected(steps, cap) gives, per frame,
(snapshot, err): the oracle's message and the BtHeader.err bits a tracker of capacity cap = (max_tracks, max_dets) must show.

a. contested(seed, T, D, n_lo): four frames on a lattice whose neighbours overlap, so that the first association of f1 is T rows by D
   columns in which neighbouring tracks compete for detections that lie between them; CONTESTED lists the (T, D) pairs, one per side of
   every solver size class, and SEEDS the seed each uses (chosen so that no association of any frame has a cost tie; the CPU test proves it).
b. tie scenes: 64 x 64 boxes (the tlwh -> xyah -> tlbr round trip is exact), equal scores, tied detections of different classes.
c. degenerate shapes: no tracks, no detections, neither, no low band, unconfirmed tracks left alone, every score on the threshold.
d. capacity: more candidates than slots, more detections than max_dets, a ninth class on one track; err is sticky until reset."""
import copy
import functools

import numpy as np

from oracle import bytetrack

ERR_DET, ERR_TRACK, ERR_HIST = 1, 2, 4          # BT_ERR_* of track_core.h
HIST = 8                                        # ADAS_BT_HIST
NTHR = 256                                      # threads of bytetrack_update_kernel
LDS_BUDGET = 156 * 1024                         # ADAS_BT_LDS_BUDGET
BIG, DEFAULT = (1024, 1024), (256, 256)


# ------------------------------------------------------------------------------------------------ BtLds, restated
def lds_fixed_bytes(MT, MD, nthr=NTHR):
    d = MT + 2 * (MD + 1) + nthr                                # u, v, minv, red_v
    i = 2 * (MD + 1) + nthr + 4 * MD + 11 * MT + 16 + 16        # way p red_i, hi lo rem y, eleven track lists, n, wsum
    return d * 8 + i * 4 + (MD + 1) + 64


def lds_cost_doubles(MT, MD, nthr=NTHR):
    f = (lds_fixed_bytes(MT, MD, nthr) + 15) & ~15
    room = (LDS_BUDGET - f) // 8 if f < LDS_BUDGET else 0
    return min(MT * MD, room)


def cost_side(T, D, cap):
    """Where bytetrack_update keeps a T x D cost matrix on a tracker of capacity cap: "lds" or "hbm" (BtStream.cost)."""
    return "lds" if T * D <= lds_cost_doubles(*cap) else "hbm"


def solver_class(D):
    """The solver bt_assign picks on the device for D columns."""
    for nc in (1, 2, 4, 8):
        if D + 1 <= 64 * nc:
            return "wave<%d>" % nc
    return "block"


# ------------------------------------------------------------------------------------------------ expected messages
def _arrays(fr):
    return (np.asarray(fr["boxes"], np.float64).reshape(-1, 4), np.asarray(fr["scores"], np.float64).reshape(-1),
            np.asarray(fr["ids"], np.int64).reshape(-1))


class CapOracle:
    """oracle.bytetrack.BYTETracker under the capacity rules of bytetrack_update:
      more than max_dets rows        the first max_dets are used, err |= 1
      more candidates than slots     slots in use = tracks in the tracked or lost list when the frame starts; the first n_free new tracks (in
                                     detection order) take the ids, the others are dropped, err |= 2: the oracle fed the frame without them
      a ninth class on one track     err |= 4 (the device leaves the vote alone; the cases keep the oracle's winner unchanged too)
    err is sticky until reset()."""

    def __init__(self, cap):
        self.t = bytetrack.BYTETracker()
        self.MT, self.MD = cap
        self.err = 0

    def reset(self):
        self.t.reset()
        self.err = 0

    def update(self, fr):
        b, s, c = _arrays(fr)
        if len(s) > self.MD:
            self.err |= ERR_DET
            b, s, c = b[:self.MD], s[:self.MD], c[:self.MD]
        n_free = self.MT - len(self.t.tracked_stracks) - len(self.t.lost_stracks)
        if int((s >= self.t.det_thresh).sum()) > n_free:
            trial = copy.deepcopy(self.t)
            trial.update(b, s, c)
            n_new = trial._count - self.t._count
            if n_new > n_free:
                self.err |= ERR_TRACK
                born = {t.track_id: t for t in trial.tracked_stracks + trial.lost_stracks if t.track_id > self.t._count}
                assert len(born) == n_new, "a new track left both lists on its first frame: the case cannot name the dropped rows"
                keep = np.ones(len(s), bool)
                for tid in range(self.t._count + n_free + 1, trial._count + 1):
                    t = born[tid]
                    tlwh = b.copy()
                    tlwh[:, 2:] -= tlwh[:, :2]
                    hit = np.nonzero(keep & (tlwh == t._tlwh).all(1) & (s == t.score) & (c == t.class_id))[0]
                    keep[hit[0]] = False
                b, s, c = b[keep], s[keep], c[keep]
        snap = self.t.update(b, s, c)
        if any(len(t.class_id_history) > HIST for t in self.t.tracked_stracks + self.t.lost_stracks):
            self.err |= ERR_HIST
        return snap, self.err


def expected(steps, cap):
    """[(snapshot, err)] per frame step, and the oracle as the last frame left it (its STrack.trajectories)."""
    o = CapOracle(cap)
    out = []
    for st in steps:
        if isinstance(st, str):
            o.reset()
        else:
            out.append(o.update(st))
    return out, o.t


def oracle_trajectories(t):
    """STrack.trajectories in message order (tracked, then lost): list of (len, 4) arrays."""
    return [np.asarray(k.trajectories, np.float64).reshape(-1, 4) for k in t.tracked_stracks + t.lost_stracks]


class Recorder:
    """A stand-in for oracle.bytetrack.lapjv_extended that solves with `solve` and keeps (cost, limit, x, y) of every call."""

    def __init__(self, solve):
        self.solve, self.calls = solve, []

    def __call__(self, cost, limit):
        x, y = self.solve(cost, limit)
        self.calls.append((np.array(cost, np.float64), float(limit), np.asarray(x).copy(), np.asarray(y).copy()))
        return x, y


# ------------------------------------------------------------------------------------------------ a. contested size-class scenes
STEP_X, STEP_Y, ROW = 34, 56, 32        # lattice: neighbours in a row overlap (boxes are 56..72 wide), rows do not (40..50 high)
SHIFT = 17                              # detections sit half a step beside a site, between two tracks

# (T, D): the solver f1's first association must reach; D + 1 on both sides of 64, 128, 256, 512, then the block solver.  (100, 130) is
# the scene the micro-batched launch of tests/test_gpu_track_edges.py carries mid-batch.
CONTESTED = [(70, 63), (64, 64), (100, 127), (128, 128), (100, 130), (255, 255), (200, 256), (511, 511), (512, 512), (300, 513), (600, 700)]
SOLVER = {(70, 63): "wave<1>", (64, 64): "wave<2>", (100, 127): "wave<2>", (128, 128): "wave<4>", (100, 130): "wave<4>", (255, 255): "wave<4>",
          (200, 256): "wave<8>", (511, 511): "wave<8>", (512, 512): "block", (300, 513): "block", (600, 700): "block"}
SIDE = {}                               # (T, D, cap) -> "lds" | "hbm", filled below
SEEDS = {}                              # (T, D) -> seed, filled below


def caps_of(T, D):
    return [BIG, DEFAULT] if T <= 255 and D <= 255 else [BIG]


for _T, _D in CONTESTED:
    for _cap in caps_of(_T, _D):
        SIDE[(_T, _D, _cap)] = cost_side(_T, _D, _cap)


def _site(k):
    return 100.0 + STEP_X * (k % ROW), 100.0 + STEP_Y * (k // ROW)


def _box(rng, cx, cy):
    w, h = rng.uniform(56, 72), rng.uniform(40, 50)
    return [int(cx - w / 2), int(cy - h / 2), int(cx + w / 2), int(cy + h / 2)]


def _score(rng, lo, hi):
    return float(np.float32(rng.uniform(lo, hi)))      # through float32, as synth.track_scene


def _beside(rng, sites, lo, hi):
    rows = []
    for k in sites:
        cx, cy = _site(int(k))
        cx += SHIFT * (1 if rng.uniform() < 0.5 else -1)
        j = rng.normal(0, 3, 2)
        rows.append((_box(rng, cx + j[0], cy + j[1]), _score(rng, lo, hi), int(rng.integers(0, 3))))
    return rows


def _frame(rows):
    return dict(boxes=[r[0] for r in rows], scores=[r[1] for r in rows], ids=[r[2] for r in rows])


def contested(seed, T, D, n_lo):
    """Frames f0..f3.  f0: T boxes on lattice sites 0..T-1, scores over det_thresh, so frame 1 activates T tracks.  f1, f2: exactly D rows
    over track_thresh, each half a step beside one of D distinct sites (all of the track sites first when D > T), and n_lo rows in
    (0.1, 0.5) beside track sites; shuffled.  f3 is f0 again."""
    rng = np.random.default_rng(seed)
    f0 = _frame([(_box(rng, *_site(k)), _score(rng, 0.62, 0.95), int(rng.integers(0, 3))) for k in range(T)])
    frames = [f0]
    for _ in range(2):
        sites = rng.permutation(T)[:D] if D <= T else np.arange(D)
        rows = _beside(rng, sites, 0.52, 0.95) + _beside(rng, rng.permutation(T)[:n_lo] if n_lo <= T else rng.integers(0, T, n_lo), 0.12, 0.48)
        frames.append(_frame([rows[i] for i in rng.permutation(len(rows))]))
    frames.append(copy.deepcopy(f0))
    return frames


def n_lo_of(D, cap):
    """D // 4 low-score rows, or as many as max_dets leaves room for beside the D high ones: (255, 255) on the default tracker has one."""
    return min(D // 4, cap[1] - D)


@functools.lru_cache(maxsize=None)
def contested_case(T, D, cap):
    return dict(name="contested-%d-%d@%d" % (T, D, cap[0]), steps=contested(SEEDS[(T, D)], T, D, n_lo_of(D, cap)))


# ------------------------------------------------------------------------------------------------ b. tie scenes
TIE_SCORE = 0.875
# D -> the tied column pairs placed on purpose (j, j'); every other column is paired with its neighbour
TIE_PAIRS = {
    100: [(3, 9), (40, 70)],                          # wave<2>: one group;  j' in group 1 on lane 6, below j's lane 40
    130: [(3, 9), (40, 128)],                         # wave<4>: one group;  j' = 128 >= j + 64 on lane 0
    300: [(3, 9), (40, 138), (100, 290)],             # wave<8>: one group;  lanes 10 < 40 and 34 < 36, two and three groups up
    600: [(3, 9), (40, 138), (10, 266), (300, 580)],  # block: one wave;  waves 0 and 2 of pass 0;  thread 10 on passes 0 and 1;  passes 1 and 2
}


def pair_columns(D):
    """All D columns in pairs (j < j'): TIE_PAIRS[D] first, then the remaining columns two by two in order."""
    special = TIE_PAIRS[D]
    taken = {c for p in special for c in p}
    rest = [c for c in range(D) if c not in taken]
    return list(special) + [(rest[i], rest[i + 1]) for i in range(0, len(rest), 2)]


def _unit_box(k, dx=0, dy=0):
    x, y = 200 + 256 * (k % 24) + dx, 200 + 256 * (k // 24) + dy
    return [x, y, x + 64, y + 64]


def _rows(boxes, score, ids):
    return dict(boxes=[list(b) for b in boxes], scores=[score] * len(boxes), ids=list(ids))


def tie_dupdet(D, score=TIE_SCORE):
    """Every track gets two identical boxes: at column j with class 1, at column j' with class 2.  With score < track_thresh the tie
    is in the second association (limit 0.5, plain IoU) and the frame has no high-score row at all."""
    pairs = pair_columns(D)
    f1 = _rows([_unit_box(k) for k in range(len(pairs))], TIE_SCORE, [0] * len(pairs))
    boxes, ids = [None] * D, [0] * D
    for k, (j, jp) in enumerate(pairs):
        boxes[j], boxes[jp], ids[j], ids[jp] = _unit_box(k), _unit_box(k), 1, 2
    f2 = _rows(boxes, score, ids)
    return [f1, f2, copy.deepcopy(f2)]


def tie_duptrk(D):
    """Two identical frame-1 rows become two tracks with consecutive ids, for every column named in TIE_PAIRS[D]; then one detection
    per column arrives.  The tie is between two ROWS: the earlier row keeps the column because an equal slack does not replace a path."""
    dup = {c for p in TIE_PAIRS[D] for c in p}
    b1 = []
    for c in range(D):
        b1 += [_unit_box(c)] * (2 if c in dup else 1)
    f1 = _rows(b1, TIE_SCORE, [0] * len(b1))
    f2 = _rows([_unit_box(c) for c in range(D)], TIE_SCORE, [1 + c % 2 for c in range(D)])
    return [f1, f2, copy.deepcopy(f2)]


def tie_sym(D):
    """2 x 2 blocks: tracks A at (0, 0) and B at (32, 0), detections at (16, -8) in column j (class 1) and (16, +8) in column j'
    (class 2).  All four IoUs are 2688 / 5504, so both perfect matchings cost the same."""
    pairs = pair_columns(D)
    b1 = []
    for k in range(len(pairs)):
        b1 += [_unit_box(k), _unit_box(k, 32, 0)]
    f1 = _rows(b1, TIE_SCORE, [0] * len(b1))
    boxes, ids = [None] * D, [0] * D
    for k, (j, jp) in enumerate(pairs):
        boxes[j], boxes[jp], ids[j], ids[jp] = _unit_box(k, 16, -8), _unit_box(k, 16, 8), 1, 2
    f2 = _rows(boxes, TIE_SCORE, ids)
    return [f1, f2, copy.deepcopy(f2)]


@functools.lru_cache(maxsize=None)
def tie_cases():
    """name -> (steps, the rule a changed solver must differ by: "last" column or "relax"ed path comparison)."""
    out = {}
    for D in sorted(TIE_PAIRS):
        out["dupdet-%d" % D] = (tie_dupdet(D), "last")
        out["duptrk-%d" % D] = (tie_duptrk(D), "relax")
        out["sym-%d" % D] = (tie_sym(D), "last")
    out["dupdet-lo-100"] = (tie_dupdet(100, 0.375), "last")      # the tie in the second association
    return out


# ------------------------------------------------------------------------------------------------ c. degenerate shapes
def _loose(seed, n, lo=0.62, hi=0.95, x0=0):
    """n well separated boxes of distinct sizes."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        cx, cy = x0 + 150 + 190 * (k % 6) + rng.uniform(-5, 5), 150 + 170 * (k // 6) + rng.uniform(-5, 5)
        w, h = rng.uniform(50, 120), rng.uniform(50, 110)
        rows.append(([int(cx - w / 2), int(cy - h / 2), int(cx + w / 2), int(cy + h / 2)], _score(rng, lo, hi), int(rng.integers(0, 3))))
    return rows


def _nudge(rows, seed, lo=0.52, hi=0.95):
    rng = np.random.default_rng(seed)
    out = []
    for b, _, c in rows:
        j = rng.integers(-4, 5, 4)
        out.append(([int(b[0] + j[0]), int(b[1] + j[1]), int(b[2] + j[2]), int(b[3] + j[3])], _score(rng, lo, hi), c))
    return out


EMPTY = dict(boxes=[], scores=[], ids=[])


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    a = _loose(1, 7)
    far = _loose(2, 3, x0=1400)
    on_thresh = [(b, 0.5, c) for b, _, c in _nudge(a, 5)]
    return {
        # T = 0, D > 0 on frame 1 and again after reset
        "no-tracks": [_frame(a), "reset", _frame(_nudge(a, 3, 0.62)), _frame(_nudge(a, 4))],
        # D = 0, T > 0: every track goes to lost; they come back
        "no-dets": [_frame(a), copy.deepcopy(EMPTY), copy.deepcopy(EMPTY), _frame(_nudge(a, 3))],
        # both zero, then first boxes on frame 3 (not activated at birth), confirmed on frame 4
        "nothing": [copy.deepcopy(EMPTY), copy.deepcopy(EMPTY), _frame(a), _frame(_nudge(a, 3))],
        # n_lo = 0 with unmatched tracks: the second association has rows and no column
        "no-low-band": [_frame(a), _frame(_nudge(a[:4], 3)), _frame(_nudge(a, 4))],
        # unconfirmed tracks (born on frame 2) with no detection left on frame 3: all removed
        "unconfirmed-alone": [_frame(a), _frame(_nudge(a, 3, 0.62) + far), _frame(_nudge(a, 4)), _frame(_nudge(a, 5) + _nudge(far, 6, 0.62))],
        # every score equals track_thresh: neither band
        "on-threshold": [_frame(a), _frame(on_thresh), _frame(_nudge(a, 6))],
    }


# ------------------------------------------------------------------------------------------------ d. capacity
@functools.lru_cache(maxsize=None)
def capacity_cases():
    """name -> (cap, steps, err after each frame, entry): entry "device" needs adas_bytetrack_update_device (update_host refuses
    more than max_dets rows)."""
    a12 = _loose(11, 12)
    one = _loose(12, 1)[0]
    hist = [_frame([(one[0], one[1], c)]) for c in (0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 0)]
    small = _frame(_loose(13, 3))
    return {
        # 12 candidates, 8 slots: ids 1..8 go to the first eight, twice; reset clears err
        "track-overflow": ((8, 16), [_frame(a12), _frame(_nudge(a12, 3, 0.62)), "reset", small], [2, 2, 0], "host"),
        # 12 rows, max_dets 8: the first eight rows are the frame; err stays on the next, legal frame
        "det-overflow": ((8, 8), [_frame(a12), _frame(_nudge(a12[:8], 3))], [1, 1], "device"),
        # one track, nine distinct classes: the ninth sets the bit and leaves the vote (class 0, the first with two) alone
        "hist-overflow": ((8, 8), hist, [0] * 9 + [4, 4], "host"),
    }


# seeds of the contested scenes: the first seed from 1 upwards at which scipy and lap_ref("first") agree on every association of every
# frame under every capacity of the pair (tests/test_track_cases_cpu.py asserts it)
SEEDS.update({(70, 63): 1, (64, 64): 1, (100, 127): 1, (128, 128): 1, (100, 130): 1, (255, 255): 1, (200, 256): 1, (511, 511): 1, (512, 512): 1,
              (300, 513): 1, (600, 700): 1})
