"""Frames, bird-view images and sprites of the UI-panel tests (tests/panels_ref.py, tests/golden/make_golden_panels.py, the host build and
the GPU tests): every byte is a closed integer formula of (row, column, channel, seed) in uint64 arithmetic, not an RNG stream, so the
golden generator and the tests rebuild identical bytes on any NumPy.  No reference dependency."""
import numpy as np

# the sprite slots in the order of ADAS_PANEL_SPRITE_* with the sizes ControlPanel.__init__ resizes its assets to (demo.py:57-74), (w, h)
SPRITES = (("fcws_warning", 100, 100), ("fcws_prompt", 100, 100), ("fcws_normal", 100, 100), ("left", 200, 200), ("right", 200, 200),
           ("straight", 200, 200), ("warn", 200, 200), ("lta_left", 300, 200), ("lta_right", 300, 200))
# name -> the attribute ControlPanel keeps it under, and the asset file it reads it from
REF_ATTR = {"fcws_warning": "collision_warning_img", "fcws_prompt": "collision_prompt_img", "fcws_normal": "collision_normal_img",
            "left": "left_curve_img", "right": "right_curve_img", "straight": "keep_straight_img", "warn": "determined_img",
            "lta_left": "left_lanes_img", "lta_right": "right_lanes_img"}
REF_FILE = {"fcws_warning": "FCWS-warning.png", "fcws_prompt": "FCWS-prompt.png", "fcws_normal": "FCWS-normal.png", "left": "left_turn.png",
            "right": "right_turn.png", "straight": "straight.png", "warn": "warn.png", "lta_left": "LTA-left_lanes.png",
            "lta_right": "LTA-right_lanes.png"}
OFFSETS = ("UNKNOWN", "RIGHT", "LEFT", "CENTER")                                               # ADAS_OFFSET_*
CURVATURES = ("UNKNOWN", "STRAIGHT", "EASY_LEFT", "HARD_LEFT", "EASY_RIGHT", "HARD_RIGHT")     # ADAS_CURVATURE_*
COLLISIONS = ("UNKNOWN", "NORMAL", "PROMPT", "WARNING")                                        # ADAS_COLLISION_*
LATCHES = (None, "Left", "Right", "Straight")                                                  # ADAS_PANEL_LATCH_*
SIZES = ((368, 416), (720, 1280))      # (rows, columns) of the golden's frames; the bird image of each is BIRD_HW
BIRD_HW = {(368, 416): (368, 416), (720, 1280): (720, 1280), (367, 403): (77, 131)}


def _mix(h, w, c, seed):
    """uint32 hash of (row, column, channel, seed) as an (h, w, c) uint64 array."""
    r = np.arange(h, dtype=np.uint64).reshape(h, 1, 1)
    q = np.arange(w, dtype=np.uint64).reshape(1, w, 1)
    k = np.arange(c, dtype=np.uint64).reshape(1, 1, c)
    m = np.uint64(0xffffffff)
    x = (r * np.uint64(7919) + q * np.uint64(104729) + k * np.uint64(1299709) + np.uint64(int(seed) * 15485863 + 12345)) & m
    x = ((x ^ (x >> np.uint64(15))) * np.uint64(2246822519)) & m
    x = ((x ^ (x >> np.uint64(13))) * np.uint64(3266489917)) & m
    return x ^ (x >> np.uint64(16))


def image(h, w, seed):
    """(h, w, 3) uint8: bytes over the whole range, 255 and odd values among them (v >> 1 is not v / 2 rounded)."""
    return (_mix(h, w, 3, seed) & np.uint64(255)).astype(np.uint8)


def frames(n, hw, seed=0):
    return np.stack([image(hw[0], hw[1], 1000 + 17 * seed + f) for f in range(n)])


def bird(hw, seed=0):
    bh, bw = BIRD_HW[tuple(hw)]
    return image(bh, bw, 5000 + seed)


def sprite(w, h, seed):
    """(h, w, 4) uint8 BGRA.  Alpha is non-zero on about half of the pixels; channel 2 is zero on about a quarter of them, independently of alpha,
    so 'alpha != 0' and 'channel 2 != 0' select different pixels in both directions."""
    x = _mix(h, w, 4, 9000 + seed)
    s = x.astype(np.uint64)
    out = (s & np.uint64(255)).astype(np.uint8)
    sel = _mix(h, w, 1, 9500 + seed)[:, :, 0]
    out[:, :, 3] = np.where((sel & np.uint64(1)) != 0, 128 + ((sel >> np.uint64(1)) & np.uint64(127)), 0).astype(np.uint8)
    out[:, :, 2] = np.where(((sel >> np.uint64(8)) & np.uint64(3)) == 0, 0, out[:, :, 2] | 1).astype(np.uint8)
    return out


def sprites():
    """{name: (h, w, 4) uint8} for the nine slots."""
    return {name: sprite(w, h, i) for i, (name, w, h) in enumerate(SPRITES)}


SMALL = (368, 416)


def transition_frame():
    """The frame every one of the golden's 96 transitions starts from."""
    return image(SMALL[0], SMALL[1], 1)


def collision_frame(hw):
    return image(hw[0], hw[1], 2)


def bird_frame(hw):
    return image(hw[0], hw[1], 3)


def sequence_frame(i):
    """(frame, bird image) of frame i of the golden's sequence."""
    return image(SMALL[0], SMALL[1], 100 + i), bird(SMALL, i % 3)


def latch_pairs(transitions):
    """{(latch before, latch after)} of rows [latch before, offset, curvature, latch after, ...]."""
    return {(t[0], t[3]) for t in transitions}


def two_sprite_rows(transitions):
    """Rows where the reference's first chain paints a turn sign and its second chain paints straight over it: latch Left or Right going in,
    curvature STRAIGHT (which keeps the latched sign in the first chain), offset neither RIGHT nor LEFT, latch Straight coming out."""
    return [t for t in transitions if t[0] in (1, 2) and t[2] == 1 and t[1] in (0, 3) and t[3] == 3]


def sequence(n=40):
    """n frames of (offset, curvature, collision) indices that walk through every latch value, both LTA signs and a two-sprite frame."""
    seq = []
    cur = [3, 2, 0, 1, 0, 4, 5, 2, 1, 1, 3, 0, 5, 0, 0, 1, 3, 1, 5, 2]      # HARD_LEFT latches Left, EASY_LEFT keeps it, STRAIGHT over it, ...
    off = [0, 3, 3, 1, 2, 0, 3]
    for i in range(n):
        seq.append((off[(i * 3 + i // 7) % len(off)], cur[i % len(cur)], (i * 5 + i // 4) % 4))
    return seq
