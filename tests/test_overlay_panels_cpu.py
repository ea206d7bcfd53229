"""CPU: the demo's three UI panels (csrc/overlay_panel_core.h, rules P1-P6).  Three layers: the golden -- the reference's own ControlPanel,
lifted from demo.py and run under stubs (tests/golden/panels.json.gz) -- pins the NumPy restatement (tests/panels_ref.py), every hash and
every latch; the restatement pins the host build of the header the kernels include (tests/hostemu/emu_overlay_panels.cpp), every record
and every byte; hand-derived known answers pin both.  Every comparison is equality.
What the golden pins: the signs and collision panels and the bird panel's placement are the reference's own lines; the resize inside the
bird panel is the project's restatement on both sides (oracle.preprocess.cv_resize_linear_u8): unpinned, as in pre-processing."""
import gzip, json, os

import numpy as np
import pytest

import panels_ref as ref
import panel_scene as PS
import emu_overlay_panels_api as emu
from oracle.preprocess import cv_resize_linear_u8

HERE = os.path.dirname(os.path.abspath(__file__))
ODD = (367, 403)


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "panels.json.gz"), "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sprites():
    return PS.sprites()


def test_scene_sprites_separate_the_two_mask_rules(sprites):
    for name, s in sprites.items():
        a, c2 = s[:, :, 3] != 0, s[:, :, 2] != 0
        assert 0.4 < a.mean() < 0.6, name
        assert (a & ~c2).any() and (~a & c2).any(), name


def test_golden_holds_every_latch_pair_and_a_two_sprite_frame(golden):
    t = golden["transitions"]
    assert len(t) == 96 and len({(r[0], r[1], r[2]) for r in t}) == 96
    assert PS.latch_pairs(t) == {(a, b) for a in range(4) for b in range(4)}
    assert PS.two_sprite_rows(t)
    assert len(golden["sequence"]) == 40 and {s["latch"] for s in golden["sequence"]} == {0, 1, 2, 3}
    assert [(s["offset"], s["curvature"], s["collision"]) for s in golden["sequence"]] == PS.sequence(40)
    assert len(golden["puttext"]) == 40 and all(len(c) == 6 for c in golden["puttext"])


def test_restatement_reproduces_the_96_transitions(golden, sprites):
    base = PS.transition_frame()
    two = 0
    for latch, off, cur, after, sha in golden["transitions"]:
        img = base.copy()
        names, got = ref.signs_panel(img, sprites, latch, off, cur)
        assert got == after, (latch, off, cur)
        assert ref.sha(img) == sha, (latch, off, cur)
        two += names[0] is not None and names[1] is not None
    assert two >= len(PS.two_sprite_rows(golden["transitions"])) > 0


def test_restatement_reproduces_collision_bird_and_the_sequence(golden, sprites):
    for hw in PS.SIZES:
        key = "%dx%d" % (hw[1], hw[0])
        for col in range(4):
            img = PS.collision_frame(hw)
            ref.collision_panel(img, sprites, col)
            assert ref.sha(img) == golden["collision"][key][col], (key, col)
        img = PS.bird_frame(hw)
        ref.bird_panel(img, PS.bird(hw))
        assert ref.sha(img) == golden["bird"][key], key
    latch = 0
    for i, s in enumerate(golden["sequence"]):
        img, bv = PS.sequence_frame(i)
        out, rec = ref.compose(img, sprites, latch, s["offset"], s["curvature"], s["collision"], bv)
        latch = rec["latch"]
        assert latch == s["latch"] and ref.sha(out) == s["sha"], i


def test_header_choice_functions_equal_the_golden(golden):
    for latch, off, cur, after, _ in golden["transitions"]:
        a, b, got = emu.choose(latch, off, cur)
        assert got == after, (latch, off, cur)
        names, _ = ref.choose_signs(latch, off, cur)
        assert [a, b] == names, (latch, off, cur)
    assert [emu.choose_collision(c) for c in range(4)] == [None, "fcws_normal", "fcws_prompt", "fcws_warning"]
    # a value outside its enum is UNKNOWN
    assert emu.choose(1, 9, -1) == emu.choose(1, 0, 0) == ("warn", None, 0)
    assert emu.choose_collision(4) is None and emu.choose_collision(-3) is None
    # the issue's example: latch Left plus STRAIGHT paints left_turn, then straight over it, and the latch becomes Straight
    assert emu.choose(1, 0, 1) == ("left", "straight", 3)


@pytest.mark.parametrize("hw", [PS.SMALL, ODD, (720, 1280)], ids=lambda hw: "%dx%d" % (hw[1], hw[0]))
def test_header_fold_equals_the_restatement(hw, sprites):
    """Every byte of frames through all three panels, and each panel alone; 416 x 368: the signs widget dims part of the bird panel;
    403 x 367 with a 131 x 77 bird image: non-integer ratios, an upscale, an odd row stride."""
    bv = PS.bird(hw)
    cases = [(7, 1, 0, 1, 3), (7, 0, 1, 0, 2), (7, 3, 3, 2, 1), (1, 0, 0, 0, 0), (2, 2, 2, 4, 0), (4, 0, 0, 0, 3), (6, 1, 3, 1, 0)]
    if hw == (720, 1280):
        cases = cases[:2] + cases[3:6]
    for i, (panels, latch, off, cur, col) in enumerate(cases):
        img = PS.image(hw[0], hw[1], 40 + i)
        want, wrec = ref.compose(img, sprites, latch, off, cur, col, bv, panels)
        got, grec = emu.frame(img, sprites, latch, off, cur, col, bv if panels & 1 else None, panels)
        assert grec == wrec, (panels, latch, off, cur, col)
        assert np.array_equal(got, want), (panels, latch, off, cur, col, np.argwhere(got != want)[:5])
        outside = ~ref.panel_pixels(hw, sprites, panels)
        if not (panels & 4):      # the collision sprite may reach below its widget
            assert np.array_equal(got[outside], img[outside])
    if hw == PS.SMALL:
        W, H = ref.geometry(hw, ref.DEFAULTS)
        assert hw[1] - W - 20 < 400, "the panels of this size are meant to overlap"


@pytest.mark.parametrize("hw", [PS.SMALL, ODD, (720, 1280)], ids=lambda hw: "%dx%d" % (hw[1], hw[0]))
def test_header_resize_equals_the_oracle(hw):
    bv = PS.bird(hw)
    W, H = ref.geometry(hw, ref.DEFAULTS)
    assert np.array_equal(emu.resize(bv, (W, H)), cv_resize_linear_u8(bv, (W, H)))
    same = PS.image(H, W, 77)      # a bird image that already is W x H: a copy
    assert np.array_equal(emu.resize(same, (W, H)), same) and np.array_equal(cv_resize_linear_u8(same, (W, H)), same)


@pytest.mark.parametrize("hw, align", [(PS.SMALL, 0), (PS.SMALL, 5), (ODD, 0), (ODD, 9), (ODD, 15), ((720, 1280), 3)],
                         ids=lambda v: str(v).replace(" ", ""))
def test_header_pieces_equal_the_restatement(hw, align, sprites):
    """The draw pass's 16-byte pieces on a buffer at every kind of alignment: two streams x two frames, the latch walking each stream's frames
    in order; every piece is taken once and lies in the buffer (the emulation reports either), and every byte equals the restatement."""
    S, B = 2, (1 if hw == (720, 1280) else 2)
    frames = PS.frames(S * B, hw, seed=3)
    birds = np.stack([PS.image(*PS.BIRD_HW[hw], 600 + f) for f in range(S * B)])
    off, cur, col = [0, 1, 3, 0][:S * B], [3, 5, 1, 1][:S * B], [3, 2, 1, 0][:S * B]
    got, recs, lat = emu.run(frames, sprites, [0, 3], off, cur, col, S, B, birds, 7, align)
    latch = [0, 3]
    for b in range(B):
        for s in range(S):
            q = b * S + s
            want, wrec = ref.compose(frames[q], sprites, latch[s], off[q], cur[q], col[q], birds[q])
            latch[s] = wrec["latch"]
            assert recs[q] == wrec, q
            assert np.array_equal(got[q], want), (q, np.argwhere(got[q] != want)[:5])
    assert list(lat) == latch


def test_known_answers_widgets(sprites):
    """Hand-derived: both widgets' border rows and columns, the last row and column dimmed and not red, 255 >> 1 == 127."""
    hw = (720, 1280)
    img = np.full(hw + (3,), 255, np.uint8)
    img[100, 200] = (1, 2, 251)
    empty = {}
    for fn in (lambda: emu.frame(img, empty, 0, 1, 2, 0, None, 6)[0], lambda: ref.compose(img, empty, 0, 1, 2, 0, None, 6)[0]):
        out = fn()
        red, dim = (0, 0, 255), (127, 127, 127)
        # signs widget: rows 0..364, columns 0..399
        for r in (0, 1, 2, 362, 363):
            assert (out[r, :400] == red).all(), r
        for c in (0, 1, 2, 397, 398):
            assert (out[:365, c] == red).all(), c
        assert tuple(out[364, 200]) == dim and tuple(out[200, 399]) == dim and tuple(out[364, 399]) == dim      # last row / column: only dimmed
        assert tuple(out[3, 3]) == dim and tuple(out[361, 396]) == dim
        assert tuple(out[100, 200]) == (0, 1, 125)
        assert tuple(out[365, 10]) == (255, 255, 255) and tuple(out[10, 400]) == (255, 255, 255)
        # collision widget: W = 320, H = 180: rows 200..359, columns 940..1279 (160 x 340)
        for r in (200, 201, 202, 357, 358):
            assert (out[r, 940:] == red).all(), r
        for c in (940, 941, 942, 1277, 1278):
            assert (out[200:360, c] == red).all(), c
        assert tuple(out[359, 1000]) == dim and tuple(out[300, 1279]) == dim and tuple(out[203, 943]) == dim
        assert tuple(out[199, 1000]) == (255, 255, 255) and tuple(out[360, 1000]) == (255, 255, 255) and tuple(out[300, 939]) == (255, 255, 255)


def test_known_answers_bird_border_and_sprite_masks():
    """Hand-derived: the bird panel's black border and copied interior; one sprite pixel per mask rule."""
    hw = (720, 1280)
    img = np.full(hw + (3,), 200, np.uint8)
    bv = np.full((180, 320, 3), 9, np.uint8)      # already W x H: a copy
    bv[0, 0] = (1, 2, 3)
    spr = np.zeros((200, 200, 4), np.uint8)
    spr[5, 7] = (10, 20, 0, 255)        # alpha set, channel 2 zero: painted by the alpha rule
    spr[6, 7] = (10, 20, 30, 0)         # alpha zero, channel 2 set: not painted by the alpha rule
    lta = np.zeros((200, 300, 4), np.uint8)
    lta[5, 7] = (10, 20, 0, 255)        # not painted by the channel-2 rule
    lta[6, 7] = (11, 21, 31, 0)         # painted by the channel-2 rule
    fc = np.zeros((100, 100, 4), np.uint8)
    fc[99, 99] = (4, 5, 6, 1)
    sp = {"left": spr, "lta_left": lta, "fcws_prompt": fc}
    for fn in (lambda *a: emu.frame(*a)[0], lambda *a: ref.compose(*a)[0]):
        out = fn(img, sp, 0, 0, 3, 2, bv, 7)          # HARD_LEFT: left; offset UNKNOWN: no LTA sign; PROMPT
        assert (out[0:10, 940:] == 0).all() and (out[190:200, 940:] == 0).all() and (out[0:200, 940:950] == 0).all() and (out[0:200, 1270:] == 0).all()
        assert tuple(out[10, 950]) == (1, 2, 3) and tuple(out[189, 1269]) == (9, 9, 9)
        assert tuple(out[15, 107]) == (10, 20, 0) and tuple(out[16, 107]) == (100, 100, 100)          # row y + 10, column x + 200 - 100
        assert tuple(out[180 + 50 + 99, 1280 - 320 - 5 + 99]) == (4, 5, 6)                                # row H + y + 50, column src_w - W - 5 + x
        out = fn(img, sp, 0, 1, 2, 0, None, 2)        # offset RIGHT: LTA-left_lanes
        assert tuple(out[15, 57]) == (100, 100, 100) and tuple(out[16, 57]) == (11, 21, 31)             # column x + 200 - 150


def test_geometry_refusals(sprites):
    assert emu.fit(PS.SMALL, sprites) == ("ok", None) and emu.fit(ODD, sprites) == ("ok", None) and emu.fit((720, 1280), sprites) == ("ok", None)
    assert emu.fit((720, 399), sprites)[0] == "signs"
    wide = dict(sprites, fcws_prompt=np.zeros((100, 110, 4), np.uint8))      # W + 5 = 109 at 416 columns
    assert emu.fit(PS.SMALL, wide) == ("collision_sprite", "fcws_prompt")
    assert emu.fit((80, 1280), {}, signs_h=60) == ("collision", None)        # H = 20: no row between H + 20 and 2H
    assert emu.fit((720, 1280), {}, border=500)[0] == "bird"
    assert emu.fit((720, 1280), dict(sprites, warn=np.zeros((800, 200, 4), np.uint8))) == ("sign_sprite", "warn")
