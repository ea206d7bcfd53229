"""GPU: the overlay's text (csrc/overlay_text.hip) through the C ABI and postproc.LaneOverlay against the NumPy restatement (tests/text_ref.py),
which tests/test_overlay_text_cpu.py pins to the host build of the same rules and to Python's own number formatting: every byte, every item
field, every flag, no tolerances."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import text_ref as R
import text_scene as TS

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")

INVALID = -1        # ADAS_ERR_INVALID
GUARD = 0xA5


@pytest.fixture(scope="module")
def fonts():
    return TS.fonts()


def make_overlay(hw, max_batch, fonts, scene, style=TS.STYLE):
    ov = PP.LaneOverlay(hw, None, max_batch)
    ov.set_fonts(fonts)
    ov.set_text_style(**style)
    ov.set_class_colors("detections", scene["det_colors"])
    ov.set_class_colors("tracks", scene["trk_colors"])
    ov.set_text_labels("detections", scene["det_names"])
    ov.set_text_labels("tracks", scene["trk_names"])
    ov.set_text_lines(scene["lines"])
    return ov


def device_run(ov, frames, scenes, mask, guard=0, n_streams=None, n_frames=1):
    """-> (frames after, the whole buffer with its guards, [items], [flags])"""
    a, caps = TS.pack_scenes(scenes)
    bufs = {k: L.DeviceBuffer.from_array(v) for k, v in a.items()}
    rows = frames.shape[2] * 3 * 2                     # two guard rows before and after, and `guard` bytes to shift the alignment
    host = np.full(frames.nbytes + 2 * rows + guard, GUARD, np.uint8)
    at = rows + guard
    host[at:at + frames.nbytes] = frames.reshape(-1)
    d = L.DeviceBuffer.from_array(host)
    ov.run_text_arrays(d.ptr + at, mask, len(scenes) if n_streams is None else n_streams, n_frames, None, caps[0], caps[1], caps[2],
                       **{k: b.ptr for k, b in bufs.items()})
    back = d.download(host.shape, np.uint8)
    items = [ov.text_items(q) for q in range(len(scenes))]
    flags = [ov.text_flags(q) for q in range(len(scenes))]
    for b in list(bufs.values()) + [d]:
        b.free()
    return back[at:at + frames.nbytes].reshape(frames.shape), (back[:at], back[at + frames.nbytes:]), items, flags


def got_tuple(it):
    return (int(it["kind"]), int(it["source"]), int(it["x"]), int(it["y"]), int(it["x1"]), int(it["y1"]), tuple(int(v) for v in it["box"]), int(it["slot"]),
            tuple(int(v) for v in it["color"]), bytes(it["text"])[:int(it["len"])].decode("latin-1"))


def check(frames, scenes, fonts, mask, got, guards, items, flags, style=TS.STYLE):
    H, W = frames.shape[1:3]
    assert (guards[0] == GUARD).all() and (guards[1] == GUARD).all(), "a guard byte was written"
    for q, s in enumerate(scenes):
        w_items, w_flags = R.layout(s, fonts, W, H, mask, style)
        assert [got_tuple(i) for i in items[q]] == [TS.item_tuple(i) for i in w_items], q
        assert flags[q] == w_flags, q
        want = R.paint(frames[q].copy(), w_items, fonts)
        assert np.array_equal(got[q], want), (q, np.argwhere(got[q] != want)[:5])
        outside = np.ones((H, W), bool)                # bytes outside every item's clipped box are the input's
        for i in w_items:
            outside[i["box"][1]:i["box"][3], i["box"][0]:i["box"][2]] = False
        assert np.array_equal(got[q][outside], frames[q][outside]), q


@pytest.mark.parametrize("guard", (0, 1, 15))
@pytest.mark.parametrize("hw", ((37, 101), (16, 64)))
def test_small_frames_every_scene_batch_1_and_3(fonts, hw, guard):
    H, W = hw
    edges, m_edges = TS.scene_edges(W, H)
    ov = make_overlay(hw, 3, fonts, edges)
    frames = TS.background(3, H, W)
    share = lambda s: dict(s, lines=edges["lines"])    # the handle's lines are shared by its frames
    labels, overflow, full = share(TS.scene_labels(W, H)[0]), share(TS.scene_overflow(W, H)[0]), share(TS.scene_full(W, H, seed=3)[0])
    check(frames[:1], [edges], fonts, m_edges, *device_run(ov, frames[:1], [edges], m_edges, guard))                       # batch 1
    scenes = [labels, overflow, full]                                                                                       # batch 3
    got, guards, items, flags = device_run(ov, frames, scenes, 63, guard)
    check(frames, scenes, fonts, 63, got, guards, items, flags)
    assert flags[1] & R.OVERFLOW and len(items[1]) == 256 and not flags[0]
    got2, guards2, items2, flags2 = device_run(ov, frames, scenes, 63, guard, n_streams=1, n_frames=3)                    # frames of one stream
    assert np.array_equal(got2, got)
    ov.close()


def test_overlapping_strings_in_both_orders(fonts):
    H, W = 37, 101
    out = []
    for swap in (False, True):
        s, mask = TS.scene_overlap(W, H, swap)
        ov = make_overlay((H, W), 1, fonts, s)
        frames = TS.background(1, H, W)
        res = device_run(ov, frames, [s], mask, 3)
        check(frames, [s], fonts, mask, *res)
        out.append(res[0])
        ov.close()
    assert not np.array_equal(out[0], out[1])


def test_a_1280x720_frame_with_every_kind(fonts):
    s, mask = TS.scene_full(1280, 720, seed=1, n_dist=14)
    ov = make_overlay((720, 1280), 1, fonts, s)
    frames = TS.background(1, 720, 1280)
    got, guards, items, flags = device_run(ov, frames, [s], mask, 5)
    check(frames, [s], fonts, mask, got, guards, items, flags)
    assert flags[0] == R.RANGE                         # the distance of 2^30
    texts = [bytes(i["text"]).decode("latin-1") for i in items[0]]
    assert " 2.12 m" in texts and " 0.38 m" in texts and " unknown m" in texts and " nan m" in texts
    # each kind alone paints its own items only
    for bit in (1, 2, 4, 8, 16, 32):
        g1, gu1, it1, fl1 = device_run(ov, frames, [s], bit, 0)
        check(frames, [s], fonts, bit, g1, gu1, it1, fl1)
        assert len(it1[0]) and all(int(i["source"]) == bit for i in it1[0])
    ov.close()


def test_second_run_sees_new_inputs_and_tables(fonts):
    """The handle keeps no text state between runs: new arrays, new lines and a new font give the new frame."""
    H, W = 37, 101
    s, mask = TS.scene_edges(W, H)
    ov = make_overlay((H, W), 1, fonts, s)
    frames = TS.background(1, H, W)
    check(frames, [s], fonts, mask, *device_run(ov, frames, [s], mask))
    s2 = dict(s, lines=[(4, 20, TS.LINE_SLOT_BINARY, (1, 250, 3), "second")])
    ov.set_text_lines(s2["lines"])
    f2 = dict(fonts)
    f2[TS.LINE_SLOT_BINARY] = TS.make_font(77, True, cell_h=12)
    ov.set_fonts({TS.LINE_SLOT_BINARY: f2[TS.LINE_SLOT_BINARY]})
    check(frames, [s2], f2, mask, *device_run(ov, frames, [s2], mask))
    ov.close()


def test_refusals(fonts):
    """Each is ADAS_ERR_INVALID with its message."""
    def refused(match, fn, *a, **k):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **k)
        assert ei.value.code == INVALID
    H, W = 16, 64
    s, _ = TS.scene_labels(W, H)
    a, caps = TS.pack_scenes([s, s])
    bufs = {k: L.DeviceBuffer.from_array(v) for k, v in a.items()}
    p = {k: b.ptr for k, b in bufs.items()}
    frames = TS.background(2, H, W)
    d_f = L.DeviceBuffer.from_array(frames)
    ov = PP.LaneOverlay((H, W), None, 2)
    refused("adas_overlay_run_text_arrays: no font set", ov.run_text_arrays, d_f.ptr, 1, 1, 1, None, *caps, **p)
    bad = dict(fonts[0], glyph_x=np.array(fonts[0]["glyph_x"]))
    bad["glyph_x"][40] = fonts[0]["atlas"].shape[1] - 1
    bad["glyph_w"] = np.array(fonts[0]["glyph_w"]); bad["glyph_w"][40] = 5
    refused("adas_overlay_set_font: slot 0: glyph_x of character 72 .*leave the atlas", ov.set_fonts, {0: bad})
    refused("adas_overlay_set_font: slot 1: cell_h 65", ov.set_fonts, {1: dict(fonts[1], atlas=np.zeros((65, fonts[1]["atlas"].shape[1]), np.uint8))})
    wide = dict(fonts[1], glyph_w=np.array(fonts[1]["glyph_w"]))
    wide["glyph_w"][3] = 65
    refused("adas_overlay_set_font: slot 1: glyph_w of character 35 is 65", ov.set_fonts, {1: wide})
    refused("adas_overlay_set_font: slot 16", ov.set_fonts, {16: fonts[0]})
    refused("adas_overlay_set_text_labels: name 1 is null or longer than 31 bytes", ov.set_text_labels, "detections", ["ok", "x" * 32])
    ov.set_text_labels("detections", ["x" * 31])
    ov.set_fonts({0: fonts[0]})
    refused("adas_overlay_run_text_arrays: the detections text needs font slot 1, which is empty", ov.run_text_arrays, d_f.ptr, "detections", 1, 1, None, *caps, **p)
    refused("adas_overlay_run_text_arrays: the distance text needs font slot 5, which is empty", ov.run_text_arrays, d_f.ptr, 8, 1, 1, None, *caps, **p)
    ov.set_fonts(fonts)
    refused("adas_overlay_run_text_arrays: unknown text bits 0x40", ov.run_text_arrays, d_f.ptr, 64, 1, 1, None, *caps, **p)
    refused("adas_overlay_run_text_arrays: 3 streams x 1 frames, the handle holds 2", ov.run_text_arrays, d_f.ptr, 1, 3, 1, None, *caps, **p)
    refused("adas_overlay_run_text_arrays: the detections text needs the detections", ov.run_text_arrays, d_f.ptr, 1, 1, 1, None, *caps,
            **dict(p, det_cls=None))
    refused("the track_ids text needs the trajectories' newest boxes", ov.run_text_arrays, d_f.ptr, 4, 1, 1, None, *caps, **dict(p, traj_len=None))
    refused("the distance text needs the distance points", ov.run_text_arrays, d_f.ptr, 8, 1, 1, None, *caps, **dict(p, dist_d=None))
    refused("the panels text needs the offset, curvature and collision types", ov.run_text_arrays, d_f.ptr, 16, 1, 1, None, *caps,
            **dict(p, collision_type=None))
    refused("own buffer holds 0 drawn frames", ov.run_text_arrays, None, 1, 1, 1, None, *caps, **p)
    refused("adas_overlay_set_text_style: max_text_items 1025", ov.set_text_style, max_text_items=1025)
    ov.set_text_style(max_text_items=256)
    with pytest.raises(ValueError, match="unknown overlay text"):
        ov.text_mask(("fps",))
    with pytest.raises(ValueError, match="at most 47"):
        ov.set_text_lines([(0, 0, 0, (0, 0, 0), "x" * 48)])
    assert np.array_equal(d_f.download(frames.shape, np.uint8), frames), "a refused run wrote"
    ov.set_class_colors("detections", TS.COLORS)
    ov.set_text_labels("detections", TS.NAMES)
    ov.run_text_arrays(d_f.ptr, 1, 2, 1, None, *caps, **p)          # and the handle still works
    assert len(ov.text_items(1)) == 8
    for b in list(bufs.values()) + [d_f]:
        b.free()
    ov.close()
