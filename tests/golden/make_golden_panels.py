#!/usr/bin/env python3
"""Golden frames of the REFERENCE's ControlPanel (demo.py:32-214), run unmodified:

    python tests/golden/make_golden_panels.py     # needs the reference checkout (ADAS_REFERENCE); writes panels.json.gz

demo.py cannot be imported (its module level opens a video and builds TensorRT engines), so the ControlPanel class is lifted out of its
syntax tree by `ast` and compiled as it stands; the three enums come from the reference's own modules under the usual import stubs (SURVEY
App. C).  The cv2 stub: imread returns the scene's sprite for the asset's file name (tests/panel_scene.py) and resize hands a sprite back
unchanged (the scene builds them at the sizes ControlPanel resizes to); resize of an image is oracle.preprocess.cv_resize_linear_u8;
copyMakeBorder is a constant pad; putText RECORDS its arguments and draws nothing.  `time` is a counter, so the FPS string is the same on
every run.

WHAT THE FIXTURE PINS.  The signs panel, the collision panel and the bird panel's placement and border are the reference's own NumPy lines:
pinned.  The resize arithmetic inside the bird panel is the project's restatement of OpenCV's INTER_LINEAR, the same on both sides of
every comparison: UNPINNED, as in pre-processing.

Contents: the 96 transitions (4 latches x 4 offset types x 6 curvature types, curve_status assigned before each call: the latch after
the call and the SHA-256 of the 416 x 368 frame after DisplaySignsPanel); the four collision types and the bird panel at 416 x 368 and
1280 x 720; one 40-frame sequence through all three calls with per-frame hashes; the putText calls of that sequence, for whoever draws
text later.  The generator asserts that all 16 (latch before, latch after) pairs and a two-sprite frame occur; the test asserts it again."""
import ast, gzip, hashlib, json, os, sys, types
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG
import panel_scene as PS
from oracle.preprocess import cv_resize_linear_u8


def sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, np.uint8).tobytes()).hexdigest()


def install_cv2(log, sprites):
    cv2 = types.ModuleType("cv2")
    for k, v in dict(INTER_LINEAR=1, FONT_HERSHEY_TRIPLEX=4, FONT_HERSHEY_SIMPLEX=0, LINE_AA=16, LINE_8=8, LINE_4=4, COLOR_BGR2RGB=4, FILLED=-1,
                     IMREAD_UNCHANGED=-1, BORDER_CONSTANT=0).items():
        setattr(cv2, k, v)
    by_file = {f: n for n, f in PS.REF_FILE.items()}

    def imread(path, flags=1):
        assert flags == cv2.IMREAD_UNCHANGED
        return sprites[by_file[os.path.basename(path)]]

    def resize(img, dsize, *a, **k):
        assert not a and not k, "the reference passes no interpolation: INTER_LINEAR"
        if img.shape[2] == 4:      # a sprite: the scene built it at the size asked for
            assert (img.shape[1], img.shape[0]) == tuple(dsize), (img.shape, dsize)
            return img
        return cv_resize_linear_u8(np.ascontiguousarray(img), dsize)

    def copyMakeBorder(src, top, bottom, left, right, borderType, value=None):
        assert borderType == cv2.BORDER_CONSTANT
        out = np.empty((src.shape[0] + top + bottom, src.shape[1] + left + right, src.shape[2]), src.dtype)
        out[:] = np.asarray(value, src.dtype)
        out[top:top + src.shape[0], left:left + src.shape[1]] = src
        return out

    def putText(img, text, org, fontFace=0, fontScale=1.0, color=(0, 0, 0), thickness=1, lineType=8, bottomLeftOrigin=False):
        log.append([str(text), [int(v) for v in org], int(fontFace), float(fontScale), [int(v) for v in color], int(thickness), int(lineType)])
        return img

    for f in (imread, resize, copyMakeBorder, putText):
        setattr(cv2, f.__name__, f)
    sys.modules["cv2"] = cv2
    return cv2


def lift_control_panel(cv2, enums):
    tree = ast.parse(open(os.path.join(MG.REF, "demo.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ControlPanel"]
    assert len(cls) == 1
    clock = types.SimpleNamespace(t=0.0)

    def tick():
        clock.t += 0.03125
        return clock.t
    ns = dict(cv2=cv2, np=np, time=types.SimpleNamespace(time=tick), **enums)
    exec(compile(ast.Module(body=cls, type_ignores=[]), "demo.py", "exec"), ns)
    return ns["ControlPanel"]


def main():
    MG.install_stubs()
    log = []
    sprites = PS.sprites()
    cv2 = install_cv2(log, sprites)
    from ObjectDetector.utils import CollisionType
    from TrafficLaneDetector.ufldDetector.utils import OffsetType, CurvatureType
    ControlPanel = lift_control_panel(cv2, dict(CollisionType=CollisionType, OffsetType=OffsetType, CurvatureType=CurvatureType))
    OFF = [getattr(OffsetType, n) for n in PS.OFFSETS]
    CUR = [getattr(CurvatureType, n) for n in PS.CURVATURES]
    COL = [getattr(CollisionType, n) for n in PS.COLLISIONS]
    cp = ControlPanel()
    for name, attr in PS.REF_ATTR.items():
        assert getattr(cp, attr) is sprites[name], name
    base = PS.transition_frame()
    transitions = []
    for latch in range(4):
        for off in range(4):
            for cur in range(6):
                cp.curve_status = PS.LATCHES[latch]
                img = base.copy()
                cp.DisplaySignsPanel(img, OFF[off], CUR[cur])
                transitions.append([latch, off, cur, PS.LATCHES.index(cp.curve_status), sha(img)])
    assert len(PS.latch_pairs(transitions)) == 16, sorted(PS.latch_pairs(transitions))
    assert PS.two_sprite_rows(transitions), "no two-sprite frame"
    collision, bird = {}, {}
    for hw in PS.SIZES:
        key = "%dx%d" % (hw[1], hw[0])
        collision[key] = []
        for col in range(4):
            img = PS.collision_frame(hw)
            cp.DisplayCollisionPanel(img, COL[col], 0.0, 0.0)
            collision[key].append(sha(img))
        img = PS.bird_frame(hw)
        cp.DisplayBirdViewPanel(img, PS.bird(hw))
        bird[key] = sha(img)
    cp = ControlPanel()
    seq, texts = [], []
    for i, (off, cur, col) in enumerate(PS.sequence(40)):
        img, bv = PS.sequence_frame(i)
        del log[:]
        cp.DisplayBirdViewPanel(img, bv)
        cp.DisplaySignsPanel(img, OFF[off], CUR[cur])
        cp.DisplayCollisionPanel(img, COL[col], 0.02, 0.0125)
        seq.append(dict(offset=off, curvature=cur, collision=col, latch=PS.LATCHES.index(cp.curve_status), sha=sha(img)))
        texts.append([list(c) for c in log])
    assert {s["latch"] for s in seq} == {0, 1, 2, 3}, "the sequence does not visit every latch value"
    res = dict(transitions=transitions, collision=collision, bird=bird, sequence=seq, puttext=texts,
               pins="signs and collision panels, bird panel placement: the reference's code; the resize inside the bird panel: unpinned")
    path = os.path.join(HERE, "panels.json.gz")
    with open(path, "wb") as raw:       # mtime 0, no file name: the same bytes on every run
        with gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as f:
            f.write(json.dumps(res).encode())
    print("transitions", len(transitions), "latch pairs", len(PS.latch_pairs(transitions)), "two-sprite rows", len(PS.two_sprite_rows(transitions)),
          "sequence", len(seq), "putText calls", sum(len(t) for t in texts), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
