"""tools/demo_headless.py hands `objectDetector.staged_frame` to transformToBirdView, so every object detector class the demo can pick
has to hand out the frame it staged: YoloDetector and EfficientdetDetector alike."""
import importlib
import os
import runpy
import sys

import pytest

from conftest import load_pkg

load_pkg()
D = importlib.import_module("adas_amd.detectors")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_frame_staging_detector_has_staged_frame():
    """Each drop-in class that uploads frames (DetectFrame) exposes the upload as the `staged_frame` property."""
    classes = [D.YoloDetector, D.EfficientdetDetector, D.UltrafastLaneDetectorV2, D.UltrafastLaneDetector]
    for cls in classes:
        assert isinstance(getattr(cls, "staged_frame", None), property), cls.__name__


@pytest.mark.gpu
def test_headless_demo_loop_efficientdet(capsys):
    """`demo_headless.py --det-type efficientdet`: the loop, the bird-view warp of the detector's staged frame included, runs end to end."""
    argv = sys.argv
    sys.argv = ["demo_headless.py", "--frames", "2", "--det-type", "efficientdet"]
    try:
        mod = runpy.run_path(os.path.join(ROOT, "tools", "demo_headless.py"), run_name="demo_headless")
        assert mod["main"]() == 2
    finally:
        sys.argv = argv
    out = capsys.readouterr().out
    assert out.count("frame ") == 2 and "FCWS" in out and "frames/s" in out
