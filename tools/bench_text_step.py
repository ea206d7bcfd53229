#!/usr/bin/env python3
"""The fused step of tools/bench_text.py with text OFF, alone, as one JSON line -- the piece that can also run in a checkout of the parent
commit, which has no text: `bench_text.py --parent-tree DIR` copies this file into DIR/tools and alternates the two trees, a process each.
    python tools/bench_text_step.py [--streams 64] [--steps 30] [--rounds 3]
Also the one place that holds the step's configuration (models, pipeline arguments, overlay stages): bench_text.py imports it from here."""
import argparse, importlib, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

H, W, IMG = 720, 1280, (1280, 720)
NAMES = ["class %d" % k for k in range(80)]
COLORS = [((37 * k) % 256, (91 * k + 40) % 256, (53 * k + 200) % 256) for k in range(80)]
OVERLAY = dict(stages=("lanes", "area", "distance", "bird", "detections", "tracks", "trajectories"), detection_colors=COLORS, track_colors=COLORS)


class PrescribedLanes:
    """Zero weights and a last-layer bias that puts both ego lanes on every row anchor (CULane head: 200 x 72 rows, 100 x 81 columns), as in
    tools/bench_panels.py."""

    def __init__(self, gr=200, r=72, gc=100, c=81):
        loc_row = np.zeros((gr, r, 4), np.float32)
        exist_row = np.zeros((2, r, 4), np.float32)
        for k in range(r):
            loc_row[int(round(0.44 * gr - 0.2 * gr / 100 * k)), k, 1] = 10.0
            loc_row[int(round(0.55 * gr + 0.22 * gr / 100 * k)), k, 2] = 10.0
        exist_row[1, :, 1:3] = 5.0
        self.bias = np.concatenate([loc_row.reshape(-1), np.zeros(gc * c * 4, np.float32), exist_row.reshape(-1), np.zeros(2 * c * 4, np.float32)])

    def __call__(self, name, shape, kind, fill=None):
        return self.bias if name == "cls.3.bias" else np.zeros(shape, np.float32)


def packages():
    from conftest import load_pkg
    load_pkg()
    return {n: importlib.import_module("adas_amd." + n) for n in ("_lib", "coreEngine", "pipeline", "models", "analysis")}


def models(P, work):
    import bench, netutil
    base = netutil.coco_like_frames(8, seed=40)
    det_path, _, _ = bench.build_detector(P["models"], P["coreEngine"], "yolov8n", base, work, "txt", target_per_frame=25.0, capacity=512)
    lane_path = P["models"].build("ufldv2_res18", wsrc=PrescribedLanes()).save(os.path.join(work, "lane.hipm"))
    return det_path, lane_path


def pipeline_kw(P, streams, precision, box_score):
    A = P["analysis"]
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    return dict(n_streams=streams, precision=precision, src_hw=(H, W), use_graph=True, track=True, box_score=box_score, max_candidates=512,
                geometry=dict(bird_wh=IMG, M=A.PerspectiveTransformation(IMG).M), birdview=dict(image=True), analysis=dict(ref_height=[car] * 80))


def window(p, cam, count, n):
    """ms per step over n steps between two host clock readings, the pipeline drained at both ends; count: [steps so far]"""
    p.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        p.step_frames(cam[count[0] % 2].ptr, (H, W), 0.6)
        count[0] += 1
    p.sync()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--box-score", type=float, default=0.1)
    a = ap.parse_args()
    P = packages()
    L = P["_lib"]
    if L.lib().adas_device_count() <= 0:
        raise SystemExit("bench_text_step.py needs an MI355X")
    import bench
    cam = [L.DeviceBuffer.from_array(bench.cam_frames(a.streams, 900 + i)) for i in range(2)]
    det_path, lane_path = models(P, tempfile.mkdtemp(prefix="txt_step_"))
    p = P["pipeline"].AdasPipeline(det_path, lane_path, overlay=dict(OVERLAY), **pipeline_kw(P, a.streams, a.precision, a.box_score))
    count = [0]
    window(p, cam, count, 5)                      # warm-up: capture, first-launch costs
    ms = [window(p, cam, count, a.steps) for _ in range(a.rounds)]
    print(json.dumps(dict(tree=ROOT, ms_per_step=ms, kernels=p.graph_kernels())))
    p.close()
    for b in cam:
        b.free()


if __name__ == "__main__":
    main()
