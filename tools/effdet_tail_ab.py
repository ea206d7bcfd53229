#!/usr/bin/env python3
"""A/B of the EfficientDet tail (adas_effdet_tail_run): the single-workgroup launch (ADAS_EFFDET_TAIL_ONE_WG=1 at create time) against the
default two-pass launch (class-max pass over anchor chunks x frames + finish pass per frame), device-event times.

Seeded synthetic heads (background logits around -8, a few object blobs: ~150 candidates per frame, as tests/test_hostemu_logic._effdet_heads
makes them) are uploaded once per point; both handles read the same device buffers.  Per point: warm-up, then `--repeats` rounds in which
the two paths alternate, each timing `--launches` back-to-back launches between two events.  Results of the two paths are compared
before anything is timed.

    python tools/effdet_tail_ab.py [--sizes 512,896] [--batches 1,64] [--launches 200] [--repeats 3] [--out FILE]
    python tools/effdet_tail_ab.py --trace-only --launches 20      # a short run for rocprofv3 --kernel-trace --stats
"""
import argparse, importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="512,896"); ap.add_argument("--batches", default="1,64")
ap.add_argument("--launches", type=int, default=200); ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--trace-only", action="store_true", help="no timing table: warm-up plus --launches launches of each path per point")
ap.add_argument("--out", default=None)
a = ap.parse_args()
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
if L.lib().adas_device_count() <= 0:
    raise SystemExit("effdet_tail_ab needs a GPU: times are device-event times")
NC, ENV = 90, "ADAS_EFFDET_TAIL_ONE_WG"
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def heads(seed, S, n_obj=12):
    """One frame's head tensors, the recipe of tests/test_hostemu_logic._effdet_heads (float32 draws to keep batch 64 at 896 quick)."""
    rng = np.random.default_rng(seed)
    A = 9 * sum((S >> l) ** 2 for l in range(3, 8))
    cls = rng.standard_normal((A, NC), dtype=np.float32) - np.float32(8.0)
    reg = np.float32(0.3) * rng.standard_normal((A, 4), dtype=np.float32)
    for _ in range(n_obj):
        a0 = int(rng.integers(0, A - 40)); c = int(rng.integers(0, NC))
        idx = a0 + rng.choice(40, 12, replace=False)
        cls[idx, c] = rng.uniform(-1.0, 3.0, 12).astype(np.float32)
        cls[idx[:3], (c + 1) % NC] = rng.uniform(0.0, 3.0, 3).astype(np.float32)
        reg[idx] = (0.05 * rng.standard_normal((12, 4))).astype(np.float32)
    return reg, cls


def make(S, B, one_wg):
    os.environ.pop(ENV, None)
    if one_wg:
        os.environ[ENV] = "1"
    try:
        return PP.EffdetTail((S, S), NC, 0.05, 0.5, 100, 2048, B)
    finally:
        os.environ.pop(ENV, None)


say("# EfficientDet tail A/B: old = one 1024-thread workgroup per frame (effdet_tail_kernel), new = effdet_scan_kernel (chunks x frames) + effdet_finish_kernel")
say("# device-event time of %d back-to-back adas_effdet_tail_run launches per sample, %d samples per path, paths alternating; ms per launch" % (a.launches, a.repeats))
say("# bytes: the class logits read once (rows x %d x 4 B per frame) + the regressions of the candidates (negligible, not counted)" % NC)
verdicts = []
for S in [int(v) for v in a.sizes.split(",")]:
    rows = [9 * (S >> l) ** 2 for l in range(3, 8)]
    offs = np.concatenate([[0], np.cumsum(rows)])
    for B in [int(v) for v in a.batches.split(",")]:
        uniq = min(B, 8)                      # eight distinct frames, repeated: the kernels see B frames' worth of bytes either way
        hs = [heads(1000 * S + b, S) for b in range(uniq)]
        bufs_r, bufs_c = [], []
        for l in range(5):
            r = np.stack([hs[b % uniq][0][offs[l]:offs[l + 1]] for b in range(B)]); c = np.stack([hs[b % uniq][1][offs[l]:offs[l + 1]] for b in range(B)])
            bufs_r.append(L.DeviceBuffer.from_array(r)); bufs_c.append(L.DeviceBuffer.from_array(c))
        rp, cp = [b.ptr for b in bufs_r], [b.ptr for b in bufs_c]
        tails = {"old": make(S, B, True), "new": make(S, B, False)}
        res = {}
        for k, t in tails.items():
            t.run(rp, cp, B)
            res[k] = [t.fetch(b) for b in range(B)]
        same = all(x["n_candidates"] == y["n_candidates"] and np.array_equal(x["boxes"], y["boxes"]) and np.array_equal(x["conf"], y["conf"])
                   and np.array_equal(x["class_id"], y["class_id"]) for x, y in zip(res["old"], res["new"]))
        ncand = [r["n_candidates"] for r in res["new"]]
        nbytes = B * sum(rows) * NC * 4
        for k, t in tails.items():
            for _ in range(a.warmup):
                t.run(rp, cp, B)
            t.fetch(0)
        if a.trace_only:
            for k, t in tails.items():
                for _ in range(a.launches):
                    t.run(rp, cp, B)
                t.fetch(0)
            say("%d^2 batch %d: results identical %s, %d launches of each path issued" % (S, B, same, a.launches))
        else:
            ms = {"old": [], "new": []}
            tm = L.StreamTimer()
            for rep in range(a.repeats):
                for k in ("old", "new"):
                    t = tails[k]
                    with tm:
                        for _ in range(a.launches):
                            t.run(rp, cp, B)
                    ms[k].append(tm.ms / a.launches)
            tm.close()
            spread = max(max(v) - min(v) for v in ms.values())
            med = {k: float(np.median(v)) for k, v in ms.items()}
            faster = max(ms["new"]) < min(ms["old"]) and (min(ms["old"]) - max(ms["new"])) > spread
            verdicts.append(faster and same)
            say("%d^2 batch %-3d  %7d anchors/frame, candidates/frame %d..%d, results identical: %s" % (S, B, sum(rows), min(ncand), max(ncand), same))
            for k in ("old", "new"):
                say("    %s  %s ms   median %.4f ms   %.1f MB logits -> %.1f GB/s" % (k, " ".join("%.4f" % v for v in ms[k]), med[k], nbytes / 1e6, nbytes / (med[k] * 1e-3) / 1e9))
            say("    old / new = %.2fx; spread over the repeats %.4f ms; new faster by more than the spread: %s" % (med["old"] / med["new"], spread, faster))
        for t in tails.values():
            t.close()
        for b in bufs_r + bufs_c:
            b.free()
if not a.trace_only:
    say("# acceptance (new faster than old at every point by more than the spread, identical results): %s" % ("met" if all(verdicts) else "NOT met"))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
