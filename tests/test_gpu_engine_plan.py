"""GPU: the plan a live engine reports (adas_engine_plan) is the plan the device-free planner gives the same tables
(adas_debug_engine_plan, tests/test_engine_plan_cpu.py) -- five detector / lane families at reduced sizes, four precisions, max_batch 2 --
and an engine whose plan was read computes what an untouched engine computes, bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import netutil
from conftest import load_pkg

pytestmark = pytest.mark.gpu

load_pkg()
L = importlib.import_module("adas_amd._lib")
LANE_KW = dict(in_h=160, in_w=800, num_grid_row=100, num_cls_row=36, num_grid_col=50, num_cls_col=41)
GRAPHS = [("yolov8n", dict(imgsz=(96, 128))), ("yolov5n", dict(imgsz=(96, 128))), ("yolov7-tiny", dict(imgsz=(96, 128))),
          ("ufldv2_res18", LANE_KW), ("efficientdet-d0", dict(imgsz=128))]
COLS = 29


def live_plan(e):
    n, wb = C.c_int32(), C.c_uint64()
    L.check(L.lib().adas_engine_plan(e.handle, None, 0, C.byref(n), C.byref(wb)))
    rows = np.zeros((n.value, COLS), np.int64)
    L.check(L.lib().adas_engine_plan(e.handle, rows.ctypes.data_as(C.POINTER(C.c_int64)), n.value, C.byref(n), C.byref(wb)))
    return rows, wb.value


def table_plan(tables, prec, max_batch):
    n, wb = C.c_int32(), C.c_uint64()
    rows = np.zeros((4096, COLS), np.int64)
    L.check(L.lib().adas_debug_engine_plan(tables, len(tables), prec, max_batch, rows.ctypes.data_as(C.POINTER(C.c_int64)), 4096, C.byref(n), C.byref(wb)))
    return rows[:n.value], wb.value


@pytest.mark.parametrize("prec", ["bf16", "fp32", "fp16", "fp16x3"])
@pytest.mark.parametrize("name,kw", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_live_plan_is_the_table_plan(name, kw, prec):
    CE = importlib.import_module("adas_amd.coreEngine")
    assert L.lib().adas_device_count() > 0
    path, _, g = netutil.model(name, **kw)
    x = (netutil.lane_frames(2, g.in_h, g.in_w) if name.startswith("ufld") else netutil.coco_like_frames(2, g.in_h, g.in_w))
    e = CE.HipEngine(path, precision=prec, max_batch=2)
    try:
        rows, wb = live_plan(e)
        want_rows, want_wb = table_plan(g.tables(), L.PRECISIONS[prec], 2)
        assert wb == want_wb == e.stats()["weight_bytes"]
        assert rows.shape == want_rows.shape and (rows == want_rows).all(), np.argwhere(rows != want_rows)[:4].tolist()
        got = e.engine_inference(x)
    finally:
        e.close()
    plain = CE.HipEngine(path, precision=prec, max_batch=2)      # never asked for its plan
    try:
        want = plain.engine_inference(x)
    finally:
        plain.close()
    assert len(got) == len(want) and len(got) > 0
    for a, b in zip(got, want):
        assert np.isfinite(b).all() and a.tobytes() == b.tobytes()
