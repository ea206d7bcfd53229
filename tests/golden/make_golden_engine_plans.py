#!/usr/bin/env python3
"""Golden load-time plans: what adas_engine_create decides for every shipped graph (models.BUILDERS at its default input size) in the four
precisions at max_batch 64 and 1 -- the rows of adas_engine_plan (include/adas_hip.h) and the weight arena's size, or the text of the
refusal where the loader refuses the graph in that precision.  Recorded from live engines on an MI355X with the loader as it was BEFORE it
was split into phases (csrc/engine_load.cpp); tests/test_engine_plan_cpu.py holds the device-free planner to these cells.
    python tests/golden/make_golden_engine_plans.py   -> tests/golden/engine_plans.json.gz
The weights are all zero (models.ZeroWeights: the plan never looks at one) and the container's blob is a hole in a sparse file.

File form: {"cols": 29, "plans": [...], "configs": {"<graph>/<precision>/<max_batch>": plan index | {"refused": text}}}.  Configurations
with the same plan share one entry; a plan is {"n": ops, "weight_bytes": ..., "columns": [29 x (int: the whole column | list: first value,
then the difference to the row before)]}."""
import ctypes as C
import gzip
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "engine_plans.json.gz")
PRECISIONS = ("bf16", "fp32", "fp16", "fp16x3")
BATCHES = (64, 1)
COLS = 29


def config_key(name, prec, max_batch):
    return f"{name}/{prec}/{max_batch}"


def refusal_text(msg):
    """The loader's message without the container's name in front ("[path]: ...")."""
    return msg.split("]: ", 1)[1] if "]: " in msg else msg


def encode_plan(rows, weight_bytes):
    cols = []
    for c in range(COLS):
        v = rows[:, c]
        cols.append(int(v[0]) if len(v) and (v == v[0]).all() else [int(x) for x in np.diff(v, prepend=0)])
    return {"n": int(rows.shape[0]), "weight_bytes": int(weight_bytes), "columns": cols}


def decode_plan(p):
    rows = np.empty((p["n"], COLS), np.int64)
    for c, col in enumerate(p["columns"]):
        rows[:, c] = np.cumsum(np.asarray(col, np.int64)) if isinstance(col, list) else col
    return rows, p["weight_bytes"]


def load(path=FIXTURE):
    """{config key: (rows, weight_bytes) | refusal text}"""
    with gzip.open(path, "rt") as f:
        d = json.load(f)
    assert d["cols"] == COLS
    plans = [decode_plan(p) for p in d["plans"]]
    return {k: (v["refused"] if isinstance(v, dict) else plans[v]) for k, v in d["configs"].items()}


def typed_lib(L):
    """The library with only the entries the recorder calls typed: it also loads a build from before adas_debug_engine_plan existed
    (ADAS_LIB=...), which _lib.lib() would refuse for the missing symbol."""
    lib = C.CDLL(L.LIB_PATH)
    for name in ("adas_engine_create", "adas_engine_destroy", "adas_engine_plan", "adas_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L._SIGS[name]
    return lib


def live_plan(L, lib, path, prec, max_batch):
    """(rows, weight_bytes) of an engine created from the container at `path`, or the refusal text.  A HIP error ends the recording."""
    h = C.c_void_p()
    rc = lib.adas_engine_create(path.encode(), L.PRECISIONS[prec], max_batch, C.byref(h))
    if rc != 0:
        msg = lib.adas_last_error().decode("utf-8", "replace")
        if rc != -3:     # only ADAS_ERR_FORMAT is a refusal of the container; anything else (a HIP error first of all) stops the run
            raise SystemExit(f"{path} {prec} max_batch {max_batch}: error {rc}: {msg}")
        return refusal_text(msg)
    try:
        n, wb = C.c_int32(), C.c_uint64()
        rc = lib.adas_engine_plan(h, None, 0, C.byref(n), C.byref(wb))
        rows = np.zeros((n.value, COLS), np.int64)
        rc = rc or lib.adas_engine_plan(h, rows.ctypes.data_as(C.POINTER(C.c_int64)), n.value, C.byref(n), C.byref(wb))
        if rc != 0:
            raise SystemExit(f"adas_engine_plan: error {rc}: {lib.adas_last_error().decode()}")
        return rows, wb.value
    finally:
        lib.adas_engine_destroy(h)


def main():
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("vehicle-cv-adas_amd")
    sys.modules["adas_amd"] = pkg
    L = importlib.import_module("adas_amd._lib")
    M = importlib.import_module("adas_amd.models")
    lib = typed_lib(L)
    plans, index, configs = [], {}, {}
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        for name in M.BUILDERS:
            g = M.build(name, wsrc=M.ZeroWeights())
            path = os.path.join(tmp, name + ".adas")
            tables = g.tables()
            with open(path, "wb") as f:
                f.write(tables)
                f.truncate(len(tables) + len(g.blob))
            del g
            for prec in PRECISIONS:
                for mb in BATCHES:
                    r = live_plan(L, lib, path, prec, mb)
                    if isinstance(r, str):
                        configs[config_key(name, prec, mb)] = {"refused": r}
                        continue
                    p = encode_plan(*r)
                    k = json.dumps(p)
                    if k not in index:
                        index[k] = len(plans)
                        plans.append(p)
                    configs[config_key(name, prec, mb)] = index[k]
            os.remove(path)
            print(f"{name}: {time.time() - t0:.1f} s since the start", flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps({"cols": COLS, "plans": plans, "configs": configs}, separators=(",", ":")).encode())
    refused = sum(isinstance(v, dict) for v in configs.values())
    print(f"{out}: {len(configs)} configurations ({refused} refused), {len(plans)} distinct plans, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
