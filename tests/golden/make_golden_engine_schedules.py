#!/usr/bin/env python3
"""Golden launch schedules: what one forward launches, layer by layer, for every shipped graph (models.BUILDERS at its default input size)
in the four precisions at (max_batch, batch) = (64, 64), (64, 1) and (1, 1) -- every layer's adas_engine_layer_kernel string and
adas_engine_launch_count after adas_engine_prepare(batch); the same for the two 16-bit precisions with ADAS_ML=1 set before the engine is
created (rows "<precision>+ml"), plus adas_engine_ml_info.  Where the loader refuses the graph in a precision, the refusal's text.
Recorded from live engines on an MI355X with the engine as it was BEFORE the schedule was decided in one place (csrc/engine_schedule.cpp);
tests/test_engine_schedule_cpu.py holds the device-free adas_debug_engine_schedule to these rows.
    python tests/golden/make_golden_engine_schedules.py   -> tests/golden/engine_schedules.json.gz
The weights are all zero (models.ZeroWeights: the schedule never looks at one) and the container's blob is a hole in a sparse file.

File form: {"strings": [...], "lists": [[string index per layer] ...],
            "configs": {"<graph>/<precision>[+ml]/<max_batch>/<batch>": {"labels": list index, "launches": n[, "ml": [launches, layers, items]]}
                                                                       | {"refused": text}}}.
Configurations with the same labels share one list."""
import ctypes as C
import gzip
import importlib
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "engine_schedules.json.gz")
PRECISIONS = ("bf16", "fp32", "fp16", "fp16x3")
ML_PRECISIONS = ("bf16", "fp16")
SHAPES = ((64, 64), (64, 1), (1, 1))          # (max_batch, batch)
LABEL_CAP = 96


def config_key(name, prec, max_batch, batch, ml=False):
    return f"{name}/{prec}{'+ml' if ml else ''}/{max_batch}/{batch}"


def all_keys(names):
    return {config_key(n, p, mb, b, ml) for n in names for ml in (False, True) for p in (ML_PRECISIONS if ml else PRECISIONS) for mb, b in SHAPES}


def refusal_text(msg):
    """The loader's message without the container's name in front ("[path]: ...")."""
    return msg.split("]: ", 1)[1] if "]: " in msg else msg


def load(path=FIXTURE):
    """{config key: {"labels": [str per layer], "launches": n, "ml": (launches, layers, items) | None} | refusal text}"""
    with gzip.open(path, "rt") as f:
        d = json.load(f)
    lists = [[d["strings"][i] for i in l] for l in d["lists"]]
    return {k: (v["refused"] if "refused" in v else {"labels": lists[v["labels"]], "launches": v["launches"], "ml": tuple(v["ml"]) if "ml" in v else None})
            for k, v in d["configs"].items()}


def typed_lib(L):
    """The library with only the entries the recorder calls typed: it also loads a build from before adas_debug_engine_schedule existed
    (ADAS_LIB=...), which _lib.lib() would refuse for the missing symbol."""
    lib = C.CDLL(L.LIB_PATH)
    for name in ("adas_engine_create", "adas_engine_destroy", "adas_engine_prepare", "adas_engine_stats", "adas_engine_layer_kernel",
                 "adas_engine_launch_count", "adas_engine_ml_info", "adas_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = L._SIGS[name]
    return lib


def live_schedules(L, lib, path, prec, max_batch, batches, ml):
    """{batch: row} of one engine created from the container at `path`, or the refusal text.  A HIP error ends the recording."""
    def must(rc, what):
        if rc != 0:
            raise SystemExit(f"{path} {prec} max_batch {max_batch}: {what}: error {rc}: {lib.adas_last_error().decode('utf-8', 'replace')}")
    h = C.c_void_p()
    rc = lib.adas_engine_create(path.encode(), L.PRECISIONS[prec], max_batch, C.byref(h))
    if rc != 0:
        msg = lib.adas_last_error().decode("utf-8", "replace")
        if rc != -3:     # only ADAS_ERR_FORMAT is a refusal of the container; anything else (a HIP error first of all) stops the run
            raise SystemExit(f"{path} {prec} max_batch {max_batch}: error {rc}: {msg}")
        return refusal_text(msg)
    try:
        nl = C.c_int()
        must(lib.adas_engine_stats(h, None, None, C.byref(nl)), "adas_engine_stats")
        rows = {}
        name = C.create_string_buffer(LABEL_CAP)
        for batch in batches:
            must(lib.adas_engine_prepare(h, batch), "adas_engine_prepare")
            labels = []
            for i in range(nl.value):
                must(lib.adas_engine_layer_kernel(h, i, batch, name, LABEL_CAP), "adas_engine_layer_kernel")
                labels.append(name.value.decode())
            row = {"labels": labels, "launches": int(lib.adas_engine_launch_count(h, batch))}
            if ml:
                a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
                must(lib.adas_engine_ml_info(h, batch, C.byref(a), C.byref(b), C.byref(c)), "adas_engine_ml_info")
                row["ml"] = [a.value, b.value, c.value]
            rows[batch] = row
        return rows
    finally:
        lib.adas_engine_destroy(h)


def main():
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("vehicle-cv-adas_amd")
    sys.modules["adas_amd"] = pkg
    L = importlib.import_module("adas_amd._lib")
    M = importlib.import_module("adas_amd.models")
    lib = typed_lib(L)
    for k in ("ADAS_ML", "ADAS_NO_GROUP"):
        os.environ.pop(k, None)
    strings, sindex, lists, lindex, configs = [], {}, [], {}, {}
    by_max = {}
    for mb, b in SHAPES:
        by_max.setdefault(mb, []).append(b)
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
            for ml in (False, True):
                if ml:
                    os.environ["ADAS_ML"] = "1"        # read when the engine is created
                for prec in (ML_PRECISIONS if ml else PRECISIONS):
                    for mb, batches in by_max.items():
                        r = live_schedules(L, lib, path, prec, mb, batches, ml)
                        for b in batches:
                            if isinstance(r, str):
                                configs[config_key(name, prec, mb, b, ml)] = {"refused": r}
                                continue
                            row = r[b]
                            ids = []
                            for s in row["labels"]:
                                if s not in sindex:
                                    sindex[s] = len(strings)
                                    strings.append(s)
                                ids.append(sindex[s])
                            k = json.dumps(ids)
                            if k not in lindex:
                                lindex[k] = len(lists)
                                lists.append(ids)
                            row["labels"] = lindex[k]
                            configs[config_key(name, prec, mb, b, ml)] = row
                os.environ.pop("ADAS_ML", None)
            os.remove(path)
            print(f"{name}: {time.time() - t0:.1f} s since the start", flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with gzip.GzipFile(out, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps({"strings": strings, "lists": lists, "configs": configs}, separators=(",", ":")).encode())
    refused = sum("refused" in v for v in configs.values())
    print(f"{out}: {len(configs)} configurations ({refused} refused), {len(lists)} distinct label lists, {len(strings)} strings, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
