"""CPU: the load-time plan of an engine (csrc/engine_load.cpp: read_container -> validate_container -> plan_engine) on a container's tables
alone -- include/adas_hip.h adas_debug_engine_plan, no device, no weight.

  recorded plans     every shipped graph x 4 precisions x max_batch 64 / 1 against tests/golden/engine_plans.json.gz, which was recorded
                     from live engines on an MI355X with the loader as it was before it was split into phases (make_golden_engine_plans.py)
  fusion boundaries  one small hand-made graph per fusion pass and the nearest graphs that must not fuse; the expected links are written
                     here from the rules of the passes, not read back from the planner
  refusals           every refusal text of the loader on a damaged table

The recorded part builds the 33 graphs with all-zero weights (models.ZeroWeights: no random number is drawn), about 15 s in all, nearly
all of it the graph builders; planning the 264 configurations takes well under a second."""
import contextlib
import ctypes as C
import importlib
import os
import struct

import numpy as np
import pytest

from conftest import load_pkg

load_pkg()
L = importlib.import_module("adas_amd._lib")
M = importlib.import_module("adas_amd.models")
import make_golden_engine_plans as G

F16, BF16, F32, X3 = L.PREC_FP16, L.PREC_BF16, L.PREC_FP32, L.PREC_FP16X3
# columns of a plan row (include/adas_hip.h)
KERNEL, SKIP, FUSE_POOL, FUSE_CONV2, DS_SRC, DS_USER, UP_SRC, POOL3, PAIR_B, C2F, DET_SRC, HALO_BN, HAS_X3H8 = 0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 13, 19, 20
K, KPAD, CIN_PAD, COUT_PAD, W_OFF, B_OFF, DS_W_OFF, X3H8_W_OFF = 21, 22, 23, 24, 25, 26, 27, 28
CONV_STEM, CONV_PW, CONV_STEM2, CONV_PAIR, CONV_C2F_PW, CONV_DET5 = 3, 4, 5, 6, 7, 8     # csrc/kernels.h
Z = M.ZeroWeights()


def plan(tables, prec, max_batch=2):
    """The rows and the weight arena's size the loader plans for these table bytes; AdasError where it refuses them."""
    n, wb = C.c_int32(), C.c_uint64()
    L.check(L.lib().adas_debug_engine_plan(tables, len(tables), prec, max_batch, None, 0, C.byref(n), C.byref(wb)))
    rows = np.zeros((n.value, G.COLS), np.int64)
    L.check(L.lib().adas_debug_engine_plan(tables, len(tables), prec, max_batch, rows.ctypes.data_as(C.POINTER(C.c_int64)), n.value, C.byref(n), C.byref(wb)))
    return rows, wb.value


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


# ------------------------------------------------------------------------------------------------------------------ recorded plans
RECORDED = G.load()


def test_fixture_covers_every_shipped_configuration():
    assert set(RECORDED) == {G.config_key(n, p, mb) for n in M.BUILDERS for p in G.PRECISIONS for mb in G.BATCHES}


@pytest.mark.parametrize("name", list(M.BUILDERS))
def test_recorded_plan(name):
    tables = M.build(name, wsrc=Z).tables()
    for prec in G.PRECISIONS:
        for mb in G.BATCHES:
            want = RECORDED[G.config_key(name, prec, mb)]
            if isinstance(want, str):
                with pytest.raises(L.AdasError) as ex:
                    plan(tables, L.PRECISIONS[prec], mb)
                assert ex.value.code == -3 and G.refusal_text(str(ex.value)) == want, (prec, mb)
                continue
            rows, wb = plan(tables, L.PRECISIONS[prec], mb)
            assert wb == want[1], (prec, mb)
            bad = np.argwhere(rows != want[0])
            assert bad.size == 0, (prec, mb, "first differing (op, column):", bad[0].tolist(), int(rows[tuple(bad[0])]), int(want[0][tuple(bad[0])]))


# --------------------------------------------------------------------------------------------------------------- fusion boundaries
H, W = 24, 40


def graph(in_h=H, in_w=W):
    g = M.Graph("t", 3, in_h, in_w, Z)
    x, cin = g.input()
    return g, x, cin


def body(c=32):
    """A graph whose first conv (3x3 stride 1: never a stem) gives a c-channel H x W map."""
    g, x, cin = graph()
    return g, g.conv(x, c, 3, 1, "c0", true_cin=cin)


def idx(g, name):
    return [i for i, r in enumerate(g.ops) if r["name"] == name][0]


def links(g, prec, max_batch=2):
    rows, _ = plan(g.tables(), prec, max_batch)
    return rows


def unfused(rows):
    """No op is skipped and no link is set."""
    return not rows[:, SKIP].any() and (rows[:, FUSE_POOL:HALO_BN] == -1).all()


# ---- 3x3 -> 3x3 pair (16-bit; the split precision keeps a pair only inside a fused C2f block)
def pair_graph(extra_reader=False, alias=False, writer_between=False, y_in_x=None):
    g, x0 = body(32)
    xb = g.buf(H, W, 64)
    x = g.conv(x0, 32, 3, 1, "x", out=xb.slice(0, 32), act=M.ACT_RELU)       # (ReLU: not itself the first conv of a pair)
    t = g.conv(x, 32, 3, 1, "A")
    if writer_between:
        g.conv(x0, 32, 1, 1, "w", out=xb.slice(32, 32))
    y = {None: None, "apart": xb.slice(32, 32), "over": xb.slice(0, 32)}[y_in_x]
    g.conv(t, 32, 3, 1, "B", out=y)
    if extra_reader:
        g.conv(t, 32, 1, 1, "r")
    if alias:
        g.alias(t, H * W, 1, 32)
    return g


def test_pair():
    g = pair_graph()
    r = links(g, F16)
    a, b = idx(g, "A"), idx(g, "B")
    assert r[a, PAIR_B] == b and r[b, SKIP] == 1 and r[a, SKIP] == 0 and r[a, KERNEL] == r[b, KERNEL] == CONV_PAIR
    assert r[:, SKIP].sum() == 1 and (r[:, PAIR_B] >= 0).sum() == 1
    assert unfused(links(g, F32)) and unfused(links(g, X3))
    r = links(pair_graph(y_in_x="apart"), BF16)             # y in x's buffer, other channels: still a pair
    assert r[a, PAIR_B] == b


@pytest.mark.parametrize("why", ["extra_reader", "alias", "writer_between", "overlap"])
def test_pair_boundaries(why):
    g = pair_graph(y_in_x="over") if why == "overlap" else pair_graph(**{why: True})
    assert unfused(links(g, F16)), why


# ---- projection shortcut link (ResNet layerN.0)
def shortcut_graph(extra_reader=False, writer_between=False):
    g, x0 = body(64)
    xb = g.buf(H, W, 128)
    x = g.conv(x0, 64, 3, 1, "x", out=xb.slice(0, 64), act=M.ACT_RELU)
    c1 = g.conv(x, 128, 3, 2, "c1", act=M.ACT_RELU)
    d = g.conv(x, 128, 1, 2, "ds", act=M.ACT_NONE)
    if writer_between:
        g.conv(x0, 64, 1, 1, "w", out=xb.slice(64, 64))
    g.conv(c1, 128, 3, 1, "c2", act=M.ACT_RELU, res=d, res_mode=M.RES_BEFORE_ACT)
    if extra_reader:
        g.conv(d, 32, 1, 1, "r")
    return g


def test_shortcut_link():
    g = shortcut_graph()
    for prec in (F16, BF16):
        r = links(g, prec)
        d, c2 = idx(g, "ds"), idx(g, "c2")
        assert r[c2, DS_SRC] == d and r[d, DS_USER] == c2 and not r[:, SKIP].any()
        assert r[d, DS_W_OFF] + 128 * 64 * 2 == r[d, W_OFF]         # the second copy of the projection weights sits right ahead of the first
    assert unfused(links(g, F32)) and unfused(links(g, X3))         # conv_halo8 (16-bit) is the only kernel that carries a projection
    assert unfused(links(shortcut_graph(extra_reader=True), F16))
    assert unfused(links(shortcut_graph(writer_between=True), F16))


# ---- upsample folded into the 1x1 conv that reads it
def upsample_graph(slice_reader=False, range_reader=False):
    g, x0 = body(32)
    p5 = g.conv(x0, 64, 3, 2, "p5")
    cat = g.buf(H, W, 96)
    g.upsample2(p5, out=cat.slice(0, 64), name="up")
    g.conv(x0, 32, 1, 1, "lat", out=cat.slice(64, 32))
    g.conv(cat, 32, 1, 1, "cv1")
    if slice_reader:
        g.conv(cat.slice(64, 32), 32, 1, 1, "r")
    if range_reader:
        g.conv(cat.slice(32, 64), 32, 1, 1, "r")
    return g


def test_upsample_fold():
    for prec in (F16, BF16, X3):
        for g in (upsample_graph(), upsample_graph(slice_reader=True)):     # another slice of the concat buffer may have its own reader
            r = links(g, prec)
            u, c = idx(g, "up"), idx(g, "cv1")
            assert r[c, UP_SRC] == u and r[u, SKIP] == 1 and r[:, SKIP].sum() == 1, prec
        assert unfused(links(upsample_graph(range_reader=True), prec))
    assert unfused(links(upsample_graph(), F32))
    with env(ADAS_NO_UPSAMPLE_FOLD="1"):
        assert unfused(links(upsample_graph(), F16))
    assert not unfused(links(upsample_graph(), F16))


# ---- three max-pools in one launch
def pool_graph(kernels=(5, 5, 5), chained=True):
    g, x0 = body(32)
    cat = g.buf(H, W, 256)
    x = g.conv(x0, 64, 1, 1, "cv1", out=cat.slice(0, 64))
    for i, k in enumerate(kernels):
        g.maxpool(cat.slice(i * 64, 64) if chained else x, k, 1, k // 2, out=cat.slice((i + 1) * 64, 64), name=f"m{i}")
    g.conv(cat.slice(0, 64 * (1 + len(kernels))), 32, 1, 1, "cv2")
    return g


def test_pool_triples():
    for g in (pool_graph(), pool_graph((5, 9, 13), chained=False)):      # SPPF, SPP
        for prec in (F16, BF16):
            r = links(g, prec)
            m0 = idx(g, "m0")
            assert r[m0, POOL3:POOL3 + 2].tolist() == [m0 + 1, m0 + 2] and r[m0 + 1, SKIP] == r[m0 + 2, SKIP] == 1 and r[:, SKIP].sum() == 2
        assert unfused(links(g, F32)) and unfused(links(g, X3))
        with env(ADAS_NO_POOL_FUSE="1"):
            assert unfused(links(g, F16))
    assert unfused(links(pool_graph((5, 5)), F16))                        # a chain of two
    assert unfused(links(pool_graph((5, 9, 11), chained=False), F16))
    assert unfused(links(pool_graph((5, 9, 13), chained=True), F16))      # 5 -> 9 -> 13 chained is no SPP
    assert unfused(links(pool_graph((5, 5, 5), chained=False), F16))      # three 5x5 pools of one tensor are no SPPF


# ---- C2f(32, 32, n = 1, shortcut) as one launch
def c2f_graph(fourth_reader=False):
    g, x0 = body(32)
    y = M._c2f(g, x0, 32, 1, True, "m")
    if fourth_reader:
        g.conv(M.View(idx_buf(g, "m.cv1.conv"), 0, 16, H, W), 32, 1, 1, "r")
    g.conv(y, 32, 1, 1, "tail")
    return g


def idx_buf(g, name):
    return g.ops[idx(g, name)]["out"].buf


def test_c2f():
    g = c2f_graph()
    c1, a, b, c2 = (idx(g, "m." + n) for n in ("cv1.conv", "m.0.cv1.conv", "m.0.cv2.conv", "cv2.conv"))
    for prec in (F16, BF16, X3):
        r = links(g, prec)
        assert r[c1, C2F:C2F + 3].tolist() == [a, b, c2] and r[[a, b, c2], SKIP].all() and r[:, SKIP].sum() == 3 and r[a, PAIR_B] == b, prec
        assert r[c1, KERNEL] == r[c2, KERNEL] == CONV_C2F_PW and r[a, KERNEL] == r[b, KERNEL] == CONV_PAIR
    assert unfused(links(g, F32))
    r = links(c2f_graph(fourth_reader=True), F16)                 # the concat buffer must exist: the pair alone stays fused
    assert (r[:, C2F] == -1).all() and r[a, PAIR_B] == b and r[:, SKIP].sum() == 1
    assert unfused(links(c2f_graph(fourth_reader=True), X3))      # ... and is released again in the split precision


# ---- Detect heads
def detect_graph(v8, export=False, extra_reader=False, nc=8):
    g, x0 = body(32)
    feats = [x0, g.conv(x0, 32, 3, 2, "p4"), g.conv(g.ops[-1]["out"], 32, 3, 2, "p5")]
    ins = []
    for i, f in enumerate(feats):
        if v8:
            ins += [g.conv(f, 64, 1, 1, f"box{i}", act=M.ACT_NONE, f32_out=True), g.conv(f, nc, 1, 1, f"cls{i}", act=M.ACT_NONE, f32_out=True)]
        else:
            ins.append(g.conv(f, 3 * (nc + 5), 1, 1, f"det{i}", act=M.ACT_NONE, f32_out=True))
    A = sum(f.h * f.w for f in feats) * (1 if v8 else 3)
    head = g.buf(1, 1, (4 + nc if v8 else nc + 5) * A, f32=True)
    g._op(M.OP_DETECT_V8 if v8 else M.OP_DETECT_V5, ins, head, params=[nc, A, 8, 16, 32], name="decode")
    if not v8:
        g.ops[-1]["w"] = g._blob(np.zeros(18, np.float32))
    g.output(head, 0, [1, 4 + nc, A] if v8 else [1, A, nc + 5], "output0")
    if export:
        g.output(ins[-1], 0, [1, ins[-1].h, ins[-1].w, ins[-1].c], "logits")
    if extra_reader:
        g.conv(ins[-1], 32, 1, 1, "r")
    return g


@pytest.mark.parametrize("v8", [True, False], ids=["v8", "v5"])
def test_detect(v8):
    g = detect_graph(v8)
    d = idx(g, "decode")
    src = [idx(g, n) for n in (["box0", "cls0", "box1", "cls1", "box2", "cls2"] if v8 else ["det0", "det1", "det2"])]
    for prec in (F16, BF16) + ((X3,) if v8 else ()):              # (the v5 fusion is 16-bit only: det5_applicable)
        r = links(g, prec)
        assert r[d, DET_SRC:DET_SRC + 6].tolist() == src + [-1] * (6 - len(src)) and r[src, SKIP].all() and r[:, SKIP].sum() == len(src), prec
        assert (r[src, KERNEL] == (CONV_PW if v8 else CONV_DET5)).all()
    assert unfused(links(g, F32))
    assert unfused(links(detect_graph(v8, export=True), F16))         # one logits tensor is a graph output too
    assert unfused(links(detect_graph(v8, extra_reader=True), F16))   # ... or has a second reader
    if v8:     # (the v5 pass has no switch of the loader's: det5_applicable reads ADAS_NO_DETECT_FUSE once per process)
        with env(ADAS_NO_DETECT_FUSE="1"):
            assert unfused(links(g, F16))


# ---- first-layer fusion
def stem_graph(kind, second=True, extra_reader=False):
    """kind 'yolo': 3x3 s2 -> 16 SiLU (+ 3x3 s2 -> 32 SiLU); 'resnet': 7x7 s2 -> 64 ReLU (+ 3x3 s2 p1 max-pool)."""
    g, x, cin = graph(2 * H, 2 * W)
    if kind == "yolo":
        s = g.conv(x, 16, 3, 2, "stem", true_cin=cin)
        n = g.conv(s, 32, 3, 2, "second") if second else g.conv(s, 32, 3, 1, "second")      # (stride 1: not the stem's second conv)
    else:
        s = g.conv(x, 64, 7, 2, "stem", true_cin=cin, act=M.ACT_RELU)
        n = g.maxpool(s, 3, 2, 1, name="second") if second else g.maxpool(s, 2, 2, 0, name="second")
    if extra_reader:
        g.conv(s, 32, 1, 1, "r")
    g.conv(n, 32, 1, 1, "tail")
    return g


@pytest.mark.parametrize("prec", [F16, X3], ids=["fp16", "fp16x3"])
@pytest.mark.parametrize("kind", ["yolo", "resnet"])
def test_stem(kind, prec):
    col = FUSE_CONV2 if kind == "yolo" else FUSE_POOL
    r = links(stem_graph(kind), prec)
    assert r[0, SKIP] == 1 and r[1, KERNEL] == CONV_STEM and r[1, col] == 2 and r[2, SKIP] == 1 and r[:, SKIP].sum() == 2
    assert r[1, FUSE_CONV2 if col == FUSE_POOL else FUSE_POOL] == -1 and (r[2, KERNEL] == CONV_STEM2) == (kind == "yolo")
    for g in (stem_graph(kind, second=False), stem_graph(kind, extra_reader=True)):       # the stem alone
        r = links(g, prec)
        assert r[0, SKIP] == 1 and r[1, KERNEL] == CONV_STEM and r[1, FUSE_POOL] == r[1, FUSE_CONV2] == -1 and r[:, SKIP].sum() == 1
    with env(ADAS_NO_STEM="1"):
        assert unfused(links(stem_graph(kind), prec))
    # each precision's own switch for the op behind the stem; the other precision's switch does nothing here
    own = {("yolo", F16): "ADAS_NO_STEM2", ("resnet", X3): "ADAS_NO_STEM_POOL_X3"}.get((kind, prec))
    for sw in ("ADAS_NO_STEM2", "ADAS_NO_STEM_POOL_X3"):
        with env(**{sw: "1"}):
            r = links(stem_graph(kind), prec)
        assert r[0, SKIP] == 1 and (r[1, col] == 2) == (sw != own), (sw, own)


def test_stem_needs_a_16_bit_or_split_precision():
    assert unfused(links(stem_graph("yolo"), F32)) and unfused(links(stem_graph("resnet"), F32))


def test_boundaries_agree_with_the_recorded_plans():
    """Where the fixture states a boundary the small graphs state too: YOLOv8n's model.2 is a fused C2f block, its Detect head and stem
    are fused, its necks' upsamples folded, its SPPF one launch -- and nothing of it in fp32."""
    g = M.build("yolov8n", wsrc=Z)
    r, _ = RECORDED[G.config_key("yolov8n", "fp16", 64)]
    c1 = idx(g, "model.2.cv1.conv")
    assert r[c1, C2F:C2F + 3].tolist() == [idx(g, "model.2.m.0.cv1.conv"), idx(g, "model.2.m.0.cv2.conv"), idx(g, "model.2.cv2.conv")]
    assert r[1, FUSE_CONV2] == 2 and (r[idx(g, "model.22.decode"), DET_SRC:DET_SRC + 6] >= 0).all()
    assert (r[:, UP_SRC] >= 0).sum() == 2 and (r[:, POOL3] >= 0).sum() == 1
    assert unfused(RECORDED[G.config_key("yolov8n", "fp32", 64)][0])
    r, _ = RECORDED[G.config_key("ufldv2_res18", "fp16", 64)]
    assert r[1, FUSE_POOL] == 2 and (r[:, DS_SRC] >= 0).sum() == 3


def test_non_conv_ops_report_zero_packing():
    g = M.build("yolov8n", wsrc=Z)
    r = links(g, F16)
    other = [i for i, o in enumerate(g.ops) if o["type"] != M.OP_CONV]
    assert len(other) > 5 and not r[other, K:COUT_PAD + 1].any()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def small_tables():
    g, x0 = body(32)
    g.conv(x0, 32, 1, 1, "c1")
    y = g.conv(x0, 8, 1, 1, "out", act=M.ACT_NONE, f32_out=True)
    g.output(y, 0, [1, H, W, 8], "y")
    return g


def patched(g, section, index, field_offset, fmt, value):
    """g's tables with one field overwritten: section 'buf' | 'op' | 'out' | 'hdr', the field's byte offset inside the record."""
    t = bytearray(g.tables())
    base = {"hdr": 0, "buf": M.HDR_SIZE, "op": M.HDR_SIZE + len(g.bufs) * M.BUF_SIZE,
            "out": M.HDR_SIZE + len(g.bufs) * M.BUF_SIZE + len(g.ops) * M.OP_SIZE}[section]
    size = {"hdr": 0, "buf": M.BUF_SIZE, "op": M.OP_SIZE, "out": M.OUT_SIZE}[section]
    struct.pack_into(fmt, t, base + index * size + field_offset, value)
    return bytes(t)


# byte offsets inside a FileOp (csrc/engine.h)
OP_N_IN, OP_IN_BUF, OP_IN_C, OP_OUT_BUF, OP_KW, OP_ACT, OP_RES_MODE, OP_RES_BUF, OP_PARAMS = 4, 8, 72, 104, 120, 132, 136, 140, 200


def refusal_cases():
    g = small_tables()
    t = g.tables()
    c1 = idx(g, "c1")
    yield "not-a-container", b"ADASHIP2" + t[8:], F16, "is not an ADASHIP1 model container"
    yield "short-header", t[:100], F16, "is not an ADASHIP1 model container"
    yield "truncated-tables", t[:M.HDR_SIZE + len(g.bufs) * M.BUF_SIZE + 100], F16, "truncated model container"
    yield "too-many-inputs", patched(g, "op", c1, OP_N_IN, "<I", 9), F16, "more than 8 inputs index out of range (container has 4 buffers)"
    yield "input-index", patched(g, "op", c1, OP_IN_BUF, "<i", 4), F16, "input buffer index out of range"
    yield "output-index", patched(g, "op", c1, OP_OUT_BUF, "<i", -1), F16, "output buffer index out of range"
    yield "residual-index", patched(patched_g(g, c1, OP_RES_MODE, 1), "op", c1, OP_RES_BUF, "<i", 99), F16, "residual buffer index out of range"
    yield "graph-output-index", patched(g, "out", 0, 0, "<I", 7), F16, "graph output buffer index out of range"
    yield "alias-forward", patched(g, "buf", 1, 12, "<I", M.BUF_ALIAS | (2 << 8)), F16, "buffer 1 is not a valid alias"
    yield "alias-size", patched(g, "buf", 2, 12, "<I", M.BUF_ALIAS | (0 << 8)), F16, "buffer 2 is not a valid alias"
    yield "output-not-fp32", patched(g, "buf", 3, 12, "<I", 0), F16, "output y is not an fp32 buffer"
    yield "activation", patched(g, "op", c1, OP_ACT, "<I", M.ACT_HSWISH), F16, "layer c1: activation 4 is not a convolution epilogue"
    # fp16x3: every 16-bit tensor a whole number of 8-channel groups -- the text coreEngine.py's fp16x3 -> fp32 retry keys on
    g12, x0 = body(32)
    g12.conv(x0, 12, 1, 1, "c12")
    yield "multiples-of-8", g12.tables(), X3, "buffer 2 has 12 channels: the split precision (fp16x3) needs multiples of 8"
    # a Linear layer (a 1x1 conv on a 1x1 map) with a residual
    gl, x, cin = graph(1, 1)
    a = gl.conv(x, 64, 1, 1, "fc1", act=M.ACT_RELU)
    gl.conv(a, 64, 1, 1, "fc2", act=M.ACT_RELU, res=a, res_mode=M.RES_AFTER_ACT)
    yield "linear-residual", gl.tables(), F16, "layer fc2: a Linear layer cannot carry a residual"
    # per-operator shapes
    gd, x0 = body(32)
    gd.dwconv(x0, 3, 1, "dw")
    yield "dwconv", patched(gd, "op", idx(gd, "dw"), OP_KW, "<I", 5), F16, "layer dw: unsupported depth-wise convolution shape"
    ga, x0 = body(32)
    ga.attention(ga.conv(x0, 128, 1, 1, "qkv", act=M.ACT_NONE), 2, 16, 32, "attn")
    yield "attention", patched(ga, "op", idx(ga, "attn"), OP_PARAMS, "<f", 3.0), F16, "layer attn: unsupported attention shape"
    gs, x0 = body(32)
    gs.shuffle(x0, 2, "shuf")
    yield "shuffle", patched(gs, "op", idx(gs, "shuf"), OP_PARAMS, "<f", 5.0), F16, "layer shuf: unsupported channel shuffle shape"
    gw, x0 = body(32)
    gw.wsum([x0, x0], [0.5, 0.5], "sum")
    yield "wsum", patched(gw, "op", idx(gw, "sum"), OP_ACT, "<I", 7), F16, "layer sum: unsupported weighted sum shape"
    ge, x0 = body(32)
    ge.se(x0, 8, "se")
    yield "se-gate", patched(ge, "op", idx(ge, "se.gate"), OP_PARAMS, "<f", 9.0), F16, "unsupported squeeze-and-excitation shape"
    yield "scale", patched(ge, "op", len(ge.ops) - 1, OP_N_IN, "<I", 1), F16, "unsupported channel scale shape"
    gp, x0 = body(32)
    gp._op(M.OP_DEPTH2SPACE, [x0], gp.buf(2 * H, 2 * W, 8), name="d2s")
    yield "depth2space", patched(gp, "op", idx(gp, "d2s"), OP_IN_C, "<i", 24), F16, "layer d2s: unsupported depth-to-space shape"
    # YOLOv6 Detect
    g6, x0 = body(32)
    ins = []
    for i in range(3):
        ins += [g6.conv(x0, 4, 1, 1, f"reg{i}", act=M.ACT_NONE, f32_out=True), g6.conv(x0, 8, 1, 1, f"cls{i}", act=M.ACT_NONE, f32_out=True)]
    g6._op(M.OP_DETECT_V6, ins, g6.buf(1, 1, 12 * 3 * H * W, f32=True), params=[8, 3 * H * W, 8, 16, 32, 0], name="det6")
    d6 = idx(g6, "det6")
    yield "detect-v6-inputs", patched(g6, "op", d6, OP_N_IN, "<I", 5), F16, "layer det6: unsupported Detect shape"
    yield "reg-max", patched(g6, "op", d6, OP_PARAMS + 20, "<f", 8.0), F16, "layer det6: YOLOv6 Detect: reg_max 8 is not supported (0: 4 distance channels; 16: 4 x 17 DFL bins)"
    yield "reg-max-channels", patched(g6, "op", d6, OP_PARAMS + 20, "<f", 16.0), F16, \
        "layer det6: YOLOv6 Detect: level 0 regression input has 4 channels, reg_max 16 needs 4 x (reg_max + 1) = 68"


def patched_g(g, op, field_offset, value):
    """A stand-in for `g` whose tables() carry one more patched uint32 of an op (so that two fields can be damaged)."""
    class _G:
        bufs, ops = g.bufs, g.ops
        tables = staticmethod(lambda: patched(g, "op", op, field_offset, "<I", value))
    return _G


REFUSALS = list(refusal_cases())


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusal(case):
    _, tables, prec, text = case
    with pytest.raises(L.AdasError) as ex:
        plan(tables, prec)
    assert ex.value.code == -3 and text in str(ex.value), str(ex.value)


def test_sound_tables_are_not_refused():
    for prec in (F16, BF16, F32, X3):
        plan(small_tables().tables(), prec)


def test_the_fp16x3_fallback_keys_on_the_loaders_text():
    """coreEngine.py retries an fp16x3 engine in fp32 when the refusal says "needs multiples of 8": the substring it looks for is in its
    source, and in the text the loader gives."""
    src = open(os.path.join(os.path.dirname(L.__file__), "coreEngine.py")).read()
    assert '"needs multiples of 8" not in str(ex)' in src
    text = [c[3] for c in REFUSALS if c[0] == "multiples-of-8"][0]
    assert "needs multiples of 8" in text


def write_refusal_cases(directory):
    """The damaged tables as files (tools: the stand-alone sanitizer harness of csrc/engine_load.cpp reads them): <id>.<precision>.tables"""
    os.makedirs(directory, exist_ok=True)
    for name, tables, prec, _ in REFUSALS:
        with open(os.path.join(directory, f"{name}.{prec}.tables"), "wb") as f:
            f.write(tables)
