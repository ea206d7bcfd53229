"""GPU: the depth-wise conv and attention kernels of csrc/dw_attn.hip, ONE launch at a time, element by element against float64
(tests/dw_attn_ref.py: half an ulp of the storage type plus a slack derived there; nothing read off the device enters a bound).
tests/test_gpu_v10.py judges the same kernels by a whole-tensor norm; tests/test_dw_attn_ref_cpu.py shows what that lets through.

Depth-wise.  Unit graph  input -> 1x1 "expand" (no activation: signed values) -> dwconv "test" -> 1x1 fp32 "tap";  the residual is a
second 1x1 conv "resid" of the graph input.  The conv's INPUT, residual and OUTPUT are fetched, the reference is applied to the fetched
operands with the container's float32 taps and bias.  Batch 3, distinct frames uniform(-1, 1), all four precisions.  The dispatcher
takes dwconv_strip_kernel when Wo >= 4 and ADAS_NO_DW_STRIP is not 1 (read at every launch): every case with Wo >= 4 runs BOTH forms
in one engine, each is checked against float64 and the two are asserted bit-identical.  Cases with Wo < 4 reach only dwconv_kernel.

  id            map    k s  c   act    res  Wo  what it is for
  k3s1          23x37  3 1  40  silu   yes  37  37 mod 4 = 1: a last strip with one real output
  k3s2          23x37  3 2  96  leaky  -    19  19 mod 4 = 3
  k5s1          23x37  5 1  8   leaky  yes  37  one 8-channel group
  k5s2          23x37  5 2  40  silu   -    19
  k7s1          23x37  7 1  96  relu   yes  37
  k7s2          23x37  7 2  8   none   -    19
  even14x12     14x12  3 2  40  relu   -    6   even extents: the last window hangs over the right and bottom edges only
  even8x8       8x8    7 2  96  leaky  -    4   exactly one strip a row
  even6x10      6x10   5 2  8   none   -    5
  win7          3x5    7 1  40  silu   yes  5   the window is larger than the map: every row and column test clamps somewhere; the
  win5          3x5    5 1  96  relu   -    5   second strip of a row holds one real output
  plain5x3      5x3    3 1  40  leaky  yes  3   plain kernel only (Wo < 4), as the dispatcher picks it
  plain6x6s2    6x6    5 2  96  silu   -    3   plain kernel only
  plain1x1      1x1    7 1  8   relu   -    1   plain kernel only: 3 work items in all, fewer than dwconv_kernel's 8 XCD partitions
  pe            9x11   3 1  64  none   yes  11  PSA's positional encoding as models._psa_block builds it, nh = 2: input qkv.slice(h 128 + 64, 64)
                                                of a 256-wide buffer, output and residual 64-channel slices at h 64 of two other buffers,
                                                one launch per head, the shared (128, 1, 3, 3) parameter cut per head
  guard         9x11   5 1  40  silu   yes  11  the output is a slice between guard channels (test_gpu_ops_exact._guarded): the guards
                                                survive and the slice holds no guard value
Every k sees none, SiLU, ReLU and leaky in both forms (k = 3: k3s1, k3s2, even14x12, pe; k = 5: k5s1, k5s2, even6x10, win5; k = 7: k7s1, k7s2,
even8x8, win7).  d.small == 0 (the 64-bit index path of dwconv_kernel) needs 2^31 work items and is out of scope.

Attention.  Unit graph  input -> 1x1 "expand" (SiLU) -> 1x1 "qkv" (no activation, no bias) -> attention "test" -> 1x1 fp32 "tap";  qkv and
the output are fetched.  Batch 3, distinct frames, key_dim 32 and head_dim 64 (the only supported sizes).  A 16-bit qkv buffer is
aligned, so fp16 and bf16 run attention_mfma_kernel here; fp32 and fp16x3 run attention_kernel<float | x3s>;
attention_kernel<f16s | uint16_t> runs in a child process under ADAS_NO_ATTN_MFMA=1 (the switch is cached at the first launch).
The qkv weights carry a gain computed on the CPU from the float64 forward of the case's own frames and weights so that the largest
|score| sits at a target: 8 (base), 0.5 (flat), 60 (peaked), 12 (the ramps).

  id         map (N)      nh  what it is for
  n1         1x1 (1)      1   one token: the softmax is 1, every other lane is padding
  n63 n64 n65  9x7 8x8 5x13   1 2 1   around the scalar kernel's 64-key chunk and the MFMA kernel's 64-query workgroup
  n128 n129  8x16 3x43    2 1   around the MFMA kernel's 128-key chunk and the scalar kernel's 128-query workgroup; N = 129: a chunk of one key
  n400       20x20 (400)  4   the network's shape: 4 MFMA chunks, 7 scalar chunks, ragged in both
  n65|n129|n400-flat      |score| < 1 (asserted on the float64 scores)
  n65|n129|n400-peaked    40 <= max |score| <= 80 (asserted on the float64 scores)
  n400-rise  each frame times ((j + 1) / N)^32 over the token index j: the running maximum arrives in the last chunk (keys 384 ... 399 for
             both kernels) and every earlier chunk is rescaled; asserted: the arg-max key of most queries lies there
  n400-fall  times ((N - j) / N)^8: the maximum arrives in the first chunk (keys 0 ... 63); asserted likewise
  n129-slice qkv is slice(8, .) of a wider buffer and the output lies between guard channels: in_coff, out_cs, out_coff, and the MFMA kernel's
             `aligned` branch at a non-zero offset; the guards survive

Measured on an MI355X (reported, fed back into nothing), worst |err| / bound: depth-wise strip = plain 0.14 (fp32) / 1.00 (fp16) / 1.00 (bf16) /
0.14 (fp16x3) -- a correctly rounded 16-bit store uses its whole half ulp at a near-tie; attention_kernel 0.16 (fp32) / 0.16 (fp16x3) / 0.88
(f16s) / 0.98 (bf16); attention_mfma_kernel 0.52 (fp16) / 0.60 (bf16).  The file takes 16 s."""
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dw_attn_ref as DA
import ops_ref as R
from conftest import load_pkg
from test_gpu_ops_exact import _check_guards, _guarded

pytestmark = pytest.mark.gpu
load_pkg()
CE = importlib.import_module("adas_amd.coreEngine")
M = importlib.import_module("adas_amd.models")

assert (M.ACT_NONE, M.ACT_SILU, M.ACT_RELU, M.ACT_LEAKY) == (R.ACT_NONE, R.ACT_SILU, R.ACT_RELU, R.ACT_LEAKY)
NONE, SILU, RELU, LEAKY = R.ACT_NONE, R.ACT_SILU, R.ACT_RELU, R.ACT_LEAKY
BATCH = 3
PRECS = list(R.PRECISIONS)
TESTS = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------------------------ depth-wise conv
def D(cid, hw, k, s, c, act, res=False, kind="unit"):
    return dict(id=cid, hw=hw, k=k, s=s, c=c, act=act, res=res, kind=kind)


DW_CASES = [
    D("k3s1", (23, 37), 3, 1, 40, SILU, True), D("k3s2", (23, 37), 3, 2, 96, LEAKY),
    D("k5s1", (23, 37), 5, 1, 8, LEAKY, True), D("k5s2", (23, 37), 5, 2, 40, SILU),
    D("k7s1", (23, 37), 7, 1, 96, RELU, True), D("k7s2", (23, 37), 7, 2, 8, NONE),
    D("even14x12", (14, 12), 3, 2, 40, RELU), D("even8x8", (8, 8), 7, 2, 96, LEAKY), D("even6x10", (6, 10), 5, 2, 8, NONE),
    D("win7", (3, 5), 7, 1, 40, SILU, True), D("win5", (3, 5), 5, 1, 96, RELU),
    D("plain5x3", (5, 3), 3, 1, 40, LEAKY, True), D("plain6x6s2", (6, 6), 5, 2, 96, SILU), D("plain1x1", (1, 1), 7, 1, 8, RELU),
    D("pe", (9, 11), 3, 1, 64, NONE, True, kind="pe"),
    D("guard", (9, 11), 5, 1, 40, SILU, True, kind="guard"),
]
assert len({c["id"] for c in DW_CASES}) == len(DW_CASES)
PE_NH = 2


def dw_out_hw(c):
    (H, W), k, s = c["hw"], c["k"], c["s"]
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def dw_forms(c):
    """The forms a case reaches: the dispatcher's own choice first."""
    return ("strip", "plain") if dw_out_hw(c)[1] >= 4 else ("plain",)


def dw_graph(c, wsrc=None):
    """The unit graph of a case.  Returns (graph, weights, names to fetch, launches): a launch is (layer name, offset of its input in
    "expand", offset of its residual in "resid", offset of its channels in the test.weight / test.bias parameter)."""
    H, W = c["hw"]
    ws = wsrc if wsrc is not None else M.SynthWeights(23, gain=1.0)
    g = M.Graph("dwunit", 3, H, W, ws)
    x, c3 = g.input()
    k, s, ch = c["k"], c["s"], c["c"]
    Ho, Wo = dw_out_hw(c)
    fetch = ["expand"]
    if c["kind"] == "pe":         # models._psa_block: v of head h is qkv channel h * (2 kd + hd) + 2 kd ...; summed = att + pe(v)
        qkv = g.conv(x, PE_NH * 128, 1, 1, "expand", act=NONE, true_cin=c3)
        att = g.conv(x, PE_NH * 64, 1, 1, "resid", act=NONE, true_cin=c3)
        pw, pb = ws("test.weight", (PE_NH * 64, 1, 3, 3), "conv"), ws("test.bias", (PE_NH * 64,), "bias")
        y = g.buf(H, W, PE_NH * 64)
        launches = []
        for h in range(PE_NH):
            g.dwconv(qkv.slice(h * 128 + 64, 64), 3, 1, "test.h%d" % h, act=NONE, out=y.slice(h * 64, 64), res=att.slice(h * 64, 64),
                     weight=pw[h * 64:(h + 1) * 64], bias=pb[h * 64:(h + 1) * 64])
            launches.append(("test.h%d" % h, h * 128 + 64, h * 64, h * 64))
        fetch += ["resid"] + [l[0] for l in launches]
    else:
        a = g.conv(x, ch, 1, 1, "expand", act=NONE, true_cin=c3)
        res = None
        if c["res"]:
            assert s == 1
            res = g.conv(x, ch, 1, 1, "resid", act=NONE, true_cin=c3)
            fetch.append("resid")
        if c["kind"] == "guard":
            y, out = _guarded(g, x, c3, Ho, Wo, ch, geom=(1, s, 0))         # the tap reads the whole guarded buffer
            g.dwconv(a, k, s, "test", act=c["act"], out=out, res=res)
            fetch += ["guard_lo", "guard_hi"]
        else:
            y = g.dwconv(a, k, s, "test", act=c["act"], res=res)
        launches = [("test", 0, 0, 0)]
        fetch.append("test")
    z = g.conv(y, 8, 1, 1, "tap", act=NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    return g, ws, fetch, launches


def dw_frames(c):
    H, W = c["hw"]
    return np.random.default_rng(5).uniform(-1, 1, (BATCH, 3, H, W)).astype(np.float32)


def run_dw(tmp_path, c, prec, monkeypatch):
    """{form: {layer: fetched activation}} of the forms the case reaches, from one engine."""
    g, ws, fetch, launches = dw_graph(c)
    path = str(tmp_path / "dwunit.hipm")
    g.save(path)
    xin = dw_frames(c)
    acts = {}
    e = CE.HipEngine(path, prec, BATCH)
    try:
        for name, _, _, _ in launches:
            assert "dwconv" in e.layer_kernel(e.layer_index(name), BATCH)
        for form in dw_forms(c):
            if form == "plain":
                monkeypatch.setenv("ADAS_NO_DW_STRIP", "1")
            else:
                monkeypatch.delenv("ADAS_NO_DW_STRIP", raising=False)
            e.engine_inference(xin)
            acts[form] = {n: e.fetch_activation(n, BATCH).copy() for n in fetch}
    finally:
        e.close()
        monkeypatch.delenv("ADAS_NO_DW_STRIP", raising=False)
    return ws, launches, acts


def check_dw(c, prec, ws, launches, acts):
    """Every launch of every form against float64.  Returns {form: worst |err| / bound}."""
    k, s, ch = c["k"], c["s"], c["c"]
    worst = {}
    first = acts[dw_forms(c)[0]]
    for form, a in acts.items():
        worst[form] = 0.0
        for name, xo, ro, wo in launches:
            x = a["expand"][:, xo:xo + ch]
            r = a["resid"][:, ro:ro + ch] if c["res"] else None
            assert np.array_equal(a["expand"], first["expand"]) and (not c["res"] or np.array_equal(a["resid"], first["resid"]))
            assert x.shape[0] == BATCH and not np.array_equal(x[0], x[1]) and not np.array_equal(x[1], x[2]), "distinct frames"
            assert (x > 0).mean() > 0.2 and (x < 0).mean() > 0.2 and np.abs(x).max() < 1e3, "signed inputs"
            w, b = ws.store["test.weight"][wo:wo + ch], ws.store["test.bias"][wo:wo + ch]       # float32, unrounded in every precision
            want, S, v = DA.dw_layer_ref(x, w, b, s, c["act"], r)
            got = a[name]
            assert got.shape == want.shape == (BATCH, ch) + dw_out_hw(c), (got.shape, want.shape)
            if c["act"] in (RELU, LEAKY):
                assert (v < 0).mean() > 0.2 and (v > 0).mean() > 0.2, "both branches of the activation"
            yard = DA.dw_yardstick(x, w, b, s, c["act"], r, want, S)
            ok, wr, err = DA.check(got, want, prec, DA.dw_slack(S, v, prec, c["act"]))
            print("dw %s %s %s %s: worst |err| / bound %.3f (|err| %.3e)  yardstick ratio %.3f" % (c["id"], prec, form, name, wr, err, yard))
            assert yard <= DA.CR.YARD_CONV, (yard, DA.CR.YARD_CONV)
            assert ok.all(), (form, name, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), got[~ok][:4], want[~ok][:4])
            worst[form] = max(worst[form], wr)
            if c["kind"] == "guard":
                _check_guards(a, got, want, prec)
    if len(acts) == 2:
        for name, _, _, _ in launches:
            assert np.array_equal(acts["strip"][name].view(np.uint32), acts["plain"][name].view(np.uint32)), "%s: the two forms differ" % name
    return worst


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", DW_CASES, ids=lambda c: c["id"])
def test_depthwise_per_element(tmp_path, monkeypatch, c, prec):
    ws, launches, acts = run_dw(tmp_path, c, prec, monkeypatch)
    assert tuple(acts) == dw_forms(c)
    check_dw(c, prec, ws, launches, acts)


# ------------------------------------------------------------------------------------------------------------------------ attention
TARGET = {"base": 8.0, "flat": 0.5, "peaked": 60.0, "rise": 12.0, "fall": 12.0}
CE_CH = 32                      # channels of the expand layer


def A(cid, hw, nh, variant="base", sliced=False):
    return dict(id=cid, hw=hw, nh=nh, variant=variant, sliced=sliced)


ATT_CASES = [A("n1", (1, 1), 1), A("n63", (9, 7), 1), A("n64", (8, 8), 2), A("n65", (5, 13), 1), A("n128", (8, 16), 2), A("n129", (3, 43), 1),
             A("n400", (20, 20), 4)]
for _cid, _hw, _nh in (("n65", (5, 13), 1), ("n129", (3, 43), 1), ("n400", (20, 20), 4)):
    ATT_CASES += [A(_cid + "-flat", _hw, _nh, "flat"), A(_cid + "-peaked", _hw, _nh, "peaked")]
ATT_CASES += [A("n400-rise", (20, 20), 4, "rise"), A("n400-fall", (20, 20), 4, "fall"), A("n129-slice", (3, 43), 1, sliced=True)]
assert len({c["id"] for c in ATT_CASES}) == len(ATT_CASES)
SCALAR16_CASES = ("n65", "n129", "n400")      # run by the child under ADAS_NO_ATTN_MFMA=1, in fp16 and bf16


def att_frames(c):
    """Distinct signed frames; the ramp variants multiply every frame by a power ramp over the token index."""
    H, W = c["hw"]
    N = H * W
    x = np.random.default_rng(7).uniform(-1, 1, (BATCH, 3, H, W))
    j = np.arange(N, dtype=np.float64).reshape(H, W)
    if c["variant"] == "rise":
        x = x * ((j + 1) / N) ** 32
    elif c["variant"] == "fall":
        x = x * ((N - j) / N) ** 8
    return x.astype(np.float32)


def _qkv_gain(c, we, be, wq):
    """The gain of the qkv weights that puts the largest |score| of the case's float64 forward at TARGET[variant] (scores are
    quadratic in it: the qkv conv has no bias).  A CPU computation on the case's own frames and weights."""
    x = att_frames(c).astype(np.float64)
    a = np.einsum("oc,bchw->bohw", we.reshape(CE_CH, 3).astype(np.float64), x) + be.astype(np.float64)[None, :, None, None]
    a = a / (1.0 + np.exp(-a))
    qkv = np.einsum("oc,bchw->bohw", wq.reshape(-1, CE_CH).astype(np.float64), a)
    q, k, _ = DA.split_heads(qkv, c["nh"])
    s0 = np.abs(DA.SCALE * np.einsum("bhci,bhcj->bhij", q, k)).max()
    return float(np.sqrt(TARGET[c["variant"]] / s0)) if s0 > 0 else 1.0


def att_graph(c, wsrc=None):
    """The unit graph of a case.  Returns (graph, names to fetch)."""
    H, W = c["hw"]
    nh = c["nh"]
    cq = nh * DA.HC
    ws = wsrc if wsrc is not None else M.SynthWeights(29, gain=1.0)
    g = M.Graph("attnunit", 3, H, W, ws)
    x, c3 = g.input()
    a = g.conv(x, CE_CH, 1, 1, "expand", act=SILU, true_cin=c3)
    wq = np.asarray(ws("qkv.weight", (cq, CE_CH, 1, 1), "conv"), np.float32)
    gain = _qkv_gain(c, np.asarray(ws("expand.weight", (CE_CH, 3, 1, 1), "conv")), np.asarray(ws("expand.bias", (CE_CH,), "bias")), wq)
    wq = (wq * np.float32(gain)).astype(np.float32)
    fetch = ["qkv", "test"]
    if c["sliced"]:
        pad = np.asarray(ws("qkv.pad", (8, CE_CH, 1, 1), "conv"), np.float32)
        full = g.conv(a, cq + 16, 1, 1, "qkv", act=NONE, bias=False, weight=np.concatenate([pad, wq, pad], 0))
        y, out = _guarded(g, x, c3, H, W, nh * DA.HD)                        # the tap reads the whole guarded buffer
        g.attention(full.slice(8, cq), nh, DA.KD, DA.HD, "test", out=out)
        fetch += ["guard_lo", "guard_hi"]
    else:
        qkv = g.conv(a, cq, 1, 1, "qkv", act=NONE, bias=False, weight=wq)
        y = g.attention(qkv, nh, DA.KD, DA.HD, "test")
    z = g.conv(y, 8, 1, 1, "tap", act=NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    return g, fetch


def run_att(tmp_dir, c, prec):
    g, fetch = att_graph(c)
    path = os.path.join(str(tmp_dir), "attnunit.hipm")
    g.save(path)
    e = CE.HipEngine(path, prec, BATCH)
    try:
        assert "attention" in e.layer_kernel(e.layer_index("test"), BATCH)
        e.engine_inference(att_frames(c))
        acts = {n: e.fetch_activation(n, BATCH).copy() for n in fetch}
    finally:
        e.close()
    return acts


def assert_variant(c, ref):
    """The case still makes its point: asserted on the float64 scores of the qkv it is given."""
    s = ref["s"]
    N, smax = s.shape[-1], float(np.abs(s).max())
    if c["variant"] == "flat":
        assert smax < 1.0, smax
    elif c["variant"] == "peaked":
        assert 40.0 <= smax <= 80.0, smax
    elif c["variant"] in ("rise", "fall"):
        arg = s.argmax(-1)
        for chunk in (DA.SCALAR_CHUNK, DA.MFMA_CHUNK):
            last0 = (N - 1) // chunk * chunk
            frac = float((arg >= last0).mean()) if c["variant"] == "rise" else float((arg < chunk).mean())
            assert frac > 0.5, (c["id"], chunk, frac)
    return smax


def check_att(c, prec, acts, kernel):
    """The fetched output against float64 on the fetched qkv under `kernel`'s bound.  Returns the worst |err| / bound."""
    nh = c["nh"]
    cq = nh * DA.HC
    qkv = acts["qkv"][:, 8:8 + cq] if c["sliced"] else acts["qkv"]
    got = acts["test"]
    assert qkv.shape == (BATCH, cq) + c["hw"] and got.shape == (BATCH, nh * DA.HD) + c["hw"], (qkv.shape, got.shape)
    assert not np.array_equal(qkv[0], qkv[1]) and not np.array_equal(qkv[1], qkv[2]), "distinct frames"
    ref = DA.attn_ref(qkv, nh)
    smax = assert_variant(c, ref)
    yard, y1, y2 = DA.attn_yardstick(qkv, nh, ref)
    ok, worst, err = DA.check(got, ref["want"], prec, DA.attn_slack(ref, kernel, prec))
    print("attention %s %s %s: worst |err| / bound %.3f (|err| %.3e)  max |score| %.2f  yardstick ratio %.3f (online %.3f, two-pass %.3f)"
          % (c["id"], prec, kernel, worst, err, smax, yard, y1, y2))
    assert yard <= DA.YARD_ATT, (yard, DA.YARD_ATT)
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), got[~ok][:4], ref["want"][~ok][:4])
    if c["sliced"]:
        _check_guards(acts, got, ref["want"], prec)
    return worst


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", ATT_CASES, ids=lambda c: c["id"])
def test_attention_per_element(tmp_path, c, prec):
    """attention_kernel<float | x3s> (fp32, fp16x3) and attention_mfma_kernel<Fp16 | Bf16> (fp16, bf16: the buffers are aligned)."""
    check_att(c, prec, run_att(tmp_path, c, prec), DA.kernel_of(prec))


def scalar16_child():
    """In a process started with ADAS_NO_ATTN_MFMA=1: attention_kernel<f16s | uint16_t> on SCALAR16_CASES under the SCALAR bound; one
    JSON line per case with the worst |err| / bound."""
    assert os.environ.get("ADAS_NO_ATTN_MFMA") == "1"
    by_id = {c["id"]: c for c in ATT_CASES}
    with tempfile.TemporaryDirectory() as tmp:
        for cid in SCALAR16_CASES:
            for prec in ("fp16", "bf16"):
                c = by_id[cid]
                nh = c["nh"]
                acts = run_att(tmp, c, prec)
                ref = DA.attn_ref(acts["qkv"], nh)
                yard = DA.attn_yardstick(acts["qkv"], nh, ref)[0]
                ok, worst, err = DA.check(acts["test"], ref["want"], prec, DA.attn_slack(ref, "scalar", prec))
                print(json.dumps(dict(id=cid, prec=prec, worst=worst, err=err, yard=yard, bad=int((~ok).sum()))), flush=True)


CHILD = "import sys; sys.path.insert(0, sys.argv[1]); import test_gpu_dw_attn_exact as T; T.scalar16_child()"


def test_scalar_16_bit_attention_kernels_in_a_fresh_process():
    """attention_kernel<f16s> and attention_kernel<uint16_t> are reached only with ADAS_NO_ATTN_MFMA=1, which the launcher reads once per
    process: a fresh child runs the 65-, 129- and 400-token cases in fp16 and bf16 under the scalar bound.  Nothing is retried."""
    r = subprocess.run([sys.executable, "-c", CHILD, TESTS], env=dict(os.environ, ADAS_NO_ATTN_MFMA="1"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    for row in rows:
        print("attention %(id)s %(prec)s scalar (child): worst |err| / bound %(worst).3f (|err| %(err).3e)  yardstick ratio %(yard).3f" % row)
    assert sorted((row["id"], row["prec"]) for row in rows) == sorted((cid, p) for cid in SCALAR16_CASES for p in ("fp16", "bf16"))
    for row in rows:
        assert row["worst"] <= 1.0 and row["bad"] == 0 and row["yard"] <= DA.YARD_ATT, row
