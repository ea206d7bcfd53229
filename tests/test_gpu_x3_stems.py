"""GPU: the split precision's first-layer kernels and LayerNorm at their own edges, each against a float64 torch reference of the same
operation and each with the kernel label that proves which kernel ran.

- conv_stem_pool_x3_kernel (conv_stem_x3.hip): the ResNet stem, 7x7 s2 conv + ReLU + 3x3 s2 p1 max-pool in one launch.  Every case also
  runs with ADAS_NO_STEM_POOL_X3=1 (conv_stem_x3_kernel<7,4,RELU>, then the x3 max-pool) and ADAS_NO_STEM=1 (input conversion, generic x3
  conv, max-pool): all three within X3_REL of float64, and the fused pool bit-identical to the two-launch one.
- conv_stem_x3_kernel<KH,NT,ACT>: every instantiation (KH 3 / 6 x 16..80 channels, 7x7 x 64), pads 0..kh/2, 1..3 input channels, ragged
  and sub-tile extents, more tiles than the 512-workgroup grid, a channel-slice output; and the first convs the stem gates refuse
  (stem_x3_applicable), which take the generic x3 path to the same bound.
- layernorm_kernel<T> (aux_kernels.hip) in all four precisions: rows far from zero (offset 100, spread ~1), lengths below one
  workgroup's 256 threads, ragged, CULane's 4,000 and above 8,192.

ADAS_NO_STEM and ADAS_NO_STEM_POOL_X3 are read at every engine creation (engine_load.cpp, fuse_stem) and are toggled here; ADAS_NO_STEM2_X3 and
ADAS_STEMP_X3_WGS are read once per process and are not.
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg

pytestmark = pytest.mark.gpu
load_pkg()
M = importlib.import_module("adas_amd.models")
CE = importlib.import_module("adas_amd.coreEngine")

X3_REL = 3e-6      # tests/test_gpu_x3.py: rel-L2 of one layer in the split precision
X3_MAX = 1e-4      # max|diff| alongside it

ACTS = {M.ACT_SILU: F.silu, M.ACT_RELU: F.relu, M.ACT_LEAKY: lambda v: F.leaky_relu(v, 0.1)}
ACT_NAME = {M.ACT_SILU: "SILU", M.ACT_RELU: "RELU", M.ACT_LEAKY: "LEAKY"}


def _conv_out(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def _errors(got, want):
    d = got.astype(np.float64) - want
    return float(np.linalg.norm(d) / (np.linalg.norm(want) + 1e-300)), float(np.abs(d).max())


def stem_graph(path, H, W, cin, k, s, pad, cout, act, pool, coff=None, seed=0):
    """NCHW fp32 input (cin channels) -> k x k stride-s conv (+ 3x3 s2 p1 max-pool) -> f32 1x1 tap.  coff: the last layer before the tap
    writes channels [coff, coff + cout) of a buffer 16 channels wider than it."""
    ws = M.SynthWeights(seed, gain=1.0)
    g = M.Graph("stemx3unit", cin, H, W, ws)
    x, ct = g.input()
    ho, wo = _conv_out(H, k, s, pad), _conv_out(W, k, s, pad)
    hp, wp = _conv_out(ho, 3, 2, 1), _conv_out(wo, 3, 2, 1)
    slot = None
    if coff is not None:
        oh, ow = (hp, wp) if pool else (ho, wo)
        slot = g.buf(oh, ow, cout + 16).slice(coff, cout)
    y = g.conv(x, cout, k, s, "stem", act=act, true_cin=ct, pad=pad, out=None if pool else slot)
    last = g.maxpool(y, 3, 2, 1, out=slot, name="pool") if pool else y
    z = g.conv(last, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=True)
    g.output(z, 0, [1, z.h * z.w * 8], "o")
    g.save(path)
    return {n: torch.from_numpy(v).double() for n, v in ws.store.items()}


def stem_reference(xin, Wt, s, pad, act, pool):
    with torch.no_grad():
        y = ACTS[act](F.conv2d(torch.from_numpy(xin).double(), Wt["stem.weight"], Wt["stem.bias"], stride=s, padding=pad))
        return (F.max_pool2d(y, 3, 2, 1) if pool else y).numpy()


def run_engine(path, batch, xin, fetch, labels):
    e = CE.HipEngine(path, "fp16x3", batch)
    try:
        e.engine_inference(xin)
        got = e.fetch_activation(fetch, batch)
        names = {n: e.layer_kernel(e.layer_index(n), batch) for n in labels}
    finally:
        e.close()
    return got, names


# ---------------------------------------------------------------------------------------------------------------- stem + max-pool
#            H    W   cin pad batch coff      conv extent   pooled extent (tiles of 4 x 16 pooled pixels)
STEM_POOL = [(64, 128, 3, 3, 2, None),   # 32 x 64      16 x 32: whole tiles
             (62, 150, 3, 3, 3, None),   # 31 x 75      16 x 38: odd conv extents (a phantom conv row and column), ragged columns
             (59, 101, 3, 0, 2, None),   # 27 x 48      14 x 24: pad 0, odd height, ragged rows and columns
             (60, 90, 2, 1, 1, None),    # 28 x 43      14 x 22: pad 1, two input channels, batch 1
             (45, 77, 1, 2, 2, None),    # 22 x 38      11 x 19: pad 2, one input channel
             (9, 20, 3, 3, 2, None),     # 5 x 10       3 x 5: smaller than one tile
             (130, 262, 3, 3, 9, None),  # 65 x 131     33 x 66: 405 tiles on the 256-workgroup grid, odd extents
             (62, 150, 3, 3, 2, 8),      # pooled output into channels 8..71 of an 80-channel buffer
             (45, 77, 2, 2, 2, 16)]      # ... into channels 16..79


@pytest.mark.parametrize("case", STEM_POOL, ids=str)
def test_stem_pool_x3_kernel(case, tmp_path, monkeypatch):
    """The fused launch keeps the conv tile (incl. the pool's halo) in LDS as fp32: conv pixels outside the conv map are the pool's
    padding through the `valid` mask alone -- with an odd conv extent the last pooled row / column reaches one conv pixel past the map,
    whose conv value is computed from real input pixels.  The fused output equals the two-launch one bit for bit: both stem kernels run
    the same K order (per tap row: main += hi.hi, cross += lo.hi, cross += hi.lo) and the same epilogue expression, and the separate pool
    takes its maximum on joined values (joining a split value is exact, and join(split(.)) is monotone)."""
    H, W, cin, pad, batch, coff = case
    path = str(tmp_path / "stempool.hipm")
    Wt = stem_graph(path, H, W, cin, 7, 2, pad, 64, M.ACT_RELU, True, coff=coff)
    xin = np.random.default_rng(3).uniform(-1, 1, (batch, cin, H, W)).astype(np.float32)
    want = stem_reference(xin, Wt, 2, pad, M.ACT_RELU, True)
    ho, wo = _conv_out(H, 7, 2, pad), _conv_out(W, 7, 2, pad)
    hp, wp = _conv_out(ho, 3, 2, 1), _conv_out(wo, 3, 2, 1)
    tiles = batch * ((hp + 3) // 4) * ((wp + 15) // 16)
    outs = {}
    for mode, env in (("fused", None), ("two launches", "ADAS_NO_STEM_POOL_X3"), ("generic", "ADAS_NO_STEM")):
        if env:
            monkeypatch.setenv(env, "1")
        got, names = run_engine(path, batch, xin, "pool", ("input", "stem", "pool"))
        if env:
            monkeypatch.delenv(env)
        rel, mx = _errors(got, want)
        print("x3 stem+pool %s conv %dx%d pooled %dx%d (%d tiles) %-12s: rel %.2e (bound %.0e)  max|diff| %.2e (bound %.0e)  %s"
              % (case, ho, wo, hp, wp, tiles, mode, rel, X3_REL, mx, X3_MAX, names))
        if mode == "fused":
            assert names["stem"].startswith("conv_stem_x3_kernel<7,4,RELU>") and names["pool"] == "(fused into the stem launch)", names
        elif mode == "two launches":
            assert names["stem"] == "conv_stem_x3_kernel<7,4,RELU>" and "maxpool" in names["pool"], names
        else:
            assert names["input"] == "input_nchw_kernel" and "x3" in names["stem"] and "stem" not in names["stem"], names
            assert "maxpool" in names["pool"], names
        assert got.shape == want.shape, (got.shape, want.shape)
        assert rel < X3_REL and mx < X3_MAX, (case, mode, rel, mx)
        outs[mode] = got
    assert np.abs(outs["fused"]).max() > 0.1
    np.testing.assert_array_equal(outs["fused"], outs["two launches"])


# ---------------------------------------------------------------------------------------------------------------- stem without its pool
#          H    W   cin  k  pad cout  act          batch coff     conv extent (tiles: 8 x 32, 7x7: 6 x 32)
STEM = [(64, 64, 3, 3, 1, 16, M.ACT_SILU, 3, None),     # 32 x 32: whole tiles
        (70, 90, 3, 3, 0, 32, M.ACT_RELU, 2, None),     # 34 x 44: pad 0
        (61, 131, 2, 3, 1, 48, M.ACT_LEAKY, 2, None),   # 31 x 66
        (640, 640, 3, 3, 1, 64, M.ACT_SILU, 2, None),   # 320 x 320: 800 tiles on the 512-workgroup grid
        (33, 47, 1, 3, 0, 80, M.ACT_SILU, 3, None),     # 16 x 23
        (9, 13, 3, 3, 1, 16, M.ACT_RELU, 2, None),      # 5 x 7: smaller than one tile
        (45, 77, 3, 3, 1, 32, M.ACT_SILU, 2, 16),       # 23 x 39 into channels 16..47 of a 48-channel buffer
        (64, 96, 3, 6, 2, 16, M.ACT_SILU, 2, None),     # 32 x 48 (YOLOv5 model.0)
        (62, 70, 2, 6, 3, 32, M.ACT_LEAKY, 2, None),    # 32 x 36: pad 3
        (75, 101, 3, 6, 2, 48, M.ACT_SILU, 3, None),    # 37 x 50
        (50, 200, 1, 6, 0, 64, M.ACT_RELU, 1, None),    # 23 x 98: pad 0
        (14, 30, 3, 6, 1, 80, M.ACT_SILU, 2, None),     # 6 x 14: pad 1, smaller than one tile
        (51, 80, 3, 7, 3, 64, M.ACT_RELU, 2, None),     # 26 x 40: the 7x7 stem without a pool behind it
        (29, 41, 2, 7, 1, 64, M.ACT_RELU, 3, 8)]        # 12 x 18, pad 1, into channels 8..71 of an 80-channel buffer


@pytest.mark.parametrize("case", STEM, ids=str)
def test_stem_x3_kernel(case, tmp_path):
    """conv_stem_x3_kernel<KH,NT,ACT>: the fp32 planes read once, split into hi / lo windows in LDS, KH K-steps of three MFMAs per tile
    pair; only the f32 tap follows the stem, so neither the pool nor the second conv joins the launch."""
    H, W, cin, k, pad, cout, act, batch, coff = case
    path = str(tmp_path / "stem.hipm")
    Wt = stem_graph(path, H, W, cin, k, 2, pad, cout, act, False, coff=coff)
    xin = np.random.default_rng(5).uniform(-1, 1, (batch, cin, H, W)).astype(np.float32)
    got, names = run_engine(path, batch, xin, "stem", ("stem",))
    want = stem_reference(xin, Wt, 2, pad, act, False)
    rel, mx = _errors(got, want)
    print("x3 stem %s conv %dx%d: rel %.2e (bound %.0e)  max|diff| %.2e (bound %.0e)  %s"
          % (case, want.shape[2], want.shape[3], rel, X3_REL, mx, X3_MAX, names["stem"]))
    assert names["stem"] == "conv_stem_x3_kernel<%d,%d,%s>" % (k, (cout + 15) // 16, ACT_NAME[act]), names
    assert got.shape == want.shape, (got.shape, want.shape)
    assert rel < X3_REL and mx < X3_MAX, (case, rel, mx)


#                    H   W  cin  k  s  pad cout act
OUTSIDE_THE_GATES = [(40, 56, 4, 3, 2, 1, 32, M.ACT_SILU),     # four input channels
                     (40, 56, 3, 3, 1, 1, 32, M.ACT_SILU),     # stride 1
                     (48, 80, 3, 7, 2, 3, 64, M.ACT_SILU)]     # a 7x7 stem with SiLU


@pytest.mark.parametrize("case", OUTSIDE_THE_GATES, ids=str)
def test_first_convs_outside_the_stem_gates(case, tmp_path):
    """First convs stem_x3_applicable refuses: the input conversion and the generic split-precision conv run them, to the same bound."""
    H, W, cin, k, s, pad, cout, act = case
    path = str(tmp_path / "nostem.hipm")
    Wt = stem_graph(path, H, W, cin, k, s, pad, cout, act, False)
    batch = 2
    xin = np.random.default_rng(6).uniform(-1, 1, (batch, cin, H, W)).astype(np.float32)
    got, names = run_engine(path, batch, xin, "stem", ("input", "stem"))
    want = stem_reference(xin, Wt, s, pad, act, False)
    rel, mx = _errors(got, want)
    print("x3 first conv outside the stem gates %s: rel %.2e (bound %.0e)  max|diff| %.2e (bound %.0e)  %s"
          % (case, rel, X3_REL, mx, X3_MAX, names))
    assert names["input"] == "input_nchw_kernel" and "x3" in names["stem"] and "stem" not in names["stem"], names
    assert got.shape == want.shape, (got.shape, want.shape)
    assert rel < X3_REL and mx < X3_MAX, (case, rel, mx)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_REL = {"fp32": 2e-6, "fp16x3": 2e-6, "fp16": 1e-3, "bf16": 8e-3}


def layernorm_graph(path, h, w, rng):
    """NCHW fp32 input -> f32 1x1 conv to 8 channels (bias ~100) -> OP_LAYERNORM over its flat h*w*8 (models.py's cls.0 call) -> f32
    linear tap.  Returns gamma and beta."""
    L = h * w * 8
    g = M.Graph("lnunit", 3, h, w, M.SynthWeights(2, gain=1.0))
    x, c3 = g.input()
    a = g.conv(x, 8, 1, 1, "pre", act=M.ACT_NONE, true_cin=c3, f32_out=True,
               weight=rng.standard_normal((8, 3, 1, 1)) * 0.6, bias_arr=100.0 + 0.5 * rng.standard_normal(8))
    gamma = (1.0 + 0.2 * rng.standard_normal(L)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(L)).astype(np.float32)
    ln = g.buf(1, 1, L)
    g._op(M.OP_LAYERNORM, [a], ln, w=g._blob(gamma), b=g._blob(beta), params=[1e-5], name="ln")
    z = g.conv(ln, 8, 1, 1, "tap", act=M.ACT_NONE, f32_out=True, wkind="linear")
    g.output(z, 0, [1, 8], "o")
    g.save(path)
    return gamma, beta


#                             h   w    length h * w * 8
@pytest.mark.parametrize("hw", [(2, 3),      # 48: fewer elements than threads
                                (5, 7),      # 280: a ragged last pass
                                (10, 50),    # 4,000: UFLDv2 CULane's cls.0
                                (16, 68)],   # 8,704: above 8,192 (the fp32 mode's generic conv, which runs the tap, takes K <= 9,216)
                         ids=lambda s: "len%d" % (s[0] * s[1] * 8))
@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "fp16", "bf16"])
def test_layernorm_kernel(hw, prec, tmp_path):
    """OP_LAYERNORM over the flat h*w*c of an fp32 tensor (UFLDv2's cls.0, models.py) with eps 1e-5 and non-trivial gamma / beta, on
    rows centred near 100 with a spread of about 1 (the offset comes from the 1x1 conv's bias), against float64 on the device's own
    LayerNorm input.  The offset is the hard part: a mean or a variance formed relative to zero (an fp32 mean of ~100, or E[x^2] -
    E[x]^2) loses the digits that the spread lives in."""
    h, w = hw
    L, batch = h * w * 8, 3
    rng = np.random.default_rng(11)
    path = str(tmp_path / "ln.hipm")
    gamma, beta = layernorm_graph(path, h, w, rng)
    e = CE.HipEngine(path, prec, batch)
    try:
        xin = rng.uniform(-1, 1, (batch, 3, h, w)).astype(np.float32)
        e.engine_inference(xin)
        pre = e.fetch_activation("pre", batch)               # NCHW of the f32 conv: the LayerNorm reads it as flat NHWC
        got = e.fetch_activation("ln", batch).reshape(batch, L)
        kn = e.layer_kernel(e.layer_index("ln"), batch)
    finally:
        e.close()
    t = pre.astype(np.float64).transpose(0, 2, 3, 1).reshape(batch, L)
    mean = t.mean(axis=1, keepdims=True)
    var = ((t - mean) ** 2).mean(axis=1, keepdims=True)
    want = (t - mean) / np.sqrt(var + 1e-5) * gamma.astype(np.float64) + beta.astype(np.float64)
    rel, mx = _errors(got, want)
    print("layernorm %-6s len %5d: input mean %.2f std %.2f  rel %.2e (bound %.0e)  max|diff| %.2e  %s"
          % (prec, L, float(mean.mean()), float(np.sqrt(var).mean()), rel, LN_REL[prec], mx, kn))
    assert kn == "layernorm_kernel", kn
    assert 95.0 < float(mean.mean()) < 105.0 and 0.3 < float(np.sqrt(var).mean()) < 3.0
    assert rel <= LN_REL[prec], (prec, L, rel, mx)
