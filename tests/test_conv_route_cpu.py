"""CPU: which kernel a convolution launches on (csrc/conv_kernels.hip, include/adas_hip.h adas_debug_conv_route) on layer descriptions
alone -- no device, no tensor.  One table of (layer, batch, precision) -> the label adas_engine_layer_kernel gives that layer in an engine
whose max_batch is the batch, with at least one row on each side of every decision of the order of choice:

  16-bit 3x3:  a narrow packing -> conv_halo;  else conv_halo_rw, conv_s2p, conv_h8, conv_halo (first that applies)
  16-bit 1x1:  conv_pw (Cin <= 512, no residual), else conv_pwg (Cin >= 128), else conv_igemm;  fp32: conv_igemm
  fp16x3:      fc_x3 / conv_pwx3 by the plan, else conv_h8x3, conv_s2d_x3 | conv_s2p_x3, else the generic kernel (conv_x3.hip)

The expected labels were recorded from the per-place ladders this table replaced as the statement of that order; where a GPU test states
the same boundary (tests/test_gpu_conv_exact.py, tests/test_gpu_x3_families.py) the row carries that test's expectation.  The two
"rw-res" rows were written from what the launch does: conv_halo_rw refuses a residual view that is not 16-byte aligned."""
import ctypes as C
import importlib

import pytest

from conftest import load_pkg

load_pkg()
L = importlib.import_module("adas_amd._lib")
M = importlib.import_module("adas_amd.models")

HALO, PW = 1, 4          # CONV_HALO, CONV_PW (csrc/kernels.h): a 3x3 pad 1 and a 1x1 pad 0 description
NONE_, SILU, RELU, LEAKY = M.ACT_NONE, M.ACT_SILU, M.ACT_RELU, M.ACT_LEAKY
F16, BF16, F32, X3 = L.PREC_FP16, L.PREC_BF16, L.PREC_FP32, L.PREC_FP16X3


def layer(hw, cin, cout, k=3, s=1, act=SILU, res=None, halo_bn=0):
    """A k x k conv (k = 3: pad 1; k = 1: pad 0) on an hw map, each tensor a whole buffer.  res = (pixel stride, channel offset) of the buffer
    the residual is a slice of (added after the activation)."""
    h, w = hw
    ho, wo = ((h - 1) // s + 1, (w - 1) // s + 1)      # the same for 3x3 pad 1 and 1x1 pad 0
    x = L.MlView(0x100000, cin, 0, cin, h, w)
    y = L.MlView(0x200000, cout, 0, cout, ho, wo)
    r = L.MlView(0x300000, res[0], res[1], cout, ho, wo) if res else L.MlView()
    return L.MlLayerDesc(HALO if k == 3 else PW, s, act, M.RES_AFTER_ACT if res else M.RES_NONE, 0, halo_bn, x, y, r, L.MlView())


def route(desc, batch, prec):
    name = C.create_string_buffer(96)
    L.check(L.lib().adas_debug_conv_route(C.byref(desc), batch, prec, name, 96))
    return name.value.decode()


MIN1, MIN2 = (16, 32), (16, 64)     # two 256-pixel tiles a frame at stride 1; one 8 x 32 output tile a frame at stride 2
BIG = (640, 640)

# (id, layer, batch, precision, label)
ROWS = [
    # ---- conv_halo_rw: 3x3 s1, 16 <= Cin <= 64, Cout > 16 and not in 65..96, tiles * channel blocks >= 1024 (16 x 32: two tiles a frame)
    ("rw-511", layer(MIN1, 64, 64), 511, F16, "conv_halo_kernel<64,SILU,s1>"),
    ("rw-512", layer(MIN1, 64, 64), 512, F16, "conv_halo_rw_kernel<2,SILU>"),
    ("rw-bn32", layer(MIN1, 32, 32, act=RELU), 512, BF16, "conv_halo_rw_kernel<1,RELU,bn32>"),
    ("rw-cin96", layer(MIN1, 96, 64), 512, F16, "conv_halo_kernel<64,SILU,s1>"),
    ("rw-cout80", layer(MIN1, 64, 80), 512, F16, "conv_halo_kernel<48,SILU,s1>"),
    ("rw-cout16", layer(MIN1, 64, 16), 512, F16, "conv_halo_kernel<16,SILU,s1>"),
    # ---- conv_s2p: 3x3 s2, Cin >= 128, Cout % 128 == 0, no residual, tiles * (Cout / 128) >= 512 (16 x 64 -> 8 x 32: one tile a frame)
    ("s2p-255", layer(MIN2, 128, 256, s=2, act=RELU), 255, F16, "conv_halo_kernel<64,RELU,s2>"),
    ("s2p-256", layer(MIN2, 128, 256, s=2, act=RELU), 256, F16, "conv_s2p_kernel<RELU>"),
    ("s2p-cin64", layer(MIN2, 64, 256, s=2), 256, F16, "conv_halo_kernel<64,SILU,s2>"),
    ("s2p-res", layer(MIN2, 128, 256, s=2, res=(256, 0)), 256, F16, "conv_halo_kernel<64,SILU,s2>"),
    # ---- conv_h8: 3x3 s1, Cin >= 64 and a multiple of 32, Cout % 128 == 0, the units fill whole rounds of 32 slots an XCD
    ("h8-128", layer(MIN1, 128, 128, act=RELU), 128, F16, "conv_h8_kernel<RELU>"),
    ("h8-res", layer(MIN1, 128, 128, act=LEAKY, res=(128, 0)), 128, BF16, "conv_h8_kernel<LEAKY>"),
    ("h8-few", layer(MIN1, 128, 128), 3, F16, "conv_halo_kernel<64,SILU,s1,bm128>"),                      # 6 tiles: under one unit a slot (h8_blocks_per_unit = 0)
    ("h8-res-coff4", layer(MIN1, 128, 128, res=(136, 4)), 128, F16, "conv_halo_kernel<64,SILU,s1>"),  # conv_h8 reads its residual 16 bytes at a time
    ("h8-cin96", layer(MIN1, 96, 128), 128, F16, "conv_h8_kernel<SILU>"),
    ("h8-cin48", layer(MIN1, 48, 128), 128, F16, "conv_halo_kernel<64,SILU,s1>"),                   # (512 items: under conv_halo_rw's 1024 too)
    ("h8-cout64", layer(MIN1, 128, 64), 128, F16, "conv_halo_kernel<64,SILU,s1,bm128>"),
    # ---- conv_halo: what is left; 128-pixel tiles under 320 workgroups of 256-pixel tiles (stride 1), its stride-2 form, a narrow packing
    ("halo-159", layer(MIN1, 96, 64, act=NONE_), 159, F16, "conv_halo_kernel<64,NONE,s1,bm128>"),
    ("halo-160", layer(MIN1, 96, 64, act=NONE_), 160, F16, "conv_halo_kernel<64,NONE,s1>"),
    ("halo-s2", layer(MIN2, 96, 64, s=2, act=LEAKY), 128, F16, "conv_halo_kernel<64,LEAKY,s2>"),
    ("halo-bn48", layer(MIN1, 96, 80, act=LEAKY), 32, BF16, "conv_halo_kernel<48,LEAKY,s1,bm128>"),
    ("halo-narrow", layer(MIN1, 64, 64, halo_bn=16), 3, F16, "conv_halo_kernel<16,SILU,s1,bm128>"),
    ("halo-narrow-rw", layer(MIN1, 64, 64, halo_bn=16), 512, F16, "conv_halo_kernel<16,SILU,s1>"),    # conv_halo_rw would take the default packing here (rw-512)
    ("halo-narrow-h8", layer(MIN1, 128, 128, halo_bn=32), 128, F16, "conv_halo_kernel<32,SILU,s1>"),  # ... and conv_h8 this one (h8-128)
    # ---- 1x1: conv_pw up to 512 input channels without a residual, conv_pwg from 128 channels, conv_igemm for the rest
    ("pw-256", layer((12, 20), 256, 64, k=1), 3, F16, "conv_pw_kernel<8>"),
    ("pw-512", layer((12, 20), 512, 256, k=1), 3, BF16, "conv_pw_kernel<16>"),
    ("pw-s2", layer((12, 20), 128, 64, k=1, s=2), 3, F16, "conv_pw_kernel<4>"),
    ("pwg64", layer((12, 20), 544, 64, k=1), 3, F16, "conv_pwg_kernel<64>"),
    ("pwg128", layer((12, 20), 544, 512, k=1, act=RELU), 70, F16, "conv_pwg_kernel<128>"),
    ("pwg-res", layer((12, 20), 544, 64, k=1, res=(64, 0)), 3, F16, "conv_pwg_kernel<64>"),
    ("pwg-res-128", layer((11, 13), 128, 128, k=1, res=(128, 0)), 3, F16, "conv_pwg_kernel<64>"),
    ("igemm-res-cin40", layer((11, 13), 40, 40, k=1, res=(40, 0)), 3, F16, "conv_igemm_kernel<f16,f16,64,64>"),      # a residual keeps it off conv_pw, 40 channels off conv_pwg
    ("igemm-res-coff2", layer((12, 20), 544, 64, k=1, res=(72, 2)), 3, BF16, "conv_igemm_kernel<bf16,bf16,64,64>"),    # conv_pwg reads its residual 8 bytes at a time
    ("igemm-3x3-cin8", layer((12, 20), 8, 64), 3, F16, "conv_igemm_kernel<f16,f16,64,64>"),                          # conv_halo starts at 16 input channels
    ("igemm-fp32", layer(MIN1, 64, 64), 512, F32, "conv_igemm_kernel<f32,f32,128,64>"),                               # fp32 mode: no halo kernels
    ("igemm-fp32-1x1", layer((12, 20), 544, 64, k=1), 3, F32, "conv_igemm_kernel<f32,f32,64,64>"),
    # ---- fp16x3: the plan's streaming kernels
    ("x3-pw", layer((12, 20), 256, 64, k=1), 3, X3, "conv_pwx3_kernel<8>"),
    ("x3-fc", layer((1, 1), 256, 264, k=1, act=RELU), 17, X3, "fc_x3_kernel"),
    ("fc", layer((1, 1), 256, 264, k=1, act=RELU), 17, F16, "fc_kernel"),
    # ---- fp16x3 fill: 64 -> 64 on 16 x 16 is one tile a frame, units = ceil(batch / 8) (test_gpu_x3_families.py, H8_FILL_CASES)
    ("x3-fill-88", layer((16, 16), 64, 64), 88, X3, "conv_x3_igemm_kernel<64,64>"),
    ("x3-fill-89", layer((16, 16), 64, 64), 89, X3, "conv_h8x3_kernel<SILU>"),
    ("x3-fill-248", layer((16, 16), 64, 64), 248, X3, "conv_h8x3_kernel<SILU>"),
    ("x3-fill-304", layer((16, 16), 64, 64), 304, X3, "conv_x3_igemm_kernel<128,64>"),
    ("x3-fill-305", layer((16, 16), 64, 64), 305, X3, "conv_h8x3_kernel<SILU>"),
    ("x3-h8-res", layer(MIN1, 64, 256, act=RELU, res=(256, 0)), 9, X3, "conv_h8x3_kernel<RELU>"),
    ("x3-h8-res-coff4", layer(MIN1, 64, 256, act=RELU, res=(264, 4)), 9, X3, "conv_x3_igemm_kernel<64,64>"),
    # ---- fp16x3 32-bit offsets at 640 x 640 (test_h8x3_at_its_offset_limit, test_s2d_x3_at_its_offset_limit)
    ("x3-h8-38", layer(BIG, 64, 64), 38, X3, "conv_h8x3_kernel<SILU>"),
    ("x3-h8-39", layer(BIG, 64, 64), 39, X3, "conv_x3_igemm_kernel<128,64>"),
    ("x3-s2d-35", layer(BIG, 32, 64, s=2), 35, X3, "conv_s2d_x3_kernel<SILU>"),
    ("x3-s2d-36", layer(BIG, 32, 64, s=2), 36, X3, "conv_s2p_x3_kernel<SILU>"),
    # ---- fp16x3 stride 2: 96 items (test_stride2_kernel_item_floor), more than 32 blocks of 64 output channels, a residual
    ("x3-s2-95", layer((32, 32), 32, 64, s=2), 95, X3, "conv_x3_igemm_kernel<64,64>"),
    ("x3-s2-96", layer((32, 32), 32, 64, s=2), 96, X3, "conv_s2d_x3_kernel<SILU>"),
    ("x3-s2p-33blocks", layer(MIN2, 32, 2112, s=2, act=LEAKY), 3, X3, "conv_s2p_x3_kernel<LEAKY>"),
    ("x3-s2d-32blocks", layer(MIN2, 32, 2048, s=2, act=LEAKY), 3, X3, "conv_s2d_x3_kernel<LEAKY>"),
    ("x3-s2-res", layer(MIN2, 64, 128, s=2, res=(128, 0)), 48, X3, "conv_x3_igemm_kernel<64,64>"),
    ("x3-s2d", layer(MIN2, 64, 128, s=2, act=NONE_), 48, X3, "conv_s2d_x3_kernel<NONE>"),
    # ---- fp16x3, the generic kernel's own choice (conv_x3.hip) stays behind one route
    ("x3-ksplit", layer((12, 20), 64, 64), 3, X3, "conv_x3_ksplit_kernel"),
    ("x3-igemm-cin8", layer((12, 20), 8, 64), 3, X3, "conv_x3_igemm_kernel<32,32>"),
]

# conv_halo_rw refuses a residual view whose pixel stride or channel offset is no multiple of 8 when it launches and conv_h8 refuses the
# same view, so the layer runs on conv_halo; with an aligned view it is conv_halo_rw's.  Written from what the launch does.
ROWS += [
    ("rw-res-coff4", layer(MIN1, 64, 128, res=(136, 4)), 256, F16, "conv_halo_kernel<64,SILU,s1>"),
    ("rw-res-coff8", layer(MIN1, 64, 128, res=(136, 8)), 256, F16, "conv_halo_rw_kernel<2,SILU>"),
]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r[0])
def test_conv_route(row):
    _, desc, batch, prec, want = row
    assert route(desc, batch, prec) == want


def test_bad_arguments_are_refused():
    d = layer(MIN1, 64, 64)
    name = C.create_string_buffer(96)
    assert L.lib().adas_debug_conv_route(C.byref(d), 0, F16, name, 96) != 0
    assert L.lib().adas_debug_conv_route(C.byref(d), 4, 7, name, 96) != 0
    assert L.lib().adas_debug_conv_route(C.byref(d), 4, F16, None, 96) != 0
