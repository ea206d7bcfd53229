"""CPU: which body of conv_h8x3_kernel a layer runs (csrc/conv_halo8_x3.hip, include/adas_hip.h adas_debug_h8x3_onepass), on layer
descriptions alone -- no device.  The one-pass body takes the H8X3 launches whose tile plan keeps every window within 384 pixels (three
128-pixel pieces per wave in the two-pass count); ADAS_H8X_ONEPASS=0 sends everything back to the two-pass body; a layer that is not on
the H8X3 route has no body to choose.  The switch is read once per process, so its test asks a child process."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import pytest

from conftest import load_pkg
from test_conv_route_cpu import F16, MIN1, ROWS, X3, layer, route

load_pkg()
L = importlib.import_module("adas_amd._lib")

RAG1 = (13, 37)
H8X3 = "conv_h8x3_kernel<SILU>"
WIDE = ((40, 40), 16), ((12, 300), 8)      # (map, batch): plans whose 256-pixel tiles need windows of more than 384 pixels (found with the export)


def onepass(desc, batch):
    return L.lib().adas_debug_h8x3_onepass(C.byref(desc), batch)


@pytest.mark.parametrize("hw,batch", [(MIN1, 46), (RAG1, 46)], ids=["16x32", "13x37"])
def test_small_windows_run_the_one_pass_body(hw, batch):
    d = layer(hw, 64, 64)
    assert route(d, batch, X3) == H8X3
    assert onepass(d, batch) == 1


@pytest.mark.parametrize("hw,batch", WIDE, ids=["40x40", "12x300"])
def test_a_wide_window_stays_on_the_two_pass_body(hw, batch):
    d = layer(hw, 64, 64)
    assert route(d, batch, X3) == H8X3
    assert onepass(d, batch) == 0


@pytest.mark.parametrize("row", [r for r in ROWS if r[3] == X3], ids=lambda r: r[0])
def test_only_the_h8x3_route_has_a_one_pass_body(row):
    _, desc, batch, _, label = row
    if not label.startswith("conv_h8x3_kernel"):
        assert onepass(desc, batch) == 0
    else:
        assert onepass(desc, batch) in (0, 1)


def test_other_routes_of_the_same_layer():
    d = layer(MIN1, 64, 64)
    assert onepass(d, 46) == 1
    assert not route(d, 3, X3).startswith("conv_h8x3_kernel") and onepass(d, 3) == 0       # too few items for the persistent kernel
    d = layer(MIN1, 64, 256, res=(264, 4))                                                      # a residual view it cannot read 16 bytes at a time
    assert not route(d, 9, X3).startswith("conv_h8x3_kernel") and onepass(d, 9) == 0
    assert not route(layer(MIN1, 64, 64), 512, F16).startswith("conv_h8x3_kernel")          # (the predicate speaks of the split precision only)


def test_bad_arguments():
    assert onepass(layer(MIN1, 64, 64), 0) == -1
    assert L.lib().adas_debug_h8x3_onepass(None, 4) == -1


def test_the_switch_turns_it_off():
    code = ("import ctypes as C, importlib, sys\n"
            "sys.path[:0] = %r\n"
            "from test_conv_route_cpu import layer, route, X3\n"
            "L = importlib.import_module('adas_amd._lib')\n"
            "for hw in ((16, 32), (13, 37)):\n"
            "    d = layer(hw, 64, 64)\n"
            "    print(route(d, 46, X3), L.lib().adas_debug_h8x3_onepass(C.byref(d), 46))\n" % ([os.path.dirname(os.path.abspath(__file__))],))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ADAS_H8X_ONEPASS="0"), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split() == [H8X3, "0", H8X3, "0"]
