"""CPU: tools/make_font_atlas.py's PIL branch writes an atlas the overlay's rules accept (the cv2 branch cannot run here: no cv2)."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def system_ttf():
    for pat in ("/usr/share/fonts/**/*.ttf", "/usr/local/share/fonts/**/*.ttf", os.path.expanduser("~/.fonts/**/*.ttf")):
        hits = sorted(glob.glob(pat, recursive=True))
        if hits:
            return hits[0]
    try:
        import matplotlib
        hits = sorted(glob.glob(os.path.join(os.path.dirname(matplotlib.__file__), "mpl-data", "fonts", "ttf", "DejaVuSans.ttf")))
        return hits[0] if hits else None
    except ImportError:
        return None


def test_pil_branch_writes_a_valid_atlas(tmp_path):
    pytest.importorskip("PIL")
    ttf = system_ttf()
    if ttf is None:
        pytest.skip("no TTF on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_font_atlas
    finally:
        sys.path.pop(0)
    out = str(tmp_path / "font.npz")
    make_font_atlas.main(["--ttf", ttf, "--px", "18", "--scale", "0.7", out])
    f = dict(np.load(out))
    a = f["atlas"]
    assert a.dtype == np.uint8 and a.ndim == 2 and 1 <= a.shape[0] <= 64
    for k in ("glyph_x", "glyph_w", "bearing_x", "advance"):
        assert f[k].shape == (95,)
    assert (f["glyph_w"] >= 0).all() and (f["glyph_w"] <= 64).all() and (f["glyph_x"] >= 0).all() and (f["glyph_x"] + f["glyph_w"] <= a.shape[1]).all()
    assert f["glyph_w"][0] == 0 and f["advance"][0] > 0             # the space draws nothing and moves the pen
    assert f["glyph_w"][ord("A") - 32] > 0 and a.max() == 255 and ((a > 0) & (a < 255)).any()      # anti-aliased coverage
    assert 0 < int(f["baseline_row"]) <= a.shape[0] and float(f["scale"]) == 0.7
    import text_ref as R          # and the rules take it: a string has the size of its advances and paints inside its box
    font = {k: (v if v.ndim else v.item()) for k, v in f.items()}
    w, h = R.text_size(font, "12.34 m")
    assert w > 0 and h == int(f["size_h"])
    img = np.zeros((40, 120, 3), np.uint8)
    items, _ = R.layout(dict(lines=[(3, 25, 0, (255, 255, 255), "12.34 m")]), {0: font}, 120, 40, R.LINES)
    R.paint(img, items, {0: font})
    x0, y0, x1, y1 = items[0]["box"]
    assert img[y0:y1, x0:x1].any() and not img[:, x1:].any() and not img[:y0].any()
