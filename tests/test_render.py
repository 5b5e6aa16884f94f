"""Display images (include/dspn_render.h, dspnet_amd/detect/render.py): what can be checked without a GPU -- the colour
table against the reference's, the index tables, the host arithmetic of the draw rows, and the argument checks of the C
entries (every call below fails its checks, or is an empty job, before any HIP call)."""
import ctypes
import json
import os

import numpy as np
import pytest

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from dspnet_amd.detect import render as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASSES = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]


def test_palette_and_names_equal_the_reference_table():
    with open(os.path.join(GOLDEN, "cityscapes_palette.json")) as f:
        labels = json.load(f)["labels"]
    assert [l["trainId"] for l in labels] == list(range(20))
    assert list(R.SEG_NAMES) == [l["name"] for l in labels]
    assert [list(c) for c in R.PALETTE] == [l["color"] for l in labels]
    table = R.palette_table()
    assert table.shape == (256, 3) and table.dtype == np.uint8 and not table[20:].any()
    np.testing.assert_array_equal(table[:20], np.array(R.PALETTE, np.uint8))
    assert R.DET2SEG == {i: 11 + i for i in range(8)}
    assert [R.SEG_NAMES[R.DET2SEG[i]] for i in range(8)] == CLASSES
    assert R.SHORT_CLASS_NAME["motorcycle"] == "mbike" and R.SHORT_CLASS_NAME["traffic light"] == "tlight"


def test_font_table():
    assert len(R.FONT) == 95 * 7 == fn.RENDER_FONT_BYTES
    assert not any(R.FONT[:7]) and all(b < 32 for b in R.FONT)
    glyph = lambda ch: list(R.FONT[(ord(ch) - 32) * 7:(ord(ch) - 31) * 7])  # noqa: E731
    assert glyph("T") == [0x1f, 4, 4, 4, 4, 4, 4] and glyph("-") == [0, 0, 0, 0x1f, 0, 0, 0]
    assert len({bytes(glyph(chr(c))) for c in range(32, 127)}) == 95       # no two characters share a pattern


def test_nearest_tables():
    ys, xs = R.nearest_tables(8, 16, 32, 64)                               # exactly 4: dst >> 2
    assert ys.dtype == np.int32 and xs.dtype == np.int32
    np.testing.assert_array_equal(ys, np.arange(32) >> 2)
    np.testing.assert_array_equal(xs, np.arange(64) >> 2)
    ys, xs = R.nearest_tables(5, 7, 13, 17)
    np.testing.assert_array_equal(ys, [0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4])         # floor(y * 5 / 13)
    np.testing.assert_array_equal(xs, [int(np.floor(x * (1.0 / (17 / 7.0)))) for x in range(17)])
    assert xs[0] == 0 and xs[-1] == 6 and (np.diff(xs) >= 0).all()
    ys, _ = R.nearest_tables(9, 9, 4, 4)                                   # a downscale: floor(y * 2.25)
    np.testing.assert_array_equal(ys, [0, 2, 4, 6])
    for Ns, Nd in [(3, 1000), (7, 7), (300, 1200), (1, 5), (6, 11), (97, 389)]:
        t, _ = R.nearest_tables(Ns, Ns, Nd, Nd)
        assert t.min() == 0 and t.max() <= Ns - 1 and len(t) == Nd
    np.testing.assert_array_equal(R.nearest_tables(6, 6, 6, 6)[0], np.arange(6))


def _det(cls, score, x0, y0, x1, y1, dist):
    return [cls, score, x0, y0, x1, y1, dist]


def test_detection_rows_demo_order_threshold_and_truncation():
    dets = np.array([_det(2, 0.9, 0.1, 0.2, 0.3, 0.4, 0.1),                # near
                     _det(0, 0.7, 0.4995, 0.5, 0.75, 0.875, 0.5),          # in between
                     _det(1, 0.6, 0.0, 0.0, 0.5, 0.5, 0.75),               # farthest: painted first; score == thresh as float32 (> 0.6 in double): kept
                     _det(3, 0.5, 0.0, 0.0, 0.5, 0.5, 0.95),               # under the threshold
                     _det(-1, 0.99, 0.0, 0.0, 0.5, 0.5, 0.99)], np.float32)
    rows = R.detection_rows(dets, 1000, 1000, CLASSES, 0.6, "demo")
    boxes = [r for r in rows if r[0] == fn.DRAW_OUTLINE]
    assert [tuple(r[5:8]) for r in boxes] == [R.PALETTE[12], R.PALETTE[11], R.PALETTE[13]]      # by distance, descending
    assert boxes[1][1:5] == (499, 500, 750, 875)                           # 0.4995f * 1000 = 499.50000644: truncated
    assert all(r[8] == 2 for r in boxes)
    # every box is followed by its tag and its text, before the next box
    kinds = [r[0] for r in rows]
    text = "person 128m"                                                   # '%.0f' of 0.5 * 255 = 127.5: half to even
    first = kinds.index(fn.DRAW_OUTLINE, 1)
    assert kinds[:first] == [0, 1] + [2] * len("rider 191m")                        # 0.75 * 255 = 191.25
    s = R.text_scale(1000)
    assert s == 2
    tag = rows[first + 1]
    assert tag[:5] == (fn.DRAW_FILL, 499, 500 - 8 * s, 499 + len(text) * 6 * s - 1, 499) and tag[5:8] == (0, 0, 128)
    glyphs = rows[first + 2:first + 2 + len(text)]
    assert "".join(chr(g[8] & 255) for g in glyphs) == text and all(g[8] >> 8 == s and g[5:8] == (255, 255, 255) for g in glyphs)
    assert [g[1] for g in glyphs] == [499 + i * 6 * s for i in range(len(text))] and all(g[2] == 500 - 7 * s for g in glyphs)
    assert R.detection_rows(np.zeros((0, 7), np.float32), 512, 512, CLASSES) == []


def test_detection_rows_eval_rounds_half_away_in_table_order():
    dets = np.array([_det(2, 0.2, 0.4995, 0.0625, 0.75, 0.9, 0.1), _det(0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)], np.float32)
    rows = R.detection_rows(dets, 1000, 1000, CLASSES, mode="eval")
    boxes = [r for r in rows if r[0] == fn.DRAW_OUTLINE]
    assert [b[1:5] for b in boxes] == [(500, 63, 750, 900), (100, 200, 300, 400)]      # 499.5000064 -> 500; 62.5 -> 63, not 62
    assert all(b[5:8] == (128, 0, 0) and b[8] == 1 for b in boxes)                     # no threshold, thickness 1
    text = [chr(r[8] & 255) for r in rows if r[0] == fn.DRAW_GLYPH]
    assert "".join(text) == "car:26m" + "person:128m"                                  # 25.5 -> 26 and 127.5 -> 128: half to even
    assert R._round_half_away(-2.5) == -3 and R._round_half_away(2.5) == 3 and R._round_half_away(2.4999) == 2


def test_thickness_switches_above_320_rows():
    d = np.array([_det(0, 0.9, 0.1, 0.1, 0.5, 0.5, 0.2)], np.float32)
    assert R.detection_rows(d, 320, 640, CLASSES)[0][8] == 1
    assert R.detection_rows(d, 321, 640, CLASSES)[0][8] == 2
    assert R.text_scale(320) == 1 and R.text_scale(767) == 1 and R.text_scale(768) == 2 and R.text_scale(1024) == 2


def test_ground_truth_boxes_under_100_square_pixels_are_skipped():
    gts = np.array([[1, 0.1, 0.1, 0.2, 0.2, 0.3],           # 10 x 10 = 100 px^2: drawn
                    [2, 0.1, 0.1, 0.19, 0.2, 0.3],          # 9 x 10: skipped
                    [-1, -1, -1, -1, -1, -1]], np.float32)  # a padding row: no area
    rows = R.detection_rows(gts, 100, 100, CLASSES, mode="eval")
    boxes = [r for r in rows if r[0] == fn.DRAW_OUTLINE]
    assert [b[1:5] for b in boxes] == [(10, 10, 20, 20)] and boxes[0][5:8] == (128, 0, 0)
    assert "".join(chr(r[8] & 255) for r in rows if r[0] == fn.DRAW_GLYPH) == "rider:77m"          # 0.3f * 255 = 76.5000030
    with pytest.raises(_lib.DspnError):
        R.detection_rows(gts, 100, 100, CLASSES, mode="demo")
    with pytest.raises(_lib.DspnError):
        R.detection_rows(gts, 100, 100, CLASSES, mode="other")


def test_text_and_legend_geometry():
    rows = R.text_rows("Ab", 10, 40, 3, (1, 2, 3))
    assert rows == [(fn.DRAW_GLYPH, 10, 40 - 21, 0, 0, 1, 2, 3, (3 << 8) | ord("A")),
                    (fn.DRAW_GLYPH, 28, 40 - 21, 0, 0, 1, 2, 3, (3 << 8) | ord("b"))]
    assert R.text_rows("", 0, 0, 1, (0, 0, 0)) == [] and R.tag_rows("", 0, 0, 1) == []
    assert R.text_rows("é中", 0, 8, 1, (0, 0, 0))[1][8] == (1 << 8) | 255       # beyond the table: the block
    legend = R.legend_rows(2048)
    squares = [r for r in legend if r[0] == fn.DRAW_FILL]
    assert len(squares) == 20
    for idx, sq in enumerate(squares):
        ax, ay = (idx * 100, 0) if idx < 10 else ((idx - 10) * 100, 15)
        assert sq[1:5] == (ax, ay, ax + 14, ay + 14) and sq[5:8] == R.PALETTE[idx]
    assert max(r[3] for r in squares) < 2048 and max(r[4] for r in squares) == 29       # inside the 30-row strip
    first_name = legend[1:1 + len("road")]
    assert [(g[1], g[2]) for g in first_name] == [(16 + 6 * i, 3) for i in range(4)] and first_name[0][8] == (1 << 8) | ord("r")
    assert len([r for r in legend if r[0] == fn.DRAW_GLYPH]) == sum(len(n) for n in R.SEG_NAMES)
    assert len([r for r in R.legend_rows(250) if r[0] == fn.DRAW_FILL]) == 6             # columns 0, 100, 200 of both lines


# ---------------------------------------------------------------------------------------------- C entries
P = ctypes.c_void_p(256)          # never dereferenced


def _classmap(scores=P, B=2, h=5, w=7, C=19, ld=20, pal=P, ys=P, xs=P, Hd=13, Wd=17, canvas=P, CH=37, CW=53, y0=3, x0=5):
    return _lib.lib().dspn_render_classmap_f32(scores, B, h, w, C, ld, pal, ys, xs, Hd, Wd, canvas, CH, CW, y0, x0, None)


def _labels(lab=P, B=2, h=5, w=7, pal=P, ys=P, xs=P, Hd=13, Wd=17, canvas=P, CH=37, CW=53, y0=3, x0=5):
    return _lib.lib().dspn_render_labels_f32(lab, B, h, w, pal, ys, xs, Hd, Wd, canvas, CH, CW, y0, x0, None)


def _data(data=P, B=2, H=13, W=17, cmap=(2, 1, 0), mean=(1.0, 2.0, 3.0), canvas=P, CH=37, CW=53, y0=3, x0=5):
    cm = None if cmap is None else (ctypes.c_int * 3)(*cmap)
    mn = None if mean is None else (ctypes.c_double * 3)(*mean)
    return _lib.lib().dspn_render_data_f32(data, B, H, W, cm, mn, canvas, CH, CW, y0, x0, None)


def _draw(canvas=P, B=3, CH=37, CW=53, y0=0, x0=0, Hd=37, Wd=53, rows=P, R_=4, start=P, font=P):
    return _lib.lib().dspn_render_draw_list_u8(canvas, B, CH, CW, y0, x0, Hd, Wd, rows, R_, start, font, None)


@pytest.mark.parametrize("call", [_classmap, _labels, _data, _draw])
def test_panel_checks_are_shared_by_the_four_entries(call):
    err = _lib.lib().dspn_last_error
    size = dict(H=-1) if call is _data else dict(Hd=-1)
    assert call(**size) == -1 and b"negative size" in err()
    assert call(B=-2) == -1 and b"negative size" in err()
    assert call(CH=0) == -1 and b"canvas height and width" in err()
    assert call(CW=-5) == -1 and b"canvas height and width" in err()
    assert call(y0=-1) == -1 and b"leaves the canvas" in err()
    assert call(x0=53 - 16) == -1 and b"leaves the canvas" in err()            # one column too far right
    assert call(y0=37 - 12) == -1 and b"leaves the canvas" in err()
    assert call(CH=1 << 15, CW=1 << 16) == -1 and b"2^31" in err()
    assert call(CH=1 << 14, CW=1 << 14, B=3) == -1 and b"2^31" in err()         # 3 * 2^28 * 3 bytes
    assert call(B=70000, CH=37, CW=53) == -1 and b"65535" in err()
    assert call(canvas=None) == -1 and b"null pointer" in err()
    # an empty job: nothing to do, no HIP call, null pointers are fine
    assert call(B=0, canvas=None) == 0
    if call is _data:
        assert call(H=0, y0=0, data=None) == 0 and call(W=0, canvas=None) == 0
    else:
        assert call(Hd=0, canvas=None) == 0 and call(Wd=0, canvas=None) == 0


def test_map_entries_reject_bad_sources():
    err = _lib.lib().dspn_last_error
    for call in (_classmap, _labels):
        assert call(h=0) == -1 and b"source height and width" in err()
        assert call(w=-3) == -1 and b"source height and width" in err()
        assert call(h=1 << 16, w=1 << 15) == -1 and b"2^31" in err()
        assert call(pal=None) == -1 and b"null pointer" in err()
        assert call(ys=None) == -1 and call(xs=None) == -1
    assert _classmap(scores=None) == -1 and _labels(lab=None) == -1
    assert _classmap(C=21, ld=20) == -1 and b"C > ld" in err()
    assert _classmap(C=0) == -1 and b"1..256" in err()
    assert _classmap(C=257, ld=260) == -1 and b"1..256" in err()
    assert _classmap(h=1 << 13, w=1 << 13, ld=32, C=19, B=1) == -1 and b"2^31" in err()        # h * w * ld
    assert _classmap(C=21, ld=20, B=0) == -1                                                  # checked even for an empty job


def test_data_entry_rejects_bad_maps():
    err = _lib.lib().dspn_last_error
    assert _data(cmap=(0, 1, 3)) == -1 and b"not a plane" in err()
    assert _data(cmap=(-1, 1, 2)) == -1 and b"not a plane" in err()
    assert _data(cmap=None) == -1 and _data(mean=None) == -1
    assert _data(mean=(0.0, float("nan"), 0.0)) == -1 and b"not a number" in err()
    assert _data(data=None) == -1 and b"null pointer" in err()
    assert _data(H=1 << 15, W=1 << 15, CH=1 << 15, CW=1 << 15, y0=0, x0=0, B=1) == -1 and b"2^31" in err()


def _host_rows(rows, starts):
    flat = np.array([tuple(r) for r in rows], fn.DRAW_ROW_FIELDS) if rows else np.zeros(1, fn.DRAW_ROW_FIELDS)
    start = np.array(starts, np.int32)
    return _lib.lib().dspn_render_check_draw_rows(flat.ctypes.data, len(rows), start.ctypes.data, len(starts) - 1), flat, start


def test_draw_entries_reject_bad_rows_and_tables():
    err = _lib.lib().dspn_last_error
    assert _draw(R_=-1) == -1 and b"R < 0" in err()
    assert _draw(rows=None) == -1 and _draw(start=None) == -1 and _draw(font=None) == -1 and b"null pointer" in err()
    assert _draw(R_=0, canvas=None, rows=None) == 0                                           # no rows: an empty job
    assert _draw(y0=30, Hd=8) == -1 and b"leaves the canvas" in err()
    ok = [(0, 1, 2, 3, 4, 255, 0, 0, 1), (1, 5, 5, 2, 2, 0, 0, 0, 0), (2, 0, 0, 0, 0, 1, 2, 3, (1 << 8) | 65)]
    assert _host_rows(ok, [0, 2, 2, 3])[0] == 0
    assert _host_rows([], [0, 0])[0] == 0 and _host_rows([], [0])[0] == 0
    assert _host_rows([(0, 1, 2, 3, 4, 255, 0, 0, 0)], [0, 1])[0] == -1 and b"t < 1" in err()
    assert _host_rows([(0, 1, 2, 3, 4, 255, 0, 0, -2)], [0, 1])[0] == -1 and b"t < 1" in err()
    assert _host_rows([(2, 0, 0, 0, 0, 1, 2, 3, 65)], [0, 1])[0] == -1 and b"scale < 1" in err()
    assert _host_rows([(3, 0, 0, 0, 0, 1, 2, 3, 1)], [0, 1])[0] == -1 and b"kind 3" in err()
    assert _host_rows([(1, 0, 0, 0, 0, 256, 2, 3, 0)], [0, 1])[0] == -1 and b"colour" in err()
    assert _host_rows([(1, 0, 0, 1 << 25, 0, 1, 2, 3, 0)], [0, 1])[0] == -1 and b"2^24" in err()
    assert _host_rows(ok, [0, 2, 1, 3])[0] == -1 and b"decreases" in err()
    assert _host_rows(ok, [0, 2, 2, 2])[0] == -1 and b"from 0 to R" in err()
    assert _host_rows(ok, [1, 2, 2, 3])[0] == -1
    lib = _lib.lib()
    assert lib.dspn_render_check_draw_rows(None, 1, P, 1) == -1 and lib.dspn_render_check_draw_rows(None, 0, None, 0) == -1
    assert lib.dspn_render_check_draw_rows(None, -1, None, 0) == -1 and b"negative" in err()
    with pytest.raises(_lib.DspnError, match="t < 1"):                                       # the packer checks before it uploads
        fn.draw_table([[(0, 1, 2, 3, 4, 255, 0, 0, 0)]], "cpu")


def test_chunk_constant_is_exported():
    import re
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dspn_render.h")).read()
    assert int(re.search(r"#define DSPN_RENDER_CHUNK_ROWS (\d+)", header).group(1)) == fn.render_chunk_rows() >= 16
    assert int(re.search(r"#define DSPN_RENDER_FONT_BYTES (\d+)", header).group(1)) == fn.RENDER_FONT_BYTES


def test_save_png_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import torch
    a = (np.arange(5 * 7 * 3) % 256).astype(np.uint8).reshape(5, 7, 3)
    R.save_png(str(tmp_path / "a.png"), torch.from_numpy(a))
    np.testing.assert_array_equal(np.asarray(Image.open(str(tmp_path / "a.png"))), a)
    R.save_png(str(tmp_path / "g.png"), a[:, :, 0])
    np.testing.assert_array_equal(np.asarray(Image.open(str(tmp_path / "g.png"))), a[:, :, 0])
    with pytest.raises(_lib.DspnError):
        R.save_png(str(tmp_path / "bad.png"), np.zeros((4, 4), np.float32))


def test_frame_warp_is_the_demo_resize_rule():
    from dspnet_amd.detect.multitask_detector import frame_warp
    # 1080p video: the long side caps the scale at 1024 / 1920 -> 576 x 1024, aspect 1.78 -> rows [64:576]: 512 x 1024
    M = frame_warp(1080, 1920, 512, 1024)
    s = 1024 / 1920.0
    np.testing.assert_allclose(M, [s, 0, 0, 0, s, -64.0], rtol=0, atol=1e-15)
    # a 2:1 frame is not cropped: 600 x 1200 would pass 1024 -> 512 x 1024
    np.testing.assert_allclose(frame_warp(1024, 2048, 512, 1024), [0.5, 0, 0, 0, 0.5, 0.0], rtol=0, atol=1e-15)
    # onto a net of another size: the cropped 512 x 1024 picture scaled to 256 x 512
    np.testing.assert_allclose(frame_warp(1080, 1920, 256, 512), [s / 2, 0, 0, 0, s / 2, -32.0], rtol=0, atol=1e-15)
    with pytest.raises(_lib.DspnError):
        frame_warp(100, 2000, 512, 1024)                     # 51 rows after the resize: nothing left below row 64
