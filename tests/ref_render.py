"""numpy restatement of the four kernels of include/dspn_render.h and of the two pictures built from them
(dspnet_amd/detect/render.py), for the GPU tests: fancy indexing for the panels, and for the draw list a plain walk of the
rows in table order, each row painting its pixel set over what is there.  Canvases are (B, CH, CW, 3) uint8 arrays
written in place."""
import numpy as np

from dspnet_amd.detect import render as R


def classmap(scores, C, palette, ysrc, xsrc, canvas, y0=0, x0=0):
    idx = np.argmax(scores[..., :C], axis=-1)                      # first maximum
    canvas[:, y0:y0 + len(ysrc), x0:x0 + len(xsrc)] = palette[idx[:, ysrc][:, :, xsrc]]


def labels(label, palette, ysrc, xsrc, canvas, y0=0, x0=0):
    idx = label.astype(np.uint8)
    canvas[:, y0:y0 + len(ysrc), x0:x0 + len(xsrc)] = palette[idx[:, ysrc][:, :, xsrc]]


def data(planes, channel_map, mean, canvas, y0=0, x0=0):
    B, _, H, W = planes.shape
    v = planes[:, list(channel_map)].astype(np.float64) + np.asarray(mean, np.float64).reshape(1, 3, 1, 1)
    v = np.clip(np.trunc(v), 0, 255).astype(np.uint8)
    canvas[:, y0:y0 + H, x0:x0 + W] = v.transpose(0, 2, 3, 1)


def _glyph_bits(font, code):
    if 32 <= code <= 126:
        return [font[(code - 32) * 7 + gy] for gy in range(7)]
    return [0x1f] * 7


def draw_row(panel, row, font):
    """one row onto panel (Hd, Wd, 3), a view of the canvas"""
    Hd, Wd = panel.shape[:2]
    kind, x0, y0, x1, y1, r, g, b, arg = [int(v) for v in row]
    colour = np.array([r, g, b], np.uint8)
    if kind in (0, 1):
        yy, xx = np.mgrid[0:Hd, 0:Wd]
        xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        if kind == 1:
            hit = (xx >= xa) & (xx <= xb) & (yy >= ya) & (yy <= yb)
        else:
            t = arg
            assert t >= 1
            o, i = t // 2, (t + 1) // 2
            outer = (xx >= xa - o) & (xx <= xb + o) & (yy >= ya - o) & (yy <= yb + o)
            inner = (xx >= xa + i) & (xx <= xb - i) & (yy >= ya + i) & (yy <= yb - i)
            hit = outer & ~inner
        panel[hit] = colour
    elif kind == 2:
        s, code = arg >> 8, arg & 0xff
        assert s >= 1
        for gy, bits in enumerate(_glyph_bits(font, code)):
            for gx in range(5):
                if (bits >> (4 - gx)) & 1:
                    for py in range(y0 + gy * s, y0 + (gy + 1) * s):
                        for px in range(x0 + gx * s, x0 + (gx + 1) * s):
                            if 0 <= py < Hd and 0 <= px < Wd:
                                panel[py, px] = colour
    else:
        raise AssertionError(kind)


def draw_list(canvas, rows_per_image, font, y0=0, x0=0, Hd=None, Wd=None):
    B, CH, CW = canvas.shape[:3]
    Hd, Wd = CH - y0 if Hd is None else Hd, CW - x0 if Wd is None else Wd
    assert len(rows_per_image) == B
    for b, rows in enumerate(rows_per_image):
        panel = canvas[b, y0:y0 + Hd, x0:x0 + Wd]
        for row in rows:                                           # table order: the last covering row wins
            draw_row(panel, row, font)


def _font():
    return np.frombuffer(R.FONT, np.uint8)


def visualize_detection(image, dets, seg_prob, classes, thresh=0.6, mean=R.DISPLAY_MEAN, num_classes=19):
    """image: uint8 (B, H, W, 3) or float32 (B, 3, H, W); dets: per image (k, 7); seg_prob: (B, h, w, ld)"""
    if image.dtype == np.uint8:
        B, H, W = image.shape[:3]
    else:
        B, H, W = image.shape[0], image.shape[2], image.shape[3]
    canvas = np.zeros((B, 2 * H + R.LEGEND_ROWS, W, 3), np.uint8)
    if image.dtype == np.uint8:
        canvas[:, :H] = image
    else:
        data(image, (0, 1, 2), mean, canvas, 0, 0)
    draw_list(canvas, [R.detection_rows(d, H, W, classes, thresh, "demo") for d in dets], _font(), 0, 0, H, W)
    ysrc, xsrc = R.nearest_tables(seg_prob.shape[1], seg_prob.shape[2], H, W)
    classmap(seg_prob, num_classes, R.palette_table(), ysrc, xsrc, canvas, H, 0)
    draw_list(canvas, [R.legend_rows(W)] * B, _font(), 2 * H, 0, R.LEGEND_ROWS, W)
    return canvas


def display_results(planes, label_seg, seg_prob, dets, gts, class_names, mean=R.DISPLAY_MEAN, num_classes=19):
    B, _, H, W = planes.shape
    canvas = np.zeros((B, 2 * H, 2 * W, 3), np.uint8)
    ysrc, xsrc = R.nearest_tables(seg_prob.shape[1], seg_prob.shape[2], H, W)
    pal = R.palette_table()
    data(planes, (0, 1, 2), mean, canvas, 0, 0)
    draw_list(canvas, [R.detection_rows(np.asarray(g, np.float32).reshape(-1, 6), H, W, class_names, mode="eval") for g in gts],
              _font(), 0, 0, H, W)
    labels(label_seg, pal, ysrc, xsrc, canvas, 0, W)
    data(planes, (0, 1, 2), mean, canvas, H, 0)
    draw_list(canvas, [R.detection_rows(d, H, W, class_names, mode="eval") for d in dets], _font(), H, 0, H, W)
    classmap(seg_prob, num_classes, pal, ysrc, xsrc, canvas, H, W)
    return canvas
