"""Display images on the device: what the reference paints with OpenCV at the end of its demo
(`Detector.visualize_detection`, detect/multitask_detector.py:336-399), of its evaluation (`display_results`,
multi_eval.py:36-104) and of the solver's validation dumps, from the tensors the graph already holds.

  host   the draw rows of an image -- a few hundred boxes, tags and characters (`detection_rows`, `text_rows`,
         `legend_rows`), the nearest-resize index tables (`nearest_tables`), the colour table and the font;
  device every pixel: class colours at display size, the input image back from the net's planes, the draw list in
         painter's order (include/dspn_render.h, one launch per panel).

The class colours and names are the dataset's (pinned by tests/golden/cityscapes_palette.json).  Text is this build's
own: a 5 x 7 font in a 6 x 8 cell, integer scale s = max(1, (H + 256) // 512), a tag of len(text) * 6s by 8s pixels --
not the Hershey font of cv2.putText, whose metrics are not restated.  Pillow is used by `save_png` only."""
import math

import numpy as np
import torch

from .. import _lib
from .. import functional as fn

# Cityscapes trainId -> (name, colour RGB): the 19 evaluated classes and trainId 19 ('lane marking' in the
# reference's copy of the label table); every other index of the 256-entry table is black, 255 (ignore) included
_TRAIN_IDS = (
    ("road", (128, 64, 128)), ("sidewalk", (244, 35, 232)), ("building", (70, 70, 70)), ("wall", (102, 102, 156)),
    ("fence", (190, 153, 153)), ("pole", (153, 153, 153)), ("traffic light", (250, 170, 30)), ("traffic sign", (220, 220, 0)),
    ("vegetation", (107, 142, 35)), ("terrain", (152, 251, 152)), ("sky", (70, 130, 180)), ("person", (220, 20, 60)),
    ("rider", (255, 0, 0)), ("car", (0, 0, 142)), ("truck", (0, 0, 70)), ("bus", (0, 60, 100)), ("train", (0, 80, 100)),
    ("motorcycle", (0, 0, 230)), ("bicycle", (119, 11, 32)), ("lane marking", (192, 64, 192)),
)
SEG_NAMES = tuple(name for name, _ in _TRAIN_IDS)
PALETTE = tuple(colour for _, colour in _TRAIN_IDS)

# detection class -> trainId whose colour its box takes (multitask_detector.py:359), and the names a tag shows (:13-15)
DET2SEG = {0: 11, 1: 12, 2: 13, 3: 14, 4: 15, 5: 16, 6: 17, 7: 18}
SHORT_CLASS_NAME = {"traffic light": "tlight", "traffic sign": "tsign", "person": "person", "rider": "rider", "car": "car",
                    "truck": "truck", "bus": "bus", "train": "train", "motorcycle": "mbike", "bicycle": "bike",
                    "vegetation": "tree"}

DISPLAY_MEAN = (123.68, 116.779, 103.939)     # what multi_eval.py:67 adds back (to data that had 123 / 117 / 104 subtracted)
TAG_RGB = (0, 0, 128)                         # color=(128, 0, 0) on the reference's BGR image
EVAL_BOX_RGB = (128, 0, 0)                    # color=(0, 0, 128) on a BGR image (multi_eval.py:84, :92)
WHITE = (255, 255, 255)
LEGEND_ROWS = 30                              # get_seg_labels(shape=(30, W, 3))

# 5 x 7 font, ASCII 32..126: seven rows from the top, two hex digits each, bit 4 the leftmost column
_GLYPHS = (
    (" ", "00000000000000"), ("!", "04040404040004"), ('"', "0A0A0A00000000"), ("#", "0A0A1F0A1F0A0A"),
    ("$", "040F140E051E04"), ("%", "18190204081303"), ("&", "0C12140815120D"), ("'", "0C040800000000"),
    ("(", "02040808080402"), (")", "08040202020408"), ("*", "0004150E150400"), ("+", "0004041F040400"),
    (",", "000000000C0408"), ("-", "0000001F000000"), (".", "00000000000C0C"), ("/", "00010204081000"),
    ("0", "0E11131519110E"), ("1", "040C040404040E"), ("2", "0E11010204081F"), ("3", "1F02040201110E"),
    ("4", "02060A121F0202"), ("5", "1F101E0101110E"), ("6", "0608101E11110E"), ("7", "1F010204080808"),
    ("8", "0E11110E11110E"), ("9", "0E11110F01020C"), (":", "000C0C000C0C00"), (";", "000C0C000C0408"),
    ("<", "02040810080402"), ("=", "00001F001F0000"), (">", "08040201020408"), ("?", "0E110102040004"),
    ("@", "0E11010D15150E"), ("A", "0E1111111F1111"), ("B", "1E11111E11111E"), ("C", "0E11101010110E"),
    ("D", "1C12111111121C"), ("E", "1F10101E10101F"), ("F", "1F10101E101010"), ("G", "0E11101711110F"),
    ("H", "1111111F111111"), ("I", "0E04040404040E"), ("J", "0702020202120C"), ("K", "11121418141211"),
    ("L", "1010101010101F"), ("M", "111B1515111111"), ("N", "11111915131111"), ("O", "0E11111111110E"),
    ("P", "1E11111E101010"), ("Q", "0E11111115120D"), ("R", "1E11111E141211"), ("S", "0F10100E01011E"),
    ("T", "1F040404040404"), ("U", "1111111111110E"), ("V", "11111111110A04"), ("W", "1111111515150A"),
    ("X", "11110A040A1111"), ("Y", "1111110A040404"), ("Z", "1F01020408101F"), ("[", "0E08080808080E"),
    ("\\", "00100804020100"), ("]", "0E02020202020E"), ("^", "040A1100000000"), ("_", "0000000000001F"),
    ("`", "08040200000000"), ("a", "00000E010F110F"), ("b", "1010161911111E"), ("c", "00000E1010110E"),
    ("d", "01010D1311110F"), ("e", "00000E111F100E"), ("f", "0609081C080808"), ("g", "000F11110F010E"),
    ("h", "10101619111111"), ("i", "04000C0404040E"), ("j", "0200060202120C"), ("k", "10101214181412"),
    ("l", "0C04040404040E"), ("m", "00001A15151111"), ("n", "00001619111111"), ("o", "00000E1111110E"),
    ("p", "00001E111E1010"), ("q", "00000D130F0101"), ("r", "00001619101010"), ("s", "00000E100E011E"),
    ("t", "08081C08080906"), ("u", "0000111111130D"), ("v", "00001111110A04"), ("w", "0000111115150A"),
    ("x", "0000110A040A11"), ("y", "000011110F010E"), ("z", "00001F0204081F"), ("{", "02040408040402"),
    ("|", "04040404040404"), ("}", "08040402040408"), ("~", "00000815020000"),
)
assert [ord(ch) for ch, _ in _GLYPHS] == list(range(32, 127))
FONT = b"".join(bytes.fromhex(rows) for _, rows in _GLYPHS)
assert len(FONT) == fn.RENDER_FONT_BYTES and max(FONT) < 32


def palette_table():
    """(256, 3) uint8: PALETTE in its first rows, black below (the `lut` of multi_eval.py:40-44)"""
    t = np.zeros((256, 3), np.uint8)
    t[:len(PALETTE)] = np.array(PALETTE, np.uint8)
    return t


def nearest_tables(hs, ws, Hd, Wd):
    """source row of every destination row and source column of every destination column of a nearest-neighbour resize
    (hs, ws) -> (Hd, Wd), as OpenCV's resizeNN states them, in double: min(floor(dst * (1 / (Nd / float(Ns)))), Ns - 1)"""
    def table(Ns, Nd):
        inv = 1.0 / (Nd / float(Ns))
        return np.minimum(np.floor(np.arange(Nd, dtype=np.float64) * inv), Ns - 1).astype(np.int32)
    return table(int(hs), int(Hd)), table(int(ws), int(Wd))


def text_scale(H):
    return max(1, (int(H) + 256) // 512)


def text_rows(text, x, y_bottom, scale, rgb):
    """one glyph row per character; (x, y_bottom) is the bottom-left corner of the text, as cv2.putText takes it: the
    cell of character i is 6s x 8s at (x + i * 6s, y_bottom - 8s), its 5 x 7 pattern sits on the cell's bottom-left"""
    s = int(scale)
    r, g, b = rgb
    return [(fn.DRAW_GLYPH, int(x) + i * 6 * s, int(y_bottom) - 7 * s, 0, 0, r, g, b, (s << 8) | min(ord(ch), 255))
            for i, ch in enumerate(text)]


def tag_rows(text, x, y_bottom, scale):
    """the filled tag of len(text) * 6s by 8s pixels whose bottom-left corner is (x, y_bottom - 1), and the text in white"""
    s = int(scale)
    if not text:
        return []
    return [(fn.DRAW_FILL, int(x), int(y_bottom) - 8 * s, int(x) + len(text) * 6 * s - 1, int(y_bottom) - 1) + TAG_RGB + (0,)] + \
        text_rows(text, x, y_bottom, s, WHITE)


def _round_half_away(v):
    """Python 2's round() on a float: half away from zero"""
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def detection_rows(dets, H, W, classes, thresh=0.6, mode="demo"):
    """the draw rows of one image, in painter's order.
    dets: (k, 7) host rows [id, score, xmin, ymin, xmax, ymax, dist] (rows with id < 0 are no detections), or, with
    mode="eval", (k, 6) ground-truth rows [cls, xmin, ymin, xmax, ymax, dist].
    mode="demo" (visualize_detection, multitask_detector.py:371-386): by distance descending (np.argsort reversed, as
      there), score > thresh, corners int(v * size) (truncation), box colour of the class, thickness 2 if H > 320 else 1,
      tag text '%s %.0fm' of the short class name;
    mode="eval" (display_results, multi_eval.py:79-94): table order, no threshold, corners int(round(v * size)) with
      halves away from zero (Python 2), box colour EVAL_BOX_RGB, thickness 1, tag text '%s:%.0fm'; ground-truth boxes under
      100 px^2 are skipped.
    The values are float32; every product and comparison is in double, as a float32 scalar times a Python number was when
    the reference was written."""
    if mode not in ("demo", "eval"):
        raise _lib.DspnError("detection_rows: mode is 'demo' or 'eval'")
    dets = np.asarray(dets, np.float32)
    dets = dets.reshape(-1, dets.shape[-1] if dets.ndim == 2 else 7)
    gt = dets.shape[1] == 6
    if gt and mode != "eval":
        raise _lib.DspnError("detection_rows: ground-truth rows are drawn with mode='eval'")
    if not gt and dets.shape[1] != 7:
        raise _lib.DspnError("detection_rows: rows are [id, score, xmin, ymin, xmax, ymax, dist] or [cls, xmin, ymin, xmax, ymax, dist]")
    H, W = int(H), int(W)
    s = text_scale(H)
    rows = []
    if gt:
        for box in dets.tolist():
            bbox = [_round_half_away(box[1] * W), _round_half_away(box[2] * H), _round_half_away(box[3] * W), _round_half_away(box[4] * H)]
            if (bbox[2] - bbox[0]) * (bbox[3] - bbox[1]) < 100:
                continue
            rows.append((fn.DRAW_OUTLINE,) + tuple(bbox) + EVAL_BOX_RGB + (1,))
            rows += tag_rows("%s:%.0fm" % (classes[int(box[0])], box[5] * 255.), bbox[0], bbox[1], s)
        return rows
    dets = dets[dets[:, 0] >= 0]
    if mode == "demo":
        dets = dets[np.argsort(dets[:, 6], axis=0)[::-1]]         # "draw nearest first": the largest distance paints first
        thickness = 2 if H > 320 else 1
    for det in dets.tolist():                                      # float32 values, every product in double (see above)
        cls_id = int(det[0])
        scaled = [det[2] * W, det[3] * H, det[4] * W, det[5] * H]
        if mode == "demo":
            if not det[1] > thresh:
                continue
            bbox = [int(v) for v in scaled]
            name = classes[cls_id]
            text = "%s %.0fm" % (SHORT_CLASS_NAME.get(name, name), det[6] * 255.)
            rows.append((fn.DRAW_OUTLINE,) + tuple(bbox) + tuple(PALETTE[DET2SEG[cls_id]]) + (thickness,))
        else:
            bbox = [_round_half_away(v) for v in scaled]
            text = "%s:%.0fm" % (classes[cls_id], det[6] * 255.)
            rows.append((fn.DRAW_OUTLINE,) + tuple(bbox) + EVAL_BOX_RGB + (1,))
        rows += tag_rows(text, bbox[0], bbox[1], s)
    return rows


def legend_rows(W):
    """the 30-row strip of get_seg_labels (multitask_detector.py:17-43): a 15 x 15 square of every class colour at
    (idx * 100, 0) for idx < 10 and ((idx - 10) * 100, 15) for 10 <= idx < 20, followed by the class name in white"""
    padding, blocksize, notes = 100, 15, 10
    rows = []
    for idx, (name, colour) in enumerate(zip(SEG_NAMES, PALETTE)):
        ax, ay = (idx * padding, 0) if idx < notes else ((idx - notes) * padding, blocksize)
        if ax >= int(W):
            continue
        rows.append((fn.DRAW_FILL, ax, ay, ax + blocksize - 1, ay + blocksize - 1) + tuple(colour) + (0,))
        rows += text_rows(name, ax + blocksize + 1, ay + 10, 1, WHITE)
    return rows


_device_tables = {}


def _constants(device):
    """the palette and the font on the device (uploaded once per device)"""
    key = str(device)
    if key not in _device_tables:
        _device_tables[key] = (torch.from_numpy(palette_table().reshape(-1)).to(device),
                               torch.from_numpy(np.frombuffer(FONT, np.uint8).copy()).to(device))
    return _device_tables[key]


def _tables_dev(hs, ws, Hd, Wd, device):
    ysrc, xsrc = nearest_tables(hs, ws, Hd, Wd)
    return torch.from_numpy(ysrc).to(device), torch.from_numpy(xsrc).to(device)


def _host_rows(dets, B):
    """(B, N, 7) tensor / array or a sequence of per-image row tables -> list of B host arrays"""
    if hasattr(dets, "detach"):
        dets = dets.detach().cpu().numpy()
    out = [np.asarray(d.detach().cpu().numpy() if hasattr(d, "detach") else d, np.float32) for d in dets]
    if len(out) != B:
        raise _lib.DspnError("render: %d row tables for a batch of %d" % (len(out), B))
    return out


def _image_panel(canvas, frame_or_data, mean, y0, x0):
    """uint8 (B, H, W, 3) RGB frames are copied, float32 (B, 3, H, W) planes go through dspn_render_data_f32"""
    if frame_or_data.dtype == torch.uint8:
        H, W = frame_or_data.shape[1:3]
        canvas[:, y0:y0 + H, x0:x0 + W].copy_(frame_or_data)
    else:
        fn.render_data(frame_or_data.contiguous(), (0, 1, 2), mean, canvas, y0, x0)


def _frame_size(frame_or_data):
    if frame_or_data.dim() != 4 or not frame_or_data.is_cuda:
        raise _lib.DspnError("render: the image is a device tensor, uint8 (B, H, W, 3) or float32 (B, 3, H, W)")
    if frame_or_data.dtype == torch.uint8 and frame_or_data.shape[3] == 3:
        return frame_or_data.shape[0], frame_or_data.shape[1], frame_or_data.shape[2]
    if frame_or_data.dtype == torch.float32 and frame_or_data.shape[1] == 3:
        return frame_or_data.shape[0], frame_or_data.shape[2], frame_or_data.shape[3]
    raise _lib.DspnError("render: the image is uint8 (B, H, W, 3) or float32 (B, 3, H, W)")


def visualize_detection(frame_or_data, dets, seg_prob, classes, thresh=0.6, mean=DISPLAY_MEAN, num_classes=19):
    """-> (B, H + H + 30, W, 3) uint8 device tensor, RGB: the image with boxes and tags, the class colours at frame size and
    the legend, stacked as np.vstack((im, seg, annotation)) (multitask_detector.py:336-391).
    frame_or_data: device uint8 (B, H, W, 3) RGB frames, or the net's input, float32 (B, 3, H, W) RGB planes, shown as
    sat_u8(trunc(data + mean)); dets: (B, N, 7) det_out (device or host) or B row tables; seg_prob: (B, h, w, ld) NHWC
    class scores as the graph holds seg_out.prob."""
    B, H, W = _frame_size(frame_or_data)
    device = frame_or_data.device
    palette, font = _constants(device)
    rows = [detection_rows(d, H, W, classes, thresh, "demo") for d in _host_rows(dets, B)]
    canvas = torch.zeros(B, 2 * H + LEGEND_ROWS, W, 3, dtype=torch.uint8, device=device)
    _image_panel(canvas, frame_or_data, mean, 0, 0)
    fn.render_draw_list(canvas, fn.draw_table(rows, device), font, 0, 0, H, W)
    ysrc, xsrc = _tables_dev(seg_prob.shape[1], seg_prob.shape[2], H, W, device)
    fn.render_classmap(seg_prob.contiguous(), num_classes, palette, ysrc, xsrc, canvas, H, 0)
    fn.render_draw_list(canvas, fn.draw_table([legend_rows(W)] * B, device), font, 2 * H, 0, LEGEND_ROWS, W)
    return canvas


def display_results(data, label_seg, seg_prob, dets, gts, class_names, mean=DISPLAY_MEAN, num_classes=19):
    """-> (B, 2H, 2W, 3) uint8 device tensor, RGB: the 2 x 2 mosaic of multi_eval.py:100,
        image + ground-truth boxes | ground-truth colours
        image + detections         | predicted colours
    data: (B, 3, H, W) float32, the net's input; label_seg: (B, h, w) float32 trainIds (255 = ignore);
    seg_prob: (B, h, w, ld) NHWC; dets: per image the rows the script keeps (id >= 0, score > .1; (k, 7));
    gts: per image (L, 6) label rows [cls, xmin, ymin, xmax, ymax, dist]."""
    B, H, W = _frame_size(data)
    device = data.device
    palette, font = _constants(device)
    det_rows = [detection_rows(d, H, W, class_names, mode="eval") for d in _host_rows(dets, B)]
    gt_rows = [detection_rows(np.asarray(g, np.float32).reshape(-1, 6), H, W, class_names, mode="eval") for g in _host_rows(gts, B)]
    canvas = torch.zeros(B, 2 * H, 2 * W, 3, dtype=torch.uint8, device=device)
    data = data.contiguous()
    ysrc, xsrc = _tables_dev(seg_prob.shape[1], seg_prob.shape[2], H, W, device)
    fn.render_data(data, (0, 1, 2), mean, canvas, 0, 0)
    fn.render_draw_list(canvas, fn.draw_table(gt_rows, device), font, 0, 0, H, W)
    fn.render_labels(label_seg.contiguous(), palette, ysrc, xsrc, canvas, 0, W)
    fn.render_data(data, (0, 1, 2), mean, canvas, H, 0)
    fn.render_draw_list(canvas, fn.draw_table(det_rows, device), font, H, 0, H, W)
    fn.render_classmap(seg_prob.contiguous(), num_classes, palette, ysrc, xsrc, canvas, H, W)
    return canvas


def save_png(path, tensor):
    """(H, W, 3) RGB or (H, W) grey uint8 tensor (device or host) -> PNG file, through Pillow: file output only"""
    try:
        from PIL import Image
    except ImportError as e:
        raise _lib.DspnError("save_png: writing image files needs Pillow, which cannot be imported (%s)" % e) from e
    a = tensor.detach().cpu().numpy() if hasattr(tensor, "detach") else np.asarray(tensor)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise _lib.DspnError("save_png: (H, W) or (H, W, 3) uint8, got %s %s" % (a.dtype, a.shape))
    Image.fromarray(np.ascontiguousarray(a)).save(path, format="PNG")


def save_pngs(paths, tensors, compress_level=6, device_deflate=False):
    """a batch of images -> PNG files: (H, W) uint8, (H, W) uint16 or (H, W, 3) uint8 RGB tensors of any mix of sizes, device
    or host (uploaded first).  The row filters of the whole batch run on the device in one call, deflate on a thread pool
    (dataset/png_encode.py); the pixels and the filtered stream inside each file are those of `save_png`'s file.
    device_deflate=True: the deflate runs on the device too (png_encode.encode_batch's keyword: larger files, compress_level
    not used; for large photo-like images)."""
    from ..dataset import png_encode
    paths, tensors = list(paths), list(tensors)
    if len(paths) != len(tensors):
        raise _lib.DspnError("save_pngs: %d paths for %d images" % (len(paths), len(tensors)))
    for path, data in zip(paths, png_encode.encode_batch(tensors, compress_level=compress_level, device_deflate=device_deflate)):
        with open(path, "wb") as f:
            f.write(data)


def save_jpeg(path, image, quality=95, device_entropy=False):
    """(H, W, 3) RGB or (H, W) grey uint8 tensor -> baseline JPEG file (4:2:0 for colour), the file Pillow would write for
    the same pixels and quality.  The encode runs on the device (dataset/jpeg_encode.py: colour conversion, downsampling,
    DCT and quantisation there, Huffman coding on the host, or on the device as well with device_entropy=True: the same bytes);
    a host tensor or array is uploaded to the current device first."""
    from ..dataset import jpeg_encode
    t = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
    if t.dtype != torch.uint8 or not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)):
        raise _lib.DspnError("save_jpeg: (H, W) or (H, W, 3) uint8, got %s %s" % (t.dtype, tuple(t.shape)))
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    (data,) = jpeg_encode.encode_batch([t.detach()], quality=quality, device_entropy=device_entropy)
    with open(path, "wb") as f:
        f.write(data)
