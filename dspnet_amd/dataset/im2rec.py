"""Record files from an image list: the database half of the reference's `tools/im2rec.py` (reading `<prefix>.lst` and
writing `<prefix>.rec` / `<prefix>.idx`), with the JPEG encode on the device, and the decode of the source files too
where they are baseline JPEGs (dataset/jpeg.py) or non-interlaced PNGs other than 16-bit greyscale (dataset/png.py: the
host inflates, the device undoes the row filters and makes the RGB bytes); Pillow decodes the rest.

    .lst   one image per line, tab-separated: integer index, one or more float label columns, path relative to `root`

    python -m dspnet_amd.dataset.im2rec PREFIX ROOT [--quality 95] [--no-pack-label] [--pass-through] [--batch 16]

Not here: `--resize` and `--center_crop` (the reference resizes with OpenCV, whose interpolation nothing in this
repository pins, so a record written here could not be checked against one written there), `--color` other than 1 (every
image is packed as three channels), PNG encoding, and the list-making half (`--list`)."""
import argparse
import io
import os

import numpy as np
import torch

from .._lib import DspnError
from . import jpeg as _jpeg
from . import jpeg_encode, recordio
from . import png as _png


def read_list(path):
    """-> list of (index, labels, relative path) in file order; labels is a list of floats.  A line with fewer than
    three columns or with columns that do not parse is an error here (the reference prints and skips it)."""
    items = []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip():
                continue
            cols = [c.strip() for c in line.strip().split("\t")]
            if len(cols) < 3:
                raise ValueError("%s:%d: an index, at least one label and a path are needed, got %d columns" % (path, lineno, len(cols)))
            try:
                items.append((int(cols[0]), [float(c) for c in cols[1:-1]], cols[-1]))
            except ValueError as e:
                raise ValueError("%s:%d: %s" % (path, lineno, e)) from e
    return items


def _header(index, labels, pack_label):
    """the reference's rule: all label columns when there are several and pack_label is set, else the first one"""
    label = np.asarray(labels, np.float32) if (len(labels) > 1 and pack_label) else labels[0]
    return recordio.IRHeader(0, label, index, 0)


def _decode(payloads, device):
    """encoded files -> (h, w, 3) RGB uint8 device tensors: baseline JPEGs and PNGs of the supported sets through the device
    decodes, everything else through Pillow; all give the pixels Pillow's convert("RGB") gives"""
    from PIL import Image
    out, jpegs, pngs = [None] * len(payloads), [], []
    for k, data in enumerate(payloads):
        if data[:2] == b"\xff\xd8":
            rc, info = _jpeg.probe_info(data)
            if rc == 0 and bool(info["supported"]):
                jpegs.append(k)
        elif _png.open_rgb(data) is not None:
            pngs.append(k)
    if jpegs:
        for k, t in zip(jpegs, _jpeg.decode_batch([payloads[k] for k in jpegs], device)):
            out[k] = t
    if pngs:
        try:
            decoded = _png.decode_rgb_batch([payloads[k] for k in pngs], device)
        except DspnError:
            decoded = ()                                        # IDAT data that does not inflate: Pillow decodes or raises, as before
        for k, t in zip(pngs, decoded):
            out[k] = t
    for k, data in enumerate(payloads):
        if out[k] is None:
            rgb = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
            out[k] = torch.from_numpy(rgb).to(device)
    return out


def write_records(prefix, root, quality=95, pack_label=True, pass_through=False, batch=16, device=None, restart_interval=0,
                  device_entropy=False):
    """reads `prefix`.lst and writes `prefix`.rec / `prefix`.idx through MXIndexedRecordIO, one record per line, keyed by
    the line's index, in list order.  pass_through: the file's bytes are packed as they are.  Otherwise each image is decoded
    to three channels (on the device where it is a JPEG or PNG a device decode supports, with Pillow otherwise) and re-encoded on
    the device, `batch` images per call, as `recordio.pack_img(header, image, quality)` would encode it.  An unreadable
    file is an error (the reference prints and skips it).  No resizing and no cropping (see the module text).
    restart_interval=n: the re-encoded files carry a restart marker every n MCUs (jpeg_encode.encode_batch), which lets the
    iterators decode them entirely on the device (device_entropy=True); the pixels they decode to are the same.
    device_entropy: encode_batch's switch for the Huffman pass on the device (the same bytes).  -> the number of records written."""
    items = read_list(prefix + ".lst")
    if not pass_through:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    rec = recordio.MXIndexedRecordIO(prefix + ".idx", prefix + ".rec", "w")
    try:
        for k in range(0, len(items), max(1, int(batch))):
            chunk = items[k:k + max(1, int(batch))]
            payloads = []
            for _, _, rel in chunk:
                with open(os.path.join(root, rel), "rb") as f:
                    payloads.append(f.read())
            headers = [_header(index, labels, pack_label) for index, labels, _ in chunk]
            if pass_through:
                packed = [recordio.pack(h, p) for h, p in zip(headers, payloads)]
            else:
                files = jpeg_encode.encode_batch(_decode(payloads, device), quality=quality, subsampling="4:2:0",
                                                 restart_interval=restart_interval, device_entropy=device_entropy)
                packed = [recordio.pack(h, f) for h, f in zip(headers, files)]
            for (index, _, _), s in zip(chunk, packed):
                rec.write_idx(index, s)
    finally:
        rec.close()
    return len(items)


def main(argv=None):
    ap = argparse.ArgumentParser(description="write PREFIX.rec / PREFIX.idx from PREFIX.lst")
    ap.add_argument("prefix")
    ap.add_argument("root")
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--no-pack-label", dest="pack_label", action="store_false")
    ap.add_argument("--pass-through", action="store_true")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--restart-interval", type=int, default=0,
                    help="MCUs between restart markers in the re-encoded files (0: none); see DESIGN.md for the choice")
    ap.add_argument("--device-entropy", action="store_true", help="Huffman-code the re-encoded files on the device too (the same bytes)")
    a = ap.parse_args(argv)
    n = write_records(a.prefix, a.root, a.quality, a.pack_label, a.pass_through, a.batch, restart_interval=a.restart_interval,
                      device_entropy=a.device_entropy)
    print("%d records -> %s.rec" % (n, a.prefix))


if __name__ == "__main__":
    main()
