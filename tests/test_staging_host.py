"""Host side of the staging path shared by the iterators (dataset/staging.py and its users in dataset/jpeg.py and
dataset/png.py): the pools and their guard event, and the routing of a batch between the device decode and Pillow.
Needs the built library, no GPU."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as jc
import ref_jpeg
import ref_png as rp
from dspnet_amd.dataset import jpeg as dj
from dspnet_amd.dataset import png as dp
from dspnet_amd.dataset import staging


# ---- 1. pools -------------------------------------------------------------------------------------------------------
class _Event(object):
    log = []

    def record(self, stream):
        self.log.append(("record", id(self), stream))

    def synchronize(self):
        self.log.append(("synchronize", id(self)))


@pytest.fixture()
def pools():
    _Event.log = []
    return staging.HostPools(False, event_type=_Event)


def test_take_grows_and_reuses(pools):
    a = pools.take("a", 10, torch.uint8)
    assert a.numel() >= 10 and a.dtype == torch.uint8 and not a.is_pinned()
    assert pools.take("a", 5, torch.uint8).data_ptr() == a.data_ptr()
    big = pools.take("a", 1000, torch.uint8)
    assert big.numel() >= 1000
    assert pools.take("a", 1000, torch.uint8).data_ptr() == big.data_ptr()
    c = pools.take("c", 0, torch.int16, floor=64)
    assert c.numel() >= 64 and c.dtype == torch.int16
    assert pools.take("empty", 0, torch.uint8).numel() >= 1
    assert _Event.log == []                                     # no upload recorded: nothing to wait for


def test_take_waits_once_for_the_last_upload(pools):
    pools.take("a", 10, torch.uint8)
    pools.take("b", 10, torch.int16)
    pools.uploaded("stream-1")
    (_, event, stream), = _Event.log
    assert stream == "stream-1"
    pools.take("b", 4, torch.int16)                             # any name: the event guards the whole set
    assert _Event.log[1:] == [("synchronize", event)]
    pools.take("a", 4, torch.uint8)
    pools.take("new", 4, torch.uint8)
    assert len(_Event.log) == 2
    pools.uploaded("stream-2")
    pools.uploaded("stream-3")                                  # the later event is the one that counts
    last = _Event.log[-1][1]
    pools.take("a", 2000, torch.uint8)
    assert _Event.log[4:] == [("synchronize", last)]


# ---- 2. JPEG routing ------------------------------------------------------------------------------------------------
def _corrupt_scan():
    """the first stream of tests/test_jpeg_host.py::test_corrupt_scans_are_errors; Pillow alone decodes it"""
    data = jc.stream("64x200-ss2-q90-std-noise")
    g = np.random.Generator(np.random.PCG64(41))
    bad = bytearray(data)
    for at in g.integers(ref_jpeg.parse(data)["scan_pos"], len(data) - 2, 8):
        bad[at] ^= 0xFF
    return bytes(bad)


def _png_rgb(h, w, seed):
    buf = io.BytesIO()
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)).save(buf, format="PNG")
    return buf.getvalue()


def _route_images(payloads, device_jpeg):
    """the host phase of an iterator over `payloads` -> (opened, batch, pixel offsets, coefficient pool, pixel pool)"""
    opened = [dj.open_image(p, device_jpeg) for p in payloads]
    sizes = [im.size[0] * im.size[1] * 3 for im in opened]
    offsets = np.cumsum([0] + sizes).tolist()
    batch = dj.CodedBatch([im.info if isinstance(im, dj.Coded) else None for im in opened], offsets)
    coefs = np.full(max(batch.count, 64), 0x5A5A, np.int16)
    pixels = np.full(offsets[-1], 0xA5, np.uint8)
    dsts = [pixels[o:o + n].reshape(im.size[1], im.size[0], 3) for o, n, im in zip(offsets, sizes, opened)]
    batch.answered([dj.decode_image(*job) for job in zip(opened, dsts, batch.slices(coefs))])
    return opened, batch, offsets, coefs, pixels


def test_jpeg_routing():
    name = "37x53-ss2-q90-std-noise"
    picture = jc.image(zlib.crc32(name.encode()), 37, 53, "noise")                             # as jc.stream makes it
    payloads = [jc.stream(name), jc.encode(picture, progressive=True, quality=90), jc.stream("50x31-grey-q90-smooth"),
                _corrupt_scan(), _png_rgb(20, 31, 3)]
    opened, batch, offsets, coefs, pixels = _route_images(payloads, True)
    assert [isinstance(im, dj.Coded) for im in opened] == [True, False, True, True, False]    # the corrupt one probes well
    assert [im.size for im in opened] == [(53, 37), (53, 37), (31, 50), (200, 64), (31, 20)]
    assert offsets == [0, 5883, 11766, 16416, 54816, 56676]
    assert batch.samples["skip"].tolist() == [0, 1, 0, 1, 1]
    assert (batch.on_device, batch.fallbacks) == (2, 3)
    assert batch.samples["img_offset"][[0, 2]].tolist() == [0, 11766]
    # coefficient slices back to back in multiples of 64; the corrupt stream keeps the slice it was planned
    at = 0
    for k, (o, n) in enumerate(batch.spans):
        assert o == at and n % 64 == 0 and (n > 0) == (k in (0, 2, 3))
        at += n
    assert batch.count == at and (coefs[at:] == 0x5A5A).all()
    for k in (0, 2):
        rc, info = dj.probe_info(payloads[k])
        want = np.zeros(int(info["coef_count"]), np.int16)
        assert rc == 0 and dj.entropy_decode(payloads[k], info, want) == 0
        o, n = batch.spans[k]
        assert n == want.size and np.array_equal(coefs[o:o + n], want)
        assert batch.samples["coef_offset"][k].tolist() == (info["coef_offset"] + o).tolist()
        assert (pixels[offsets[k]:offsets[k + 1]] == 0xA5).all()                               # left to the device
    for k in (1, 3, 4):
        want = np.asarray(Image.open(io.BytesIO(payloads[k])).convert("RGB"))
        assert np.array_equal(pixels[offsets[k]:offsets[k + 1]].reshape(want.shape), want)


def test_device_jpeg_off_never_probes(monkeypatch):
    monkeypatch.setattr(dj, "probe_info", lambda payload: pytest.fail("probed with device_jpeg off"))
    payloads = [jc.stream("37x53-ss2-q90-std-noise"), jc.stream("50x31-grey-q90-smooth"), _png_rgb(20, 31, 3)]
    opened, batch, offsets, coefs, pixels = _route_images(payloads, False)
    assert not any(isinstance(im, dj.Coded) for im in opened)
    assert batch.count == 0 and (batch.on_device, batch.fallbacks) == (0, 3) and batch.samples["skip"].tolist() == [1, 1, 1]
    for k, p in enumerate(payloads):
        want = jc.pillow_pixels(p)
        assert np.array_equal(pixels[offsets[k]:offsets[k + 1]].reshape(want.shape), want)


def test_truncated_scan_raises_pillows_error():
    """probes as supported, fails the entropy pass, and Pillow refuses it too: that error reaches the caller"""
    cut = jc.stream("37x53-ss2-q90-std-noise")[:-40]
    im = dj.open_image(cut, True)
    assert isinstance(im, dj.Coded)
    with pytest.raises(OSError, match="truncated"):
        dj.decode_image(im, np.zeros((37, 53, 3), np.uint8), np.zeros(int(im.info["coef_count"]), np.int16))


# ---- 3. PNG label routing -------------------------------------------------------------------------------------------
def _label_expression(payload):
    im = Image.open(io.BytesIO(payload))
    return np.asarray(im if im.mode in ("L", "P") else im.convert("L"))


def _route_labels(payloads, device_png):
    opened = [dp.open_label(p, device_png) for p in payloads]
    sizes = [im.size[0] * im.size[1] for im in opened]
    offsets = np.cumsum([0] + sizes).tolist()
    batch = dp.CodedBatch([im.info if isinstance(im, dp.CodedLabel) else None for im in opened], offsets)
    raw = np.full(max(batch.count, 1), 0x5A, np.uint8)
    labels = np.full(offsets[-1], 0xA5, np.uint8)
    dsts = [labels[o:o + n].reshape(im.size[1], im.size[0]) for o, n, im in zip(offsets, sizes, opened)]
    return opened, batch, offsets, raw, labels, list(zip(opened, dsts, batch.slices(raw)))


def _idat(payload):
    return b"".join(d for k, d in rp.chunks(payload) if k == b"IDAT")


def test_png_label_routing():
    g = np.random.Generator(np.random.PCG64(31))
    h, w = 37, 53
    grey = g.integers(0, 256, (h, w), dtype=np.uint8)
    payloads = [rp.write(grey, rp.filters_for(g, h, "mix")), rp.write(grey, rp.filters_for(g, h, "mix"), palette=True),
                rp.write_interlaced(grey), rp.write_rgb(g.integers(0, 256, (h, w, 3), dtype=np.uint8), rp.filters_for(g, h, "mix")),
                rp.write(g.integers(0, 65536, (h, w), dtype=np.uint16), rp.filters_for(g, h, "mix"))]
    opened, batch, offsets, raw, labels, jobs = _route_labels(payloads, True)
    assert [isinstance(im, dp.CodedLabel) for im in opened] == [True, True, False, False, False]
    assert all(im.size == (w, h) for im in opened)
    batch.answered([dp.decode_label(*job) for job in jobs])
    assert batch.samples["skip"].tolist() == [0, 0, 1, 1, 1] and (batch.on_device, batch.fallbacks) == (2, 3)
    assert batch.spans == [(0, h * (w + 1)), (h * (w + 1), h * (w + 1)), (2 * h * (w + 1), 0)] + [(2 * h * (w + 1), 0)] * 2
    for k in (0, 1):
        o, n = batch.spans[k]
        assert raw[o:o + n].tobytes() == zlib.decompress(_idat(payloads[k]))
        assert (batch.samples["raw_offset"][k], batch.samples["out_offset"][k]) == (o, offsets[k])
        assert (labels[offsets[k]:offsets[k + 1]] == 0xA5).all()                               # left to the device
    for k in (2, 3, 4):
        assert np.array_equal(labels[offsets[k]:offsets[k + 1]].reshape(h, w), _label_expression(payloads[k]))
    # a record without a label map is neither on the device nor a fallback
    batch.answered([True, False, None, None, True])
    assert batch.samples["skip"].tolist() == [0, 1, 1, 1, 0] and (batch.on_device, batch.fallbacks) == (2, 1)
    # device_png off: Pillow throughout, nothing is probed
    opened, batch, offsets, raw, labels, jobs = _route_labels(payloads[:2], False)
    assert not any(isinstance(im, dp.CodedLabel) for im in opened) and batch.count == 0
    batch.answered([dp.decode_label(*job) for job in jobs])
    assert (batch.on_device, batch.fallbacks) == (0, 2)
    assert np.array_equal(labels.reshape(2, h, w), np.stack([_label_expression(p) for p in payloads[:2]]))


def test_damaged_idat_raises_pillows_error():
    """two damaged bytes in the middle of the deflate stream under a valid chunk CRC: `probe` accepts the file, the
    inflate reports a zlib error, and Pillow alone raises OSError("broken data stream ...") on these bytes -- so does the job"""
    g = np.random.Generator(np.random.PCG64(5))
    h, w = 37, 53
    z = bytearray(zlib.compress(rp.filter_rows(g.integers(0, 256, (h, w), dtype=np.uint8), rp.filters_for(g, h, "mix"), 1), 6))
    z[len(z) // 2] ^= 0xFF
    z[len(z) // 2 + 1] ^= 0x55
    data = rp.assemble(w, h, 8, 0, None, idat_chunks=1, compressed=bytes(z))
    with pytest.raises(OSError, match="broken data stream"):
        np.asarray(Image.open(io.BytesIO(data)))
    im = dp.open_label(data, True)
    assert isinstance(im, dp.CodedLabel)
    raw = np.zeros(im.info["raw_bytes"], np.uint8)
    assert dp.inflate_into(data, im.info, raw) == dp.INFLATE_ZLIB
    with pytest.raises(OSError, match="broken data stream"):
        dp.decode_label(im, np.zeros((h, w), np.uint8), raw)
