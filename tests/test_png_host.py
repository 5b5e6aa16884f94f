"""Host half of the PNG decode (dspnet_amd/dataset/png.py; no GPU): the numpy reading of the reconstruction in
tests/ref_png.py is pinned to Pillow, `probe` agrees with Pillow on what a stream is and names why it will not take one,
and malformed input ends in DspnError (probe) or a status (inflate_into), never in another exception or a stray write."""
import io
import struct
import zlib

import numpy as np
import pytest

import ref_png as rp
from dspnet_amd import _lib
from dspnet_amd.dataset import iterator as it
from dspnet_amd.dataset import png as dp


def _pinned_streams():
    """(name, payload): every filter type on row 0 and on later rows, all-one-type images and random mixes, the widths
    around 1 and 64, both byte widths, random bytes; plus streams Pillow wrote"""
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(2024))
    out = []
    for bpp in (1, 2):
        for w in (1, 2, 3, 63, 64, 65):
            for kind in (0, 1, 2, 3, 4, "mix"):
                h = 7 if w < 63 else 4
                arr = rp.random_image(g, h, w, bpp)
                out.append(("w%d-b%d-%s" % (w, bpp, kind), rp.write(arr, rp.filters_for(g, h, kind))))
        for first in range(5):                                  # type `first` on row 0, every type below it
            arr = rp.random_image(g, 6, 9, bpp)
            out.append(("first%d-b%d" % (first, bpp), rp.write(arr, [first, 0, 1, 2, 3, 4], idat_chunks=1)))
    arr = g.integers(0, 256, (9, 33), dtype=np.uint8)
    out.append(("palette-mix", rp.write(arr, rp.filters_for(g, 9, "mix"), palette=True)))
    smooth = (np.add.outer(np.arange(40), np.arange(70)) // 3).astype(np.uint8)
    for name, im in (("pillow-L", Image.fromarray(smooth)), ("pillow-L-noise", Image.fromarray(rp.random_image(g, 31, 17, 1))),
                     ("pillow-I16", Image.fromarray((smooth.astype(np.uint16) * 257 + 3))),
                     ("pillow-P", Image.fromarray(smooth % 19).convert("P"))):
        buf = io.BytesIO()
        im.save(buf, format="PNG")
        out.append((name, buf.getvalue()))
    return out


STREAMS = _pinned_streams()


def test_numpy_reading_equals_pillow():
    assert len(STREAMS) > 80
    seen = set()
    for name, data in STREAMS:
        want, got = rp.pillow(data), rp.decode(data)
        assert got.dtype == want.dtype and got.shape == want.shape, name
        np.testing.assert_array_equal(got, want, err_msg=name)
        seen |= set(np.frombuffer(zlib.decompress(b"".join(d for k, d in rp.chunks(data) if k == b"IDAT")), np.uint8)
                    [0::dp.probe(data)["row_bytes"] + 1].tolist())
    assert seen == {0, 1, 2, 3, 4}
    assert rp.pillow(dict(STREAMS)["pillow-I16"]).dtype == np.uint16


def test_probe_fields_agree_with_pillow():
    from PIL import Image
    for name, data in STREAMS:
        info, im = dp.probe(data), Image.open(io.BytesIO(data))
        assert (info["width"], info["height"]) == im.size, name
        mode = {(8, 0): "L", (8, 3): "P", (16, 0): "I;16"}[(info["bit_depth"], info["colour_type"])]
        assert im.mode == mode and info["supported"] and info["reason"] == "ok" and info["reason_code"] == 0, name
        bpp = 2 if mode == "I;16" else 1
        assert info["bytes_per_pixel"] == bpp and info["row_bytes"] == bpp * im.size[0] and info["interlace"] == 0
        assert info["raw_bytes"] == im.size[1] * (info["row_bytes"] + 1), name


def test_inflate_into_then_reconstruction_equals_pillow():
    for name, data in STREAMS:
        info = dp.probe(data)
        buf = np.full(info["raw_bytes"] + 32, 0xA5, np.uint8)
        assert dp.inflate_into(data, info, buf[16:-16]) == 0, name
        assert (buf[:16] == 0xA5).all() and (buf[-16:] == 0xA5).all()
        rows = rp.unfilter(buf[16:-16].tobytes(), info["height"], info["row_bytes"], info["bytes_per_pixel"])
        got = rows.view(">u2").astype(np.uint16) if info["bytes_per_pixel"] == 2 else rows
        np.testing.assert_array_equal(got, rp.pillow(data), err_msg=name)


def _unsupported_streams():
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(5))
    grey = g.integers(0, 256, (12, 10), dtype=np.uint8)

    def saved(im, **kw):
        buf = io.BytesIO()
        im.save(buf, format="PNG", **kw)
        return buf.getvalue()

    rgb = Image.fromarray(g.integers(0, 256, (12, 10, 3), dtype=np.uint8))
    return [
        ("depth 1", saved(Image.fromarray(grey > 127)), "bit depth below 8"),
        ("depth 2", saved(Image.fromarray(grey % 4).convert("P"), bits=2), "bit depth below 8"),
        ("depth 4", saved(Image.fromarray(grey % 16).convert("P"), bits=4), "bit depth below 8"),
        ("RGB", saved(rgb), "colour type"),
        ("RGB by hand", rp.write_rgb(np.asarray(rgb), [4] * 12), "colour type"),
        ("RGBA", saved(rgb.convert("RGBA")), "colour type"),
        ("grey + alpha", saved(rgb.convert("LA")), "colour type"),
        ("interlaced", rp.write_interlaced(grey), "interlace"),
        ("interlaced 16", rp.write_interlaced(grey.astype(np.uint16) * 250), "interlace"),
        ("tRNS", saved(Image.fromarray(grey), transparency=7), "tRNS"),
        ("tRNS palette", saved(Image.fromarray(grey % 19).convert("P"), transparency=0), "tRNS"),
        ("APNG", saved(Image.fromarray(grey), save_all=True, append_images=[Image.fromarray(grey[::-1].copy())]), "acTL"),
    ]


def test_every_unsupported_reason_on_streams_pillow_opens():
    from PIL import Image
    codes = set()
    for name, data, word in _unsupported_streams():
        im = Image.open(io.BytesIO(data))
        im.load()                                               # Pillow opens and decodes it
        info = dp.probe(data)
        assert (info["width"], info["height"]) == im.size, name
        assert not info["supported"] and word in info["reason"] and info["reason_code"] != 0, (name, info["reason"])
        assert info["reason"] == dp.REASONS[info["reason_code"]]
        codes.add(info["reason_code"])
    assert codes == {dp.LOW_DEPTH, dp.COLOUR, dp.INTERLACE, dp.TRNS, dp.APNG}
    np.testing.assert_array_equal(rp.pillow(rp.write_interlaced(np.arange(120, dtype=np.uint8).reshape(12, 10))),
                                  np.arange(120, dtype=np.uint8).reshape(12, 10))


def _probe_or_error(data):
    """probe's verdict, or "error" for DspnError; any other exception escapes and fails the test"""
    try:
        return dp.probe(data)
    except _lib.DspnError:
        return "error"


def test_malformed_streams_raise_dspn_error():
    g = np.random.Generator(np.random.PCG64(9))
    good = rp.write(rp.random_image(g, 5, 6, 1), [0, 1, 2, 3, 4])
    for kind in (b"IHDR", b"PLTE", b"IDAT", b"IEND"):           # a flipped bit in every critical chunk
        data = rp.write(rp.random_image(g, 5, 6, 1), [4] * 5, palette=True)
        at = data.index(kind) + 4 + (0 if kind == b"IEND" else 1)
        bad = data[:at] + bytes([data[at] ^ 0x10]) + data[at + 1:]
        with pytest.raises(_lib.DspnError, match="CRC"):
            dp.probe(bad)
    anc = good[:33] + rp.chunk(b"teXt", b"k\0v")[:-1] + b"\0" + good[33:]      # a bad CRC on an ancillary chunk is not checked
    assert dp.probe(anc)["supported"]
    with pytest.raises(_lib.DspnError, match="signature"):
        dp.probe(b"\x89PNX" + good[4:])
    with pytest.raises(_lib.DspnError, match="IHDR"):
        dp.probe(good[:8] + good[33:])
    with pytest.raises(_lib.DspnError, match="IDAT"):
        dp.probe(good[:33] + rp.chunk(b"IEND"))
    with pytest.raises(_lib.DspnError, match="IEND"):
        dp.probe(good[:-12])
    with pytest.raises(_lib.DspnError, match="past the end"):
        dp.probe(good[:33] + struct.pack(">I", 1 << 20) + good[37:])
    for w, h in ((0, 5), (5, 0)):
        ihdr = rp.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
        with pytest.raises(_lib.DspnError, match="zero width or height"):
            dp.probe(good[:8] + ihdr + good[33:])


def test_truncation_at_every_byte():
    """of two small streams: probe says DspnError for every proper prefix (IEND is the last chunk), nothing else escapes"""
    g = np.random.Generator(np.random.PCG64(10))
    for data in (rp.write(rp.random_image(g, 4, 5, 1), [1, 2, 3, 4], idat_chunks=2),
                 rp.write(rp.random_image(g, 3, 2, 2), [4, 3, 0], idat_chunks=1)):
        assert dp.probe(data)["supported"]
        for n in range(len(data)):
            assert _probe_or_error(data[:n]) == "error", n


def test_inflate_into_returns_a_status():
    g = np.random.Generator(np.random.PCG64(11))
    arr = rp.random_image(g, 6, 7, 1)
    rows, bpp = rp.stream_rows(arr)
    raw = rp.filter_rows(rows, [0, 1, 2, 3, 4, 0], bpp)

    def status(data, info=None):
        info = info or dp.probe(data)
        assert info["supported"] and info["raw_bytes"] == len(raw)
        buf = np.full(info["raw_bytes"] + 32, 0xA5, np.uint8)
        rc = dp.inflate_into(data, info, buf[16:-16])
        assert (buf[:16] == 0xA5).all() and (buf[-16:] == 0xA5).all(), "a guard byte was written"
        return rc

    assert status(rp.assemble(7, 6, 8, 0, raw)) == 0
    five = bytearray(raw)
    five[3 * 8] = 5
    assert status(rp.assemble(7, 6, 8, 0, bytes(five))) == dp.INFLATE_FILTER
    assert status(rp.assemble(7, 6, 8, 0, raw[:-1])) == dp.INFLATE_LENGTH
    assert status(rp.assemble(7, 6, 8, 0, raw + b"\0")) == dp.INFLATE_LENGTH
    assert status(rp.assemble(7, 6, 8, 0, raw + bytes(100000))) == dp.INFLATE_LENGTH
    z = zlib.compress(raw)
    assert status(rp.assemble(7, 6, 8, 0, None, compressed=z[:2] + bytes([z[2] ^ 0xff]) + z[3:])) != 0   # a spoiled deflate block
    assert status(rp.assemble(7, 6, 8, 0, None, compressed=b"\x00\x01" + z[2:])) == dp.INFLATE_ZLIB        # not a zlib header
    # the deflate data cut at every byte: the chunks stay well-formed, so probe is content and the inflate has to say no
    for n in range(len(z)):
        assert status(rp.assemble(7, 6, 8, 0, None, compressed=z[:n] or b"", idat_chunks=1)) != 0, n


def test_device_png_refuses_the_decoded_cache(tmp_path):
    """the refusal comes before any file is opened or any device touched"""
    with pytest.raises(ValueError, match="device_png=True with cache_decoded=True"):
        it.MultiTaskRecordIter(str(tmp_path / "none.rec"), 4, (3, 64, 128), device_png=True, cache_decoded=True)
    assert "device_png" in it.MultiTaskRecordIter.__init__.__code__.co_varnames
