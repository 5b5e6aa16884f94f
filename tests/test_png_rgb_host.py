"""Host half of the colour PNG decode (dspnet_amd/dataset/png.py: probe_rgb, the descriptor, the workspace query; no GPU):
the numpy reading of tests/ref_png_rgb.py is pinned to Pillow's convert("RGB") over every (colour type, bit depth) pair,
`probe_rgb` names why it will not take a stream, and malformed input ends in DspnError."""
import ctypes
import re
import os

import numpy as np
import pytest

import ref_png as rp
import ref_png_rgb as rr
from dspnet_amd import _lib
from dspnet_amd.dataset import png as dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _streams():
    """(name, payload, colour, depth): every pair at a width that is no multiple of the samples per byte, with and without
    tRNS, every filter type on later rows; palette streams with a 2-entry PLTE under indices beyond it"""
    g = np.random.Generator(np.random.PCG64(4242))
    out = []
    for colour, depth in rr.PAIRS:
        for trns in (False, True):
            for w in (1, 7, 9, 13):
                h = 6
                s = rr.random_samples(g, h, w, colour, depth)
                data = rr.write(s, colour, depth, [0, 1, 2, 3, 4, int(g.integers(0, 5))], trns=trns, idat_chunks=1 + w % 3)
                out.append(("c%d-d%d-w%d%s" % (colour, depth, w, "-trns" if trns else ""), data, colour, depth))
        if colour == 3:
            s = rr.random_samples(g, 5, 11, colour, depth)
            s[0, :2, 0] = (0, 2 ** depth - 1)
            data = rr.write(s, colour, depth, rp.filters_for(g, 5, "mix"), plte_entries=2)
            out.append(("c3-d%d-short-plte" % depth, data, colour, depth))
    return out


STREAMS = _streams()


def test_numpy_reading_equals_pillow_convert_rgb():
    assert len(STREAMS) == 14 * 8 + 4
    for name, data, _, _ in STREAMS:
        want, got = rr.pillow(data), rr.decode(data)
        assert got.dtype == np.uint8 and got.shape == want.shape, name
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_short_plte_gives_black_beyond_it():
    for name, data, _, depth in STREAMS:
        if name.endswith("short-plte") and depth > 1:
            got = rr.pillow(data)
            assert (got[0, 1] == 0).all() and (got[0, 0] == np.frombuffer(rr.default_palette(2), np.uint8)[:3]).all(), name


def test_probe_rgb_supports_every_pair_and_sizes_the_rows():
    for name, data, colour, depth in STREAMS:
        info = dp.probe_rgb(data)
        w, h = info["width"], info["height"]
        rb, bpp = rr.geometry(w, colour, depth)
        assert info["supported"] and info["reason"] == "ok" and info["reason_code"] == dp.RGB_OK, name
        assert (info["bit_depth"], info["colour_type"], info["interlace"]) == (depth, colour, 0), name
        assert info["row_bytes"] == rb and info["bytes_per_pixel"] == bpp and info["raw_bytes"] == h * (rb + 1), name
        assert (info["palette"] is not None) == (colour == 3), name
        assert set(info) == set(dp.probe(data)) | {"palette"}
        buf = np.full(info["raw_bytes"] + 32, 0xA5, np.uint8)
        assert dp.inflate_into(data, info, buf[16:-16]) == 0, name
        assert (buf[:16] == 0xA5).all() and (buf[-16:] == 0xA5).all()
        rows = rp.unfilter(buf[16:-16].tobytes(), h, rb, bpp)
        np.testing.assert_array_equal(rr.to_rgb(rows, w, colour, depth, info["palette"]), rr.pillow(data), err_msg=name)


def test_probe_rgb_names_each_reason():
    g = np.random.Generator(np.random.PCG64(5))
    rgb = rr.random_samples(g, 4, 5, 2, 8)
    good = rr.write(rgb, 2, 8, [0, 1, 2, 3])
    raw = rp.filter_rows(rr.pack_rows(rgb, 8), [0] * 4, 3)
    cases = {
        dp.RGB_GREY16: rp.write(rp.random_image(g, 4, 5, 2), [0] * 4),
        dp.RGB_INTERLACE: rp.write_interlaced(np.zeros((9, 9), np.uint8)),
        dp.RGB_APNG: rp.assemble(5, 4, 8, 2, raw, before_idat=[rp.chunk(b"acTL", b"\0" * 8)]),
        dp.RGB_NONSTANDARD: rp.assemble(5, 4, 4, 2, raw),        # RGB at 4 bits
        dp.RGB_NO_PLTE: rp.SIGNATURE + b"".join(rp.chunk(k, d) for k, d in rp.chunks(rr.write(
            rr.random_samples(g, 4, 5, 3, 8), 3, 8, [0] * 4)) if k != b"PLTE"),
    }
    assert dp.probe_rgb(good)["supported"] and len(cases) == len(dp.RGB_REASONS) - 1
    for code, data in cases.items():
        info = dp.probe_rgb(data)
        assert not info["supported"] and info["reason_code"] == code and info["reason"] == dp.RGB_REASONS[code], code
        assert info["raw_bytes"] == 0 and info["palette"] is None
    assert "greyscale" in dp.RGB_REASONS[dp.RGB_GREY16] and "interlace" in dp.RGB_REASONS[dp.RGB_INTERLACE]
    assert "acTL" in dp.RGB_REASONS[dp.RGB_APNG] and "PLTE" in dp.RGB_REASONS[dp.RGB_NO_PLTE]
    # a PLTE behind IDAT, or one that is not whole entries, is no palette either
    parts = list(rp.chunks(rr.write(rr.random_samples(g, 4, 5, 3, 8), 3, 8, [0] * 4, idat_chunks=1)))
    late = rp.SIGNATURE + b"".join(rp.chunk(k, d) for k, d in (parts[0], parts[2], parts[1], parts[3]))
    assert dp.probe_rgb(late)["reason_code"] == dp.RGB_NO_PLTE
    ragged = rp.SIGNATURE + b"".join(rp.chunk(k, d[:4] if k == b"PLTE" else d) for k, d in parts)
    assert dp.probe_rgb(ragged)["reason_code"] == dp.RGB_NO_PLTE
    # what `probe` says of the same streams is untouched
    assert dp.probe(good)["reason_code"] == dp.COLOUR and dp.probe(cases[dp.RGB_GREY16])["supported"]


def test_probe_rgb_raises_on_malformed_streams():
    good = STREAMS[0][1]
    bad_crc = bytearray(good)
    bad_crc[20] ^= 1                                            # inside IHDR
    no_idat = rp.SIGNATURE + b"".join(rp.chunk(k, d) for k, d in rp.chunks(good) if k != b"IDAT")
    zero = rp.assemble(0, 4, 8, 2, b"")
    for data, text in ((b"", "signature"), (b"\x89PNG\r\n\x1a\r" + good[8:], "signature"), (good[:-12], "IEND"),
                       (good[:40], "past the end"), (bytes(bad_crc), "CRC"), (no_idat, "IDAT"), (zero, "zero width"),
                       (rp.SIGNATURE + rp.chunk(b"IDAT", b"x") + good[8:], "IHDR")):
        with pytest.raises(_lib.DspnError, match=text):
            dp.probe_rgb(data)
        with pytest.raises(_lib.DspnError, match=text):
            dp.probe(data)


def test_inflate_into_statuses_at_packed_row_lengths():
    g = np.random.Generator(np.random.PCG64(6))
    s = rr.random_samples(g, 5, 9, 0, 2)                        # 3 bytes per row
    data = rr.write(s, 0, 2, [0, 1, 2, 3, 4])
    info = dp.probe_rgb(data)
    assert info["row_bytes"] == 3 and info["raw_bytes"] == 20
    raw = bytearray(rp.filter_rows(rr.pack_rows(s, 2), [0] * 5, 1))
    raw[8] = 5                                                  # row 2's filter byte
    buf = np.zeros(20, np.uint8)

    def status(payload):
        return dp.inflate_into(payload, dp.probe_rgb(payload), buf)

    assert status(rp.assemble(9, 5, 2, 0, bytes(raw))) == dp.INFLATE_FILTER
    assert status(rp.assemble(9, 5, 2, 0, bytes(raw[:-1]))) == dp.INFLATE_LENGTH
    assert status(rp.assemble(9, 5, 2, 0, b"", compressed=b"\x78\x9c\xff\xff")) == dp.INFLATE_ZLIB
    assert status(data) == dp.INFLATE_OK


def test_descriptor_layout():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dspn_png.h")).read(), flags=re.S)
    body = re.search(r"typedef struct dspn_png_rgb_sample \{(.*?)\} dspn_png_rgb_sample;", text, re.S).group(1)
    names = [n.strip() for kind, group in re.findall(r"(long long|int)\s+([^;]+);", body) for n in group.split(",")]
    kinds = [kind for kind, group in re.findall(r"(long long|int)\s+([^;]+);", body) for _ in group.split(",")]
    assert tuple(names) == dp.RGB_SAMPLE.names
    assert [dp.RGB_SAMPLE[n].itemsize for n in names] == [8 if k == "long long" else 4 for k in kinds]
    assert [dp.RGB_SAMPLE.fields[n][1] for n in names] == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    assert dp.RGB_SAMPLE.itemsize == 48 and "#define DSPN_PNG_RGB_SAMPLE_BYTES 48" in text
    assert dp.PALETTE_BYTES == 768 and "#define DSPN_PNG_PALETTE_BYTES 768" in text


def _samples(rows):
    s = np.zeros(len(rows), dp.RGB_SAMPLE)
    for d, row in zip(s, rows):
        for k, v in row.items():
            d[k] = v
    return s


def test_workspace_query_is_pure():
    """no HIP call: it runs here; the largest extent of the descriptors that pass through the workspace"""
    rgb8 = dict(width=2048, height=1024, bit_depth=8, colour_type=2, recon_offset=1 << 40)
    assert dp.rgb_workspace_bytes(_samples([rgb8] * 16)) == 0
    assert _lib.lib().dspn_png_rgb_workspace_bytes(None, 4) == 0 and dp.rgb_workspace_bytes(_samples([])) == 0
    rgba16 = dict(width=5, height=7, bit_depth=16, colour_type=6, recon_offset=48)
    grey1 = dict(width=9, height=3, bit_depth=1, colour_type=0, recon_offset=1000)
    assert dp.rgb_workspace_bytes(_samples([rgb8, rgba16])) == 48 + 7 * 40
    assert dp.rgb_workspace_bytes(_samples([grey1, rgba16, rgb8])) == 1000 + 3 * 2
    for bad in (dict(grey1, skip=1), dict(grey1, bit_depth=16), dict(grey1, colour_type=5), dict(grey1, width=0),
                dict(grey1, height=-1), dict(grey1, recon_offset=-8), dict(grey1, bit_depth=3),
                dict(rgba16, width=0x7fffffff, height=0x7fffffff, recon_offset=(1 << 62))):
        assert dp.rgb_workspace_bytes(_samples([bad, rgba16])) == 48 + 7 * 40, bad
    s = _samples([grey1, rgba16])
    before = s.tobytes()
    dp.rgb_workspace_bytes(s)
    assert s.tobytes() == before


def test_rgb_batch_argument_checks_without_gpu():
    """refused before any HIP call"""
    lib = _lib.lib()
    p = ctypes.c_void_p(256)                                    # never dereferenced
    call = lib.dspn_png_rgb_batch
    assert call(p, 64, p, -1, None, 0, p, 64, None, 0, None) == -1 and b"negative" in lib.dspn_last_error()
    assert call(p, 64, p, 1, None, 0, p, 64, None, -1, None) == -1 and b"negative" in lib.dspn_last_error()
    assert call(p, 64, p, 1, None, -1, p, 64, None, 0, None) == -1 and b"negative" in lib.dspn_last_error()
    assert call(None, 64, p, 1, None, 0, p, 64, None, 0, None) == -1 and b"null" in lib.dspn_last_error()
    assert call(p, 64, p, 1, None, 1, p, 64, None, 0, None) == -1 and b"null palettes" in lib.dspn_last_error()
    assert call(p, 64, p, 1, None, 0, p, 64, None, 16, None) == -1 and b"null workspace" in lib.dspn_last_error()
    assert call(p, 64, ctypes.c_void_p(260), 1, None, 0, p, 64, None, 0, None) == -1 and b"aligned" in lib.dspn_last_error()
    assert call(None, 0, None, 0, None, 0, None, 0, None, 0, None) == 0
