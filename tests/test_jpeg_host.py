"""Host half of the JPEG decode (include/dspn_jpeg.h): dspn_jpeg_probe and dspn_jpeg_entropy_decode against an independent
numpy reading of the stream (tests/ref_jpeg.py), which is itself pinned to Pillow's pixels byte for byte.  No GPU."""
import functools
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import ref_jpeg
from dspnet_amd import _lib
from dspnet_amd.dataset import jpeg as dj

GUARD = 64                                                     # int16 guard words on each side of a coefficient buffer
GUARD_WORD = 0x5A5A


@functools.lru_cache(maxsize=None)
def _reference(name):
    """ref_jpeg's reading of a case, computed once and shared by the tests below (treated as read-only)"""
    return ref_jpeg.decode(jc.stream(name))


def _decode_guarded(data, info):
    n = int(info["coef_count"])
    buf = np.full(n + 2 * GUARD, GUARD_WORD, np.int16)
    rc = dj.entropy_decode(data, info, buf[GUARD:GUARD + n])
    assert (buf[:GUARD] == GUARD_WORD).all() and (buf[GUARD + n:] == GUARD_WORD).all(), "guard words overwritten"
    return rc, buf[GUARD:GUARD + n]


@pytest.mark.parametrize("prefix", jc.GROUPS)
def test_reference_equals_pillow(prefix):
    """the yardstick itself: ref_jpeg's pixels == Pillow's (libjpeg-turbo, accurate IDCT, fancy upsampling)"""
    for name in jc.group(prefix):
        np.testing.assert_array_equal(_reference(name)[2], jc.pillow_pixels(jc.stream(name)), err_msg=name)


@pytest.mark.parametrize("prefix", jc.GROUPS)
def test_probe_fields_equal_reference_parse(prefix):
    for name in jc.group(prefix):
        P = _reference(name)[0]
        info = dj.probe(jc.stream(name))
        nc = P["ncomp"]
        assert info["supported"] and info["reason"] == "ok", name
        assert (info["width"], info["height"], info["ncomp"]) == (P["width"], P["height"], nc), name
        assert info["restart_interval"] == P["restart_interval"], name
        for key in ("hsamp", "vsamp", "blocks_w", "blocks_h"):
            assert info[key][:nc].tolist() == P[key], (name, key)
        blocks = [P["blocks_w"][c] * P["blocks_h"][c] for c in range(nc)]
        assert info["coef_count"] == 64 * sum(blocks), name
        assert info["coef_offset"][:nc].tolist() == [64 * sum(blocks[:c]) for c in range(nc)], name
        for c in range(nc):
            np.testing.assert_array_equal(info["quant"][c], P["quant"][c], err_msg=name)


@pytest.mark.parametrize("prefix", jc.GROUPS)
def test_entropy_decode_equals_reference_coefficients(prefix):
    for name in jc.group(prefix):
        P, planes, _ = _reference(name)
        data = jc.stream(name)
        rc, info = dj.probe_info(data)
        assert rc == 0
        rc, coefs = _decode_guarded(data, info)
        assert rc == 0, (name, _lib.lib().dspn_last_error())
        for c in range(P["ncomp"]):
            o = int(info["coef_offset"][c])
            np.testing.assert_array_equal(coefs[o:o + planes[c].size], planes[c].reshape(-1), err_msg="%s component %d" % (name, c))


def test_restart_cases_carry_restart_intervals():
    """the restart streams of the matrix do exercise DRI / RSTn"""
    names = [n for n in (c[0] for c in jc.CASES) if "rst" in n]
    assert len(names) >= 12
    for name in names:
        assert dj.probe(jc.stream(name))["restart_interval"] > 0, name
    assert dj.probe(jc.stream("16x16-ss2-rstblocks1"))["restart_interval"] == 1


def test_unsupported_streams_have_distinct_reasons():
    rgb = jc.image(3, 40, 56, "smooth")
    progressive = jc.encode(rgb, quality=90, progressive=True)
    buf = io.BytesIO()
    Image.fromarray(np.dstack([rgb, rgb[:, :, 0]]), "CMYK").save(buf, format="JPEG", quality=90)
    cmyk = buf.getvalue()
    base = bytearray(jc.encode(rgb, quality=90))
    sof = base.find(b"\xff\xc0")
    assert sof > 0 and base[sof + 4] == 8
    base[sof + 4] = 12                                          # the frame's sample precision
    infos = [dj.probe(progressive), dj.probe(cmyk), dj.probe(bytes(base))]
    assert [i["supported"] for i in infos] == [False, False, False]
    assert [i["reason_code"] for i in infos] == [1, 6, 5]       # DSPN_JPEG_PROGRESSIVE, _COMPONENTS, _PRECISION
    assert len({i["reason"] for i in infos}) == 3
    for i in infos:                                             # the sizes are known all the same
        assert (i["height"], i["width"]) == (40, 56)
    assert infos[1]["ncomp"] == 4


def _must_fail(data):
    """probe or entropy decode refuses `data` with a message; the guard words of the buffer probe sized stay intact"""
    lib = _lib.lib()
    rc, info = dj.probe_info(data)
    if rc == 0:
        assert info["supported"]
        rc, _ = _decode_guarded(data, info)
    assert rc != 0
    assert len(lib.dspn_last_error()) > 5
    return lib.dspn_last_error()


def test_truncated_streams_are_errors():
    data = jc.stream("37x53-ss2-q90-std-noise")
    scan = ref_jpeg.parse(data)["scan_pos"]
    assert _decode_guarded(data, dj.probe_info(data)[1])[0] == 0
    g = np.random.Generator(np.random.PCG64(40))
    # the byte in front of EOI is the last one with scan bits in it: every shorter prefix has lost data
    cuts = sorted(set(g.integers(0, scan, 20).tolist()) | set(g.integers(scan, len(data) - 3, 20).tolist())
                  | {0, 1, 2, scan - 1, scan, len(data) - 3})
    assert len(cuts) >= 40
    for cut in cuts:
        _must_fail(data[:cut])
    assert b"jpeg" in _must_fail(b"")                           # zero-length input


def test_corrupt_scans_are_errors():
    """seeded byte flips inside the scan: a decoder that lost its place runs into a missing code, a coefficient index
    past 63, a marker inside a block, or does not end at the marker that closes the scan"""
    data = jc.stream("64x200-ss2-q90-std-noise")
    scan = ref_jpeg.parse(data)["scan_pos"]
    g = np.random.Generator(np.random.PCG64(41))
    for trial in range(12):
        bad = bytearray(data)
        for at in g.integers(scan, len(data) - 2, 8):
            bad[at] ^= 0xFF
        _must_fail(bytes(bad))
    # a restart stream whose markers are renumbered
    rst = bytearray(jc.stream("37x53-ss2-rstblocks3"))
    at = rst.find(b"\xff\xd1", ref_jpeg.parse(bytes(rst))["scan_pos"])
    assert at > 0
    rst[at + 1] = 0xD3
    assert b"restart marker" in _must_fail(bytes(rst))


def test_header_references_out_of_range_are_errors():
    data = bytearray(jc.stream("16x16-ss0-q90-std-smooth"))
    sos = data.find(b"\xff\xda")
    bad = bytearray(data)
    bad[sos + 6] = 0x33                                         # first component: DC table 3, AC table 3 (never defined)
    assert b"Huffman table" in _must_fail(bytes(bad))
    sof = data.find(b"\xff\xc0")
    bad = bytearray(data)
    bad[sof + 12] = 3                                           # first component: quantisation table 3 (never defined)
    assert b"quantisation table" in _must_fail(bytes(bad))


def test_entropy_decode_refuses_another_streams_info():
    a, b = jc.stream("16x16-ss0-q90-std-smooth"), jc.stream("17x33-ss0-q90-std-smooth")
    info = dj.probe_info(b)[1]
    buf = np.zeros(int(info["coef_count"]), np.int16)
    assert dj.entropy_decode(a, info, buf) != 0 and b"does not describe" in _lib.lib().dspn_last_error()
