"""Host half of the JPEG encode (include/dspn_jpeg_encode.h): dspn_jpeg_quant_tables against the tables of Pillow's
streams, and dspn_jpeg_entropy_encode against Pillow's files byte for byte -- the coefficients of a Pillow stream, read
back with the decoder's host half and cut to the real block grids, must come out as the very file they were read from.
That pins markers, Huffman coding, byte stuffing, padding bits and the dummy blocks.  No GPU."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import jpeg_encode_cases as ec
import ref_jpeg
from dspnet_amd import _lib
from dspnet_amd.dataset import jpeg_encode as je

GUARD = 64


def test_quant_tables_equal_pillows_for_every_quality():
    grey = jc.image(5, 8, 8, "smooth", 1)
    rgb = jc.image(6, 8, 8, "smooth", 3)
    for q in range(1, 101):
        lum, chrom = je.quant_tables(q)
        assert lum.dtype == np.uint8 and lum.shape == (64,) and chrom.shape == (64,)
        data = jc.encode(rgb, quality=q)
        P = ref_jpeg.parse(data)                                # natural order, read from the DQT segments
        np.testing.assert_array_equal(lum, P["quant"][0], err_msg="quality %d" % q)
        np.testing.assert_array_equal(chrom, P["quant"][1], err_msg="quality %d" % q)
        np.testing.assert_array_equal(chrom, P["quant"][2], err_msg="quality %d" % q)
        tables = Image.open(io.BytesIO(data)).quantization      # Pillow's own reading: the same values in its order
        assert sorted(tables) == [0, 1]
        assert sorted(tables[0]) == sorted(lum.tolist()) and sorted(tables[1]) == sorted(chrom.tolist()), q
        assert list(tables[0]) in (lum.tolist(), lum[ref_jpeg.ZIGZAG].tolist()), q
        assert list(tables[1]) in (chrom.tolist(), chrom[ref_jpeg.ZIGZAG].tolist()), q
        tables = Image.open(io.BytesIO(jc.encode(grey, quality=q))).quantization
        assert sorted(tables) == [0] and list(tables[0]) in (lum.tolist(), lum[ref_jpeg.ZIGZAG].tolist()), q


@pytest.mark.parametrize("size", ec.SIZES, ids=lambda s: "%dx%d" % s)
def test_entropy_round_trip_equals_pillows_file(size):
    cases = [c for c in ec.CASES if (c[0], c[1]) == size]
    assert len(cases) == 16
    for case in cases:
        want = ec.pillow_file(case)
        s, n = ec.sample_of(case)
        coefs = ec.pillow_real_blocks(case)
        assert coefs.size == n
        got = je.entropy_encode(coefs, s, capacity=len(want))
        assert got == want, ec.name(case)
        assert je.entropy_encode(coefs, s, capacity=7) == want, ec.name(case)     # a short first guess is repeated


def test_the_24x40_case_has_dummy_luma_blocks():
    """at 4:2:0 the MCU grid of 24 x 40 holds 4 x 6 luma blocks, the real grid 3 x 5: a dummy row and a dummy column"""
    case = (24, 40, "4:2:0", 95, "noise")
    s, _ = ec.sample_of(case)
    assert (int(s["blocks_h"][0]), int(s["blocks_w"][0])) == (3, 5)
    P = ref_jpeg.parse(ec.pillow_file(case))
    assert (P["blocks_h"][0], P["blocks_w"][0]) == (4, 6)
    assert [int(v) for v in s["blocks_h"][1:]] == P["blocks_h"][1:] and [int(v) for v in s["blocks_w"][1:]] == P["blocks_w"][1:]


def _raw_call(coefs, s, cap, guard=GUARD):
    """one dspn_jpeg_entropy_encode into a buffer of `cap` bytes with guard bytes behind it -> (status, length, buffer)"""
    buf = np.full(cap + guard, 0xA5, np.uint8)
    rec = np.array([s], je.SAMPLE)
    n = ctypes.c_size_t(0)
    rc = _lib.lib().dspn_jpeg_entropy_encode(coefs.ctypes.data, rec.ctypes.data, buf.ctypes.data, cap, ctypes.byref(n))
    return rc, n.value, buf


def test_capacity_one_byte_short_is_refused_and_guards_stay():
    for case in [(24, 40, "4:2:0", 95, "noise"), (1, 1, "grey", 30, "smooth"), (64, 200, "4:4:4", 95, "noise")]:
        want = ec.pillow_file(case)
        s, _ = ec.sample_of(case)
        coefs = ec.pillow_real_blocks(case)
        rc, n, buf = _raw_call(coefs, s, len(want))
        assert rc == 0 and n == len(want) and buf[:n].tobytes() == want and (buf[n:] == 0xA5).all()
        rc, n, buf = _raw_call(coefs, s, len(want) - 1)
        assert rc == -2 and n == len(want), "the status names the needed size through *length"
        assert ("needs %d bytes" % len(want)).encode() in _lib.lib().dspn_last_error()
        assert (buf[len(want) - 1:] == 0xA5).all(), "written past the capacity"
        assert buf[:len(want) - 1].tobytes() == want[:-1]
        rc, n, buf = _raw_call(coefs, s, 0)
        assert rc == -2 and n == len(want) and (buf == 0xA5).all()


def test_argument_checks():
    lib = _lib.lib()
    lum, chrom = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    for q in (0, 101, -5):
        assert lib.dspn_jpeg_quant_tables(q, lum.ctypes.data, chrom.ctypes.data) == -1
        assert b"quality" in lib.dspn_last_error()
        with pytest.raises(_lib.DspnError, match="quality"):
            je.quant_tables(q)
    assert lib.dspn_jpeg_quant_tables(50, None, chrom.ctypes.data) == -1 and b"null" in lib.dspn_last_error()
    assert lib.dspn_jpeg_quant_tables(50, lum.ctypes.data, None) == -1 and b"null" in lib.dspn_last_error()

    case = (16, 16, "4:2:0", 95, "smooth")
    good, _ = ec.sample_of(case)
    coefs = ec.pillow_real_blocks(case)
    out = np.zeros(4096, np.uint8)
    n = ctypes.c_size_t(0)

    def call(s, coefs_p=coefs.ctypes.data, out_p=out.ctypes.data, n_p=ctypes.byref(n), rec=True):
        r = np.array([s], je.SAMPLE)
        return lib.dspn_jpeg_entropy_encode(coefs_p, r.ctypes.data if rec else None, out_p, out.size, n_p)

    assert call(good) == 0
    for kw in (dict(coefs_p=None), dict(out_p=None), dict(n_p=None), dict(rec=False)):
        assert call(good, **kw) == -1 and b"null" in lib.dspn_last_error(), kw
    for field, value, text in (("width", 0, b"image of"), ("height", 0, b"image of"), ("width", 70000, b"image of"),
                               ("ncomp", 2, b"components"), ("hsamp", 3, b"sampling"), ("vsamp", 0, b"sampling")):
        bad = np.array([good], je.SAMPLE)
        bad[field][0] = value
        assert call(bad[0]) == -1 and text in lib.dspn_last_error(), field
    bad = np.array([good], je.SAMPLE)
    bad["blocks_w"][0, 0] += 1
    assert call(bad[0]) == -1 and b"real grid" in lib.dspn_last_error()
    bad = np.array([good], je.SAMPLE)
    bad["coef_offset"][0, 1] += 1
    assert call(bad[0]) == -1 and b"multiple of 64" in lib.dspn_last_error()
    bad = np.array([good], je.SAMPLE)
    bad["quant"][0, 0, 5] = 0
    assert call(bad[0]) == -1 and b"quantisation table" in lib.dspn_last_error()
    # the geometry query refuses the same sizes, and a coefficient base that is not a whole block
    cnt = ctypes.c_longlong(0)
    for field, value in (("width", 0), ("height", 0), ("ncomp", 4), ("hsamp", 4)):
        bad = np.array([good], je.SAMPLE)
        bad[field][0] = value
        assert lib.dspn_jpeg_encode_geometry(bad.ctypes.data, 0, ctypes.byref(cnt)) == -1 and len(lib.dspn_last_error()) > 5
    rec = np.array([good], je.SAMPLE)
    assert lib.dspn_jpeg_encode_geometry(rec.ctypes.data, 32, ctypes.byref(cnt)) == -1
    assert lib.dspn_jpeg_encode_geometry(None, 0, ctypes.byref(cnt)) == -1 and b"null" in lib.dspn_last_error()
    assert lib.dspn_jpeg_encode_geometry(rec.ctypes.data, 128, ctypes.byref(cnt)) == 0 and cnt.value == 64 * 6
    assert rec[0]["coef_offset"].tolist() == [128, 128 + 256, 128 + 320]
    assert lib.dspn_jpeg_encode_workspace_bytes(640) >= 640 and lib.dspn_jpeg_encode_workspace_bytes(0) == 0


def test_coefficients_baseline_coding_cannot_carry_are_errors():
    case = (8, 8, "grey", 95, "smooth")
    s, n = ec.sample_of(case)
    coefs = np.zeros(n, np.int16)
    coefs[0] = 2047
    assert len(je.entropy_encode(coefs, s)) > 100
    coefs[0] = 2048                                             # a DC difference of 12 bits
    with pytest.raises(_lib.DspnError, match="DC difference"):
        je.entropy_encode(coefs, s)
    coefs[0], coefs[9] = 0, -1024                               # an AC value of 11 bits
    with pytest.raises(_lib.DspnError, match="AC coefficient"):
        je.entropy_encode(coefs, s)
