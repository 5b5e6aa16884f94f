"""The PNG encode without a GPU: the filter rule of include/dspn_png_encode.h, restated in tests/ref_png_encode.py, against the
stream inside Pillow's own files; the argument checks of the C entry point (they return before any HIP call, so stand-in
pointers do); the size query; the front end's refusals; and the host half (deflate and chunks) around a reference stream."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_png  # noqa: E402
import ref_png_encode as ref  # noqa: E402

from dspnet_amd import _lib  # noqa: E402
from dspnet_amd.dataset import png  # noqa: E402
from dspnet_amd.dataset import png_encode as pe  # noqa: E402

pytest.importorskip("PIL.Image")
CASES = ref.cases()


@pytest.mark.parametrize("name,a", CASES, ids=[n for n, _ in CASES])
def test_rule_equals_pillow(name, a):
    got, want = ref.filter_image(a), ref.pillow_filtered(a)
    assert ref.filter_types(got, a) == ref.filter_types(want, a)
    assert got == want


def test_case_list_reaches_every_filter_and_the_ties():
    names = [n for n, _ in CASES]
    assert len(set(names)) == len(names)
    taken = {}
    for name, a in CASES:
        taken[name] = ref.filter_types(ref.pillow_filtered(a), a)
    assert {t for types in taken.values() for t in types} == {0, 1, 2, 4}      # Average is never written
    for name, ft in ref.TIE_TYPES.items():
        assert taken[name][1] == ft
    for name, types in taken.items():
        if name.startswith("zeros_"):
            assert set(types) == {0}
        if name.startswith("h1_"):
            assert set(types) <= {0, 1}
        assert types[0] in (0, 1)                                               # the first row never takes Up or Paeth
    assert 0 in taken["noise_L"] and 2 in taken["repeated_rows_L"] and 1 in taken["hramp_L"] and 4 in taken["dramp_L"]
    assert max(a.shape[1] * (a.itemsize if a.ndim == 2 else 3) for _, a in CASES) > ref.STAGE


def sample_table(**kw):
    s = np.zeros(1, pe.SAMPLE)
    base = dict(src_offset=0, out_offset=0, width=5, height=7, bytes_per_pixel=3, src_pitch=15)
    base.update(kw)
    for k, v in base.items():
        s[k] = v
    return s


def test_argument_validation_without_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)                # never dereferenced: every call below fails its checks first

    def call(n=1, src=p, src_bytes=105, out=p, out_bytes=112, ws=p, ws_bytes=64, samples=None, **kw):
        s = sample_table(**kw)
        rc = lib.dspn_png_filter_batch(s.ctypes.data if samples is None else samples, n, src, src_bytes, out, out_bytes, ws, ws_bytes, None)
        return rc, lib.dspn_last_error()

    assert call(n=-1) == (-1, b"png_filter: negative count (n -1)")
    assert call(n=0)[0] == 0                                                    # a no-op, before anything is looked at
    for kw in (dict(src=None), dict(out=None), dict(ws=None), dict(samples=ctypes.c_void_p(0))):
        rc, text = call(**kw)
        assert rc == -1 and b"null argument" in text
    for kw in (dict(src_bytes=0), dict(out_bytes=0), dict(src_bytes=-5)):
        rc, text = call(**kw)
        assert rc == -1 and b"empty pool" in text
    for bpp in (0, 4, -1, 8):
        rc, text = call(bytes_per_pixel=bpp)
        assert rc == -1 and b"bytes_per_pixel is 1, 2 or 3, got %d" % bpp in text
    for kw in (dict(width=0), dict(height=0), dict(width=-3), dict(width=(1 << 24) // 3 + 1, src_pitch=1 << 25)):
        rc, text = call(**kw)
        assert rc == -1 and b"sizes from 1" in text
    rc, text = call(src_pitch=14)
    assert rc == -1 and b"a pitch of 14 bytes for rows of 15" in text
    for kw in (dict(src_bytes=104), dict(src_offset=1), dict(src_offset=-1), dict(src_pitch=16), dict(src_offset=1 << 62)):
        rc, text = call(**kw)
        assert rc == -1 and b"run past src_bytes" in text, kw
    for kw in (dict(out_bytes=111), dict(out_offset=1), dict(out_offset=-1), dict(out_offset=(1 << 63) - 1)):
        rc, text = call(**kw)
        assert rc == -1 and b"run past out_bytes" in text, kw
    rc, text = call(ws_bytes=39)
    assert rc == -2 and b"workspace of 39 bytes, 40 needed" in text
    rc, text = call(ws=ctypes.c_void_p(260))
    assert rc == -1 and b"8-byte aligned" in text
    # the second image of a table is checked like the first
    two = np.concatenate([sample_table(), sample_table(bytes_per_pixel=5)])
    assert lib.dspn_png_filter_batch(two.ctypes.data, 2, p, 105, p, 112, p, 128, None) == -1
    assert b"image 1: bytes_per_pixel" in lib.dspn_last_error()
    # 2^31 rows in one batch do not fit the row table
    tall = np.concatenate([sample_table(width=1, height=(1 << 30), bytes_per_pixel=1, src_pitch=1)] * 2)
    assert lib.dspn_png_filter_batch(tall.ctypes.data, 2, p, 1 << 40, p, 1 << 40, p, 128, None) == -1
    assert b"2^31 - 1 rows" in lib.dspn_last_error()


def test_size_queries():
    lib = _lib.lib()
    assert pe.filtered_bytes(5, 7, 3) == 7 * 16 and pe.filtered_bytes(1, 1, 1) == 2 and pe.filtered_bytes(2048, 1024, 1) == 1024 * 2049
    assert pe.filtered_bytes(4096, 2048, 3) == 2048 * 12289 and pe.filtered_bytes(33, 2, 2) == 2 * 67
    for bad in ((0, 7, 1), (5, 0, 1), (-1, 7, 1), (5, 7, 0), (5, 7, 4), (1 << 24, 1, 1), (1 << 23, 1, 2)):
        assert pe.filtered_bytes(*bad) == 0, bad
    assert pe.filtered_bytes((1 << 24) - 1, (1 << 31) - 1, 1) == ((1 << 31) - 1) * (1 << 24)           # no 32-bit product
    assert lib.dspn_png_filter_workspace_bytes(0) == 0 and lib.dspn_png_filter_workspace_bytes(-3) == 0
    assert lib.dspn_png_filter_workspace_bytes(1) == 40 and lib.dspn_png_filter_workspace_bytes(2) == 80
    assert lib.dspn_png_filter_workspace_bytes(32) == 32 * 36 + 8


@pytest.mark.parametrize("entry", [pe.encode_batch, pe.filter_batch])
def test_front_end_refusals(entry):
    import torch
    ok = np.zeros((3, 4), np.uint8)
    for bad, text in ((np.zeros((4, 4), np.float32), r"float32 \(4, 4\)"), (np.zeros((4, 4, 4), np.uint8), r"uint8 \(4, 4, 4\)"),
                      (np.zeros((0, 4), np.uint8), r"uint8 \(0, 4\)"), (np.zeros((4, 0, 3), np.uint8), r"uint8 \(4, 0, 3\)"),
                      (np.zeros((4, 4, 3), np.uint16), r"uint16 \(4, 4, 3\)"), (torch.zeros(4, 4), r"float32 \(4, 4\)"),
                      (torch.zeros(4, dtype=torch.uint8), r"uint8 \(4,\)"), (torch.zeros(2, 2, dtype=torch.int16), r"int16 \(2, 2\)"),
                      ([[1, 2], [3, 4]], r"list \(\)")):
        with pytest.raises(_lib.DspnError, match="image 1: .*got " + text):       # refused before anything is uploaded
            entry([ok, bad])
    assert entry([]) == []


@pytest.mark.parametrize("name", ["rb65_L", "rb66_I16", "rb69_RGB", "1x1_I16", "noise_RGB"])
def test_host_half_writes_a_strict_file(name):
    """deflate and chunks around a reference stream: exactly IHDR, IDAT, IEND with good CRCs, and Pillow reads the pixels back"""
    from PIL import Image
    a = dict(CASES)[name]
    rows, bpp = ref.stream_rows(a)
    payload = pe.assemble(ref.filter_image(a), a.shape[1], a.shape[0], bpp)
    assert [k for k, _ in ref_png.chunks(payload)] == [b"IHDR", b"IDAT", b"IEND"]
    assert payload[:8] == png.SIGNATURE and payload[-12:] == ref_png.chunk(b"IEND")
    assert b"".join([payload[:8]] + [ref_png.chunk(k, d) for k, d in ref_png.chunks(payload)]) == payload      # every CRC
    assert ref.idat(payload) == ref.filter_image(a)
    im = Image.open(io.BytesIO(payload))
    assert im.mode == {1: "L", 2: "I;16", 3: "RGB"}[bpp] and im.size == (a.shape[1], a.shape[0])
    np.testing.assert_array_equal(np.asarray(im), a)
    if bpp != 3:
        info = png.probe(payload)
        assert info["supported"] and info["bytes_per_pixel"] == bpp
        np.testing.assert_array_equal(ref_png.decode(payload), a)
