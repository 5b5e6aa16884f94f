"""Host side of the device entropy pass of the JPEG encode (include/dspn_jpeg_encode.h): dspn_jpeg_encode_headers against the
prefix of dspn_jpeg_entropy_encode_restart's file, the workspace bound, the argument checks that come before any HIP call, and
the old entries' files after the header writer was factored out of them.  No GPU."""
import ctypes

import numpy as np
import pytest

import jpeg_encode_cases as ec
from dspnet_amd import _lib
from dspnet_amd.dataset import jpeg_encode as je

SOS = b"\xff\xda"


def _scan_start(data):
    """index of the first byte of the scan: behind the SOS segment (no marker segment of these files holds FF DA inside)"""
    at = data.index(SOS)
    return at + 2 + int.from_bytes(data[at + 2:at + 4], "big")


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("interval", [0, 8])
def test_headers_equal_the_files_prefix(layout, interval):
    case = (21, 37, layout, 95, "noise")
    s, _ = ec.sample_of(case)
    want = je.entropy_encode(ec.pillow_real_blocks(case), s, restart_interval=interval)
    got = je.headers(s, interval)
    assert got == want[:_scan_start(want)]
    assert (b"\xff\xdd\x00\x04\x00\x08" in got) == (interval == 8)
    assert got[:2] == b"\xff\xd8" and got[-(10 if layout == "grey" else 14):-(8 if layout == "grey" else 12)] == SOS


def test_headers_too_small_at_every_capacity():
    s, _ = ec.sample_of((9, 15, "4:2:0", 30, "noise"))
    rec = np.array([s], je.SAMPLE)
    want = je.headers(s, 3)
    lib = _lib.lib()
    n = ctypes.c_size_t(0)
    for cap in range(len(want) + 1):
        buf = np.full(cap + 16, 0xA5, np.uint8)
        rc = lib.dspn_jpeg_encode_headers(rec.ctypes.data, 3, buf.ctypes.data, cap, ctypes.byref(n))
        assert n.value == len(want)
        assert rc == (0 if cap == len(want) else -2), cap
        if cap < len(want):
            assert b"need" in lib.dspn_last_error()
        assert buf[:cap].tobytes() == want[:cap] and (buf[cap:] == 0xA5).all(), cap


def test_headers_refuse_null_and_bad_arguments():
    s, _ = ec.sample_of((9, 15, "4:2:0", 30, "noise"))
    rec = np.array([s], je.SAMPLE)
    lib = _lib.lib()
    n = ctypes.c_size_t(7)
    buf = np.zeros(1024, np.uint8)
    assert lib.dspn_jpeg_encode_headers(None, 0, buf.ctypes.data, 1024, ctypes.byref(n)) == -1 and b"null" in lib.dspn_last_error()
    assert lib.dspn_jpeg_encode_headers(rec.ctypes.data, 0, buf.ctypes.data, 1024, None) == -1 and b"null" in lib.dspn_last_error()
    assert lib.dspn_jpeg_encode_headers(rec.ctypes.data, 0, None, 1024, ctypes.byref(n)) == -1 and b"null" in lib.dspn_last_error()
    for bad in (-1, 65536):
        assert lib.dspn_jpeg_encode_headers(rec.ctypes.data, bad, buf.ctypes.data, 1024, ctypes.byref(n)) == -1
        assert b"restart interval" in lib.dspn_last_error() and n.value == 0
    rec[0]["blocks_w"][1] += 1
    assert lib.dspn_jpeg_encode_headers(rec.ctypes.data, 0, buf.ctypes.data, 1024, ctypes.byref(n)) == -1
    assert b"real grid" in lib.dspn_last_error()
    assert not buf.any()


def test_workspace_bytes_is_pure_and_covers_its_bound():
    """a 1 x 1 4:2:0 image: 3 real blocks, 6 slots.  The documented bound: 209 bytes of stream per real block and 5 per
    dummy, one flag bit per stream byte, 12 bytes per slot"""
    lib = _lib.lib()
    s, n = ec.sample_of((1, 1, "4:2:0", 95, "noise"))
    assert n == 192
    got = lib.dspn_jpeg_entropy_encode_workspace_bytes(n, 1)
    stream = 3 * 209 + 3 * 5
    assert got >= stream + (stream + 7) // 8 + 12 * 6
    assert got == lib.dspn_jpeg_entropy_encode_workspace_bytes(n, 1)
    assert lib.dspn_jpeg_entropy_encode_workspace_bytes(64 * 2000, 16) > lib.dspn_jpeg_entropy_encode_workspace_bytes(64 * 1000, 16)
    for bad in ((0, 1), (-64, 1), (192, 0), (192, 1025)):
        assert lib.dspn_jpeg_entropy_encode_workspace_bytes(*bad) == 0


def test_batch_calls_check_their_arguments_before_any_hip_call():
    """no device is touched: the pointers are made up and never followed"""
    lib = _lib.lib()
    p = 1 << 20
    ws = lib.dspn_jpeg_entropy_encode_workspace_bytes(192, 1)
    scan, write = lib.dspn_jpeg_entropy_encode_scan_batch, lib.dspn_jpeg_entropy_encode_write_batch
    assert scan(None, 192, p, p, 1, p, p, p, ws, None) == -1 and b"null" in lib.dspn_last_error()
    assert scan(p, 192, p, None, 1, p, p, p, ws, None) == -1 and b"null" in lib.dspn_last_error()
    assert scan(p, 192, p, p, 0, p, p, p, ws, None) == -1 and b"batch" in lib.dspn_last_error()
    assert scan(p, 192, p, p, 1025, p, p, p, ws, None) == -1 and b"batch" in lib.dspn_last_error()
    assert scan(p, 100, p, p, 1, p, p, p, ws, None) == -1 and b"multiple of 64" in lib.dspn_last_error()
    assert scan(p + 2, 192, p, p, 1, p, p, p, ws, None) == -1 and b"aligned" in lib.dspn_last_error()
    assert scan(p, 192, p, p, 1, p, p, p, ws - 1, None) == -2 and b"workspace" in lib.dspn_last_error()
    assert write(192, 1, None, p, 10, p, ws, None) == -1 and b"null" in lib.dspn_last_error()
    assert write(192, 0, p, p, 10, p, ws, None) == -1 and b"batch" in lib.dspn_last_error()
    assert write(192, 1, p, p, 0, p, ws, None) == -1 and b"out_bytes" in lib.dspn_last_error()
    assert write(100, 1, p, p, 10, p, ws, None) == -1 and b"multiple of 64" in lib.dspn_last_error()
    assert write(192, 1, p, p, 10, p + 4, ws, None) == -1 and b"aligned" in lib.dspn_last_error()
    assert write(192, 1, p, p, 10, p, ws - 1, None) == -2 and b"workspace" in lib.dspn_last_error()


def test_encode_batch_refuses_both_restart_settings_before_a_device():
    with pytest.raises(ValueError, match="at most one"):
        je.encode_batch([object()], device_entropy=True, restart_interval=1, restart_rows=1)


def test_the_old_entries_still_write_pillows_files():
    for case in ec.CASES[:8]:
        s, _ = ec.sample_of(case)
        assert je.entropy_encode(ec.pillow_real_blocks(case), s) == ec.pillow_file(case), ec.name(case)
        assert je.entropy_encode(ec.pillow_real_blocks(case), s, restart_interval=0, capacity=5) == ec.pillow_file(case), ec.name(case)
