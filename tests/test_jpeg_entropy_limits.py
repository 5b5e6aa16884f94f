"""The magnitude sizes the two entropy passes accept (include/dspn_jpeg.h), on hand-assembled streams: the host pass
(dspn_jpeg_entropy_decode) takes AC sizes up to 15, the device's decode (csrc/jpeg_huff.h, here in its host build) refuses
more than 10 with DSPN_JPEG_BAD_SIZE, and both refuse a DC size above 11.  Each stream is one 8 x 8 grey block behind a
one-symbol DC table and a two-symbol AC table, DRI = 1; the expected values are the ones packed.  No GPU."""
import struct

import numpy as np
import pytest

from dspnet_amd import _lib
from dspnet_amd.dataset import jpeg as dj

BAD_SIZE = 3                                                    # DSPN_JPEG_BAD_SIZE


def _natural(k):
    """zigzag position -> row-major index, by walking the diagonals"""
    r = c = 0
    for _ in range(k):
        if (r + c) & 1:
            r, c = (r, c + 1) if r == 7 else ((r + 1, c) if c == 0 else (r + 1, c - 1))
        else:
            r, c = (r + 1, c) if c == 7 else ((r, c + 1) if r == 0 else (r - 1, c + 1))
    return 8 * r + c


def _magnitude(v, size):
    """the `size` bits that follow a symbol for the value v"""
    assert v and abs(v).bit_length() == size
    return format(v if v > 0 else v + (1 << size) - 1, "0%db" % size)


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def _stream(dc_size, dc_value, run, ac_size, ac_value):
    """DC code '0' -> dc_size; AC codes '00' -> (run, ac_size) and '01' -> EOB"""
    bits = "0" + (_magnitude(dc_value, dc_size) if dc_size else "")
    bits += "00" + _magnitude(ac_value, ac_size) + "01"
    bits += "1" * (-len(bits) % 8)
    data = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    counts_dc, counts_ac = bytes([1] + [0] * 15), bytes([0, 2] + [0] * 14)
    return (b"\xff\xd8" + _segment(0xDB, bytes([0]) + bytes([1] * 64)) +
            _segment(0xC0, bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0])) +
            _segment(0xC4, bytes([0x00]) + counts_dc + bytes([dc_size])) +
            _segment(0xC4, bytes([0x10]) + counts_ac + bytes([run << 4 | ac_size, 0x00])) +
            _segment(0xDD, bytes([0, 1])) + _segment(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + data + b"\xff\xd9")


def _host_pass(payload):
    rc, info = dj.probe_info(payload)
    assert rc == 0 and info["supported"] and int(info["coef_count"]) == 64 and int(info["restart_interval"]) == 1
    out = np.full(64, -23131, np.int16)
    return dj.entropy_decode(payload, info, out), out


def _device_pass(payload):
    info = dj.probe_info(payload)[1]
    scan, seg = dj.scan_index(payload, info)
    assert int(scan["segments"]) == 1
    s = np.zeros(1, dj.SAMPLE)
    dj.fill_sample(s[0], info, 0, 0)
    out = np.full(64, -23131, np.int16)
    status = dj.entropy_decode_segments(np.frombuffer(payload, np.uint8), s[0], scan, seg, out)
    return status, out


def _block(run, value):
    want = np.zeros(64, np.int16)
    want[_natural(1 + run)] = value
    return want


@pytest.mark.parametrize("size,value,run", [(11, 1500, 4), (11, -2047, 0), (15, 20000, 9), (15, -32767, 15), (15, 16384, 7)])
def test_ac_sizes_11_to_15_are_the_hosts_alone(size, value, run):
    payload = _stream(0, 0, run, size, value)
    rc, got = _host_pass(payload)
    assert rc == 0
    np.testing.assert_array_equal(got, _block(run, value))
    assert dj.status_parts(_device_pass(payload)[0]) == (BAD_SIZE, 0)


@pytest.mark.parametrize("value,run", [(1023, 4), (-1023, 0), (512, 15), (-700, 7)])
def test_ac_size_10_decodes_on_both(value, run):
    payload = _stream(0, 0, run, 10, value)
    rc, got = _host_pass(payload)
    assert rc == 0
    np.testing.assert_array_equal(got, _block(run, value))
    status, dev = _device_pass(payload)
    assert status == 0
    np.testing.assert_array_equal(dev, got)


@pytest.mark.parametrize("value", [2047, -1024])
def test_dc_size_11_decodes_on_both(value):
    """the control of the next test: the same stream one DC size lower is well formed"""
    payload = _stream(11, value, 0, 1, 1)
    want = _block(0, 1)
    want[0] = value
    rc, got = _host_pass(payload)
    assert rc == 0
    np.testing.assert_array_equal(got, want)
    status, dev = _device_pass(payload)
    assert status == 0
    np.testing.assert_array_equal(dev, want)


@pytest.mark.parametrize("value", [2048, -4095])
def test_dc_size_12_is_refused_by_both(value):
    payload = _stream(12, value, 0, 1, 1)
    rc, _ = _host_pass(payload)
    assert rc != 0 and "DC difference" in _lib.lib().dspn_last_error().decode()
    assert dj.status_parts(_device_pass(payload)[0]) == (BAD_SIZE, 0)
