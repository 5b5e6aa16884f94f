"""Restart intervals on the host (include/dspn_jpeg_encode.h, include/dspn_jpeg.h): the encoder's restart markers against
Pillow's files byte for byte, dspn_jpeg_scan_index against a numpy restatement (tests/ref_jpeg_scan.py) and on damaged
marker sequences, and the device's Huffman decode (csrc/jpeg_huff.h) built for the host against the host entropy pass.
No GPU."""
import ctypes

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_encode_cases as ec
import jpeg_restart_cases as rc
import ref_jpeg_scan
from dspnet_amd import _lib
from dspnet_amd.dataset import jpeg as dj
from dspnet_amd.dataset import jpeg_encode as je

_PILLOW_SS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def _pillow_restart_file(case, **restart):
    layout, q = case[2], case[3]
    kw = {} if layout == "grey" else {"subsampling": _PILLOW_SS[layout]}
    return jc.encode(ec.pixels(case), quality=q, **kw, **restart)


def _mcus(s):
    hs, vs = (int(s["hsamp"]), int(s["vsamp"])) if int(s["ncomp"]) == 3 else (1, 1)
    return je.mcus_per_row(s), (int(s["height"]) + 8 * vs - 1) // (8 * vs)


# ---- encoder ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ec.SIZES, ids=lambda s: "%dx%d" % s)
def test_restart_files_equal_pillows(size):
    """coefficients from Pillow's own file; intervals of 1, 3, one MCU row and more than the image holds (DRI, no marker)"""
    cases = [c for c in ec.CASES if (c[0], c[1]) == size]
    assert len(cases) == 16
    for case in cases:
        s, _ = ec.sample_of(case)
        coefs = ec.pillow_real_blocks(case)
        per_row, rows = _mcus(s)
        for n in sorted({1, 3, per_row, per_row * rows + 5}):
            want = _pillow_restart_file(case, restart_marker_blocks=n)
            assert je.entropy_encode(coefs, s, restart_interval=n) == want, "%s interval %d" % (ec.name(case), n)
        assert _pillow_restart_file(case, restart_marker_rows=1) == je.entropy_encode(coefs, s, restart_interval=per_row)


def test_interval_zero_is_the_old_entry():
    lib = _lib.lib()
    for case in [c for c in ec.CASES if (c[0], c[1]) == (21, 37)]:
        s, _ = ec.sample_of(case)
        coefs = ec.pillow_real_blocks(case)
        want = ec.pillow_file(case)
        rec, out, n = np.array([s], je.SAMPLE), np.empty(len(want) + 8, np.uint8), ctypes.c_size_t(0)
        assert lib.dspn_jpeg_entropy_encode(coefs.ctypes.data, rec.ctypes.data, out.ctypes.data, out.size, ctypes.byref(n)) == 0
        assert out[:n.value].tobytes() == want == je.entropy_encode(coefs, s, restart_interval=0) == je.entropy_encode(coefs, s)


def test_marker_numbers_wrap_after_eight():
    case = (64, 200, "4:2:0", 95, "noise")                      # 13 x 4 MCUs, one per interval: 51 markers
    s, _ = ec.sample_of(case)
    got = je.entropy_encode(ec.pillow_real_blocks(case), s, restart_interval=1)
    assert got == _pillow_restart_file(case, restart_marker_blocks=1)
    a = np.frombuffer(got, np.uint8)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    rst = [int(a[q + 1]) - 0xD0 for q in ff if 0xD0 <= a[q + 1] <= 0xD7]
    assert rst == [k % 8 for k in range(51)]


@pytest.mark.parametrize("layout", ec.LAYOUTS)
def test_noise_at_quality_100_meets_the_padding(layout):
    """uniform noise at quality 100: 0xFF bytes, and so stuffed FF 00, next to the padded bytes in front of the markers"""
    case = (24, 40, layout, 100, "noise")
    s, n = ec.sample_of(case)
    for interval in (1, 3):
        want = _pillow_restart_file(case, restart_marker_blocks=interval)
        assert want.count(b"\xff\x00") >= 8
        info, coefs = jc._coded(want)
        real = np.zeros(n, np.int16)
        for c in range(int(s["ncomp"])):
            pw, ph, bw, bh = int(info["blocks_w"][c]), int(info["blocks_h"][c]), int(s["blocks_w"][c]), int(s["blocks_h"][c])
            plane = coefs[int(info["coef_offset"][c]):][:64 * pw * ph].reshape(ph, pw, 64)
            real[int(s["coef_offset"][c]):][:64 * bw * bh] = plane[:bh, :bw].reshape(-1)
        assert je.entropy_encode(real, s, restart_interval=interval) == want


def test_encode_refuses_an_interval_out_of_range():
    case = ec.CASES[0]
    s, _ = ec.sample_of(case)
    with pytest.raises(_lib.DspnError, match="restart interval"):
        je.entropy_encode(ec.pillow_real_blocks(case), s, restart_interval=65536)


# ---- scan index -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.RESTART_NAMES + rc.EDGE_NAMES)
def test_scan_index_equals_the_restatement(name):
    data = rc.any_stream(name)
    info, scan, seg, _ = rc.indexed(data)
    ref = ref_jpeg_scan.index(data)
    mcus = ref["mcus_w"] * ref["mcus_h"]
    assert dj.scan_segments(info) == int(scan["segments"]) == -(-mcus // ref["interval"]) == seg.size - 1
    np.testing.assert_array_equal(seg, ref["offsets"])
    assert (int(scan["data_offset"]), int(scan["data_bytes"])) == (ref["scan_pos"], int(ref["offsets"][-1]))
    assert (int(scan["restart_interval"]), int(scan["mcus_w"]), int(scan["mcus_h"])) == (ref["interval"], ref["mcus_w"], ref["mcus_h"])
    assert int(scan["first_segment"]) == 0
    nc = int(info["ncomp"])
    assert scan["dc_table"][:nc].tolist() == ref["td"] and scan["ac_table"][:nc].tolist() == ref["ta"]
    for cls, counts, values in ((0, scan["dc_counts"], scan["dc_values"]), (1, scan["ac_counts"], scan["ac_values"])):
        for t in range(4):
            want = ref["tables"].get((cls, t))
            if want is None:
                assert not counts[t].any() and not values[t].any()
            else:
                np.testing.assert_array_equal(counts[t], want[0])
                np.testing.assert_array_equal(values[t][:want[1].size], want[1])
                assert not values[t][want[1].size:].any()


def test_scan_segments_is_zero_without_an_interval():
    info, _ = jc._coded(jc.stream("16x16-ss2-q90-std-noise"))
    assert dj.scan_segments(info) == 0 and not dj.device_entropy_ok(info)


def _marker_positions(data):
    info, scan, seg, _ = rc.indexed(data)
    return [int(scan["data_offset"]) + int(o) - 2 for o in seg[1:-1]]     # the FF of every restart marker


def test_scan_index_accepts_a_fill_byte_and_an_interval_above_the_mcu_count():
    data = jc.stream("64x200-ss2-rstblocks3")
    info, scan, seg, coefs = rc.indexed(data)
    q = _marker_positions(data)[4]
    filled = data[:q] + b"\xff" + data[q:]
    sc2, seg2 = dj.scan_index(filled, info)
    want = seg.astype(np.int64) + (np.arange(seg.size) > 4)
    np.testing.assert_array_equal(seg2, want)
    status, got = rc.host_decode(filled, sc2, seg2)
    assert status == 0
    np.testing.assert_array_equal(got, coefs)
    one = rc.edge_stream("one-segment")
    info1, scan1, seg1, _ = rc.indexed(one)
    assert int(info1["restart_interval"]) == 25 > int(scan1["mcus_w"]) * int(scan1["mcus_h"]) and int(scan1["segments"]) == 1 and seg1.size == 2 and one.count(b"\xff\xdd") == 1


def test_scan_index_rejects_bad_marker_sequences_in_the_entropy_passes_words():
    data = jc.stream("64x200-ss0-rstblocks3")
    info = rc.indexed(data)[0]
    q = _marker_positions(data)
    assert data[q[2]:q[2] + 2] == b"\xff\xd2"
    renumbered = data[:q[2] + 1] + b"\xd5" + data[q[2] + 2:]
    dropped = data[:q[10]] + data[q[10] + 2:]
    for bad, number in ((renumbered, 2), (dropped, 2)):
        with pytest.raises(_lib.DspnError, match="jpeg: missing restart marker %d" % number) as e:
            dj.scan_index(bad, info)
        out = np.zeros(int(info["coef_count"]), np.int16)
        assert dj.entropy_decode(bad, info, out) != 0            # the host pass refuses it too, with the same words
        assert "restart marker %d" % number in _lib.lib().dspn_last_error().decode()
        assert str(e.value).count("missing restart marker") == 1


def test_scan_index_refuses_what_stays_on_the_host():
    plain = jc.stream("16x16-ss2-q90-std-noise")
    with pytest.raises(_lib.DspnError, match="no restart interval"):
        dj.scan_index(plain, jc._coded(plain)[0])
    wide = jc.encode(jc.image(3, 8, 8 * (dj.DEVICE_MAX_INTERVAL + 1), "smooth", 1), quality=30, restart_marker_rows=1)
    info = jc._coded(wide)[0]
    assert int(info["restart_interval"]) == dj.DEVICE_MAX_INTERVAL + 1 and not dj.device_entropy_ok(info)
    with pytest.raises(_lib.DspnError, match="restart interval of %d MCUs" % (dj.DEVICE_MAX_INTERVAL + 1)):
        dj.scan_index(wide, info)
    edge = jc.encode(jc.image(3, 8, 8 * dj.DEVICE_MAX_INTERVAL, "smooth", 1), quality=30, restart_marker_rows=1)
    assert dj.device_entropy_ok(jc._coded(edge)[0]) and int(rc.indexed(edge)[1]["segments"]) == 1


def test_python_constants_are_the_headers():
    import os
    import re
    import dspnet_amd
    text = open(os.path.join(os.path.dirname(dspnet_amd.__file__), "..", "include", "dspn_jpeg.h")).read()
    assert int(re.search(r"#define DSPN_JPEG_DEVICE_MAX_INTERVAL (\d+)", text).group(1)) == dj.DEVICE_MAX_INTERVAL
    assert "#define DSPN_JPEG_STATUS_SEGMENTS ((1 << 27) - 1)" in text and dj.STATUS_SEGMENTS == (1 << 27) - 1
    assert len(re.findall(r"DSPN_JPEG_BAD_\w+ = \d", text)) == len(dj.STATUS_CODES) - 1


# ---- the device's decode, built for the host --------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.RESTART_NAMES + rc.EDGE_NAMES)
def test_shared_decode_equals_the_host_entropy_pass(name):
    data = rc.any_stream(name)
    status, got = rc.host_decode(data)
    assert status == 0
    np.testing.assert_array_equal(got, rc.indexed(data)[3])     # every block written, zeros included: none of the fill left


def test_shared_decode_at_a_stuffed_segment_end():
    data = rc.stuffed_end_stream()
    status, got = rc.host_decode(data)
    assert status == 0
    np.testing.assert_array_equal(got, rc.indexed(data)[3])


def test_shared_decode_reports_the_first_bad_segment_and_stays_inside():
    data = jc.stream(rc.CHECKED_NAMES[1])
    bad, segment = rc.flipped(data, 1)
    info, scan, seg, coefs = rc.indexed(data)
    sc, sg = dj.scan_index(bad, info)
    s = np.zeros(1, dj.SAMPLE)
    n = int(info["coef_count"])
    dj.fill_sample(s[0], info, 64, 0)                           # a guard block on either side of the sample's coefficients
    out = np.full(n + 128, -23131, np.int16)
    status = dj.entropy_decode_segments(np.frombuffer(bad, np.uint8), s[0], sc, sg, out)
    assert dj.status_parts(status) == (1, segment)
    assert (out[:64] == -23131).all() and (out[-64:] == -23131).all()
    short = rc.cut_short(data, 1, 3)
    sc, sg = dj.scan_index(short, info)
    status, _ = rc.host_decode(short, sc, sg)
    code, where = dj.status_parts(status)
    assert code != 0 and where == 1


def test_shared_decode_treats_contradicting_descriptors_as_no_work():
    data = jc.stream("37x53-ss1-rstblocks3")
    info, scan, seg, _ = rc.indexed(data)
    pool = np.frombuffer(data, np.uint8)
    s = np.zeros(1, dj.SAMPLE)
    dj.fill_sample(s[0], info, 0, 0)
    spoils = [("data_bytes", len(data)), ("data_offset", -1), ("first_segment", 1), ("first_segment", -1), ("segments", 3),
              ("restart_interval", 0), ("restart_interval", dj.DEVICE_MAX_INTERVAL + 1), ("mcus_w", 1), ("mcus_h", 9000)]
    for field, value in spoils:
        sc = scan.copy()
        sc[field] = value
        out = np.full(int(info["coef_count"]), -23131, np.int16)
        assert dj.entropy_decode_segments(pool, s[0], sc, np.ascontiguousarray(seg), out) == 0, field
        assert (out == -23131).all(), field
    sc = scan.copy()
    sc["dc_table"][1] = 7
    out = np.full(int(info["coef_count"]), -23131, np.int16)
    assert dj.entropy_decode_segments(pool, s[0], sc, np.ascontiguousarray(seg), out) == 0 and (out == -23131).all()
    # a segment table that runs backwards or past the data, and counts that are no prefix code: status 7, nothing outside
    for spoil in ("backwards", "past", "counts"):
        sc, sg = scan.copy(), seg.copy()
        if spoil == "backwards":
            sg[3] = sg[2] - 1
        elif spoil == "past":
            sg[-1] = int(scan["data_bytes"]) + 1
        else:
            sc["ac_counts"][0][0] = 3
        out = np.full(int(info["coef_count"]) + 64, -23131, np.int16)
        status = dj.entropy_decode_segments(pool, s[0], sc, sg, out)
        assert dj.status_parts(status)[0] == 7, spoil
        assert (out[-64:] == -23131).all()
