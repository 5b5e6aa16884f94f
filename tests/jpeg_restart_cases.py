"""Restart-interval streams for tests/test_jpeg_restart_host.py and tests/test_jpeg_restart_gpu.py: the restart streams of
jpeg_cases.CASES, edge streams made with Pillow in the test run, the host half of each (probe, scan index, host entropy
pass) computed once, the host build of the device's decode, and damaged streams the scan index still accepts."""
import functools

import numpy as np

import jpeg_cases as jc
from dspnet_amd.dataset import jpeg as dj

RESTART_NAMES = [c[0] for c in jc.CASES if "-rst" in c[0]]
assert len(RESTART_NAMES) == 15
CHECKED_NAMES = ["16x16-ss2-rstblocks1", "50x31-grey-rstblocks3"]     # what tools/jpeg_huff_check.cpp is run over


@functools.lru_cache(maxsize=None)
def edge_stream(name):
    """streams CASES does not hold: (height, width), layout and restart settings in the name's table below"""
    (h, w), ch, content, kw = EDGES[name]
    return jc.encode(jc.image(jc.zlib.crc32(name.encode()), h, w, content, ch), **kw)


EDGES = {
    "last-short": ((24, 40), 3, "noise", dict(subsampling=2, quality=90, restart_marker_blocks=4)),     # 6 MCUs: 4 + 2
    "one-segment": ((37, 53), 3, "smooth", dict(subsampling=1, quality=90, restart_marker_blocks=25)),   # 20 MCUs: DRI above the MCU count
    "many-segments": ((40, 72), 1, "noise", dict(quality=90, restart_marker_blocks=2)),                  # 45 MCUs: 23 segments
    "noise-q100": ((33, 47), 3, "noise", dict(subsampling=0, quality=100, restart_marker_blocks=1)),     # stuffed bytes everywhere
    "optimised": ((37, 53), 3, "noise", dict(subsampling=2, quality=90, optimize=True, restart_marker_rows=1)),
}
for _w in (1, 2, 3, 4, 5, 6):
    EDGES["narrow-%d" % _w] = ((18, _w), 3, "noise", dict(subsampling=2, quality=90, restart_marker_blocks=1))
EDGE_NAMES = sorted(EDGES)


def any_stream(name):
    return edge_stream(name) if name in EDGES else jc.stream(name)


def ends_on_stuffed_byte(payload):
    """whether some restart interval's data ends exactly on a stuffed FF 00"""
    info, scan, seg, _ = indexed(payload)
    at = int(scan["data_offset"])
    for i in range(int(scan["segments"]) - 1):
        end = at + int(seg[i + 1]) - 2                          # the marker's FF (no fill bytes in Pillow's streams)
        if payload[end - 2:end] == b"\xff\x00":
            return True
    end = at + int(seg[-1])
    return payload[end - 2:end] == b"\xff\x00"


@functools.lru_cache(maxsize=None)
def stuffed_end_stream():
    """a seeded noise stream at quality 100 one of whose intervals ends on a stuffed byte (searched once, deterministically)"""
    for seed in range(400):
        p = jc.encode(jc.image(seed, 16, 24, "noise", 3), subsampling=0, quality=100, restart_marker_blocks=1)
        if ends_on_stuffed_byte(p):
            return p
    raise AssertionError("no stream whose interval ends on a stuffed byte among the seeds")


@functools.lru_cache(maxsize=None)
def indexed(payload):
    """-> (info, scan record, segment offsets, host entropy pass's coefficients); read-only, once per distinct stream"""
    info, coefs = jc._coded(payload)
    scan, seg = dj.scan_index(payload, info)
    seg.setflags(write=False)
    return info, scan, seg, coefs


def host_decode(payload, scan=None, seg=None):
    """the device's decode built for the host over one stream (the pool is the stream itself) -> (status word, coefficients)"""
    info = indexed(payload)[0] if scan is None else dj.probe_info(payload)[1]
    if scan is None:
        _, scan, seg, _ = indexed(payload)
    s = np.zeros(1, dj.SAMPLE)
    dj.fill_sample(s[0], info, 0, 0)
    out = np.full(int(info["coef_count"]), -23131, np.int16)
    pool = np.frombuffer(payload, np.uint8)
    return dj.entropy_decode_segments(pool, s[0], scan, np.ascontiguousarray(seg), out), out


@functools.lru_cache(maxsize=None)
def flipped(payload, want_code):
    """the first single-bit flip inside the entropy-coded data that the scan index still accepts and that the host build of
    the device's decode rejects with `want_code` -> (damaged stream, bad segment)"""
    info, scan, seg, _ = indexed(payload)
    at, n = int(scan["data_offset"]), int(scan["data_bytes"])
    for pos in range(at, at + n):
        for bit in range(8):
            b = bytearray(payload)
            b[pos] ^= 1 << bit
            b = bytes(b)
            try:
                sc, sg = dj.scan_index(b, info)
            except Exception:                                   # the flip made or broke a marker
                continue
            status, _ = host_decode(b, sc, sg)
            if status and dj.status_parts(status)[0] == want_code:
                return b, dj.status_parts(status)[1]
    raise AssertionError("no single-bit flip gives status code %d" % want_code)


def cut_short(payload, segment, nbytes):
    """`nbytes` bytes of data taken out in front of the marker that ends `segment`: the index (which reads only the 0xFF
    bytes) adjusts the table to match"""
    info, scan, seg, _ = indexed(payload)
    end = int(scan["data_offset"]) + int(seg[segment + 1]) - (2 if segment + 1 < int(scan["segments"]) else 0)
    return payload[:end - nbytes] + payload[end:]
