"""The entropy pass of the JPEG encode on the device (dspn_jpeg_entropy_encode_scan_batch / _write_batch, and
encode_batch(device_entropy=True) on top of them).  The yardstick is the host pass (dspn_jpeg_entropy_encode_restart), itself
pinned to Pillow's files: the scans must be equal byte for byte, nothing is written outside an image's range, and what the
host pass refuses is refused."""
import os
import re

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_encode_cases as ec
import ref_jpeg
from dspnet_amd import _lib
from dspnet_amd.dataset import jpeg_encode as je
from dspnet_amd.dataset import recordio

GUARD = 256


def _scan_of(data):
    """the bytes between the SOS header and EOI of a file"""
    at = data.index(b"\xff\xda")
    assert data[-2:] == b"\xff\xd9"
    return data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):-2]


def _device_scans(coefs, samples, intervals, dev, short=0, stream=None):
    """the two calls over host coefficients and descriptors, 0xA5 around the workspace and around every image's range of
    the output -> (scan_bytes, status, [bytes per image]); `short`: out_bytes ends that many bytes inside the last range.
    Asserts that no guard byte and no byte of an unwritten range changed."""
    import torch
    lib = _lib.lib()
    B = len(samples)
    cdev = torch.from_numpy(np.ascontiguousarray(coefs)).to(dev)
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    ivs = torch.tensor(list(intervals), dtype=torch.int32).to(dev)
    ws_bytes = lib.dspn_jpeg_entropy_encode_workspace_bytes(cdev.numel(), B)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = torch.full((B,), -7, dtype=torch.int64, device=dev)
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
    torch.cuda.synchronize(dev)
    _lib.check(lib.dspn_jpeg_entropy_encode_scan_batch(cdev.data_ptr(), cdev.numel(), desc.data_ptr(), ivs.data_ptr(), B, sizes.data_ptr(),
                                                       status.data_ptr(), ws.data_ptr() + GUARD, ws_bytes, st))
    torch.cuda.synchronize(dev)
    sizes, status = sizes.cpu().numpy(), status.cpu().numpy()
    assert ((status == 0) | (sizes == 0)).all() and (sizes >= 0).all()
    offsets = GUARD + np.concatenate([[0], np.cumsum(sizes + GUARD)])
    out = torch.full((int(offsets[-1]),), 0xA5, dtype=torch.uint8, device=dev)
    off = torch.from_numpy(offsets[:-1].astype(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    _lib.check(lib.dspn_jpeg_entropy_encode_write_batch(cdev.numel(), B, off.data_ptr(), out.data_ptr(), int(offsets[-1]) - GUARD - short,
                                                        ws.data_ptr() + GUARD, ws_bytes, st))
    torch.cuda.synchronize(dev)
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    assert (ws[:GUARD] == 0xA5).all() and (ws[-GUARD:] == 0xA5).all(), "guard bytes of the workspace overwritten"
    covered = np.zeros(out.size, bool)
    scans = []
    for k in range(B):
        a, b = int(offsets[k]), int(offsets[k]) + int(sizes[k])
        if short and k == B - 1:
            scans.append(None)
        else:
            covered[a:b] = True
            scans.append(out[a:b].tobytes())
    assert (out[~covered] == 0xA5).all(), "bytes outside the images' ranges were written"
    return sizes, status, scans


def _host_scan(coefs, sample, interval):
    return _scan_of(je.entropy_encode(coefs, sample, restart_interval=interval))


def _pool(cases, repeat=1):
    """Pillow's coefficients of `cases`, back to back, `repeat` times -> (pool, descriptors)"""
    samples = np.zeros(len(cases) * repeat, je.SAMPLE)
    parts, co = [], 0
    for k in range(len(samples)):
        case = cases[k % len(cases)]
        samples[k], n = ec.sample_of(case, coef_base=co)
        parts.append(ec.pillow_real_blocks(case))
        co += n
    return np.concatenate(parts), samples


def _grey(blocks, width_blocks, coef_base):
    """descriptor of a grey image whose real grid is `blocks` (n, 64) natural-order blocks, width_blocks across"""
    s = np.zeros(1, je.SAMPLE)
    n = je.fill_sample(s[0], 8 * width_blocks, 8 * (len(blocks) // width_blocks), 1, (1, 1), je.quant_tables(90), coef_base, 0)
    assert n == blocks.size
    return s[0]


def _group(cases):
    """encode_batch takes one quality and one chroma layout per call (a grey image goes with any layout)"""
    groups = {}
    for c in cases:
        groups.setdefault(("4:2:0" if c[2] == "grey" else c[2], c[3]), []).append(c)
    return groups


@pytest.mark.gpu
def test_all_cases_equal_pillows_files(gpu_device):
    """the 112 cases (1 x 1 ... 64 x 200: dummy luma blocks in both directions, grey rasters): their Pillow coefficients in
    ONE mixed batch through the two calls, and their pixels through encode_batch per quality and layout"""
    import torch
    cases = ec.CASES
    assert len(cases) == 112
    pool, samples = _pool(cases)
    sizes, status, scans = _device_scans(pool, samples, [0] * len(cases), gpu_device)
    assert not status.any()
    for c, got in zip(cases, scans):
        assert got == _scan_of(ec.pillow_file(c)), ec.name(c)
    for (ss, q), sub in _group(cases).items():
        images = [torch.from_numpy(ec.pixels(c).copy()).to(gpu_device) for c in sub]
        got = je.encode_batch(images, quality=q, subsampling=ss, device_entropy=True)
        assert got == je.encode_batch(images, quality=q, subsampling=ss)
        assert got == [ec.pillow_file(c) for c in sub]


@pytest.mark.gpu
def test_restart_intervals_equal_the_host_pass_and_pillow(gpu_device):
    """72 x 56 grey at interval 1 has 63 intervals (RSTn wraps seven times); 65535 is longer than every image (DRI, no
    marker); restart_rows=1 gives every image its own interval"""
    import torch
    colour, grey = (48, 80, "4:2:0", 95, "smooth"), (72, 56, "grey", 95, "noise")
    assert colour in ec.BATCH_CASES and grey in ec.BATCH_CASES
    for kw in [dict(restart_interval=n) for n in (1, 2, 7, 8, 65535)] + [dict(restart_rows=1)]:
        for (ss, q), sub in _group(ec.BATCH_CASES).items():
            images = [torch.from_numpy(ec.pixels(c).copy()).to(gpu_device) for c in sub]
            got = je.encode_batch(images, quality=q, subsampling=ss, device_entropy=True, **kw)
            assert got == je.encode_batch(images, quality=q, subsampling=ss, **kw), (kw, ss, q)
            for c, f in zip(sub, got):
                if c in (colour, grey):
                    pkw = {"restart_marker_blocks": kw["restart_interval"]} if "restart_interval" in kw else {"restart_marker_rows": 1}
                    if c == colour:
                        pkw["subsampling"] = 2
                    assert f == jc.encode(ec.pixels(c), quality=q, **pkw), (kw, ec.name(c))
                if c == grey and kw.get("restart_interval") == 1:
                    assert len(re.findall(rb"\xff[\xd0-\xd7]", _scan_of(f))) == 62
                if kw.get("restart_interval") == 65535:
                    assert b"\xff\xdd\x00\x04\xff\xff" in f and not re.search(rb"\xff[\xd0-\xd7]", _scan_of(f))


def _crafted():
    """blocks in natural order, as images: grey rasters and one 4:2:0 image with dummy luma blocks"""
    zz = ref_jpeg.ZIGZAG
    zero = np.zeros(64, np.int16)
    last = zero.copy(); last[zz[63]] = 5                        # 3 ZRL, no EOB
    runs = zero.copy(); runs[zz[16]] = -3; runs[zz[17]] = 1; runs[zz[33]] = 700; runs[0] = -9     # runs of 15, 0 and 15 ...
    runs16 = zero.copy(); runs16[zz[17]] = 2; runs16[zz[34]] = -2                                  # ... and of exactly 16
    big = [np.full(64, 1023 if k % 2 == 0 else -1023, np.int16) for k in range(4)]                 # DC alternates: differences of +-2046
    minus, plus = np.full(64, -1, np.int16), np.full(64, 1, np.int16)
    rasters = [(np.stack([zero] * 5), 5), (np.stack([last, zero, last]), 3), (np.stack([runs, runs16, runs, zero]), 2),
               (np.stack(big), 4), (np.stack([minus, plus, minus, minus, plus, zero]), 3)]
    return rasters


@pytest.mark.gpu
def test_crafted_coefficients(gpu_device):
    """no pixels: all-zero blocks, only coefficient 63, runs of 15 and 16, +-1023 everywhere with 11-bit DC differences of
    both signs, all -1 (value bits all 0), all +1; each raster with intervals 0 and 1, and the same blocks as the
    components of a 4:2:0 image of 17 x 17 pixels (3 x 3 luma blocks real, 4 x 4 in the MCU grid: dummies beside and below)"""
    samples, parts, ivs, co = [], [], [], 0
    for blocks, across in _crafted():
        for ri in (0, 1):
            samples.append(_grey(blocks, across, co))
            parts.append(blocks.reshape(-1))
            ivs.append(ri)
            co += blocks.size
    colour = np.zeros(1, je.SAMPLE)
    n = je.fill_sample(colour[0], 17, 17, 3, (2, 2), je.quant_tables(90), co, 0)
    assert n == 64 * (9 + 4 + 4) and (int(colour[0]["blocks_w"][0]), int(colour[0]["blocks_h"][0])) == (3, 3)
    g = np.random.Generator(np.random.PCG64(11))
    blocks = (g.integers(-40, 41, (17, 64)) * (g.random((17, 64)) < .2)).astype(np.int16)
    blocks[:, 0] = g.integers(-1000, 1000, 17)
    for ri in (0, 1, 2):
        c = colour[0].copy()
        c["coef_offset"] += co - int(colour[0]["coef_offset"][0])
        samples.append(c)
        parts.append(blocks.reshape(-1))
        ivs.append(ri)
        co += blocks.size
    pool, samples = np.concatenate(parts), np.array(samples, je.SAMPLE)
    sizes, status, scans = _device_scans(pool, samples, ivs, gpu_device)
    assert not status.any()
    for k, got in enumerate(scans):
        assert got == _host_scan(pool, samples[k], ivs[k]), k


@pytest.mark.gpu
def test_stuffed_bytes_and_a_stuffed_byte_before_a_marker(gpu_device):
    """dense noise at quality 100 (seed 0 of 32 x 256, found on the CPU): the host pass's scan holds at least 50 stuffed
    FF 00 pairs and an interval that ends FF 00 directly in front of its RSTn"""
    import torch
    img = jc.image(0, 32, 256, "noise", 1)
    t = [torch.from_numpy(img).to(gpu_device)]
    want = je.encode_batch(t, quality=100, restart_interval=1)
    scan = _scan_of(want[0])
    assert scan.count(b"\xff\x00") >= 50 and re.search(rb"\xff\x00\xff[\xd0-\xd7]", scan)
    assert je.encode_batch(t, quality=100, restart_interval=1, device_entropy=True) == want
    want = je.encode_batch(t, quality=100)
    assert _scan_of(want[0]).count(b"\xff\x00") >= 50
    assert je.encode_batch(t, quality=100, device_entropy=True) == want


@pytest.mark.gpu
def test_tile_edges(gpu_device):
    """The kernels' constants: count and emit take 4 slots per workgroup and trip (a wave per slot); the scan's tile is
    1024 slots (256 threads x 4) and one workgroup scans 256 tile sums per trip; the stuffing pass takes 16 bytes per lane,
    1024 bytes per wave (a chunk), 4 chunks per workgroup and trip, and one workgroup scans 256 chunk counts per trip.
    Grey images of 3, 4, 5 and 1023, 1024, 1025 blocks, alone (the batch ends there) and in one batch; images whose
    unstuffed scan is 1023, 1024 and 1025 bytes long, alone and in one batch; one image of 257 scan tiles and more than
    256 chunks (a second trip of both one-workgroup scans)."""
    import torch

    def both(images, **kw):
        t = [torch.from_numpy(a).to(gpu_device) for a in images]
        want = je.encode_batch(t, **kw)
        assert je.encode_batch(t, device_entropy=True, **kw) == want
        return want

    blocks = [jc.image(300 + n, 8, 8 * n, "noise", 1) for n in (3, 4, 5, 1023, 1024, 1025)]
    for a in blocks:
        both([a], quality=60)
        both([a], quality=60, restart_interval=1)
    both(blocks, quality=60)
    both(blocks, quality=60, restart_interval=5)
    edges = [jc.image(seed, 8, 122, "noise", 1) for seed in (5, 2, 28)]
    for a, length in zip(edges, (1023, 1024, 1025)):
        (f,) = both([a], quality=95)
        scan = _scan_of(f)
        assert len(scan) - scan.count(b"\xff\x00") == length
    both(edges, quality=95)
    both(edges[::-1] + edges, quality=95, restart_interval=4)
    yy, xx = np.arange(512, dtype=np.float32)[:, None], np.arange(8 * 4097, dtype=np.float32)[None, :]
    large = (128 + 100 * np.sin(xx / 9) * np.cos(yy / 7) + 5 * ((xx * 7 + yy * 13) % 5)).astype(np.uint8)
    (f,) = both([large], quality=90)
    assert len(_scan_of(f)) > 257 * 1024


@pytest.mark.gpu
def test_a_batch_of_1024_descriptors(gpu_device):
    pool, samples = _pool(ec.BATCH_CASES, repeat=128)
    ivs = [(0, 1, 3, 65535)[(k // 8) % 4] for k in range(1024)]
    sizes, status, scans = _device_scans(pool, samples, ivs, gpu_device)
    assert not status.any()
    want = {}
    for k, got in enumerate(scans):
        key = (k % 8, ivs[k])
        if key not in want:
            want[key] = _host_scan(pool, samples[k], ivs[k])
        assert got == want[key], k


@pytest.mark.gpu
def test_refused_samples_write_nothing_and_leave_their_neighbours_alone(gpu_device):
    """status 1: skip, a wrong grid, a coef_offset past coef_count, a restart interval of -1 and of 65536 (and descriptors
    that name more blocks than the pool holds); status 2: an AC value of 1024, a DC difference of 2048 -- for that image
    only.  _device_scans checks that a refused image has scan_bytes 0 and that nothing outside the ranges is written."""
    cases = [ec.BATCH_CASES[k % 8] for k in range(12)]
    pool, samples = _pool(cases)
    pool = pool.copy()
    ivs = [0, 2, 0, 3, 0, 0, 1, 0, 0, 5, 0, 0]
    samples[1]["skip"] = 1
    samples[3]["blocks_w"][0] += 1
    samples[5]["coef_offset"][0] = pool.size
    ivs[6] = -1
    ivs[8] = 65536
    at = int(samples[9]["coef_offset"][0])
    pool[at + 64 + 17] = 1024                                   # an AC value of 11 bits
    at = int(samples[11]["coef_offset"][0])
    pool[at], pool[at + 64] = 1024, -1024                       # a DC difference of 12 bits
    sizes, status, scans = _device_scans(pool, samples, ivs, gpu_device)
    assert status.tolist() == [0, 1, 0, 1, 0, 1, 1, 0, 1, 2, 0, 2]
    for k in np.flatnonzero(status == 0):
        assert scans[k] == _host_scan(pool, samples[k], ivs[k]), k
    for k, what in ((9, "AC coefficient of 11 bits"), (11, "DC difference of 12 bits")):
        with pytest.raises(_lib.DspnError, match=what):
            je.entropy_encode(pool, samples[k], restart_interval=ivs[k])
    # descriptors that overlap: twice the blocks the pool holds; the second half is refused, the first is right
    pool, samples = _pool(ec.BATCH_CASES[:5])
    twice = np.concatenate([samples, samples])
    sizes, status, scans = _device_scans(pool, twice, [0] * 10, gpu_device)
    assert status.tolist() == [0] * 5 + [1] * 5
    for k in range(5):
        assert scans[k] == _host_scan(pool, twice[k], 0), k


@pytest.mark.gpu
def test_an_output_one_byte_short_leaves_the_last_image_unwritten(gpu_device):
    pool, samples = _pool(ec.BATCH_CASES[:4])
    sizes, status, scans = _device_scans(pool, samples, [0, 1, 0, 2], gpu_device, short=1)
    assert not status.any() and scans[3] is None
    for k in range(3):
        assert scans[k] == _host_scan(pool, samples[k], [0, 1, 0, 2][k])


@pytest.mark.gpu
def test_encode_batch_raises_the_host_passs_refusal(gpu_device, monkeypatch):
    import torch
    real = je.encode_blocks

    def spoiled(images, samples, coefs, *a, **kw):
        ws = real(images, samples, coefs, *a, **kw)
        coefs[64 + 9] = -1024
        return ws

    monkeypatch.setattr(je, "encode_blocks", spoiled)
    images = [torch.from_numpy(ec.pixels(c).copy()).to(gpu_device) for c in ec.BATCH_CASES[3::4]]      # two grey images
    for flag in (False, True):
        with pytest.raises(_lib.DspnError, match="AC coefficient of 11 bits"):
            je.encode_batch(images, device_entropy=flag)


@pytest.mark.gpu
def test_callers_give_the_same_bytes(gpu_device, tmp_path):
    import torch
    from PIL import Image
    from dspnet_amd.dataset import im2rec
    from dspnet_amd.detect import render
    cases = [(21, 37, "4:2:0", 95, "noise"), (24, 40, "4:2:0", 95, "smooth")]
    bgr = [torch.from_numpy(np.ascontiguousarray(ec.pixels(c)[:, :, ::-1])).to(gpu_device) for c in cases]
    headers = [recordio.IRHeader(0, float(k), k, 0) for k in range(2)]
    assert recordio.pack_img_batch(headers, bgr, quality=90, device_entropy=True) == recordio.pack_img_batch(headers, bgr, quality=90)
    assert (recordio.pack_img_batch(headers, bgr, restart_interval=2, device_entropy=True)
            == recordio.pack_img_batch(headers, bgr, restart_interval=2))
    for k, c in enumerate([cases[0], (9, 15, "grey", 30, "noise")]):
        t = torch.from_numpy(ec.pixels(c).copy()).to(gpu_device)
        render.save_jpeg(str(tmp_path / ("a%d.jpg" % k)), t, quality=c[3])
        render.save_jpeg(str(tmp_path / ("b%d.jpg" % k)), t, quality=c[3], device_entropy=True)
        assert (tmp_path / ("a%d.jpg" % k)).read_bytes() == (tmp_path / ("b%d.jpg" % k)).read_bytes() == ec.pillow_file(c)
    os.makedirs(str(tmp_path / "img"))
    for k, c in enumerate(cases):
        Image.fromarray(ec.pixels(c)).save(str(tmp_path / "img" / ("%d.png" % k)))
    for name in ("host", "dev"):
        with open(str(tmp_path / (name + ".lst")), "w") as f:
            f.writelines("%d\t%f\timg/%d.png\n" % (k, k + .5, k) for k in range(2))
    assert im2rec.write_records(str(tmp_path / "host"), str(tmp_path), quality=92, device=gpu_device) == 2
    assert im2rec.write_records(str(tmp_path / "dev"), str(tmp_path), quality=92, device=gpu_device, device_entropy=True) == 2
    assert (tmp_path / "host.rec").read_bytes() == (tmp_path / "dev.rec").read_bytes()
    assert (tmp_path / "host.idx").read_bytes() == (tmp_path / "dev.idx").read_bytes()


@pytest.mark.gpu
def test_a_call_on_another_stream_gives_the_same_bytes(gpu_device):
    import torch
    cases = ec.BATCH_CASES
    pool, samples = _pool(cases)
    side = torch.cuda.Stream(gpu_device)
    sizes, status, scans = _device_scans(pool, samples, [3] * len(cases), gpu_device, stream=side)
    assert not status.any()
    for k, got in enumerate(scans):
        assert got == _host_scan(pool, samples[k], 3)
    sub = [c for c in cases if c[2] == "4:2:2" and c[3] == 95]
    images = [torch.from_numpy(ec.pixels(c).copy()).to(gpu_device) for c in sub]
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.stream(side):
        got = je.encode_batch(images, quality=95, subsampling="4:2:2", device_entropy=True)
    assert got == [ec.pillow_file(c) for c in sub]
