"""The record pipeline's kernels at the edges the thumbnail-sized suites pass over: JPEG decode (csrc/jpeg.hip) and encode
(csrc/jpeg_encode.hip) with rows of more than one chunk, more work than one trip of their fixed grids, kMaxB descriptors
and runs of skipped ones; the warp (csrc/augment.hip) with more than one workgroup across, real-size sources and
saturated coordinates.  Every comparison is exact: bytes, int16 coefficients, float bits.

The yardsticks: Pillow for both JPEG directions (tests/jpeg_cases.py, tests/jpeg_encode_cases.py), oracle/augment.py for the
warp (pinned to OpenCV by the committed vectors of tests/test_record_iter.py).

Largest sides.  Pillow (libjpeg) neither writes nor reads a side above 65 500 (JPEG_MAX_DIMENSION), so the comparisons
with Pillow run at 65 500 x 1 and 1 x 65 500: 64 chunks, 8188 blocks across, 65 500 row units.  The format's own limit,
65 535, which the decode kernels admit (8192 blocks across), is run on made-up coefficients against the reconstruction of
tests/ref_jpeg.py, which the CPU tests here and tests/test_jpeg_host.py pin to Pillow.  The encoder's front end refuses a
side above 65 500 like Pillow does, so for it 65 500 is the largest extent there is."""
import numpy as np
import pytest

import augment_cases as ac
import jpeg_cases as jc
import jpeg_encode_cases as ec
import ref_jpeg
from dspnet_amd.dataset import jpeg as dj
from dspnet_amd.dataset import jpeg_encode as je

DEC = jc.kernel_constants("jpeg.hip", ("kT", "kMaxB", "kGrid", "kBlocksPerWg", "kRowPix"))
ENC = jc.kernel_constants("jpeg_encode.hip", ("kT", "kMaxB", "kGrid", "kBlocksPerWg", "kRowSamples"))
WARP = jc.kernel_constants("augment.hip", ("kT",))

# the 1024-descriptor calls: eight distinct samples dealt round; skipped: the first, the last, a run in the middle, and
# two runs that end / start next to a live sample at the ends (equal entries of first[] at both ends of the search)
BATCH = 1024
SKIP = frozenset([0, 1, 2, 300, 511, 512, 513, 514, 700, 701, 1021, 1022, 1023])


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# 1. JPEG decode: the inputs and the host half, without a GPU
def _chunk_layout():
    """what decode_batch makes of CHUNK_NAMES in one call: per case (name, h, w, img_offset)"""
    out, at = [], 0
    for n in jc.CHUNK_NAMES:
        h, w = jc.edge_size(n)
        out.append((n, h, w, at))
        at += 3 * h * w
    return out


def test_chunk_cases_cover_the_chunk_counts_and_both_store_paths():
    """every layout meets one, two and three or more chunks, 1025 (one pixel in the second chunk) and 1027; over the
    call, a second chunk starts on a dword boundary with four pixels to store (the dword path), off one, and with a tail"""
    rp = DEC["kRowPix"]
    assert rp == 1024, "kRowPix changed: move CHUNK_WIDTHS in tests/jpeg_cases.py with it"
    for lname, _, _ in jc.EDGE_LAYOUTS:
        widths = {w for n, h, w, _ in _chunk_layout() if n.endswith("-" + lname)}
        assert {rp + 1, rp + 3} <= widths and {1, 2} <= {_cdiv(w, rp) for w in widths} and max(_cdiv(w, rp) for w in widths) >= 3, lname
    starts = set()                                             # (dword aligned, four whole pixels) at each start of a second chunk
    for n, h, w, at in _chunk_layout():
        for y in range(h):
            if w > rp:                                          # the pool itself is at least dword aligned (asserted on the device)
                starts.add(((at + 3 * (y * w + rp)) % 4 == 0, w - rp >= 4))
    assert {(True, True), (False, True), (True, False), (False, False)} <= starts
    assert {jc.edge_size(n)[0] for n in jc.CHUNK_NAMES} == set(jc.CHUNK_HEIGHTS)


@pytest.mark.parametrize("part", ["chunk", "extent", "batch", "narrow"])
def test_probe_of_every_edge_stream_equals_reference_parse(part):
    assert len(jc.EDGE_CASES) == len(jc.CHUNK_NAMES + jc.EXTENT_NAMES + jc.BATCH_NAMES + jc.NARROW_NAMES)
    for name in {"chunk": jc.CHUNK_NAMES, "extent": jc.EXTENT_NAMES, "batch": jc.BATCH_NAMES, "narrow": jc.NARROW_NAMES}[part]:
        data = jc.edge_stream(name)
        P = ref_jpeg.parse(data)
        rc, info = dj.probe_info(data)
        nc = P["ncomp"]
        assert rc == 0 and info["supported"], name
        assert (int(info["height"]), int(info["width"])) == jc.edge_size(name) == (P["height"], P["width"]), name
        assert info["blocks_w"][:nc].tolist() == P["blocks_w"] and info["blocks_h"][:nc].tolist() == P["blocks_h"], name
        assert int(info["coef_count"]) == 64 * sum(bw * bh for bw, bh in zip(P["blocks_w"], P["blocks_h"])), name


@pytest.mark.parametrize("layout", [l[0] for l in jc.EDGE_LAYOUTS])
def test_host_entropy_decode_and_restatement_equal_pillow_on_chunk_cases(layout):
    """the host half at these widths, and the yardstick of the 65 535 test below; with them the images of 1 to 6 pixels
    across and the tall extents, where libjpeg-turbo upsamples a chroma plane of at most two columns by repetition"""
    for name in (n for n in jc.CHUNK_NAMES + jc.NARROW_NAMES + jc.EXTENT_NAMES[2:] if n.endswith("-" + layout)):
        data = jc.edge_stream(name)
        P = ref_jpeg.parse(data)
        info, coefs = jc._coded(data)
        planes = [coefs[int(info["coef_offset"][c]):][:64 * P["blocks_w"][c] * P["blocks_h"][c]].reshape(P["blocks_h"][c], P["blocks_w"][c], 64)
                  for c in range(P["ncomp"])]
        np.testing.assert_array_equal(ref_jpeg.pixels(P, planes), jc.edge_pillow_pixels(name), err_msg=name)


def _decode_call():
    """the 1024-descriptor call -> (names, coded streams, descriptors, regions, bytes of the pool)"""
    names = [jc.BATCH_NAMES[k % len(jc.BATCH_NAMES)] for k in range(BATCH)]
    coded = [jc._coded(jc.edge_stream(n)) for n in names]
    return (names, coded) + jc.describe_batch(coded, SKIP)


def test_decode_call_exceeds_one_trip_of_each_kernel_with_kmaxb_samples():
    _, _, samples, _, _ = _decode_call()
    assert len(samples) == DEC["kMaxB"] == dj.MAX_BATCH, "kMaxB changed: grow BATCH (and MAX_BATCH of dataset/jpeg.py) with it"
    live = samples[samples["skip"] == 0]
    assert len(live) == BATCH - len(SKIP) and {0, BATCH - 1} <= SKIP
    blocks = sum(int((s["blocks_w"][:s["ncomp"]].astype(np.int64) * s["blocks_h"][:s["ncomp"]]).sum()) for s in live)
    units = sum(int(s["height"]) * _cdiv(int(s["width"]), DEC["kRowPix"]) for s in live)
    grow = ": grow BATCH_SHAPES in tests/jpeg_cases.py"
    assert DEC["kBlocksPerWg"] == DEC["kT"] // 8
    assert blocks > DEC["kGrid"] * DEC["kBlocksPerWg"], "jpeg_idct_kernel covers %d blocks in one trip" % (DEC["kGrid"] * DEC["kBlocksPerWg"]) + grow
    assert blocks % (DEC["kGrid"] * DEC["kBlocksPerWg"]) % DEC["kBlocksPerWg"] != 0, "the last workgroup pass should be partly idle"
    assert units > DEC["kGrid"], "jpeg_colour_kernel covers %d row units in one trip" % DEC["kGrid"] + grow
    assert any(int(s["img_offset"]) % 4 for s in live) and len({(int(s["ncomp"]), int(s["hsamp"]), int(s["vsamp"])) for s in live}) == 4


def test_decode_batch_names_its_batch_limit():
    """refused before a stream is read or a device touched"""
    data = jc.stream("8x8-ss0-q90-std-smooth")
    with pytest.raises(ValueError, match="batch limit.* %d" % DEC["kMaxB"]):
        dj.decode_batch([data] * (DEC["kMaxB"] + 1), "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# 1. JPEG decode on the device
@pytest.mark.gpu
def test_decode_rows_of_several_chunks_equal_pillow(gpu_device):
    """one call over the 32 chunk cases, in the order test_chunk_cases_cover_... lays out"""
    import torch
    payloads = [jc.edge_stream(n) for n in jc.CHUNK_NAMES]
    got = dj.decode_batch(payloads, gpu_device)
    assert got[0].data_ptr() % 4 == 0
    for (name, h, w, at), g in zip(_chunk_layout(), got):
        assert g.data_ptr() - got[0].data_ptr() == at and tuple(g.shape) == (h, w, 3), name
        assert torch.equal(g.cpu(), torch.from_numpy(jc.edge_pillow_pixels(name).copy())), name


@pytest.mark.gpu
def test_decode_largest_sides_pillow_reads_equal_pillow(gpu_device):
    import torch
    got = dj.decode_batch([jc.edge_stream(n) for n in jc.EXTENT_NAMES], gpu_device)
    assert sorted(tuple(g.shape) for g in got) == [(1, jc.MAX_SIDE, 3)] * 2 + [(jc.MAX_SIDE, 1, 3)] * 2
    for name, g in zip(jc.EXTENT_NAMES, got):
        assert torch.equal(g.cpu(), torch.from_numpy(jc.edge_pillow_pixels(name).copy())), name


@pytest.mark.gpu
def test_decode_chroma_planes_of_one_to_three_columns_equal_pillow(gpu_device):
    """the defect the 65 500 x 1 extent showed: 4:2:0 and 4:2:2 images up to 4 pixels wide take libjpeg-turbo's box
    upsampling (down the rows too), 5 and 6 pixels the triangle filter"""
    import torch
    got = dj.decode_batch([jc.edge_stream(n) for n in jc.NARROW_NAMES], gpu_device)
    for name, g in zip(jc.NARROW_NAMES, got):
        assert torch.equal(g.cpu(), torch.from_numpy(jc.edge_pillow_pixels(name).copy())), name


def _made_up(seed, h, w, ncomp):
    """a 4:2:0 or grey image of h x w as the host half would hand it over, with seeded coefficients -> (info, coefs, P of
    ref_jpeg, planes of ref_jpeg)"""
    g = np.random.Generator(np.random.PCG64(seed))
    hs = 2 if ncomp == 3 else 1
    mx, my = _cdiv(w, 8 * hs), _cdiv(h, 8 * hs)
    bw, bh = [mx * hs, mx, mx][:ncomp], [my * hs, my, my][:ncomp]
    lum, chrom = je.quant_tables(90)
    quant = [lum, chrom, chrom][:ncomp]
    planes = []
    for c in range(ncomp):
        p = g.integers(-6, 7, (bh[c], bw[c], 64))
        p[:, :, 0] = g.integers(-80, 81, (bh[c], bw[c]))        # with the AC terms: samples over the whole range, clamps included
        planes.append(p.astype(np.int16))
    info = np.zeros(1, dj.INFO)[0]
    info["width"], info["height"], info["ncomp"], info["supported"] = w, h, ncomp, 1
    info["hsamp"][:ncomp], info["vsamp"][:ncomp] = [hs, 1, 1][:ncomp], [hs, 1, 1][:ncomp]
    info["blocks_w"][:ncomp], info["blocks_h"][:ncomp] = bw, bh
    sizes = [64 * a * b for a, b in zip(bw, bh)]
    info["coef_offset"][:ncomp] = np.cumsum([0] + sizes[:-1])
    info["coef_count"] = sum(sizes)
    for c in range(ncomp):
        info["quant"][c] = quant[c]
    P = dict(width=w, height=h, ncomp=ncomp, quant=quant, hsamp=[hs, 1, 1][:ncomp], vsamp=[hs, 1, 1][:ncomp])
    return info, np.concatenate([p.reshape(-1) for p in planes]), P, planes


@pytest.mark.gpu
def test_decode_sides_of_65535_equal_the_restatement(gpu_device):
    """the largest sides the descriptor check admits (8192 blocks across, 64 chunks, 65 535 row units), beyond what Pillow
    reads: seeded coefficients, the reconstruction of ref_jpeg as the yardstick, guard bytes around every output"""
    made = [_made_up(50 + k, h, w, nc) for k, (h, w, nc) in enumerate([(1, 65535, 3), (65535, 1, 3), (1, 65535, 1), (65535, 1, 1)])]
    assert max(int(m[0]["blocks_w"][0]) for m in made) == 8192 == max(int(m[0]["blocks_h"][0]) for m in made)
    pool, regions = jc.launch_guarded([(m[0], m[1]) for m in made], (), gpu_device)
    covered = np.zeros(pool.size, bool)
    for (info, _, P, planes), (at, n) in zip(made, regions):
        covered[at:at + n] = True
        np.testing.assert_array_equal(pool[at:at + n], ref_jpeg.pixels(P, planes).reshape(-1), err_msg="%d x %d" % (P["height"], P["width"]))
    assert (pool[~covered] == 0xA5).all()


@pytest.mark.gpu
def test_decode_second_grid_trips_with_kmaxb_descriptors_and_skip_runs(gpu_device):
    names, coded, _, _, _ = _decode_call()
    pool, regions = jc.launch_guarded(coded, SKIP, gpu_device)
    covered = np.zeros(pool.size, bool)
    for k, (name, (at, n)) in enumerate(zip(names, regions)):
        covered[at:at + n] = True
        if k in SKIP:
            assert (pool[at:at + n] == 0xA5).all(), "the region of skipped sample %d was written" % k
        elif not np.array_equal(pool[at:at + n], jc.edge_pillow_pixels(name).reshape(-1)):
            raise AssertionError("sample %d (%s) differs from Pillow" % (k, name))
    assert (pool[~covered] == 0xA5).all() and (~covered).sum() == 2 * 64 * BATCH


# ---------------------------------------------------------------------------------------------------------------------
# 2. JPEG encode
def _encode_cases():
    return [ec.BATCH_CASES[k % len(ec.BATCH_CASES)] for k in range(BATCH)]


def test_encode_call_exceeds_one_trip_of_each_kernel_with_kmaxb_samples():
    samples, _, _, _ = ec.describe_batch(_encode_cases(), SKIP)
    assert len(samples) == ENC["kMaxB"], "kMaxB changed: grow BATCH with it"
    live = samples[samples["skip"] == 0]
    assert len(live) == BATCH - len(SKIP)
    blocks = sum(int((s["blocks_w"][:s["ncomp"]].astype(np.int64) * s["blocks_h"][:s["ncomp"]]).sum()) for s in live)
    units = sum(sum(int(s["blocks_h"][c]) * 8 * _cdiv(int(s["blocks_w"][c]) * 8, ENC["kRowSamples"]) for c in range(int(s["ncomp"])))
                for s in live)
    grow = ": grow BATCH_CASES in tests/jpeg_encode_cases.py"
    assert ENC["kBlocksPerWg"] == ENC["kT"] // 8
    assert blocks > ENC["kGrid"] * ENC["kBlocksPerWg"], "jpeg_enc_fdct_kernel covers %d blocks in one trip" % (ENC["kGrid"] * ENC["kBlocksPerWg"]) + grow
    assert units > ENC["kGrid"], "jpeg_enc_planes_kernel covers %d row units in one trip" % ENC["kGrid"] + grow
    assert {c[2] for c in ec.BATCH_CASES} == set(ec.LAYOUTS) and any(int(s["img_offset"]) % 4 for s in live)


@pytest.mark.gpu
def test_encode_second_grid_trips_with_kmaxb_descriptors_and_skip_runs(gpu_device):
    cases = _encode_cases()
    coefs, samples, ws = ec.low_level_batch(cases, gpu_device, skip=SKIP)
    ec.check_batch(cases, coefs, samples, ws, untouched=SKIP)


@pytest.mark.gpu
def test_encode_largest_sides_equal_pillows_files(gpu_device):
    """65 500 x 1 and 1 x 65 500 in one call, as greyscale and as 4:2:0 (the side Pillow and encode_batch both stop at)"""
    import torch
    assert je.MAX_SIDE == jc.MAX_SIDE
    for ch, kw in ((1, {}), (3, dict(subsampling=2))):
        imgs = [jc.image(60 + ch, 1, jc.MAX_SIDE, "noise", ch), jc.image(70 + ch, jc.MAX_SIDE, 1, "noise", ch)]
        got = je.encode_batch([torch.from_numpy(a).to(gpu_device) for a in imgs], quality=90, subsampling="4:2:0")
        for a, f in zip(imgs, got):
            assert f == jc.encode(a, quality=90, **kw), (a.shape, kw)
    with pytest.raises(ValueError, match=str(je.MAX_SIDE)):
        je.encode_batch([torch.zeros(1, je.MAX_SIDE + 1, dtype=torch.uint8, device=gpu_device)])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the warp
WARP_WIDTHS = [252, 256, 260, 1020, 1024, 1028, 2052]
LUT = np.arange(256, dtype=np.uint8)[::-1].copy()


def test_warp_widths_cover_one_and_more_workgroups_across():
    kt = WARP["kT"]
    assert {_cdiv(w, kt) for w in WARP_WIDTHS} >= {1, 2, 5, 9} and any(w % kt for w in WARP_WIDTHS) and any(w % kt == 0 for w in WARP_WIDTHS)
    assert {w // 4 for w in WARP_WIDTHS} >= {kt, kt + 1}, "the label grid should meet exactly kT and kT + 1 quarter-columns"
    assert {_cdiv(w // 4, kt) for w in WARP_WIDTHS} == {1, 2, 3}


def _shifted(src, tx, ty, H, W, border):
    """dst(x, y) = src(x - tx, y - ty), `border` outside: plain indexing, no interpolation code"""
    ys, xs = np.arange(H) - ty, np.arange(W) - tx
    ok = ((ys >= 0) & (ys < src.shape[0]))[:, None] & ((xs >= 0) & (xs < src.shape[1]))[None, :]
    v = src[np.clip(ys, 0, src.shape[0] - 1)[:, None], np.clip(xs, 0, src.shape[1] - 1)[None, :]]
    return np.where(ok.reshape(ok.shape + (1,) * (src.ndim - 2)), v, border).astype(np.uint8)


def _finish(w, ws, flip, lut):
    """flip, planes R, G, B of a BGR image minus the mean, labels at every fourth pixel through the table"""
    if flip:
        w, ws = w[:, ::-1], ws[:, ::-1]
    d = np.stack([(w[:, :, 2 - c].astype(np.float64) - ac.MEAN[c]).astype(np.float32) for c in range(3)])
    q = ws[::4, ::4]
    return d, (q if lut is None else lut[q]).astype(np.float32)


@pytest.fixture(scope="module")
def frame():
    """a source of the training records' size, 1024 x 2048, random bytes (read-only)"""
    g = np.random.Generator(np.random.PCG64(31))
    img, seg = g.integers(0, 256, (1024, 2048, 3), dtype=np.uint8), g.integers(0, 256, (1024, 2048), dtype=np.uint8)
    img.setflags(write=False); seg.setflags(write=False)
    return img, seg


@pytest.mark.gpu
@pytest.mark.parametrize("W", WARP_WIDTHS)
def test_warp_wide_outputs_equal_the_oracle(gpu_device, frame, W):
    """per shape four samples: a rotation that leaves a small source on every side; the same kind without a label map
    and with the other borders; an integer translation, whose output is a slice of the source; a source as wide as the
    output at a scale near 1 (at 8 x 2052 the 1024 x 2048 frame, sampled from its first to its last column and past its
    bottom row).  Flips alternate and swap between the two heights; each shape runs with and without the table."""
    g = np.random.Generator(np.random.PCG64(1000 + W))
    for H in (4, 8):
        hw = [(int(g.integers(20, 70)), int(g.integers(20, 90))), (int(g.integers(20, 70)), int(g.integers(20, 90))), (H + 5, W + 9)]
        imgs = [g.integers(0, 256, s + (3,), dtype=np.uint8) for s in hw]
        segs = [g.integers(0, 256, s, dtype=np.uint8) for s in hw]
        if (H, W) == (8, 2052):
            imgs.append(frame[0]); segs.append(frame[1])
            far = -1018.0                                       # output rows read source rows 1014 .. 1025: the last ones are border
        else:
            imgs.append(g.integers(0, 256, (H + 12, W - 4, 3), dtype=np.uint8)); segs.append(g.integers(0, 256, (H + 12, W - 4), dtype=np.uint8))
            far = -3.0
        Ms = []
        for b in range(2):                                      # scaled up to the output's width, so all four sides show border
            th = g.uniform(-1.5, 1.5) * H / W                 # a slope of a few output rows over the width
            sx, sy = g.uniform(.6, .9) * W / hw[b][1], g.uniform(.4, 1.5) * H / hw[b][0]
            Ms.append([sx * np.cos(th), -sy * np.sin(th), g.uniform(.05, .15) * W, sx * np.sin(th), sy * np.cos(th), g.uniform(-1, 1)])
        tx, ty = 7, -2
        Ms.append([1, 0, tx, 0, 1, ty])
        s, th = W / float(imgs[3].shape[1]), 0.002
        Ms.append([s * np.cos(th), -s * np.sin(th), 1.5, s * np.sin(th), s * np.cos(th), far])
        flips = [(b + H // 4) % 2 for b in range(4)]
        borders = [(128, 255), (7, 3), (7, 3), (128, 255)]
        for lut in (LUT, None):
            got, got_seg, samples = ac.run_batch(gpu_device, imgs, segs, Ms, H, W, flips, borders, no_seg={1}, lut=lut)
            for b in range(4):
                d, q = ac.oracle_sample(imgs[b], segs[b], Ms[b], H, W, flips[b], borders[b], has_seg=b != 1, lut=lut)
                np.testing.assert_array_equal(got[b], d, err_msg="image %d of %d x %d" % (b, H, W))
                np.testing.assert_array_equal(got_seg[b], q, err_msg="labels %d of %d x %d" % (b, H, W))
            d, q = _finish(_shifted(imgs[2], tx, ty, H, W, borders[2][0]), _shifted(segs[2], tx, ty, H, W, borders[2][1]), flips[2], lut)
            np.testing.assert_array_equal(got[2], d, err_msg="the translated image of %d x %d is not a slice of its source" % (H, W))
            np.testing.assert_array_equal(got_seg[2], q, err_msg="the translated labels of %d x %d are not a slice of their source" % (H, W))
        # the wide source is sampled from end to end
        m = samples[3]["minv"]
        assert m[2] < 1 and m[0] * (W - 1) + m[1] * (H - 1) + m[2] > imgs[3].shape[1] - 3


@pytest.mark.gpu
def test_warp_saturated_coordinates_are_border(gpu_device, frame):
    """source coordinates past 32 767 and below -32 768 saturate to short and read border, in the kernel as in the
    oracle; every other pixel equals the oracle's"""
    H, W = 4, 2052
    img, seg = frame[0][:16], frame[1][:16]
    Ms = [[.05, 0, -5, 0, 1, -1]] * 2 + [[.05, 0, 1800, 0, 1, -1]] * 2        # source x = 20 x + 100 and 20 x - 36 000
    flips, borders = [0, 1, 0, 1], [(128, 255), (7, 3), (7, 3), (128, 255)]
    got, got_seg, samples = ac.run_batch(gpu_device, [img] * 4, [seg] * 4, Ms, H, W, flips, borders, lut=LUT)
    for b in range(4):
        d, q = ac.oracle_sample(img, seg, Ms[b], H, W, flips[b], borders[b], lut=LUT)
        np.testing.assert_array_equal(got[b], d, err_msg="image %d" % b)
        np.testing.assert_array_equal(got_seg[b], q, err_msg="labels %d" % b)
        xd = np.arange(W)[::-1] if flips[b] else np.arange(W)
        sx = samples[b]["minv"][0] * xd + samples[b]["minv"][2]
        out, inside = (sx > 32768) | (sx < -32769), (sx >= 0) & (sx < img.shape[1] - 1)
        assert out.sum() > 100 and inside.sum() > 50, "the row should hold saturated and ordinary pixels"
        for c in range(3):
            assert (got[b][c][:, out] == np.float32(borders[b][0] - ac.MEAN[c])).all()
            assert (got[b][c][1:, inside] != np.float32(borders[b][0] - ac.MEAN[c])).any()
        assert (got_seg[b][:, out[::4]] == float(LUT[borders[b][1]])).all()
