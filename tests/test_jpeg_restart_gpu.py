"""The entropy pass on the device (dspn_jpeg_entropy_decode_batch, include/dspn_jpeg.h) and the encoder's restart markers
on the GPU: the device's coefficients against the host entropy pass's over every restart stream of jpeg_cases.CASES and
the edge streams of jpeg_restart_cases, mixed batches inside guarded pools, a batch whose segments pass the grid once, bad
streams (already rejected cleanly by the host build of the same decode under tools/jpeg_huff_check.cpp), the encoder's
round trip and both iterators."""
import os

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_restart_cases as rc
from dspnet_amd import _lib
from dspnet_amd.dataset import jpeg as dj
from dspnet_amd.dataset import jpeg_encode as je

GUARD = 61                                                     # odd: every img_offset and every scan lands on an odd byte
FILL16 = -23131                                                # 0xA5A5


def _launch(entries, dev, reconstruct=True, spoil=None):
    """entries: (payload, mode), mode "device" (entropy pass on the device), "host" (coefficients from the host pass) or
    "skip"; a third element names the sound stream a damaged payload was made from (same header, same geometry).  Every
    pool carries guards of 0xA5 around every sample's part.  -> dict of host arrays and the regions"""
    import torch
    B = len(entries)
    samples, scans = np.zeros(B, dj.SAMPLE), np.zeros(B, dj.SCAN)
    coefs, pool, segs = [np.full(64, FILL16, np.int16)], [np.full(GUARD, 0xA5, np.uint8)], [np.full(3, 0xA5A5A5A5, np.uint32)]
    co, po, so, io_ = 64, GUARD, 3, 0
    cregions, iregions = [], []
    for k, (payload, mode, *sound) in enumerate(entries):
        if mode == "device":
            info, scan, seg, host = rc.indexed(sound[0] if sound else payload)
            if sound:
                scan, seg = dj.scan_index(payload, info)
        else:
            info, host = jc._coded(payload)
        io_ += GUARD
        dj.fill_sample(samples[k], info, co, io_)
        samples[k]["skip"] = int(mode == "skip")
        n = int(info["width"]) * int(info["height"]) * 3
        iregions.append((io_, n))
        io_ += n + GUARD
        cregions.append((co, host.size))
        coefs += [host if mode == "host" else np.full(host.size, FILL16, np.int16), np.full(64, FILL16, np.int16)]
        co += host.size + 64
        if mode == "device":
            scans[k] = scan
            a, nb = int(scan["data_offset"]), int(scan["data_bytes"])
            scans[k]["data_offset"], scans[k]["first_segment"] = po, so
            pool += [np.frombuffer(payload, np.uint8, nb, a), np.full(GUARD, 0xA5, np.uint8)]
            po += nb + GUARD
            segs += [seg, np.full(3, 0xA5A5A5A5, np.uint32)]
            so += seg.size + 3
    if spoil:
        spoil(samples, scans)
    coefs, pool, segs = np.concatenate(coefs), np.concatenate(pool), np.concatenate(segs)
    t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    cdev = torch.from_numpy(coefs.copy()).to(dev)
    pdev, sdev, scdev, segdev = t(pool), t(samples), t(scans), t(segs).view(torch.int32)
    status = torch.full((B + 2,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    images = torch.full((io_ + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    dj.entropy_decode_device(pdev, sdev, scdev, segdev, cdev, status[1:B + 1])
    if reconstruct:
        dj.reconstruct(cdev, sdev, images)
    torch.cuda.synchronize(dev)
    st = status.cpu().numpy()
    assert st[0] == 0x5A5A5A5A and st[-1] == 0x5A5A5A5A, "guard words of the status array overwritten"
    for name, before, after in (("byte pool", pool, pdev), ("segment table", segs, segdev), ("descriptors", samples, sdev),
                                ("scans", scans, scdev)):
        assert before.tobytes() == after.cpu().numpy().tobytes(), "the %s was written" % name
    return {"coefs": cdev.cpu().numpy(), "before": coefs, "status": st[1:-1], "images": images.cpu().numpy(),
            "cregions": cregions, "iregions": iregions}


def _check(entries, out, bad=()):
    """device and host samples: the host pass's coefficients and Pillow's pixels; skipped ones and every guard: untouched"""
    covered_c, covered_i = np.zeros(out["coefs"].size, bool), np.zeros(out["images"].size, bool)
    for k, ((payload, mode, *_), (ca, cn), (ia, n)) in enumerate(zip(entries, out["cregions"], out["iregions"])):
        got = out["coefs"][ca:ca + cn]
        if k in bad:
            assert out["status"][k] != 0, "sample %d: no status" % k
            covered_c[ca:ca + cn] = covered_i[ia:ia + n] = True    # unspecified, but inside the sample's own regions
            continue
        assert out["status"][k] == 0, "sample %d: status %s" % (k, dj.status_parts(out["status"][k]),)
        if mode == "skip":
            continue                                            # stays uncovered: must still hold the fill
        covered_c[ca:ca + cn] = covered_i[ia:ia + n] = True
        np.testing.assert_array_equal(got, jc._coded(payload)[1], err_msg="coefficients of sample %d (%s)" % (k, mode))
        px = jc.pillow_pixels(payload)
        np.testing.assert_array_equal(out["images"][ia:ia + n].reshape(px.shape), px, err_msg="pixels of sample %d" % k)
    assert (out["coefs"][~covered_c] == FILL16).all(), "coefficients outside the decoded samples were written"
    assert (out["images"][~covered_i] == 0xA5).all(), "image bytes outside the decoded samples were written"


@pytest.mark.gpu
def test_device_coefficients_equal_the_host_entropy_pass(gpu_device):
    entries = [(jc.stream(name), "device") for name in rc.RESTART_NAMES]
    out = _launch(entries, gpu_device)
    _check(entries, out)


@pytest.mark.gpu
def test_decode_batch_device_entropy_equals_pillow(gpu_device):
    names = rc.RESTART_NAMES + ["16x16-ss2-q90-std-noise", "50x31-grey-q90-smooth"]     # the last two: no DRI, host pass
    payloads = [jc.stream(n) for n in names]
    got = dj.decode_batch(payloads, gpu_device, device_entropy=True)
    for name, p, g in zip(names, payloads, got):
        np.testing.assert_array_equal(g.cpu().numpy(), jc.pillow_pixels(p), err_msg=name)
    plain = dj.decode_batch(payloads, gpu_device)
    assert all((a == b).all() for a, b in zip(got, plain))


@pytest.mark.gpu
def test_mixed_batch_in_guarded_pools(gpu_device):
    """device-entropy samples, host-entropy samples (no DRI, and one WITH restart markers decoded on the host) and skipped
    ones of both kinds in one batch"""
    plan = [("37x53-ss2-rstblocks3", "device"), ("17x33-ss1-q90-std-noise", "host"), ("64x200-ss0-rstrows1", "skip"),
            ("50x31-grey-rstblocks3", "device"), ("37x53-ss0-q100-opt-noise", "skip"), ("64x200-grey-rstrows1", "device"),
            ("64x200-ss1-rstblocks3", "host"), ("1x1-grey-q90-smooth", "host"), ("16x16-ss2-rstblocks1", "device")]
    entries = [(jc.stream(n), m) for n, m in plan]
    out = _launch(entries, gpu_device)
    _check(entries, out)
    for k, (_, mode) in enumerate(entries):
        if mode == "host":                                      # the entropy launch left the host's coefficients alone
            ca, cn = out["cregions"][k]
            assert (out["coefs"][ca:ca + cn] == out["before"][ca:ca + cn]).all()


@pytest.mark.gpu
def test_edges(gpu_device):
    """a last segment shorter than the interval, one segment over the whole image, more than 8 segments, a segment that
    ends on a stuffed FF 00, images 1 to 6 pixels across, optimised tables, noise at quality 100"""
    streams = [rc.edge_stream(n) for n in rc.EDGE_NAMES] + [rc.stuffed_end_stream()]
    assert rc.ends_on_stuffed_byte(streams[-1])
    segs = {n: int(rc.indexed(rc.edge_stream(n))[1]["segments"]) for n in rc.EDGE_NAMES}
    assert segs["last-short"] == 2 and segs["one-segment"] == 1 and segs["many-segments"] == 23
    entries = [(p, "device") for p in streams]
    out = _launch(entries, gpu_device)
    _check(entries, out)


@pytest.mark.gpu
def test_segments_pass_the_grid_once(gpu_device):
    """1024 descriptors of one greyscale stream with an interval of one MCU: more segments than grid x block"""
    k = jc.kernel_constants("jpeg.hip", ["kTE", "kGridE", "kMaxB"])
    lanes = k["kTE"] * k["kGridE"]
    blocks = lanes // k["kMaxB"] + 1                            # per image: just past one trip of the grid
    bw = 12
    bh = -(-blocks // bw)
    payload = jc.encode(jc.image(11, 8 * bh, 8 * bw, "noise", 1), quality=90, restart_marker_blocks=1)
    info, scan, seg, host = rc.indexed(payload)
    B = k["kMaxB"]
    assert lanes < B * int(scan["segments"]) < 2 * lanes
    import torch
    samples, scans = np.zeros(B, dj.SAMPLE), np.zeros(B, dj.SCAN)
    for b in range(B):
        dj.fill_sample(samples[b], info, 64 + b * host.size, 0)
        scans[b] = scan
    scans["data_offset"], scans["first_segment"] = 0, 0         # every descriptor reads the same bytes and the same table
    a, nb = int(scan["data_offset"]), int(scan["data_bytes"])
    t = lambda x: torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(gpu_device)  # noqa: E731
    cdev = torch.full((128 + B * host.size,), FILL16, dtype=torch.int16, device=gpu_device)
    status = torch.empty(B, dtype=torch.int32, device=gpu_device)
    dj.entropy_decode_device(t(np.frombuffer(payload, np.uint8, nb, a)), t(samples), t(scans), t(seg).view(torch.int32), cdev, status)
    torch.cuda.synchronize(gpu_device)
    got = cdev.cpu().numpy()
    assert not status.cpu().numpy().any()
    assert (got[:64] == FILL16).all() and (got[-64:] == FILL16).all()
    assert (got[64:-64].reshape(B, host.size) == host[None]).all()


@pytest.mark.gpu
def test_bad_streams_leave_a_status_and_stay_inside(gpu_device):
    """streams the index accepts whose entropy data is bad: a flipped bit that yields an undefined code, and a segment cut
    short (the index adjusts the table).  Single-bit flips and cuts of these two streams are what tools/jpeg_huff_check.cpp
    ran under the host sanitizers; here the host build of the decode has rejected each before the device sees it."""
    base = jc.stream(rc.CHECKED_NAMES[1])
    flipped, segment = rc.flipped(base, 1)
    short = rc.cut_short(base, 4, 3)
    info = rc.indexed(base)[0]
    want = {}
    for k, bad in ((1, flipped), (3, short)):
        sc, sg = dj.scan_index(bad, info)                       # accepted by the index
        want[k] = rc.host_decode(bad, sc, sg)[0]
        assert want[k] != 0
    assert dj.status_parts(want[1]) == (dj.STATUS_CODES.index("a Huffman code that is not in its table"), segment)
    assert dj.status_parts(want[3])[1] == 4
    good = [jc.stream("37x53-ss2-rstblocks3"), jc.stream(rc.CHECKED_NAMES[0]), base]
    entries = [(good[0], "device"), (flipped, "device", base), (good[1], "device"), (short, "device", base), (good[2], "device")]
    out = _launch(entries, gpu_device)
    assert [int(s) for s in out["status"]] == [0, want[1], 0, want[3], 0]       # the host build's words, for those samples only
    _check(entries, out, bad=(1, 3))


@pytest.mark.gpu
def test_decode_batch_names_the_stream_and_the_code(gpu_device):
    base = jc.stream(rc.CHECKED_NAMES[1])
    flipped, segment = rc.flipped(base, 1)
    with pytest.raises(_lib.DspnError, match=r"stream 1: a Huffman code that is not in its table in restart interval %d \(status code 1\)" % segment):
        dj.decode_batch([base, flipped], gpu_device, device_entropy=True)


@pytest.mark.gpu
def test_encoder_round_trip_with_restart_rows(gpu_device):
    import torch
    shapes = [((37, 53), "4:2:0"), ((64, 200), "4:2:2"), ((21, 37), "4:4:4"), ((50, 31), "grey"), ((1, 1), "4:2:0")]
    ss = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
    for layout in ("4:2:0", "4:2:2", "4:4:4"):
        arrays = [jc.image(7 + k, h, w, "noise", 1 if l == "grey" else 3) for k, ((h, w), l) in enumerate(shapes) if l in (layout, "grey")]
        files = je.encode_batch([torch.from_numpy(a).to(gpu_device) for a in arrays], quality=92, subsampling=layout, restart_rows=1)
        for a, f in zip(arrays, files):
            want = jc.encode(a, quality=92, restart_marker_rows=1, **({} if a.ndim == 2 else {"subsampling": ss[layout]}))
            assert f == want, (layout, a.shape)
        decoded = dj.decode_batch(files, gpu_device, device_entropy=True)
        for f, d in zip(files, decoded):
            np.testing.assert_array_equal(d.cpu().numpy(), jc.pillow_pixels(f))
    with pytest.raises(ValueError, match="at most one"):
        je.encode_batch([torch.zeros(8, 8, 3, dtype=torch.uint8, device=gpu_device)], restart_interval=2, restart_rows=1)
    one = je.encode_batch([torch.from_numpy(arrays[0]).to(gpu_device)], quality=92, subsampling="4:4:4", restart_interval=3)
    assert one[0] == jc.encode(arrays[0], quality=92, subsampling=0, restart_marker_blocks=3)


# ---- iterators ------------------------------------------------------------------------------------------------------------
def _write_sources(root, n, g):
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "cityscapes", "SegmentationClass"))
    lines = []
    for i in range(n):
        hw = [(48, 96), (64, 128), (40, 72), (56, 120)][i % 4]
        yy, xx = np.mgrid[:hw[0], :hw[1]]
        chans = [127 + 100 * np.sin(xx / g.uniform(5, 15) + g.uniform(0, 3)) * np.cos(yy / g.uniform(5, 15)) for _ in range(3)]
        img = np.clip(np.stack(chans, -1) + g.normal(0, 6, hw + (3,)), 0, 255).astype(np.uint8)
        name = "JPEGImages/city_%06d_leftImg8bit.jpg" % i
        Image.fromarray(img).save(os.path.join(root, name), format="JPEG", quality=95, progressive=(i == 2))
        rows = np.full((10, 6), -1.0)
        for k in range(1 + i % 3):
            x0, y0 = g.uniform(0, .8), g.uniform(0, .8)
            rows[k] = [g.integers(0, 8), x0, y0, x0 + g.uniform(.01, .3), y0 + g.uniform(.01, .3), g.uniform(0, 1)]
        label = [2, 6] + rows.reshape(-1).tolist()
        lines.append("\t".join([str(i)] + ["%f" % v for v in label] + [name]) + "\n")
        seg = g.integers(0, 19, hw).astype(np.uint8)
        Image.fromarray(seg).save(os.path.join(root, "cityscapes", "SegmentationClass", "city_%06d_gtFine_labelTrainIds.png" % i))
    with open(os.path.join(root, "train.lst"), "w") as f:
        f.writelines(lines)


@pytest.fixture(scope="module")
def restart_records(tmp_path_factory, gpu_device):
    """eight records written by im2rec with a restart interval of 4 MCUs (one source is progressive: Pillow decodes it for
    the writer, the record it becomes is an ordinary restart stream)"""
    from dspnet_amd.dataset import im2rec
    root = str(tmp_path_factory.mktemp("restart_records"))
    _write_sources(root, 8, np.random.Generator(np.random.PCG64(19)))
    assert im2rec.write_records(os.path.join(root, "train"), root, quality=92, batch=3, device=gpu_device, restart_interval=4) == 8
    return os.path.join(root, "train.rec")


@pytest.mark.gpu
@pytest.mark.parametrize("enable_aug", [True, False])
def test_record_iterator_device_entropy_yields_the_same_batches(gpu_device, restart_records, enable_aug):
    import torch
    from dspnet_amd.dataset import iterator as it
    kw = dict(enable_aug=enable_aug, device=gpu_device, device_jpeg=True)
    a = it.MultiTaskRecordIter(restart_records, 4, (3, 64, 128), **kw)
    b = it.MultiTaskRecordIter(restart_records, 4, (3, 64, 128), device_entropy=True, **kw)
    seen = 0
    for epoch in range(2):
        while a.iter_next():
            (ba, fa), (bb, fb) = a.next(), b.next()
            assert fa == fb and torch.equal(ba.data[0], bb.data[0])
            assert torch.equal(ba.label[0], bb.label[0]) and torch.equal(ba.label[1], bb.label[1])
            seen += 4
        assert not b.iter_next()
        a.reset(); b.reset()
    assert seen == 16
    assert (a.jpeg_device_entropy, a.jpeg_fallbacks) == (0, 0) and (b.jpeg_device_entropy, b.jpeg_fallbacks) == (16, 0)
    with pytest.raises(ValueError, match="device_jpeg"):
        it.MultiTaskRecordIter(restart_records, 4, (3, 64, 128), device_entropy=True)


@pytest.mark.gpu
@pytest.mark.parametrize("is_train", [True, False])
def test_det_iterator_device_entropy_yields_the_same_batches(gpu_device, restart_records, tmp_path, is_train):
    """the records' JPEGs as files of an image list, plus one file without restart markers (host pass in the same batch)"""
    import torch
    from dspnet_amd.dataset import det_iterator as di
    from dspnet_amd.dataset import rand_sampler as rs
    from dspnet_amd.dataset import recordio
    root = str(tmp_path)
    rec = recordio.MXIndexedRecordIO(restart_records.replace(".rec", ".idx"), restart_records, "r")
    files = []
    for i in range(8):
        _, payload = recordio.unpack(rec.read_idx(i))
        assert dj.device_entropy_ok(dj.probe_info(payload)[1])
        files.append("r%d.jpg" % i)
        with open(os.path.join(root, files[-1]), "wb") as f:
            f.write(payload)
    rec.close()
    files.append("plain.jpg")
    with open(os.path.join(root, "plain.jpg"), "wb") as f:
        f.write(jc.stream("64x200-ss2-q90-std-smooth"))
    lines = []
    for k, name in enumerate(files):
        lab = np.array([[k % 8, .10, .15, .55, .70], [(k + 3) % 8, .45, .30, .92, .88]])
        lines.append("\t".join([str(k), "2", "5"] + ["{0:.4f}".format(x) for x in lab.ravel()] + [name]) + "\n")
    with open(os.path.join(root, "all.lst"), "w") as f:
        f.writelines(lines)
    db = di.ListImdb(os.path.join(root, "all.lst"), root)

    def batches(**kw):
        samplers = [rs.RandCropper(min_overlap=.1, min_scale=.3, max_scale=1., min_aspect_ratio=.5, max_aspect_ratio=2., max_trials=25)]
        itr = di.DetIter(db, 3, (3, 33, 41), mean_pixels=[123, 117, 104], rand_samplers=samplers, rand_mirror=True, shuffle=True,
                         rand_seed=233, is_train=is_train, device=gpu_device, device_jpeg=True, **kw)
        out = []
        while len(out) < 6:
            if not itr.iter_next():
                itr.reset()
            bt = itr.next()
            out.append((bt.data[0].cpu().clone(), list(itr.batch_indices)))
        return itr, out

    a, want = batches()
    b, got = batches(device_entropy=True)
    torch.cuda.synchronize()
    for (da, ia), (db_, ib) in zip(want, got):
        assert ia == ib and torch.equal(da, db_)
    assert a.jpeg_device_entropy == 0 and b.jpeg_device_entropy == 16 and b.jpeg_fallbacks == 0      # 18 images, 2 of them plain.jpg
