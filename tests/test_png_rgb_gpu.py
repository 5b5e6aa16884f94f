"""Device half of the colour PNG decode (dspn_png_rgb_batch) and its front ends (decode_rgb_batch, im2rec, DetIter's
device_png=True): the RGB bytes equal Pillow's convert("RGB") byte for byte at every filter stride (3, 4, 6 and 8 bytes next
to the 1 and 2 of tests/test_png_gpu.py), at the row lengths on each side of a dword edge, at wave and band edges, for
packed rows and palettes; nothing is written outside an image's output; descriptors that lie are left alone."""
import io
import os

import numpy as np
import pytest

import ref_png as rp
import ref_png_rgb as rr
from dspnet_amd import _lib
from dspnet_amd.dataset import det_iterator as di
from dspnet_amd.dataset import png as dp

HEIGHTS = (1, 2, 64, 65, 1024, 1025)
WIDTHS = (1, 2, 3, 4, 5, 6, 70)
KINDS = (0, 1, 2, 3, 4, "mix")
STRIDES = {3: (2, 8), 4: (6, 8), 6: (2, 16), 8: (6, 16)}        # filter stride -> the (colour type, depth) that has it
PAD, GUARD = 256, 61
_cache = {}


def _case(g, h, w, colour, depth, kind, values=None, **kw):
    data = rr.write(rr.random_samples(g, h, w, colour, depth, values), colour, depth, rp.filters_for(g, h, kind), **kw)
    return ("%dx%d-c%d-d%d-%s%s" % (h, w, colour, depth, kind, "" if values is None else "-v%d" % len(values)), data, rr.pillow(data))


def geometry_cases():
    """[(name, payload, Pillow's RGB)], built once: per stride every width x filter kind with the heights dealt round and
    every height x filter kind with the widths dealt round; random, two-valued and constant images in turn (the last two
    make Paeth ties)"""
    if "geometry" in _cache:
        return _cache["geometry"]
    g = np.random.Generator(np.random.PCG64(78))
    shapes, k = [], 0
    for bpp in STRIDES:
        for w in WIDTHS:
            for kind in KINDS:
                shapes.append((HEIGHTS[k % len(HEIGHTS)], w, bpp, kind)); k += 1
        for h in HEIGHTS:
            for kind in KINDS:
                shapes.append((h, WIDTHS[k % len(WIDTHS)], bpp, kind)); k += 5
    out = []
    for n, (h, w, bpp, kind) in enumerate(shapes):
        colour, depth = STRIDES[bpp]
        top = 2 ** depth - 1
        values = (None, (3, top - 2), (top // 3,))[n % 3]
        out.append(_case(g, h, w, colour, depth, kind, values, idat_chunks=1 + n % 3))
    _cache["geometry"] = out
    return out


def packed_cases():
    """depths 1, 2 and 4, greyscale and palette, at widths around the samples per byte, every filter kind; palette 8-bit
    with a short PLTE; and the whole-byte formats the geometry cases leave out (grey 8, grey + alpha 8 and 16)"""
    if "packed" in _cache:
        return _cache["packed"]
    g = np.random.Generator(np.random.PCG64(79))
    out, k = [], 0
    for depth in (1, 2, 4):
        for colour in (0, 3):
            for w in (1, 7, 8, 9, 17):
                for kind in KINDS:
                    kw = dict(plte_entries=(2 ** depth, 2, 1)[k % 3], trns=bool(k % 2)) if colour == 3 else dict(trns=bool(k % 2))
                    out.append(_case(g, (5, 66, 3)[k % 3], w, colour, depth, kind, **kw)); k += 1
    for entries in (256, 5, 1):
        out.append(_case(g, 66, 19, 3, 8, "mix", plte_entries=entries))
    for colour, depth in ((0, 8), (4, 8), (4, 16)):
        for kind in KINDS:
            out.append(_case(g, (65, 7)[k % 2], (5, 33)[k % 2], colour, depth, kind, trns=bool(k % 3)))
            k += 1
    _cache["packed"] = out
    return out


class _Run(object):
    """one dspn_png_rgb_batch call over `picked`.  Every pool is the inside of a larger tensor of 0xA5 (PAD bytes on either
    side, so an offset a little outside a pool is still inside the test's memory), the images lie GUARD bytes apart in all
    three pools, so raw, workspace and output offsets take every residue mod 4."""

    def __init__(self, picked, dev, skip=(), spoil=None, guard=GUARD, ws_cut=0, extra_palettes=1):
        import torch
        infos = [dp.probe_rgb(data) for _, data, _ in picked]
        s = self.samples = np.zeros(len(picked), dp.RGB_SAMPLE)
        raw = np.full(2 * PAD + sum(i["raw_bytes"] + guard for i in infos) + guard, 0x5A, np.uint8)
        ro = wo = oo = 0
        self.out_regions, self.ws_regions, palettes = [], [], []
        for k, ((name, data, _), info) in enumerate(zip(picked, infos)):
            ro, wo, oo = ro + guard, wo + guard, oo + guard
            assert info["supported"] and dp.inflate_into(data, info, raw[PAD + ro:PAD + ro + info["raw_bytes"]]) == 0, name
            direct = (info["colour_type"], info["bit_depth"]) == (2, 8)
            s[k]["raw_offset"], s[k]["recon_offset"], s[k]["out_offset"] = ro, -1 if direct else wo, oo
            for f in ("width", "height", "bit_depth", "colour_type"):
                s[k][f] = info[f]
            s[k]["skip"] = int(k in skip)
            s[k]["palette_index"] = -7
            if info["colour_type"] == 3:
                s[k]["palette_index"] = len(palettes)
                palettes.append(info["palette"].ljust(dp.PALETTE_BYTES, b"\0"))
            n, m = info["height"] * info["width"] * 3, 0 if direct else info["height"] * info["row_bytes"]
            self.out_regions.append((oo, n))
            self.ws_regions.append((wo, m))
            ro, wo, oo = ro + info["raw_bytes"], wo + m, oo + n
        self.raw_bytes, self.ws_bytes, self.out_bytes = ro + guard, wo + guard - ws_cut, oo + guard
        self.n_palettes = len(palettes)
        palettes += [b"\x77" * dp.PALETTE_BYTES] * extra_palettes       # beyond the declared count
        assert dp.rgb_workspace_bytes(s) <= self.ws_bytes + ws_cut
        if spoil:
            spoil(s, self)
        out = torch.full((2 * PAD + self.out_bytes,), 0xA5, dtype=torch.uint8, device=dev)
        ws = torch.full((2 * PAD + self.ws_bytes + ws_cut,), 0xA5, dtype=torch.uint8, device=dev)
        raw_dev = torch.from_numpy(raw).to(dev)
        desc = torch.from_numpy(s.view(np.uint8).reshape(-1).copy()).to(dev)
        pal = torch.from_numpy(np.frombuffer(b"".join(palettes), np.uint8).copy()).to(dev)
        lib = _lib.lib()
        self.rc = lib.dspn_png_rgb_batch(raw_dev.data_ptr() + PAD, self.raw_bytes, desc.data_ptr(), len(picked), pal.data_ptr(),
                                         self.n_palettes, out.data_ptr() + PAD, self.out_bytes, ws.data_ptr() + PAD, self.ws_bytes,
                                         torch.cuda.current_stream(dev).cuda_stream)
        self.error = lib.dspn_last_error()
        torch.cuda.synchronize(dev)
        self.out, self.ws = out.cpu().numpy(), ws.cpu().numpy()

    def check(self, picked, untouched=()):
        """every image not in `untouched` equals Pillow; those, and every byte outside the images in the output tensor and
        outside the reconstructed rows in the workspace tensor, are as they were"""
        assert self.rc == 0, self.error
        covered = np.zeros(self.out.size, bool)
        for k, ((name, _, want), (at, n)) in enumerate(zip(picked, self.out_regions)):
            got = self.out[PAD + at:PAD + at + n]
            if k in untouched:
                assert (got == 0xA5).all(), "image %d (%s) was written" % (k, name)
                continue
            covered[PAD + at:PAD + at + n] = True
            np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=name)
        assert (self.out[~covered] == 0xA5).all(), "a byte outside the images' outputs was written"
        scratch = np.zeros(self.ws.size, bool)
        for k, (at, m) in enumerate(self.ws_regions):
            if k not in untouched:
                scratch[PAD + at:PAD + at + m] = True
        assert (self.ws[~scratch] == 0xA5).all(), "a workspace byte outside the reconstructed rows was written"


# ---- kernel geometry ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("part", range(3))
def test_every_stride_equals_pillow(gpu_device, part):
    """three batched calls, each a third of the matrix dealt round-robin, so every call mixes strides, sizes and filter
    types"""
    picked = geometry_cases()[part::3]
    assert len(picked) >= 100
    run = _Run(picked, gpu_device)
    for regions in (run.out_regions, run.ws_regions):
        assert {at % 4 for at, n in regions if n} == {0, 1, 2, 3}
    assert {int(o) % 4 for o in run.samples["raw_offset"]} == {0, 1, 2, 3}
    run.check(picked)


def test_geometry_cases_cover_the_matrix():
    seen = set()
    for name, data, want in geometry_cases():
        info = dp.probe_rgb(data)
        filters = set(np.frombuffer(rr.header(data)[5], np.uint8)[0::info["row_bytes"] + 1].tolist())
        seen.add((info["bytes_per_pixel"], info["width"], info["height"], tuple(sorted(filters)) if len(filters) > 1 else filters.pop()))
    for bpp in STRIDES:
        assert {w for b, w, h, f in seen if b == bpp} == set(WIDTHS) and {h for b, w, h, f in seen if b == bpp} == set(HEIGHTS)
        for f in range(5):
            assert {w for b, w, h, k in seen if b == bpp and k == f} == set(WIDTHS)
            assert {h for b, w, h, k in seen if b == bpp and k == f} == set(HEIGHTS)
        assert any(isinstance(k, tuple) for b, w, h, k in seen if b == bpp)


# ---- packed rows and palettes ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_packed_rows_and_palettes_equal_pillow(gpu_device):
    picked = packed_cases()
    assert len(picked) == 180 + 3 + 18
    _Run(picked, gpu_device).check(picked)


# ---- guards ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_guard_bytes_and_skip(gpu_device):
    picked = geometry_cases()[::23] + packed_cases()[::17]
    assert len(picked) >= 20
    skip = {1, 5, len(picked) - 1}
    _Run(picked, gpu_device, skip=skip, guard=64).check(picked, untouched=skip)


@pytest.mark.gpu
def test_all_rgb8_batch_needs_no_workspace(gpu_device):
    picked = [c for c in geometry_cases() if "-c2-d8-" in c[0]][:9]
    run = _Run(picked, gpu_device)
    assert dp.rgb_workspace_bytes(run.samples) == 0
    run.check(picked)


# ---- untrustworthy descriptors --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_untrustworthy_descriptors_write_nothing(gpu_device):
    """offsets a little outside each pool (inside the padding of the test's tensors), a height whose products wrap 32 bits,
    pairs that are not on this path, palette indices out of range: the image is left alone, its neighbours are decoded"""
    small = [c for c in geometry_cases() if c[2].shape[0] <= 65]
    rgb8 = [c for c in small if "-c2-d8-" in c[0]][:4]
    rgba16 = [c for c in small if "-c6-d16-" in c[0]][:6]
    pal = [c for c in packed_cases() if "-c3-" in c[0]][:3]
    grey = [c for c in packed_cases() if "-c0-d8-" in c[0]][:2]
    picked = rgb8 + rgba16 + pal + grey + small[-3:]
    bad = set(range(15))

    def spoil(s, run):
        s[0]["raw_offset"] = -1
        s[1]["out_offset"] = -8
        s[2]["out_offset"] = run.out_bytes - 2                  # its last bytes past the output pool
        s[3]["height"] = (1 << 30) + 1                          # height * (row_bytes + 1) = 4 rows' worth mod 2^32 (width 1: 3 + 1)
        s[3]["width"] = 1
        s[4]["raw_offset"] = run.raw_bytes - 3                  # past the raw pool
        s[5]["recon_offset"] = -4
        s[6]["recon_offset"] = run.ws_bytes - 5                 # past the workspace
        s[7]["bit_depth"] = 4                                   # RGBA at 4 bits
        s[8]["colour_type"] = 5
        s[9]["colour_type"], s[9]["bit_depth"] = 0, 16          # 16-bit greyscale is not on this path
        s[10]["palette_index"] = run.n_palettes                 # one past the tables
        s[11]["palette_index"] = -1
        s[12]["palette_index"] = 0x7fffffff
        s[13]["width"] = s[13]["height"] = 0x7fffffff           # the products overflow 63 bits
        s[14]["height"] = 0

    assert len(picked) == 18
    run = _Run(picked, gpu_device, spoil=spoil)
    run.check(picked, untouched=bad)


@pytest.mark.gpu
def test_workspace_too_small_leaves_those_images_alone(gpu_device):
    """the entry cannot read the descriptors (device memory): a workspace that ends before an image's reconstructed rows
    makes the device refuse that image alone; the bytes behind the declared workspace stay as they were"""
    picked = [c for c in geometry_cases() if "-c6-d16-" in c[0] and c[2].shape[0] <= 65][:5]
    run = _Run(picked, gpu_device, ws_cut=GUARD + 1)             # the last image's rows end one byte past it
    run.check(picked, untouched={4})


# ---- front ends -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rgb_batch_argument_checks(gpu_device):
    import torch
    lib = _lib.lib()
    t = torch.full((1024,), 0xA5, dtype=torch.uint8, device=gpu_device)
    p = t.data_ptr()
    call = lib.dspn_png_rgb_batch
    good = (p, 64, p, 1, p, 1, p, 64, p, 64, None)

    def with_(i, v):
        return good[:i] + (v,) + good[i + 1:]

    for i in (0, 2, 6):
        assert call(*with_(i, None)) == -1 and b"null argument" in lib.dspn_last_error()
    assert call(*with_(4, None)) == -1 and b"null palettes" in lib.dspn_last_error()
    assert call(*with_(8, None)) == -1 and b"null workspace" in lib.dspn_last_error()
    for i in (1, 3, 5, 7, 9):
        assert call(*with_(i, -1)) == -1 and b"negative" in lib.dspn_last_error()
    assert call(*with_(2, p + 4)) == -1 and b"aligned" in lib.dspn_last_error()
    assert call(None, 0, None, 0, None, 0, None, 0, None, 0, None) == 0     # an empty batch is a no-op
    torch.cuda.synchronize(gpu_device)
    assert (t.cpu() == 0xA5).all()


@pytest.mark.gpu
def test_decode_rgb_batch_equals_pillow(gpu_device):
    import torch
    g = np.random.Generator(np.random.PCG64(80))
    picked = [_case(g, 9 + k, 13 - k % 5, colour, depth, "mix", trns=bool(k % 2)) for k, (colour, depth) in enumerate(rr.PAIRS)]
    picked += geometry_cases()[7::41]
    got = dp.decode_rgb_batch([c[1] for c in picked], gpu_device)
    assert len(got) == len(picked) and dp.decode_rgb_batch([], gpu_device) == []
    base = got[0].untyped_storage().data_ptr()
    for (name, _, want), t in zip(picked, got):
        assert t.dtype == torch.uint8 and tuple(t.shape) == want.shape and t.device == torch.device(gpu_device), name
        assert t.untyped_storage().data_ptr() == base, "views of one pool"
        np.testing.assert_array_equal(t.cpu().numpy(), want, err_msg=name)


@pytest.mark.gpu
def test_decode_rgb_batch_names_the_reason(gpu_device):
    good = geometry_cases()[0][1]
    with pytest.raises(ValueError, match="stream 1 .*interlace"):
        dp.decode_rgb_batch([good, rp.write_interlaced(np.zeros((9, 9), np.uint8))], gpu_device)
    with pytest.raises(ValueError, match="stream 2 .*16-bit greyscale"):
        dp.decode_rgb_batch([good, good, rp.write(np.zeros((3, 3), np.uint16), [0] * 3)], gpu_device)
    with pytest.raises(_lib.DspnError, match="stream 1"):
        dp.decode_rgb_batch([good, good[:-12]], gpu_device)
    parts = list(rp.chunks(good))
    spoiled = rp.SIGNATURE + b"".join(rp.chunk(k, b"\x00\x01" + d[2:] if k == b"IDAT" else d) for k, d in parts)
    with pytest.raises(_lib.DspnError, match="png_inflate .stream 1."):
        dp.decode_rgb_batch([good, spoiled], gpu_device)


def _smooth(g, h, w):
    yy, xx = np.mgrid[:h, :w]
    chans = [127 + 100 * np.sin(xx / g.uniform(5, 15) + g.uniform(0, 3)) * np.cos(yy / g.uniform(5, 15)) for _ in range(3)]
    return np.clip(np.stack(chans, -1) + g.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def _write_files(root, g):
    """a tiny mixed image set -> [(file name, is the one interlaced PNG)]: PNGs as RGB 8 (Pillow's writer and ours), RGBA 8,
    palette 4-bit, greyscale 8, RGB 16 and one interlaced; JPEGs baseline and progressive"""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    files = []

    def put(name, data):
        with open(os.path.join(root, name), "wb") as f:
            f.write(data)
        files.append(name)

    def pillow_bytes(arr, **kw):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, **kw)
        return buf.getvalue()

    put("a.png", pillow_bytes(_smooth(g, 40, 61), format="PNG"))
    put("b.jpg", pillow_bytes(_smooth(g, 47, 56), format="JPEG", quality=90))
    put("c.png", rr.write(_smooth(g, 33, 45), 2, 8, rp.filters_for(g, 33, "mix")))
    put("d.png", rr.write(rr.random_samples(g, 38, 51, 6, 8), 6, 8, rp.filters_for(g, 38, "mix")))
    put("e.jpg", pillow_bytes(_smooth(g, 54, 51), format="JPEG", quality=90, progressive=True))
    put("f.png", rr.write(rr.random_samples(g, 45, 37, 3, 4), 3, 4, rp.filters_for(g, 45, "mix"), plte_entries=11))
    put("g.png", rp.write_interlaced(_smooth(g, 36, 44)[:, :, 0].copy()))
    put("h.png", rr.write(rr.random_samples(g, 41, 39, 2, 16), 2, 16, rp.filters_for(g, 41, "mix")))
    put("i.png", pillow_bytes(_smooth(g, 35, 48)[:, :, 1].copy(), format="PNG"))
    return files


@pytest.mark.gpu
def test_write_records_decodes_png_sources_on_the_device(gpu_device, tmp_path, monkeypatch):
    """the records over PNG and JPEG sources equal the ones written with every PNG forced through Pillow, and the PNGs that
    probe_rgb supports went through decode_rgb_batch, not Pillow"""
    from dspnet_amd.dataset import im2rec
    root = str(tmp_path)
    files = _write_files(os.path.join(root, "img"), np.random.Generator(np.random.PCG64(31)))
    for prefix in ("dev", "host"):
        with open(os.path.join(root, prefix + ".lst"), "w") as f:
            f.writelines("%d\t%f\t%f\timg/%s\n" % (k, k % 3, k * .5, name) for k, name in enumerate(files))
    calls, real = [], dp.decode_rgb_batch

    def counted(payloads, device):
        calls.append(len(payloads))
        return real(payloads, device)

    monkeypatch.setattr(dp, "decode_rgb_batch", counted)
    assert im2rec.write_records(os.path.join(root, "dev"), root, quality=92, batch=4, device=gpu_device) == len(files)
    supported = [name.endswith(".png") and name != "g.png" for name in files]
    assert calls == [sum(supported[k:k + 4]) for k in range(0, len(files), 4)] and sum(calls) == 6
    monkeypatch.setattr(dp, "open_rgb", lambda content: None)      # every PNG through Pillow, as before
    assert im2rec.write_records(os.path.join(root, "host"), root, quality=92, batch=4, device=gpu_device) == len(files)
    assert sum(calls) == 6
    for ext in (".rec", ".idx"):
        with open(os.path.join(root, "dev" + ext), "rb") as a, open(os.path.join(root, "host" + ext), "rb") as b:
            assert a.read() == b.read()


def _imdb(root, files):
    lines = []
    for k, name in enumerate(files):
        lab = np.array([[k % 8, .10, .15, .55, .70], [(k + 3) % 8, .45, .30, .92, .88], [(k + 5) % 8, .30, .05, .62, .40]][:2 + k % 2])
        lines.append("\t".join([str(k), "2", "5"] + ["{0:.4f}".format(x) for x in lab.ravel()] + [name]) + "\n")
    with open(os.path.join(root, "all.lst"), "w") as f:
        f.writelines(lines)
    return di.ListImdb(os.path.join(root, "all.lst"), root)


def _batches(db, dev, is_train, count, **kw):
    from dspnet_amd.dataset import rand_sampler as rs
    crop = dict(min_scale=.3, max_scale=1., min_aspect_ratio=.5, max_aspect_ratio=2., max_trials=25)
    samplers = [rs.RandCropper(min_overlap=o, **crop) for o in (.1, .5, .9)] + \
               [rs.RandPadder(min_scale=1., max_scale=4., min_aspect_ratio=.5, max_aspect_ratio=2., min_gt_scale=.05)]
    it = di.DetIter(db, 3, (3, 33, 41), mean_pixels=[123, 117, 104], rand_samplers=samplers, rand_mirror=True, shuffle=True,
                    rand_seed=233, is_train=is_train, device=dev, **kw)
    out = []
    while len(out) < count:
        if not it.iter_next():
            it.reset()
        b = it.next()
        out.append((b.data[0].cpu().clone(), None if b.label[0] is None else b.label[0].cpu().clone(), list(it.batch_indices)))
    return it, out


@pytest.mark.gpu
@pytest.mark.parametrize("is_train", [True, False])
@pytest.mark.parametrize("device_jpeg", [False, True])
def test_det_iter_device_png_yields_the_same_batches(gpu_device, tmp_path, is_train, device_jpeg):
    """9 files, batches of 3, two epochs: the interlaced PNG falls back once per epoch, nothing else does"""
    import torch
    root = str(tmp_path)
    db = _imdb(root, _write_files(root, np.random.Generator(np.random.PCG64(32))))
    a, want = _batches(db, gpu_device, is_train, 6, device_jpeg=device_jpeg)
    b, got = _batches(db, gpu_device, is_train, 6, device_jpeg=device_jpeg, device_png=True)
    torch.cuda.synchronize()
    assert a.device_png is False and b.device_png is True
    for (da, la, ia), (db_, lb, ib) in zip(want, got):
        assert ia == ib and torch.equal(da, db_)
        assert (la is None and lb is None) if not is_train else torch.equal(la, lb)
    assert sorted(sum((i for _, _, i in got), [])) == sorted(list(range(9)) * 2)
    assert b.png_fallbacks == 2 and a.png_fallbacks == 0
    if device_jpeg:                                             # the progressive JPEG and the interlaced PNG; without
        assert b.jpeg_fallbacks == 4 and a.jpeg_fallbacks == 16    # device_png every PNG is Pillow's
    else:
        assert b.jpeg_fallbacks == 0 and a.jpeg_fallbacks == 0
