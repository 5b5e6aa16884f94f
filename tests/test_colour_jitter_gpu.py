"""dspn_colour_jitter_batch_u8 and its two iterator hooks on the GPU: every comparison is byte equality with the numpy
restatement of include/dspn_colour_jitter.h (tests/ref_colour_jitter.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ref_colour_jitter as ref
from dspnet_amd import _lib
from dspnet_amd.dataset import colour_jitter as cj
from dspnet_amd.dataset import det_iterator as di
from dspnet_amd.dataset import iterator as ri
from dspnet_amd.dataset import jpeg
from dspnet_amd.dataset import rand_sampler as rs
from dspnet_amd.dataset import recordio

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 61, 0xA5
SIZES = [(1, 1), (1, 5), (3, 1), (2, 3), (5, 7), (17, 33), (64, 64), (33, 130)]
PARAMS = ([(dh, 0, 0, 1024) for dh in (1, -1, 180, -180)] +
          [(0, dl, 0, 1024) for dl in (1, -1, 255, -255)] +
          [(0, 0, ds, 1024) for ds in (1, -1, 255, -255)] +
          [(7, -13, 21, 1024), (-18, 32, -32, 1024)] +                      # all three together
          [(0, 0, 0, g) for g in (0, 512, 1536, 4096)] +                     # gain alone; 4096 saturates
          [(5, 9, -20, 1300), (-3, -40, 11, 700)] +                         # shifts and gain
          [(0, 0, 0, 1024)])                                                # identity: untouched
TRAIN = cj.ColorJitter(random_hue_prob=0.5, random_saturation_prob=0.5, random_illumination_prob=0.5, random_contrast_prob=0.5)
MEAN = (123.68, 116.779, 103.939)


def _pool(images, lead=0):
    """lead guard bytes, then the images with GUARD guard bytes between them (none behind the last one: it ends with the
    pool) -> (pool, offsets)"""
    parts, offsets, at = [np.full(lead, GUARD_BYTE, np.uint8)], [], lead
    for k, im in enumerate(images):
        if k:
            parts.append(np.full(GUARD, GUARD_BYTE, np.uint8))
            at += GUARD
        offsets.append(at)
        parts.append(im.reshape(-1))
        at += im.size
    return np.concatenate(parts), offsets


def _smooth(gen, h, w, k=0):
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 3 + yy * 2 + 40 * k) % 256, (xx * yy // 7 + 90) % 256, (255 - xx - yy) % 256], axis=2)
    return np.clip(smooth + gen.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


# ---- 1. byte equality, every alignment, guards ----------------------------------------------------------------------
@pytest.mark.parametrize("lead", range(4))
def test_batch_equals_restatement_and_guards_stay(gpu_device, lead):
    gen = np.random.RandomState(41)
    images, params = [], []
    for p in PARAMS:
        for h, w in SIZES:
            im = gen.randint(0, 256, (h, w, 3)).astype(np.uint8)
            im.reshape(-1, 3)[::5] = gen.randint(0, 256)                    # greys among them
            images.append(im)
            params.append(p)
    pool, offsets = _pool(images, lead)
    want, _ = _pool([ref.jitter(im, *p) for im, p in zip(images, params)], lead)
    assert set(o % 4 for o, im in zip(offsets, images) if im.shape[:2] == (33, 130)) == {0, 1, 2, 3}
    assert want.shape == pool.shape and not np.array_equal(want, pool)
    pool_dev = torch.from_numpy(pool).to(gpu_device)
    keep = cj.apply(pool_dev, params, offsets, [im.shape[:2] for im in images])
    torch.cuda.synchronize()
    assert keep                                                             # what the caller holds until the launch has run
    got = pool_dev.cpu().numpy()
    assert np.array_equal(got, want)                                        # images, identity rows and guards alike


# ---- 2. every colour; more work items than the grid has workgroups ---------------------------------------------------
def test_every_colour(gpu_device):
    v = torch.arange(1 << 24, dtype=torch.int32, device=gpu_device)
    img = torch.stack([v >> 16, (v >> 8) & 255, v & 255], dim=1).to(torch.uint8).view(4096, 4096, 3)
    p = (7, -13, 21, 1300)
    from concurrent.futures import ThreadPoolExecutor
    rows = np.array_split(img.cpu().numpy(), 64)                            # blocks whose temporaries stay in the host's cache
    with ThreadPoolExecutor(8) as pool:                                     # numpy's loops release the GIL
        want = torch.from_numpy(np.concatenate(list(pool.map(lambda block: ref.jitter(block, *p), rows)))).to(gpu_device)
    (got,) = cj.jitter_images([img], [p])
    torch.cuda.synchronize()
    assert got.data_ptr() != img.data_ptr() and int(img[255, 4095, 2]) == 255      # a new tensor; the source is as it was
    wrong = int((got != want).any(dim=2).sum())
    assert wrong == 0, "%d of 2^24 colours differ" % wrong


# ---- 3. descriptors that cannot be trusted --------------------------------------------------------------------------
_INT_MIN, _INT_MAX = -(1 << 31), (1 << 31) - 1
BAD = {
    "offset_minus_1": dict(img_offset=-1), "offset_far_negative": dict(img_offset=-(1 << 40)),
    "offset_is_pool_size": dict(img_offset="pool"), "offset_one_past_fitting": dict(img_offset="fit+1"),
    "offset_huge": dict(img_offset=(1 << 62)), "offset_most_negative": dict(img_offset=-(1 << 63)),
    "height_width_int_max": dict(height=_INT_MAX, width=_INT_MAX), "height_int_max": dict(height=_INT_MAX),
    "zero_height": dict(height=0), "zero_width": dict(width=0), "zero_size": dict(height=0, width=0),
    "negative_height": dict(height=-1), "negative_sizes": dict(height=-5, width=-7),
    "dh_181": dict(dh=181), "dh_minus_181": dict(dh=-181), "dh_int_min": dict(dh=_INT_MIN),
    "dl_256": dict(dl=256), "dl_minus_256": dict(dl=-256), "ds_256": dict(ds=256), "ds_minus_256": dict(ds=-256),
    "ds_int_max": dict(ds=_INT_MAX), "gain_minus_1": dict(gain=-1), "gain_65536": dict(gain=65536),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_untrustworthy_descriptor_writes_nothing(gpu_device, case):
    gen = np.random.RandomState(42)
    images = [gen.randint(0, 256, (5, 7, 3)).astype(np.uint8) for _ in range(3)]
    pool, offsets = _pool(images, lead=3)
    params = [(3, -4, 5, 1100), (-6, 7, 8, 900), (9, 10, -11, 1200)]
    samples = cj.describe(params, offsets, [(5, 7)] * 3)
    for field, value in BAD[case].items():
        if value == "pool":
            value = pool.size
        elif value == "fit+1":
            value = pool.size - 5 * 7 * 3 + 1
        samples[field][1] = value
    want, _ = _pool([ref.jitter(images[0], *params[0]), images[1], ref.jitter(images[2], *params[2])], lead=3)
    pool_dev = torch.from_numpy(pool).to(gpu_device)
    cj.launch(pool_dev, torch.from_numpy(samples.view(np.uint8).reshape(-1)).to(gpu_device))
    torch.cuda.synchronize()
    assert np.array_equal(pool_dev.cpu().numpy(), want)                     # the neighbours are done, the rest is as it was


# ---- 4. the C ABI's argument checks; a stream of the caller's --------------------------------------------------------
def test_argument_checks_and_a_side_stream(gpu_device):
    lib = _lib.lib()
    fn = lib.dspn_colour_jitter_batch_u8
    img = np.random.RandomState(43).randint(0, 256, (9, 11, 3)).astype(np.uint8)
    pool_dev = torch.from_numpy(img.reshape(-1)).to(gpu_device)
    desc = cj.describe([(4, 5, 6, 1111)], [0], [(9, 11)]).view(np.uint8).reshape(-1)
    desc_dev = torch.from_numpy(np.concatenate([desc, desc])).to(gpu_device)
    P, D, nb = pool_dev.data_ptr(), desc_dev.data_ptr(), pool_dev.numel()
    assert fn(None, 0, None, 0, None) == 0 and fn(P, nb, None, 0, None) == 0       # n == 0: nothing is looked at
    assert fn(None, nb, D, 1, None) == -1 and b"null" in lib.dspn_last_error()
    assert fn(P, nb, None, 1, None) == -1 and b"null" in lib.dspn_last_error()
    assert fn(P, nb, D, -1, None) == -1 and b"negative" in lib.dspn_last_error()
    assert fn(P, -1, D, 1, None) == -1 and b"negative" in lib.dspn_last_error()
    assert fn(P, nb, D + 4, 1, None) == -1 and b"8-byte aligned" in lib.dspn_last_error()
    assert fn(P, nb, D, 65536, None) == -1 and b"65535" in lib.dspn_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(pool_dev.cpu().numpy().reshape(9, 11, 3), img)            # none of them launched
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    assert fn(P, nb, D, 1, ctypes.c_void_p(side.cuda_stream)) == 0
    side.synchronize()
    assert np.array_equal(pool_dev.cpu().numpy().reshape(9, 11, 3), ref.jitter(img, 4, 5, 6, 1111))
    with torch.cuda.stream(side):                                           # the front end takes the current stream
        (twice,) = cj.jitter_images([pool_dev.view(9, 11, 3)], [(0, 0, 0, 512)])
    side.synchronize()
    assert np.array_equal(twice.cpu().numpy(), ref.jitter(ref.jitter(img, 4, 5, 6, 1111), 0, 0, 0, 512))


# ---- 5. DetIter -----------------------------------------------------------------------------------------------------
def _samplers():
    crop = dict(min_scale=.3, max_scale=1., min_aspect_ratio=.5, max_aspect_ratio=2., max_trials=25)
    return [rs.RandCropper(min_overlap=o, **crop) for o in (.1, .3, .5, .7, .9)] + \
           [rs.RandPadder(min_scale=1., max_scale=4., min_aspect_ratio=.5, max_aspect_ratio=2., min_gt_scale=.05)]


def _write_list(root, images, ext, **save):
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    lines = []
    for k, im in enumerate(images):
        name = "im%d.%s" % (k, ext)
        Image.fromarray(im).save(os.path.join(root, name), **save)
        lab = np.array([[k % 8, .10, .15, .55, .70], [(k + 3) % 8, .45, .30, .92, .88], [(k + 5) % 8, .30, .05, .62, .40]][:2 + k % 2])
        lines.append("\t".join([str(k), "2", "5"] + ["{0:.4f}".format(x) for x in lab.ravel()] + [name]) + "\n")
    with open(os.path.join(root, "all.lst"), "w") as f:
        f.writelines(lines)
    return di.ListImdb(os.path.join(root, "all.lst"), root)


def _det_iter(db, dev, **kw):
    return di.DetIter(db, 4, (3, 33, 41), mean_pixels=list(MEAN), rand_samplers=_samplers(), rand_mirror=True, shuffle=True,
                      rand_seed=233, device=dev, **kw)


def _det_batches(it, count):
    """the first `count` delivered batches (an epoch here is one batch) -> [(data, label, indices)]"""
    out = []
    while len(out) < count:
        if not it.iter_next():
            it.reset()
        b = it.next()
        out.append((b.data[0].cpu().clone(), b.label[0].cpu().clone(), list(it.batch_indices)))
    return out


@pytest.mark.parametrize("device_jpeg", [False, True])
def test_det_iter_equals_unjittered_iter_over_jittered_files(gpu_device, tmp_path, device_jpeg):
    gen = np.random.RandomState(44)
    images = [_smooth(gen, 40 + 7 * k, 61 - 5 * k, k) for k in range(4)]
    if device_jpeg:
        db = _write_list(str(tmp_path / "src"), images, "jpg", quality=90)
        payloads = [open(db.image_path_from_index(k), "rb").read() for k in range(4)]
        decoded = jpeg.decode_batch(payloads, gpu_device)
    else:
        db = _write_list(str(tmp_path / "src"), images, "png")
    it = _det_iter(db, gpu_device, device_jpeg=device_jpeg, color_jitter=TRAIN, jitter_seed=77)
    got = _det_batches(it, 2)
    torch.cuda.synchronize()
    if device_jpeg:
        assert it.jpeg_fallbacks == 0
    draws = np.random.RandomState(77)
    cj.draw(TRAIN, 4, draws)                                                # the batch the constructor builds
    plain = _det_batches(_det_iter(db, gpu_device, device_jpeg=device_jpeg), 2)
    for j, (data, label, indices) in enumerate(got):
        params = cj.draw(TRAIN, 4, draws)
        assert (params != np.asarray(cj.IDENTITY)).any()
        by_image = {idx: params[slot] for slot, idx in enumerate(indices)}
        assert sorted(by_image) == [0, 1, 2, 3]
        if device_jpeg:
            order = sorted(by_image)
            jittered = [t.cpu().numpy() for t in cj.jitter_images([decoded[k] for k in order], [by_image[k] for k in order])]
        else:
            jittered = [ref.jitter(images[k], *by_image[k]) for k in range(4)]
        want = _det_batches(_det_iter(_write_list(str(tmp_path / ("ref%d" % j)), jittered, "png"), gpu_device), j + 1)[j]
        assert want[2] == indices and torch.equal(want[1], label)           # the geometry draws are not affected
        assert torch.equal(want[0], data)
        assert plain[j][2] == indices and torch.equal(plain[j][1], label) and not torch.equal(plain[j][0], data)


# ---- 6. MultiTaskRecordIter -----------------------------------------------------------------------------------------
def _write_records(root, images_bgr, gen):
    """records with PNG payloads (lossless), their label maps and the list; boxes as tests/test_record_iter.py draws them"""
    from PIL import Image
    os.makedirs(os.path.join(root, "cityscapes", "SegmentationClass"), exist_ok=True)
    rec = recordio.MXIndexedRecordIO(os.path.join(root, "train.idx"), os.path.join(root, "train.rec"), "w")
    lines = []
    for i, img in enumerate(images_bgr):
        h, w = img.shape[:2]
        boxes = np.full((10, 6), -1.0)
        x0, y0 = gen.uniform(0, .5, 3), gen.uniform(0, .5, 3)
        boxes[:3] = np.stack([gen.randint(0, 8, 3), x0, y0, x0 + gen.uniform(.2, .45, 3), y0 + gen.uniform(.2, .45, 3),
                              gen.uniform(0, 1, 3)], axis=1)
        label = np.concatenate([[2, 6], boxes.ravel()]).astype(np.float32)
        rec.write_idx(i, recordio.pack_img(recordio.IRHeader(0, label, i, 0), img, img_fmt=".png"))
        seg = gen.randint(0, 19, (h, w)).astype(np.uint8)
        Image.fromarray(seg).save(os.path.join(root, "cityscapes", "SegmentationClass", "city_%06d_gtFine_labelTrainIds.png" % i))
        lines.append("%d\tJPEGImages/city_%06d_leftImg8bit.jpg\n" % (i, i))
    rec.close()
    with open(os.path.join(root, "train.lst"), "w") as f:
        f.writelines(lines)
    return os.path.join(root, "train.rec")


def _record_epochs(itr, epochs=2):
    out = []
    for _ in range(epochs):
        while itr.iter_next():
            batch, _ = itr.next()
            out.append([t.cpu().clone() for t in (batch.data[0], batch.label[0], batch.label[1])])
        itr.reset()
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


def test_record_iter_jitter(gpu_device, tmp_path, monkeypatch):
    n, B, shape = 9, 4, (3, 32, 64)
    images = [_smooth(np.random.RandomState(50 + k), 48, 80, k) for k in range(n)]           # BGR, as pack_img takes them
    path = _write_records(str(tmp_path / "src"), images, np.random.RandomState(45))
    kw = dict(enable_aug=True, device=gpu_device, color_jitter=TRAIN, jitter_seed=78)
    itr = ri.MultiTaskRecordIter(path, B, shape, prefetch=True, **kw)
    # the tables: one per _reset_aug_params, from a stream of their own (the constructor draws two, reset() one more)
    draws = np.random.RandomState(78)
    tables = [cj.draw(TRAIN, n, draws) for _ in range(4)]
    assert np.array_equal(itr.jitter_params, tables[1])
    orders = [itr.index_table.copy()]
    got = []
    for epoch in range(2):
        while itr.iter_next():
            batch, _ = itr.next()
            got.append([t.cpu().clone() for t in (batch.data[0], batch.label[0], batch.label[1])])
        itr.reset()
        orders.append(itr.index_table.copy())
        assert np.array_equal(itr.jitter_params, tables[2 + epoch])
    torch.cuda.synchronize()
    assert len(got) == 4
    # prefetch on or off: the same batches over two epochs and a reset()
    assert _same(got, _record_epochs(ri.MultiTaskRecordIter(path, B, shape, prefetch=False, **kw)))
    # an un-jittered iterator over records whose pixels the restatement jittered, epoch by epoch
    plain = _record_epochs(ri.MultiTaskRecordIter(path, B, shape, enable_aug=True, device=gpu_device))
    assert not _same(got, plain) and all(torch.equal(g[1], p[1]) and torch.equal(g[2], p[2]) for g, p in zip(got, plain))
    for epoch in range(2):
        table, order = tables[1 + epoch], orders[epoch]
        jittered = list(images)
        for slot in range(n):                                               # slot -> the record shown there this epoch
            rgb = ref.jitter(images[order[slot]][:, :, ::-1], *table[slot])
            jittered[order[slot]] = np.ascontiguousarray(rgb[:, :, ::-1])
        want = _record_epochs(ri.MultiTaskRecordIter(_write_records(str(tmp_path / ("ref%d" % epoch)), jittered,
                                                                    np.random.RandomState(45)), B, shape, enable_aug=True,
                                                     device=gpu_device), epoch + 1)
        assert _same(got[2 * epoch:2 * epoch + 2], want[2 * epoch:2 * epoch + 2])
    # enable_aug=False never jitters
    calls = []
    real = cj.apply
    monkeypatch.setattr(cj, "apply", lambda *a, **k: calls.append(1) or real(*a, **k))
    off = ri.MultiTaskRecordIter(path, B, shape, enable_aug=False, device=gpu_device, color_jitter=TRAIN, jitter_seed=78)
    assert off.jitter_params is None
    assert _same(_record_epochs(off), _record_epochs(ri.MultiTaskRecordIter(path, B, shape, enable_aug=False, device=gpu_device)))
    assert calls == []
    # the flat keys of **cfg.train stay ignored: only the explicit argument switches the feature on
    flat = ri.MultiTaskRecordIter(path, B, shape, enable_aug=True, device=gpu_device, **TRAIN._asdict())
    assert flat.jitter_params is None and _same(_record_epochs(flat), plain) and calls == []
    on = ri.MultiTaskRecordIter(path, B, shape, prefetch=False, **kw)
    on.next()
    assert calls


# ---- 7. off means off -----------------------------------------------------------------------------------------------
def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_off_means_off(gpu_device, tmp_path, monkeypatch):
    gen = np.random.RandomState(46)
    db = _write_list(str(tmp_path / "src"), [_smooth(gen, 40 + 7 * k, 61 - 5 * k, k) for k in range(4)], "png")
    calls = []
    real = cj.apply
    monkeypatch.setattr(cj, "apply", lambda *a, **k: calls.append(1) or real(*a, **k))
    runs = {}
    for name, kw in (("none", {}), ("zero", dict(color_jitter=cj.ColorJitter(), jitter_seed=5)),
                     ("eval", dict(color_jitter=TRAIN, is_train=False))):
        it = _det_iter(db, gpu_device, **kw)
        batches = _det_batches(it, 2) if name != "eval" else None
        runs[name] = (batches, np.random.get_state())
        assert it._jitter is None and it._jitter_rs is None
    assert calls == []                                                      # never entered
    for a, b in zip(runs["none"][0], runs["zero"][0]):
        assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert _state_equal(runs["none"][1], runs["zero"][1])
    # ... and with the feature on the global stream is where it is without it: the jitter draws are private
    it = _det_iter(db, gpu_device, color_jitter=TRAIN, jitter_seed=5)
    _det_batches(it, 2)
    assert calls and _state_equal(np.random.get_state(), runs["none"][1])
