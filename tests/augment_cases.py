"""The descriptor plumbing of one dspn_augment_batch_u8 call and its reference (oracle/augment.py: warp_affine and
finish_sample), shared by tests/test_record_iter.py and tests/test_pipeline_edges_gpu.py."""
import ctypes as c

import numpy as np

from dspnet_amd.dataset import iterator as it
from oracle import augment as oa

MEAN = [123.68, 116.779, 103.939]


def run_batch(dev, imgs, segs, Ms, H, W, flips, borders, no_seg=(), lut=None, mean=MEAN):
    """one call of the C entry over BGR images (h, w, 3) and label maps (h, w) of any sizes.  Ms: forward 2 x 3 affines;
    borders: per sample (image border, label border); no_seg: samples whose seg_offset is -1; lut: (256,) uint8 or None
    -> (data (B, 3, H, W), labels (B, H / 4, W / 4), the descriptors)"""
    import torch
    from dspnet_amd import _lib
    B = len(imgs)
    samples = np.zeros(B, it._SAMPLE)
    io, so = 0, 0
    for b, im in enumerate(imgs):
        samples[b] = (io, -1 if b in no_seg else so, im.shape[0], im.shape[1], int(flips[b]), borders[b][0], borders[b][1], 0,
                      it.invert_affine(Ms[b]))
        io += im.size
        so += segs[b].size
    ipool = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(dev)
    spool = torch.from_numpy(np.concatenate([s.reshape(-1) for s in segs])).to(dev)
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    ldev = None if lut is None else torch.from_numpy(lut).to(dev)
    data = torch.empty(B, 3, H, W, device=dev)
    seg_out = torch.empty(B, H // 4, W // 4, device=dev)
    _lib.check(it._entry()(ipool.data_ptr(), spool.data_ptr(), desc.data_ptr(), B, H, W, it._CMAP_BGR, (c.c_double * 3)(*mean),
                           0 if ldev is None else ldev.data_ptr(), data.data_ptr(), seg_out.data_ptr(),
                           torch.cuda.current_stream(dev).cuda_stream), "augment")
    return data.cpu().numpy(), seg_out.cpu().numpy(), samples


def oracle_sample(img, seg, M, H, W, flip, border, has_seg=True, lut=None, mean=MEAN):
    """what the call yields for one sample -> (data (3, H, W) float32, labels (H / 4, W / 4) float32)"""
    w = oa.warp_affine(img, np.array(M).reshape(2, 3), (W, H), True, int(border[0]))
    ws = oa.warp_affine(seg, np.array(M).reshape(2, 3), (W, H), False, int(border[1]))
    if flip:
        w, ws = w[:, ::-1], ws[:, ::-1]
    table = np.arange(256, dtype=np.float64) if lut is None else lut.astype(np.float64)
    d, q = oa.finish_sample(w, ws, (3, H, W), mean, table)
    return d, (q if has_seg else np.zeros_like(q))
