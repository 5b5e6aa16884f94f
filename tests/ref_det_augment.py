"""numpy integer restatement of the arithmetic contract of include/dspn_det_augment.h, shared by
tests/test_det_iterator_host.py and tests/test_det_augment_gpu.py.  It reads the same descriptors and tables the launch
reads (det_iterator.pack_batch), so the packing is under test as well.

Per output (y, x) and channel c:
    xd  = mirror ? W - 1 - x : x
    acc = sum_j qy[y][j] * ( sum_i qx[xd][i] * P(clamp(fy[y] + j), clamp(fx[xd] + i)) )
    P   = image pixel at window origin + canvas position, `fill` where that lies outside the image
    v   = min(255, max(0, (acc + (1 << 21)) >> 22))
    out = float32(float64(v) - mean[c])"""
import numpy as np


def unpack_table(tables, offset, n, k):
    """-> (first int64[n], coef int64[n, k]) of the table at `offset` ints: n first-indices, then n * k int16"""
    first = tables[offset:offset + n].astype(np.int64)
    count = (n * k + 1) // 2
    coef = tables[offset + n:offset + n + count].view(np.int16)[:n * k].reshape(n, k).astype(np.int64)
    return first, coef


def canvas(image, x0, y0, cw, ch, fill):
    """the (ch, cw, 3) window of `image` whose origin is (x0, y0) in image coordinates, `fill` outside the image"""
    h, w = image.shape[:2]
    out = np.full((ch, cw, 3), fill, np.int64)
    ys, xs = np.arange(ch) + y0, np.arange(cw) + x0
    yin, xin = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    out[np.ix_(yin, xin)] = image[np.ix_(ys[yin], xs[xin])]
    return out


def resample(can, fx, qx, fy, qy):
    """the separable integer resize of an int64 (ch, cw, 3) canvas -> int64 acc (H, W, 3), before shift and clamp"""
    ch, cw = can.shape[:2]
    xi = np.clip(fx[:, None] + np.arange(qx.shape[1])[None, :], 0, cw - 1)          # (W, kx)
    rows = (can[:, xi, :] * qx[None, :, :, None]).sum(axis=2)                       # (ch, W, 3)
    assert np.abs(rows).max() < 2 ** 31, "the row sums are int32 in the contract"
    yi = np.clip(fy[:, None] + np.arange(qy.shape[1])[None, :], 0, ch - 1)          # (H, ky)
    return (rows[yi] * qy[:, :, None, None]).sum(axis=1)                            # (H, W, 3)


def augment_one(image, s, tables, H, W, mean):
    """one sample: image (src_h, src_w, 3) uint8, s its descriptor record -> (3, H, W) float32"""
    fx, qx = unpack_table(tables, int(s["xtab"]), W, int(s["kx"]))
    fy, qy = unpack_table(tables, int(s["ytab"]), H, int(s["ky"]))
    can = canvas(image.astype(np.int64), int(s["x0"]), int(s["y0"]), int(s["canvas_w"]), int(s["canvas_h"]), int(s["fill"]))
    acc = resample(can, fx, qx, fy, qy)
    v = np.clip((acc + (1 << 21)) >> 22, 0, 255)
    if s["mirror"]:
        v = v[:, ::-1]
    out = v.astype(np.float64) - np.asarray(mean, np.float64)[None, None, :]
    return np.ascontiguousarray(out.transpose(2, 0, 1)).astype(np.float32)


def augment_batch(pool, samples, tables, H, W, mean):
    """pool: the uint8 byte pool the descriptors index -> (len(samples), 3, H, W) float32"""
    out = np.zeros((len(samples), 3, H, W), np.float32)
    for k, s in enumerate(samples):
        n = int(s["src_h"]) * int(s["src_w"]) * 3
        image = pool[int(s["img_offset"]):int(s["img_offset"]) + n].reshape(int(s["src_h"]), int(s["src_w"]), 3)
        out[k] = augment_one(image, s, tables, H, W, mean)
    return out


def augment_images(images, windows, methods, mirrors, H, W, mean, fill=128):
    """convenience over det_iterator.pack_batch: a list of (h, w, 3) uint8 arrays with their windows (x0, y0, w, h; None =
    the whole image), methods and mirror flags -> (pool, samples, tables, expected (B, 3, H, W) float32)"""
    from dspnet_amd.dataset import det_iterator as di
    plans, offset = [], 0
    for im, win, method, mirror in zip(images, windows, methods, mirrors):
        h, w = im.shape[:2]
        plans.append({"src_w": w, "src_h": h, "img_offset": offset, "window": win or (0, 0, w, h), "method": method,
                      "mirror": mirror, "fill": fill})
        offset += im.size
    samples, tables = di.pack_batch(plans, H, W)
    pool = np.concatenate([np.ascontiguousarray(im, np.uint8).reshape(-1) for im in images])
    return pool, samples, tables, augment_batch(pool, samples, tables, H, W, mean)


def device_batch_on_host(self, prep):
    """stands in for DetIter._device_batch: the same descriptors, tables and (Pillow-decoded) pixel pool through the
    restatement -> (B, 3, H, W) float32 on the CPU; slots past the samples of `prep` stay zero"""
    import torch
    H, W = self._data_shape
    out = np.zeros((self.batch_size, 3, H, W), np.float32)
    n = prep["count"]
    out[:n] = augment_batch(prep["pixels"].numpy(), prep["samples"], prep["tables"], H, W, self._mean_pixels)
    return torch.from_numpy(out)
