"""Colour jitter of both iterators on the device (include/dspn_colour_jitter.h): the `ColorJitter` settings of the
reference's config/config.py -- hue, saturation, illumination as integer shifts in 8-bit HLS, contrast as a gain -- applied
in place, by one launch per batch, to the decoded uint8 RGB pool that the crop / resize / warp launches read.

The reference hands these settings to MXNet's C++ detection augmenter, whose text is not in the reference; the semantics
follow its defaults as this project understands them and the per-pixel integers are this build's own (the header states
them; PARITY STATUS: unpinned).

  draw          the per-image parameters [dh, dl, ds, gain] from a RandomState of the caller's: host, pure
  apply         descriptors up, one launch over a pool; nothing at all when every row is the identity
  jitter_images the public use on a list of device images

DetIter(color_jitter=..., jitter_seed=...) and MultiTaskRecordIter(color_jitter=..., jitter_seed=...) draw from a
private RandomState, so the streams that drive their geometry are the same with the feature on or off."""
import collections

import numpy as np
import torch

from .. import _lib

# config/config.py of the reference: field names and defaults
ColorJitter = collections.namedtuple("ColorJitter", [
    "random_hue_prob", "max_random_hue", "random_saturation_prob", "max_random_saturation",
    "random_illumination_prob", "max_random_illumination", "random_contrast_prob", "max_random_contrast"])
ColorJitter.__new__.__defaults__ = (0.0, 18, 0.0, 32, 0.0, 32, 0.0, 0.5)

SAMPLE = _lib.layout("dspn_jitter_sample")                     # include/dspn_colour_jitter.h
UNIT_GAIN = 1024
IDENTITY = (0, 0, 0, UNIT_GAIN)


def _checked(cfg):
    """a ColorJitter or a dict with its keys -> a ColorJitter whose every draw the launch accepts"""
    if isinstance(cfg, dict):
        cfg = ColorJitter(**cfg)
    if not isinstance(cfg, ColorJitter):
        raise TypeError("color_jitter is None, a ColorJitter or a dict with its keys, got %r" % (cfg,))
    if not (0 <= int(cfg.max_random_hue) <= 180 and 0 <= int(cfg.max_random_saturation) <= 255 and
            0 <= int(cfg.max_random_illumination) <= 255 and 0 <= cfg.max_random_contrast <= 1):
        raise ValueError("color_jitter: max_random_hue is 0..180, max_random_saturation and max_random_illumination are "
                         "0..255, max_random_contrast is 0..1, got %r" % (cfg,))
    return cfg


def config(cfg):
    """None, a ColorJitter or a dict with its keys -> a ColorJitter, or None when nothing would ever be applied"""
    if cfg is None:
        return None
    cfg = _checked(cfg)
    probs = (cfg.random_hue_prob, cfg.random_saturation_prob, cfg.random_illumination_prob, cfg.random_contrast_prob)
    return cfg if any(p > 0 for p in probs) else None


def draw(cfg, n, rs):
    """the parameters of n images -> (n, 4) int32 of [dh, dl, ds, gain], drawn from the np.random.RandomState `rs`.  Per
    image, in the order hue, saturation, illumination, contrast: a component with probability 0 draws nothing; otherwise
    u = rs.uniform(0, 1) and the component is applied iff u < prob; when applied, a shift is rs.randint(-m, m + 1) with
    m = int(max) and contrast is c = rs.uniform(-max, max), gain = int(np.rint((1 + c) * 1024))."""
    cfg = _checked(cfg)
    out = np.empty((int(n), 4), np.int32)
    out[:] = IDENTITY
    shifts = ((0, cfg.random_hue_prob, cfg.max_random_hue), (2, cfg.random_saturation_prob, cfg.max_random_saturation),
              (1, cfg.random_illumination_prob, cfg.max_random_illumination))
    for row in out:
        for col, prob, most in shifts:
            if prob > 0 and rs.uniform(0, 1) < prob:
                m = int(most)
                row[col] = rs.randint(-m, m + 1)
        if cfg.random_contrast_prob > 0 and rs.uniform(0, 1) < cfg.random_contrast_prob:
            c = rs.uniform(-cfg.max_random_contrast, cfg.max_random_contrast)
            row[3] = int(np.rint((1 + c) * UNIT_GAIN))
    return out


def describe(params, offsets, sizes):
    """-> the SAMPLE array of images of sizes[k] = (height, width) at byte offsets[k] of a pool, with params[k]"""
    params = np.asarray(params).reshape(-1, 4)
    if not len(params) == len(offsets) == len(sizes):
        raise ValueError("colour_jitter: %d parameter rows, %d offsets, %d sizes" % (len(params), len(offsets), len(sizes)))
    samples = np.zeros(len(params), SAMPLE)
    samples["img_offset"] = np.asarray(offsets, np.int64)
    if len(sizes):
        samples["height"], samples["width"] = np.asarray(sizes, np.int64).reshape(-1, 2).T
    samples["dh"], samples["dl"], samples["ds"], samples["gain"] = params.T
    return samples


def launch(pool_dev, desc_dev, stream=None):
    """dspn_colour_jitter_batch_u8: pool_dev the uint8 device pool, desc_dev a uint8 device tensor of descriptors"""
    dev = pool_dev.device
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().dspn_colour_jitter_batch_u8(pool_dev.data_ptr(), pool_dev.numel(), desc_dev.data_ptr(),
                                                      desc_dev.numel() // SAMPLE.itemsize, st), "colour_jitter")


def apply(pool_dev, params, offsets, sizes, stream=None):
    """jitter, in place, the (height, width, 3) RGB images at byte `offsets` of the uint8 device pool, image k with
    params[k] = [dh, dl, ds, gain]: one upload of descriptors, one launch.  Nothing is uploaded or launched when every row
    is the identity.  -> what must stay alive until the stream has run the launch"""
    params = np.asarray(params).reshape(-1, 4)
    if not len(params) or (params == np.asarray(IDENTITY)).all():
        return ()
    assert pool_dev.dtype == torch.uint8 and pool_dev.is_contiguous()
    samples = describe(params, offsets, sizes)
    host = torch.from_numpy(samples.view(np.uint8).reshape(-1))
    if stream is None:
        # out of pinned memory and on the current stream, like the launch: the host does not wait here for what that
        # stream still has to do (the iterators call this behind their decode launches)
        host = host.pin_memory()
        desc_dev = host.to(pool_dev.device, non_blocking=True)
    else:
        desc_dev = host.to(pool_dev.device)                      # complete on return, whatever stream the launch takes
    launch(pool_dev, desc_dev, stream)
    return (desc_dev, host)


def jitter_images(images, params):
    """images: a list of (h, w, 3) uint8 RGB device tensors of any mix of sizes; params: (n, 4) rows of [dh, dl, ds, gain]
    -> new tensors, views of one pool, jittered by one launch"""
    images = list(images)
    if not images:
        return []
    for k, im in enumerate(images):
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("jitter_images: image %d is not (h, w, 3) uint8, got %s %s" % (k, tuple(im.shape), im.dtype))
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    counts = [h * w * 3 for h, w in sizes]
    pool = torch.cat([im.reshape(-1) for im in images])
    offsets = np.cumsum([0] + counts[:-1])
    keep = apply(pool, params, offsets, sizes)
    if keep:
        torch.cuda.current_stream(pool.device).synchronize()    # the descriptors go out of scope here
    return [part.view(h, w, 3) for part, (h, w) in zip(pool.split(counts), sizes)]
