"""The SSD samplers of the reference (tools/rand_sampler.py): RandCropper draws crop boxes constrained by their overlap
with the ground truth, RandPadder draws zoom-out canvases.  Host code, pure numpy: a few dozen numbers per image.

The sequence of random draws is the reference's, draw for draw -- trials that `continue` have consumed theirs, and the
padder's `uniform(0., 1 - width)` runs with a negative upper end -- so for a given seed the boxes and labels equal the
reference's to the last float64 bit (tests/golden/rand_sampler.npz).

rng=None draws from the global `np.random`, as the reference does; otherwise pass a `np.random.RandomState`.

One extension: label columns beyond the fifth (the distance column MultiBoxTarget takes here) are carried through
unchanged for every surviving row.  With 5-column labels the output is exactly the reference's."""
import math

import numpy as np


class RandSampler(object):
    """base class (:4-34): max_trials, the number of trials after which a sampler gives up; max_sample, the number of
    samples it stops at"""

    def __init__(self, max_trials, max_sample, rng=None):
        assert max_trials > 0
        self.max_trials = int(max_trials)
        assert max_sample >= 0
        self.max_sample = int(max_sample)
        self.rng = np.random if rng is None else rng

    def sample(self, label):
        """label: (n, 5+) ground truths, rows of -1 below the valid ones -> list of (crop_box, label); [] when no trial
        was accepted"""
        return NotImplementedError                             # :34 returns (not raises) it


def _pad_rows(rows, count):
    """:123-125 / :265-267: -1 rows below the surviving ones, up to the row count of the label that came in"""
    return np.pad(rows, ((0, count - rows.shape[0]), (0, 0)), "constant", constant_values=(-1, -1))


class RandCropper(RandSampler):
    """random crops (:37-175): scale in [min_scale, max_scale] (0, 1], aspect ratio in [min_aspect_ratio <= 1,
    max_aspect_ratio >= 1], accepted when the best IoU with a ground truth reaches min_overlap and every ground truth
    the crop touches has its centre inside it"""

    def __init__(self, min_scale=1., max_scale=1., min_aspect_ratio=1., max_aspect_ratio=1., min_overlap=0.,
                 max_trials=50, max_sample=1, rng=None):
        super(RandCropper, self).__init__(max_trials, max_sample, rng)
        assert min_scale <= max_scale, "min_scale must <= max_scale"
        assert 0 < min_scale and min_scale <= 1, "min_scale must in (0, 1]"
        assert 0 < max_scale and max_scale <= 1, "max_scale must in (0, 1]"
        self.min_scale = min_scale
        self.max_scale = max_scale
        assert 0 < min_aspect_ratio and min_aspect_ratio <= 1, "min_ratio must in (0, 1]"
        assert 1 <= max_aspect_ratio, "max_ratio must >= 1"
        self.min_aspect_ratio = min_aspect_ratio
        self.max_aspect_ratio = max_aspect_ratio
        assert 0 <= min_overlap and min_overlap <= 1, "min_overlap must in [0,1]"
        self.min_overlap = min_overlap
        self.config = {'gt_constraint': 'center'}             # :74, the only value the reference ever sets

    def sample(self, label):
        uniform = self.rng.uniform
        samples = []
        count = 0
        for trial in range(self.max_trials):
            if count >= self.max_sample:
                return samples
            scale = uniform(self.min_scale, self.max_scale)
            min_ratio = max(self.min_aspect_ratio, scale * scale)
            max_ratio = min(self.max_aspect_ratio, 1. / scale / scale)
            ratio = math.sqrt(uniform(min_ratio, max_ratio))
            width = scale * ratio
            height = scale / ratio
            left = uniform(0., 1 - width)
            top = uniform(0., 1 - height)
            rand_box = (left, top, left + width, top + height)
            valid_mask = np.where(label[:, 0] > -1)[0]
            gt = label[valid_mask, :]
            ious = self._check_satisfy(rand_box, gt)
            if ious is not None:
                l, t, r, b = rand_box
                new_gt_boxes = []
                new_width = r - l
                new_height = b - t
                for i in range(valid_mask.size):
                    if ious[i] > 0:                             # :114 a box the crop does not touch is dropped ...
                        xmin = max(0., (gt[i, 1] - l) / new_width)   # :115-118 ... and the others are clamped to [0, 1]
                        ymin = max(0., (gt[i, 2] - t) / new_height)
                        xmax = min(1., (gt[i, 3] - l) / new_width)
                        ymax = min(1., (gt[i, 4] - t) / new_height)
                        new_gt_boxes.append([gt[i, 0], xmin, ymin, xmax, ymax] + list(gt[i, 5:]))
                if not new_gt_boxes:
                    continue
                new_gt_boxes = np.array(new_gt_boxes)
                label = _pad_rows(new_gt_boxes, label.shape[0])  # :123 reassigned: later samples see the cropped label
                samples.append((rand_box, label))
                count += 1
        return samples

    def _check_satisfy(self, rand_box, gt_boxes):
        """IoU of the crop with every ground truth, or None when the crop is refused (:130-175)"""
        l, t, r, b = rand_box
        num_gt = gt_boxes.shape[0]
        ls = np.ones(num_gt) * l
        ts = np.ones(num_gt) * t
        rs = np.ones(num_gt) * r
        bs = np.ones(num_gt) * b
        mask = np.where(ls < gt_boxes[:, 1])[0]
        ls[mask] = gt_boxes[mask, 1]
        mask = np.where(ts < gt_boxes[:, 2])[0]
        ts[mask] = gt_boxes[mask, 2]
        mask = np.where(rs > gt_boxes[:, 3])[0]
        rs[mask] = gt_boxes[mask, 3]
        mask = np.where(bs > gt_boxes[:, 4])[0]
        bs[mask] = gt_boxes[mask, 4]
        w = rs - ls
        w[w < 0] = 0
        h = bs - ts
        h[h < 0] = 0
        inter_area = h * w
        union_area = np.ones(num_gt) * max(0, r - l) * max(0, b - t)
        union_area += (gt_boxes[:, 3] - gt_boxes[:, 1]) * (gt_boxes[:, 4] - gt_boxes[:, 2])
        union_area -= inter_area
        with np.errstate(divide="ignore", invalid="ignore"):
            ious = inter_area / union_area
        ious[union_area <= 0] = 0                               # :157
        max_iou = np.amax(ious)                                 # (raises on a label without a valid row, like :158)
        if max_iou < self.min_overlap:
            return None
        if self.config['gt_constraint'] == 'center':            # :162 the centre of every touched box lies in the crop
            for i in range(ious.shape[0]):
                if ious[i] > 0:
                    gt_x = (gt_boxes[i, 1] + gt_boxes[i, 3]) / 2.0
                    gt_y = (gt_boxes[i, 2] + gt_boxes[i, 4]) / 2.0
                    if gt_x < l or gt_x > r or gt_y < t or gt_y > b:
                        return None
        elif self.config['gt_constraint'] == 'corner':
            for i in range(ious.shape[0]):
                if ious[i] > 0:
                    if gt_boxes[i, 1] < l or gt_boxes[i, 3] > r or gt_boxes[i, 2] < t or gt_boxes[i, 4] > b:
                        return None
        return ious


class RandPadder(RandSampler):
    """random zoom-out canvases (:178-270): scale in [min_scale >= 1, max_scale], aspect ratio as in the cropper,
    accepted when every ground truth keeps at least min_gt_scale of the canvas in its smaller side"""

    def __init__(self, min_scale=1., max_scale=1., min_aspect_ratio=1., max_aspect_ratio=1., min_gt_scale=.01,
                 max_trials=50, max_sample=1, rng=None):
        super(RandPadder, self).__init__(max_trials, max_sample, rng)
        assert min_scale <= max_scale, "min_scale must <= max_scale"
        assert min_scale >= 1, "min_scale must in (0, 1]"
        self.min_scale = min_scale
        self.max_scale = max_scale
        assert 0 < min_aspect_ratio and min_aspect_ratio <= 1, "min_ratio must in (0, 1]"
        assert 1 <= max_aspect_ratio, "max_ratio must >= 1"
        self.min_aspect_ratio = min_aspect_ratio
        self.max_aspect_ratio = max_aspect_ratio
        assert 0 <= min_gt_scale and min_gt_scale <= 1, "min_gt_scale must in [0, 1]"
        self.min_gt_scale = min_gt_scale

    def sample(self, label):
        uniform = self.rng.uniform
        samples = []
        count = 0
        for trial in range(self.max_trials):
            if count >= self.max_sample:
                return samples
            scale = uniform(self.min_scale, self.max_scale)
            min_ratio = max(self.min_aspect_ratio, scale * scale)
            max_ratio = min(self.max_aspect_ratio, 1. / scale / scale)
            ratio = math.sqrt(uniform(min_ratio, max_ratio))
            width = scale * ratio
            if width < 1:
                continue
            height = scale / ratio
            if height < 1:
                continue
            left = uniform(0., 1 - width)                       # :244 the upper end is negative: left, top <= 0
            top = uniform(0., 1 - height)
            right = left + width
            bot = top + height
            rand_box = (left, top, right, bot)
            valid_mask = np.where(label[:, 0] > -1)[0]
            gt = label[valid_mask, :]
            new_gt_boxes = []
            for i in range(gt.shape[0]):
                xmin = (gt[i, 1] - left) / width                # :253-256 nothing is clamped
                ymin = (gt[i, 2] - top) / height
                xmax = (gt[i, 3] - left) / width
                ymax = (gt[i, 4] - top) / height
                new_size = min(xmax - xmin, ymax - ymin)
                if new_size < self.min_gt_scale:                # :258 one too-small box voids the whole trial
                    new_gt_boxes = []
                    break
                new_gt_boxes.append([gt[i, 0], xmin, ymin, xmax, ymax] + list(gt[i, 5:]))
            if not new_gt_boxes:
                continue
            new_gt_boxes = np.array(new_gt_boxes)
            label = _pad_rows(new_gt_boxes, label.shape[0])      # :265 reassigned, as in the cropper
            samples.append((rand_box, label))
            count += 1
        return samples
