"""Host staging shared by the iterators and the decode_batch calls: the pools a batch is decoded into before it goes to
the device, and the part of a coded batch (dataset/jpeg.py, dataset/png.py) that does not depend on the format.

Order of the device phase of one batch, on the current stream:
  1. every pool-to-device copy of the batch is enqueued (`CodedBatch.upload`; non-blocking, out of pinned memory);
  2. the event of the pool set is recorded (`HostPools.uploaded`);
  3. the descriptors are uploaded and the kernels launched (`CodedBatch.launch`).
The event has to follow every copy that reads the pools, or a pool could be rewritten under a copy.  It comes before
step 3 because nothing there reads the pools: the thread that waits for the event in `take` may rewrite the set as soon
as the last pool byte has left, not only after the descriptor uploads (synchronous, out of pageable memory) and the
launches behind them."""
import numpy as np
import torch


class HostPools(object):
    """a set of named host staging buffers and the one event that guards them: a set is rewritten only after the upload
    that last read it has completed.  `take` is the only way to a buffer, so the rule holds whatever the call order.
    pinned: true exactly when the batches go to a GPU"""

    def __init__(self, pinned, event_type=torch.cuda.Event):
        self._pinned, self._event_type = bool(pinned), event_type
        self._buffers, self._uploaded = {}, None

    def take(self, name, count, dtype, floor=1):
        """-> the buffer `name` with at least max(count, floor) elements, for writing; grown on demand, reused otherwise"""
        if self._uploaded is not None:
            self._uploaded.synchronize()
            self._uploaded = None
        cur = self._buffers.get(name)
        if cur is None or cur.numel() < count:
            cur = torch.empty(max(count, floor), dtype=dtype)
            if self._pinned:
                cur = cur.pin_memory()
            self._buffers[name] = cur
        return cur

    def uploaded(self, stream):
        """every copy out of this set has been enqueued on `stream`"""
        self._uploaded = self._event_type()
        self._uploaded.record(stream)


class Decoded(object):
    """decoded pixels of a cached record, with the `size` a batch layout reads from a PIL image"""

    def __init__(self, a):
        self.a = a
        self.size = (a.shape[1], a.shape[0])


class CodedBatch(object):
    """a batch of streams of which the host does the serial half and the device the rest; it owns the descriptors, the
    layout of the coded pool (coefficients, filtered rows) and the device front end.  The host half of a sample goes
    wrong only on a worker thread, so the decision what the device does falls in `answered`.
    A subclass names SAMPLE, FLOOR (the least element count its entry accepts) and gives `_describe` and `_launch`."""

    def __init__(self, infos, out_offsets, device_side=None):
        """infos: per sample the probed record of a stream for the device, or None; out_offsets: where each sample's
        decoded bytes start in the output pool; device_side: per sample, true where the device itself produces the
        sample's coded slice (dataset/jpeg.py: the entropy pass on the device).  Such slices lie behind everyone
        else's, so the host's part of the coded pool is its first `host_count` elements and only that is uploaded."""
        self.samples = np.zeros(len(infos), self.SAMPLE)
        self.spans, self.count = [None] * len(infos), 0
        side = [False] * len(infos) if device_side is None else [bool(d) for d in device_side]
        for want in (False, True):
            for k, (s, info, out) in enumerate(zip(self.samples, infos, out_offsets)):
                if side[k] != want:
                    continue
                n = self._describe(s, info, self.count, out) if info is not None else 0
                self.spans[k] = (self.count, n)
                self.count += n
            if not want:
                self.host_count = self.count
        self.on_device = self.fallbacks = 0

    def slices(self, pool):
        """each sample's slice of the host array `pool` (empty where the sample is not coded, or coded on the device)"""
        return [pool[at:at + n] if at + n <= self.host_count else pool[:0] for at, n in self.spans]

    def answered(self, answers):
        """what the workers said per sample: True -- its coded slice is filled, the device finishes it; False -- the host
        decoded it into the output pool; None -- there was nothing to decode"""
        self.samples["skip"] = [0 if a else 1 for a in answers]
        self.on_device, self.fallbacks = answers.count(True), answers.count(False)

    def upload(self, coded, device, decoded=None):
        """step 1 of the module note.  coded: the host pool the slices came from; decoded: the host output pool, cut to
        the batch.  -> the device output pool (None without `decoded`: the caller brings its own).
        The coded route is taken exactly when some sample is left to the device; then the host's bytes go up only if
        there are any.  Otherwise the host's pool goes up as it is and nothing of this format is uploaded or launched."""
        if self.on_device and self.host_count == self.count:
            self._coded_dev = coded[:max(self.count, self.FLOOR)].to(device, non_blocking=True)
        elif self.on_device:                                   # the device fills the rest of the pool itself
            self._coded_dev = torch.empty(max(self.count, self.FLOOR), dtype=coded.dtype, device=device)
            if self.host_count:
                self._coded_dev[:self.host_count].copy_(coded[:self.host_count], non_blocking=True)
        if decoded is None:
            return None
        return upload_decoded(decoded, device, self.on_device, self.fallbacks)

    def _descriptors(self):
        """the bytes of the descriptor upload: the samples, and behind them whatever tables a subclass's launch reads"""
        return self.samples.view(np.uint8).reshape(-1)

    def launch(self, out_dev):
        """step 3 of the module note -> what must stay alive until the stream has run the launch"""
        if not self.on_device:
            return ()
        desc_dev = torch.from_numpy(self._descriptors()).to(out_dev.device)
        return (self._coded_dev, desc_dev) + tuple(self._launch(self._coded_dev, desc_dev, out_dev))


def upload_decoded(decoded, device, on_device, on_host):
    """the device output pool of a batch of which `on_device` samples are finished by launches and `on_host` were decoded
    into the host pool `decoded`: with nothing for the device the host's pool goes up as it is; otherwise the host's bytes go
    up only if there are any"""
    if not on_device:
        return decoded.to(device, non_blocking=True)
    out = torch.empty(decoded.numel(), dtype=decoded.dtype, device=device)
    if on_host:
        out.copy_(decoded, non_blocking=True)
    return out
