"""Seeded images and Pillow's files for tests/test_jpeg_encode_host.py and tests/test_jpeg_encode_gpu.py: sizes x chroma
layouts x qualities x contents, and the coefficients of a Pillow stream cut down to the real block grids the encoder works on."""
import functools
import zlib

import numpy as np

import jpeg_cases as jc
from dspnet_amd.dataset import jpeg as dj
from dspnet_amd.dataset import jpeg_encode as je

SIZES = [(1, 1), (8, 8), (16, 16), (24, 40), (21, 37), (9, 15), (64, 200)]          # (height, width)
LAYOUTS = ["4:2:0", "4:2:2", "4:4:4", "grey"]
QUALITIES = [95, 30]
CONTENTS = ["noise", "smooth"]
CASES = [(h, w, layout, q, content) for (h, w) in SIZES for layout in LAYOUTS for q in QUALITIES for content in CONTENTS]
_PILLOW_SS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def name(case):
    return "%dx%d-%s-q%d-%s" % case


@functools.lru_cache(maxsize=None)
def pixels(case):
    """the image of a case: (h, w, 3) RGB, or (h, w) for grey (treated as read-only)"""
    h, w, layout, _, content = case
    return jc.image(zlib.crc32(name(case).encode()), h, w, content, 1 if layout == "grey" else 3)


@functools.lru_cache(maxsize=None)
def pillow_file(case):
    """what Pillow writes for the case: the yardstick"""
    layout, q = case[2], case[3]
    kw = {} if layout == "grey" else {"subsampling": _PILLOW_SS[layout]}
    return jc.encode(pixels(case), quality=q, **kw)


def sample_of(case, coef_base=0, img_offset=0):
    """-> (descriptor record, number of coefficients) of a case"""
    h, w, layout, q, _ = case
    s = np.zeros(1, je.SAMPLE)
    n = je.fill_sample(s[0], w, h, 1 if layout == "grey" else 3, je.SUBSAMPLING.get(layout, (1, 1)), je.quant_tables(q), coef_base,
                       img_offset)
    return s[0], n


@functools.lru_cache(maxsize=None)
def pillow_real_blocks(case):
    """the coefficients of Pillow's stream, read back with the decoder's host half and cut to the real grids, in the layout
    sample_of(case) describes (coef_base 0); int16, read-only"""
    data = pillow_file(case)
    rc, info = dj.probe_info(data)
    assert rc == 0 and info["supported"], name(case)
    padded = np.zeros(int(info["coef_count"]), np.int16)
    assert dj.entropy_decode(data, info, padded) == 0, name(case)
    s, n = sample_of(case)
    assert (int(info["width"]), int(info["height"]), int(info["ncomp"])) == (int(s["width"]), int(s["height"]), int(s["ncomp"]))
    out = np.zeros(n, np.int16)
    for c in range(int(s["ncomp"])):
        pw, ph = int(info["blocks_w"][c]), int(info["blocks_h"][c])
        bw, bh = int(s["blocks_w"][c]), int(s["blocks_h"][c])
        assert bw <= pw and bh <= ph
        np.testing.assert_array_equal(info["quant"][c], s["quant"][c], err_msg=name(case))
        plane = padded[int(info["coef_offset"][c]):][:64 * pw * ph].reshape(ph, pw, 64)
        o = int(s["coef_offset"][c])
        out[o:o + 64 * bw * bh] = plane[:bh, :bw].reshape(-1)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------
# The low-level harness of tests/test_jpeg_encode_gpu.py and tests/test_pipeline_edges_gpu.py
GUARD = 256                                                    # guard bytes (a whole number of int16 blocks and of dwords)
# the eight images a 1024-descriptor call repeats: all four layouts, odd sizes (odd image offsets), both qualities
BATCH_CASES = [(56, 72, "4:4:4", 95, "noise"), (40, 88, "4:2:2", 30, "noise"), (48, 80, "4:2:0", 95, "smooth"),
               (72, 56, "grey", 95, "noise"), (33, 95, "4:4:4", 30, "smooth"), (71, 49, "4:2:0", 95, "noise"),
               (64, 64, "4:2:2", 95, "noise"), (47, 91, "grey", 30, "noise")]


@functools.lru_cache(maxsize=None)
def reference_blocks(case):
    """ref_jpeg's reading of Pillow's stream, cut to the real grids: per component (blocks_h, blocks_w, 64); read-only"""
    import ref_jpeg
    data = pillow_file(case)
    P = ref_jpeg.parse(data)
    planes = ref_jpeg.coefficients(data, P)
    s, _ = sample_of(case)
    return [planes[c][:int(s["blocks_h"][c]), :int(s["blocks_w"][c])].copy() for c in range(P["ncomp"])]


def describe_batch(cases, skip=()):
    """descriptors of one dspn_jpeg_encode_blocks_batch_u8 call over `cases` with GUARD bytes around every sample's pixels
    and coefficients -> (samples, [(pixel offset, image)], int16 count of the coefficient pool, bytes of the image pool)"""
    samples = np.zeros(len(cases), je.SAMPLE)
    pix, co, io_ = [], GUARD // 2, 0
    for k, case in enumerate(cases):
        img = pixels(case)
        io_ += GUARD
        pix.append((io_, img))
        n = je.fill_sample(samples[k], case[1], case[0], 1 if case[2] == "grey" else 3, je.SUBSAMPLING.get(case[2], (1, 1)),
                           je.quant_tables(case[3]), co, io_)
        samples[k]["skip"] = int(k in skip)
        co += n + GUARD // 2
        io_ += img.size + GUARD
    return samples, pix, co, io_


def low_level_batch(cases, dev, skip=(), spoil=None, stream=None):
    """one dspn_jpeg_encode_blocks_batch_u8 call over `cases` with GUARD bytes of 0xA5 around every sample's pixels and
    coefficients and around the workspace -> (coefficient pool as int16 with guards, samples, workspace bytes with guards)"""
    import torch
    from dspnet_amd import _lib
    samples, pix, co, io_ = describe_batch(cases, skip)
    if spoil:
        spoil(samples)
    pool = np.full(io_, 0xA5, np.uint8)
    for at, img in pix:
        pool[at:at + img.size] = img.reshape(-1)
    pdev = torch.from_numpy(pool).to(dev)
    cdev = torch.full((co,), -23131, dtype=torch.int16, device=dev)                 # 0xA5A5
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    ws_bytes = _lib.lib().dspn_jpeg_encode_workspace_bytes(co)
    assert ws_bytes >= co
    ws = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    cmap = (je._c.c_int * 3)(0, 1, 2)
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
    torch.cuda.synchronize(dev)                                 # the fills above ran on the current stream
    _lib.check(_lib.lib().dspn_jpeg_encode_blocks_batch_u8(pdev.data_ptr(), pdev.numel(), cmap, desc.data_ptr(), len(cases),
                                                           cdev.data_ptr(), co, ws.data_ptr() + GUARD, ws_bytes, st))
    torch.cuda.synchronize(dev)
    return cdev.cpu().numpy(), samples, ws.cpu().numpy()


def regions(samples, k):
    s = samples[k]
    return [(int(s["coef_offset"][c]), 64 * int(s["blocks_w"][c]) * int(s["blocks_h"][c])) for c in range(int(s["ncomp"]))]


def check_batch(cases, coefs, samples, ws, untouched=()):
    covered = np.zeros(coefs.size, bool)
    for k, case in enumerate(cases):
        for c, (at, n) in enumerate(regions(samples, k)):
            covered[at:at + n] = True
            if k in untouched:
                assert (coefs[at:at + n] == -23131).all(), "sample %d (%s) was written" % (k, name(case))
                assert (ws[GUARD + at:GUARD + at + n] == 0xA5).all(), "the planes of sample %d (%s) were written" % (k, name(case))
            else:
                np.testing.assert_array_equal(coefs[at:at + n], reference_blocks(case)[c].reshape(-1),
                                              err_msg="%s component %d" % (name(case), c))
    assert (coefs[~covered] == -23131).all(), "guard words of the coefficient pool overwritten"
    assert (~covered).sum() == (GUARD // 2) * (len(cases) + 1)
    assert (ws[:GUARD] == 0xA5).all() and (ws[-GUARD:] == 0xA5).all(), "guard bytes of the workspace overwritten"
