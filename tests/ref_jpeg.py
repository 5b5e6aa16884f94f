"""An independent numpy reading of a baseline JPEG stream, written for clarity: markers, Huffman decoding through a full
16-bit window table, and the integer reconstruction libjpeg-turbo performs with its accurate IDCT and fancy upsampling
(the contract in include/dspn_jpeg.h).  Test infrastructure: the product never imports it.

    parse(data)   -> dict (width, height, ncomp, hsamp, vsamp, blocks_w, blocks_h, restart_interval, quant, ...)
    decode(data)  -> (parse dict, [coefficient planes (blocks_h, blocks_w, 64) int16, natural order], RGB (h, w, 3) uint8)
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])


def _window_table(counts, values):
    """canonical Huffman code -> two lists over every 16-bit window: code length (0: no code) and symbol"""
    length = np.zeros(1 << 16, np.int64)
    symbol = np.zeros(1 << 16, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            lo = code << (16 - l)
            length[lo:lo + (1 << (16 - l))] = l
            symbol[lo:lo + (1 << (16 - l))] = values[k]
            code += 1
            k += 1
        code <<= 1
    return length.tolist(), symbol.tolist()


def parse(data):
    assert data[:2] == b"\xff\xd8"
    p = 2
    out = {"restart_interval": 0}
    qt, huff = {}, {}
    while True:
        assert data[p] == 0xFF
        while data[p] == 0xFF:
            p += 1
        m = data[p]
        p += 1
        L = (data[p] << 8) | data[p + 1]
        seg = data[p + 2:p + L]
        p += L
        if m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0, "16-bit quantisation table"
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[seg[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                n = sum(counts)
                huff[(seg[q] >> 4, seg[q] & 15)] = _window_table(counts, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDD:
            out["restart_interval"] = (seg[0] << 8) | seg[1]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            out["sof"] = m
            out["precision"] = seg[0]
            out["height"], out["width"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            out["ncomp"] = seg[5]
            out["ids"] = [seg[6 + 3 * c] for c in range(seg[5])]
            out["hsamp"] = [seg[7 + 3 * c] >> 4 for c in range(seg[5])]
            out["vsamp"] = [seg[7 + 3 * c] & 15 for c in range(seg[5])]
            out["tq"] = [seg[8 + 3 * c] for c in range(seg[5])]
        elif m == 0xDA:
            assert seg[0] == out["ncomp"]
            out["td"] = [seg[2 + 2 * c] >> 4 for c in range(seg[0])]
            out["ta"] = [seg[2 + 2 * c] & 15 for c in range(seg[0])]
            break
    out["scan_pos"] = p
    nc = out["ncomp"]
    if nc == 1:
        out["hsamp"], out["vsamp"] = [1], [1]
    hmax, vmax = max(out["hsamp"]), max(out["vsamp"])
    out["mcux"] = -(-out["width"] // (8 * hmax))
    out["mcuy"] = -(-out["height"] // (8 * vmax))
    out["blocks_w"] = [out["mcux"] * h for h in out["hsamp"]]
    out["blocks_h"] = [out["mcuy"] * v for v in out["vsamp"]]
    out["quant"] = [qt[t] for t in out["tq"]]
    out["huff"] = huff
    return out


def _segments(data, start):
    """the entropy-coded bytes split at the RSTn markers, byte stuffing removed"""
    segs, cur, p = [], bytearray(), start
    while True:
        b = data[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
        elif data[p + 1] == 0:
            cur.append(0xFF)
            p += 2
        elif 0xD0 <= data[p + 1] <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            p += 2
        elif data[p + 1] == 0xFF:
            p += 1
        else:
            segs.append(bytes(cur))
            return segs


def _windows(seg):
    bits = np.concatenate([np.unpackbits(np.frombuffer(seg, np.uint8)), np.ones(48, np.uint8)]).astype(np.int64)
    n = bits.size - 16
    win = np.zeros(n, np.int64)
    for k in range(16):
        win += bits[k:k + n] << (15 - k)
    return win.tolist()


def coefficients(data, P):
    nc = P["ncomp"]
    planes = [np.zeros((P["blocks_h"][c], P["blocks_w"][c], 64), np.int16) for c in range(nc)]
    segs = _segments(data, P["scan_pos"])
    ri = P["restart_interval"] or P["mcux"] * P["mcuy"]
    mcu = 0
    for seg in segs:
        win, pos, pred = _windows(seg), 0, [0] * nc
        for _ in range(min(ri, P["mcux"] * P["mcuy"] - mcu)):
            my, mx = divmod(mcu, P["mcux"])
            for c in range(nc):
                dl, ds = P["huff"][(0, P["td"][c])]
                al, as_ = P["huff"][(1, P["ta"][c])]
                for v in range(P["vsamp"][c]):
                    for h in range(P["hsamp"][c]):
                        blk = planes[c][my * P["vsamp"][c] + v, mx * P["hsamp"][c] + h]
                        w = win[pos]
                        assert dl[w]
                        pos += dl[w]
                        s = ds[w]
                        if s:
                            val = win[pos] >> (16 - s)
                            pos += s
                            pred[c] += val if val >> (s - 1) else val - (1 << s) + 1
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            w = win[pos]
                            assert al[w]
                            pos += al[w]
                            r, s = as_[w] >> 4, as_[w] & 15
                            if s:
                                k += r
                                val = win[pos] >> (16 - s)
                                pos += s
                                blk[ZIGZAG[k]] = val if val >> (s - 1) else val - (1 << s) + 1
                                k += 1
                            elif r == 15:
                                k += 16
                            else:
                                break
            mcu += 1
    assert mcu == P["mcux"] * P["mcuy"]
    return planes


def _pass(i, s):
    """one 1-D pass of the slow integer IDCT over the LAST axis of i (int64)"""
    i0, i1, i2, i3, i4, i5, i6, i7 = [i[..., k] for k in range(8)]
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    o = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)
    return (o + (1 << (s - 1))) >> s


def plane_samples(coefs, quant):
    """(bh, bw, 64) quantised coefficients -> (bh * 8, bw * 8) samples 0..255"""
    bh, bw, _ = coefs.shape
    x = (coefs.astype(np.int64) * quant).reshape(bh, bw, 8, 8)         # [row, column]
    x = _pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)                 # down the columns
    x = _pass(x, 18)                                                   # along the rows
    x = np.clip(x + 128, 0, 255)
    return x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _upsample_h2v1(p):
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def _upsample_h2v2(p):
    above = np.concatenate([p[:1], p[:-1]], 0)
    below = np.concatenate([p[1:], p[-1:]], 0)
    rows = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    rows[0::2] = 3 * p + above
    rows[1::2] = 3 * p + below
    left = np.concatenate([rows[:, :1], rows[:, :-1]], 1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), np.int64)
    out[:, 0::2] = (3 * rows + left + 8) >> 4
    out[:, 1::2] = (3 * rows + right + 7) >> 4
    return out


def pixels(P, planes):
    W, H, nc = P["width"], P["height"], P["ncomp"]
    comp = [plane_samples(planes[c], P["quant"][c]) for c in range(nc)]
    y = comp[0][:H, :W]
    if nc == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    hs, vs = P["hsamp"][0], P["vsamp"][0]
    cw, ch = -(-W // hs), -(-H // vs)
    chroma = []
    for c in (1, 2):
        p = comp[c][:ch, :cw]
        if hs == 2 and cw <= 2:                                 # jdsample.c: fancy upsampling only for downsampled_width > 2
            p = np.repeat(np.repeat(p, 2, 1), vs, 0)
        elif (hs, vs) == (2, 1):
            p = _upsample_h2v1(p)
        elif (hs, vs) == (2, 2):
            p = _upsample_h2v2(p)
        else:
            assert (hs, vs) == (1, 1)
        chroma.append(p[:H, :W] - 128)
    cb, cr = chroma
    F = lambda v: int(v * 65536 + 0.5)  # noqa: E731
    r = y + ((F(1.402) * cr + 32768) >> 16)
    b = y + ((F(1.772) * cb + 32768) >> 16)
    g = y + ((-F(0.34414) * cb + 32768 - F(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    P = parse(data)
    planes = coefficients(data, P)
    return P, planes, pixels(P, planes)
