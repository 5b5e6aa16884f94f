"""Restatement of include/dspn_colour_jitter.h, written from the header's text: one vectorised version in numpy int64 (the
integer formulas as they stand there) and one in Python `fractions` that forms every quantity as the exact rational the
header names (S = 255 d / den, H = N / d, W / 7650, ...) and rounds it half up."""
from fractions import Fraction

import numpy as np


# ---- numpy int64: the header's integers -----------------------------------------------------------------------------
def forward(rgb):
    """(..., 3) RGB 0..255 -> (H, L, S) int64 arrays"""
    rgb = np.asarray(rgb).astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    mx, mn = rgb.max(axis=-1), rgb.min(axis=-1)
    d, sm = mx - mn, mx + mn
    L = (sm + 1) >> 1
    grey = d == 0
    d1 = np.where(grey, 1, d)                                   # the grey pixels' quotients are thrown away
    den = np.where(grey, 1, np.where(sm <= 255, sm, 510 - sm))
    S = np.where(grey, 0, (510 * d + den) // (2 * den))
    x = np.where(mx == r, g - b, np.where(mx == g, b - r, r - g))
    base = np.where(mx == r, 0, np.where(mx == g, 60, 120))
    N = 30 * x + base * d
    H = (2 * N + d) // (2 * d1)                                 # numpy's // is floor division
    H = np.where(H < 0, H + 180, H)
    H = np.where(H >= 180, H - 180, H)
    return np.where(grey, 0, H), L, S


def inverse(H, L, S):
    """H 0..180, L and S 0..255 -> (..., 3) int64 RGB"""
    H, L, S = (np.asarray(v).astype(np.int64) for v in (H, L, S))
    Q2 = np.where(2 * L <= 255, L * (255 + S), 255 * (L + S) - L * S)
    Q1 = 510 * L - Q2
    out = []
    for off in (60, 0, -60):
        t = (H + off) % 180
        W = np.where(t < 30, 30 * Q1 + (Q2 - Q1) * t,
                     np.where(t < 90, 30 * Q2, np.where(t < 120, 30 * Q1 + (Q2 - Q1) * (120 - t), 30 * Q1)))
        out.append(np.where(S == 0, L, (W + 3825) // 7650))
    return np.stack(out, axis=-1)


def contrast(v, gain):
    return np.minimum(255, (np.asarray(v).astype(np.int64) * int(gain) + 512) >> 10)


def jitter(img, dh, dl, ds, gain):
    """(..., 3) uint8 RGB -> the same shape, uint8: shifts, then contrast, with the header's skips"""
    out = np.asarray(img).astype(np.int64)
    dh, dl, ds, gain = int(dh), int(dl), int(ds), int(gain)
    if dh or dl or ds:
        H, L, S = forward(out)
        out = inverse(np.clip(H + dh, 0, 180), np.clip(L + dl, 0, 255), np.clip(S + ds, 0, 255))
    if gain != 1024:
        out = contrast(out, gain)
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    return out.astype(np.uint8)


# ---- fractions: the exact rationals, rounded half up ----------------------------------------------------------------
def rhu(q):
    """round half up: floor(q + 1/2)"""
    return (Fraction(q) + Fraction(1, 2)).__floor__()


def forward_exact(r, g, b):
    mx, mn = max(r, g, b), min(r, g, b)
    d, sm = mx - mn, mx + mn
    L = rhu(Fraction(sm, 2))
    if d == 0:
        return 0, L, 0
    S = rhu(Fraction(255 * d, sm if sm <= 255 else 510 - sm))
    if mx == r:
        deg = Fraction(30 * (g - b), d)
    elif mx == g:
        deg = Fraction(30 * (b - r), d) + 60
    else:
        deg = Fraction(30 * (r - g), d) + 120
    H = rhu(deg)
    if H < 0:
        H += 180
    if H >= 180:
        H -= 180
    return H, L, S


def inverse_exact(H, L, S):
    if S == 0:
        return L, L, L
    l, s = Fraction(L, 255), Fraction(S, 255)
    q2 = l * (1 + s) if 2 * L <= 255 else l + s - l * s
    q1 = 2 * l - q2
    out = []
    for off in (60, 0, -60):
        t = (H + off) % 180
        if t < 30:
            v = q1 + (q2 - q1) * Fraction(t, 30)
        elif t < 90:
            v = q2
        elif t < 120:
            v = q1 + (q2 - q1) * Fraction(120 - t, 30)
        else:
            v = q1
        out.append(rhu(255 * v))
    return tuple(out)


def jitter_exact(rgb, dh, dl, ds, gain):
    """one pixel"""
    out = tuple(int(v) for v in rgb)
    if dh or dl or ds:
        H, L, S = forward_exact(*out)
        out = inverse_exact(min(max(H + dh, 0), 180), min(max(L + dl, 0), 255), min(max(S + ds, 0), 255))
    if gain != 1024:
        out = tuple(min(255, rhu(Fraction(v * gain, 1024))) for v in out)
    return out
