"""What `PIL.ImageDraw.Draw(im).polygon(xy, fill=v)` paints, restated in numpy / plain Python (modes L and I, no
outline, vertices anywhere).  It is the reference of the device rasteriser (dspnet_amd/csrc/polygon.hip) and is itself
held equal to the installed Pillow, pixel for pixel, by tests/test_polygon_host.py; nothing here imports Pillow, so
the GPU tests can compute their expectations from it alone.

The rule, per polygon:
  * vertices are truncated toward zero to integers; fewer than two points is an error, as in Pillow;
  * edges join consecutive points, and the last point to the first only when they differ;
  * a horizontal edge paints its own span; every other edge has dx = float32(x1 - x0) / float32(y1 - y0) and crosses
    row y at float32(float32(y - y0) * dx) + x0, rounded after the multiply and after the add;
  * rows run from max(ymin, 0) to min(ymax, H); an edge is active for its ymin <= y <= its ymax; its crossing is
    entered twice where y is its ymax and not the last row;
  * the corner rule, derived from Pillow's behaviour (its source was not to hand): where an edge begins on row y (not
    the last row) or ends on the polygon's last row, take the FIRST earlier non-vertical edge of the list that has
    the same integer vertex at the same end.  If that edge leans the same way (dx of the same sign), the two make a
    corner whose rows would otherwise be disconnected: on the adjacent row (y + 1, or y - 1 on the last row) both
    edges' crossings are taken, and the later edge's own entry on row y becomes the integer
    round_half_up(max(a, b)) + 1 (corner to the right of the adjacent row's span) or round_half_up(min(a, b)) - 1
    (to the left) -- unless that lies beyond the vertex, in which case, as when the first edge found leans the
    other way, nothing changes.  Each edge decides its own entry, so a row's entries are a multiset: no order matters;
  * the entries are sorted and taken in pairs (a, b), each painting round_half_up(a) .. round_half_down(b), away from
    zero below zero; a running x_pos keeps the spans of one row from overlapping; everything is clipped to the image.
"""
import math

import numpy as np

f32 = np.float32


def round_half_up(f):
    f = float(f)
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(abs(f) + 0.5))


def round_half_down(f):
    f = float(f)
    return int(math.ceil(f - 0.5)) if f >= 0 else -int(math.ceil(abs(f) - 0.5))


def int_points(xy):
    """the binding's view of `xy`: a flat list or a list of pairs, each coordinate truncated toward zero"""
    flat = []
    for p in xy:
        if isinstance(p, (tuple, list, np.ndarray)):
            flat.extend(p)
        else:
            flat.append(p)
    if len(flat) % 2:
        raise ValueError("incorrect coordinate type")
    pts = [(int(flat[i]), int(flat[i + 1])) for i in range(0, len(flat), 2)]
    if len(pts) < 2:
        raise TypeError("coordinate list must contain at least 2 coordinates")
    return pts


def edge_list(pts):
    """-> list of (x0, y0, x1, y1, ymin, ymax, dx) in Pillow's order, horizontal edges included (dx 0)"""
    out = []

    def add(x0, y0, x1, y1):
        dx = f32(0) if y0 == y1 else f32(f32(x1 - x0) / f32(y1 - y0))
        out.append((x0, y0, x1, y1, min(y0, y1), max(y0, y1), dx))

    for i in range(len(pts) - 1):
        add(*pts[i], *pts[i + 1])
    if pts[-1] != pts[0]:
        add(*pts[-1], *pts[0])
    return out


def crossing(e, y):
    return f32(f32(f32(y - e[1]) * e[6]) + f32(e[0]))


def end_vertex(e, off):
    """the edge's upper end (off 1: the vertex on its first row) or lower end (off -1), as (x, y)"""
    upper = (e[1] < e[3]) == (off == 1)
    return (e[0], e[1]) if upper else (e[2], e[3])


def corner_entry(T, i, off):
    """the corner rule for edge i of T at its upper (off 1) or lower (off -1) vertex: the entry that replaces the
    edge's crossing on that vertex's row, or None"""
    c = T[i]
    if c[6] == 0:
        return None
    vertex = end_vertex(c, off)
    for k in range(i):
        o = T[k]
        if o[6] == 0 or end_vertex(o, off) != vertex:
            continue
        if (o[6] > 0) != (c[6] > 0):
            return None
        y = vertex[1] + off
        a, b = crossing(c, y), crossing(o, y)
        if (off == -1) == (c[6] > 0):
            r = round_half_up(max(a, b)) + 1
            return f32(r) if r <= vertex[0] else None
        r = round_half_up(min(a, b)) - 1
        return f32(r) if r >= vertex[0] else None
    return None


def row_entries(T, y, last_row):
    """the row's unsorted entry list: T the non-horizontal edges in order, last_row the polygon's clipped ymax"""
    xx = []
    for i, c in enumerate(T):
        if not (c[4] <= y <= c[5]):
            continue
        x = crossing(c, y)
        if y == c[5] and y < last_row:
            xx += [x, x]
            continue
        r = None
        if y == c[4] and y < last_row:
            r = corner_entry(T, i, 1)
        elif y == c[5] and y == last_row:
            r = corner_entry(T, i, -1)
        xx.append(x if r is None else r)
    return xx


def row_spans(xx):
    """sorted pairs -> the [x_start, x_end] spans Pillow hands to its hline, before clipping"""
    xx = sorted(xx)
    x_pos = 0
    spans = []
    for i in range(1, len(xx), 2):
        x_end = round_half_down(xx[i])
        if x_end < x_pos:
            continue
        x_start = round_half_up(xx[i - 1])
        if x_pos > x_start:
            x_start = x_pos
            if x_end < x_start:
                continue
        spans.append((x_start, x_end))
        x_pos = x_end + 1
    return spans


def fill_polygon(img, xy, value):
    """paints `value` into the 2-D array `img` in place, as ImageDraw.polygon(xy, fill=value) would"""
    H, W = img.shape
    pts = int_points(xy)

    def hline(x0, y, x1):
        if 0 <= y < H:
            x0, x1 = max(x0, 0), min(x1, W - 1)
            if x0 <= x1:
                img[y, x0:x1 + 1] = value

    E = edge_list(pts)
    ymin, ymax, T = H - 1, 0, []
    for e in E:
        ymin, ymax = min(ymin, e[4]), max(ymax, e[5])
        if e[4] == e[5]:
            hline(min(e[0], e[2]), e[4], max(e[0], e[2]))
        else:
            T.append(e)
    ymin, ymax = max(ymin, 0), min(ymax, H)
    for y in range(ymin, ymax + 1):
        for xs, xe in row_spans(row_entries(T, y, ymax)):
            hline(xs, y, xe)
    return img


def paint(H, W, polygons, dtype=np.int32, background=0):
    """polygons: iterable of (xy, value), painted in order"""
    img = np.full((H, W), background, dtype)
    for xy, v in polygons:
        fill_polygon(img, xy, v)
    return img


def comb(teeth, x0=0, y_top=1, y_bottom=9, pitch=2):
    """`teeth` spikes on a bar: a row through the spikes has 2 * teeth crossings"""
    pts = [(x0, y_bottom)]
    for t in range(teeth):
        pts += [(x0 + pitch * t, y_bottom - 2), (x0 + pitch * t, y_top), (x0 + pitch * t + 1, y_top),
                (x0 + pitch * t + 1, y_bottom - 2)]
    return pts + [(x0 + pitch * teeth, y_bottom)]


HAND_CASES = {
    "axis_rectangle": [(2, 3), (12, 3), (12, 9), (2, 9)],
    "horizontal_runs": [(1, 2), (5, 2), (9, 2), (9, 7), (13, 7), (6, 7), (1, 7)],
    "vertical_runs": [(3, 1), (3, 5), (3, 10), (8, 10), (8, 4), (8, 1)],
    "repeated_points": [(2, 2), (2, 2), (11, 4), (11, 4), (11, 4), (5, 10)],
    "closed_explicitly": [(2, 2), (12, 3), (6, 11), (2, 2)],
    "two_points": [(2, 3), (11, 8)],
    "two_points_flat": [(2, 3), (11, 3)],
    "two_points_same": [(4, 4), (4, 4)],
    "bow_tie": [(1, 1), (13, 10), (13, 1), (1, 10)],
    "comb_70_crossings": comb(35),
    "wholly_left": [(-20, 2), (-3, 4), (-9, 12)],
    "wholly_below": [(2, 30), (9, 34), (4, 40)],
    "wholly_above": [(2, -30), (9, -34), (4, -4)],
    "over_every_edge": [(-6, -5), (30, -2), (25, 20), (-3, 17)],
    "apex_pairs": [(29, 0), (18, 0), (10, 4)],
    "retraced_edge": [(3, 3), (7, 2), (0, 6), (3, 0), (7, 2)],
    "float_vertices": [(1.9, 1.9), (13.9, -0.9), (-0.5, 11.99), (6.5, 6.5)],
}


def owner_from_tables(edges, polys, jobs, B, H, W):
    """the device kernel's arithmetic on the host tables of include/dspn_polygon.h (dataset/cityscapes_labels.py builds
    them), row job by row job: what dspn_polygon_rasterize must write.  -> owner (B, H, W) int32"""
    owner = np.zeros((B, H, W), np.int32)

    def span(b, y, xa, xb, order):
        xa, xb = max(xa, 0), min(xb, W - 1)
        if xa <= xb:
            owner[b, y, xa:xb + 1] = np.maximum(owner[b, y, xa:xb + 1], order)

    for p, y, last_row, cap, _ in jobs.tolist():
        e0, e1, b, order = polys[p].tolist()
        xx = []
        for x0, y0, ymin, ymax, dxb, topb, botb, x1 in edges[e0:e1].tolist():
            dx, top, bot = (np.array([v], np.int32).view(np.float32)[0] for v in (dxb, topb, botb))
            if ymin == ymax:
                if ymin == y:
                    span(b, y, min(x0, x1), max(x0, x1), order)
                continue
            if not (ymin <= y <= ymax):
                continue
            x = f32(f32(f32(y - y0) * dx) + f32(x0))
            if y == ymax and y < last_row:
                xx += [x, x]
                continue
            if y == ymin and y < last_row and top == top:
                x = top
            elif y == ymax and y == last_row and bot == bot:
                x = bot
            xx.append(x)
        assert len(xx) <= cap, (len(xx), cap)
        xx.sort()
        for i in range(1, len(xx), 2):
            span(b, y, round_half_up(xx[i - 1]), round_half_down(xx[i]), order)
    return owner


def street_scene(seed, H=1024, W=2048, cars=40, people=40):
    """a seeded street-like scene of about 100 integer polygons, in painter's order: sky, buildings with jagged
    rooflines, vegetation, road, sidewalk, then poles, vehicles and people, some of them partly outside the image"""
    rng = np.random.default_rng(seed)
    polys = []

    def jagged(xa, xb, base, amp, step):
        xs = list(range(xa, xb, step)) + [xb]
        return [(x, int(base + rng.integers(-amp, amp + 1))) for x in xs]

    horizon = H * 4 // 10
    polys.append([(0, 0), (W - 1, 0), (W - 1, horizon), (0, horizon)])
    x = -20
    while x < W:
        w = int(rng.integers(W // 12, W // 5))
        polys.append(jagged(x, x + w, horizon - int(rng.integers(H // 8, H // 3)), H // 60 + 1, max(W // 90, 2))
                     + [(x + w, horizon + H // 20), (x, horizon + H // 20)])
        x += w - int(rng.integers(0, W // 40 + 1))
    for _ in range(4):
        cx, cy = int(rng.integers(0, W)), horizon - int(rng.integers(0, H // 6))
        r = int(rng.integers(H // 12, H // 5))
        ang = np.sort(rng.uniform(0, 2 * np.pi, 40))
        polys.append([(int(cx + r * rng.uniform(0.7, 1.1) * np.cos(t)), int(cy + r * rng.uniform(0.7, 1.1) * np.sin(t)))
                      for t in ang])
    polys.append(jagged(0, W - 1, horizon + H // 20, 2, max(W // 30, 2)) + [(W - 1, H + 5), (0, H + 5)])
    polys.append(jagged(0, W // 3, horizon + H // 16, 3, max(W // 50, 2)) + [(W // 5, H - 1), (-8, H - 1)])
    for _ in range(8):
        px, top = int(rng.integers(0, W)), int(rng.integers(H // 10, horizon))
        polys.append([(px, top), (px + max(W // 300, 1), top), (px + max(W // 300, 1), horizon + H // 8), (px, horizon + H // 8)])
    for _ in range(cars):
        cx, cy = int(rng.integers(-W // 20, W)), int(rng.integers(horizon, H))
        w, h = int(rng.integers(W // 40, W // 8)), int(rng.integers(H // 30, H // 8))
        polys.append([(cx, cy), (cx + w // 5, cy - h), (cx + 4 * w // 5, cy - h), (cx + w, cy), (cx + w, cy + h // 2),
                      (cx + 3 * w // 4, cy + h // 2 + 2), (cx + w // 4, cy + h // 2 + 2), (cx, cy + h // 2)])
    for _ in range(people):
        cx, cy = int(rng.integers(0, W)), int(rng.integers(horizon, H))
        w, h = int(rng.integers(max(W // 200, 2), W // 40 + 3)), int(rng.integers(H // 30, H // 6))
        polys.append([(cx, cy), (cx + w // 2, cy - h // 6), (cx + w, cy), (cx + w + 1, cy + h // 2), (cx + w - 1, cy + h),
                      (cx + w // 2, cy + h - h // 3), (cx + 1, cy + h), (cx - 1, cy + h // 2)])
    return polys
