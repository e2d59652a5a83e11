"""Plain-loop checker of the polygon rasteriser: pycocotools' rleFrPoly restated point by point in Python floats (IEEE
fp64, every operation rounded once) and lists.  The union of an annotation's polygons is decode / OR / rle.encode, not the kernels' sweep.

``fused=True`` evaluates step 2 as a contracting compiler would, ``fma(s, t, ys)`` (one rounding of the exact ys + s t, through ``fractions``): the
GPU test uses it to show that its polygons tell a contracted kernel from the stated one."""
import math
from fractions import Fraction

import numpy as np

from afigan_amd import rle


def _lin(b, s, t, fused):
    """(int)(b + s t + .5)"""
    if fused:
        return int(float(Fraction(b) + Fraction(s) * Fraction(t)) + .5)
    return int(b + s * t + .5)


def boundary_points(xy, fused=False):
    """Step 1 and 2: the upsampled boundary points (u, v) of a polygon given as a flat coordinate sequence."""
    k = len(xy) // 2
    X = [int(5 * float(xy[2 * j]) + .5) for j in range(k)]
    Y = [int(5 * float(xy[2 * j + 1]) + .5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ye - ys)
        if dx == 0 and dy == 0:
            u.append(xs)
            v.append(ys)
            continue
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        s = float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy
        n = max(dx, dy)
        for d in range(n + 1):
            t = n - d if flip else d
            if dx >= dy:
                u.append(t + xs)
                v.append(_lin(ys, s, t, fused))
            else:
                u.append(_lin(xs, s, t, fused))
                v.append(t + ys)
    return u, v


def crossings(xy, H, W, fused=False):
    """Step 3: the crossing values a, in boundary order (0 <= a <= H W)."""
    u, v = boundary_points(xy, fused)
    out = []
    for p in range(1, len(u)):
        if u[p] == u[p - 1]:
            continue
        xd = float(u[p] if u[p] < u[p - 1] else u[p] - 1)
        xd = (xd + .5) / 5 - .5
        if math.floor(xd) != xd or xd < 0 or xd > W - 1:
            continue
        yd = float(min(v[p], v[p - 1]))
        yd = (yd + .5) / 5 - .5
        yd = 0.0 if yd < 0 else (float(H) if yd > H else yd)
        yd = math.ceil(yd)
        out.append(int(xd) * H + int(yd))
    return out


def poly_starts(xy, H, W, fused=False):
    """Step 4: the crossing values of odd multiplicity below H W, ascending."""
    count = {}
    for a in crossings(xy, H, W, fused):
        count[a] = count.get(a, 0) + 1
    return sorted(a for a, c in count.items() if c & 1 and a < H * W)


def mask_of_starts(starts, H, W):
    """The bool [H, W] mask of ascending starts: pixel (y, x) is set iff the number of starts <= x H + y is odd."""
    f = [False] * (H * W)
    on, i = False, 0
    for j in range(H * W):
        while i < len(starts) and starts[i] <= j:
            on = not on
            i += 1
        f[j] = on
    return np.array(f, dtype=bool).reshape(W, H).T.copy()


def poly_mask(xy, H, W, fused=False):
    return mask_of_starts(poly_starts(xy, H, W, fused), H, W)


def ann_mask(polys, H, W, fused=False):
    """Step 5: the union of an annotation's polygons (no polygon: the empty mask)."""
    m = np.zeros((H, W), dtype=bool)
    for xy in polys:
        m |= poly_mask(xy, H, W, fused)
    return m


def ann_counts(polys, H, W, fused=False):
    return rle.encode(ann_mask(polys, H, W, fused))


def ann_starts(polys, H, W, fused=False):
    return [int(v) for v in np.cumsum(ann_counts(polys, H, W, fused))[:-1]]
