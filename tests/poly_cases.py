"""Inputs of the polygon rasteriser's tests (tests/test_poly_host.py, tests/test_gpu_poly.py) and the checker's answers for them, each computed
once per session by tests/poly_f64.py; treat everything returned here as read-only.  Nothing here touches the GPU."""
import numpy as np

import poly_f64 as Q

HAND = (  # (polygon, (H, W), crossings, starts, area, (x0, x1, y0, y1) of the set pixels)
    ([2, 2, 8, 2, 8, 7, 2, 7], (12, 14), 12, 12, 30, (2, 7, 2, 6)),
    ([2.5, 2.5, 8.5, 2.5, 8.5, 7.5, 2.5, 7.5], (12, 14), 12, 12, 30, (3, 8, 3, 7)),
    ([1, 1, 12, 3, 6, 10], (12, 14), 22, 20, 43, None),
    ([10, 10, 60, 10, 60, 60], (80, 70), 100, 98, 1225, None),
)

RANDOM_SEED, RANDOM_N = 26, 400                        # chosen on the checker: tests/test_poly_host.py holds the floor on the fused form
CANVASES = ((5, 5), (40, 37), (1, 9), (9, 1), (7, 12), (12, 14), (33, 25), (16, 40), (23, 8), (40, 5))


def _vertex(rng, lim, mode):
    v = rng.uniform(-6.0, lim + 6.0)                    # up to 6 px outside the canvas on every side
    if mode == 0:
        return float(round(v))
    if mode == 1:
        return round(v * 2) / 2
    return float(v)


def _polygon(rng, H, W, k=None, mode=None):
    k = int(rng.integers(3, 13)) if k is None else k
    mode = int(rng.integers(3)) if mode is None else mode
    xy = []
    for _ in range(k):
        xy += [_vertex(rng, W, mode), _vertex(rng, H, mode)]
    return xy


def special_polygons():
    """(polygon, (H, W), what): the shapes the issue names."""
    return [([3.0, 4.0], (9, 8), "one vertex"),
            ([1.0, 1.0, 6.0, 7.0], (9, 8), "two vertices"),
            ([1.0, 1.0, 1.0, 1.0, 6.0, 2.0, 6.0, 2.0, 3.0, 8.0], (10, 9), "repeated consecutive vertices"),
            ([-5.0, -5.0, -1.0, -5.0, -1.0, -1.0, -5.0, -1.0], (9, 8), "left of and above the canvas"),
            ([20.0, 2.0, 25.0, 2.0, 25.0, 7.0], (9, 8), "right of the canvas"),
            ([1.0, 12.0, 6.0, 12.0, 6.0, 15.0, 1.0, 15.0], (9, 8), "below the canvas"),
            ([-3.0, -3.0, 12.0, -3.0, 12.0, 13.0, -3.0, 13.0], (9, 8), "covers the whole canvas"),
            ([0.0, 0.0, 8.0, 0.0, 8.0, 9.0, 0.0, 9.0], (9, 8), "the canvas itself")]


_CACHE = {}


def random_set():
    """[(polygon, (H, W))]: RANDOM_N seeded polygons of 3 to 12 vertices, integer / half-integer / arbitrary, on the CANVASES, then the specials."""
    if "random" not in _CACHE:
        rng = np.random.default_rng(RANDOM_SEED)
        out = []
        for i in range(RANDOM_N):
            H, W = CANVASES[i % len(CANVASES)]
            out.append((_polygon(rng, H, W), (H, W)))
        out += [(p, hw) for p, hw, _ in special_polygons()]
        _CACHE["random"] = out
    return _CACHE["random"]


def random_set_starts(fused=False):
    key = "random starts fused" if fused else "random starts"
    if key not in _CACHE:
        _CACHE[key] = [Q.poly_starts(p, H, W, fused) for p, (H, W) in random_set()]
    return _CACHE[key]


def union_set():
    """[(polygons of one annotation, (H, W), what)]: 1 to 4 polygons, masks of different sizes."""
    if "union" not in _CACHE:
        rng = np.random.default_rng(RANDOM_SEED + 1)
        box = lambda x0, y0, x1, y1: [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]   # noqa: E731
        out = [([box(2, 2, 9, 9), box(5, 4, 14, 12)], (16, 18), "overlapping"),
               ([box(1, 1, 5, 5), box(8, 7, 13, 12)], (16, 18), "disjoint"),
               ([box(1, 1, 14, 14), box(4, 4, 9, 9)], (16, 18), "nested"),
               ([[1.0, 1.0, 12.0, 3.0, 6.0, 10.0]] * 2, (12, 14), "identical twice"),
               ([], (7, 9), "no polygon"),
               ([box(2, 2, 6, 6), box(6, 2, 10, 6)], (9, 12), "sharing an edge"),
               ([box(0, 0, 5, 4), box(0, 4, 5, 8)], (8, 5), "one ends where the next column starts"),
               ([box(-3, -3, 20, 20), [2.0, 2.0, 5.0, 2.0, 4.0, 6.0]], (11, 13), "everything and a triangle")]
        for i in range(40):
            H, W = CANVASES[(3 * i + 1) % len(CANVASES)]
            out.append(([_polygon(rng, H, W) for _ in range(int(rng.integers(1, 5)))], (H, W), "random"))
        _CACHE["union"] = out
    return _CACHE["union"]


def union_set_starts():
    if "union starts" not in _CACHE:
        _CACHE["union starts"] = [Q.ann_starts(ps, H, W) for ps, (H, W), _ in union_set()]
    return _CACHE["union starts"]


def zigzag(teeth, H=8):
    """A comb along a canvas H = 8 px high: `teeth` edges that rise and fall between y = 1 and y = 7 every 2 px, closed along the bottom.  Each
    tooth edge crosses two pixel columns and the bottom edge every column, so on a canvas of W >= 2 teeth columns it has 4 teeth crossings
    (teeth + 3 vertices), and on W = 2 teeth - 1 columns two fewer."""
    xy = []
    for i in range(teeth + 1):
        xy += [2.0 * i, 1.0 if i % 2 == 0 else 7.0]
    xy += [2.0 * teeth, float(H), 0.0, float(H)]
    return xy


def zigzag_case(crossings):
    """(polygon, (H, W)) of a zigzag with exactly `crossings` crossings (even: a closed boundary passes every column an even number of times)."""
    assert crossings % 2 == 0 and crossings >= 6
    if crossings % 4 == 0:
        teeth = crossings // 4
        return zigzag(teeth), (8, 2 * teeth)
    teeth = (crossings + 2) // 4
    return zigzag(teeth), (8, 2 * teeth - 1)
