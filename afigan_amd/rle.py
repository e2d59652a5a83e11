"""COCO run-length encoding of binary masks on the host (numpy only): what pycocotools' mask API gives an evaluator, restated from the format.

A mask [H, W] is read in column-major order, j = x H + y, with f[-1] = 0.  A *start* is a j with f[j] != f[j - 1]; with the starts
B_0 < ... < B_{m-1} the *counts* are [B_0, B_1 - B_0, ..., H W - B_{m-1}]: m + 1 run lengths, zeros first (the first is 0 when f[0] = 1),
[H W] for an empty mask.  The *string* writes every count c_i (c_i - c_{i-2} when i > 2) as 5-bit groups, low bits first, bit 5 = "another
group follows", each group + 48 as one character; the value ends at the first group from which sign extension (bit 4) restores it.
An RLE is ``{"size": [H, W], "counts": str}``; ``decode`` and ``area`` also take the uncompressed form (``counts`` a sequence of ints).

The device side (ops.mask_paste_rle) returns the starts; ``counts_from_starts`` and ``to_strings`` turn a whole image's detections into
strings without a Python loop per run.  ``from_polygons`` is pycocotools' polygon-to-RLE conversion, rasterised on the device
(ops.polygons_rle, csrc/poly_rle.hip)."""
import numpy as np


def encode(mask):
    """The counts (int64 array) of a bool / uint8 [H, W] mask."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"rle.encode: a [H, W] mask expected, got shape {m.shape}")
    f = (m != 0).T.reshape(-1)                                           # column-major
    n = f.size
    starts = np.flatnonzero(f != np.concatenate(([False], f[:-1])))
    return np.diff(np.concatenate(([0], starts, [n]))).astype(np.int64)


def counts_from_starts(starts, nstarts, hw):
    """The counts of every detection from the packed starts of ops.mask_paste_rle: ``starts`` [T] (detection after detection, ascending inside
    one), ``nstarts`` [R], ``hw`` = (H, W).  A list of R int64 arrays."""
    starts = np.asarray(starts).astype(np.int64).reshape(-1)
    nstarts = np.asarray(nstarts).astype(np.int64).reshape(-1)
    n = int(hw[0]) * int(hw[1])
    if int(nstarts.sum()) != starts.size:
        raise ValueError(f"rle.counts_from_starts: {starts.size} starts for nstarts summing to {int(nstarts.sum())}")
    out, o = [], 0
    for k in nstarts.tolist():
        out.append(np.diff(starts[o:o + k], prepend=0, append=n))
        o += k
    return out


def _deltas(counts):
    x = np.array(counts, dtype=np.int64).reshape(-1)
    if x.size > 3:
        x[3:] -= np.asarray(counts, dtype=np.int64).reshape(-1)[1:-2]
    return x


def to_strings(counts_list):
    """The strings of many count sequences at once (one pass of array operations over all their values)."""
    xs = [_deltas(c) for c in counts_list]
    if not xs:
        return []
    x = np.concatenate(xs) if len(xs) > 1 else xs[0]
    # groups per value: the smallest k >= 1 with -2^(5k-1) <= x < 2^(5k-1), i.e. bit_length(x >= 0 ? x : ~x) + 1 sign bit, in fives
    y = np.where(x >= 0, x, ~x)
    if y.size and int(y.max()) >= 1 << 52:
        raise ValueError("rle.to_strings: a count beyond 2^52")
    k = np.maximum(1, (np.frexp(y.astype(np.float64))[1].astype(np.int64) + 5) // 5)     # frexp's exponent of an integer is its bit length
    ends = np.cumsum(k)
    total = int(ends[-1]) if ends.size else 0
    owner = np.repeat(np.arange(x.size), k)
    pos = np.arange(total) - np.repeat(ends - k, k)
    g = (x[owner] >> (5 * pos)) & 31
    g |= np.where(pos < k[owner] - 1, 32, 0)
    buf = (g + 48).astype(np.uint8).tobytes()
    out, v = [], 0
    for c in xs:                                                        # one slice per sequence
        n = int(k[v:v + c.size].sum())
        o = int(ends[v - 1]) if v else 0
        out.append(buf[o:o + n].decode("ascii"))
        v += c.size
    return out


def to_string(counts):
    return to_strings([counts])[0]


def from_string(s):
    """The counts (int64 array) of a COCO RLE string."""
    if isinstance(s, str):
        s = s.encode("ascii")
    g = np.frombuffer(bytes(s), dtype=np.uint8).astype(np.int64) - 48
    if g.size == 0:
        return np.zeros(0, np.int64)
    if ((g < 0) | (g > 63)).any() or g[-1] & 32:
        raise ValueError("rle.from_string: not a COCO RLE string")
    last = (g & 32) == 0                                                # the last group of its value
    first = np.concatenate(([0], np.flatnonzero(last)[:-1] + 1))
    pos = np.arange(g.size) - np.repeat(first, np.diff(np.concatenate((first, [g.size]))))
    if pos.max() > 11:
        raise ValueError("rle.from_string: a value of more than 12 groups")
    x = np.add.reduceat((g & 31) << (5 * pos), first)
    k = pos[last] + 1
    x = np.where(g[last] & 16, x | (np.int64(-1) << (5 * k)), x)        # sign extension from bit 4 of the last group
    # c_i = x_i + c_{i-2} for i > 2: running sums along the odd indices from 1 and along the even indices from 2
    c = x.copy()
    c[1::2] = np.cumsum(x[1::2])
    if c.size > 2:
        c[2::2] = np.cumsum(x[2::2])
    return c


def _counts_of(rle):
    c = rle["counts"]
    return from_string(c) if isinstance(c, (str, bytes)) else np.asarray(c, dtype=np.int64).reshape(-1)


def decode(rle):
    """The bool [H, W] mask of an RLE ({"size": [H, W], "counts": str or sequence})."""
    H, W = (int(v) for v in rle["size"])
    c = _counts_of(rle)
    if (c < 0).any() or int(c.sum()) != H * W:
        raise ValueError(f"rle.decode: counts summing to {int(c.sum())} for a {H} x {W} mask")
    f = np.repeat(np.arange(c.size) & 1, c).astype(bool)
    return np.ascontiguousarray(f.reshape(W, H).T)


def area(rle):
    """The number of set pixels."""
    return int(_counts_of(rle)[1::2].sum())


def from_polygons(polygons, sizes):
    """pycocotools' frPyObjects + merge for polygon annotations, on the GPU (ops.polygons_rle): ``polygons`` a list of N annotations, each a list
    of flat coordinate sequences; ``sizes`` (H, W) or one pair per annotation.  A list of N ``{"size": [H, W], "counts": str}``."""
    from . import ops
    _, _, _, hw2, _ = ops.polygons_batch(polygons, sizes)                  # (checked here too, so that nothing is uploaded for a bad input)
    starts, start_off, _ = ops.polygons_rle(polygons, sizes)
    starts, off = starts.cpu().numpy().astype(np.int64), start_off.cpu().numpy()
    counts = [np.diff(starts[off[i]:off[i + 1]], prepend=0, append=int(hw2[i, 0]) * int(hw2[i, 1])) for i in range(len(polygons))]
    return [{"size": [int(h), int(w)], "counts": s} for (h, w), s in zip(hw2.tolist(), to_strings(counts))]


def to_rle(counts, hw):
    return {"size": [int(hw[0]), int(hw[1])], "counts": to_string(counts)}
