"""numpy restatement of pycocotools' polygon rasteriser (rleFrPoly, then rleMerge as a union over an annotation's parts), written from the
rules in include/mi355det.h, for tests/test_oracle_poly.py and tests/test_gpu_poly.py.

It is deliberately the slow, literal form: the walk is one concatenated list of points (not edge by edge), the run lengths come from the
sort and the skip-a-zero-difference loop (not from the parity of the multiplicities), and the union goes through bitmaps and `any`.  The
kernels use the shortcuts; the two structural facts that license them are tested against this file, not assumed by it.

Python floats and numpy float64 are IEEE doubles without fused multiply-add, int() and astype(int64) truncate toward zero like the C cast,
and int / int is the correctly rounded quotient, which is what `(double)(ye-ys)/dx` gives for these magnitudes."""
import numpy as np

from object_detectors_amd.rle import counts_stats
from tests import rle_oracle as ro


def scale(xy):
    """Step 1: X[j] = (int)(5*x[j] + .5), Y likewise, the ring closed with X[k] = X[0]."""
    k = len(xy) // 2
    X = [int(5 * float(xy[2 * j]) + .5) for j in range(k)]
    Y = [int(5 * float(xy[2 * j + 1]) + .5) for j in range(k)]
    return X + [X[0]], Y + [Y[0]]


def walk_edge(xs, ys, xe, ye):
    """Step 2 for one edge: (u, v) int64 arrays of its dx + 1 or dy + 1 points, from the original start to the original end."""
    dx, dy = abs(xe - xs), abs(ys - ye)
    flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
    if flip:
        xs, xe, ys, ye = xe, xs, ye, ys
    if dx == 0 and dy == 0:
        # C computes s = 0/0 and v = (int)NaN here.  The point's v is never read: both pairs it belongs to have equal u, or are dropped
        # for xd < 0 before yd is looked at (tests/test_oracle_poly.py::test_zero_length_edge_v_is_never_read).
        return np.asarray([xs], np.int64), np.asarray([ys], np.int64)
    s = (ye - ys) / dx if dx >= dy else (xe - xs) / dy
    n = dx if dx >= dy else dy
    d = np.arange(n + 1, dtype=np.int64)
    t = n - d if flip else d
    if dx >= dy:
        u = t + xs
        v = np.trunc(ys + s * t.astype(np.float64) + .5).astype(np.int64)
    else:
        v = t + ys
        u = np.trunc(xs + s * t.astype(np.float64) + .5).astype(np.int64)
    return u, v


def boundary_points(u, v, h, w):
    """Step 3 over one list of walk points: the kept a = x*h + y, in walk order (int64)."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    j = np.flatnonzero(u[1:] != u[:-1]) + 1
    xd = np.where(u[j] < u[j - 1], u[j], u[j] - 1).astype(np.float64)
    xd = (xd + .5) / 5 - .5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    j, xd = j[keep], xd[keep]
    yd = np.minimum(v[j], v[j - 1]).astype(np.float64)
    yd = (yd + .5) / 5 - .5
    yd = np.where(yd < 0, 0.0, np.where(yd > h, float(h), yd))
    yd = np.ceil(yd)
    return xd.astype(np.int64) * h + yd.astype(np.int64)


def polygon_points(xy, h, w):
    """Steps 1-3: the whole ring walked as ONE list (the edges' points one after the other)."""
    X, Y = scale(xy)
    us, vs = zip(*[walk_edge(X[j], Y[j], X[j + 1], Y[j + 1]) for j in range(len(X) - 1)])
    return boundary_points(np.concatenate(us), np.concatenate(vs), h, w)


def polygon_points_per_edge(xy, h, w):
    """The points of each edge walked ALONE, concatenated: what structural fact (b) says is the same multiset."""
    X, Y = scale(xy)
    return np.concatenate([boundary_points(*walk_edge(X[j], Y[j], X[j + 1], Y[j + 1]), h, w) for j in range(len(X) - 1)])


def points_to_counts(a, h, w):
    """Step 4, the loop of rleFrPoly: h*w appended, sorted, differences; a zero difference is skipped together with the one after it."""
    a = sorted(int(v) for v in a) + [h * w]
    diffs = [a[0]] + [a[j] - a[j - 1] for j in range(1, len(a))]
    b = [diffs[0]]
    j = 1
    while j < len(diffs):
        if diffs[j] > 0:
            b.append(diffs[j])
            j += 1
        else:
            j += 1
            if j < len(diffs):
                b[-1] += diffs[j]
                j += 1
    return np.asarray(b, np.int64)


def polygon_counts(xy, h, w):
    """frPyObjects of one polygon: int64 counts."""
    return points_to_counts(polygon_points(xy, h, w), h, w)


def parts_of(seg):
    """A list of polygons, or one flat polygon -> list of polygons."""
    return [seg] if len(seg) and not isinstance(seg[0], (list, tuple, np.ndarray)) else list(seg)


def annotation_mask(seg, h, w):
    """Step 5: decode every part, `any` over them (the reference's convert_coco_poly_to_mask); uint8 [h, w]."""
    m = np.zeros((h, w), bool)
    for poly in parts_of(seg):
        c = polygon_counts(poly, h, w)
        # rleDecode of counts that may hold zeros: alternating runs, beginning with zeros
        bits = np.repeat(np.arange(c.size) & 1, c).astype(bool)
        assert bits.size == h * w
        m |= bits.reshape(w, h).T
    return m.astype(np.uint8)


def annotation_counts(seg, h, w):
    """merge(frPyObjects(seg, h, w)): the canonical run lengths of the union."""
    return ro.encode(annotation_mask(seg, h, w))


def random_polygon(rng, h, w, decimals, k=None):
    """A seeded test polygon: k vertices (3..11 unless given) from -6 to size + 6 on all sides, rounded to `decimals` (0, 1, 2: the
    rounding ties of 5x + .5 and the u = 2 (mod 5) columns), sometimes with a repeated vertex or a vertex on the line of an edge."""
    k = int(rng.integers(3, 12)) if k is None else k
    pts = np.round(np.stack([rng.uniform(-6, w + 6, k), rng.uniform(-6, h + 6, k)], 1), decimals)
    mode, j = int(rng.integers(0, 4)), int(rng.integers(0, k))
    if mode == 0:                                            # a repeated vertex: a zero-length edge
        pts = np.insert(pts, j, pts[j], 0)
    elif mode == 1:                                          # a vertex between two others (collinear up to the rounding)
        pts = np.insert(pts, j + 1, np.round((pts[j] + pts[(j + 1) % k]) / 2, decimals), 0)
    return [float(v) for v in pts.reshape(-1)]


def random_annotation(rng, h, w, parts=None):
    """1 to 5 polygons (0 decimals, 1 or 2, drawn per polygon)."""
    parts = int(rng.integers(1, 6)) if parts is None else parts
    return [random_polygon(rng, h, w, int(rng.integers(0, 3))) for _ in range(parts)]


def encode_annotations(segs, sizes):
    """[(seg, (h, w))] -> (concatenated int64 counts, offsets list [A + 1], area int64 [A], bbox int32 [A, 4]); area and box by
    rle.counts_stats, annotation by annotation (the sizes may differ)."""
    cs = [annotation_counts(s, h, w) for s, (h, w) in zip(segs, sizes)]
    offs = np.concatenate([[0], np.cumsum([c.size for c in cs])]).astype(np.int64).tolist()
    area, bbox = np.zeros(len(cs), np.int64), np.zeros((len(cs), 4), np.int32)
    for j, (c, (h, _w)) in enumerate(zip(cs, sizes)):
        a, b = counts_stats(c, [0, c.size], h)
        area[j], bbox[j] = a[0], b[0]
    return (np.concatenate(cs) if cs else np.zeros(0, np.int64)), offs, area, bbox
