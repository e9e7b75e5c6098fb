"""tests/poly_oracle.py (pycocotools rleFrPoly + the union over an annotation's parts, restated) pinned by hand-checked cases, and the two
structural facts the kernels of csrc/poly_kernels.hip rely on, checked against it over seeded random polygons.  CPU only.

Hand work for three of the pinned cases (u, v are 5x upsampled; a kept point is a = x*h + y):

12 x 12, [1,1, 9,1, 9,9, 1,9]: the ring is (5,5) -> (45,5) -> (45,45) -> (5,45) -> (5,5).
  top edge     x-major, u rises 5..45, v = 5.  xd = (u-1+.5)/5 - .5 is an integer when u-1 = 7, 12, .., 42: x = 1..8.
               yd = (5+.5)/5 - .5 = .6, ceil 1.  a = 12x + 1 = 13, 25, .., 97.
  right edge   u stays 45: nothing.
  bottom edge  x-major, flipped, walked from u = 45 down to 5, v = 45.  u falls, so xd comes from u itself: u = 42, 37, .., 7: x = 8..1.
               yd = (45+.5)/5 - .5 = 8.6, ceil 9.  a = 12x + 9 = 21, 33, .., 105.
  left edge    nothing.
  sorted with 144 appended: 13 21 25 33 .. 97 105 144, differences 13, (8, 4) x 7, 8, 39: columns 1..8, rows 1..8.

12 x 12, [1,1, 9,1, 9,9]: (5,5) -> (45,5) -> (45,45) -> (5,5).
  top edge     as above: 13, 25, .., 97.
  right edge   nothing.
  diagonal     dx = dy = 40 counts as x-major, flipped, s = 1, walked from u = 45 down with v = u.  u = 42, .., 7: x = 8..1;
               yd = (min(v) + .5)/5 - .5 = (5x+2+.5)/5 - .5 = x exactly.  a = 13x = 104, 91, .., 13.
  sorted: 13 13 25 26 37 39 49 52 61 65 73 78 85 91 97 104 144.  The differences begin 13, 0, 12, 1, 11, 2: the 0 is skipped and the
  12 added to the first count, 25; then 1, 11, 2, 10, .., 6, 7, 40.  Column x holds rows 1..x-1 (column 1 is empty).

5 x 6, [-3,-3, 2.4,-3, 2.4,7, -3,7]: 5*-3 + .5 = -14.5 truncates toward zero to -14; 5*2.4 + .5 = 12.5 to 12; 5*7 + .5 to 35.
  top edge     u rises -14..12, v = -14: u-1 = -13, -8, -3, 2, 7 give xd = -3, -2, -1, 0, 1; the negative ones are dropped.
               yd = (-14+.5)/5 - .5 = -3.2, clamped to 0.  a = 0, 5.
  bottom edge  walked from u = 12 down, v = 35: u = 7, 2 give x = 1, 0 (u = -3, -8, -13 dropped).  yd = 6.6, clamped to h = 5.  a = 10, 5.
  sorted with 30 appended: 0 5 5 10 30, differences 0, 5, 0, 5, 20: the first count is 0, then 5, the 0 is skipped and the 5 after it
  added: [0, 10, 20].  Columns 0 and 1 are full."""
import numpy as np
import pytest

from tests import poly_oracle as po
from tests import rle_oracle as ro

SQUARE = [1, 1, 9, 1, 9, 9, 1, 9]
SQUARE_COUNTS = [13, 8, 4, 8, 4, 8, 4, 8, 4, 8, 4, 8, 4, 8, 4, 8, 39]

PINNED = [
    (12, 12, SQUARE, SQUARE_COUNTS),
    (12, 12, [1, 1, 9, 1, 9, 9], [25, 1, 11, 2, 10, 3, 9, 4, 8, 5, 7, 6, 6, 7, 40]),
    (4, 4, [0, 0, 4, 0, 4, 4, 0, 4], [0, 16]),
    (5, 6, [-3, -3, 2.4, -3, 2.4, 7, -3, 7], [0, 10, 20]),
    (6, 6, [3, 3, 3, 3, 3, 3], [36]),
    (4, 4, [1.5, 1.5, 1.9, 1.6, 1.7, 1.9], [16]),
    (3, 6, [.5, .5, 5.5, .5, 5.5, 2.5, .5, 2.5], [4, 2, 1, 2, 1, 2, 1, 2, 1, 2]),
    (5, 5, [2, 1, 5, 1, 5, 6, 2, 6], [11, 4, 1, 4, 1, 4]),
    (10, 9, [2.5, .5, 7.3, 3.2, 4.1, 8.8], [31, 4, 7, 6, 4, 4, 7, 2, 25]),
]

SIZES = [(1, 1), (7, 5), (37, 53), (5, 30), (30, 4)]


def box_mask(h, w, *boxes):
    m = np.zeros((h, w), np.uint8)
    for x0, y0, x1, y1 in boxes:
        m[y0:y1, x0:x1] = 1
    return m


# (parts, the union's pixels by hand as [x0, y0, x1, y1) boxes): an xor over the parts fails every one of them but the touching pair
UNIONS = [
    ("overlapping", [SQUARE, [5, 5, 11, 5, 11, 11, 5, 11]], [(1, 1, 9, 9), (5, 5, 11, 11)]),
    ("nested", [SQUARE, [3, 3, 6, 3, 6, 6, 3, 6]], [(1, 1, 9, 9)]),
    ("touching", [[1, 1, 5, 1, 5, 9, 1, 9], [5, 1, 9, 1, 9, 9, 5, 9]], [(1, 1, 9, 9)]),
    ("duplicated", [SQUARE, SQUARE], [(1, 1, 9, 9)]),
    ("three deep", [SQUARE, SQUARE, [3, 3, 6, 3, 6, 6, 3, 6]], [(1, 1, 9, 9)]),
]


@pytest.mark.parametrize("h,w,poly,want", PINNED)
def test_pinned_polygons(h, w, poly, want):
    got = po.polygon_counts(poly, h, w)
    assert got.tolist() == want
    assert po.annotation_counts(poly, h, w).tolist() == ([c for c in want])          # one flat polygon is an annotation of one part
    assert po.annotation_counts([poly], h, w).tolist() == want


def test_pinned_square_is_the_pixels_1_to_8():
    assert np.array_equal(po.annotation_mask([SQUARE], 12, 12), box_mask(12, 12, (1, 1, 9, 9)))
    assert np.array_equal(ro.decode(SQUARE_COUNTS, 12, 12), box_mask(12, 12, (1, 1, 9, 9)))


@pytest.mark.parametrize("name,parts,boxes", UNIONS, ids=[u[0] for u in UNIONS])
def test_union_of_parts(name, parts, boxes):
    want = box_mask(12, 12, *boxes)
    assert np.array_equal(po.annotation_mask(parts, 12, 12), want)
    c = po.annotation_counts(parts, 12, 12)
    assert c.tolist() == ro.encode(want).tolist() and (c[1:] > 0).all()
    if name != "overlapping":
        assert c.tolist() == SQUARE_COUNTS


def test_empty_annotation_is_the_zero_mask():
    assert po.annotation_counts([], 5, 7).tolist() == [35]
    counts, offs, area, bbox = po.encode_annotations([[], [SQUARE]], [(5, 7), (12, 12)])
    assert offs == [0, 1, 1 + len(SQUARE_COUNTS)] and counts.tolist() == [35] + SQUARE_COUNTS
    assert area.tolist() == [0, 64] and bbox.tolist() == [[0, 0, 0, 0], [1, 1, 8, 8]]


def test_zero_length_edge_v_is_never_read():
    """C leaves v of a zero-length edge's point undefined ((int) of a NaN); poly_oracle.walk_edge puts ys there.  Any other value gives the
    same points, also where the vertex lies left of the image and u of the neighbouring y-major edges is off by one."""
    rng = np.random.default_rng(5)
    real = po.walk_edge
    try:
        for _ in range(300):
            h, w = SIZES[int(rng.integers(0, len(SIZES)))]
            poly = po.random_polygon(rng, h, w, int(rng.integers(0, 3)))
            j = 2 * int(rng.integers(0, len(poly) // 2))
            poly = poly[:j] + poly[j:j + 2] + poly[j:]                       # vertex j twice
            want = po.polygon_points(poly, h, w)
            po.walk_edge = lambda xs, ys, xe, ye: (real(xs, ys, xe, ye) if (xs, ys) != (xe, ye)
                                                   else (np.asarray([xs], np.int64), np.asarray([-(1 << 31)], np.int64)))
            got = po.polygon_points(poly, h, w)
            po.walk_edge = real
            assert np.array_equal(got, want)
    finally:
        po.walk_edge = real


def _random_cases(seed, n):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        h, w = SIZES[int(rng.integers(0, len(SIZES)))]
        yield h, w, po.random_polygon(rng, h, w, int(rng.integers(0, 3)))


def parity_counts(points, h, w):
    """The shortcut of the kernels: the run boundaries are the positions below h*w that occur an odd number of times."""
    pos, mult = np.unique(np.asarray(points, np.int64), return_counts=True)
    t = pos[(mult & 1).astype(bool) & (pos < h * w)]
    return np.diff(np.concatenate([[0], t, [h * w]]))


def test_fact_a_parity():
    """Step 4 (sort, differences, skip a zero difference with the one after it) == the parity rule; the counts add up to h*w and only the
    first may be 0."""
    zero_first = 0
    for h, w, poly in _random_cases(11, 1500):
        a = po.polygon_points(poly, h, w)
        c = po.points_to_counts(a, h, w)
        assert c.tolist() == parity_counts(a, h, w).tolist(), (h, w, poly)
        assert int(c.sum()) == h * w and (c[1:] > 0).all() and c[0] >= 0
        zero_first += int(c[0] == 0)
    assert zero_first > 0                                                  # the case exists in the sample


def test_fact_b_edge_independence():
    """The points of the ring walked as one list == the points of every edge walked alone, as multisets."""
    for h, w, poly in _random_cases(12, 1500):
        one = np.sort(po.polygon_points(poly, h, w))
        alone = np.sort(po.polygon_points_per_edge(poly, h, w))
        assert np.array_equal(one, alone), (h, w, poly)


def coverage_counts(parts, h, w):
    """The kernels' union: every part's r-th boundary is a +1 (even r) or -1 (odd r) event; a boundary of the union is a position where
    "coverage > 0" differs before and after all events of that position."""
    ev = []
    for poly in parts:
        t = np.cumsum(parity_counts(po.polygon_points_per_edge(poly, h, w), h, w))[:-1]
        ev += [(int(p), -1 if r & 1 else 1) for r, p in enumerate(t)]
    ev.sort()
    out, cov, prev, j = [], 0, 0, 0
    while j < len(ev):
        p, before = ev[j][0], cov > 0
        while j < len(ev) and ev[j][0] == p:
            cov += ev[j][1]
            j += 1
        if (cov > 0) != before:
            out.append(p - prev)
            prev = p
    return out + [h * w - prev]


def test_union_by_coverage_events():
    rng = np.random.default_rng(13)
    for _ in range(400):
        h, w = SIZES[int(rng.integers(0, len(SIZES)))]
        parts = po.random_annotation(rng, h, w)
        if rng.integers(0, 4) == 0:
            parts.append(parts[0])                                         # a duplicated part
        assert coverage_counts(parts, h, w) == po.annotation_counts(parts, h, w).tolist(), (h, w, parts)
