"""numpy restatement of the COCO run-length encoding (pycocotools rleEncode / rleDecode / rleArea / rleToBbox / rleToString / rleFrString),
written from the definitions, for tests/test_rle_codec.py and tests/test_gpu_rle.py.

Run lengths: the pixels of an [H, W] mask in column-major order i = x*H + y, bit(-1) = 0; a transition is an i with bit(i) != bit(i-1); the
counts are the gaps between successive transitions, the first from 0, the last to H*W.  So the counts begin with a run of zeros (maybe 0), a
mask with T transitions has T + 1 of them, all-zero is [H*W], all-one is [0, H*W].

String: for count i, x = counts[i], from i = 3 on minus counts[i-2] (signed); then c = x & 0x1f, x >>= 5 (arithmetic),
more = (c & 0x10) ? x != -1 : x != 0, bit 0x20 of c = more, character c + 48, until more is false."""
import numpy as np


def encode(mask):
    """[H, W] of 0 / 1 (or bool) -> int64 counts."""
    m = np.asarray(mask).astype(bool)
    flat = m.T.reshape(-1)                                  # column-major
    prev = np.concatenate([[False], flat[:-1]])
    t = np.flatnonzero(flat != prev)
    edges = np.concatenate([[0], t, [flat.size]])
    return np.diff(edges).astype(np.int64)


def decode(counts, h, w):
    c = np.asarray(counts, np.int64)
    assert int(c.sum()) == h * w and (c >= 0).all()
    bits = np.repeat(np.arange(c.size) & 1, c).astype(np.uint8)
    return bits.reshape(w, h).T


def area(counts):
    return int(np.asarray(counts, np.int64)[1::2].sum())


def bbox(mask):
    """[xmin, ymin, xmax - xmin + 1, ymax - ymin + 1] of the set pixels, zeros when there are none."""
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def to_string(counts):
    out = []
    cnts = [int(v) for v in counts]
    for i, x in enumerate(cnts):
        if i > 2:
            x -= cnts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                         # Python's >> on a negative int is arithmetic
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def from_string(s):
    cnts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return np.asarray(cnts, np.int64)


def encode_batch(masks):
    """[D, H, W] -> (concatenated int64 counts, offsets list [D + 1], areas list, bboxes list)."""
    cs = [encode(m) for m in masks]
    offs = np.concatenate([[0], np.cumsum([c.size for c in cs])]).astype(np.int64)
    counts = np.concatenate(cs) if cs else np.zeros(0, np.int64)
    return counts, offs.tolist(), [area(c) for c in cs], [bbox(m) for m in masks]
