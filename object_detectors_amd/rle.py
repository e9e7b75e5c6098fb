"""COCO run-length encodings of instance masks: the batch the run-length kernels return (`ops.mask_rle_dense`, `ops.mask_rle_paste`) and the
`counts` string codec of the library (mi355det_rle_to_string / mi355det_rle_from_string = pycocotools rleToString / rleFrString).

A mask's counts are the lengths of its alternating runs of 0 and 1 over the pixels in column-major order, beginning with a run of zeros
(pycocotools rleEncode); `{"size": [H, W], "counts": str}` is what pycocotools `mask.encode(...)` + `counts.decode("utf-8")` hands to
`COCO.loadRes` (torchvision_models/detection/coco_eval.py:107-140)."""
import ctypes as C

import numpy as np
import torch

from ._lib import Mi355detError, lib


def _status(n, what):
    if n < 0:
        msg = lib().mi355det_last_error().decode()
        if n == -1:
            raise ValueError(f"mi355det {what}: {msg}")
        raise Mi355detError(f"mi355det {what} failed ({n}): {msg}")
    return n


def counts_to_string(counts, cap=None):
    """int32 run lengths of one mask -> the compressed ASCII string.  `cap` (bytes of the output buffer, the terminating NUL included) is
    7 characters per count + 1 unless given."""
    c = np.ascontiguousarray(counts, dtype=np.int32)
    n = int(c.shape[0])
    cap = 7 * n + 1 if cap is None else int(cap)
    buf = C.create_string_buffer(max(cap, 1))
    wrote = _status(lib().mi355det_rle_to_string(c.ctypes.data_as(C.c_void_p), n, buf, cap), "rle_to_string")
    return buf.raw[:wrote].decode("ascii")


def string_to_counts(s, cap=None):
    """The inverse: the compressed string -> int32 numpy run lengths.  `cap` (room for that many counts) is one per character unless given."""
    raw = s.encode("ascii") if isinstance(s, str) else bytes(s)
    cap = len(raw) if cap is None else int(cap)
    out = np.empty(max(cap, 1), np.int32)
    n = _status(lib().mi355det_rle_from_string(raw, out.ctypes.data_as(C.c_void_p), cap), "rle_from_string")
    return out[:n].copy()


def pack_strings(strings):
    """The `counts` strings of many masks (str or bytes) as the operands of `ops.rle_strings`: one uint8 array with all strings back to
    back and int64 offsets [n + 1].  A string ends at its first NUL, as it does for string_to_counts."""
    strings = list(strings)
    if all(isinstance(s, str) for s in strings):
        raw = "".join(strings).encode("ascii")             # ASCII: a string's length is its number of bytes
    else:
        strings = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in strings]
        raw = b"".join(strings)
    if b"\0" in raw:
        strings = [(s.encode("ascii") if isinstance(s, str) else s).split(b"\0", 1)[0] for s in strings]
        raw = b"".join(strings)
    offsets = np.zeros(len(strings) + 1, np.int64)
    np.cumsum(np.fromiter(map(len, strings), np.int64, len(strings)), out=offsets[1:])
    return np.frombuffer(bytearray(raw), np.uint8), offsets      # a writable copy: torch takes it without a warning


def counts_stats(counts, offsets, h):
    """Set pixels (int64 [D]) and tight boxes [xmin, ymin, xmax - xmin + 1, ymax - ymin + 1] (int32 [D, 4], zeros for an empty mask) of
    run lengths over columns of height h (one for all masks, or one per mask): concatenated int32 counts, mask d owning
    counts[offsets[d]:offsets[d + 1]]."""
    n = len(offsets) - 1
    area, bbox = np.zeros(n, np.int64), np.zeros((n, 4), np.int32)
    heights = np.broadcast_to(np.asarray(h, np.int64), (n,))
    for d in range(n):
        h = int(heights[d])
        c = np.asarray(counts[offsets[d]:offsets[d + 1]], np.int64)
        end = np.cumsum(c)
        first, last = (end - c)[1::2], end[1::2] - 1           # the runs of ones: first and last pixel index
        live = last >= first
        if not live.any():
            continue
        first, last = first[live], last[live]
        area[d] = int((last - first + 1).sum())
        x0, x1 = first // h, last // h
        whole = x1 > x0                                          # a run that goes on into the next column covers y = 0 and y = h - 1
        ymin = 0 if whole.any() else int((first % h).min())
        ymax = h - 1 if whole.any() else int((last % h).max())
        bbox[d] = (int(x0.min()), ymin, int(x1.max() - x0.min()) + 1, ymax - ymin + 1)
    return area, bbox


def boundary_dilation(h, w, ratio=0.02):
    """The erosion depth d of boundary IoU for an h x w image: int(round(ratio * sqrt(h^2 + w^2))) in float64, ties to even, at least 1
    (the boundary-IoU API's mask_to_boundary).  Host only."""
    ratio = float(ratio)
    if not ratio > 0 or not np.isfinite(ratio):
        raise ValueError(f"boundary_dilation: the dilation ratio must be positive, not {ratio}")
    d = int(round(ratio * np.sqrt(int(h) ** 2 + int(w) ** 2)))
    return 1 if d < 1 else d


def boundary_dilations(sizes, ratio=0.02):
    """boundary_dilation of every row of sizes [n, 2] = [h, w]: int32 numpy [n] (the same float64 expression, np.round = ties to even)."""
    boundary_dilation(1, 1, ratio)                         # the ratio's check
    s = np.asarray(sizes, np.int64).reshape(-1, 2)
    d = np.round(float(ratio) * np.sqrt((s[:, 0] ** 2 + s[:, 1] ** 2).astype(np.float64)))
    return np.maximum(d, 1).astype(np.int32)


class RLEBatch:
    """The run-length encodings of the D masks of one image.

    size      (H, W)
    counts    int32 tensor [offsets[D]]: the masks' counts one after the other (on the device when a kernel made them)
    offsets   host list [D + 1]: mask d owns counts[offsets[d]:offsets[d + 1]]
    area      int64 tensor [D]: set pixels (pycocotools `area`), or None
    bbox      int32 tensor [D, 4]: [x, y, w, h] of the set pixels, zeros for an empty mask (pycocotools `toBbox`), or None
    """

    def __init__(self, size, counts, offsets, area=None, bbox=None):
        self.size = (int(size[0]), int(size[1]))
        self.counts = counts
        self.offsets = [int(o) for o in offsets]
        self.area, self.bbox = area, bbox
        if not self.offsets or self.offsets[0] != 0 or self.offsets[-1] != int(counts.shape[0]) or \
                any(b <= a for a, b in zip(self.offsets, self.offsets[1:])):
            raise ValueError("RLEBatch: offsets must rise from 0 to len(counts), at least one count per mask")
        self._host = None

    def __len__(self):
        return len(self.offsets) - 1

    def counts_host(self):
        """The counts as one int32 numpy array (copied from the device once)."""
        if self._host is None:
            self._host = np.ascontiguousarray(self.counts.detach().cpu().numpy(), dtype=np.int32)
        return self._host

    def counts_of(self, d):
        return self.counts_host()[self.offsets[d]:self.offsets[d + 1]]

    def stats(self):
        """(area int64 [D], bbox int32 [D, 4]): what the kernels returned, or - for a batch built from counts alone, a ground truth read
        from json - pycocotools `area` / `toBbox` worked out from the counts on the host."""
        if self.area is None or self.bbox is None:
            area, bbox = counts_stats(self.counts_host(), self.offsets, self.size[0])
            self.area, self.bbox = torch.from_numpy(area).to(self.counts.device), torch.from_numpy(bbox).to(self.counts.device)
        return self.area, self.bbox

    def to_coco(self):
        """[{"size": [H, W], "counts": str}] - the `segmentation` field of a COCO result, one per mask."""
        h, w = self.size
        return [{"size": [h, w], "counts": counts_to_string(self.counts_of(d))} for d in range(len(self))]

    def boundary(self, dilation_ratio=0.02, budget_bytes=1 << 30):
        """The masks' boundaries `mask & ~eroded` as another RLEBatch, made on the device (ops.rle_boundary; the rule: boundary_dilation
        and include/mi355det.h, "Mask boundaries as run lengths").  Its area and bbox are the boundaries'."""
        from . import ops
        d = boundary_dilation(self.size[0], self.size[1], dilation_ratio)
        if not self.counts.is_cuda:
            raise ValueError("RLEBatch.boundary needs CUDA/HIP tensors (no CPU fallback)")
        _area, bbox = self.stats()
        counts, offsets, area, box = ops.rle_boundary(self.counts, np.asarray(self.offsets, np.int64), [self.size] * len(self), d, bbox,
                                                      budget_bytes=budget_bytes)
        return RLEBatch(self.size, counts, offsets, area, box)

    def decode(self):
        """The bitmaps back: uint8 [D, H, W] on the host."""
        h, w = self.size
        out = np.zeros((len(self), h, w), np.uint8)
        for d in range(len(self)):
            c = self.counts_of(d).astype(np.int64)
            if int(c.sum()) != h * w or (c < 0).any():
                raise ValueError(f"RLEBatch.decode: the counts of mask {d} do not add up to {h}x{w}")
            bits = np.repeat(np.arange(c.shape[0], dtype=np.int64) & 1, c).astype(np.uint8)
            out[d] = bits.reshape(w, h).T                  # column-major pixel order
        return torch.from_numpy(out)
