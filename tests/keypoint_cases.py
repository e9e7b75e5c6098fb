"""The seeded keypoint data set of tests/test_gpu_keypoints.py, built here so that tests/test_keypoints_host.py can check on the CPU the
condition under which the device's match arrays must equal the host form's (oks_oracle.separation_violations).

Instances sit in clusters of one or two on a coarse grid (CELL px apart, an instance at most 300 px across), so that the similarity of a
detection to a ground truth of another cluster underflows to exactly 0.0: e = d^2 / vars / area / 2 > 745 for d > 2000, vars <= 0.16 and
area <= 20000.  A row of a similarity matrix then holds a few values of ordinary size and exact zeros.

6 images, 2 categories.  The groups, as (category id, image id):
    (3, 11)   66 ground truths (the lane loops wrap) and 26 detections (the cut to 20 applies)
    (3, 4)    ground truth, no detection              (8, 4)    detections, no ground truth
    (3, 7)    a crowd that two detections match (the re-match), beside an ordinary pair
    (3, 30)   a ground truth with num_keypoints == 0, not a crowd, that two detections lie on: only the first takes it, and its match is
              ignored; beside an ordinary pair
    (8, 2)    areas on both sides of 32^2 and 96^2 and exactly on them, ground truths and (unmatched, far off) detections
    (8, 19)   ordinary pairs; one annotation without the `num_keypoints` field
and detections on an image id (999) and with a category id (77) that the ground truth does not know."""
import numpy as np

IMG_IDS = [11, 4, 7, 30, 2, 19]
CAT_IDS = [3, 8]
CELL = 3000.0
SIGMAS_3 = [0.05, 0.1, 0.2]


class _Builder:
    def __init__(self, K, seed):
        self.K, self.rng = K, np.random.RandomState(seed)
        self.anns, self.results, self.cell = [], [], {}

    def _place(self, image_id, w, h, near=None):
        """The top-left corner of a new instance: the next grid cell of its image, or 40 px off the instance `near` (same cluster)."""
        if near is not None:
            return near["bbox"][0] + 40.0, near["bbox"][1] + 25.0
        n = self.cell.get(image_id, 0)
        self.cell[image_id] = n + 1
        return CELL * (n % 9) + 100.0, CELL * (n // 9) + 100.0

    def gt(self, image_id, category_id, w, h, area=None, crowd=0, visible=None, near=None, with_count=True):
        K, rng = self.K, self.rng
        x, y = self._place(image_id, w, h, near)
        v = rng.randint(0, 3, K) if visible is None else np.full(K, visible)
        if visible is None:
            v[rng.randint(K)] = 2                                   # one labelled keypoint at least
        kx, ky = x + rng.rand(K) * w, y + rng.rand(K) * h
        kp = np.stack([np.where(v > 0, kx, 0.0), np.where(v > 0, ky, 0.0), v.astype(np.float64)], 1)
        ann = {"id": len(self.anns) + 1, "image_id": image_id, "category_id": category_id, "bbox": [float(x), float(y), float(w), float(h)],
               "area": float(0.5 * w * h if area is None else area), "iscrowd": crowd, "keypoints": [float(t) for t in kp.reshape(-1)]}
        if with_count:
            ann["num_keypoints"] = int((v > 0).sum())
        self.anns.append(ann)
        return ann

    def dt(self, image_id, category_id, ann=None, jitter=0.05, keypoints=None):
        """A detection: `ann`'s keypoints moved by N(0, jitter * sqrt(area)) (unlabelled ones: anywhere in the box), or `keypoints`."""
        K, rng = self.K, self.rng
        if keypoints is None:
            g = np.asarray(ann["keypoints"], np.float64).reshape(K, 3)
            x, y, w, h = ann["bbox"]
            s = jitter * np.sqrt(ann["area"])
            kx = np.where(g[:, 2] > 0, g[:, 0] + rng.randn(K) * s, x + rng.rand(K) * w)
            ky = np.where(g[:, 2] > 0, g[:, 1] + rng.randn(K) * s, y + rng.rand(K) * h)
            keypoints = np.stack([kx, ky, np.ones(K)], 1)
        row = {"image_id": image_id, "category_id": category_id, "score": float(rng.rand()),
               "keypoints": [float(t) for t in np.asarray(keypoints, np.float64).reshape(-1)]}
        self.results.append(row)
        return row

    def spread(self, image_id, category_id, x, y, w, h):
        """A detection far from every ground truth whose keypoints span exactly [x, x + w] x [y, y + h]: area w * h, never matched."""
        K, rng = self.K, self.rng
        kx, ky = x + rng.rand(K) * w, y + rng.rand(K) * h
        kx[0], ky[0], kx[1], ky[1] = x, y, x + w, y + h
        return self.dt(image_id, category_id, keypoints=np.stack([kx, ky, np.ones(K)], 1))


def build(K=17, seed=5):
    """-> (dataset dict, result rows) of the module docstring for K keypoints per instance."""
    b = _Builder(K, seed)
    rng = b.rng
    # (3, 11): 66 ground truths, 26 detections
    big = [b.gt(11, 3, 60 + 200 * rng.rand(), 60 + 200 * rng.rand()) for _ in range(66)]
    for j in range(26):
        b.dt(11, 3, big[(5 * j) % 66], jitter=0.02 + 0.1 * rng.rand())
    # (3, 4): ground truth only; (8, 4): detections only
    b.gt(4, 3, 120, 150)
    b.gt(4, 3, 50, 70)
    for _ in range(3):
        b.spread(4, 8, 100 + 500 * rng.rand(), 100.0, 80.0, 90.0)
    # (3, 7): a crowd matched twice
    crowd = b.gt(7, 3, 200, 180, crowd=1)
    b.dt(7, 3, crowd, jitter=0.02)
    b.dt(7, 3, crowd, jitter=0.03)
    b.dt(7, 3, b.gt(7, 3, 90, 140), jitter=0.04)
    # (3, 30): num_keypoints == 0 without iscrowd, two detections inside its doubled box (similarity exactly 1.0 for both)
    blank = b.gt(30, 3, 100, 100, visible=0)
    x, y, w, h = blank["bbox"]
    for _ in range(2):
        b.spread(30, 3, x - 0.5 * w + 10 * rng.rand(), y - 0.5 * h + 10 * rng.rand(), 1.5 * w, 1.5 * h)
    b.dt(30, 3, b.gt(30, 3, 80, 120), jitter=0.05)
    # (8, 2): areas around the bounds
    for area in (1024.0, 1023.5, 9216.0, 9216.5, 500.0, 5000.0, 12000.0):
        a = b.gt(2, 8, 100, 140, area=area)
        b.dt(2, 8, a, jitter=0.04)
    second = b.gt(2, 8, 100, 140, area=4000.0, near=b.anns[-1])       # a row with two values of ordinary size
    b.dt(2, 8, second, jitter=0.06)
    for w, h in ((32.0, 32.0), (31.0, 33.0), (96.0, 96.0), (96.0, 96.5), (20.0, 20.0), (64.0, 64.0)):
        b.spread(2, 8, 500.0 + 10 * w, 1500.0, w, h)
    # (8, 19): ordinary pairs, one annotation without num_keypoints
    for j in range(4):
        a = b.gt(19, 8, 70 + 100 * rng.rand(), 90 + 100 * rng.rand(), with_count=j != 2)
        b.dt(19, 8, a, jitter=0.03 + 0.05 * j)
        if j == 1:
            b.dt(19, 8, a, jitter=0.2)
    # an image and a category the ground truth does not know
    b.dt(999, 3, big[0])
    b.dt(11, 77, big[1])
    dataset = {"images": [{"id": i} for i in IMG_IDS], "categories": [{"id": c} for c in CAT_IDS], "annotations": b.anns}
    order = rng.permutation(len(b.results))                             # images and categories interleaved, as a results file may be
    return dataset, [b.results[j] for j in order]


CASES = {"coco17": (17, None, 5), "custom3": (3, SIGMAS_3, 9)}       # name -> (K, sigmas (None: COCO's), seed)
