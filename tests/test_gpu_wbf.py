"""Weighted boxes fusion on the device (object_detectors_amd/ensemble.py, csrc/fusion_kernels.hip) against the literal host form
(tests/wbf_oracle.py).  Both sides do the same correctly rounded float64 operations in the same order, so score and box are compared as bit
patterns and everything else, the result order included, with ==."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import wbf_cases as wc
from tests import wbf_oracle as wo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = wc.hand_cases()
RANDOM = wc.random_cases()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _fusion(c):
    from object_detectors_amd.ensemble import WeightedBoxesFusion
    f = WeightedBoxesFusion(c["images"], device=DEV, **c["kw"])
    for m, rows in enumerate(c["models"]):
        f.add_results(m, rows)
    return f


def _host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _check(c, got=None, want=None):
    """The front end's result for the case against the literal form's: bits for score and box, == for the rest; -> (got, want)."""
    got = _host(_fusion(c).run()) if got is None else got
    want = wo.fuse(c["models"], c["images"], **c["kw"]) if want is None else want
    assert got["score"].dtype == got["box"].dtype == np.float64 and got["members"].dtype == np.int32
    assert got["score"].shape == want["score"].shape and got["box"].shape == want["box"].shape
    print(c["name"], ": clusters", len(want["score"]), "| differing bit patterns: score", int((_bits(got["score"]) != _bits(want["score"])).sum()),
          "box", int((_bits(got["box"]) != _bits(want["box"])).sum()))
    assert np.array_equal(got["image_id"], want["image_id"]) and np.array_equal(got["category_id"], want["category_id"])      # the order too
    assert np.array_equal(_bits(got["score"]), _bits(want["score"]))
    assert np.array_equal(_bits(got["box"]), _bits(want["box"]))
    assert np.array_equal(got["members"], want["members"])
    assert np.array_equal(got["cluster_of"], want["cluster_of"])
    assert got["dropped"] == want["dropped"]
    images = sorted(c["images"])
    assert np.array_equal(np.asarray(images, np.int64)[got["image_index"]], got["image_id"])
    return got, want


@pytest.mark.parametrize("c", HAND, ids=[c["name"] for c in HAND])
def test_hand_case(c):
    got, _want = _check(c)
    wc.check_expectation(c, got)


def test_lane_chunk_and_lds_boundaries():
    from object_detectors_amd import ops
    n = ops.wbf_lds_clusters()
    c, sizes = wc.boundary_case(n)
    assert sizes[9] == n + 1 and [sizes[i] for i in range(1, 9)] == [0, 1, 2, 63, 64, 65, 130, 130]
    got, _want = _check(c)
    for image, clusters in sizes.items():
        rows = got["image_id"] == image
        assert int(rows.sum()) == clusters and sorted(got["members"][rows].tolist()) == wc.boundary_members(sizes, image)


@pytest.fixture(scope="module")
def random_wants():
    return [wo.fuse(c["models"], c["images"], **c["kw"]) for c in RANDOM]


@pytest.mark.parametrize("k", range(len(RANDOM)), ids=[c["name"] for c in RANDOM])
def test_random_set(random_wants, k):
    c, want = RANDOM[k], random_wants[k]
    n = want["members"]
    assert (n > 1).mean() >= .30 and (n > 2).mean() >= .05           # the literal form alone says that the set is not degenerate
    f = _fusion(c)
    got, _want = _check(c, _host(f.run()), want)
    again = _host(f.run())                                          # without re-adding: the same bits
    for key in ("score", "box"):
        assert np.array_equal(_bits(again[key]), _bits(got[key]))
    for key in ("image_id", "category_id", "members", "cluster_of"):
        assert np.array_equal(again[key], got[key])
    assert again["dropped"] == got["dropped"]


def test_add_with_device_tensors_equals_add_results():
    """add() with device tensors of many images at once (float32 scores and boxes of values float32 holds) against add_results() with dicts."""
    from object_detectors_amd.ensemble import WeightedBoxesFusion
    c = RANDOM[1]
    models = [[dict(r, bbox=[float(np.float32(v)) for v in r["bbox"]], score=float(np.float32(r["score"]))) for r in rows] for rows in c["models"]]
    c32 = dict(c, models=models)
    want, _literal = _check(c32)                                     # through add_results
    f = WeightedBoxesFusion(c["images"], device=DEV, **c["kw"])
    for m, rows in enumerate(models):
        half = len(rows) // 2
        for part in (rows[:half], rows[half:]):
            f.add(m, torch.tensor([r["image_id"] for r in part], device=DEV), torch.tensor([r["category_id"] for r in part], device=DEV),
                  torch.tensor([r["score"] for r in part], dtype=torch.float32, device=DEV),
                  torch.tensor([r["bbox"] for r in part], dtype=torch.float32, device=DEV))
    got = _host(f.run())
    for key in ("score", "box"):
        assert np.array_equal(_bits(got[key]), _bits(want[key]))
    for key in ("image_id", "category_id", "members", "cluster_of"):
        assert np.array_equal(got[key], want[key])


def _ground_truth(c):
    """A COCO ground truth for a random set: model 0's detections above 0.5 as annotations."""
    anns = [{"id": j + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"], "area": r["bbox"][2] * r["bbox"][3],
             "iscrowd": 0} for j, r in enumerate(r for r in c["models"][0] if r["score"] > .5)]
    return {"images": [{"id": i} for i in c["images"]], "categories": [{"id": k} for k in range(1, 7)], "annotations": anns}


def test_feed_equals_add_results():
    from object_detectors_amd.cocoeval import COCOEval
    c = RANDOM[0]
    dataset = _ground_truth(c)
    f = _fusion(dict(c, models=c["models"][1:]))
    quiet = open(os.devnull, "w")
    fed = f.feed(COCOEval(dataset, "bbox", device=DEV)).evaluate().accumulate().summarize(file=quiet)
    ev = COCOEval(dataset, "bbox", device=DEV)
    rows = f.to_results()
    ev.add_results(rows)
    listed = ev.evaluate().accumulate().summarize(file=quiet)
    assert len(rows) == int(f.result["score"].shape[0]) > 100 and set(rows[0]) == {"image_id", "category_id", "score", "bbox"}
    assert np.array_equal(_bits(fed), _bits(listed)) and fed[0] > 0.05


def test_fuse_results_is_the_one_call_form():
    from object_detectors_amd.ensemble import fuse_results
    c = RANDOM[1]
    rows = fuse_results(c["models"], c["images"], device=DEV, **c["kw"])
    want = wo.fuse(c["models"], c["images"], **c["kw"])
    assert [r["image_id"] for r in rows] == want["image_id"].tolist() and [r["category_id"] for r in rows] == want["category_id"].tolist()
    assert np.array_equal(_bits([r["score"] for r in rows]), _bits(want["score"]))
    assert np.array_equal(_bits([r["bbox"] for r in rows]), _bits(want["box"]))


def test_op_skips_a_group_that_does_not_fit():
    """mi355det_wbf_fuse with offsets past num_boxes: the group is skipped, the others are fused."""
    from object_detectors_amd import ops
    boxes = torch.tensor([[0, 0, 10, 10], [1, 0, 11, 10], [50, 50, 60, 60]], dtype=torch.float64, device=DEV)
    scores = torch.tensor([.9, .8, .7], dtype=torch.float64, device=DEV)
    leader, fused, score, members, _sums = ops.wbf_fuse(torch.tensor([0, 2, 7, 3], device=DEV), boxes, scores)
    assert leader.cpu().tolist() == [0, 0, -1] and int(members[0]) == 2
    assert _bits(score[:1].cpu().numpy())[0] == _bits(np.asarray([(.9 + .8) / 2]))[0]
    want = (np.float64(.9) * np.asarray([0., 0, 10, 10]) + np.float64(.8) * np.asarray([1., 0, 11, 10])) / (np.float64(.9) + np.float64(.8))
    assert np.array_equal(_bits(fused[0].cpu().numpy()), _bits(want))


def _write(tmp_path, **objs):
    paths = {}
    for name, obj in objs.items():
        paths[name] = str(tmp_path / f"{name}.json")
        with open(paths[name], "w") as f:
            json.dump(obj, f)
    return paths


def test_fuse_models_tool(tmp_path):
    """tools/fuse_models.py in a child process on a tiny ground truth: the table and the fused file."""
    c = RANDOM[0]
    p = _write(tmp_path, gt=_ground_truth(c), a=c["models"][1], b=c["models"][2])
    out = str(tmp_path / "fused.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuse_models.py"), "--gt", p["gt"], "--results", p["a"], p["b"], "--weights", "2", "1",
                        "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    head = [j for j, l in enumerate(lines) if l.split() == ["a", "b", "fusion"]]
    assert len(head) == 1 and lines[0].startswith("== fusion of 2 result sets")
    table = lines[head[0] + 1:head[0] + 13]
    assert [l.split()[0] for l in table] == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]
    assert all(len(l.split()) == 4 for l in table)
    want = wo.fuse(c["models"][1:], c["images"], weights=(2, 1))
    with open(out) as f:
        rows = json.load(f)
    assert np.array_equal(_bits([r["score"] for r in rows]), _bits(want["score"])) and np.array_equal(_bits([r["bbox"] for r in rows]), _bits(want["box"]))


def test_compare_models_fuse_block(tmp_path, capsys):
    """tools/compare_models.py --fuse: the output without the flag, byte for byte, then the side-by-side block."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("compare_models", os.path.join(ROOT, "tools", "compare_models.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    c = RANDOM[0]
    p = _write(tmp_path, gt=_ground_truth(c), a=c["models"][1], b=c["models"][2])
    args = ["--gt", p["gt"], "--results", p["a"], p["b"]]
    tool.main(args)
    plain = capsys.readouterr().out
    tool.main(args + ["--fuse"])
    out = capsys.readouterr().out
    assert out.startswith(plain) and "fusion" not in plain
    block = out[len(plain):].splitlines()
    assert block[0].startswith("== fusion: weighted boxes fusion of ['a', 'b'], iou_thr 0.55, conf_type avg") and len(block) == 2 + 12
    assert block[1].split() == ["a", "b", "fusion"] and block[2].split()[0] == "AP"


def test_run_makes_one_host_read():
    """run() synchronises with the host once: the founder count with the dropped counts.  torch's sync debug mode warns at every
    synchronising call (a boolean-mask index or a nonzero would be one more)."""
    import warnings
    f = _fusion(RANDOM[1])
    f.run()                                                         # uploads and first-call work are not what is counted
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            f.run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # switching the mode on prints a notice of its own ("... is a prototype feature"); a synchronising call says "called a synchronizing ..."
    syncs = [str(w.message) for w in seen if "called a synchronizing" in str(w.message)]
    print("synchronising calls in run():", len(syncs), syncs)
    assert len(syncs) == 1


def _lvis_ground_truth(c):
    """_ground_truth as an LVIS ground truth: frequencies r / c / f, category 6 negative on the even images, category 5 not exhaustive on
    every third."""
    d = _ground_truth(c)
    for k, cat in enumerate(d["categories"]):
        cat["frequency"] = "rcf"[k % 3]
    for im in d["images"]:
        im["neg_category_ids"] = [6] if im["id"] % 2 == 0 else []
        im["not_exhaustive_category_ids"] = [5] if im["id"] % 3 == 0 else []
    return d


def test_feed_lvis_and_the_lvis_table(tmp_path, capsys):
    """feed(LVISEval) against add_results(to_results()) on the thirteen statistics, and tools/fuse_models.py --lvis (in this process)."""
    import importlib.util
    from object_detectors_amd.lviseval import RESULT_KEYS, LVISEval
    c = RANDOM[0]
    dataset = _lvis_ground_truth(c)
    f = _fusion(dict(c, models=c["models"][1:], kw=dict(weights=(2, 1))))
    fed = f.feed(LVISEval(dataset, device=DEV)).run().get_results()
    listed = LVISEval(dataset, f.to_results(), device=DEV).run().get_results()
    assert tuple(fed) == RESULT_KEYS and np.array_equal(_bits(list(fed.values())), _bits(list(listed.values()))) and fed["AP"] > 0.05
    spec = importlib.util.spec_from_file_location("fuse_models", os.path.join(ROOT, "tools", "fuse_models.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    p = _write(tmp_path, gt=dataset, a=c["models"][1], b=c["models"][2])
    tool.main(["--gt", p["gt"], "--results", p["a"], p["b"], "--weights", "2", "1", "--lvis"])
    lines = capsys.readouterr().out.splitlines()
    assert "(LVIS rules)" in lines[0]
    head = [j for j, l in enumerate(lines) if l.split() == ["a", "b", "fusion"]][0]
    table = [l.split() for l in lines[head + 1:head + 14]]
    assert [row[0] for row in table] == list(RESULT_KEYS) and len(lines) == head + 14
    assert [float(row[3]) for row in table] == [float(f"{v:.4f}") for v in fed.values()]
