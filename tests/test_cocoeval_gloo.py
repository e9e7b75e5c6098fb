"""Multi-process (world_size 2, gloo, CPU) test of CocoEvaluator.synchronize_between_processes: the ranks' stored detections are merged, an
image seen on both ranks is kept once (its first occurrence).  State only: no kernel runs."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DATASET = {"images": [{"id": i} for i in (1, 2, 3, 4, 5)], "categories": [{"id": 1}],
           "annotations": [{"id": i, "image_id": i, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100, "iscrowd": 0} for i in (1, 2, 3, 4, 5)]}


def _prediction(image_id, rank):
    # the score says which rank the prediction came from
    return {"boxes": torch.tensor([[0., 0., 10., 10. + image_id]]), "scores": torch.tensor([0.5 + 0.25 * rank]), "labels": torch.tensor([1])}


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    ev = CocoEvaluator(DATASET, ["bbox"])
    mine = (1, 2, 3) if rank == 0 else (3, 4, 5)                 # image 3 is on both ranks
    ev.update({i: _prediction(i, rank) for i in mine[:2]})
    ev.update({i: _prediction(i, rank) for i in mine[2:]})
    ev.synchronize_between_processes()
    ids = list(ev.predictions)
    scores = {i: float(p["scores"][0]) for i, p in ev.predictions.items()}
    boxes_ok = all(float(p["boxes"][0, 3]) == 10. + i for i, p in ev.predictions.items())
    ok = (ids == [1, 2, 3, 4, 5] and scores == {1: 0.5, 2: 0.5, 3: 0.5, 4: 0.75, 5: 0.75} and boxes_ok
          and ev.img_ids == [1, 2, 3, 3, 4, 5])
    q.put((rank, ok, ids, scores))
    dist.barrier()
    dist.destroy_process_group()


def test_synchronize_merges_the_ranks_and_keeps_an_image_once():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _r, ok, _i, _s in res), res


def test_synchronize_without_a_process_group_is_a_no_op():
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    ev = CocoEvaluator(DATASET, ["bbox"])
    ev.update({1: _prediction(1, 0), 2: {}})
    ev.synchronize_between_processes()
    assert list(ev.predictions) == [1] and ev.img_ids == [1]
