"""Mirror of yolo/procedures/eval_results.py: the COCO mAP of a list of result dicts (test_one_epoch.to_coco_results), which selects the
checkpoints (:52-57).  Scored by the device evaluator (object_detectors_amd/cocoeval.py); neither pycocotools nor a results file is needed
for that, so eval_results writes none.  save_partial_results / eval_partial_results keep the reference's file protocol: every rank pickles
its rows to bbox_results/temp_res/<rank>.json, one process chains them, writes bbox_results/<dset>/results_<epoch>.json and scores it."""
import itertools
import json
import os
import pickle

from ...cocoeval import COCOEval

TEMP_DIR = "bbox_results/temp_res"


def _validation_path(validation_path):
    cwd = os.getenv("owd")                                  # the launch directory the reference's hydra config exports
    return os.path.join(cwd, validation_path) if cwd else validation_path


def _coco_map(results, dset_name, validation_path):
    if dset_name in ("coco", "drones"):
        if not results:
            print("empty list return zero map")
            return 0
        ev = COCOEval(validation_path, "bbox")
        ev.add_results(results)
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
        return ev.stats[0]
    if dset_name == "lvis":
        raise NotImplementedError("eval_results: LVIS evaluation (300 detections per image over all categories, negative and non-exhaustive "
                                  "category lists) is not implemented")
    raise ValueError(f"eval_results: unknown dataset {dset_name!r}")


def save_partial_results(results, rank):
    os.makedirs(TEMP_DIR, exist_ok=True)
    with open(os.path.join(TEMP_DIR, "{}.json".format(rank)), "wb") as f:
        pickle.dump(results, f)


def eval_partial_results(epoch, dset_name, validation_path):
    results = []
    for filename in os.listdir(TEMP_DIR):
        if filename.endswith(".json"):
            with open(os.path.join(TEMP_DIR, filename), "rb") as f:
                results = list(itertools.chain(results, pickle.load(f)))
    os.makedirs(f"bbox_results/{dset_name}/", exist_ok=True)
    with open(f"./bbox_results/{dset_name}/results_{epoch}.json", "w") as f:
        json.dump(results, f, indent=4)
    return _coco_map(results, dset_name, _validation_path(validation_path))


def eval_results(results, dset_name, validation_path):
    return _coco_map(results, dset_name, _validation_path(validation_path))
