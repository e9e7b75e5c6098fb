"""Inputs for the weighted boxes fusion tests (tests/test_oracle_wbf.py, tests/test_gpu_wbf.py): hand cases with written expectations, the
lane / chunk / LDS boundary case and seeded random sets.  A case is a dict: "name", "images" (ids), "models" (one COCO result list per
model), "kw" (weights, iou_thr, skip_box_thr, conf_type) and "expect" (what the hand case states, see check_expectation)."""
import numpy as np

RANDOM_SEEDS = (29, 31)
RANDOM_WEIGHTS = ((1.0, 1.0, 1.0), (2.0, 1.0, 0.5))


def det(image, category, score, corners):
    x1, y1, x2, y2 = corners
    return {"image_id": image, "category_id": category, "score": score, "bbox": [x1, y1, x2 - x1, y2 - y1]}


def case(name, models, expect, images=(1, 2), **kw):
    return {"name": name, "images": list(images), "models": models, "kw": kw, "expect": expect}


def hand_cases():
    A, B, C = [0, 0, 10, 10], [2, 0, 12, 10], [3.5, 0, 13.5, 10]
    H1, H2 = [0, 0, 3, 1], [1, 0, 4, 1]
    T1, T2, T3 = [0, 0, 4, 4], [6, 0, 10, 4], [3, 0, 7, 4]
    out = [
        # the third box overlaps the first alone at 0.4815; it joins because the fused box has moved
        case("drift", [[det(1, 1, .9, A), det(1, 1, .8, B), det(1, 1, .7, C)]],
             {"clusters": 1, "corners": [[1.6875, 0, 11.6875, 10]], "members": [3]}, iou_thr=.55),
        case("drift_reordered", [[det(1, 1, .9, A), det(1, 1, .7, B), det(1, 1, .8, C)]], {"clusters": 2, "members": [1, 2]}, iou_thr=.55),
        case("exact_half", [[det(1, 1, .9, H1), det(1, 1, .8, H2)]], {"clusters": 2}, iou_thr=.5),
        case("exact_half_lower_threshold", [[det(1, 1, .9, H1), det(1, 1, .8, H2)]], {"clusters": 1}, iou_thr=.4999),
        # the third box overlaps both clusters at exactly 1/7: the first made wins
        case("tie", [[det(1, 1, .9, T1), det(1, 1, .8, T2), det(1, 1, .5, T3)]], {"clusters": 2, "same_cluster": [(0, 2)], "members": [1, 2]},
             iou_thr=.1),
        # avg, two models of weight 1: a lone box (image 1) is halved, a pair (image 2) is not
        case("avg_equal_weights", [[det(1, 1, .8, A), det(2, 1, .8, A)], [det(2, 1, .6, A)]], {"clusters": 2, "scores": [.4, .7], "members": [1, 2]},
             weights=(1, 1)),
        # weights (2, 1): lone .6 -> 1.2 / 3; pair .6, .9 -> ((1.2 + .9) / 2) * 2 / 3
        case("avg_weights_2_1", [[det(1, 1, .6, A), det(2, 1, .6, A)], [det(2, 1, .9, A)]], {"clusters": 2, "scores": [.4, .7], "members": [1, 2]},
             weights=(2, 1)),
        case("max_weights_2_1", [[det(1, 1, .6, A), det(2, 1, .6, A)], [det(2, 1, .9, A)]], {"clusters": 2, "scores": [.6, .6], "members": [1, 2]},
             weights=(2, 1), conf_type="max"),
        # strict <: the score at the threshold stays
        case("skip_box_thr", [[det(1, 1, .2, A), det(1, 1, .3, T2), det(2, 1, .5, A)]],
             {"clusters": 2, "dropped": {"below_skip_box_thr": 1}, "cluster_of": [-1, 0, 1]}, skip_box_thr=.3),
        # the same box from both models with equal scores fuses (image 1); with equal scores model 0's box comes first, so its cluster is
        # the first made and wins the tie of the box between them (image 2)
        case("equal_scores_two_models", [[det(1, 1, .9, A), det(2, 1, .9, T1), det(2, 1, .5, T3)], [det(1, 1, .9, A), det(2, 1, .9, T2)]],
             {"clusters": 3, "same_cluster": [(0, 3), (1, 2)], "members": [2, 2, 1], "corners": [A, None, T2]}, weights=(1, 1), iou_thr=.1),
        case("categories_never_mix", [[det(1, 1, .9, A)], [det(1, 2, .9, A)]], {"clusters": 2, "members": [1, 1]}, weights=(1, 1)),
    ]
    bad = {"score_not_positive": det(1, 1, 0.0, A), "box_not_finite": det(1, 1, .9, [0, float("nan"), 10, 10]),
           "box_empty": {"image_id": 1, "category_id": 1, "score": .9, "bbox": [0, 0, 0, 10]}, "unknown_image": det(99, 1, .9, A)}
    for reason, row in bad.items():
        out.append(case("drop_" + reason, [[row, det(1, 1, .7, B)]], {"clusters": 1, "dropped": {reason: 1}, "cluster_of": [-1, 0]}))
    return out


def check_expectation(c, got):
    """`got`: a fusion result with numpy arrays (the literal form's, or the device's copied to the host) against what the hand case states."""
    e = c["expect"]
    assert len(got["score"]) == e["clusters"], c["name"]
    if "members" in e:
        assert got["members"].tolist() == e["members"], c["name"]
    if "scores" in e:
        assert np.allclose(got["score"], e["scores"], rtol=0, atol=1e-12), (c["name"], got["score"])
    for row, corners in enumerate(e.get("corners", [])):
        if corners is not None:
            b = got["box"][row]
            assert np.allclose([b[0], b[1], b[0] + b[2], b[1] + b[3]], corners, rtol=0, atol=1e-12), (c["name"], b)
    for a, b in e.get("same_cluster", []):
        assert got["cluster_of"][a] == got["cluster_of"][b] >= 0, c["name"]
    if "cluster_of" in e:
        assert got["cluster_of"].tolist() == e["cluster_of"], c["name"]
    dropped = dict.fromkeys(got["dropped"], 0)
    dropped.update(e.get("dropped", {}))
    assert got["dropped"] == dropped, c["name"]


def boundary_case(lds_clusters):
    """One model, one group per image, disjoint boxes so that every candidate founds a cluster: 0, 1, 2, 63, 64, 65 and 130 clusters (images
    1..7); images 8 and 9: 130 clusters, and one cluster more than the kernel keeps in LDS, that each get a second member in reverse creation
    order.  In image 9 the last cluster, the one past LDS, then gets a third member that overlaps the founder's box at 7 / 13 < 0.55 and the
    re-divided box at about 0.58: it joins only if the arg-max reads the box that was stored after the join.
    -> (case, {image: clusters})."""
    sizes = {1: 0, 2: 1, 3: 2, 4: 63, 5: 64, 6: 65, 7: 130, 8: 130, 9: lds_clusters + 1}
    rows = []
    for image, n in sizes.items():
        spot = lambda k, dx=0.: [20. * (k % 16) + dx, 20. * (k // 16), 20. * (k % 16) + 10 + dx, 20. * (k // 16) + 10]
        rows += [det(image, 1, .99 - .5 * k / max(n, 1), spot(k)) for k in range(n)]
        if image in (8, 9):                                       # shifted by one: IoU 90 / 110 with the founder; the last cluster first
            rows += [det(image, 1, .2 + .001 * k, spot(k, 1.)) for k in range(n)]
        if image == 9:
            rows.append(det(image, 1, .1, spot(n - 1, 3.)))
    order = np.random.RandomState(5).permutation(len(rows))      # a results file is not sorted
    return case("boundary", [[rows[j] for j in order]], None, images=sorted(sizes)), sizes


def boundary_members(sizes, image):
    """The member counts boundary_case() must give on `image`, sorted."""
    n = sizes[image]
    return [1] * n if image < 8 else [2] * n if image == 8 else [2] * (n - 1) + [3]


def random_case(seed, weights=RANDOM_WEIGHTS[0], conf_type="avg", iou_thr=.55):
    """40 images, 6 categories, 3 models.  Each image has a few objects; a model reports an object with a jittered box, sometimes twice, and
    adds boxes of its own; the scores are multiples of 1/20, so exact ties are common (within and across models)."""
    rng = np.random.RandomState(seed)
    models = [[], [], []]
    for image in range(1, 41):
        for _obj in range(rng.randint(0, 7)):
            cat = int(rng.randint(1, 7))
            x, y = rng.uniform(0, 400, 2)
            w, h = np.exp(rng.uniform(np.log(16), np.log(200), 2))
            for m in range(3):
                for _rep in range(rng.choice([0, 1, 1, 1, 2, 3])):
                    j = rng.randn(4) * .04
                    box = [x + j[0] * w, y + j[1] * h, w * (1 + j[2]), h * (1 + j[3])]
                    models[m].append({"image_id": image, "category_id": cat, "score": int(rng.randint(1, 20)) / 20, "bbox": [float(v) for v in box]})
        for m in range(3):
            for _noise in range(rng.randint(0, 4)):
                box = np.concatenate([rng.uniform(0, 400, 2), np.exp(rng.uniform(np.log(16), np.log(200), 2))])
                models[m].append({"image_id": image, "category_id": int(rng.randint(1, 7)), "score": int(rng.randint(1, 20)) / 20,
                                  "bbox": [float(v) for v in box]})
    models = [[res[j] for j in rng.permutation(len(res))] for res in models]
    return case(f"random_{seed}_{conf_type}_{'_'.join(str(w) for w in weights)}", models, None, images=range(1, 41), weights=weights,
                conf_type=conf_type, iou_thr=iou_thr)


def random_cases():
    return [random_case(RANDOM_SEEDS[0]), random_case(RANDOM_SEEDS[1], RANDOM_WEIGHTS[1]), random_case(RANDOM_SEEDS[1], RANDOM_WEIGHTS[1], "max", .4)]
