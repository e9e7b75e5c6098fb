"""The literal form of the error breakdown (tests/tide_oracle.py) pinned on the CPU: hand-checked cases for every kind, every branch of the
order of tests and every claim conflict, and - on the generator's cases - each fix against a literally edited result file run through
tests/cocoeval_oracle.py, compared with ==."""
import numpy as np
import pytest

from object_detectors_amd import tide                             # the module under test must exist: nothing here passes without it
from tests import cocoeval_oracle as co
from tests import tide_cases, tide_oracle

HAND = tide_cases.hand_cases()
SEEDS = (11, 12, 13, 14)
SMALL = dict(num_images=14, num_cats=6)


def test_names_agree_with_the_module():
    assert tide.KINDS == tide_oracle.KINDS and tide.FIXES == tide_oracle.FIXES


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    case = HAND[name]
    an = tide_oracle.analyse(case["dataset"], case["results"])
    slot = {id(r): d for d, r in enumerate(an["dt_items"])}
    names = (None,) + tide_oracle.KINDS[:5]
    for j, r in enumerate(case["results"]):
        d = slot[id(r)]
        assert names[an["kind"][d]] == case["kinds"][j], (name, j)
        got = None if an["partner"][d] < 0 else an["gt_items"][int(an["partner"][d])]["id"]
        assert got == case["partners"][j], (name, j)
    assert sorted(a["id"] for a, m in zip(an["gt_items"], an["missed"]) if m) == case["missed"]
    assert an["counts"][:5].sum() == an["counts"][6] == sum(k is not None for k in case["kinds"])
    assert an["counts"][5] == len(case["missed"])
    levels = case["levels"]
    base = tide_cases.expected_ap(levels["base"])
    assert an["ap_base"] == base
    for j, fix in enumerate(tide_oracle.FIXES):
        want = tide_cases.expected_ap(levels.get(fix, levels["base"]))
        assert an["ap_fixed"][j] == want, (name, fix, an["ap_fixed"][j], want)
        if want == -1 or base == -1:
            assert np.isnan(an["dap"][j])
        else:
            assert an["dap"][j] == want - base
    for key in ("loc_winner", "cls_winner"):                      # the one result that claims the partner; every other one is dropped
        if key in case:
            match = an["fix_dt_match"][1] if key == "loc_winner" else an["cls_match"]
            ignore = an["fix_dt_ignore"][1] if key == "loc_winner" else an["cls_ignore"]
            for j, r in enumerate(case["results"]):
                assert (match[slot[id(r)]], ignore[slot[id(r)]]) == ((1, 0) if j == case[key] else (0, 1)), (name, j)


def test_hand_prices_by_value():
    """A few of the prices above as plain numbers, so that a slip in expected_ap itself would show."""
    an = tide_oracle.analyse(HAND["bkg"]["dataset"], HAND["bkg"]["results"])
    assert an["ap_base"] == 0.5 and abs(an["dap"][tide_oracle.FIXES.index("Bkg")] - 0.5) < 1e-15
    an = tide_oracle.analyse(HAND["dupe"]["dataset"], HAND["dupe"]["results"])
    assert abs(an["ap_base"] - (51 + 50 * 2 / 3) / 101) < 1e-15 and an["ap_fixed"][tide_oracle.FIXES.index("Dupe")] == 1.0
    an = tide_oracle.analyse(HAND["cls"]["dataset"], HAND["cls"]["results"])
    assert an["ap_base"] == 0.25 and abs(an["dap"][0] - 0.75) < 1e-15


def test_a_lost_claim_still_explains_the_ground_truth():
    an = tide_oracle.analyse(HAND["loc_conflict"]["dataset"], HAND["loc_conflict"]["results"])
    assert an["missed"].sum() == 0 and an["fix_dt_ignore"][1].sum() == 1 and an["counts"][1] == 2


def test_crowds_are_invisible():
    """The crowd case with the crowd flag cleared is a different answer: the flag, not the geometry, hides the ground truth."""
    case = HAND["crowd"]
    plain = dict(case["dataset"], annotations=[dict(a, iscrowd=0) for a in case["dataset"]["annotations"]])
    an = tide_oracle.analyse(plain, case["results"])
    slot = {id(r): d for d, r in enumerate(an["dt_items"])}
    assert an["kind"][slot[id(case["results"][0])]] == tide_oracle.CLS


@pytest.fixture(scope="module")
def generated():
    out = []
    for seed in SEEDS:
        dataset, results = tide_cases.generate(seed, **SMALL)
        out.append((dataset, results, tide_oracle.analyse(dataset, results)))
    return out


def test_generator_conditions(generated):
    """No two identical ground-truth boxes in an image, at most 100 detections per (image, category) with the moved ones, and every kind at
    least five times over the seeds used."""
    counts = np.zeros(7, np.int64)
    for dataset, results, an in generated:
        boxes = [(a["image_id"], tuple(a["bbox"])) for a in dataset["annotations"]]
        assert len(set(boxes)) == len(boxes)
        per_image = {}
        for r in results:
            per_image[r["image_id"]] = per_image.get(r["image_id"], 0) + 1
        assert max(per_image.values()) <= 100
        counts += an["counts"]
        assert an["counts"][:5].sum() == an["counts"][6]
    print(dict(zip(tide_oracle.KINDS + ("FP",), counts.tolist())))
    assert (counts[:6] >= 5).all(), counts


@pytest.mark.parametrize("fix", ("base",) + tide_oracle.FIXES)
def test_literal_edits(generated, fix):
    """AP50 of the fix == stats[1] of the literally edited files, on every generated case."""
    for dataset, results, an in generated:
        new_dataset, new_results = tide_oracle.literal_edit(dataset, results, an, fix)
        want = co.stats(new_dataset, new_results)[1]
        got = an["ap_base"] if fix == "base" else an["ap_fixed"][tide_oracle.FIXES.index(fix)]
        print(fix, got, want)
        assert got == want
        if fix not in ("base",):
            changed = len(new_results) != len(results) or len(new_dataset["annotations"]) != len(dataset["annotations"]) or \
                any(a is not b for a, b in zip(results, new_results))
            assert changed                                        # the edit is not empty: the kind occurs in this case
