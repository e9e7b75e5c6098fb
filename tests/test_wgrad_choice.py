"""The host decisions of the weight gradient (csrc/wgrad_choice.h: geometry, the tuner's candidates and pick, the resolver) on the CPU.

tests/wgrad_choice_main.cpp includes only that header; it is compiled here with the host compiler and its output compared with
tests/golden/wgrad_choice.json, which was recorded from the host code that preceded the header (see the fixture's "about").  The Python
restatements in tests/conv_matrix.py and object_detectors_amd/tune.py are compared with the same program.
"""
import json
import os
import shutil
import subprocess

import pytest

from object_detectors_amd import tune
from tests import conv_matrix as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_choice.json")
EINVAL = -1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("wgrad_choice") / "wgrad_choice_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "wgrad_choice_main.cpp"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return [json.loads(l) for l in r.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def shape_line(sh):
    """The mi355det_conv_shape of a conv_matrix shape, as tests/test_gpu_conv_exact.py builds it."""
    ho, wo = MX.out_hw(sh)
    return " ".join(str(v) for v in (sh.n, sh.h, sh.w, sh.cin, ho, wo, sh.cout, sh.k, sh.s, (sh.k - 1) // 2, sh.cin + sh.xpad, sh.cout + sh.ypad))


def test_program_output_matches_the_recorded_decisions(program, golden):
    got = program(golden["input"])
    assert len(got) == len(golden["output"])
    for line, g, want in zip([l for l in golden["input"] if l[0] in "SR"], got, golden["output"]):
        assert g == want, line


def test_fixture_holds_the_shapes_and_settings(golden):
    shapes = [l[2:] for l in golden["input"] if l[0] == "S"]
    for sh in MX.WGRAD_SHAPES:
        assert shape_line(sh) in shapes, sh
    assert "8 100 100 256 100 100 10836 3 1 1 256 10840" in shapes                      # cls_logits of the 1204-class head
    assert "2 40 40 64 40 40 256 3 1 1 64 256" in shapes                                # the tuner-contract shape of tests/test_gpu_conv.py
    assert sum(s.startswith("32 ") for s in shapes) >= 20                               # Darknet-53, batch 32
    outs = [o for o in golden["output"] if isinstance(o, dict)]
    assert len(outs) == len(shapes) >= 7 + 11 + 20 + 2
    assert any(o["geom"][8] == 0 and o["geom"][0] * 128 * 2 > 2 ** 31 for o in outs)     # an input beyond the 31-bit offsets
    for o in outs:
        assert [w["bytes"] for w in o["ws"]] == [0, 1 << 20, o["geom"][6]] and all(len(w["grid"]) == 2 * 5 * 4 for w in o["ws"])
    kernels = [k for o in outs for w in o["ws"] for c, k in zip(w["cands"], w["kernels"]) if c & MX.WGRAD_FORM8]
    assert 128 in kernels and 256 in kernels              # the 256 x 256 candidate that is timed as the 128 x 128 kernel, and the usual one
    text = json.dumps(outs)
    for part in ("is not valid for", "workspace bytes (strict mode", "was forced (debug key 7)", "does not fit the 31-bit offsets"):
        assert part in text, part


def test_python_restatements_agree_with_the_header(program):
    outs = program(["S " + shape_line(sh) for sh in MX.WGRAD_SHAPES])
    singles, want = [], []
    for sh, o in zip(MX.WGRAD_SHAPES, outs):
        m = o["geom"][0]
        ho, wo = MX.out_hw(sh)
        assert m == sh.n * ho * wo
        assert bool(o["geom"][8]) == MX.wgrad8_applies(sh), sh
        for sp in MX.WGRAD_SPLITS:
            assert MX.split_valid(m, sp) == tune.wgrad_split_valid(m, sp) == (sp in o["valid"]), (sh, sp)
        # every value of the coverage table is launched as it is under strict mode (room for all its slabs)
        for v in MX.wgrad_values(sh):
            sp = v & (MX.WGRAD_FORM8 - 1)
            singles.append(f"R {shape_line(sh)} {o['geom'][6]} 1 -1 {v} 1")
            chunk = ((m + sp - 1) // sp + 63) // 64 * 64
            want.append(f"ok {sp} {chunk} k{256 if v & MX.WGRAD_FORM8 else 128} 1 f{MX.wgrad_route(v)[1]}")
    assert singles
    got = program(singles)
    for line, g, w in zip(singles, got, want):
        assert g.replace(" x ", " 1 ") == w, line


def test_strict_cases_of_the_exact_grid(program):
    """The two weight-gradient cases of test_gpu_conv_exact.py::test_strict_mode_rejects_what_would_fall_back, without a GPU."""
    cases = ((MX.shp(2, 13, 11, 64, 200, 3, 1), 4), (MX.shp(2, 40, 40, 64, 256, 3, 1), 10))
    got = program([f"R {shape_line(sh)} {1 << 20} 1 -1 {split} 1" for sh, split in cases])
    for (sh, split), g in zip(cases, got):
        status, msg = g.split(" ", 2)[1:]
        assert g.startswith("err ") and int(status) == EINVAL, g
        assert "strict" in msg and str(split) in msg, msg
