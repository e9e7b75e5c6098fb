"""The coverage table (tests/conv_matrix.py) against the kernel sources and the committed tune records (CPU only).

A new tuner candidate, a new accepted epilogue or a record entry that selects an unchecked (configuration, epilogue) pair fails here until
tests/conv_matrix.py - and with it tests/test_gpu_conv_exact.py - covers it.
"""
import json
import os
import re
from collections import defaultdict

import pytest

from tests import conv_matrix as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "object_detectors_amd", "csrc")
RECORDS = os.path.join(ROOT, "object_detectors_amd", "tune_records")
EPI_NAMES = {"EPI_STATS": "STATS", "EPI_F32": "F32", "EPI_RES": "RES", "EPI_PLAIN": "PLAIN", "EPI_AFF": "AFF", "EPI_BNRED": "BNRED"}


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


ROW = re.compile(r"^\s*CFG_ROW\(\s*(\d+),\s*([eA-Z0-9 |]+?),\s*(REQ_[A-Z_0-9]+),\s*(\d+),\s*(\d+),\s*([01]),\s*([01]),", re.M)
MASKS = dict({"e" + n: (n,) for n in EPI_NAMES.values()}, eALL=tuple(EPI_NAMES.values()))


def cfg_rows():
    """conv_kernels.hip: the rows of the tile configuration table, in file order (= the order the tuner tries them)."""
    rows = [{"id": int(m[1]), "epis": tuple(sorted({n for e in m[2].split("|") for n in MASKS[e.strip()]})), "req": m[3], "a": int(m[4]),
             "b": int(m[5]), "tuned": m[6] == "1", "solo": m[7] == "1"} for m in ROW.finditer(src("conv_kernels.hip"))]
    assert len(rows) == src("conv_kernels.hip").count("CFG_ROW(") - 1 and len({r["id"] for r in rows}) == len(rows)      # (- 1: the #define)
    return rows


def igemm_candidates():
    """The ids the tuner tries: on wide outputs (in order), and the alternatives to the plain tile (id 0) on narrow ones."""
    tuned = [r for r in cfg_rows() if r["tuned"]]
    wide = tuple(r["id"] for r in tuned if not r["req"].startswith("REQ_NARROW"))
    return wide, tuple(sorted(r["id"] for r in tuned if r["req"] == "REQ_NARROW_DX"))


def run_cfg_epilogues():
    """id -> epilogues its table row accepts."""
    return {r["id"]: r["epis"] for r in cfg_rows()}


def covered():
    """(cfg, epilogue) -> set of has_tails values of the cases that run it."""
    cov = defaultdict(set)
    for c in MX.CASES:
        ep = MX.epilogue(c)
        if ep is not None:
            cov[(c.cfg, ep)].add(MX.has_tails(c))
    return cov


def test_table_lists_the_tuner_candidates():
    wide, narrow = igemm_candidates()
    assert wide == MX.WIDE_IDS, "conv_kernels.hip: the tuned rows of the configuration table changed: update tests/conv_matrix.py"
    assert narrow == MX.NARROW_IDS


def test_table_epilogue_sets_match_run_cfg():
    acc = run_cfg_epilogues()
    for cfg in (0,) + MX.WIDE_IDS + MX.NARROW_IDS:
        want = acc[cfg]
        assert tuple(sorted(MX.ACCEPTS[cfg])) == want, f"configuration {cfg}: its table row accepts {want}"


@pytest.mark.parametrize("cfg", (0,) + MX.WIDE_IDS + MX.NARROW_IDS)
def test_every_id_and_epilogue_has_a_clean_and_a_tail_case(cfg):
    cov = covered()
    for ep in MX.ACCEPTS[cfg]:
        got = cov.get((cfg, ep), set())
        assert True in got, f"configuration {cfg}, epilogue {ep}: no case with tails"
        assert False in got, f"configuration {cfg}, epilogue {ep}: no case on whole tiles"


def test_table_shape_requirements():
    cases = MX.CASES
    fwd = [c for c in cases if c.entry.startswith("fwd")]
    assert any(c.shape.cin == 32 for c in fwd) and any(c.shape.cout == 32 and c.entry.startswith("dgrad") for c in cases)
    for co in (32, 64, 72, 255, 324, 36, 819):
        assert any(c.shape.cout == co for c in fwd), co
    assert any(MX.gemm_cout_pad(c) // 128 > 8 for c in fwd), "a launch with more than 8 channel tiles (XCD-blocked tile order)"
    assert any(c.entry == "fwd_ex" and c.shape.s == 2 and c.cfg == 3 for c in cases)
    assert any(c.shape.k == 1 for c in fwd) and any(c.shape.k == 1 and c.entry == "dgrad" and c.shape.s == 2 for c in cases)
    assert any(c.shape.h == 13 and c.shape.s == 2 and MX.out_hw(c.shape) == (7, 7) for c in cases)
    assert any(c.shape.xpad and c.shape.ypad and c.shape.rpad and c.opts.get("res") for c in cases)
    for form in ("four", "cat", "single"):
        for res in (False, True):
            assert any(c.opts.get("s2") == form and bool(c.opts.get("res")) == res for c in cases), (form, res)
    for e in ("dgrad_ws", "dgrad_mask", "dgrad_bn", "fwd_ex_f32", "fwd_f32"):
        assert any(c.entry == e for c in cases), e
    assert any(c.entry == "dgrad_ws" and c.opts["res"] for c in cases)
    for relu in (0, 1, 2):
        assert any(c.entry == "fwd_ex" and c.opts.get("relu") == relu for c in cases), relu
    assert any(c.opts.get("image_stride") for c in cases)
    for sh in ((c.shape.n, c.shape.h, c.shape.w, c.shape.cin, c.shape.cout) for c in cases):
        assert sh[0] * sh[1] * sh[2] * max(sh[3], sh[4]) <= 2 * 40 * 40 * 1024, sh


def wgrad_candidates():
    m = re.search(r"constexpr int WG_SPLITS\[\] = \{([^}]*)\}", src("wgrad_choice.h"))
    form = int(re.search(r"constexpr int WG_FORM8 = 1 << (\d+);", src("wgrad_choice.h")).group(1))
    return tuple(int(v) for v in m.group(1).split(",")), 1 << form


def test_wgrad_table_covers_the_split_candidates_and_both_forms():
    cands, form8 = wgrad_candidates()
    assert cands == MX.WGRAD_SPLITS and form8 == MX.WGRAD_FORM8
    cases = [c for c in MX.CASES if c.entry == "wgrad"]
    for sh in MX.WGRAD_SHAPES:
        got = {c.opts["split"] for c in cases if c.shape == sh}
        assert got == set(MX.wgrad_values(sh)), sh
    routes = {MX.wgrad_route(c.opts["split"]) for c in cases}
    assert routes == {(f, r) for f in (False, True) for r in (0, 1, 2)}, routes
    assert {c.opts["dbias"] for c in cases} == {False, True}


# ---- committed tune records
def igemm_key_fields(key):
    """Low fields of conv_kernels.hip: igemm_key - exact whatever the wide fields above them carry.  EPI_BNRED (5) carries into the sox
    field (key * 5 + epi): a decoded (sox 1, STATS) is (sox 0, BNRED) - forward launches never have sox 1."""
    f16, key = key % 2, key // 2
    epi, key = key % 5, key // 5
    sox, key = key % 3, key // 3
    code, key = key % 7, key // 7
    t = key % 31
    if epi == 0 and sox >= 1:
        epi, sox = 5, sox - 1
    return {"f16": f16, "epi": epi, "sox": sox, "sin": code // 2, "so": code % 2 if code % 2 else 2, "T": t}


def effective_cfg(cfg, f):
    """The kernel a record entry really launches where the low fields decide (conv_kernels.hip: run_cfg falls back to 1)."""
    ep = [k for k, v in MX.EPI.items() if v == f["epi"]][0]
    if cfg in MX.DX_IDS and not (f["T"] == 9 and f["sin"] == 1 and f["so"] == 1 and f["sox"] == 0):
        return 1, ep
    if cfg in MX.ACCEPTS and ep not in MX.ACCEPTS[cfg]:
        return 1, ep
    return cfg, ep


def records():
    out = []
    for name in sorted(os.listdir(RECORDS)):
        if name.endswith(".json"):
            with open(os.path.join(RECORDS, name)) as f:
                out.append((name, json.load(f)["entries"]))
    return out


def test_records_exist():
    assert len(records()) >= 3


@pytest.mark.parametrize("name,entries", records(), ids=[r[0] for r in records()])
def test_every_record_choice_is_a_covered_case(name, entries):
    cov = covered()
    storages = set(MX.STORAGES)
    wg_routes = {MX.wgrad_route(c.opts["split"]) for c in MX.CASES if c.entry == "wgrad"}
    s2 = {c.opts.get("s2") for c in MX.CASES}
    for table, key, value in entries:
        if table == "igemm":
            f = igemm_key_fields(key)
            assert ("fp16" if f["f16"] else "bf16") in storages
            cfg, ep = effective_cfg(value, f)
            assert cfg in MX.ACCEPTS, f"{name}: configuration {value} is not in the table"
            assert (cfg, ep) in cov, f"{name}: ({value} -> {cfg}, {ep}) has no case"
            assert (value, ep) in cov or cfg != value, f"{name}: ({value}, {ep}) has no case"
        elif table == "wgrad":
            assert key % 2 in (0, 1)
            sp = value & (MX.WGRAD_FORM8 - 1)
            assert value & ~(MX.WGRAD_FORM8 | (MX.WGRAD_FORM8 - 1)) == 0 and sp >= 1, f"{name}: wgrad value {value}"
            assert MX.wgrad_route(value) in wg_routes, f"{name}: wgrad value {value}"
        else:
            assert table == "s2cat" and value in (0, 1)
            assert {0: "four", 1: "cat"}[value] in s2


def test_coverage_check_bites():
    """Removing an id from the table, or a record entry for a pair no case runs, must fail the checks above."""
    cov = covered()
    assert (44, "F32") not in cov and (40, "BNRED") not in cov          # excluded by their table rows: no case, and a record naming them...
    f = {"f16": 0, "epi": MX.EPI["F32"], "sox": 0, "sin": 1, "so": 1, "T": 9}
    assert effective_cfg(44, f) == (1, "F32")                            # ...runs configuration 1, which is covered
    stripped = defaultdict(set)
    for (cfg, ep), v in cov.items():
        if cfg != 27:
            stripped[(cfg, ep)] = v
    assert any(stripped.get((27, ep), set()) != {True, False} for ep in MX.ACCEPTS[27])
