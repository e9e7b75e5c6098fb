"""The string kernels (csrc/rle_string_kernels.hip: mi355det_rle_strings_count / _emit) against tests/rle_oracle.py and rle.counts_stats, and
the mask store's two routes against each other.  Integers only: every comparison is `==` on whole arrays."""
import numpy as np
import pytest
import torch

from tests import rle_oracle as ro

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _token_forms(string):
    """{(characters, negative)} of the tokens of a counts string."""
    out, k = set(), 0
    for ch in string:
        c = ord(ch) - 48
        k += 1
        if not c & 0x20:
            out.add((k, bool(c & 0x10)))
            k = 0
    return out


def _with_counts(rng, k, h):
    """k counts that fill whole columns of height h: runs of 1..9, the first maybe 0, the last stretched to the column end."""
    c = rng.integers(1, 10, k).astype(np.int64)
    if k > 1 and rng.random() < 0.5:
        c[0] = 0
    c[-1] += (-int(c.sum())) % h
    return c.tolist(), (h, int(c.sum()) // h)


def cases():
    """[(counts, (h, w))]: the masks of the one call, of different sizes, adjacent in one buffer."""
    rng = np.random.default_rng(7)
    out = [_with_counts(rng, k, h) for k, h in zip((1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 200), (3, 1, 7, 5, 2, 7, 11, 7, 3, 7, 13))]
    out.append(([5, 1000000000, 3, 7, 599999985], (40000, 40000)))           # tokens of 7 characters, one negative, one positive
    for L in range(1, 7):                                                        # the widest tokens of L characters, negative and positive
        top = 1 << (5 * L - 1)
        counts = [0, top + 3, 1, 3, top]                                         # tokens 3: -top, 4: top - 1
        out.append((counts, (1, sum(counts)) if L % 2 else (sum(counts), 1)))
    out.append(([12], (3, 4)))                                                   # all zeros
    out.append(([0, 12], (3, 4)))                                                # all ones
    out.append(([3, 0, 4, 2, 3], (3, 4)))                                        # a zero-length run of ones inside
    out.append(([2, 3, 7], (4, 3)))                                              # a run that crosses a column end
    out.append(([2, 2, 8], (4, 3)))                                              # a run that ends exactly on a column end
    out.append(([11, 1], (3, 4)))                                                # a single set pixel at the last position
    out.append(([0, 1], (1, 1)))
    return out


def blobs():
    """200 seeded blob masks of at most 24 x 32."""
    rng = np.random.default_rng(11)
    out = []
    for _ in range(200):
        h, w = int(rng.integers(1, 25)), int(rng.integers(1, 33))
        m = np.zeros((h, w), np.uint8)
        for _ in range(int(rng.integers(0, 4))):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            m[y:y + int(rng.integers(1, h + 1)), x:x + int(rng.integers(1, w + 1))] = 1
        m &= (rng.random((h, w)) > rng.choice([0.0, 0.1, 0.5])).astype(np.uint8)
        out.append(m)
    return out


@pytest.fixture(scope="module")
def one_call():
    """The strings, the sizes and what the rules say, computed once."""
    from object_detectors_amd.rle import counts_stats, counts_to_string
    strings, sizes = [], []
    for counts, size in cases():
        strings.append(ro.to_string(counts))
        sizes.append(size)
    for m in blobs():
        strings.append(counts_to_string(ro.encode(m)))                           # the host codec
        sizes.append(m.shape)
    counts = [ro.from_string(s) for s in strings]
    area, bbox = np.zeros(len(strings), np.int64), np.zeros((len(strings), 4), np.int32)
    for j, (c, (h, w)) in enumerate(zip(counts, sizes)):
        assert int(c.sum()) == h * w and (c >= 0).all()
        a, b = counts_stats(c, [0, len(c)], h)
        area[j], bbox[j] = a[0], b[0]
        assert area[j] == ro.area(c)
    return {"strings": strings, "sizes": np.asarray(sizes, np.int32), "counts": np.concatenate(counts).astype(np.int32),
            "runs": np.concatenate([[0], np.cumsum([len(c) for c in counts])]).astype(np.int64), "area": area, "bbox": bbox}


def _segs(want, which=None):
    which = range(len(want["strings"])) if which is None else which
    return [{"size": [int(v) for v in want["sizes"][j]], "counts": want["strings"][j]} for j in which]


def test_the_cases_hold_what_they_should(one_call):
    forms = set().union(*(_token_forms(s) for s in one_call["strings"]))
    assert forms >= {(k, neg) for k in range(1, 8) for neg in (False, True)}
    lens = np.diff(one_call["runs"])[:11].tolist()
    assert lens == [1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 200]
    assert max(len(s) for s in one_call["strings"]) > 3 * 57                     # more than three chunks of one wavefront
    for m, b in zip(blobs(), one_call["bbox"][-200:]):
        assert ro.bbox(m) == b.tolist()                                          # the boxes of the rules are the bitmaps' boxes


def test_one_call_against_the_rules(one_call):
    from object_detectors_amd import ops
    from object_detectors_amd.rle import pack_strings
    packed, offsets = pack_strings(one_call["strings"])
    for _ in range(2):                                                           # the same bits every run
        counts, runs, area, bbox, status = ops.rle_strings(packed, offsets, one_call["sizes"], DEV)
        assert status is None
        assert runs.dtype == np.int64 and np.array_equal(runs, one_call["runs"])
        assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), one_call["counts"])
        assert area.dtype == torch.int64 and np.array_equal(area.cpu().numpy(), one_call["area"])
        assert bbox.dtype == torch.int32 and np.array_equal(bbox.cpu().numpy(), one_call["bbox"])


def test_no_mask_and_empty_strings():
    from object_detectors_amd import ops
    counts, runs, area, bbox, status = ops.rle_strings(np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros((0, 2), np.int32), DEV)
    assert status is None and runs.tolist() == [0] and counts.numel() == 0 and area.numel() == 0 and tuple(bbox.shape) == (0, 4)
    counts, runs, area, bbox, status = ops.rle_strings(np.zeros(0, np.uint8), np.zeros(3, np.int64), np.asarray([[2, 2], [1, 3]], np.int32), DEV)
    assert status.tolist() == [ops.RLESTR_SUM, ops.RLESTR_SUM] and runs.tolist() == [0, 0, 0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2048, 2049, 8191, 8192, 8193, 16385])
def test_run_offsets_at_the_edges_of_the_scan(n):
    """The offsets scan (csrc/offsets_scan.h) at one item, a wave boundary, the step from the small block to the large one (256 x 8 items),
    a round of 1024 x 8 items and the carry into a third round: the smallest strings there are, a deterministic mix of six forms, and a refused one (its counts do not add up) at 0, 8191 and n - 1."""
    from object_detectors_amd import ops
    from object_detectors_amd.rle import pack_strings
    pool = [([4], (2, 2)), ([0, 4], (2, 2)), ([1, 1, 2], (2, 2)), ([3], (1, 3)), ([1, 2], (1, 3)), ([1, 1, 1], (1, 3)), ([1, 2], (2, 2))]
    refused = len(pool) - 1
    text = [ro.to_string(c) for c, _size in pool]
    assert all(1 <= len(s) <= 3 for s in text)
    decoded = [ro.from_string(s).astype(np.int32) for s in text]                 # the host oracle: a string owns one count per token
    p_area = np.asarray([ro.area(c) for c in decoded], np.int64)                 # of the refused form: never compared
    p_bbox = np.asarray([ro.bbox(ro.decode(c, h, w)) if j != refused else [0] * 4 for j, (c, (_c, (h, w))) in enumerate(zip(decoded, pool))],
                        np.int32)
    kind = (np.arange(n) + np.arange(n) // 5) % refused
    bad_at = np.asarray(sorted({j for j in (0, 8191, n - 1) if 0 <= j < n}), np.int64)
    kind[bad_at] = refused
    runs = np.concatenate([[0], np.cumsum(np.asarray([len(c) for c in decoded], np.int64)[kind])])
    assert n < 6 or len(set(np.diff(runs).tolist())) == 3
    packed, offsets = pack_strings([text[k] for k in kind])
    sizes = np.asarray([pool[k][1] for k in kind], np.int32).reshape(-1, 2)
    d_bytes, d_off, d_sz = torch.from_numpy(packed).to(DEV), torch.from_numpy(offsets).to(DEV), torch.from_numpy(sizes).to(DEV)
    table, status = ops.rle_strings_count(d_bytes, offsets, d_off, d_sz)
    host = table.cpu().numpy()
    assert np.array_equal(host[:n + 1], runs) and int(host[n + 1]) == len(bad_at)
    want = np.zeros(n, np.uint8)
    want[bad_at] = ops.RLESTR_SUM
    assert np.array_equal(status.cpu().numpy(), want)
    counts, area, bbox = ops.rle_strings_emit(d_bytes, d_off, d_sz, table, int(runs[-1]))
    assert np.array_equal(counts.cpu().numpy(), np.concatenate([decoded[k] for k in kind]) if n else np.zeros(0, np.int32))
    good = kind != refused                                                       # a refused mask's area and box are of no use
    assert np.array_equal(area.cpu().numpy()[good], p_area[kind][good])
    assert np.array_equal(bbox.cpu().numpy()[good], p_bbox[kind][good])


def test_status_bits(one_call):
    """Each malformed kind sets its bit on its mask only; the ranges the kernels are given are checked by them, not trusted."""
    from object_detectors_amd import ops
    from object_detectors_amd.rle import pack_strings
    good = ro.to_string([3, 2, 7])                                               # 3 x 4
    bad = [("1!", ops.RLESTR_ALPHABET), (good + "~", ops.RLESTR_ALPHABET), ("P" * 7 + "0", ops.RLESTR_LONG), (good + "P", ops.RLESTR_OPEN),
           (ro.to_string([0, 2 ** 31 - 1, 0]) + ro.to_string([1]), ops.RLESTR_INT32), (ro.to_string([2 ** 33]), ops.RLESTR_INT32),
           (ro.to_string([13, -1]), ops.RLESTR_NEGATIVE), (ro.to_string([3, 2, 6]), ops.RLESTR_SUM), ("", ops.RLESTR_SUM)]
    strings, sizes = [good], [(3, 4)]
    for s, _bit in bad:
        strings += [s, good]
        sizes += [(3, 4), (3, 4)]
    packed, offsets = pack_strings(strings)
    counts, runs, area, bbox, status = ops.rle_strings(packed, offsets, np.asarray(sizes, np.int32), DEV)
    assert status[0::2].tolist() == [0] * (len(bad) + 1)
    for j, (s, bit) in enumerate(bad):
        assert status[2 * j + 1] & bit, (s, status[2 * j + 1])
    host = counts.cpu().numpy()
    for j in range(0, len(strings), 2):                                          # the valid neighbours are untouched
        assert host[runs[j]:runs[j + 1]].tolist() == [3, 2, 7] and area[j].item() == 2 and bbox[j].tolist() == [1, 0, 1, 2]
    # device offsets that leave the buffer or descend: skipped with a status, nothing read, no count owned
    d_bytes = torch.from_numpy(pack_strings([good, good])[0]).to(DEV)
    host_off = np.asarray([0, 3, 6], np.int64)
    d_sz = torch.tensor([[3, 4], [3, 4]], dtype=torch.int32, device=DEV)
    for dev_off, want in (([0, 3, 1 << 40], [0, ops.RLESTR_RANGE]), ([-5, 3, 6], [ops.RLESTR_RANGE, 0]), ([4, 3, 6], [ops.RLESTR_RANGE, 0])):
        table, st = ops.rle_strings_count(d_bytes, host_off, torch.tensor(dev_off, dtype=torch.int64, device=DEV), d_sz)
        assert st.tolist() == want and table.tolist() == [0, 3 if want[0] == 0 else 0, 3, 1]
    table, st = ops.rle_strings_count(d_bytes, host_off, torch.tensor(host_off, device=DEV),
                                      torch.tensor([[0, 4], [1 << 16, 1 << 15]], dtype=torch.int32, device=DEV))
    assert st.tolist() == [ops.RLESTR_SIZE, ops.RLESTR_SIZE] and table.tolist() == [0, 0, 0, 2]


def _raised(fn):
    try:
        fn()
    except Exception as e:                                                       # noqa: BLE001 - the exception itself is compared
        return type(e), str(e)
    return None


MALFORMED = {"alphabet": "1!", "alphabet_high": "32~", "long": "P" * 7 + "0", "open": "327P",
             "int32": ro.to_string([0, 2 ** 31 - 1, 0]) + ro.to_string([1]), "int32_raw": ro.to_string([2 ** 33]),
             "negative": ro.to_string([13, -1]), "sum": "326", "empty": ""}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_input_raises_what_the_host_route_raises(one_call, kind):
    from object_detectors_amd.cocoeval import _MaskStore
    segs = _segs(one_call, [40, 5]) + [{"size": [3, 4], "counts": MALFORMED[kind]}] + _segs(one_call, [8, 30])
    want = _raised(lambda: _MaskStore("cpu").add_segmentations(segs))
    assert want is not None and want[0] is ValueError
    assert _raised(lambda: _MaskStore(DEV).add_segmentations(segs)) == want
    assert _raised(lambda: _MaskStore(DEV).add_segmentations([dict(s, counts=s["counts"].encode()) for s in segs])) == want
    if kind == "sum":                                                            # the host route decodes every string before it sums the first
        both = segs + [{"size": [3, 4], "counts": MALFORMED["open"]}]
        want = _raised(lambda: _MaskStore("cpu").add_segmentations(both))
        assert "rle_from_string" in want[1] and _raised(lambda: _MaskStore(DEV).add_segmentations(both)) == want
    store = _MaskStore(DEV)                                                      # a later valid call on the same process
    store.add_segmentations(_segs(one_call))
    counts, runs, area, bbox, sizes = store.tensors()
    assert np.array_equal(counts.cpu().numpy(), one_call["counts"]) and np.array_equal(runs.cpu().numpy(), one_call["runs"])
    assert np.array_equal(area.cpu().numpy(), one_call["area"].astype(np.float64)) and np.array_equal(sizes, one_call["sizes"])
    assert np.array_equal(bbox.cpu().numpy(), one_call["bbox"].astype(np.float64))


def test_the_store_takes_the_device_route_and_both_routes_agree(one_call, monkeypatch):
    from object_detectors_amd import ops
    from object_detectors_amd.cocoeval import _MaskStore
    calls = []
    real = ops.rle_strings
    monkeypatch.setattr(ops, "rle_strings", lambda *a, **k: calls.append(len(a[1]) - 1) or real(*a, **k))
    small = [j for j in range(len(one_call["strings"])) if int(one_call["sizes"][j].prod()) < (1 << 20)]     # the host route builds no bitmap either
    segs = _segs(one_call, small)
    dev, cpu = _MaskStore(DEV), _MaskStore("cpu")
    dev.add_segmentations(segs[:50])
    dev.add_segmentations(segs[50:])
    cpu.add_segmentations(segs)
    assert calls == [50, len(segs) - 50]
    for a, b in zip(dev.tensors(), cpu.tensors()):
        a, b = (x.cpu().numpy() if torch.is_tensor(x) else x for x in (a, b))
        assert a.dtype == b.dtype and np.array_equal(a, b)
    mixed = _MaskStore(DEV)                                                      # a count list among the strings: the host route, as before
    mixed.add_segmentations(segs[:3] + [{"size": [3, 4], "counts": [12]}])
    assert calls == [50, len(segs) - 50] and mixed.tensors()[1].tolist()[-2:] == [int(dev.tensors()[1][3]), int(dev.tensors()[1][3]) + 1]
