"""mi355det_rle_boundary_plan is host code: its checks and its scratch layout, called through ctypes without a GPU."""
import ctypes as C

import numpy as np
import pytest


def _plan(runs, geom, budget, index=None, num_counts=None):
    from object_detectors_amd import _lib
    L = _lib.lib()
    runs, geom = np.ascontiguousarray(runs, np.int64), np.ascontiguousarray(geom, np.int32).reshape(-1, 7)
    index = None if index is None else np.ascontiguousarray(index, np.int64)
    n = geom.shape[0] if index is None else index.shape[0]
    slices, starts, need = np.full(max(n, 1), -7, np.int64), np.full(n + 1, -7, np.int64), np.zeros(1, np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    c = L.mi355det_rle_boundary_plan(p(runs), len(runs) - 1, int(runs[-1]) if num_counts is None else num_counts, p(index), p(geom), n, budget,
                                     p(slices), p(starts), p(need))
    return int(c), slices[:n], starts, int(need[0]), L.mi355det_last_error().decode()


def _need(m, bw, bh):
    """Three planes of bw x ceil(bh / 64) words and the scanned counts, an even number of int32."""
    return 0 if bw == 0 or bh == 0 else 8 * 3 * bw * ((bh + 63) // 64) + 4 * ((m + 1) // 2 * 2)


# (counts of the mask, h, w, d, box)
MASKS = [(3, 30, 40, 1, (5, 5, 10, 10)), (1, 30, 40, 1, (0, 0, 0, 0)), (41, 70, 45, 2, (0, 0, 45, 70)), (7, 480, 640, 16, (100, 50, 300, 200)),
         (2, 30, 40, 1, (0, 0, 40, 30)), (5, 100, 150, 4, (149, 99, 1, 1))]


def _tables():
    runs = np.concatenate([[0], np.cumsum([m[0] for m in MASKS])])
    geom = [[h, w, d, *box] for _m, h, w, d, box in MASKS]
    need = [_need(m, box[2], box[3]) for m, _h, _w, _d, box in MASKS]
    return runs, geom, need


def test_one_chunk_lays_the_slices_end_to_end():
    runs, geom, need = _tables()
    c, slices, starts, ws, _msg = _plan(runs, geom, 1 << 30)
    assert c == 1 and starts[:2].tolist() == [0, len(MASKS)]
    assert slices.tolist() == np.concatenate([[0], np.cumsum(need)[:-1]]).tolist() and ws == sum(need)
    assert all(s % 8 == 0 for s in slices)


def test_chunks_stay_within_the_budget_and_hold_one_mask_at_least():
    runs, geom, need = _tables()
    for budget in (0, 1, 300, 2000, 30000, max(need), sum(need) - 1):
        c, slices, starts, ws, _msg = _plan(runs, geom, budget)
        starts = starts[:c + 1].tolist()
        assert starts[0] == 0 and starts[-1] == len(MASKS) and all(b > a for a, b in zip(starts, starts[1:]))
        for a, b in zip(starts, starts[1:]):
            assert slices[a] == 0 and slices[a:b].tolist() == np.concatenate([[0], np.cumsum(need[a:b])[:-1]]).tolist()
            if sum(v > 0 for v in need[a:b]) >= 2:                  # one mask that needs scratch may exceed the budget on its own
                assert sum(need[a:b]) <= budget
            if b < len(MASKS):                                       # and the next mask did not fit
                assert sum(need[a:b]) > 0 and sum(need[a:b]) + need[b] > budget
        assert ws == max(sum(need[a:b]) for a, b in zip(starts, starts[1:]))
    c, _s, starts, ws, _msg = _plan(runs, geom, 1)
    assert c >= 4 and ws == max(need)                                # every mask that needs scratch opens a chunk


def test_index_and_no_masks():
    runs, geom, need = _tables()
    c, slices, starts, ws, _msg = _plan(runs, [geom[3], geom[0]], 1 << 30, index=[3, 0])
    assert c == 1 and slices.tolist() == [0, need[3]] and ws == need[3] + need[0]
    c, _s, starts, ws, _msg = _plan(runs, np.zeros((0, 7)), 1 << 30)
    assert c == 0 and starts[0] == 0 and ws == 0


@pytest.mark.parametrize("change,word", [
    (dict(d=0), "dilation"), (dict(h=0), "h, w"), (dict(h=1 << 16, w=1 << 15), "h*w"), (dict(box=(5, 5, 36, 10)), "box"), (dict(box=(5, 21, 10, 10)), "box"),
    (dict(box=(-1, 5, 10, 10)), "box"), (dict(box=(5, 5, -1, 10)), "box"), (dict(index=[6]), "index"), (dict(index=[-1]), "index"),
    (dict(num_counts=2), "runs"), (dict(runs=[0, 3000]), "more counts than pixels"), (dict(runs=[3, 0]), "runs"), (dict(budget=-1), "bad arguments")])
def test_refusals_before_any_launch(change, word):
    g = dict(h=30, w=40, d=1, box=(5, 5, 10, 10))
    g.update({k: v for k, v in change.items() if k in g})
    c, _s, _st, _ws, msg = _plan(change.get("runs", [0, 3]), [[g["h"], g["w"], g["d"], *g["box"]]], change.get("budget", 1 << 20),
                                 index=change.get("index"), num_counts=change.get("num_counts"))
    assert c == -1 and word in msg, msg
