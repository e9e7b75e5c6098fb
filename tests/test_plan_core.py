"""plan_core on the CPU: the shared pieces of the two step executors driven with a stub library that only records names."""
import ctypes as C
import types

import pytest
import torch

from object_detectors_amd import _lib, plan_core
from object_detectors_amd.plan_core import Act, BackwardSchedule, GradAccumulator, PlanBase, cached_plan, check_images, comm_hook


class StubLib:
    """Every entry point is a function of that name returning 0."""

    def __getattr__(self, name):
        def fn(*a):
            return 0
        fn.__name__ = name
        setattr(self, name, fn)
        return fn


def make_plan():
    return PlanBase(None, StubLib(), 2, 64, 64, True, 0)


def act(c=8, needs_grad=True):
    return Act(torch.zeros((2, 4, 4, c), dtype=torch.bfloat16), 2, 4, 4, c, c, needs_grad=needs_grad)


def make_acc(plan):
    def dgrad_call(shp, dy_ptr, wd, g, rptr, rld):
        return (plan.L.mi355det_conv_dgrad, (shp, dy_ptr, wd, g, rptr, rld))
    return GradAccumulator(plan.L, "cpu", torch.bfloat16, plan, dgrad_call)


def pv(p):
    return None if p is None else p.value


def names(plan):
    return [fn.__name__ for fn, _a in plan.bwd]


def add_args(entry):
    fn, (p, pld, q, qld, c, pixels, out, old, _stream) = entry
    assert fn.__name__ == "mi355det_add_bf16"
    return pv(p), pld, pv(q), qld, c, pixels, pv(out), old


def test_comm_hook_is_one_object():
    from object_detectors_amd.yolo.nets import engine as yolo_engine
    from object_detectors_amd.tvision import engine as tv_engine
    assert yolo_engine.comm_hook is comm_hook and tv_engine.comm_hook is comm_hook
    assert yolo_engine.Act is Act and yolo_engine._vp is plan_core._vp
    for name in ("bn_name", "arch", "BLOCKS"):
        assert hasattr(yolo_engine, name)


def test_single_consumer_nothing_pending_gets_null_residual():
    plan = make_plan()
    acc, x = make_acc(plan), act()
    acc.add_dgrad(x, "shp", "dy", "wd")
    assert names(plan) == ["mi355det_conv_dgrad"]
    shp, dy, wd, g, rptr, rld = plan.bwd[0][1]
    assert (shp, dy, wd, rptr, rld) == ("shp", "dy", "wd", None, 0)
    assert g is x.grad and x.grad_written and (g.n, g.h, g.w, g.c, g.ld) == (2, 4, 4, 8, 8)
    assert any(b is g.buf for b in plan.grad_bufs)


def test_pending_tensor_is_the_residual_then_adds_then_in_place():
    plan = make_plan()
    acc, x = make_acc(plan), act()
    t1, t2, t3 = act(), act(), act()
    for t in (t1, t2, t3):
        acc.add_tensor(x, t)
    assert plan.bwd == [] and x.parts == [t1, t2, t3]
    acc.add_dgrad(x, "shp", "dy", "wd")
    g = x.grad
    assert names(plan) == ["mi355det_conv_dgrad", "mi355det_add_bf16", "mi355det_add_bf16"]
    assert pv(plan.bwd[0][1][4]) == pv(t1.ptr) and plan.bwd[0][1][5] == t1.ld
    for entry, t in zip(plan.bwd[1:], (t2, t3)):
        assert add_args(entry) == (pv(g.ptr), g.ld, pv(t.ptr), t.ld, x.c, x.pixels, pv(g.ptr), g.ld)
    assert x.parts == []
    # (c) a second consumer accumulates in place: residual == dx
    acc.add_dgrad(x, "shp2", "dy2", "wd2")
    fn, (shp, _dy, _wd, g2, rptr, rld) = plan.bwd[-1]
    assert fn.__name__ == "mi355det_conv_dgrad" and shp == "shp2" and g2 is g and pv(rptr) == pv(g.ptr) and rld == g.ld
    # a tensor arriving after the gradient was written is added at once
    t4 = act()
    acc.add_tensor(x, t4)
    assert add_args(plan.bwd[-1]) == (pv(g.ptr), g.ld, pv(t4.ptr), t4.ld, x.c, x.pixels, pv(g.ptr), g.ld) and x.parts == []
    assert len(plan.grad_bufs) == 1 and plan.grad_bufs[0] is g.buf


def test_own_call_form_and_no_gradient_needed():
    plan = make_plan()
    acc = make_acc(plan)
    frozen = act(needs_grad=False)
    acc.add_tensor(frozen, act())
    acc.add_dgrad(frozen, "shp", "dy", "wd")
    assert plan.bwd == [] and frozen.grad is None and frozen.parts == [] and plan.grad_bufs == []
    x, t = act(), act()
    acc.add_tensor(x, t)
    acc.add_dgrad(x, "shp", "dy", "wd", lambda shp, dy, wd, g, rptr, rld: (plan.L.mi355det_conv_dgrad_mask, (g, rptr, rld)))
    assert names(plan) == ["mi355det_conv_dgrad_mask"]
    assert plan.bwd[0][1][0] is x.grad and pv(plan.bwd[0][1][1]) == pv(t.ptr) and x.grad_written


def test_finalize_aliases_one_part_and_sums_more():
    plan = make_plan()
    acc = make_acc(plan)
    a, t = act(), act()
    assert acc.finalize(a) is None and not a.grad_written
    acc.add_tensor(a, t)
    assert acc.finalize(a) is t and a.grad is t and a.grad_written           # alias: no copy, no buffer
    assert plan.bwd == [] and plan.grad_bufs == []
    assert acc.finalize(a) is t
    b, p0, p1, p2 = act(), act(), act(), act()
    for t in (p0, p1, p2):
        acc.add_tensor(b, t)
    g = acc.finalize(b)
    assert g is b.grad and b.grad_written and b.parts == []
    assert len(plan.grad_bufs) == 1 and plan.grad_bufs[0] is g.buf
    assert g.buf.data_ptr() not in [t.buf.data_ptr() for t in (p0, p1, p2)]
    assert [add_args(e) for e in plan.bwd] == [
        (pv(p0.ptr), p0.ld, pv(p1.ptr), p1.ld, b.c, b.pixels, pv(g.ptr), g.ld),
        (pv(g.ptr), g.ld, pv(p2.ptr), p2.ld, b.c, b.pixels, pv(g.ptr), g.ld)]


class StubStream:
    def __init__(self, handle):
        self.cuda_stream = handle

    def wait_event(self, ev):
        pass


class StubEvent:
    def record(self, stream):
        pass


def make_schedule(plan):
    main, side = StubStream(0), StubStream(7)
    return BackwardSchedule(plan, "cpu", torch.bfloat16, 16, 0, streams=(main, side), new_event=StubEvent), main, side


def hook(entry):
    fn, args = entry
    assert fn is comm_hook
    return args


def test_schedule_waits_before_overwriting_a_dz_buffer():
    plan = make_plan()
    sched, main, side = make_schedule(plan)
    assert plan.side is side and len(plan.dz2) == 2 and plan.dz2[0].numel() == 16 and plan.wgrad_ws.numel() >= 16
    shp = _lib.ConvShape()
    taken, done = [], []          # dz index of every acquisition, the event its weight gradient recorded
    for k in range(5):
        before = len(plan.bwd)
        di = sched.next_dz()
        emitted = plan.bwd[before:]
        if k < 2:
            assert emitted == []                                   # nothing has read this buffer yet
        else:
            assert len(emitted) == 1
            fn, ev = hook(emitted[0])
            assert fn == main.wait_event and ev is done[k - 2] and taken[k - 2] == di
        taken.append(di)
        before = len(plan.bwd)
        sched.wgrad(shp, None, None, None, None, dz_index=di)
        pub0, pub1, wg, rec = plan.bwd[before:]
        ev = hook(pub0)[0].__self__
        assert hook(pub0) == (ev.record, main) and hook(pub1) == (side.wait_event, ev)
        assert wg[0].__name__ == "mi355det_conv_wgrad" and wg[1][-1].value == 7 and wg[1][-2] == plan.wgrad_ws.numel()
        assert hook(rec)[1] is side
        done.append(hook(rec)[0].__self__)
    assert taken == [0, 1, 0, 1, 0] and len(set(map(id, done))) == 5


def test_schedule_untied_weight_gradient_publish_and_close():
    plan = make_plan()
    sched, main, side = make_schedule(plan)
    shp = _lib.ConvShape()
    sched.wgrad(shp, None, None, None, None)                       # dy is not a dz buffer: nothing to wait for later
    sched.wgrad(shp, None, None, None, None, record=False)
    assert sched.wg_done == [None, None]
    assert [e[0].__name__ for e in plan.bwd] == ["comm_hook", "comm_hook", "mi355det_conv_wgrad", "comm_hook",
                                                 "comm_hook", "comm_hook", "mi355det_conv_wgrad"]
    assert sched.next_dz() == 0 and sched.next_dz() == 1 and len(plan.bwd) == 7
    sched.close(plan)
    rec, join = hook(plan.bwd[-2]), hook(plan.bwd[-1])
    assert rec == (rec[0].__self__.record, side) and join == (main.wait_event, rec[0].__self__)
    assert plan.side_stream is side


def test_run_walks_the_list_in_order():
    plan = make_plan()
    seen = []
    plan.fwd = [(plan.L.mi355det_a, (1,)), (comm_hook, (seen.append, "hook")), (plan.L.mi355det_b, ())]
    plan._run(plan.fwd)
    assert seen == ["hook"]
    with pytest.raises(RuntimeError):
        comm_hook()


def test_plan_cache_is_an_lru(monkeypatch):
    monkeypatch.delenv("MI355DET_TUNE_LOAD", raising=False)
    monkeypatch.delenv("MI355DET_TUNE_SAVE", raising=False)
    syncs = []
    monkeypatch.setattr(plan_core.torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(synchronize=lambda: syncs.append(1)))
    installed = []
    eng = types.SimpleNamespace(plans={}, MAX_PLANS=2, grad_syncs=[types.SimpleNamespace(install=installed.append)])
    built = []

    def get(key, training=True):
        def build():
            built.append(key)
            return ("plan", key)
        return cached_plan(eng, key, build, training, False)
    a, b = get("a"), get("b", training=False)
    assert list(eng.plans) == ["a", "b"] and installed == [a] and syncs == []
    assert get("a") is a and built == ["a", "b"]                   # a hit builds nothing ...
    assert list(eng.plans) == ["b", "a"]                           # ... and moves the plan to most recent
    get("c")
    assert list(eng.plans) == ["a", "c"] and syncs == [1]          # the least recently used plan went, behind a synchronize
    assert get("b", training=False) is not b and list(eng.plans) == ["c", "b"] and built == ["a", "b", "c", "b"]
    assert len(installed) == 2


def test_engines_keep_their_plan_limit():
    from object_detectors_amd.tvision.engine import RetinaNetEngine
    from object_detectors_amd.yolo.nets.engine import YoloV3Engine
    assert YoloV3Engine.MAX_PLANS == 4 and RetinaNetEngine.MAX_PLANS == 4


def test_check_images_messages():
    def images(shape, cuda=True):
        return types.SimpleNamespace(shape=shape, is_cuda=cuda, dim=lambda: len(shape))
    assert check_images(images((2, 3, 64, 96))) == (2, 64, 96)
    for bad in (images((3, 64, 64)), images((2, 1, 64, 64)), images((2, 3, 64, 64), cuda=False)):
        with pytest.raises(ValueError, match=r"expected a CUDA tensor \[n,3,H,W\]"):
            check_images(bad)
    with pytest.raises(ValueError) as e:
        check_images(images((2, 3, 64, 48)))
    assert str(e.value) == "input size must be a multiple of 32"
    from object_detectors_amd.tvision.engine import SIZE_DIVISIBLE
    with pytest.raises(ValueError) as e:
        check_images(images((2, 3, 40, 64)), SIZE_DIVISIBLE)
    assert str(e.value) == "input size must be a multiple of 32 (GeneralizedRCNNTransform.batch_images size_divisible)"


def test_act_slice_shares_the_buffer():
    a = act(c=16)
    s = a.slice(4, 8)
    assert s.buf is a.buf and s.c == 8 and s.ld == 16 and s.ptr.value == a.ptr.value + 2 * 4 and s.parts == [] and s.needs_grad
    assert isinstance(a.ptr, C.c_void_p) and a.pixels == 32
