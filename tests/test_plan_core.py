"""plan_core on the CPU: the shared pieces of the two step executors driven with a stub library that only records names."""
import ctypes as C
import gc
import types
import weakref

import pytest
import torch

from object_detectors_amd import _lib, plan_core
from object_detectors_amd.plan_core import IMAGE, Act, BackwardSchedule, GradAccumulator, PlanBase, at, audit, cached_plan, check_images, comm_hook


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
    def dgrad_call(shp, dy, wd, g, r, rld):
        return (plan.L.mi355det_conv_dgrad, shp, dy, wd, g, r, rld)
    return GradAccumulator(plan.L, "cpu", torch.bfloat16, plan, dgrad_call)


def owned_tensors(plan):
    """The tensors the plan retains, by identity."""
    return {k for k, v in plan.owned.items() if isinstance(v, torch.Tensor)}


def bufs(*acts):
    return {id(a.buf) for a in acts}


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
    assert yolo_engine.Act is Act
    for mod, plan_cls in ((yolo_engine, yolo_engine.Plan), (tv_engine, tv_engine.RetinaPlan)):      # one emitter, no pointer helper of their own
        assert plan_cls.emit is PlanBase.emit and plan_cls.set_image is PlanBase.set_image and plan_cls.epilogue is PlanBase.epilogue
        assert not hasattr(mod, "_vp") and getattr(mod, "address", plan_core.address) is plan_core.address
    for name in ("bn_name", "arch", "BLOCKS"):
        assert hasattr(yolo_engine, name)


def test_single_consumer_nothing_pending_gets_null_residual():
    plan = make_plan()
    acc, x = make_acc(plan), act()
    acc.add_dgrad(x, "shp", "dy", "wd")
    assert names(plan) == ["mi355det_conv_dgrad"]
    shp, dy, wd, gp, rptr, rld = plan.bwd[0][1]
    assert (shp, dy, wd, rptr, rld) == ("shp", "dy", "wd", None, 0)
    g = x.grad
    assert pv(gp) == pv(g.ptr) and x.grad_written and (g.n, g.h, g.w, g.c, g.ld) == (2, 4, 4, 8, 8)
    assert owned_tensors(plan) == bufs(g) and plan.owned[id(g.buf)] is g.buf


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
    assert fn.__name__ == "mi355det_conv_dgrad" and shp == "shp2" and x.grad is g and pv(g2) == pv(g.ptr) and pv(rptr) == pv(g.ptr) and rld == g.ld
    # a tensor arriving after the gradient was written is added at once
    t4 = act()
    acc.add_tensor(x, t4)
    assert add_args(plan.bwd[-1]) == (pv(g.ptr), g.ld, pv(t4.ptr), t4.ld, x.c, x.pixels, pv(g.ptr), g.ld) and x.parts == []
    assert owned_tensors(plan) == bufs(g, t1, t2, t3, t4)         # ONE gradient buffer, and every operand a call points at


def test_own_call_form_and_no_gradient_needed():
    plan = make_plan()
    acc = make_acc(plan)
    frozen = act(needs_grad=False)
    acc.add_tensor(frozen, act())
    acc.add_dgrad(frozen, "shp", "dy", "wd")
    assert plan.bwd == [] and frozen.grad is None and frozen.parts == [] and plan.owned == {}
    x, t = act(), act()
    acc.add_tensor(x, t)
    acc.add_dgrad(x, "shp", "dy", "wd", lambda shp, dy, wd, g, r, rld: (plan.L.mi355det_conv_dgrad_mask, g, r, rld))
    assert names(plan) == ["mi355det_conv_dgrad_mask"]
    assert pv(plan.bwd[0][1][0]) == pv(x.grad.ptr) and pv(plan.bwd[0][1][1]) == pv(t.ptr) and x.grad_written
    assert owned_tensors(plan) == bufs(x.grad, t)


def test_finalize_aliases_one_part_and_sums_more():
    plan = make_plan()
    acc = make_acc(plan)
    a, t = act(), act()
    assert acc.finalize(a) is None and not a.grad_written
    acc.add_tensor(a, t)
    assert acc.finalize(a) is t and a.grad is t and a.grad_written           # alias: no copy, no buffer
    assert plan.bwd == [] and plan.owned == {}
    assert acc.finalize(a) is t
    b, p0, p1, p2 = act(), act(), act(), act()
    for t in (p0, p1, p2):
        acc.add_tensor(b, t)
    g = acc.finalize(b)
    assert g is b.grad and b.grad_written and b.parts == []
    assert owned_tensors(plan) == bufs(g, p0, p1, p2)
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


def build_local_plan():
    """A plan whose every operand exists only as a local of this function: -> (plan, weak references to the operands)."""
    plan = make_plan()
    L = plan.L
    t, off_t = torch.zeros(64), torch.zeros(96)
    a = act(c=16).slice(4, 8)
    scale, res = torch.ones(8), act()
    shp = _lib.ConvShape(2, 4, 4, 8, 4, 4, 8, 1, 1, 0, 8, 8)
    e = plan.epilogue(scale, at(scale, 16), res, 1, 0, 0.1)
    assert (e.scale, e.shift, e.residual, e.residual_ld, e.relu) == (scale.data_ptr(), scale.data_ptr() + 16, pv(res.ptr), res.ld, 1)
    fn, args = plan.emit(plan.fwd, L.mi355det_conv_fwd_ex, shp, a, t, e, at(off_t, 128), 0, None, 2.5, plan.stream)
    assert plan.fwd == [(fn, args)] and isinstance(args, tuple) and fn.__name__ == "mi355det_conv_fwd_ex"
    assert args[0]._obj is shp and args[3]._obj is e and args[5:8] == (0, None, 2.5) and args[8] is plan.stream
    assert (pv(args[1]), pv(args[2]), pv(args[4])) == (a.buf.data_ptr() + 2 * 4, t.data_ptr(), off_t.data_ptr() + 128)
    plan.emit(plan.bwd, L.mi355det_add_bf16, res, res.ld, a, a.ld, plan.stream)
    return plan, [weakref.ref(o) for o in (t, off_t, a.buf, scale, res.buf, shp, e)]


def test_ownership_survives_the_builder():
    plan, refs = build_local_plan()
    gc.collect()
    assert all(r() is not None for r in refs)
    assert all(id(r()) in plan.owned for r in refs)
    audit(plan)
    del plan
    gc.collect()
    assert all(r() is None for r in refs)


def test_audit_names_the_call_that_points_outside():
    plan, _refs = build_local_plan()
    audit(plan)
    stray = torch.zeros(8)
    plan.bwd.append((plan.L.mi355det_add_bf16, (C.c_void_p(stray.data_ptr()), 8)))
    with pytest.raises(ValueError, match=r"bwd\[1\] mi355det_add_bf16: argument 0 "):
        audit(plan)
    plan.bwd.pop()
    audit(plan)
    whole = torch.zeros(64)
    part = whole[:5]                                  # owned: 20 bytes; the byte behind them belongs to `whole`, which the plan does not own
    plan.cast = []
    plan.emit(plan.cast, plan.L.mi355det_cast_rows_bf16, part, at(part, 19))
    audit(plan)
    plan.cast.append((plan.L.mi355det_cast_rows_bf16, (None, C.c_void_p(part.data_ptr() + 20))))
    with pytest.raises(ValueError, match=r"cast\[1\] mi355det_cast_rows_bf16: argument 1 "):
        audit(plan)
    plan.cast.pop()
    e = plan.fwd[0][1][3]._obj
    e.residual = stray.data_ptr()
    with pytest.raises(ValueError, match=r"fwd\[0\] mi355det_conv_fwd_ex: argument 3\.residual "):
        audit(plan)
    e.residual = None
    audit(plan)


def test_audit_skips_streams_and_hooks():
    plan = make_plan()
    sched, _main, _side = make_schedule(plan)            # side stream handle 7: no tensor lives there
    x, dy, dw = act(), act(), torch.zeros(8, 8)
    sched.wgrad(_lib.ConvShape(), x, dy, dw, None)
    sched.close(plan)
    audit(plan)
    plan.bwd.append((plan.L.mi355det_x, (C.c_void_p(8),)))
    with pytest.raises(ValueError, match=r"bwd\[\d+\] mi355det_x: argument 0 "):
        audit(plan)


def test_set_image_patches_every_slot_and_holds_the_tensor():
    plan = make_plan()
    L, w = plan.L, torch.zeros(8)
    plan.emit(plan.fwd, L.mi355det_stem_fwd_stats, IMAGE, w, 2, plan.stream)
    plan.emit(plan.fwd, L.mi355det_other, w, 3)
    plan.emit(plan.fwd, L.mi355det_stem_l1_fwd, IMAGE, w, 0.1)
    plan.emit(plan.bwd, L.mi355det_stem_bwd_fused, IMAGE, w, plan.stream)
    slots = [plan.fwd[0][1], plan.fwd[2][1], plan.bwd[0][1]]
    assert all(isinstance(a, list) and a[0] is None for a in slots) and isinstance(plan.fwd[1][1], tuple)
    assert [len(a) for a in slots] == [4, 3, 3] and pv(slots[0][1]) == w.data_ptr() and slots[0][2] == 2
    audit(plan)                                           # a null slot points nowhere
    bwd_with_hooks = list(plan.bwd)                       # parallel.GradSync.install copies the entries into a new list
    for _ in range(2):
        img = torch.rand(2, 3, 8, 8)
        ref = weakref.ref(img)
        plan.set_image(img)
        del img
        gc.collect()
        assert ref() is not None and plan.image is ref()
        assert all(pv(a[0]) == ref().data_ptr() for a in slots) and pv(bwd_with_hooks[0][1][0]) == ref().data_ptr()
        audit(plan)
    gc.collect()
    plan.image = None                                     # without the tensor the slot dangles, and audit says so
    with pytest.raises(ValueError, match=r"fwd\[0\] mi355det_stem_fwd_stats: argument 0 "):
        audit(plan)


def test_operands_as_objects_give_the_pinned_calls():
    plan = make_plan()
    sched, _main, side = make_schedule(plan)
    shp = _lib.ConvShape(2, 4, 4, 8, 4, 4, 8, 3, 1, 1, 8, 8)
    x, dy, dw, db = act(c=16).slice(8, 8), torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16), torch.zeros(8, 3, 3, 8), torch.zeros(8)
    sched.wgrad(shp, x, dy, dw, db, record=False)
    sched.wgrad(shp, x, dy, dw, None, record=False, groups=4)
    with pytest.raises(AssertionError):
        sched.wgrad(shp, x, dy, dw, db, groups=4)          # the grouped weight gradient has no bias sum
    ws, nbytes = plan.wgrad_ws.data_ptr(), plan.wgrad_ws.numel()
    (f0, a0), (f1, a1) = [e for e in plan.bwd if e[0] is not comm_hook]
    assert f0.__name__ == "mi355det_conv_wgrad" and f1.__name__ == "mi355det_gconv_wgrad"
    assert a0[0]._obj is shp and [pv(v) for v in a0[1:6]] == [pv(x.ptr), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), ws]
    assert a0[6] == nbytes and a0[7].value == side.cuda_stream and len(a0) == 8
    assert a1[0]._obj is shp and a1[1] == 4 and [pv(v) for v in a1[2:6]] == [pv(x.ptr), dy.data_ptr(), dw.data_ptr(), ws]
    assert a1[6] == nbytes and a1[7].value == side.cuda_stream and len(a1) == 8
    # a data gradient in its own form (the engines' fused epilogues): operands go in as objects, the entry holds their addresses
    acc = GradAccumulator(plan.L, "cpu", torch.bfloat16, plan, None)
    y, part, wd = act(), act(), torch.zeros(64, dtype=torch.bfloat16)
    acc.add_tensor(y, part)
    acc.add_dgrad(y, shp, dy, wd, lambda shp, dy, wd, g, r, rld: (plan.L.mi355det_conv_dgrad_mask, shp, dy, wd, g, x, x.ld, None, 1, plan.stream))
    fn, args = plan.bwd[-1]
    assert fn.__name__ == "mi355det_conv_dgrad_mask" and args[0]._obj is shp and args[5:8] == (16, None, 1) and args[8] is plan.stream
    assert [pv(v) for v in args[1:5]] == [dy.data_ptr(), wd.data_ptr(), pv(y.grad.ptr), pv(x.ptr)]
    assert y.parts == [] and y.grad_written          # the form ignored the residual: the accumulator handed it over all the same (as before)
    assert owned_tensors(plan) >= {id(dy), id(dw), id(db), id(wd), id(plan.wgrad_ws)} | bufs(x, y.grad)
    audit(plan)
