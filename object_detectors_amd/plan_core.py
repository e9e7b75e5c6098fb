"""What the step executors share (yolo/nets/engine.py, tvision/engine.py): a step is a static list of (function, ctypes args) tuples built
once per input shape - a "plan".  Here live the activation record, the plan cache, the list runner, the batched weight pack, the
side-stream scheduling of the weight gradients and the accumulation of activation gradients.  Graph construction, parameter layout and the
BatchNorm passes are each engine's own."""
import contextlib
import ctypes as C

import torch

from . import _lib, tune
from ._lib import check


def _vp(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off) if t is not None else None


def comm_hook(*a):   # marker: (comm_hook, (callable, *args)) entries run a python callback inside a call list
    raise RuntimeError("marker only")


class Act:
    """A [n,h,w,c] bf16 activation living in (a channel slice of) an NHWC buffer."""

    def __init__(self, buf, n, h, w, c, ld, ch_off=0, needs_grad=True):
        self.buf, self.n, self.h, self.w, self.c, self.ld, self.ch_off = buf, n, h, w, c, ld, ch_off
        self.needs_grad = needs_grad
        self.grad = None
        self.grad_written = False    # a launch has written `grad`: later contributions accumulate in place
        self.parts = []              # contributions that already exist as tensors, waiting for the first launch that writes `grad`
        self.conv_consumers = 0      # convolutions reading this activation (their dgrads all add into its gradient)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 2 * self.ch_off)

    @property
    def pixels(self):
        return self.n * self.h * self.w

    def slice(self, c0, c):
        return Act(self.buf, self.n, self.h, self.w, c, self.ld, self.ch_off + c0)


def check_images(images, why=""):
    """-> (n, H, W) of a step's input batch."""
    if images.dim() != 4 or images.shape[1] != 3 or not images.is_cuda:
        raise ValueError("expected a CUDA tensor [n,3,H,W]")
    n, _, H, W = images.shape
    if H % 32 or W % 32:
        raise ValueError("input size must be a multiple of 32" + why)
    return n, H, W


def cached_plan(eng, key, build, training, dp):
    """eng.plans as an LRU of eng.MAX_PLANS plans (most recently used last); a miss runs `build()` under tune.plan_build.
    dp: every rank is known to build this plan, so rank 0's timing choices may be broadcast (a collective)."""
    p = eng.plans.pop(key, None)
    if p is None:
        while len(eng.plans) >= eng.MAX_PLANS:
            torch.cuda.current_stream().synchronize()           # nothing of the evicted plan may still be running
            eng.plans.pop(next(iter(eng.plans)))
        p = tune.plan_build(build, share=None if dp else False)
        if training:
            for gs in getattr(eng, "grad_syncs", ()):           # parallel.GradSync.attach(): every plan gets the bucket hooks
                gs.install(p)
    eng.plans[key] = p
    return p


def build_pack_table(L, eng, specs, shape_of, need_dgrad):
    """Table of ONE batched launch that packs the fp32 master weights of `specs` into eng.packed: -> (device table, entries, blocks).
    shape_of(spec) -> (geometry-independent ConvShape, cout_pad)."""
    items = (_lib.PackItem * max(1, len(specs)))()
    for i, s in enumerate(specs):
        wf, wd = eng.packed[s.name]
        items[i].w = eng.params[s.name + ".weight"].data_ptr()
        items[i].w_fwd = wf.data_ptr()
        items[i].w_dgrad = wd.data_ptr() if (need_dgrad and wd is not None) else None
        items[i].shape, items[i].cout_pad = shape_of(s)
        items[i].w_is_ohwi = 1
    ne, nb = C.c_int32(0), C.c_int32(0)
    nbytes = L.mi355det_pack_table_bytes(items, len(specs), C.byref(ne), C.byref(nb))
    host = torch.empty(max(nbytes, 1), dtype=torch.uint8)
    check(L.mi355det_pack_table_build(items, len(specs), C.c_void_p(host.data_ptr()), nbytes), "pack_table_build")
    return host.to(eng.device), ne.value, nb.value


class PlanBase:
    """Buffers + prepared call lists for one (batch, H, W, mode)."""

    def __init__(self, eng, L, n, H, W, training, stream):
        self.eng, self.L, self.n, self.H, self.W, self.training = eng, L, n, H, W, training
        self.stream = C.c_void_p(stream)
        self.fwd, self.bwd, self.pack = [], [], []
        self.keep = []            # ctypes structs / tensors that must outlive the call lists
        self.ops = []             # forward-ordered op records for the backward builder
        self.layers = {}
        # Every gradient buffer is OWNED by the plan: the call lists bake raw device pointers, and a buffer that was only reachable through
        # an activation's `parts` queue was freed as soon as the queue handed it to a call (residual of a data gradient, operand of an
        # add) - the caching allocator then gave the block to whoever asked next (round 4 found the Faster R-CNN box head's weight packs,
        # created in the first training call, overwritten by every later backward: tests/test_gpu_fullsize_tv.py).
        self.grad_bufs = []

    def _run(self, calls):
        for fn, args in calls:
            if fn is comm_hook:
                args[0](*args[1:])
                continue
            st = fn(*args)
            if st != 0:
                check(st, fn.__name__)

    def build_pack_table(self, specs, shape_of, need_dgrad):
        """Per-step weight packing (the optimizer changes the fp32 masters): one batched launch."""
        self.pack_table, ne, nb = build_pack_table(self.L, self.eng, specs, shape_of, need_dgrad)
        self.pack.append((self.L.mi355det_pack_weights_batched, (_vp(self.pack_table), ne, nb, self.stream)))

    @contextlib.contextmanager
    def autotuning(self):
        """Plan-build time: launches inside time the library's candidate tile configurations on the plan's own buffers."""
        self.L.mi355det_conv_autotune_mode(1)
        try:
            yield
        finally:
            self.L.mi355det_conv_autotune_mode(0)

    def autotune_wgrads(self, convs):
        """Time the weight-gradient split counts; convs: (ConvShape, x pointer, dy pointer, dw tensor).  Leaves flat_g zero."""
        ws_ptr, ws_bytes = _vp(self.wgrad_ws), self.wgrad_ws.numel()
        for shp, x_ptr, dy_ptr, dw in convs:
            st = self.L.mi355det_conv_wgrad_autotune(C.byref(shp), x_ptr, dy_ptr, _vp(dw), ws_ptr, ws_bytes, self.stream)
            if st < 0:
                check(st, "conv_wgrad_autotune")
        torch.cuda.synchronize()
        self.eng.flat_g.zero_()


class BackwardSchedule:
    """Weight gradients off the dependency chain.  dz lives in two ping-pong buffers so that the weight-gradient GEMM of a layer runs on a
    SECOND stream while the main stream already does the activation backward / data gradient of the next layers; events order the two
    streams.  Owns plan.dz2 / side / wgrad_ws; appends to plan.bwd.
    (one stream for everything was the A/B of round 3: +1.0 ms per step, profiles/r03_ab_results.md)"""

    def __init__(self, plan, dev, dtype, dz_elems, ws_bytes, streams=None, new_event=None):
        """streams: (main, side), default the current stream of `dev` and a new one."""
        self.L, self.bwd = plan.L, plan.bwd
        self.main, self.side = streams or (torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev))
        self.new_event = new_event or torch.cuda.Event
        self.side_ptr = C.c_void_p(self.side.cuda_stream)
        plan.side = self.side
        plan.dz2 = self.dz2 = [torch.zeros(dz_elems, device=dev, dtype=dtype) for _ in range(2)]
        plan.wgrad_ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)       # shared: the side stream runs them in order
        self.ws = (_vp(plan.wgrad_ws), plan.wgrad_ws.numel())
        self.wg_done = [None, None]        # event: last wgrad that read dz2[i]
        self.flip = 0

    def py(self, fn, *a):
        self.bwd.append((comm_hook, (fn,) + a))

    def next_dz(self):
        """Index of the dz buffer to write next; the main stream first waits for the weight gradient that last read it."""
        di, self.flip = self.flip, self.flip ^ 1
        if self.wg_done[di] is not None:
            self.py(self.main.wait_event, self.wg_done[di])
        return di

    def publish(self):
        """What the main stream has produced so far becomes visible to the side stream."""
        ev = self.new_event()
        self.py(ev.record, self.main)
        self.py(self.side.wait_event, ev)

    def wgrad(self, shp, x_ptr, dy_ptr, dw, dbias, dz_index=None, record=True, groups=1):
        """mi355det_conv_wgrad (groups > 1: mi355det_gconv_wgrad, which has no bias sum) on the side stream, behind everything the main
        stream has issued; dz_index: dy is dz2[dz_index]."""
        self.publish()
        if groups > 1:
            assert dbias is None
            self.bwd.append((self.L.mi355det_gconv_wgrad, (C.byref(shp), groups, x_ptr, dy_ptr, _vp(dw)) + self.ws + (self.side_ptr,)))
        else:
            self.bwd.append((self.L.mi355det_conv_wgrad, (C.byref(shp), x_ptr, dy_ptr, _vp(dw), _vp(dbias)) + self.ws + (self.side_ptr,)))
        if record:
            ev = self.new_event()
            self.py(ev.record, self.side)
            if dz_index is not None:
                self.wg_done[dz_index] = ev

    def close(self, plan):
        ev = self.new_event()
        self.py(ev.record, self.side)
        self.py(self.main.wait_event, ev)             # join: backward is complete on the main stream
        plan.side_stream = self.side


class GradAccumulator:
    """An activation's gradient is the sum of its consumers' contributions (ops are walked in reverse).  Contributions that already exist
    as tensors queue up in `Act.parts`; the first data-gradient GEMM takes one of them as its epilogue residual, later ones accumulate
    in place (residual == dx), what is left goes through mi355det_add_bf16.
    dgrad_call(shape, dy_ptr, packed_w, grad_act, residual_ptr, residual_ld) -> the (fn, args) entry of one data gradient."""

    def __init__(self, L, dev, dtype, plan, dgrad_call):
        self.L, self.dev, self.dtype, self.dgrad_call = L, dev, dtype, dgrad_call
        self.bwd, self.grad_bufs, self.stream = plan.bwd, plan.grad_bufs, plan.stream

    def dense(self, a):
        g = Act(torch.zeros((a.n, a.h, a.w, a.c), device=self.dev, dtype=self.dtype), a.n, a.h, a.w, a.c, a.c)
        self.grad_bufs.append(g.buf)
        return g

    def grad_of(self, a):
        if a.grad is None:
            a.grad = self.dense(a)
        return a.grad

    def _add(self, a, p, q, out):
        self.bwd.append((self.L.mi355det_add_bf16, (p.ptr, p.ld, q.ptr, q.ld, a.c, a.pixels, out.ptr, out.ld, self.stream)))

    def _drain(self, a):
        while a.parts:
            self._add(a, a.grad, a.parts.pop(0), a.grad)

    def add_tensor(self, x, t):
        if not x.needs_grad:
            return
        if x.grad_written:
            self._add(x, x.grad, t, x.grad)
        else:
            x.parts.append(t)

    def add_dgrad(self, x, shp, dy_ptr, wd, call=None):
        """call: this data gradient's own form (fused epilogues, the FPN's upsample backward) instead of dgrad_call."""
        if not x.needs_grad:
            return
        g, call = self.grad_of(x), call or self.dgrad_call
        if x.grad_written:
            self.bwd.append(call(shp, dy_ptr, wd, g, g.ptr, g.ld))
            return
        r = x.parts.pop(0) if x.parts else None
        self.bwd.append(call(shp, dy_ptr, wd, g, r.ptr if r else None, r.ld if r else 0))
        x.grad_written = True
        self._drain(x)

    def finalize(self, a):
        """Gradient of `a` once every consumer has contributed; None if nothing flows back."""
        if a.grad_written:
            return a.grad
        if not a.parts:
            return None
        if len(a.parts) == 1:
            a.grad = a.parts.pop(0)          # alias, no copy
        else:
            a.grad = self.dense(a)
            self._add(a, a.parts.pop(0), a.parts.pop(0), a.grad)
            self._drain(a)
        a.grad_written = True
        return a.grad
