"""What the step executors share (yolo/nets/engine.py, tvision/engine.py): a step is a static list of (function, ctypes args) tuples built
once per input shape - a "plan".  Here live the activation record, the plan cache, the emitter through which every call enters a list (and
the plan comes to own what the call points at), the list runner, the batched weight pack, the side-stream scheduling of the weight gradients
and the accumulation of activation gradients.  Graph construction, parameter layout and the BatchNorm passes are each engine's own."""
import collections
import contextlib
import ctypes as C

import torch

from . import _lib, tune
from ._lib import check

IMAGE = object()                                     # operand of PlanBase.emit: the image of the current step (PlanBase.set_image)
at = collections.namedtuple("at", "base nbytes")     # operand: `nbytes` past the address of a tensor or Act
CALL_LISTS = ("pack", "fwd_const", "fwd", "bwd", "bwd_base", "cast", "cast_box")


def address(a, owned=None, off=0):
    """The ctypes value of one call operand: tensor -> its data pointer, Act -> its slice pointer, at(..) -> that plus a byte offset,
    ctypes Structure -> byref; numbers, None and stream pointers as they are.  `owned` (a plan's) retains every tensor / struct that is
    turned into an address; without it the caller keeps them alive for the duration of an immediate call."""
    if isinstance(a, at):
        return address(a.base, owned, off + a.nbytes)
    if isinstance(a, Act):
        return address(a.buf, owned, off + 2 * a.ch_off)
    if isinstance(a, (torch.Tensor, C.Structure)):
        if owned is not None:
            owned[id(a)] = a
        return C.c_void_p(a.data_ptr() + off) if isinstance(a, torch.Tensor) else C.byref(a)
    return a


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
        return address(self)

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


def build_pack_table(L, eng, specs, shape_of, need_dgrad, owned=None):
    """Table of ONE batched launch that packs the fp32 master weights of `specs` into eng.packed: -> (device table, entries, blocks).
    shape_of(spec) -> (geometry-independent ConvShape, cout_pad).  The table lives in device memory: the addresses in it are retained
    through `owned` like any operand, but audit() cannot read them back."""
    items = (_lib.PackItem * max(1, len(specs)))()
    for i, s in enumerate(specs):
        wf, wd = eng.packed[s.name]
        items[i].w = address(eng.params[s.name + ".weight"], owned)
        items[i].w_fwd = address(wf, owned)
        items[i].w_dgrad = address(wd if need_dgrad else None, owned)
        items[i].shape, items[i].cout_pad = shape_of(s)
        items[i].w_is_ohwi = 1
    ne, nb = C.c_int32(0), C.c_int32(0)
    nbytes = L.mi355det_pack_table_bytes(items, len(specs), C.byref(ne), C.byref(nb))
    host = torch.empty(max(nbytes, 1), dtype=torch.uint8)
    check(L.mi355det_pack_table_build(items, len(specs), address(host), nbytes), "pack_table_build")
    return host.to(eng.device), ne.value, nb.value


class PlanBase:
    """Buffers + prepared call lists for one (batch, H, W, mode)."""

    def __init__(self, eng, L, n, H, W, training, stream):
        self.eng, self.L, self.n, self.H, self.W, self.training = eng, L, n, H, W, training
        self.stream = C.c_void_p(stream)
        self.fwd, self.bwd, self.pack = [], [], []
        self.ops = []             # forward-ordered op records for the backward builder
        self.layers = {}
        # The call lists bake raw device pointers, so the plan OWNS what they point at: emit() is the only place where plan-building code
        # turns a tensor / Act / struct into an address, and it retains the object here (by identity) as it does so.  Why: a gradient
        # buffer that was only reachable through an activation's `parts` queue was freed as soon as the queue handed it to a call
        # (residual of a data gradient, operand of an add) - the caching allocator then gave the block to whoever asked next (round 4
        # found the Faster R-CNN box head's weight packs, created in the first training call, overwritten by every later backward:
        # tests/test_gpu_fullsize_tv.py).  audit() checks the result.
        self.owned = {}
        self.image, self.img_slots = None, []     # the step's input (set_image) and the (argument list, index) places that hold its address

    def emit(self, calls, fn, *args):
        """Append (fn, resolved args) to `calls` and return the entry; see address() for the operand forms.  IMAGE leaves a null that
        set_image() patches (such an entry's arguments are a list)."""
        out = [None if a is IMAGE else address(a, self.owned) for a in args]
        slots = [(out, i) for i, a in enumerate(args) if a is IMAGE]
        self.img_slots += slots
        calls.append((fn, out if slots else tuple(out)))
        return calls[-1]

    def epilogue(self, scale, shift, residual, relu, out_image_stride=0, slope=0.0):
        """ConvEpilogue whose pointer fields come from operands (residual: an Act or None) that the plan retains with the struct."""
        e = _lib.ConvEpilogue(address(scale, self.owned), address(shift, self.owned), address(residual, self.owned),
                              residual.ld if residual is not None else 0, relu, out_image_stride, slope)
        self.owned[id(e)] = e
        return e

    def set_image(self, images):
        """Point every IMAGE slot (forward and backward stem kernels read the fp32 input) at `images`, which stays referenced until the
        next call: the slots never dangle."""
        self.image, ptr = images, address(images)
        for args, i in self.img_slots:
            args[i] = ptr

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
        table, ne, nb = build_pack_table(self.L, self.eng, specs, shape_of, need_dgrad, self.owned)
        self.emit(self.pack, self.L.mi355det_pack_weights_batched, table, ne, nb, self.stream)

    @contextlib.contextmanager
    def autotuning(self):
        """Plan-build time: launches inside time the library's candidate tile configurations on the plan's own buffers."""
        self.L.mi355det_conv_autotune_mode(1)
        try:
            yield
        finally:
            self.L.mi355det_conv_autotune_mode(0)

    def autotune_wgrads(self, convs):
        """Time the weight-gradient split counts; convs: (ConvShape, x operand, dy operand, dw tensor).  Leaves flat_g zero."""
        for shp, x, dy, dw in convs:
            fn, args = self.emit([], self.L.mi355det_conv_wgrad_autotune, shp, x, dy, dw, self.wgrad_ws, self.wgrad_ws.numel(), self.stream)
            st = fn(*args)
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
        self.L, self.bwd, self.emit = plan.L, plan.bwd, plan.emit
        self.main, self.side = streams or (torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev))
        self.new_event = new_event or torch.cuda.Event
        self.side_ptr = C.c_void_p(self.side.cuda_stream)
        plan.side = self.side
        plan.dz2 = self.dz2 = [torch.zeros(dz_elems, device=dev, dtype=dtype) for _ in range(2)]
        plan.wgrad_ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)       # shared: the side stream runs them in order
        self.ws = (plan.wgrad_ws, plan.wgrad_ws.numel())
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

    def wgrad(self, shp, x, dy, dw, dbias, dz_index=None, record=True, groups=1):
        """mi355det_conv_wgrad (groups > 1: mi355det_gconv_wgrad, which has no bias sum) on the side stream, behind everything the main
        stream has issued; x, dy, dw, dbias: operands of emit; dz_index: dy is dz2[dz_index]."""
        self.publish()
        if groups > 1:
            assert dbias is None
            self.emit(self.bwd, self.L.mi355det_gconv_wgrad, shp, groups, x, dy, dw, *self.ws, self.side_ptr)
        else:
            self.emit(self.bwd, self.L.mi355det_conv_wgrad, shp, x, dy, dw, dbias, *self.ws, self.side_ptr)
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
    dgrad_call(shape, dy, packed_w, grad_act, residual, residual_ld) -> (fn, *operands of emit) of one data gradient; dy, residual: Act / tensor."""

    def __init__(self, L, dev, dtype, plan, dgrad_call):
        self.L, self.dev, self.dtype, self.dgrad_call = L, dev, dtype, dgrad_call
        self.bwd, self.emit, self.stream = plan.bwd, plan.emit, plan.stream

    def dense(self, a):
        return Act(torch.zeros((a.n, a.h, a.w, a.c), device=self.dev, dtype=self.dtype), a.n, a.h, a.w, a.c, a.c)

    def grad_of(self, a):
        if a.grad is None:
            a.grad = self.dense(a)
        return a.grad

    def _add(self, a, p, q, out):
        self.emit(self.bwd, self.L.mi355det_add_bf16, p, p.ld, q, q.ld, a.c, a.pixels, out, out.ld, self.stream)

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

    def add_dgrad(self, x, shp, dy, wd, call=None):
        """call: this data gradient's own form (fused epilogues, the FPN's upsample backward) instead of dgrad_call."""
        if not x.needs_grad:
            return
        g, call = self.grad_of(x), call or self.dgrad_call
        r = g if x.grad_written else x.parts.pop(0) if x.parts else None
        self.emit(self.bwd, *call(shp, dy, wd, g, r, r.ld if r else 0))
        if x.grad_written:
            return
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


def audit(plan):
    """Every non-null pointer baked into the plan's call lists - c_void_p arguments other than the plan's streams, the pointer fields of
    structs passed by reference (ConvEpilogue), the image slots - must lie inside a tensor the plan retains (`owned`, `image`).  Raises
    ValueError naming the list, the index and the function.  Out of reach: the addresses inside the device-resident pack table
    (build_pack_table retains their tensors; the table itself is GPU memory)."""
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in [*plan.owned.values(), plan.image] if isinstance(t, torch.Tensor)]
    side = getattr(plan, "side", None)
    good = {None, plan.stream.value, side and side.cuda_stream}      # null, the streams, and every address already found inside a span
    for name in CALL_LISTS:
        for i, (fn, args) in enumerate(getattr(plan, name, None) or ()):
            for j, a in enumerate(() if fn is comm_hook else args):
                obj = getattr(a, "_obj", None)                       # byref(struct): its pointer fields
                fields = [("." + f, getattr(obj, f)) for f, t in getattr(obj, "_fields_", ()) if t is C.c_void_p]
                for field, p in [("", a.value)] if isinstance(a, C.c_void_p) else fields:
                    if p not in good and not any(lo <= p < hi for lo, hi in spans):
                        raise ValueError(f"{name}[{i}] {fn.__name__}: argument {j}{field} = {p:#x} is in no tensor the plan owns")
                    good.add(p)
