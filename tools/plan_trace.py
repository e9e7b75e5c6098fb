#!/usr/bin/env python3
"""Canonical trace of the call lists of small plans of every engine: the proof that a change to the plan builders left every step as it was.

    python tools/plan_trace.py OUT.json          # at two commits, then `diff` the two files

Per plan and per list (pack, fwd_const, fwd, bwd, bwd_base, cast) every entry becomes [function name, canonical arguments]: numbers
verbatim, a ConvShape as its 12 fields, a ConvEpilogue as its scalars plus null / non-null of its pointers, and every pointer, tensor, stream
and event as the index of its first appearance within the plan (null for None) - addresses differ between runs, the wiring must not.
A python callback entry is the callable's __qualname__ (with the index of the object a bound method belongs to) and its arguments.
`bwd_marks` is dumped as it is."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from object_detectors_amd import _lib, tune  # noqa: E402
from object_detectors_amd.yolo.nets.engine import comm_hook  # noqa: E402

LISTS = ("pack", "fwd_const", "fwd", "bwd", "bwd_base", "cast")


class Canon:
    def __init__(self):
        self.ids = {}

    def ref(self, key):
        return {"ref": self.ids.setdefault(key, len(self.ids))}

    def value(self, a):
        if a is None:
            return None
        if isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, C.c_void_p):
            return None if a.value is None else self.ref(("p", a.value))
        if isinstance(a, _lib.ConvShape):
            return {"ConvShape": [getattr(a, f) for f, _t in _lib.ConvShape._fields_]}
        if isinstance(a, _lib.ConvEpilogue):
            return {"ConvEpilogue": {f: (getattr(a, f) is not None) if t is C.c_void_p else getattr(a, f) for f, t in _lib.ConvEpilogue._fields_}}
        if hasattr(a, "_obj"):                                       # ctypes.byref(struct)
            return self.value(a._obj)
        if isinstance(a, torch.Tensor):
            return self.ref(("p", a.data_ptr()))
        if isinstance(a, torch.cuda.Stream):
            return self.ref(("p", a.cuda_stream))
        if isinstance(a, torch.cuda.Event):
            return self.ref(("e", id(a)))
        if isinstance(a, (list, tuple)):
            return [self.value(v) for v in a]
        if callable(a):
            out = {"call": getattr(a, "__qualname__", type(a).__name__)}
            if getattr(a, "__self__", None) is not None and isinstance(a.__self__, (torch.cuda.Stream, torch.cuda.Event)):
                out["self"] = self.value(a.__self__)
            return out
        raise TypeError(f"plan_trace: no canonical form for {type(a)}")

    def entry(self, fn, args):
        if fn is comm_hook:
            return ["comm_hook", self.value(args[0]), [self.value(v) for v in args[1:]]]
        return [fn.__name__, [self.value(v) for v in args]]


def trace(plan):
    c = Canon()
    out = {}
    for name in LISTS:
        calls = getattr(plan, name, None)
        if calls is not None:
            out[name] = [c.entry(fn, args) for fn, args in calls]
    out["bwd_marks"] = [list(m) for m in getattr(plan, "bwd_marks", [])]
    return out


def yolo_configs(dev):
    from object_detectors_amd.parallel import GradSync
    from object_detectors_amd.yolo.nets.engine import YoloV3Engine

    def plans(tag, modes, attach=False, freeze=False, **kw):
        tune.clear()
        eng = YoloV3Engine(device=dev, **kw)
        if attach:
            GradSync(eng.flat_g, bucket_mb=1).attach(eng)
        for training in modes:
            yield f"yolo/{tag}/{'train' if training else 'eval'}", eng.plan(2, 128, 128, training)
        if freeze:
            eng.freeze_inference()
            eng.forward(torch.rand((2, 3, 128, 128), device=dev), training=False)
            yield f"yolo/{tag}/eval_frozen", eng._last_plan
    yield from plans("darknet_53", (True, False), freeze=True, backbone="darknet_53")
    yield from plans("darknet_21_fp16", (True, False), backbone="darknet_21", storage="fp16")
    yield from plans("darknet_21_atomic", (True,), backbone="darknet_21", deterministic=False)
    yield from plans("darknet_21_fuse_bn", (True,), backbone="darknet_21", fuse_bn_reduce=True)
    yield from plans("darknet_21_gradsync", (True,), attach=True, backbone="darknet_21")


def tv_configs(dev):
    from object_detectors_amd.tvision.engine import FasterRCNNEngine, RetinaNetEngine
    for tag, make, modes in (("retinanet_t3", lambda: RetinaNetEngine(trainable_layers=3, device=dev), (True, False)),
                             ("retinanet_t5", lambda: RetinaNetEngine(trainable_layers=5, device=dev), (True,)),
                             ("fasterrcnn", lambda: FasterRCNNEngine(device=dev), (True, False))):
        for size in ((128, 128), (160, 128)):
            tune.clear()
            eng = make()
            for training in modes:
                yield f"{tag}/{size[0]}x{size[1]}/{'train' if training else 'eval'}", eng.plan(2, size[0], size[1], training)


def main():
    dev = torch.device("cuda:0")
    out = {}
    for gen in (yolo_configs, tv_configs):
        for name, plan in gen(dev):
            out[name] = trace(plan)
            print(name, {k: len(v) for k, v in out[name].items()}, file=sys.stderr, flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
