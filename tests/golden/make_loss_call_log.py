"""Record what the loss stack asks of the library: per scenario the ordered Device.call names with their scalar arguments.

The scenarios run through the real host stack over the stand-in library (tests/fake_lib.py), so no GPU is needed and no number
means anything; what is pinned is WHICH entry points a combination of losses reaches, in which order, how often and with which
settings and coefficients.  tests/test_loss_call_log.py replays the scenarios and compares with the file written here, so the
file is regenerated only when the calls are MEANT to change:

    python tests/golden/make_loss_call_log.py        # writes tests/golden/loss_call_log.json

It needs a tree that imports: a built libmsegk.so (./build.sh), or MSEGK_LIB pointing at any library that loads -- importing
medicalseg_amd loads the library once before tests/fake_lib.py can put the stand-in in its place.

An argument is written as: an int or a float as itself (a c_float as the float32 value it carries), a pointer as "ptr" or None
(null), a tensor as {"t": [n, d, h, w, c, ld]}, an array of ints as a list, an array of pointers as its length in {"ptrs": n}.
An entry point the stand-in lacks (msk_bce_*) is recorded and not called.  The logits are empty arena tensors with a stub
producer: only the loss calls and their memory traffic appear.
"""
import contextlib
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "loss_call_log.json")
SOURCES = ("fake_msegk.c", "fake_msegk_region.c", "fake_msegk_pyramid.c")
SHAPE = (16, 16, 16)
HEAD_EXTENTS = ((2, 2, 2), (4, 4, 4), (8, 8, 8))


def _plain(a):
    from medicalseg_amd._lib import MskTensor
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, MskTensor):
        return {"t": [a.n, a.d, a.h, a.w, a.c, a.ld]}
    if isinstance(a, C.c_void_p):
        return None if a.value is None else "ptr"
    if isinstance(a, C.Array):
        if issubclass(a._type_, C.c_void_p):
            return {"ptrs": len(a)}
        return [int(v) for v in a]
    if isinstance(a, C._SimpleCData):
        return a.value
    return "ptr"      # byref(...) and the like


@contextlib.contextmanager
def recorder():
    """Device.call replaced by one that notes [name, args...]; yields the list"""
    from medicalseg_amd.device import Device
    log = []
    real = Device.call

    def recording(self, name, *args):
        log.append([name] + [_plain(a) for a in args])
        if getattr(getattr(self.lib, name), "missing", False):
            return None
        return real(self, name, *args)
    Device.call = recording
    try:
        yield log
    finally:
        Device.call = real


class _Producer:
    """stands in as the model that produced the logits: Scalar.backward hands it the gradients"""

    def __init__(self, num_outputs=1):
        self.num_outputs = num_outputs
        self.grads = []

    def backward(self, grads):
        self.grads.append(grads)


def _inputs(ncls, heads=False):
    """a new arena generation with empty logits (one tensor, or the four of a native-heads model) and a device label"""
    from medicalseg_amd.device import Tensor, get_device, to_tensor
    dev = get_device()
    dev.arena.reset()
    extents = [SHAPE] + (list(HEAD_EXTENTS) if heads else [])
    prod = _Producer(len(extents))
    outs = []
    for i, (d, h, w) in enumerate(extents):
        t = Tensor.empty(dev, 1, d, h, w, ncls)
        t.producer, t.out_index = prod, i
        if i:
            t.native_head = (HEAD_EXTENTS, i - 1)
        outs.append(t)
    y = to_tensor(np.random.default_rng(0).integers(0, ncls, (1,) + SHAPE).astype(np.int32))
    return outs, y, prod


def _finish(loss_list, prod):
    total = sum(loss_list)
    total.backward()
    float(total)
    assert len(prod.grads) == 1


def ce_dice(log):                       # (a) the benchmark's loss
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    (z,), y, prod = _inputs(3)
    del log[:]
    terms, _ = MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])(z, y)
    _finish(terms, prod)


def dice_softmax_weighted(log):         # (b) the dummy CE weights and their upload
    from medicalseg_amd.models import DiceLoss
    (z,), y, prod = _inputs(3)
    del log[:]
    loss, _ = DiceLoss(sigmoid_norm=False, weight=[1.0, 2.0, 0.5])(z, y)
    _finish([loss], prod)


def ce_and_bce(log):                    # (c) a writing and an accumulating node on one logits tensor
    from medicalseg_amd.models import BCELoss, CrossEntropyLoss
    (z,), y, prod = _inputs(3)
    del log[:]
    _finish([CrossEntropyLoss()(z, y), BCELoss(weight='dynamic', pos_weight='dynamic')(z, y)], prod)


def dicece(log):                        # (d)
    from medicalseg_amd.models import DiceCELoss
    (z,), y, prod = _inputs(3)
    del log[:]
    loss, _ = DiceCELoss()(z, y)
    _finish([loss], prod)


def weighted_ce_and_focal_dicece(log):  # (e)
    from medicalseg_amd.models import CrossEntropyLoss, DiceCELoss, MixedLoss
    (z,), y, prod = _inputs(3)
    del log[:]
    terms, _ = MixedLoss([CrossEntropyLoss(weight=[1.0, 2.0, 3.0]), DiceCELoss(lambda_ce=0.5, gamma=2)], [1, 1])(z, y)
    _finish(terms, prod)


def four_native_heads(log):             # (f) one msk_label_pyramid for the three heads
    from medicalseg_amd.models import DiceCELoss
    from medicalseg_amd.utils import loss_computation
    outs, y, prod = _inputs(3, heads=True)
    del log[:]
    loss_list, _ = loss_computation(outs, y, {"types": [DiceCELoss() for _ in outs], "coef": [0.4, 0.1, 0.2, 0.3]})
    _finish(loss_list, prod)
    assert len(prod.grads[0]) == 4 and sum(c[0] == "msk_label_pyramid" for c in log) == 1


def same_loss_twice(log):               # (g) the second call takes the cached node: no second forward
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    (z,), y, prod = _inputs(3)
    del log[:]
    mixed = MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])
    first, _ = mixed(z, y)
    float(sum(first))
    second, _ = mixed(z, y)
    assert second[0].terms[0][1] is first[0].terms[0][1]
    _finish(first + second, prod)
    assert sum(c[0] == "msk_loss_fwd_ex" for c in log) == 1


def ce_then_another_ignore_index(log):  # (h) changed settings evaluate the node again
    from medicalseg_amd.models import CrossEntropyLoss
    (z,), y, prod = _inputs(3)
    del log[:]
    first = CrossEntropyLoss()(z, y)
    float(first)
    second = CrossEntropyLoss(ignore_index=0)(z, y)
    _finish([first, second], prod)
    assert sum(c[0] == "msk_loss_fwd_ex" for c in log) == 2


SCENARIOS = (ce_dice, dice_softmax_weighted, ce_and_bce, dicece, weighted_ce_and_focal_dicece, four_native_heads,
             same_loss_twice, ce_then_another_ignore_index)


def run(scenario):
    """the calls of one scenario, as the JSON file holds them (inside fake_lib.standin)"""
    with recorder() as log:
        scenario(log)
        return json.loads(json.dumps(log))


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import fake_lib
    with tempfile.TemporaryDirectory() as tmp, fake_lib.standin(tmp, *SOURCES):
        out = {s.__name__: run(s) for s in SCENARIOS}
    with open(OUT, "w") as fh:      # one call per line
        fh.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(c) for c in v)) for k, v in out.items()) + "\n}\n")
    print("wrote", OUT, {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
