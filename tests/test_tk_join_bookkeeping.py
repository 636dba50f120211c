"""Host bookkeeping of the join backward taken along by out_tr.conv1's data gradient (nn.AddAct.backward_in_dgrad), WITHOUT a GPU:
the no-compute stand-in library of tests/test_host_dryrun.py plus an msk_conv3d_bwd_bnact_join that answers what the test chooses.
When the entry point reports the join consumed (0), the state AddAct.backward(share_b) would have left must be there when up_tr32's
backward starts, the join's own call must not run, and the join's output gradient must not exist; when it declines (1), and in the
nets that never ask it (ELU, VNetDeepSup), everything is as before."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (16, 16, 16)


@pytest.fixture(scope="module")
def fake_join_pkg(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fakejoin") / "libfake_msegk_join.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-w", "-o", so, os.path.join(HERE, "fake_msegk.c"),
                           os.path.join(HERE, "fake_msegk_join.c")])
    for m in [k for k in sys.modules if k.startswith("medicalseg_amd")]:
        del sys.modules[m]
    import importlib
    lib = importlib.import_module("medicalseg_amd._lib")
    real = lib.LIB_PATH
    lib.LIB_PATH = so
    lib._lib = None
    import medicalseg_amd
    from medicalseg_amd.device import Device
    Device._current = None
    yield medicalseg_amd
    lib.LIB_PATH = real
    lib._lib = None
    Device._current = None
    for m in [k for k in sys.modules if k.startswith("medicalseg_amd")]:
        del sys.modules[m]


class _Counted:
    """a library entry point that counts its calls"""

    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *args):
        self.n += 1
        return self.fn(*args)


def _step(model, rc):
    """forward + backward of one tiny step; returns what was seen when up_tr32's backward started, and the call counts"""
    from medicalseg_amd.device import get_device, to_tensor
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    dev = get_device()
    lib = dev.lib
    assert not getattr(lib.msk_conv3d_bwd_bnact_join, "missing", False)
    lib.fake_join_calls.restype = C.c_long
    lib.fake_join_set_rc(rc)
    model.train()
    logits = model(to_tensor(np.zeros((1, 1) + SHAPE, np.float32)))
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1] * len(logits)}
    if len(logits) > 1:
        losses["types"] = [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1]) for _ in logits]
        losses["coef"] = [1.0 / len(logits)] * len(logits)
    ll, _ = loss_computation(logits, to_tensor(np.zeros((1,) + SHAPE, np.int32)), losses)
    seen = {}
    up, real_backward = model.up_tr32, model.up_tr32.backward
    join = up._join

    def spy(dout):
        a, b, u = join.a, join.b, join.unit
        seen.update(dout=dout, feat_grad=model._feat.grad, a_written=a.grad_written, b_written=b.grad_written, a_grad=a.grad,
                    b_grad_from=b.grad_from, presummed=(getattr(u, "presummed", False), getattr(u, "presummed_pg", False)),
                    maxes=getattr(u, "presummed_maxes", None), bwd_done=getattr(join, "_bwd_done", False))
        return real_backward(dout)

    own = _Counted(lib.msk_add_act_join_bwd_pg)
    up.backward = spy
    lib.msk_add_act_join_bwd_pg = own
    try:
        sum(ll).backward()
    finally:
        del up.backward
        lib.msk_add_act_join_bwd_pg = own.fn
    return seen, int(lib.fake_join_calls()), own.n


def _joins_with_unit(model):
    return sum(1 for n in ("up_tr32", "up_tr64", "up_tr128", "up_tr256", "down_tr32", "down_tr64", "down_tr128", "down_tr256")
               if getattr(getattr(model, n)._join, "unit", None) is not None)


def test_consumed_join_leaves_what_its_own_backward_would(fake_join_pkg):
    from medicalseg_amd.models import VNet
    model = VNet(num_classes=3)
    seen, asked, own_calls = _step(model, rc=0)
    assert asked == 1
    assert seen["dout"] is None and seen["feat_grad"] is None         # the join's output gradient was never allocated
    assert seen["bwd_done"] and seen["a_written"] and seen["a_grad"] is not None
    assert seen["b_grad_from"] is seen["a_grad"] and not seen["b_written"]      # share_b: written once, b reads it from a.grad
    assert seen["presummed"] == (True, True) and seen["maxes"]
    n_unit = _joins_with_unit(model)
    assert n_unit >= 2 and own_calls == n_unit - 1                   # every other join ran its own call, up_tr32's did not
    assert not model.up_tr32._join._bwd_done                          # consumed: the next step starts clean
    # a second step on the same model goes the same way
    seen2, asked2, own2 = _step(model, rc=0)
    assert asked2 == 1 and seen2["feat_grad"] is None and own2 == own_calls


def test_declined_join_runs_as_before(fake_join_pkg):
    from medicalseg_amd.models import VNet
    model = VNet(num_classes=3)
    seen, asked, own_calls = _step(model, rc=1)
    assert asked == 1
    assert seen["dout"] is not None and seen["dout"] is seen["feat_grad"]
    assert not seen["bwd_done"] and not seen["a_written"] and seen["b_grad_from"] is None and seen["presummed"] == (False, False)
    assert own_calls == _joins_with_unit(model)
    ja, jb = model.up_tr32._join.a, model.up_tr32._join.b
    assert ja.grad_written and (jb.grad_written or jb.grad_from is not None)     # the join's own backward did the work


def test_elu_and_deep_supervision_never_ask(fake_join_pkg):
    from medicalseg_amd.models import VNet, VNetDeepSup
    seen, asked, own_calls = _step(VNet(elu=True, num_classes=3), rc=0)
    assert asked == 0 and own_calls == 0 and seen["dout"] is not None and not seen["bwd_done"]
    seen, asked, own_calls = _step(VNetDeepSup(num_classes=3), rc=0)
    assert asked == 0 and seen["dout"] is not None and not seen["bwd_done"]
