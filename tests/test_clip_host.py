"""Gradient clipping and Nesterov momentum WITHOUT a GPU: the numpy statement (tests/clip_reference.py) against hand-computed
values, msk_grad_clip_workspace of the built library (it needs no device), and the control flow of optimizer.Momentum / SGD /
Adam with grad_clip / use_nesterov through the real host stack over a stand-in library (tests/fake_msegk.c +
tests/fake_msegk_clip.c; numbers are garbage by construction, nothing numeric is asserted there)."""
import ctypes as C
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import clip_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NNUNET_YML = os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_nnunet_96.yml")


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def test_coefficient_is_one_until_the_clip_bites_and_rounded_once_when_it_does():
    g = np.array([3.0, 4.0, 0.0, 12.0], np.float32)                       # S = 169, norm = 13
    rec = R.record(g, 1.0, 13.0)
    assert rec.tolist() == [169.0, 13.0, 1.0, 0.0]                        # norm == c: exactly 1
    assert R.record(g, 1.0, 1e9)[2] == 1.0 and R.record(g, 1.0, np.inf)[2] == 1.0
    assert R.record(g, 0.5, 6.5).tolist() == [169.0, 6.5, 1.0, 0.0]       # grad_scale enters the norm
    rec = R.record(g, 1.0, 12.0)
    assert rec[1] == 13.0 and rec[2] == float(np.float32(12.0 / 13.0)) and rec[2] < 1.0
    rec = R.record(g, 1.0, 0.1)                                           # clip_norm enters as the float32 the kernel holds
    assert rec[2] == float(np.float32(np.float64(np.float32(0.1)) / 13.0))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            R.record(g, 1.0, bad)
    assert R.coef_of(np.inf, 12.0) == 0.0 and R.coef_of(np.nan, 12.0) == 1.0   # what the formulas say about inf / NaN gradients


def test_ordered_sum_of_squares_agrees_with_fsum():
    n = 1048581
    g = (np.random.default_rng(0).standard_normal(n) * 1e-3).astype(np.float32)
    exact = math.fsum((g.astype(np.float64) ** 2).tolist())
    assert abs(R.sumsq(g) - exact) <= 1e-12 * exact


def test_nesterov_and_clamp_steps_match_hand_computed_examples():
    p, v = R.sgd_step([1, 2, -1], [0.5, -1, 2], [0, 1, -1], lr=0.5, mu=0.5, wd=0.25, nesterov=True)
    # t = g + wd p = [0.75, -0.5, 1.75];  v = 0.5 v + t;  p -= 0.5 (t + 0.5 v)
    assert v.tolist() == [0.75, 0.0, 1.25] and p.tolist() == [0.4375, 2.25, -2.1875]
    p0, v0 = R.sgd_step([1, 2, -1], [0.5, -1, 2], [0, 1, -1], lr=0.5, mu=0.5, wd=0.25)
    assert v0.tolist() == v.tolist() and p0.tolist() == [0.625, 2.0, -1.625]
    # gs_eff = 0.5 * 0.5;  g' = [0.75, -1, 0.0625] clamped to +-0.5;  v = 0.5 * 2 + g'
    p, v = R.sgd_step([0, 0, 0], [3, -4, 0.25], [2, 2, 2], lr=1.0, mu=0.5, wd=0.0, grad_scale=0.5, coef=0.5, lo=-0.5, hi=0.5)
    assert v.tolist() == [1.5, 0.5, 1.0625] and p.tolist() == [-1.5, -0.5, -1.0625]
    assert R.clipped([np.nan, 1.0], 1.0, lo=-0.5, hi=0.5).tolist()[1] == 0.5 and np.isnan(R.clipped([np.nan], 1.0, lo=-1, hi=1))[0]


# ---- msk_grad_clip_workspace: the built library, no device -----------------------------------------------------------------------
def test_workspace_size_needs_no_gpu():
    path = os.environ.get("MSEGK_LIB") or os.path.join(ROOT, "medicalseg_amd", "lib", "libmsegk.so")
    assert os.path.exists(path), "run ./build.sh (or __graft_entry__.build()) first"
    fn = C.CDLL(path).msk_grad_clip_workspace
    fn.restype, fn.argtypes = C.c_int, [C.c_size_t, C.POINTER(C.c_size_t)]
    for count, want in ((1, 8), (4096, 8), (4097, 16), (45607944, 8 * 11135), (2 ** 31 - 1, 8 * 524288)):
        b = C.c_size_t(0)
        assert fn(count, C.byref(b)) == 0 and b.value == want, (count, b.value)
    b = C.c_size_t(77)
    assert fn(0, C.byref(b)) != 0 and fn(2 ** 31, C.byref(b)) != 0 and b.value == 77
    assert fn(1, None) != 0


# ---- control flow through the real host stack ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fake_pkg(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fake") / "libfake_msegk_clip.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-w", "-o", so, os.path.join(HERE, "fake_msegk.c"),
                           os.path.join(HERE, "fake_msegk_clip.c")])
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


@pytest.fixture
def calls(fake_pkg, monkeypatch):
    """names of the library calls made through Device.call, in order"""
    from medicalseg_amd.device import Device
    names = []
    real = Device.call

    def recording(self, name, *args):
        names.append(name)
        return real(self, name, *args)
    monkeypatch.setattr(Device, "call", recording)
    return names


NNUNET = dict(momentum=0.99, weight_decay=3e-5, use_nesterov=True, grad_clip={"type": "ClipGradByGlobalNorm", "clip_norm": 12})


def _model():
    from medicalseg_amd.models import VNet
    return VNet(num_classes=3)


def _clip_calls():
    from medicalseg_amd import _lib
    fn = _lib.load().fake_clip_calls
    fn.restype = C.c_long
    return [fn(i) for i in range(3)]


def test_options_are_honoured_without_a_warning_and_the_rest_still_warn(fake_pkg):
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    assert nn.ClipGradByGlobalNorm is optim.ClipGradByGlobalNorm and nn.ClipGradByValue is optim.ClipGradByValue
    assert nn.ClipGradByNorm is optim.ClipGradByNorm
    assert optim.OPTIMIZERS == ("Momentum", "SGD", "Adam")
    model = _model()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        opt = optim.Momentum(1e-3, parameters=model.parameters(), **NNUNET)
        optim.SGD(1e-3, parameters=model.parameters(), use_nesterov=True, grad_clip=nn.ClipGradByValue(0.5))
        adam = optim.Adam(1e-3, parameters=model.parameters(), grad_clip=nn.ClipGradByGlobalNorm(1.0))
    assert not w, [str(x.message) for x in w]
    assert opt.use_nesterov and isinstance(opt._clip.clip, optim.ClipGradByGlobalNorm) and opt._clip.clip.clip_norm == 12.0
    assert opt._clip.rec_ptr and opt._clip.ws_ptr and adam._clip.rec_ptr
    assert opt.grad_norm() is None and adam.grad_norm() is None               # no clipped step yet
    with pytest.warns(UserWarning, match=r"\['lazy_mode'\] are not implemented"):
        optim.Momentum(1e-3, parameters=model.parameters(), lazy_mode=True, **NNUNET)
    with pytest.warns(UserWarning, match=r"\['multi_precision'\] are not implemented"):
        optim.Adam(1e-3, parameters=model.parameters(), multi_precision=True)
    by_value = optim.Momentum(1e-3, parameters=model.parameters(), grad_clip=optim.ClipGradByValue(2.0, -1.0))
    assert (by_value._clip.lo, by_value._clip.hi) == (-1.0, 2.0) and by_value._clip.rec_ptr is None
    assert (optim.ClipGradByValue(3).min, optim.ClipGradByValue(3).max) == (-3.0, 3.0)
    for cls in (optim.Momentum, optim.SGD, optim.Adam):
        with pytest.raises(NotImplementedError, match="per-tensor"):
            cls(1e-3, parameters=model.parameters(), grad_clip=optim.ClipGradByNorm(1.0))
        with pytest.raises(NotImplementedError, match="per-tensor"):
            cls(1e-3, parameters=model.parameters(), grad_clip={"type": "ClipGradByNorm", "clip_norm": 1.0})
    with pytest.raises(ValueError):
        optim.Momentum(1e-3, parameters=model.parameters(), grad_clip={"type": "ClipByMagic"})
    with pytest.raises(ValueError):
        optim.ClipGradByGlobalNorm(0.0)
    with pytest.raises(TypeError):
        optim.Momentum(1e-3, parameters=model.parameters(), grad_clip=12)


def test_eager_mode_stays_off_and_plain_momentum_calls_what_it_called(fake_pkg, calls):
    from medicalseg_amd import optimizer as optim
    model = _model()
    plain = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    assert plain._clip is None and plain.use_nesterov is False                 # no record, no workspace
    assert plain.enable_eager(model) is True and plain.enable_eager(model, on=False) is False
    before = _clip_calls()
    del calls[:]
    plain.step()
    assert calls == ["msk_sgd_momentum"] and _clip_calls() == before
    plain_adam = optim.Adam(1e-3, parameters=model.parameters())
    del calls[:]
    plain_adam.step()
    assert calls == ["msk_adam"] and plain_adam._clip is None

    opt = optim.Momentum(1e-3, parameters=model.parameters(), **NNUNET)
    assert opt.enable_eager(model) is False and opt.enable_eager(model) is False and opt._eager is False
    assert not model._grad_ready_hooks or all(getattr(h, "__self__", None) is not opt for h in model._grad_ready_hooks)
    del calls[:]
    opt.step()
    assert calls == ["msk_grad_clip_coef", "msk_sgd_momentum_clip"]
    assert opt.grad_norm() == 0.0                                              # the stand-in leaves the zeroed record
    nest = optim.Momentum(1e-3, parameters=model.parameters(), use_nesterov=True)
    assert nest.enable_eager(model) is False
    del calls[:]
    nest.step()
    assert calls == ["msk_sgd_momentum_clip"] and nest.grad_norm() is None     # no global-norm clip: nothing is measured
    adam = optim.Adam(1e-3, parameters=model.parameters(), grad_clip=optim.ClipGradByGlobalNorm(1.0))
    del calls[:]
    adam.step()
    assert calls == ["msk_grad_clip_coef", "msk_adam_clip"] and abs(adam.beta1_pow - 0.81) < 1e-12
    assert [a - b for a, b in zip(_clip_calls(), before)] == [2, 2, 1]


def test_config_builds_the_nnunet_optimizer_and_train_runs_and_checkpoints(fake_pkg, calls, tmp_path):
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.core import train
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.utils import resume
    cfg = Config(NNUNET_YML)
    assert cfg.dic["optimizer"] == {"type": "sgd", "momentum": 0.99, "use_nesterov": True, "weight_decay": 3.0e-5,
                                    "grad_clip": {"type": "ClipGradByGlobalNorm", "clip_norm": 12}}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        opt = cfg.optimizer
    assert not [x for x in w if "IGNORED" in str(x.message)], [str(x.message) for x in w]
    assert type(opt) is optim.Momentum and opt.use_nesterov and opt.momentum == 0.99 and opt.weight_decay == 3.0e-5
    assert isinstance(opt._clip.clip, optim.ClipGradByGlobalNorm) and opt._clip.clip.clip_norm == 12.0
    # everything but the optimizer block is the affine-patch config
    base = Config(os.path.join(ROOT, "configs", "synthetic", "vnet_synthetic_ct_patch_affine_96.yml"))
    assert {k: v for k, v in cfg.dic.items() if k != "optimizer"} == {k: v for k, v in base.dic.items() if k != "optimizer"}

    model = cfg.model
    ds = SyntheticCT(num_samples=2, shape=(16, 16, 16), num_classes=3)
    del calls[:]
    train(model, ds, optimizer=opt, save_dir=str(tmp_path / "o"), iters=2, batch_size=1, save_interval=2, log_iters=1,
          losses=cfg.loss)
    assert opt._eager is False                                                 # train() asked; the optimizer declined
    assert calls.count("msk_grad_clip_coef") == 2 and calls.count("msk_sgd_momentum_clip") == 2
    assert not [c for c in calls if c in ("msk_sgd_momentum", "msk_sgd_momentum_eager", "msk_sgd_momentum_finish")]
    i = calls.index("msk_grad_clip_coef")
    assert calls[i + 1] == "msk_sgd_momentum_clip"
    assert os.path.exists(tmp_path / "o" / "iter_2" / "model.pdopt")
    sd = opt.state_dict()
    assert "in_tr.conv1.weight_velocity_0" in sd and not [k for k in sd if "clip" in k]
    plain = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.99)
    assert sorted(plain.state_dict()) == sorted(k for k in sd if k != "LR_Scheduler")   # state_dict is unchanged
    assert resume(model, opt, str(tmp_path / "o" / "iter_2")) == 2 and not opt.last_load["missing"]
