"""VNetDeepSup(native_heads=True) on the GPU: nnU-Net's deep supervision, every head scored at its own extent against the
nearest-neighbour down-sampled label (tests/pyramid_reference.py), nothing resized.

The oracle is oracle.vnet_numpy.VNetDeepSupOracle with the resize taken out (a subclass here; the oracle file is as it was).
Tolerances: those of tests/test_gpu_deepsup.py for the outputs, loss terms, gradients and the optimizer step (calibrated there
against the same oracle run in float32), those of tests/test_gpu_region_loss.py for DiceCELoss and its gradient.

The data of the whole-net gradient check.  PReLU's derivative jumps at 0, so a float32 evaluation cannot be held to the float64
oracle's branch at a voxel whose pre-activation lies within float32 rounding of 0, and in a small layer one voxel is a large
share of a weight gradient.  With the generator seed of tests/test_gpu_deepsup.py (5) the 32x32x12 configuration has such
voxels: in the float64 oracle a pre-activation of up_tr128.ops.1.relu1 (8x8x8, 512 voxels) is 2.27e-7 at rms 1.0 (2 float32
ulps), and one of up_tr64.relu2 is 3.6e-9.  Taking the other branch at the first of them IN THE ORACLE moves
up_tr128.ops.1.conv1.weight by 0.1018 of max|g| (relative L2 0.0074) -- the figures the device shows for that tensor at that
seed, to four digits, with the default and with the exact-fp32 convolution kernels alike (the up-sampling model at that seed:
0.0672, under the same bound of 0.1; profiles/r20_deepsup_native_gradient_kink.txt); every other tensor is far inside the
bounds.  This configuration's data is therefore drawn with seed 6, at which the float64 oracle's PReLUs over fewer than 4096
voxels keep their pre-activations at least 15 float32 ulps (of the tensor's rms) from 0; the 16^3 configuration keeps seed 5
(4 ulps).  Tolerances, configurations, reference and checks are untouched."""
import os
import warnings

import numpy as np
import pytest

import pyramid_reference as P
import region_reference as R
from helpers import dev, redzone_check, rel_err  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

from oracle import vnet_numpy as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SITES = [("down_tr128", 128), ("down_tr256", 256), ("up_tr256.x", 256), ("up_tr256.skip", 128),
         ("up_tr128.x", 256), ("up_tr128.skip", 64)]

# (input extent, classes, kernels, strides, batch, head extents h1 h2 h3): the two configurations of test_gpu_deepsup.py
CFGS = [
    ((16, 16, 16), 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4, 2, [(2, 2, 2), (4, 4, 4), (8, 8, 8)]),
    ((32, 32, 12), 5, ((2, 2, 4), (2, 2, 2), (2, 2, 2), (2, 2, 2)), ((2, 2, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2)), 1,
     [(4, 4, 4), (8, 8, 8), (16, 16, 9)]),
]
IDS = ["iso16", "mri32x32x12"]
SEEDS = {"iso16": 5, "mri32x32x12": 6}      # see the module docstring
NNUNET_COEF = [8 / 15, 1 / 15, 2 / 15, 4 / 15]
SMOOTH = float(np.float32(1e-5))


class NativeOracle(O.VNetDeepSupOracle):
    """the heads as their convolutions leave them"""

    def _resize(self, x, size):
        return x


def _l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _oracle(params, ncls, K, S, x, labels, masks, dtype):
    om = NativeOracle(params, 1, ncls, K, S, dtype=dtype)
    outs = om.forward(x, train=True, dropout_masks=masks)
    Ls = [O.MixedLossOracle(outer_coef=0.25, dtype=dtype) for _ in outs]
    res = [L(o, y) for L, o, y in zip(Ls, outs, labels)]
    return om, outs, res, om.backward([r[2] for r in res])


def _model(params, ncls, K, S, **kw):
    from medicalseg_amd.models import VNetDeepSup
    model = VNetDeepSup(elu=False, in_channels=1, num_classes=ncls, kernel_size=K, stride_size=S, **kw)
    missing, unexpected = model.set_state_dict(params)
    assert not missing and not unexpected
    return model


@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_native_forward_backward_step(cfg):
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    shape, ncls, K, S, N, heads = cfg
    rng = np.random.default_rng(SEEDS[IDS[CFGS.index(cfg)]])
    params = O.init_params_deepsup(4, 1, ncls, K, S)
    model = _model(params, ncls, K, S, native_heads=True)
    assert list(model.state_dict().keys()) == [n for n, _, _ in O.param_specs_deepsup(1, ncls, K, S)]
    x = rng.standard_normal((N, 1) + shape).astype(np.float32)
    y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
    labels = [y] + P.label_pyramid(y, heads)
    masks = {s: (rng.random((N, c)) < 0.5).astype(np.float32) * 2.0 for s, c in SITES}

    om, outs_ref, res_ref, g_ref = _oracle(params, ncls, K, S, x, labels, masks, np.float64)
    _, outs32, _, g32 = _oracle(params, ncls, K, S, x, labels, masks, np.float32)
    noise = {k: np.abs(g32[k] - g_ref[k]).max() / (np.abs(g_ref[k]).max() + 1e-30) for k in g_ref}
    noise_l2 = {k: _l2(g32[k], g_ref[k]) for k in g_ref}

    model.train()
    model.set_dropout_masks(masks)
    outs = model(x)
    assert len(outs) == 4
    assert [o.shape for o in outs] == [(N, ncls) + e for e in [shape] + heads]
    for o, ref, o32 in zip(outs, outs_ref, outs32):
        assert rel_err(o.numpy(), ref) < max(2e-4, 4 * rel_err(o32, ref))

    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1]) for _ in range(4)], "coef": [0.25] * 4}
    loss_list, per = loss_computation(outs, to_tensor(y), losses)
    assert len(loss_list) == 8
    for i, r in enumerate(res_ref):
        print("head %d: CE %.6f (oracle %.6f), Dice %.6f (oracle %.6f)" % (i, float(loss_list[2 * i]), r[0][0],
                                                                           float(loss_list[2 * i + 1]), r[0][1]))
        assert abs(float(loss_list[2 * i]) - r[0][0]) < 1e-4 * abs(r[0][0])
        assert abs(float(loss_list[2 * i + 1]) - r[0][1]) < 1e-4
    assert np.abs(np.asarray(per) - res_ref[-1][1]).max() < 1e-4  # the LAST output's dice: h3 at its own extent

    model.clear_gradients()
    sum(loss_list).backward()
    l2s = []
    frozen = {n for n, p in model.named_parameters() if getattr(p, "frozen", False)}
    assert frozen == {n for n in om.unused if not n.endswith(("._mean", "._variance"))}
    for name, p in model.named_parameters():
        if name in frozen:
            continue
        g, ref = p.grad_numpy(), g_ref[name]
        scale = np.abs(ref).max()
        if scale < 1e-9:
            assert np.abs(g).max() < 1e-4
            continue
        err, l2 = np.abs(g - ref).max() / scale, _l2(g, ref)
        l2s.append(l2)
        assert l2 < max(2e-2, 6 * noise_l2[name]), (name, l2, noise_l2[name])
        assert err < max(1e-1, 6 * noise[name]), (name, err, noise[name])
    assert float(np.median(l2s)) < max(3e-3, 3 * float(np.median(list(noise_l2.values()))))
    for head in ("out_tr64", "out_tr128", "out_tr256"):
        assert _l2(dict(model.named_parameters())[head + ".weight"].grad_numpy(), g_ref[head + ".weight"]) < \
            max(2e-3, 6 * noise_l2[head + ".weight"])

    before = {n: p.numpy() for n, p in model.named_parameters() if n in frozen}
    opt = optim.Momentum(learning_rate=1e-2, momentum=0.9, parameters=model.parameters(), weight_decay=1e-4)
    opt.step()
    vel = {}
    O.sgd_momentum_step(om.p, g_ref, vel, 1e-2, 0.9, 1e-4, names=om.trainable)
    after = dict(model.named_parameters())
    for n in frozen:
        assert np.array_equal(after[n].numpy().view(np.uint32), before[n].view(np.uint32)), n   # out_tr_all: bitwise unmoved
    for n in ("out_tr64.weight", "out_tr256.bias", "out_tr32.conv2.weight", "in_tr.conv1.weight"):
        assert np.abs(after[n].numpy() - om.p[n]).max() < 1e-4 * (np.abs(om.p[n]).max() + 1e-3), n
    dev().sync()


def _rel_ok(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.all(np.where(ref == 0, got == 0, np.abs(got - ref) <= tol * np.abs(ref))))


def _grad_ok(got, ref):
    """max-abs <= 2e-5 max|g| and relative L2 <= 1e-5 (tests/test_gpu_region_loss.py)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    if scale == 0:
        return not got.any()
    return np.abs(got - ref).max() <= 2e-5 * scale and np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref)


@pytest.mark.parametrize("cfg", CFGS, ids=IDS)
def test_dicece_on_every_head_against_the_pyramid_label(cfg):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import DiceCELoss
    from medicalseg_amd.utils import loss_computation
    shape, ncls, K, S, N, heads = cfg
    rng = np.random.default_rng(8)
    model = _model(O.init_params_deepsup(4, 1, ncls, K, S), ncls, K, S, native_heads=True)
    model.train()
    x = rng.standard_normal((N, 1) + shape).astype(np.float32)
    y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
    shell = np.ones(y.shape, bool)
    shell[:, 1:-1, 1:-1, 1:-1] = False
    y[shell] = 255                                         # what label_pad=255 leaves around a patch
    y[rng.random(y.shape) < 0.05] = 255                    # and some inside
    for e in heads:                                        # the voxel that every level's first voxel copies: each level holds some
        y[(slice(None),) + tuple(int(P.src_index(s, o)[0]) for s, o in zip(shape, e))] = 255
    labels = [y] + P.label_pyramid(y, heads)
    outs = model(x)
    loss_list, dice = loss_computation(outs, to_tensor(y), {"types": [DiceCELoss() for _ in range(4)], "coef": NNUNET_COEF})
    assert len(loss_list) == 4
    z = [o.numpy() for o in outs]
    sum(loss_list).backward()
    n_ignored = []
    for i, (o, lab, coef, term) in enumerate(zip(outs, labels, NNUNET_COEF, loss_list)):
        assert lab.shape == (N, o.d, o.h, o.w)
        ref = R.region_loss(z[i], lab, smooth=SMOOTH, lambda_f=1.0)
        got = o.grad.numpy()
        print("output %d %s: loss %.7f (statement %.7f), grad max-abs err %.2e of max|g|, %d voxels ignored" % (
            i, lab.shape, float(term) / coef, ref["loss"], np.abs(got - coef * ref["grad"]).max() / np.abs(coef * ref["grad"]).max(),
            int((lab == 255).sum())))
        assert _rel_ok(float(term), coef * ref["loss"]), (i, float(term), coef * ref["loss"])
        assert _grad_ok(got, coef * ref["grad"]), i
        ignored = np.moveaxis(got, 1, -1)[lab == 255]
        n_ignored.append(ignored.shape[0])
        assert not ignored.any(), i                        # exactly 0 under the mask of the head's own label
    assert _rel_ok(np.asarray(dice), R.region_loss(z[3], labels[3], smooth=SMOOTH, lambda_f=1.0)["dice"])
    assert all(k > 0 for k in n_ignored), n_ignored        # every head had voxels under the mask: the check above can fail


def test_the_switch_is_inert_when_off_and_eval_inference_is_the_same():
    from medicalseg_amd.core.infer import inference
    shape, ncls, K, S, N, heads = CFGS[0]
    rng = np.random.default_rng(13)
    params = O.init_params_deepsup(4, 1, ncls, K, S)
    x = rng.standard_normal((N, 1) + shape).astype(np.float32)
    off, default, native = (_model(params, ncls, K, S, native_heads=False), _model(params, ncls, K, S),
                            _model(params, ncls, K, S, native_heads=True))
    # eval mode first (a training forward moves the BatchNorm running statistics): one output from the native model, and
    # inference() returns the same bits through either
    res = []
    for m in (native, off):
        m.eval()
        res.append(len(m(x)))
        pred, logits = inference(m, x)
        res.append((pred.numpy().copy(), logits.numpy().view(np.uint32)))
    assert (res[0], res[2]) == (1, 4)
    assert np.array_equal(res[1][0], res[3][0]) and np.array_equal(res[1][1], res[3][1])
    got = []
    for m in (off, default):
        m.train()
        m.set_dropout_masks({})
        got.append([o.numpy().view(np.uint32) for o in m(x)])
    assert len(got[0]) == 4 and all(np.array_equal(a, b) for a, b in zip(*got))
    # ... and in training mode the native model's first output is the up-sampling model's, its heads the un-resized ones
    native.train()
    native.set_dropout_masks({})
    outs = native(x)
    assert np.array_equal(outs[0].numpy().view(np.uint32), got[1][0])
    assert [(o.d, o.h, o.w) for o in outs[1:]] == heads


def test_three_training_steps_from_the_nnunet_yaml():
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.core import evaluate
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd.models import DiceCELoss, VNetDeepSup
    from medicalseg_amd.utils import loss_computation
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # data_root warning
        cfg = Config(os.path.join(ROOT, "configs", "synthetic", "vnetdeepsup_synthetic_ct_patch_nnunet_96.yml"))
    cfg.dic["val_dataset"]["shape"] = [16, 16, 16]
    model, opt, losses = cfg.model, cfg.optimizer, cfg.loss
    assert isinstance(model, VNetDeepSup) and model.native_heads and isinstance(opt, optim.Momentum)
    assert [type(t) for t in losses["types"]] == [DiceCELoss] * 4 and np.allclose(losses["coef"], NNUNET_COEF)
    model.train()
    rng = np.random.default_rng(17)
    x = rng.standard_normal((2, 1, 16, 16, 16)).astype(np.float32)
    y = rng.integers(0, 3, (2, 16, 16, 16)).astype(np.int32)
    y[:, 0] = 255
    yt = to_tensor(y)
    watch = ["out_tr64.weight", "out_tr128.weight", "out_tr256.weight"]
    frozen = [n for n, p in model.named_parameters() if getattr(p, "frozen", False)]
    assert frozen and all(n.startswith("out_tr_all.") for n in frozen)
    start = {n: p.numpy() for n, p in model.named_parameters() if n in watch or n in frozen}
    values = []
    for _ in range(3):
        outs = model(x)
        loss_list, dice = loss_computation(outs, yt, losses)
        assert len(loss_list) == 4 and np.asarray(dice).shape == (3,)
        loss = sum(loss_list)
        loss.backward()
        opt.step()
        model.clear_gradients()
        values.append(float(loss))
    assert np.all(np.isfinite(values)), values
    after = dict(model.named_parameters())
    for n in watch:
        assert np.isfinite(after[n].numpy()).all() and not np.array_equal(after[n].numpy(), start[n]), n
    for n in frozen:
        assert np.array_equal(after[n].numpy().view(np.uint32), start[n].view(np.uint32)), n
    # validation reads the full-resolution output only: eval mode computes no head
    res = evaluate(model, cfg.val_dataset, losses, print_detail=False)
    assert np.isfinite(res["mdice"])
