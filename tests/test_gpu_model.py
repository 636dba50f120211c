"""Whole-network parity on the GPU: VNet forward, backward, loss and SGD trajectory vs the
numpy oracle (float64) on identical inputs/weights; preprocessing vs the reference goldens.

Tolerances: logits 2e-4 relative to max|logit|; parameter gradients 2e-3 relative to the
largest gradient entry of the tensor (fp32 conv chains of depth ~30 vs float64);
per-channel dice / mDice 1e-4 absolute (the north-star's "Dice within 1e-4")."""
import os

import numpy as np
import pytest

from helpers import dev, redzone_check, rel_err  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu

from oracle import preprocess_numpy as P  # noqa: E402
from oracle import vnet_numpy as O  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SITES = [("down_tr128", 128), ("down_tr256", 256), ("up_tr256.x", 256), ("up_tr256.skip", 128),
         ("up_tr128.x", 256), ("up_tr128.skip", 64)]


def _build(ncls, K, S, seed=1):
    from medicalseg_amd.models import VNet
    params = O.init_params(seed, 1, ncls, K, S)
    model = VNet(elu=False, in_channels=1, num_classes=ncls, kernel_size=K, stride_size=S)
    missing, unexpected = model.set_state_dict(params)
    assert not missing and not unexpected
    return model, params


def _masks(rng, N):
    return {s: (rng.random((N, c)) < 0.5).astype(np.float32) * 2.0 for s, c in SITES}


CFGS = [
    ((16, 16, 16), 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4, 2),
    ((32, 32, 12), 5, ((2, 2, 4), (2, 2, 2), (2, 2, 2), (2, 2, 2)), ((2, 2, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2)), 1),
]


def _oracle_run(params, ncls, K, S, x, y, train, masks, dtype):
    om = O.VNetOracle(params, 1, ncls, K, S, dtype=dtype)
    lg = om.forward(x, train=train, dropout_masks=masks)
    ol = O.MixedLossOracle(dtype=dtype)
    ll, per, dz = ol(lg, y)
    return om, lg, ll, per, om.backward(dz)


def _l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("mode", ["eval", "train_nodrop", "train_dropout"])
@pytest.mark.parametrize("cfg", CFGS)
def test_vnet_forward_backward_parity(cfg, mode, impl):
    """Whole-net forward/backward vs the float64 oracle.

    Two sources of legitimate fp32 deviation are calibrated, not hidden:
      * conditioning: at these test sizes the deep-level BN batches are 1^3..2^3 voxels x N,
        so some gradients are ill-conditioned in ANY fp32 implementation -- the same oracle
        run in float32 gives the per-tensor noise floor `noise`;
      * PReLU kink flips: a pre-activation within ~2e-6 of zero takes the other branch under
        a different fp32 summation order; one flip moves a few gradient entries by ~1%
        (verified: dy equals an exact host recomputation from the kernel's own inputs).
    Per tensor: relative-L2 error <= 2e-2 and max-abs error <= 1e-1 -- loose enough for a few
    flips (observed: up to 1.2e-2 even with the VALU reference kernels, impl=1, which share all
    Python wiring) and tight enough to catch any structural error (a missing/duplicated
    gradient term is O(1)); over all tensors the MEDIAN relative-L2 error must be <= 3e-3
    (observed 1e-6..1.4e-3).  Forward logits, both losses and per-class dice stay strict, and
    every kernel is checked tightly (1e-5 class) against the oracle in tests/test_gpu_ops.py."""
    shape, ncls, K, S, N = cfg
    train = mode != "eval"
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(0)
    dev().set_option("conv_impl", impl)
    try:
        model, params = _build(ncls, K, S)
        x = rng.standard_normal((N, 1) + shape).astype(np.float32)
        y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
        masks = _masks(rng, N) if mode == "train_dropout" else ({} if train else None)

        om, lg_ref, ll_ref, per_ref, g_ref = _oracle_run(params, ncls, K, S, x, y, train, masks, np.float64)
        _, lg32, _, _, g32 = _oracle_run(params, ncls, K, S, x, y, train, masks, np.float32)
        lg_noise = rel_err(lg32, lg_ref)
        noise = {k: np.abs(g32[k] - g_ref[k]).max() / (np.abs(g_ref[k]).max() + 1e-30) for k in g_ref}
        noise_l2 = {k: _l2(g32[k], g_ref[k]) for k in g_ref}

        model.train() if train else model.eval()
        model.set_dropout_masks(masks)
        logits = model(x)
        lg = logits[0].numpy()
        assert lg.shape == (N, ncls) + shape
        assert rel_err(lg, lg_ref) < max(2e-4, 4 * lg_noise)
        losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
        loss_list, per = loss_computation(logits, to_labels(y), losses)
        assert abs(float(loss_list[0]) - ll_ref[0]) < 1e-4 * abs(ll_ref[0])
        assert abs(float(loss_list[1]) - ll_ref[1]) < 1e-4
        assert np.abs(np.asarray(per) - per_ref).max() < 1e-4
        model.clear_gradients()
        sum(loss_list).backward()
        errs, l2s = [], []
        for name, p in model.named_parameters():
            g = p.grad_numpy()
            ref = g_ref[name]
            scale = np.abs(ref).max()
            if scale < 1e-9:  # conv bias ahead of a train-mode BN: exactly 0 in exact arithmetic
                assert np.abs(g).max() < 1e-4
                continue
            err, l2 = np.abs(g - ref).max() / scale, _l2(g, ref)
            errs.append(err)
            l2s.append(l2)
            assert l2 < max(2e-2, 6 * noise_l2[name]), (name, l2, noise_l2[name])
            assert err < max(1e-1, 6 * noise[name]), (name, err, noise[name])
        if train:  # running statistics moved like the oracle's
            sd = model.state_dict()
            for k in om.p:
                if k.endswith("._mean") or k.endswith("._variance"):
                    assert np.abs(sd[k] - om.p[k]).max() < 2e-4 * (1 + np.abs(om.p[k]).max()), k
        # the bulk of the tensors must agree tightly: flips touch only a few of them
        assert float(np.median(l2s)) < max(3e-3, 3 * float(np.median(list(noise_l2.values()))))
        print(mode, "impl", impl, "grad err: max-abs worst %.2e median %.2e | L2 worst %.2e median %.2e" %
              (max(errs), float(np.median(errs)), max(l2s), float(np.median(l2s))))
    finally:
        dev().set_option("conv_impl", 0)


def to_labels(y):
    from medicalseg_amd.device import to_tensor
    return to_tensor(y)


def test_training_trajectory_matches_oracle():
    """5 SGD steps (lr 1e-3 poly, momentum 0.9, L2 1e-4) in eval-mode BN like the reference's
    intended alignment test (vnet.py:351-397), plus 3 steps in train mode.  The float64 oracle
    is the reference; the float32 run of the oracle calibrates what fp32 can achieve."""
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    shape, ncls, K, S, N = CFGS[0]
    for train, steps in ((False, 5), (True, 3)):
        rng = np.random.default_rng(11)
        model, params = _build(ncls, K, S, seed=4)
        om = O.VNetOracle(params, 1, ncls, K, S)
        ol, vel = O.MixedLossOracle(), {}
        om32 = O.VNetOracle(params, 1, ncls, K, S, dtype=np.float32)
        ol32, vel32 = O.MixedLossOracle(dtype=np.float32), {}
        sched = optim.lr.PolynomialDecay(1e-3, decay_steps=100, end_lr=0, power=0.9)
        opt = optim.Momentum(sched, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
        model.train() if train else model.eval()
        for step in range(steps):
            x = rng.standard_normal((N, 1) + shape).astype(np.float32)
            y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
            masks = {} if train else None  # dropout off: keeps the 16^3 trajectory well conditioned
            ref_total, _, per_ref, _ = O.train_step(om, ol, vel, x, y, step, lr0=1e-3, decay_steps=100,
                                                    train=train, dropout_masks=masks)
            r32, _, _, _ = O.train_step(om32, ol32, vel32, x, y, step, lr0=1e-3, decay_steps=100,
                                        train=train, dropout_masks=masks)
            model.set_dropout_masks(masks)
            logits = model(x)
            loss_list, per = loss_computation(logits, to_labels(y), losses)
            loss = sum(loss_list)
            loss.backward()
            assert abs(opt.get_lr() - O.poly_lr(step, 1e-3, 100, 0.0, 0.9)) < 1e-12
            opt.step()
            sched.step()
            model.clear_gradients()
            tol = max(2e-6 * abs(ref_total), 4 * abs(r32 - ref_total))
            assert abs(float(loss) - ref_total) < tol, (train, step, float(loss), ref_total, r32)
            assert np.abs(np.asarray(per) - per_ref).max() < 1e-4
        sd = model.state_dict()
        for k in om.trainable:
            e = np.abs(sd[k] - om.p[k]).max()
            e32 = np.abs(om32.p[k].astype(np.float64) - om.p[k]).max()
            # absolute floor 1e-6: weights are O(1e-2), one fp32 ulp there is ~1e-9..4e-9 and the
            # update after a few steps is O(1e-5), so 1e-6 still pins the trajectory to ~1e-4 relative
            assert e <= 4 * e32 + 1e-6, (k, e, e32)


@pytest.mark.parametrize("shape", [(16, 16, 16), (32, 32, 32)])
def test_eager_optimizer_is_bitwise_the_plain_order(shape):
    """optimizer.Momentum.enable_eager (round 5): every block's update + weight re-pack runs on the weight-gradient stream as soon
    as that block's backward is enqueued, step() only joins.  Four training steps (train-mode BatchNorm, dropout masks from the
    device RNG) must leave EVERY parameter, velocity and BatchNorm buffer bitwise equal to the plain loss.backward();
    optimizer.step() order (core/train.py:139-140), and the loss of every step equal."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    ncls, K, S, N = 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4, 2
    results = []
    for eager in (False, True, "all"):
        rng = np.random.default_rng(5)
        nn.Dropout3D._site_counter = 0          # the mask stream is keyed by (seed, step, site): both models get sites 1..6
        model, _ = _build(ncls, K, S, seed=6)
        sched = optim.lr.PolynomialDecay(1e-2, decay_steps=100, end_lr=0, power=0.9)
        opt = optim.Momentum(sched, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        if eager:
            assert opt.enable_eager(model) is True
            if eager == "all":
                opt.eager_min_floats = 0        # every block updated as it reports (default: only the four blocks above 1 M parameters)
        losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
        model.train()
        model.set_dropout_masks(None)
        nn.Dropout3D.step, nn.Dropout3D.seed = 0, 3
        vals = []
        for step in range(4):
            x = rng.standard_normal((N, 1) + shape).astype(np.float32)
            y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
            logits = model(x)
            loss_list, per = loss_computation(logits, to_labels(y), losses)
            loss = sum(loss_list)
            loss.backward()
            if eager:
                assert len(opt._eager_done) == (10 if eager == "all" else 4)   # blocks updated during backward; the rest in step()
            opt.step()
            sched.step()
            model.clear_gradients()
            vals.append(float(loss))
        sd = model.state_dict()
        vel = dev().d2h(opt.velocity_ptr, (model.arena.count,), np.float32)
        results.append((vals, sd, vel))
    va, sda, vela = results[0]
    for vb, sdb, velb in results[1:]:
        assert va == vb, (va, vb)
        for k in sda:
            assert np.array_equal(sda[k], sdb[k]), k
        assert np.array_equal(vela, velb)
    assert np.abs(vela).max() > 0


# call counts of the weight-pack and absmax launches in the third training step of the 16^3 VNet below, as measured
# at commit 1a969f7 (deterministic: the comparison is exact)
PACK_LAUNCHES_STEP3 = {
    False: {"absmax": 10, "pack_weights_batch": 1, "pack_weights_foldn": 1, "pack_weights_tightk": 1, "pack_weights_wino": 4,
            "wbf_pack_absmax": 1, "wbf_pack_weights": 1},
    True: {"absmax": 10, "pack_weights_batch": 9, "pack_weights_foldn": 1, "pack_weights_tightk": 1, "pack_weights_wino": 4,
           "wbf_pack_absmax": 2, "wbf_pack_weights": 2},
}


@pytest.mark.parametrize("eager", [False, True])
def test_training_step_pack_launches_do_not_move(eager):
    """Where the packed weights are rebuilt is part of the step's launch plan: in steady state the optimizer kernels rebuild
    every row in use in batched launches and no convolution packs for itself.  Pins the call counts of every pack_weights*,
    wbf_pack_* and absmax* tag of the third step, for the plain and the eager optimizer order."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    ncls, K, S, N, shape = 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4, 2, (16, 16, 16)
    rng = np.random.default_rng(5)
    nn.Dropout3D._site_counter = 0
    model, _ = _build(ncls, K, S, seed=6)
    opt = optim.Momentum(1e-2, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
    if eager:
        assert opt.enable_eager(model) is True
        opt.eager_min_floats = 0
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    model.train()
    model.set_dropout_masks(None)
    nn.Dropout3D.step, nn.Dropout3D.seed = 0, 3
    d = dev()
    d.prof_reset()
    d.prof_enable(True)
    try:
        for step in range(3):
            if step == 2:
                d.prof_reset()
            x = rng.standard_normal((N, 1) + shape).astype(np.float32)
            y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
            loss_list, _ = loss_computation(model(x), to_labels(y), losses)
            sum(loss_list).backward()
            opt.step()
            model.clear_gradients()
        d.sync()
    finally:
        d.prof_enable(False)
    got = {t: c for t, (c, _) in d.prof_report().items() if t.startswith(("pack_weights", "wbf_pack_", "absmax"))}
    print("\npack launches of step 3, eager %s: %r" % (eager, dict(sorted(got.items()))))
    assert got == PACK_LAUNCHES_STEP3[eager]


def test_late_weight_gradient_does_not_see_the_updated_prelu_slopes():
    """Advisor, round 5: in_tr.conv1's weight gradient (the LAST kernel of the side stream) evaluates PReLU backward from the
    slopes of in_tr.relu1 -- a tensor of the parameter arena that the optimizer updates behind ev_late while that kernel is
    still running.  With a learning rate that moves the slopes by O(1) per step, a kernel that read them after the update
    would produce a visibly different conv1 gradient; it reads a snapshot taken before ev_late, so two steps in the eager /
    late-split order leave in_tr bitwise equal to the plain order (full join before one update).  64^3: the late kernel runs
    for longer than the update that follows ev_late, so the two do overlap."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    ncls, K, S, shape = 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4, (64, 64, 64)
    results = []
    for eager in (False, True, True):
        rng = np.random.default_rng(11)
        nn.Dropout3D._site_counter = 0
        model, _ = _build(ncls, K, S, seed=6)
        opt = optim.Momentum(0.5, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        if eager:
            assert opt.enable_eager(model) is True
        losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
        model.train()
        model.set_dropout_masks({})
        x = rng.standard_normal((1, 1) + shape).astype(np.float32)
        y = rng.integers(0, ncls, (1,) + shape).astype(np.int32)
        a0 = model.state_dict()["in_tr.relu1._weight"].copy()
        for step in range(2):
            logits = model(x)
            loss_list, per = loss_computation(logits, to_labels(y), losses)
            sum(loss_list).backward()
            opt.step()
            model.clear_gradients()
        sd = model.state_dict()
        results.append({k: v for k, v in sd.items() if k.startswith("in_tr.")})
        assert np.abs(sd["in_tr.relu1._weight"] - a0).max() > 1e-3      # the slopes DID move by something a gradient would show
    for other in results[1:]:
        for k in results[0]:
            assert np.array_equal(results[0][k], other[k]), k


@pytest.mark.parametrize("shape,N", [((64, 64, 64), 2), ((32, 32, 32), 1)])
def test_shared_join_gradient_is_bitwise_the_two_writes(shape, N):
    """Round 6: a residual join (vnet.py:110-111,154) hands d(a + b) to both operands.  nn.AddAct.backward(share_b=True) writes it
    ONCE and the LUConv behind the join reads it as the old values of its accumulating data gradient (msk_conv3d_bwd_bnact_acc:
    one-kernel epilogue at 64^3 -- incl. the dense-halves store behind the 16 + 16 concat -- and wbf_tout_k / the copy fall-back at
    32^3).  Same additions in the same order: every parameter gradient of a training step must equal the two-writes form bit for
    bit, with dropout on (the dropout levels keep the two writes) and off."""
    from medicalseg_amd import nn
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    ncls, K, S = 3, ((2, 2, 2),) * 4, ((2, 2, 2),) * 4
    rng = np.random.default_rng(21)
    x = rng.standard_normal((N, 1) + shape).astype(np.float32)
    y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
    masks = _masks(rng, N)
    saved = nn.SHARE_JOIN_GRAD
    results = []
    try:
        for share in (False, True):
            nn.SHARE_JOIN_GRAD = share
            for mk in ({}, masks):
                model, _ = _build(ncls, K, S, seed=8)
                model.train()
                model.set_dropout_masks(mk)
                losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
                ll, _ = loss_computation(model(x), to_labels(y), losses)
                model.clear_gradients()
                sum(ll).backward()
                results.append({n_: p.grad_numpy().copy() for n_, p in model.named_parameters()})
    finally:
        nn.SHARE_JOIN_GRAD = saved
    for a_, b_ in ((results[0], results[2]), (results[1], results[3])):
        for k in a_:
            assert np.array_equal(a_[k], b_[k]), k
    assert any(np.abs(v).max() > 0 for v in results[2].values())


def test_eval_mdice_matches_oracle():
    """core.val.evaluate's mDice on a synthetic validation set == oracle soft dice."""
    from medicalseg_amd.core import evaluate
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    shape, ncls, K, S, _ = CFGS[0]
    model, params = _build(ncls, K, S, seed=2)
    ds = SyntheticCT(num_samples=3, shape=shape, num_classes=ncls, mode="val")
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    res = evaluate(model, ds, losses, print_detail=False)
    om = O.VNetOracle(params, 1, ncls, K, S)
    md = 0.0
    for i in range(3):
        im, lab, _ = ds[i]
        lg = om.forward(im[None], train=False, record=False)
        _, per, _ = O.dice(lg, lab[None])
        md += per.mean()
    assert abs(res["mdice"] - md / 3) < 1e-4


def test_eval_auc_roc_matches_numpy_restatement():
    """evaluate(auc_roc=True) (core/val.py:121-131,174): device softmax of the logits of every validation volume, collected
    on the host, one-vs-rest macro AUC -- against the float64 oracle's logits -> numpy softmax -> sklearn's roc_auc_score
    (what the reference's utils/metric.py:102-105 calls; its 4-D shape check is the only thing not reproduced)."""
    skm = pytest.importorskip("sklearn.metrics")
    from medicalseg_amd.core import evaluate
    from medicalseg_amd.datasets import SyntheticCT
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    shape, ncls, K, S, _ = CFGS[0]
    model, params = _build(ncls, K, S, seed=2)
    ds = SyntheticCT(num_samples=3, shape=shape, num_classes=ncls, mode="val")
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    res = evaluate(model, ds, losses, print_detail=False, auc_roc=True)
    om = O.VNetOracle(params, 1, ncls, K, S)
    scores, labs = [], []
    for i in range(3):
        im, lab, _ = ds[i]
        lg = om.forward(im[None], train=False, record=False)
        scores.append(np.moveaxis(O.softmax(lg, axis=1), 1, -1).reshape(-1, ncls))
        labs.append(np.asarray(lab).reshape(-1))
    ref = skm.roc_auc_score(np.concatenate(labs), np.concatenate(scores), multi_class="ovr")
    print("auc_roc %.6f (oracle + sklearn %.6f), mdice %.4f" % (res["auc_roc"], ref, res["mdice"]))
    assert abs(res["auc_roc"] - ref) < 1e-4 and 0.0 <= res["auc_roc"] <= 1.0


def test_preprocess_matches_reference_goldens():
    from medicalseg_amd import preprocess as pp
    g = np.load(os.path.join(HERE, "golden", "preprocess_golden.npz"))
    for i in range(5):
        o1, sp = pp.resample(g[f"rs{i}_img"], spacing=[0.7, 0.8, 2.5], new_shape=list(g[f"rs{i}_shape"]), order=1)
        assert o1.dtype == np.float32
        assert np.abs(o1 - g[f"rs{i}_o1"]).max() <= 1e-6 * np.abs(g[f"rs{i}_o1"]).max() + 1e-6
        assert np.allclose(sp, g[f"rs{i}_spacing"])
        o0, _ = pp.resample(g[f"rs{i}_lab"], new_shape=list(g[f"rs{i}_shape"]), order=0)
        assert o0.dtype == np.int32 and np.array_equal(o0, g[f"rs{i}_o0"])       # bit exact (index work)
        of0, _ = pp.resample(g[f"rs{i}_img"], new_shape=list(g[f"rs{i}_shape"]), order=0)
        assert np.array_equal(of0, g[f"rs{i}_of0"])
    _, sp4 = pp.resample(np.zeros((8, 8, 8), np.float32), spacing=[9.0, 1.0, 2.0, 3.0], new_shape=[4, 4, 4])
    assert np.allclose(sp4, g["rs_sp4"])
    assert np.array_equal(pp.HUnorm(g["hu_in"].reshape(1, 3, 3)).ravel(), g["hu_out"])
    assert np.array_equal(pp.HUnorm(g["hu_vol_in"]), g["hu_vol_out"])
    assert np.array_equal(pp.HUnorm(g["hu_vol_in"], -1000, 400, -1500), g["hu_vol_out_custom"])
    assert np.array_equal(pp.normalize(g["nm_in"]), g["nm_out_auto"])
    assert np.array_equal(pp.normalize(g["nm_in"], 0, 2650), g["nm_out_bounds"])
    assert np.array_equal(pp.label_remap(g["lr_in"], {1: 0, 2: 1, 3: 1, 5: 2}), g["lr_out"])
    assert np.array_equal(pp.label_remap(g["lr_in"], {1: 2, 2: 3}), g["lr_out_chain"])
    ct, _ = pp.resample(pp.HUnorm(g["pipe_ct_in"]), new_shape=[16, 16, 16], order=1)
    assert np.abs(ct - g["pipe_ct_out"]).max() < 2e-5 * 255
    mr, _ = pp.resample(pp.normalize(g["pipe_mr_in"], 0, 2650), new_shape=[16, 16, 6], order=1)
    assert np.abs(mr - g["pipe_mr_out"]).max() < 2e-6
    v = g["nm_in"]
    assert np.array_equal(pp.max_normalize(v), P.max_normalize(v).astype(np.float32))


def test_preprocess_size_independent_properties():
    """Full-size (512x512x64 -> 128^3) checks that need no oracle run: identity resample,
    constant volumes stay constant, order-0 output values are a subset of the input's."""
    from medicalseg_amd import preprocess as pp
    rng = np.random.default_rng(2)
    v = rng.standard_normal((64, 96, 80)).astype(np.float32)
    same, _ = pp.resample(v, new_shape=list(v.shape), order=1)
    assert np.array_equal(same, v)
    big = np.full((128, 256, 64), 3.25, np.float32)
    out, _ = pp.resample(big, new_shape=[128, 128, 128], order=1)
    assert np.all(out == 3.25)
    lab = rng.integers(0, 20, (100, 120, 12)).astype(np.int32)
    o, _ = pp.resample(lab, new_shape=[64, 64, 12], order=0)
    assert set(np.unique(o)) <= set(np.unique(lab))
    # corners are preserved by the align-corner map
    assert o[0, 0, 0] == lab[0, 0, 0] and o[-1, -1, -1] == lab[-1, -1, -1]


def test_in_loop_device_preprocessing_feeds_the_model():
    """BASELINE configs[4] flow: raw MRI slab -> pinned H2D -> normalize(0,2650) -> resample(order 1)
    -> max-normalise on the device -> VNet (20 classes, anisotropic kernels), no host round trip;
    values equal the oracle's preprocessing, logits equal a forward on the oracle-preprocessed input."""
    from medicalseg_amd.models import VNet
    from medicalseg_amd.preprocess import DevicePipeline
    rng = np.random.default_rng(3)
    raw = (rng.random((60, 60, 12)) * 2650).astype(np.float32)
    raw_lab = rng.integers(0, 20, (60, 60, 12)).astype(np.int32)
    pipe = DevicePipeline()
    chain = pipe.image(raw).normalize(0, 2650).resample([32, 32, 12], 1).max_normalize()
    lab = pipe.label(raw_lab).resample([32, 32, 12], 0)
    ref, _ = P.resample(P.normalize(raw.copy(), 0, 2650), [32, 32, 12], 1)
    ref = P.max_normalize(ref)[None].astype(np.float32)
    assert np.abs(chain.numpy() - ref[0, 0]).max() < 2e-6
    assert np.array_equal(lab.numpy(), P.resample(raw_lab, [32, 32, 12], 0)[0])
    K = [[2, 2, 4], [2, 2, 2], [2, 2, 2], [2, 2, 2]]
    S = [[2, 2, 1], [2, 2, 1], [2, 2, 2], [2, 2, 2]]
    model = VNet(num_classes=20, kernel_size=K, stride_size=S)
    model.eval()
    a = model(chain.tensor())[0].numpy()
    b = model(ref)[0].numpy()
    assert a.shape == (1, 20, 32, 32, 12) and rel_err(a, b) < 1e-5
    assert lab.int_tensor().shape == (1, 32, 32, 12)


def test_checkpoint_resume_continues_bitwise(tmp_path):
    """SURVEY 8 f2 (core/train.py:230-254, utils/utils.py:115-135): iter_N/model.pdparams +
    model.pdopt written through utils.save, loaded by utils.resume into a FRESH model/optimizer;
    the continued trajectory must equal the uninterrupted one bit for bit (weights, BN buffers,
    velocity and the LR-scheduler position all travel)."""
    import pickle

    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation, resume, save
    shape, ncls, N = (16, 16, 16), 3, 2
    rng = np.random.default_rng(11)
    xs = [rng.standard_normal((N, 1) + shape).astype(np.float32) for _ in range(4)]
    ys = [rng.integers(0, ncls, (N,) + shape).astype(np.int32) for _ in range(4)]
    w = [1.0, 2.0, 0.5]  # explicit CE weights: the cached first-batch weights are not checkpointed (F8)

    def make():
        nn.seed(3)
        model = VNet(num_classes=ncls)
        model.train()
        model.set_dropout_masks({})  # dropout RNG state is not checkpointed either
        sched = optim.lr.PolynomialDecay(1e-2, decay_steps=10, end_lr=0, power=0.9)
        opt = optim.Momentum(sched, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        losses = {"types": [MixedLoss([CrossEntropyLoss(weight=w), DiceLoss()], [1, 1])], "coef": [1]}
        return model, opt, sched, losses

    def step(model, opt, sched, losses, i):
        ll, _ = loss_computation(model(xs[i]), to_labels(ys[i]), losses)
        sum(ll).backward()
        opt.step()
        sched.step()
        model.clear_gradients()

    model, opt, sched, losses = make()
    for i in range(2):
        step(model, opt, sched, losses, i)
    ck = tmp_path / "iter_2"
    save(model.state_dict(), str(ck / "model.pdparams"))
    save(opt.state_dict(), str(ck / "model.pdopt"))
    for i in range(2, 4):
        step(model, opt, sched, losses, i)
    ref_sd, ref_opt = model.state_dict(), opt.state_dict()

    # the files are plain pickles of {name: ndarray} with the reference's key names
    sd = pickle.load(open(ck / "model.pdparams", "rb"))
    assert list(sd.keys()) == [n for n, _, _ in O.param_specs(1, ncls)]
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in sd.values())
    od = pickle.load(open(ck / "model.pdopt", "rb"))
    assert "in_tr.conv1.weight_velocity_0" in od and "LR_Scheduler" in od

    model2, opt2, sched2, losses2 = make()
    # a paddle-written file also carries this name table; it must be ignored
    sd["StructuredToParameterName@@"] = {k: "param_%d" % i for i, k in enumerate(sd)}
    save(sd, str(ck / "model.pdparams"))
    assert resume(model2, opt2, str(ck)) == 2
    assert sched2.last_epoch == sched.last_epoch - 2
    for i in range(2, 4):
        step(model2, opt2, sched2, losses2, i)
    sd2, opt_sd2 = model2.state_dict(), opt2.state_dict()
    for k in ref_sd:
        assert np.array_equal(ref_sd[k], sd2[k]), k
    for k in ref_opt:
        if k != "LR_Scheduler":
            assert np.array_equal(ref_opt[k], opt_sd2[k]), k
    assert ref_opt["LR_Scheduler"] == opt_sd2["LR_Scheduler"]


def test_resume_from_a_paddle_written_optimizer_state(tmp_path):
    """SURVEY 8 f2 / round-5 verdict item 8 (reference utils/utils.py:115-135 loads model.pdparams AND model.pdopt): a model.pdopt
    written by Paddle names its accumulators after Paddle's INTERNAL parameter names (`conv3d_0.w_0_velocity_0`); the table
    `StructuredToParameterName@@` inside the sibling model.pdparams maps the structured names onto them.  A fabricated pair in that
    naming must resume with its momentum: the continued trajectory equals the uninterrupted one bit for bit."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation, resume, save
    shape, ncls, N = (16, 16, 16), 3, 1
    rng = np.random.default_rng(12)
    xs = [rng.standard_normal((N, 1) + shape).astype(np.float32) for _ in range(3)]
    ys = [rng.integers(0, ncls, (N,) + shape).astype(np.int32) for _ in range(3)]

    def make():
        nn.seed(4)
        model = VNet(num_classes=ncls)
        model.train()
        model.set_dropout_masks({})
        opt = optim.Momentum(1e-2, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        losses = {"types": [MixedLoss([CrossEntropyLoss(weight=[1.0, 2.0, 0.5]), DiceLoss()], [1, 1])], "coef": [1]}
        return model, opt, losses

    def step(model, opt, losses, i):
        ll, _ = loss_computation(model(xs[i]), to_labels(ys[i]), losses)
        sum(ll).backward()
        opt.step()
        model.clear_gradients()

    model, opt, losses = make()
    step(model, opt, losses, 0)
    sd, od = model.state_dict(), opt.state_dict()
    # Paddle's naming: parameters conv3d_<i>.w_0 / .b_0, batch_norm3d_<i>.w_0 ..., accumulators <internal>_velocity_0
    table, kinds = {}, {}
    trainable = {p.name for p in model.arena.params}
    for k in sd:
        if k not in trainable:
            continue
        layer = k.rsplit(".", 1)[0]
        kinds.setdefault(layer, len(kinds))
        table[k] = "layer_%d.%s_0" % (kinds[layer], "w" if k.endswith(("weight", "_weight")) else "b")
    assert len(set(table.values())) == len(table)
    paddle_opt = {table[k[:-len("_velocity_0")]] + "_velocity_0": v for k, v in od.items() if k.endswith("_velocity_0")}
    assert len(paddle_opt) == len(table) and not any(k in od for k in paddle_opt)     # none of the keys is one of ours
    paddle_opt["LR_Scheduler"] = {"last_epoch": 1, "last_lr": 1e-2}
    ck = tmp_path / "iter_1"
    save(dict(sd, **{"StructuredToParameterName@@": table}), str(ck / "model.pdparams"))
    save(paddle_opt, str(ck / "model.pdopt"))
    for i in (1, 2):
        step(model, opt, losses, i)
    ref = model.state_dict()

    model2, opt2, losses2 = make()
    assert resume(model2, opt2, str(ck)) == 1
    assert opt2.last_load["missing"] == [] and opt2.last_load["unexpected"] == []
    vel = dev().d2h(opt2.velocity_ptr, (model2.arena.count,), np.float32)
    assert np.abs(vel).max() > 0                                     # the momentum DID arrive
    for i in (1, 2):
        step(model2, opt2, losses2, i)
    got = model2.state_dict()
    for k in ref:
        assert np.array_equal(ref[k], got[k]), k
    # without the table the same file is reported as foreign (momentum restarts): nothing is skipped silently
    model3, opt3, _ = make()
    opt3.set_state_dict(paddle_opt)
    assert len(opt3.last_load["missing"]) == len(table) and len(opt3.last_load["unexpected"]) == len(table)


def test_winograd_and_direct_kernels_agree_on_a_training_step():
    """The product dispatch uses the Winograd F(4,5) / F(2,5) kernels for the 5^3 layers; `direct_conv` (env
    MSEGK_DIRECT_CONV=1) selects the direct kernels (exact fp32 fmaf chains).  One training step at 32^3 (every level
    down to 8^3 tiles for a Winograd kernel) must agree between the two: logits 2e-5 of max|logit|, loss 1e-5,
    updated weights 1e-5 of their scale."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(21)
    x = rng.standard_normal((2, 1, 32, 32, 32)).astype(np.float32)
    y = rng.integers(0, 3, (2, 32, 32, 32)).astype(np.int32)
    out = []
    for direct in (0, 1):
        dev().set_option("direct_conv", direct)
        try:
            nn.seed(5)
            model = VNet(num_classes=3)
            model.train()
            model.set_dropout_masks({})
            opt = optim.Momentum(1e-2, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
            losses = {"types": [MixedLoss([CrossEntropyLoss(weight=[1.0, 1.0, 1.0]), DiceLoss()], [1, 1])], "coef": [1]}
            dev().prof_reset()
            dev().prof_enable(True)
            logits = model(x)
            lg = logits[0].numpy()
            ll, _ = loss_computation(logits, to_labels(y), losses)
            loss = float(sum(ll))
            sum(ll).backward()
            opt.step()
            dev().prof_enable(False)
            tags = dev().prof_report()
            ran_wino = any(k.startswith(("conv_halo_wino", "wgrad_wino", "wbf_")) for k in tags)
            assert ran_wino == (direct == 0), sorted(tags)
            sd = model.state_dict()
            out.append((lg, loss, sd["up_tr32.ops.0.conv1.weight"], sd["down_tr64.ops.1.conv1.weight"], sd["in_tr.conv1.weight"]))
        finally:
            dev().prof_enable(False)
            dev().set_option("direct_conv", 0)
    (lg_w, loss_w, *w_w), (lg_d, loss_d, *w_d) = out
    assert rel_err(lg_w, lg_d) < 2e-5
    assert abs(loss_w - loss_d) < 1e-5 * abs(loss_d)
    for a, b in zip(w_w, w_d):
        assert np.abs(a - b).max() < 1e-5 * np.abs(b).max()


@pytest.mark.parametrize("model_name", ["VNet", "VNetDeepSup"])
def test_fused_inference_matches_eval_forward(model_name):
    """inside nn.fused_inference() the eval-mode net runs conv+BN+PReLU units as single folded
    convolutions.  Logits agree with the unfused eval forward (2e-5 of max|logit|), the argmax map agrees except
    at numerical ties, evaluate() -- which uses the fused path -- returns the unfused mDice, a later change of
    the parameters is picked up by the next scope, and backward through a fused forward is refused."""
    from medicalseg_amd import models, nn
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor
    rng = np.random.default_rng(5)
    model = getattr(models, model_name)(num_classes=3)
    state = model.state_dict()
    for k_, v in state.items():                      # non-trivial running statistics and slopes
        if k_.endswith("._mean"):
            state[k_] = rng.standard_normal(v.shape).astype(np.float32) * 0.1
        elif k_.endswith("._variance"):
            state[k_] = rng.uniform(0.5, 1.5, v.shape).astype(np.float32)
        elif "relu" in k_ and k_.endswith("_weight"):
            state[k_] = rng.uniform(0.1, 0.4, v.shape).astype(np.float32)
    model.set_state_dict(state)
    model.eval()
    x = rng.standard_normal((1, 1, 32, 32, 32)).astype(np.float32)
    plain = model(to_tensor(x))[0].numpy()
    with nn.fused_inference():
        outs = model(to_tensor(x))
        fused = outs[0].numpy()
        with pytest.raises(RuntimeError, match="fused_inference"):
            model.backward(outs[0] if model_name == "VNet" else list(outs))
    scale = np.abs(plain).max()
    assert np.abs(fused - plain).max() <= 2e-5 * scale, np.abs(fused - plain).max() / scale
    pred, logit = infer.inference(model, to_tensor(x))
    assert np.array_equal(logit.numpy(), fused)                       # inference() takes the fused path itself
    top2 = np.sort(plain, axis=1)
    clear = (top2[:, -1] - top2[:, -2]) > 1e-4 * scale
    assert np.array_equal(pred.numpy()[:, 0][clear], plain.argmax(1)[clear])
    # a parameter change between scopes is seen (weights are refolded per scope)
    state["in_tr.bn1._mean"] = state["in_tr.bn1._mean"] + 0.5
    name = [k_ for k_ in state if k_.endswith("ops.0.bn1._mean")][0]
    state[name] = state[name] + 0.5
    model.set_state_dict(state)
    plain2 = model(to_tensor(x))[0].numpy()
    with nn.fused_inference():
        fused2 = model(to_tensor(x))[0].numpy()
    assert np.abs(plain2 - plain).max() > 1e-3 * scale
    assert np.abs(fused2 - plain2).max() <= 2e-5 * np.abs(plain2).max()


def test_vnet_32cube_batch2_gradients_calibrated():
    """Whole-net forward / backward at 32^3, batch 2 (every BatchNorm layer sees >= 16 values per channel) against the
    float64 oracle, with the three kernel sets on identical weights and data.

    Forward quantities are strict: logits 2e-5 of max|logit| (measured 2.7e-6), losses 2e-5, per-class dice 1e-5.
    Gradients: this network amplifies per-layer rounding about 1000x on the way back (BatchNorm backward subtracts two
    projections; the surviving signal is small) -- the float64 oracle re-run in FLOAT32 is itself 7.7e-4 (median
    per-tensor rel-L2) away from float64, and the exact-fp32 direct kernels 4.9e-4 / 5.7e-3 (median / worst tensor).  A
    per-tensor bound of 1e-3 is therefore not attainable by any fp32 implementation; what is asserted:
      * every tensor rel-L2 <= 8e-3, median <= 4e-3 for the product kernels (round 3, scaled low pieces: 1.2e-3 median / 1.6e-3 worst; round 2: 3.0e-3 median /
        4.1e-3 ... 6.5e-3 worst), median <= 5e-3 for the two A/B kernel sets;
      * NO ranking between the kernel sets: the medians are noise realisations -- the exact-fp32 Winograd set measured
        6.1e-3 / 8.8e-3 and later 1.6e-3 when only the summation order of the FIRST layer's kernel changed
        (conv_c1_mfma_k), with its own kernels untouched;
    a structural error (missing term, wrong scale) is O(1) and a 1 % systematic error doubles the worst tensor;
      * (round 3) the SYSTEMATIC part separately: the least-squares scale of every weight tensor's gradient against the
        oracle's is within 1e-3 of one (measured <= 2e-4) -- rounding noise projects out, a wrong factor does not."""
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    shape, ncls, N = (32, 32, 32), 3, 2
    K = S = ((2, 2, 2),) * 4
    rng = np.random.default_rng(4)
    x = rng.standard_normal((N, 1) + shape).astype(np.float32)
    y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
    params = O.init_params(2, 1, ncls, K, S)
    om, lg_ref, ll_ref, per_ref, g_ref = _oracle_run(params, ncls, K, S, x, y, True, {}, np.float64)
    d = dev()
    stats = {}
    for tag, opts in (("product", {}), ("fp32_wino", {"wino_bf3": 0}), ("fp32_direct", {"direct_conv": 1})):
        for k_, v_ in opts.items():
            d.set_option(k_, v_)
        try:
            model, _ = _build(ncls, K, S, seed=2)
            model.train()
            model.set_dropout_masks({})
            d.prof_reset()
            d.set_option("prof_only_halo", 0)
            d.prof_enable(True)
            logits = model(x)
            lg = logits[0].numpy()
            losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
            loss_list, per = loss_computation(logits, to_labels(y), losses)
            model.clear_gradients()
            sum(loss_list).backward()
            d.sync()
            d.prof_enable(False)
            tags = d.prof_report()
            ran_wbf = (any(k.startswith(("wbf_gemm_k", "wbf_gemm_h2_k")) for k in tags)
                       and any(k.startswith(("wbf_wgrad_k", "wbf_wgrad_h2_k")) for k in tags))
            assert ran_wbf == (tag == "product"), sorted(tags)
            e_lg = rel_err(lg, lg_ref)
            assert e_lg < 2e-5, (tag, e_lg)
            assert abs(float(loss_list[0]) - ll_ref[0]) < 2e-5 * abs(ll_ref[0])
            assert abs(float(loss_list[1]) - ll_ref[1]) < 2e-5
            assert np.abs(np.asarray(per) - per_ref).max() < 1e-5
            l2s, bias = {}, {}
            for name, p in model.named_parameters():
                ref = g_ref[name]
                if np.abs(ref).max() < 1e-9:   # conv bias ahead of a train-mode BN: exactly 0 in exact arithmetic
                    assert np.abs(p.grad_numpy()).max() < 1e-4
                    continue
                g = p.grad_numpy().astype(np.float64)
                l2s[name] = _l2(g, ref)
                # SYSTEMATIC part of the error: the least-squares scale of g against the oracle, minus one.  Rounding noise
                # is (nearly) orthogonal to the reference and averages out in this projection -- for a tensor of n values it
                # is ~ rel-L2 / sqrt(n) --, a wrong factor in some kernel (a 1 % error in one layer's weight gradient, which
                # the rel-L2 bound alone would let pass) shows at full size.
                if ref.size >= 1000:
                    bias[name] = float(np.vdot(g, ref) / np.vdot(ref, ref) - 1.0)
            worst = max(l2s, key=l2s.get)
            wb = max(bias, key=lambda k_: abs(bias[k_]))
            stats[tag] = (float(np.median(list(l2s.values()))), l2s[worst], abs(bias[wb]))
            print("32^3 N=2 %-11s logits %.2e | gradient rel-L2 median %.2e worst %.2e (%s) | worst scale bias of a weight tensor %.2e (%s)" %
                  (tag, e_lg, stats[tag][0], l2s[worst], worst, bias[wb], wb))
            assert l2s[worst] < 8e-3 and stats[tag][0] < 5e-3, (tag, worst, l2s[worst])
            assert abs(bias[wb]) < 1e-3, (tag, wb, bias[wb])
        finally:
            for k_ in opts:
                d.set_option(k_, 1 if k_ == "wino_bf3" else 0)
    assert stats["product"][0] < 4e-3


def test_training_trajectory_product_pipeline_vs_exact_fp32_kernels():
    """50 optimizer steps at 32^3, batch 2, from identical weights with (a) the product pipeline (16-bit matrix pipe, fp16 two-piece operands: conv_split 2),
    (b) the exact-fp32 Winograd kernels (wino_bf3 = 0), (c) the direct exact-fp32 kernels (direct_conv = 1), then the
    eval-mode mDice of a held-out batch (core/val.py's metric).  north_star: "Dice within 1e-4".  Training is a chaotic
    map, so two EXACT-fp32 implementations already drift apart; that drift (b vs c) is the noise band, and (a) must stay
    inside max(1e-4, 2 x band) of (c) for mDice and the final losses."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation
    rng = np.random.default_rng(31)
    N, S_ = 2, 32
    xs = rng.standard_normal((4, N, 1, S_, S_, S_)).astype(np.float32)
    # learnable labels: a smooth function of the input so that 50 steps move the Dice
    ys = ((xs[:, :, 0] > 0.3).astype(np.int32) + (xs[:, :, 0] > 1.0).astype(np.int32))
    xv = rng.standard_normal((N, 1, S_, S_, S_)).astype(np.float32)
    yv = ((xv[:, 0] > 0.3).astype(np.int32) + (xv[:, 0] > 1.0).astype(np.int32))
    d = dev()
    res = {}
    for tag, opts in (("product", {}), ("fp32_wino", {"wino_bf3": 0}), ("fp32_direct", {"direct_conv": 1})):
        for k_, v_ in opts.items():
            d.set_option(k_, v_)
        try:
            nn.seed(11)
            model = VNet(num_classes=3)
            model.train()
            model.set_dropout_masks({})
            opt = optim.Momentum(1e-3, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
            losses = {"types": [MixedLoss([CrossEntropyLoss(weight=[1.0, 1.0, 1.0]), DiceLoss()], [1, 1])], "coef": [1]}
            traj = []
            for it in range(50):
                logits = model(xs[it % 4])
                ll, _ = loss_computation(logits, to_labels(ys[it % 4]), losses)
                loss = sum(ll)
                loss.backward()
                opt.step()
                model.clear_gradients()
                if it % 10 == 9:
                    traj.append(float(loss))
            model.eval()
            ll, per = loss_computation(model(xv), to_labels(yv), losses)
            res[tag] = (np.array(traj), float(np.mean(np.asarray(per))), float(sum(ll)))
        finally:
            for k_ in opts:
                d.set_option(k_, 1 if k_ == "wino_bf3" else 0)
    (ta, ma, la), (tb, mb, lb), (tc, mc, lc) = res["product"], res["fp32_wino"], res["fp32_direct"]
    band_m, band_l, band_t = abs(mb - mc), abs(lb - lc), np.abs(tb - tc).max()
    print("mDice product (fp16 two-piece split) %.6f fp32-wino %.6f fp32-direct %.6f | |d| product-direct %.2e, fp32 band %.2e" %
          (ma, mb, mc, abs(ma - mc), band_m))
    print("eval loss |d| %.2e (band %.2e); train-loss trajectory |d| %.2e (band %.2e); losses %s" %
          (abs(la - lc), band_l, np.abs(ta - tc).max(), band_t, ta))
    assert ta[-1] < ta[0]                                  # it trains
    assert abs(ma - mc) < max(1e-4, 2 * band_m)
    assert abs(la - lc) < max(1e-4 * abs(lc), 2 * band_l)
    assert np.abs(ta - tc).max() < max(1e-4 * np.abs(tc).max(), 2 * band_t)


def test_adam_and_dice_options_trajectory_matches_oracle():
    """`optimizer: {type: adam}` (cvlibs/config.py:214-216) with MixedLoss([CE, DiceLoss(sigmoid_norm=False, weight)])
    (dice_loss.py:36-43,68-69): three eval-mode-BN steps through the product's classes against the float64 oracle."""
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    shape, ncls, K, S, N = CFGS[0]
    dw = np.array([0.5, 2.0, 1.25][:ncls] + [1.0] * max(0, ncls - 3))
    rng = np.random.default_rng(21)
    model, params = _build(ncls, K, S, seed=6)
    om = O.VNetOracle(params, 1, ncls, K, S)
    m1, m2, ce_w = {}, {}, None
    opt = optim.Adam(1e-4, parameters=model.parameters(), weight_decay=1e-4)
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss(sigmoid_norm=False, weight=list(dw))], [1, 1])],
              "coef": [1]}
    model.eval()
    for step in range(3):
        x = rng.standard_normal((N, 1) + shape).astype(np.float32)
        y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
        z = om.forward(x, train=False)
        if ce_w is None:
            ce_w = O.class_weights(z)
        ce, dce = O.cross_entropy(z, y, ce_w, 255)
        dl, per_ref, ddl = O.dice(z, y, sigmoid_norm=False, weight=dw)
        grads = om.backward(dce + ddl)
        O.adam_step(om.p, grads, m1, m2, step + 1, 1e-4, weight_decay=1e-4, names=om.trainable)
        logits = model(x)
        loss_list, per = loss_computation(logits, to_labels(y), losses)
        loss = sum(loss_list)
        loss.backward()
        opt.step()
        model.clear_gradients()
        assert abs(float(loss) - (ce + dl)) < 5e-5 * abs(ce + dl), (step, float(loss), ce + dl)
        assert np.abs(np.asarray(per) - per_ref).max() < 1e-4
    sd = model.state_dict()
    # Adam's first steps move every weight by ~lr regardless of the gradient's size: tensors whose gradient is at the
    # fp32 noise level (sign flips) may differ by 2*lr per step; everything else follows the oracle closely
    worst = max(np.abs(sd[k] - om.p[k]).max() for k in om.trainable)
    med = np.median([np.abs(sd[k] - om.p[k]).mean() for k in om.trainable])
    print("adam trajectory: worst %.2e  median of means %.2e" % (worst, med))
    assert worst <= 3 * 2 * 1e-4 + 1e-6 and med < 2e-5


def test_reverse_transform_resizes_logits_back():
    """core/infer.py:43-59,88-90: with a Resize3D among the val transforms the logits are brought back to the original
    shape (trilinear, align_corners=False) before the argmax."""
    from medicalseg_amd import models
    from medicalseg_amd.core import infer
    from medicalseg_amd.device import to_tensor

    class Resize3D:  # get_reverse_list matches on the class name and reads .size (infer.py:36-38)
        def __init__(self, size):
            self.size = size

    rng = np.random.default_rng(9)
    model = models.VNet(num_classes=3)
    model.eval()
    x = rng.standard_normal((1, 1, 16, 16, 16)).astype(np.float32)
    _, logit = infer.inference(model, to_tensor(x))
    small = logit.numpy()
    pred, back = infer.inference(model, to_tensor(x), ori_shape=(24, 20, 31), transforms=[Resize3D((16, 16, 16))])
    assert tuple(back.shape) == (1, 3, 24, 20, 31) and tuple(pred.shape) == (1, 1, 24, 20, 31)
    ref = O.trilinear_resize(small.astype(np.float64), (24, 20, 31))
    assert np.abs(back.numpy() - ref).max() < 1e-5 * np.abs(ref).max()
    top2 = np.sort(ref, axis=1)
    clear = (top2[:, -1] - top2[:, -2]) > 1e-4 * np.abs(ref).max()
    assert np.array_equal(pred.numpy()[:, 0][clear], ref.argmax(1)[clear])
    # unchanged shape: no resize
    _, same = infer.inference(model, to_tensor(x), ori_shape=(16, 16, 16), transforms=[Resize3D((16, 16, 16))])
    assert np.array_equal(same.numpy(), small)


@pytest.mark.parametrize("train", [False, True])
def test_vnet_elu_matches_oracle(train):
    """VNet(elu=True) (ELUCons, vnet.py:25-29; nn.ELU as its own pass around the activation-less unit kernels): state dict
    without PReLU tensors, logits, loss and every gradient against the float64 oracle's ELU branch, eval- and train-mode
    BatchNorm (dropout off)."""
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss, VNet
    from medicalseg_amd.utils import loss_computation
    shape, ncls, K, S, N = CFGS[0]
    full = O.init_params(7, 1, ncls, K, S)
    params = {k: v for k, v in full.items() if "relu" not in k}
    model = VNet(elu=True, in_channels=1, num_classes=ncls, kernel_size=K, stride_size=S)
    assert sorted(model.state_dict()) == sorted(params)             # ELU carries no parameter
    missing, unexpected = model.set_state_dict(params)
    assert not missing and not unexpected
    rng = np.random.default_rng(17)
    x = rng.standard_normal((N, 1) + shape).astype(np.float32)
    y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
    om = O.VNetOracle(params, 1, ncls, K, S)
    om.elu = True
    om.trainable = [n for n in om.trainable if "relu" not in n]
    masks = {} if train else None
    lg = om.forward(x, train=train, dropout_masks=masks)
    ol = O.MixedLossOracle()
    ll, per, dz = ol(lg, y)
    g = om.backward(dz)
    model.train() if train else model.eval()
    model.set_dropout_masks(masks)
    losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1])], "coef": [1]}
    logits = model(x)
    scale = np.abs(lg).max()
    assert np.abs(logits[0].numpy() - lg).max() < 2e-4 * scale
    loss_list, per_d = loss_computation(logits, to_labels(y), losses)
    loss = sum(loss_list)
    loss.backward()
    assert abs(float(loss) - sum(ll)) < 1e-4 * abs(sum(ll))
    grads = {name: p_.grad_numpy() for name, p_ in model.named_parameters()}
    assert sorted(grads) == sorted(om.trainable)
    errs = []
    for k in om.trainable:
        ref = g[k]
        if np.abs(ref).max() < 1e-9:   # conv bias ahead of a train-mode BatchNorm: exactly 0 in exact arithmetic
            assert np.abs(grads[k]).max() < 1e-4
            continue
        errs.append(np.linalg.norm((grads[k] - ref).ravel()) / np.linalg.norm(ref.ravel()))
    print("elu %s grad err: L2 worst %.2e median %.2e" % ("train" if train else "eval", max(errs), np.median(errs)))
    # 16^3: the deep BatchNorm layers see 1-8 voxels per channel in train mode (same bounds as the PReLU net's test above)
    assert max(errs) < (2e-2 if train else 1e-4)
    model.clear_gradients()


@pytest.mark.parametrize("which", ["VNetDeepSup", "UNet3D"])
def test_eager_optimizer_other_models_bitwise(which):
    """The eager optimizer on the other two models that report their blocks (VNetDeepSup: the deep-supervision heads are read
    AFTER some decoder blocks reported -- they are not blocks, their parameters wait for step(); UNet3D: InstanceNorm units):
    three training steps bitwise equal to the plain order, as tools/bench_workloads.py and core.train() now run them."""
    from medicalseg_amd import nn
    from medicalseg_amd import optimizer as optim
    from medicalseg_amd import models
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    ncls, N, shape = 3, 2, (32, 32, 16)
    results = []
    for eager in (False, True):
        rng = np.random.default_rng(9)
        nn.seed(21)
        nn.Dropout3D._site_counter = 0
        if which == "UNet3D":
            model = models.UNet3D(in_channels=1, num_classes=ncls, base_channels=16, depth=3)
        else:
            model = models.VNetDeepSup(elu=False, in_channels=1, num_classes=ncls)
        n_out = getattr(model, "num_outputs", 1)
        opt = optim.Momentum(1e-2, parameters=model.parameters(), momentum=0.9, weight_decay=1e-4)
        if eager:
            assert opt.enable_eager(model) is True
            opt.eager_min_floats = 0            # (these small test models have no block above the default 1 M parameters)
        losses = {"types": [MixedLoss([CrossEntropyLoss(), DiceLoss()], [1, 1]) for _ in range(n_out)], "coef": [1.0 / n_out] * n_out}
        model.train()
        nn.Dropout3D.step, nn.Dropout3D.seed = 0, 3
        vals = []
        for step in range(3):
            x = rng.standard_normal((N, 1) + shape).astype(np.float32)
            y = rng.integers(0, ncls, (N,) + shape).astype(np.int32)
            loss_list, _ = loss_computation(model(x), to_labels(y), losses)
            loss = sum(loss_list)
            loss.backward()
            if eager:
                assert len(opt._eager_done) >= 2
            opt.step()
            model.clear_gradients()
            vals.append(float(loss))
        results.append((vals, model.state_dict(), dev().d2h(opt.velocity_ptr, (model.arena.count,), np.float32)))
    (va, sda, vela), (vb, sdb, velb) = results
    assert va == vb, (va, vb)
    for k in sda:
        assert np.array_equal(sda[k], sdb[k]), k
    assert np.array_equal(vela, velb) and np.abs(vela).max() > 0
