"""GPU: the stage-1 training step — losses.compute_gt / lidf_loss (csrc/lidf_loss.hip) and
pipeline.lidf_forward_train — against the reference's own run (tests/golden/g9_train_step.npz) and the float64
restatement of tests/train_loss_ref.py."""
import numpy as np
import pytest
import torch

import train_loss_ref as tl
from util import (assert_f64_close, closed_form_params, closed_form_pointnet, make_module, make_pointnet)

pytestmark = pytest.mark.gpu


def _close(a, b, what, bad):
    """2e-4 of the reference tensor's own largest entry, as the training tests hold gradients — without their floor
    of 1.0 on the scale: most gradients of this step are far below 1 (full_rgb_feat 3e-3, the PointNet 1e-4 to
    5e-2), and a floor would leave them unchecked."""
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    print(what, "err %.3g scale %.3g err/scale %.3g" % (err, scale, err / scale if scale else float("inf")))
    if not err <= 2e-4 * scale:   # (collected, so that one run reports every tensor that misses)
        bad.append((what, err, scale))


def _zero_bias_bound(P, prob_w=0.5):
    """prob_dec's last bias: its derivative is sum_p g_logit[p], which is 0 exactly (log_softmax over a ray's pairs
    does not change when one number is added to every logit), so the reference's value (4.7e-10 in g9) and the
    product's are both the rounding of that cancellation and share no digits. sum_p |g_logit[p]| <= prob_w *
    sum_rays 2 n_label / L = 2 prob_w, and P float32 terms rounded and summed leave at most (P + 1) * 2^-24 of it."""
    return 2 * prob_w * (P + 1) * 2.0 ** -24


def _ray_major(d, dev):
    """The product's data_dict for one case of the fixture (or any restatement dict): the pair list re-ordered
    ray-major with voxels ascending inside a ray. Returns (dd, order) with ray_major = reference[order]."""
    R, V = d["miss_bid"].shape[0], d["voxel_bound"].shape[0]
    order = torch.argsort(d["pair_ray"] * V + d["pair_vox"], stable=True)
    pair_ray, pair_vox = d["pair_ray"][order], d["pair_vox"][order]
    pair_off = torch.zeros(R + 1, dtype=torch.int64)
    pair_off[1:] = torch.cumsum(torch.bincount(pair_ray, minlength=R), 0)
    dd = {"bs": d["bs"], "h": d["h"], "w": d["w"], "xyz_flat": d["xyz_flat"].to(dev),
          "ray_bid": d["miss_bid"].int().to(dev), "ray_flat": d["miss_flat"].int().to(dev),
          "pair_off": pair_off.int().to(dev), "pair_ray": pair_ray.int().to(dev), "pair_vox": pair_vox.int().to(dev),
          "voxel_bound": d["voxel_bound"].to(dev),
          "pred_pos": d["pred_pos"].to(dev).requires_grad_(True),
          "pred_prob_end": d["pred_prob_end"][order].contiguous().to(dev).requires_grad_(True)}
    return dd, order


def _check_loss(d, dd, order, epoch, opt, ref32, what, report=None):
    """lidf_loss on dd against the float64 restatement on d; ref32 = (loss [8], g_pred_pos, g_pred_prob_end) of a
    float32 evaluation (the fixture, or the restatement in float32)."""
    from implicit_depth_amd import LidfLossOptions, lidf_loss
    out = lidf_loss(dd, LidfLossOptions(**opt), "train", epoch)
    assert tuple(out) == tl.LOSS_KEYS and all(v.dim() == 0 and v.is_cuda for v in out.values())
    assert out["loss_net"].requires_grad and not any(out[k].requires_grad for k in tl.LOSS_KEYS if k != "loss_net")
    out["loss_net"].backward()
    loss64, gp64, gl64 = tl.loss_and_grads(d, torch.float64, epoch, **opt)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.shape[0])
    for i, k in enumerate(tl.LOSS_KEYS):
        assert_f64_close("%s %s" % (what, k), out[k].detach().cpu().reshape(1), loss64[i].reshape(1),
                         ref32[0][i].reshape(1), report=report)
    assert_f64_close(what + " g_pred_pos", dd["pred_pos"].grad.cpu(), gp64, ref32[1], report=report)
    assert_f64_close(what + " g_pred_prob_end", dd["pred_prob_end"].grad.cpu()[inv], gl64, ref32[2], report=report)
    return out


@pytest.mark.parametrize("name", sorted(tl.G9_CASES))
def test_fixture_labels_and_loss(cuda, name):
    from implicit_depth_amd.losses import compute_gt
    from implicit_depth_amd.query import to_reference_order
    g, _ = tl.g9_files()
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    dd, order = _ray_major(d, cuda)
    compute_gt(dd)
    P = d["pair_ray"].shape[0]
    perm = to_reference_order(dd["pair_ray"], dd["pair_vox"])
    assert torch.equal(perm.cpu(), torch.argsort(order))   # (ray-major arrays indexed by perm: the reference's order)
    assert torch.equal(dd["gt_pos"].cpu(), d["gt_pos"])
    assert dd["pcl_label"].dtype == torch.int64 and torch.equal(dd["pcl_label"][perm].cpu(), d["pcl_label"])
    assert torch.equal(dd["pcl_label_float"].cpu(), dd["pcl_label"].float().cpu())
    assert dd["n_label"].dim() == 0 and int(dd["n_label"]) == int(d["pcl_label"].sum())
    # the label-selected pair of every ray: the reference's index (voxel-major) of the same pair, P for an empty ray
    _, _, want = tl.compute_gt_ref(d["xyz_flat"], d["miss_bid"], d["miss_flat"], d["voxel_bound"], d["pair_ray"],
                                   d["pair_vox"])
    if epoch < 6:
        assert torch.equal(want, d["max_pair_id"])
    got = dd["gt_max_pair_id"].cpu()
    got_ref = torch.where(got < P, order[got.clamp(max=P - 1)], torch.full_like(got, P))
    assert torch.equal(got_ref, want)
    table = dd["pix2ray"].cpu().long()
    lin = d["miss_bid"] * (d["h"] * d["w"]) + d["miss_flat"]
    assert torch.equal(table[lin], torch.arange(lin.shape[0])) and int((table >= 0).sum()) == lin.shape[0]
    _check_loss(d, dd, order, epoch, opt, (ref["loss"], ref["g_pred_pos"], ref["g_pred_prob_end"]), "g9 " + name)


def _g9_modules(g, dev):
    sp, so, sn = (int(v) for v in g["seeds"])
    prob = make_module("IMNET", closed_form_params("IMNET", 385, sp), 385, dev).train()
    off = make_module("IEF", closed_form_params("IEF", 385, so), 385, dev).train()
    pnet = make_pointnet(closed_form_pointnet(sn), dev).train()
    return pnet, prob, off


def _g9_step(g, name, dev):
    from implicit_depth_amd import LidfLossOptions, LidfOptions, lidf_forward_train
    epoch, opt = tl.g9_opt(name)
    batch, feat = tl.g9_batch(g)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    feat = feat.to(dev).requires_grad_(True)
    mods = _g9_modules(g, dev)
    np.random.seed(int(g["np_seed"]))   # (sample_miss_rays draws the window as the reference does)
    ok, dd, loss = lidf_forward_train(batch, feat, *mods, opt=LidfOptions(miss_sample_num=int(g["miss_sample_num"])),
                                      loss_opt=LidfLossOptions(**opt), epoch=epoch)
    assert ok
    loss["loss_net"].backward()
    return dd, loss, feat, mods


@pytest.mark.parametrize("name", sorted(tl.G9_CASES))
def test_whole_step_against_the_reference(cuda, name):
    g, gp = tl.g9_files()
    d, ref = tl.g9_case(g, name)
    dd, loss, feat, mods = _g9_step(g, name, cuda)
    assert torch.equal(dd["miss_bid"].cpu(), d["miss_bid"]) and torch.equal(dd["miss_flat_img_id"].cpu(), d["miss_flat"])
    assert dd["pair_ray"].shape[0] == d["pair_ray"].shape[0]
    bad = []
    for i, k in enumerate(tl.LOSS_KEYS):
        _close(loss[k].detach().cpu(), ref["loss"][i], (name, k), bad)
    _close(feat.grad.cpu(), ref["g_full_rgb_feat"], (name, "full_rgb_feat"), bad)
    stride = int(g["param_stride"])
    for mod, m in zip(("pnet_model", "prob_dec", "offset_dec"), mods):
        for k, p in m.named_parameters():
            want = torch.from_numpy(gp["%s_g_%s.%s" % (name, mod, k)])
            got = p.grad.detach().cpu().reshape(-1)
            got = got[::stride] if got.numel() > 4096 else got
            if (mod, k) == ("prob_dec", "linear_4.bias"):
                bound = _zero_bias_bound(d["pair_ray"].shape[0])
                print((name, mod, k), "got %.3g reference %.3g bound %.3g" % (float(got), float(want), bound))
                assert abs(float(got)) <= bound and abs(float(want)) <= bound
                continue
            _close(got, want, (name, mod, k), bad)
    assert not bad, bad


def test_whole_step_is_bit_identical_and_trains(cuda):
    """Two runs of the same seeded step: identical loss, predictions and parameter gradients; an optimiser step
    then changes every trainable parameter."""
    g, _ = tl.g9_files()
    runs = []
    for _ in range(2):
        dd, loss, feat, mods = _g9_step(g, "e0", cuda)
        run = {"loss_net": loss["loss_net"].detach().clone(), "full_rgb_feat": feat.grad.clone(),
               "pred_pos": dd["pred_pos"].detach().clone(), "pred_prob_end": dd["pred_prob_end"].detach().clone()}
        for mod, m in zip(tl.G9_MODULES, (mods[1], mods[2], mods[0])):
            run.update({"%s.%s" % (mod, k): p.grad.clone() for k, p in m.named_parameters()})
        runs.append(run)
    # Every sum of the step has a fixed order — the new labels / loss launches and every parameter gradient — except
    # the one DESIGN.md 5.9 names: RoIAlign's backward adds the taps of boxes clamped at the image border with float
    # atomics. On this 16 x 24 frame every box is clamped, so full_rgb_feat's gradient is the same sum in another
    # order: equal to rounding (a few units of 2^-24 of its largest entry), not bit for bit.
    differ = [k for k in runs[0] if k != "full_rgb_feat" and not torch.equal(runs[0][k], runs[1][k])]
    assert not differ, differ
    a, b = runs[0]["full_rgb_feat"], runs[1]["full_rgb_feat"]
    assert (a - b).abs().max().item() <= 16 * 2.0 ** -24 * a.abs().max().item()
    named = [("%s.%s" % (mod, k), p) for mod, m in zip(("pnet_model", "prob_dec", "offset_dec"), mods)
             for k, p in m.named_parameters()]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in named)
    before = {k: p.detach().clone() for k, p in named}
    torch.optim.SGD([p for _, p in named], lr=0.1).step()
    same = [k for k, p in named if torch.equal(before[k], p.detach())]
    print("unchanged by the step:", same)
    # One parameter cannot move, here or in the reference: prob_dec's last bias, whose derivative is 0 exactly
    # (_zero_bias_bound). The reference's own autograd records 4.7e-10 for it, and lr * 4.7e-10 is below half an ulp
    # of the bias. What is asserted for it instead is that the cancellation happens.
    assert same in ([], ["prob_dec.linear_4.bias"]), same
    g_bias = dict(named)["prob_dec.linear_4.bias"].grad
    assert g_bias.abs().max().item() <= _zero_bias_bound(dd["pair_ray"].shape[0])


def _synthetic_step(B, h, w, hole_frac, dev, seed=3, **loss_opt):
    from implicit_depth_amd import LidfLossOptions, LidfOptions, lidf_forward_train
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    from util import orc
    batch, feat = synthetic_batch(B, h, w, seed=seed, hole_frac=hole_frac)
    cnt = batch["corrupt_mask"].reshape(B, -1).sum(1)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    pnet = make_pointnet(orc.init_pointnet(3, 1.5), dev).train()
    prob = make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, dev).train()
    off = make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, dev).train()
    opt = LidfOptions()
    np.random.seed(77)
    ok, dd, loss = lidf_forward_train(batch, feat.to(dev).requires_grad_(True), pnet, prob, off, opt=opt,
                                      loss_opt=LidfLossOptions(**loss_opt), epoch=0)
    return ok, dd, loss, cnt, opt


def _restatement_dict(dd):
    """lidf_forward_train's data_dict as the restatement's input (CPU, pairs ray-major as they are)."""
    c = lambda t: t.detach().cpu()  # noqa: E731
    return {"bs": dd["bs"], "h": dd["h"], "w": dd["w"], "xyz_flat": c(dd["xyz_flat"]), "miss_bid": c(dd["miss_bid"]),
            "miss_flat": c(dd["miss_flat_img_id"]), "pair_ray": c(dd["pair_ray"]).long(),
            "pair_vox": c(dd["pair_vox"]).long(), "voxel_bound": c(dd["voxel_bound"]), "gt_pos": c(dd["gt_pos"]),
            "pcl_label": c(dd["pcl_label"]), "pred_pos": c(dd["pred_pos"]), "pred_prob_end": c(dd["pred_prob_end"])}


@pytest.mark.parametrize("B,h,w,hole_frac", [(2, 96, 128, 1.0), (8, 240, 320, 1.9)])
def test_loss_at_size_against_float64(cuda, B, h, w, hole_frac):
    # (hard_neg is left to the fixture, which keeps every top-k boundary clear of ties: among 16,000 selected rays
    # the k-th and (k+1)-th value differ by rounding, and float32 and float64 then select different elements)
    opt = dict(smooth_w=0.5)
    ok, dd, loss, cnt, popt = _synthetic_step(B, h, w, hole_frac, cuda, **opt)
    assert ok
    R = dd["total_miss_sample_num"]
    if B == 8:   # the shipped window: every frame has more corrupt pixels than miss_sample_num
        assert int(cnt.min()) > popt.miss_sample_num and R == B * popt.miss_sample_num
    L = int(dd["n_label"])
    assert L > 0
    d = _restatement_dict(dd)
    gt_pos, label, max_id = tl.compute_gt_ref(d["xyz_flat"], d["miss_bid"], d["miss_flat"], d["voxel_bound"],
                                              d["pair_ray"], d["pair_vox"])
    assert torch.equal(gt_pos, d["gt_pos"]) and torch.equal(label, d["pcl_label"])
    assert torch.equal(max_id, dd["gt_max_pair_id"].cpu()) and L == int(label.sum())
    assert torch.equal(dd["max_pair_id"].cpu(), max_id)   # epoch 0: the query selected by the labels
    # the fused loss on the step's own pred_pos / logits as fresh leaves, against the restatement in f64 / f32
    dd2 = dict(dd)
    dd2["pred_pos"] = dd["pred_pos"].detach().clone().requires_grad_(True)
    dd2["pred_prob_end"] = dd["pred_prob_end"].detach().clone().requires_grad_(True)
    ref32 = tl.loss_and_grads(d, torch.float32, 0, **opt)
    order = torch.arange(d["pair_ray"].shape[0])
    report = []
    out = _check_loss(d, dd2, order, 0, opt, ref32, "%dx%dx%d" % (B, h, w), report)
    assert torch.equal(out["loss_net"].detach(), loss["loss_net"].detach())
    print("R %d P %d L %d worst ratio %.2f" % (R, d["pair_ray"].shape[0], L, max(r["ratio_max"] for r in report)))


def test_no_labelled_pair(cuda):
    """NaN prob_loss as torch.mean of an empty tensor in the reference; the other losses finite, no gradient on the
    logits."""
    from implicit_depth_amd import lidf_loss
    from implicit_depth_amd.losses import compute_gt
    g, _ = tl.g9_files()
    d, _ = tl.g9_case(g, "e0")
    d["voxel_bound"] = d["voxel_bound"] + 50.0
    dd, _ = _ray_major(d, cuda)
    compute_gt(dd)
    assert int(dd["n_label"]) == 0 and int(dd["pcl_label"].sum()) == 0
    out = lidf_loss(dd)
    out["loss_net"].backward()
    assert torch.isnan(out["prob_loss"]) and torch.isnan(out["loss_net"])
    assert all(torch.isfinite(out[k]) for k in ("pos_loss", "surf_norm_loss", "smooth_loss", "acc", "err", "angle_err"))
    assert torch.isfinite(dd["pred_pos"].grad).all() and bool((dd["pred_prob_end"].grad == 0).all())


def test_early_exits(cuda):
    from implicit_depth_amd import lidf_forward_train
    from implicit_depth_amd.synthetic import init_decoder_params, synthetic_batch
    from util import orc
    pnet = make_pointnet(orc.init_pointnet(3, 1.5), cuda).train()
    prob = make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, cuda).train()
    off = make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, cuda).train()

    def run(edit):
        batch, feat = synthetic_batch(1, 48, 64, seed=5)
        edit(batch)
        batch = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in batch.items()}
        return lidf_forward_train(batch, feat.to(cuda).requires_grad_(True), pnet, prob, off)
    ok, dd, loss = run(lambda b: b["valid_mask"].zero_())                    # no valid point: no occupied voxel
    assert not ok and loss == {} and "miss_bid" not in dd

    def outside(b):   # every valid point outside the grid (z beyond its far face): V == 0
        b["xyz_corrupt"][:, 2] += 10.0
    ok, dd, loss = run(outside)
    assert not ok and loss == {} and dd["voxel_bound"].shape[0] == 0 and "miss_bid" not in dd
    ok, dd, loss = run(lambda b: b["corrupt_mask"].zero_())                  # no miss ray
    assert not ok and loss == {} and dd["total_miss_sample_num"] == 0 and "pair_ray" not in dd

    def far_apart(b):   # valid points in the left columns only, one corrupt pixel at the right edge
        b["valid_mask"][..., 8:] = 0
        b["corrupt_mask"].zero_()
        b["corrupt_mask"][..., 24, 63] = 1
    ok, dd, loss = run(far_apart)                                            # no intersecting pair
    assert not ok and loss == {} and dd["pair_ray"].shape[0] == 0 and "gt_pos" not in dd
    ok, dd, loss = run(lambda b: None)
    assert ok and torch.isfinite(loss["loss_net"])


def test_terms_left_out_of_loss_net(cuda):
    """surf_norm_w = 0, or epoch < surf_norm_epo: the term is reported but enters neither loss_net nor the gradient."""
    from implicit_depth_amd import LidfLossOptions, lidf_loss
    from implicit_depth_amd.losses import compute_gt
    g, _ = tl.g9_files()
    d, _ = tl.g9_case(g, "e6")
    res = {}
    for key, opt, epoch in (("w0", dict(surf_norm_w=0.0), 0), ("late", dict(surf_norm_epo=3), 2),
                            ("on", dict(surf_norm_epo=3), 3)):
        dd, order = _ray_major(d, cuda)
        compute_gt(dd)
        out = lidf_loss(dd, LidfLossOptions(**opt), "train", epoch)
        out["loss_net"].backward()
        res[key] = (out, dd["pred_pos"].grad.clone(), dd["pred_prob_end"].grad.clone())
        want = 100.0 * out["pos_loss"] + 0.5 * out["prob_loss"]
        if key == "on":
            want = want + 10.0 * out["surf_norm_loss"]
        assert abs(float(out["loss_net"]) - float(want)) <= 1e-6 * abs(float(want))
    assert torch.equal(res["w0"][1], res["late"][1]) and torch.equal(res["w0"][2], res["late"][2])
    assert torch.equal(res["w0"][0]["surf_norm_loss"], res["on"][0]["surf_norm_loss"])
    assert not torch.equal(res["on"][1], res["late"][1]) and torch.equal(res["on"][2], res["late"][2])
    # without the normal term a ray's position gradient is the L1 term alone: +-pos_w / (3 R)
    R = d["pred_pos"].shape[0]
    assert (res["w0"][1].abs() - 100.0 / (3 * R)).abs().max().item() <= 1e-6 * 100.0 / (3 * R)


def test_normal_maps_on_request(cuda):
    from implicit_depth_amd import lidf_loss
    from implicit_depth_amd.losses import compute_gt
    g, _ = tl.g9_files()
    d, _ = tl.g9_case(g, "e6")
    dd, _ = _ray_major(d, cuda)
    compute_gt(dd)
    lidf_loss(dd)
    assert "gt_surf_norm_img" not in dd
    lidf_loss(dd, normal_maps=True)
    for key, pos in (("gt_surf_norm_img", d["gt_pos"]), ("pred_surf_norm_img", d["pred_pos"])):
        img = d["xyz_flat"].clone()
        img[d["miss_bid"], d["miss_flat"]] = pos
        want, _, _ = tl.image_normals(img.reshape(d["bs"], d["h"], d["w"], 3).permute(0, 3, 1, 2))
        assert (dd[key].cpu() - want).abs().max().item() <= 1e-5


def test_lidf_loss_checks_a_reused_dict(cuda):
    """compute_gt's entries left in a dict whose rays or pairs have changed since, or an index of the wrong dtype,
    are refused before a kernel indexes with them."""
    from implicit_depth_amd import lidf_loss
    from implicit_depth_amd.losses import compute_gt
    g, _ = tl.g9_files()
    d, _ = tl.g9_case(g, "e0")
    dd, _ = _ray_major(d, cuda)
    compute_gt(dd)
    R = d["miss_bid"].shape[0]
    for edit in (lambda t: t.update(pair_off=t["pair_off"].long()),
                 lambda t: t.update(pair_off=t["pair_off"][:-1].contiguous()),
                 lambda t: t.update(pix2ray=t["pix2ray"][:-1].contiguous()),
                 lambda t: t.update(pix2ray=t["pix2ray"].long()),
                 lambda t: t.update(ray_bid=t["ray_bid"][:R - 1].contiguous(),
                                    ray_flat=t["ray_flat"][:R - 1].contiguous()),
                 lambda t: t.update(gt_max_pair_id=t["gt_max_pair_id"].int()),
                 lambda t: t.update(h=t["h"] + 1)):
        t = dict(dd)
        edit(t)
        with pytest.raises(RuntimeError):
            lidf_loss(t)
    assert torch.isfinite(lidf_loss(dd)["loss_net"])
