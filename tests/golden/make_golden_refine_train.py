"""make_golden_refine_train.py — the stage-2 TRAINING step of the reference as golden vectors.

Run where the reference's sources are (make_golden.REF; it imports them):   python tests/golden/make_golden_refine_train.py
Runs the reference's own stage-2 iteration (trainers/train_refine.py:374-399) on the CPU with train_refine.yaml on the
two-frame 16 x 24 batch recipe of g9 (make_golden_train.make_batch): the frozen LIDF.forward(batch, 'train', epoch),
RefineNet.forward('train', epoch, data_dict) and loss_net.backward(). Nothing of the reference is copied; the stubs of
make_golden.py stand in for cv2 / torchvision / torch_scatter / the two JIT extensions. Weights are closed-form
(stage 1: g9's seeds), the ResNet is replaced by FixedFeatures, grid.valid_sample_num = -1, grid.miss_sample_num = 24.

  g10_refine_train.npz         the batch, full_rgb_feat, the seeds, and per case: the sampled rays, the pair list in
                               the reference's voxel-major order, gt_pos, stage 1's pred_pos, max_pair_id and eight
                               loss values, the perturbation scalar (NaN: none drawn), pred_pos_refine, the end voxels
                               of the last iteration, the six values of loss_dict_refine and, after
                               loss_net.backward(), the gradient of pred_pos_refine (retain_grad)
  g10_refine_train_params.npz  per case the gradient of every pnet_model / offset_dec parameter of the RefineNet;
                               tensors of more than 4096 elements at every PARAM_STRIDE-th element, as g9

Cases (epoch 0; model.maxpool_label_epo is 0 in train_refine.yaml, so stage 1 selects by the arg-max of its logits):
  plain      loss.pos_w 100 / surf_norm_w 10 (train_refine.yaml), a perturbation drawn
  hn         hard_neg True, hard_neg_ratio 0.1, pos_w 20 / surf_norm_w 2 (train_refine_hardneg.yaml), the same draw
  smooth     plain + smooth_w 1.0 (the only case whose loss_net holds the smoothness term), the same draw
  noperturb  plain, with a numpy seed whose first draw says 'no perturbation'

The generator asserts what keeps the fixture from being a coin flip of float32 rounding; it searches the numpy seeds,
the depth shift and the stage-2 decoder's weight seed until all of it holds, and fails loudly otherwise:
  no leaky-ReLU pre-activation of the stage-2 decoder, in either iteration, within 2e-5 of 0 (the PointNet's minimum
  is recorded as min_preact_pnet and must not be exactly 0); the position that enters each iteration — after the
  perturbation — has no coordinate within 2e-4 of a voxel face (twice tests/util.py:TOL, the bound the product's
  pred_pos is held to: an end voxel is an index, one flip changes every gradient); every ray's two largest stage-1
  logits more than 1e-4 apart; no coordinate of pred_pos_refine - gt_pos within 2e-4 of 0 (the L1 gradient is a
  sign); top-k gaps above 1e-6 relative (hard_neg); interior normals longer than 1e-4; a ray without pairs; sampled
  pixels in the last row and the last column; sampled pixels whose right or lower neighbour is not sampled.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, closed_form_params, closed_form_pointnet, install_stubs, orc  # noqa: E402
from make_golden_train import (FixedFeatures, MISS_SAMPLE_NUM, PARAM_STRIDE, apply_overrides,  # noqa: E402
                               differentiable_roi_align, find_face, load_stage1, make_batch, save_npz, strided, topk_gap)

EPOCH = 0
PNET_REFINE_SEED = 43
# name -> (perturbed, loss.* overrides)
CASES = (("plain", True, {}),
         ("hn", True, dict(hard_neg=True, hard_neg_ratio=0.1, pos_w=20.0, surf_norm_w=2.0)),
         ("smooth", True, dict(smooth_w=1.0)),
         ("noperturb", False, {}))
LOSS_KEYS = ("pos_loss", "prob_loss", "surf_norm_loss", "smooth_loss", "loss_net", "acc", "err", "angle_err")
REFINE_LOSS_KEYS = ("pos_loss", "surf_norm_loss", "smooth_loss", "loss_net", "err", "angle_err")


def load_refine(refine, seeds, factor=1.0):
    """Closed-form weights at the widths the options give the two stage-2 modules; seeds = (offset_dec, pnet_model)."""
    r = refine.opt.refine
    refine.offset_dec.load_state_dict(closed_form_params(r.offdec_type, refine.offset_dec.inp_dim, seed=seeds[0],
                                                         gf=r.imnet_gf, factor=factor))
    refine.pnet_model.load_state_dict(closed_form_pointnet(seeds[1], cin=r.pnet_in, out=r.pnet_out, gf=r.pnet_gf))


def build(stage1_seeds, refine_seed, loss, overrides=None):
    """The reference's LIDF and RefineNet with train_refine.yaml (+ overrides: make_golden_train.apply_overrides) and
    closed-form weights; stage 1 frozen."""
    import models.pipeline as pl
    from opt import Params
    cfg = os.path.join(REF, "experiments", "implicit_depth")
    opt = Params(os.path.join(cfg, "default_config.yaml"))
    opt.update(os.path.join(cfg, "train_refine.yaml"))
    opt.dist.ddp = False
    opt.gpu_id = 0
    opt.grid.valid_sample_num = -1
    opt.grid.miss_sample_num = MISS_SAMPLE_NUM
    for k, v in loss.items():
        setattr(opt.loss, k, v)
    apply_overrides(opt, overrides)
    assert opt.model.maxpool_label_epo == 0 and opt.refine.perturb and opt.refine.perturb_prob == 0.8
    torch.manual_seed(1234)
    dev = torch.device("cpu")
    lidf = pl.LIDF(opt, dev).eval()
    load_stage1(lidf, stage1_seeds)
    for p in lidf.parameters():   # trainers/train_refine.py:71-73
        p.requires_grad = False
    refine = pl.RefineNet(opt, dev).eval()
    load_refine(refine, (refine_seed, PNET_REFINE_SEED))
    return pl, lidf, refine, opt


def stage1(lidf, batch, feat, np_seed):
    """The frozen LIDF.forward(batch, 'train', epoch), numpy seeded just before it as a trainer's iteration would be."""
    lidf.resnet_model = FixedFeatures(feat)
    np.random.seed(np_seed)
    ok, dd, loss = lidf(batch, "train", EPOCH)
    assert ok and not dd["pred_pos"].requires_grad
    return dd, loss


def peek_perturbation():
    """What RefineNet.get_pred_refine (models/pipeline.py:926-935) is about to draw from np.random, without
    consuming it: the product's restatement of those lines on a saved generator state. run_refine asserts that the
    reference's own first iteration then started from exactly pred_pos + noise * miss_ray_dir."""
    from implicit_depth_amd.query import refine_perturb_noise
    state = np.random.get_state()
    noise = refine_perturb_noise(0.8)
    np.random.set_state(state)
    return noise


def run_refine(pl, refine, dd, checks):
    """RefineNet.forward('train', epoch, dd) + loss_net.backward(); `checks` collects the asserted quantities."""
    refine.zero_grad()
    pre, pre_pnet, entered, end_voxels = [], [], [], []
    hooks = [m.register_forward_hook(lambda mod, i, o: pre.append(o.detach().abs().min().item()))
             for m in (refine.offset_dec.linear_1, refine.offset_dec.linear_2, refine.offset_dec.linear_3)]
    hooks += [m.register_forward_hook(lambda mod, i, o: pre_pnet.append(o.detach().abs().min().item()))
              for m in refine.pnet_model.children()]
    real_aabb, real_scatter, inner = pl.pcl_aabb, pl.scatter, refine.compute_loss

    class Aabb:   # the position that enters an iteration is what get_pred_refine hands to pcl_aabb (:939)
        @staticmethod
        def forward(pos, *a):
            entered.append(pos.detach().clone())
            return real_aabb.forward(pos.detach(), *a)

    def scatter(src, index, dim=0, out=None, dim_size=None, reduce="sum"):   # (:944: end_voxel_id, in place)
        r = real_scatter(src, index, dim=dim, out=out, dim_size=dim_size, reduce=reduce)
        if out is not None:
            end_voxels.append(out.clone())
        return r

    def compute_loss(d, exp_type, ep):
        d["pred_pos_refine"].retain_grad()
        return inner(d, exp_type, ep)
    noise = peek_perturbation()
    pl.pcl_aabb, pl.scatter, refine.compute_loss = Aabb, scatter, compute_loss
    try:
        dd, loss = refine("train", EPOCH, dd)
    finally:
        pl.pcl_aabb, pl.scatter, refine.compute_loss = real_aabb, real_scatter, inner
        for hk in hooks:
            hk.remove()
    loss["loss_net"].backward()
    assert len(entered) == 2 and len(end_voxels) == 2
    start = dd["pred_pos"] if noise is None else dd["pred_pos"] + noise * dd["miss_ray_dir"]
    assert torch.equal(entered[0], start), "the perturbation drawn is not the one peeked"
    checks.update(min_preact=min(pre), min_preact_pnet=min(pre_pnet), entered=entered, noise=noise,
                  end_voxel_id=end_voxels[1])
    return dd, loss


def conditions(dd, hard_neg, checks):
    """The asserted properties of one case; returns a list of the violated ones."""
    bad = []
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    R = dd["total_miss_sample_num"]
    ray = dd["miss_ray_intersect_idx"]
    bid, flat = dd["miss_bid"], dd["miss_flat_img_id"]
    pred, gt = dd["pred_pos_refine"].detach(), dd["gt_pos"]
    if checks["min_preact"] <= 2e-5:
        bad.append("pre-activation %.3g" % checks["min_preact"])
    if checks["min_preact_pnet"] == 0.0:
        bad.append("a PointNet pre-activation is exactly 0")
    part = dd["part_size"]
    for it, pos in enumerate(checks["entered"]):
        off = (pos.double() - dd["xmin"].double()) / part
        dist = ((off - off.round()).abs() * part).min().item()
        if dist <= 2e-4:
            bad.append("iteration %d input %.3g from a voxel face" % (it, dist))
    lg = dd["pred_prob_end"].detach()[:, 0].double()
    for r in range(R):
        v = torch.sort(lg[ray == r], descending=True)[0]
        if v.numel() > 1 and (v[0] - v[1]).item() <= 1e-4:
            bad.append("ray %d logit gap %.3g" % (r, (v[0] - v[1]).item()))
    if (pred - gt).abs().min().item() <= 2e-4:
        bad.append("pred_pos_refine - gt_pos coordinate %.3g" % (pred - gt).abs().min().item())
    if not bool((torch.bincount(ray, minlength=R) == 0).any()):
        bad.append("no ray without pairs")
    y, x = flat // w, flat % w
    sampled = torch.zeros(bs, h * w, dtype=torch.bool)
    sampled[bid, flat] = True
    if not bool((y == h - 1).any()) or not bool((x == w - 1).any()):
        bad.append("no sampled pixel in the last row / column")
    right = sampled[bid, (flat + 1).clamp(max=h * w - 1)] | (x == w - 1)
    below = sampled[bid, (flat + w).clamp(max=h * w - 1)] | (y == h - 1)
    if bool(right.all()) or bool(below.all()):
        bad.append("every right / lower neighbour is sampled")
    inner = (y < h - 1) & (x < w - 1)
    unit, sq = [], []
    for pos in (gt, pred):
        img = dd["xyz_flat"].clone()
        img[bid, flat] = pos
        img = img.reshape(bs, h, w, 3).double()
        dx, dy = torch.zeros_like(img), torch.zeros_like(img)
        dx[:, :, :-1] = img[:, :, 1:] - img[:, :, :-1]
        dy[:, :-1] = img[:, 1:] - img[:, :-1]
        n = torch.linalg.cross(dx, dy, dim=-1).reshape(bs, h * w, 3)[bid, flat]
        nrm = n.norm(dim=-1)
        if nrm[inner].min().item() < 1e-4:
            bad.append("normal of length %.3g" % nrm[inner].min().item())
        unit.append(n / (nrm.unsqueeze(-1) + 1e-8))
        sq = [(dx * dx).sum(-1).reshape(bs, h * w)[bid, flat], (dy * dy).sum(-1).reshape(bs, h * w)[bid, flat]]
    if hard_neg:
        cos = torch.nn.functional.cosine_similarity(unit[1], unit[0], dim=-1)
        vecs = {"pos": (pred - gt).abs().mean(-1), "surf_norm": (1 - cos) / 2, "dx": sq[0], "dy": sq[1]}
        for name, v in vecs.items():
            if topk_gap(v) <= 1e-6:
                bad.append("top-k gap of %s %.3g" % (name, topk_gap(v)))
    return bad


def np_seeds(lidf, batch, feat):
    """The first numpy seed after whose stage 1 a perturbation is drawn, and the first after which none is."""
    found = {}
    for seed in range(2024, 2124):
        with torch.no_grad():
            stage1(lidf, batch, feat, seed)
        found.setdefault(peek_perturbation() is not None, seed)
        if len(found) == 2:
            return found[True], found[False]
    raise SystemExit("g10: no numpy seed pair")


def g9_sources(g9, overrides=None):
    """Stage-1 settings (shift, face, full_rgb_feat, (prob_dec, offset_dec, pnet_model) seeds) to try: the stored
    stage-1 fixture's own first, then its weights and features on other depth shifts."""
    s1 = tuple(int(v) for v in g9["seeds"])
    feat = torch.from_numpy(np.asarray(g9["full_rgb_feat"])).clone()
    f = g9["face_ray"]
    yield float(g9["depth_shift"]), (int(f[0]), int(f[1]), int(f[2]), int(f[3]), float(f[4])), feat, s1
    for shift in (0.0, 0.003, 0.007, -0.004, 0.011, -0.009, 0.014, -0.013):
        if abs(shift - float(g9["depth_shift"])) > 1e-9:
            face = find_face(build(s1, 31, {}, overrides)[1], shift)
            if face is not None:
                yield shift, face, feat, s1


def generate(verbose=True, overrides=None, cases=CASES, sources=None, tag="g10"):
    """sources: an iterable like g9_sources' (default: from g9_train_step.npz)."""
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    install_stubs()
    differentiable_roi_align()
    if sources is None:
        sources = g9_sources(np.load(os.path.join(HERE, "g9_train_step.npz")))
    for shift, face, feat, s1 in sources:
        pl, lidf, _, _ = build(s1, 31, {}, overrides)
        batch = make_batch(shift, face)
        seed_p, seed_n = np_seeds(lidf, batch, feat)
        if verbose:
            print("%s: shift %g: numpy seeds %d (perturbed) / %d (not)" % (tag, shift, seed_p, seed_n))
        why = {}
        pl, lidf, refine, _ = build(s1, 31, {}, overrides)
        starts = []
        wanted = sorted({c[1] for c in cases}, reverse=True)   # (the starts the cases use: perturbed, unperturbed)
        for perturbed, np_seed in ((p, seed_p if p else seed_n) for p in wanted):   # (stage 1 does not depend on the stage-2 seed)
            dd, _ = stage1(lidf, batch, feat, np_seed)
            starts.append((perturbed, dd, np.random.get_state()))
        for rseed in range(31, 6000):
            load_refine(refine, (rseed, PNET_REFINE_SEED))
            ok = True
            for perturbed, dd, state in starts:
                np.random.set_state(state)
                checks = {}
                dd, _ = run_refine(pl, refine, dict(dd), checks)
                assert (checks["noise"] is not None) == perturbed
                bad = conditions(dd, True, checks)
                if bad:
                    why[bad[0].split(" ")[0]] = why.get(bad[0].split(" ")[0], 0) + 1
                    ok = False
                    break
            if ok:
                break
        else:
            if verbose:
                print("%s: shift %g rejected: %s" % (tag, shift, why))
            continue
        if verbose:
            print("%s: stage-2 decoder seed %d (rejections on the way: %s)" % (tag, rseed, why))
        main = {"seeds_stage1": np.array(s1), "seeds_refine": np.array((rseed, PNET_REFINE_SEED)),
                "np_seed_perturbed": np.int64(seed_p), "np_seed_unperturbed": np.int64(seed_n),
                "depth_shift": np.float32(shift), "miss_sample_num": np.int64(MISS_SAMPLE_NUM),
                "param_stride": np.int64(PARAM_STRIDE), "epoch": np.int64(EPOCH), "full_rgb_feat": feat.numpy()}
        for k in ("rgb", "xyz", "xyz_corrupt", "depth_corrupt", "corrupt_mask", "valid_mask"):
            main["batch_" + k] = batch[k].numpy()
        main["intr"] = torch.stack([batch[k].float() for k in ("fx", "fy", "cx", "cy")], 1).numpy()
        params = {}
        for name, perturbed, loss_kw in cases:
            pl, lidf, refine, opt = build(s1, rseed, loss_kw, overrides)
            np_seed = seed_p if perturbed else seed_n
            dd, loss1 = stage1(lidf, batch, feat, np_seed)
            checks = {}
            dd, loss = run_refine(pl, refine, dd, checks)
            bad = conditions(dd, bool(loss_kw.get("hard_neg")), checks)
            assert not bad, (name, bad)
            assert (checks["noise"] is not None) == perturbed
            assert all(p.grad is None for p in lidf.parameters())
            for k in ("miss_bid", "miss_flat_img_id", "gt_pos", "max_pair_id", "occ_vox_intersect_idx",
                      "miss_ray_intersect_idx", "pred_pos", "pred_pos_refine", "voxel_bound"):
                main["%s_%s" % (name, k)] = dd[k].detach().numpy()
            main[name + "_np_seed"] = np.int64(np_seed)
            main[name + "_noise"] = np.float64(float("nan") if checks["noise"] is None else checks["noise"])
            main[name + "_end_voxel_id"] = checks["end_voxel_id"].numpy()
            main[name + "_loss_stage1"] = np.array([float(loss1[k].detach()) for k in LOSS_KEYS], dtype=np.float32)
            main[name + "_loss"] = np.array([float(loss[k].detach()) for k in REFINE_LOSS_KEYS], dtype=np.float32)
            main[name + "_min_preact"] = np.float32(checks["min_preact"])
            main[name + "_min_preact_pnet"] = np.float32(checks["min_preact_pnet"])
            main[name + "_g_pred_pos_refine"] = dd["pred_pos_refine"].grad.numpy()
            for mod in ("pnet_model", "offset_dec"):
                for k, p in getattr(refine, mod).named_parameters():
                    params["%s_g_%s.%s" % (name, mod, k)] = strided(p.grad).numpy().copy()
            if verbose:
                print("%s %s: R=%d P=%d noise=%s loss_net=%.6f min|preact|=%.3g (PointNet %.3g)" % (
                    tag, name, dd["total_miss_sample_num"], dd["miss_ray_intersect_idx"].shape[0], checks["noise"],
                    float(loss["loss_net"].detach()), checks["min_preact"], checks["min_preact_pnet"]))
        return main, params
    raise SystemExit("%s: no configuration satisfies the conditions" % tag)


def write(main, params):
    save_npz(os.path.join(HERE, "g10_refine_train.npz"), main)
    save_npz(os.path.join(HERE, "g10_refine_train_params.npz"), params)


if __name__ == "__main__":
    main, params = generate()
    write(main, params)
    for f in ("g10_refine_train.npz", "g10_refine_train_params.npz"):
        size = os.path.getsize(os.path.join(HERE, f))
        print("%-30s %8d bytes" % (f, size))
        assert size < (1 << 20), f
