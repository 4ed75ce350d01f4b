"""make_golden_train.py — the stage-1 TRAINING step of the reference as golden vectors.

Run in the authoring container only (it imports /root/reference/src):   python tests/golden/make_golden_train.py
Runs the reference's own LIDF.forward(batch, 'train', epoch) (models/pipeline.py:652-711) with train_lidf.yaml on a
two-frame 16 x 24 batch like g3's and stores its inputs and outputs; nothing of the reference is copied. The stubs of
make_golden.py stand in for cv2 / torchvision / torch_scatter / the two JIT extensions, as for g3.

  g9_train_step.npz         the batch, full_rgb_feat, the seeds, and per case: the sampled rays, gt_pos, pcl_label,
                            max_pair_id (the reference's voxel-major pair order), pred_pos, pred_prob_end, the eight
                            loss_dict values, and after loss_net.backward() the gradients of pred_pos, pred_prob_end
                            (retain_grad) and full_rgb_feat
  g9_train_step_params.npz  per case the gradient of every prob_dec / offset_dec / pnet_model parameter. A committed
                            file stays under 1 MiB, and the four cases' parameter gradients are 1.4 M floats: tensors
                            of more than 4096 elements are stored at every PARAM_STRIDE-th element of their flattened
                            form (11 is coprime to every dimension, so every row and column is visited), the rest whole

Cases: epoch 0 (pairs selected by the labels) and epoch 6 (by the arg-max of the logits), each with loss.hard_neg
False and True (hard_neg_ratio 0.1). grid.valid_sample_num = -1; grid.miss_sample_num = 24, so that the random window
of get_miss_ray is active in frame 1 (35 corrupt pixels) and inactive in frame 0 (18); np.random.seed fixed.

The generator asserts what makes the fixture pin the algorithm and not a coin flip of float32 rounding (a search over
the decoders' weight seeds, the face ray and a small depth shift finds a configuration that satisfies all of it):
  no hidden (leaky-ReLU) pre-activation of the two decoders within 2e-5 of 0 (as g5_decoder_grads; the PointNet's
  240,000 ReLU pre-activations cannot all be kept that far from 0 — about 20 of them fall inside at any seed — so their
  minimum is recorded as min_preact_pnet and not asserted); in the epoch-6 cases every ray's two largest logits more than 1e-4 apart; no gt_pos coordinate within 1e-5 of a voxel face,
  except ONE ray put on a face shared by two occupied voxels on purpose (two labels); the k-th and (k+1)-th value of
  every top-k more than 1e-6 apart (relative); away from the last row and column no sampled pixel's normal shorter than
  1e-4; at least one ray with pairs and no label, one ray without pairs, sampled pixels in the last row and the last
  column, and sampled pixels whose right or lower neighbour is not sampled.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# (importing the existing generator puts the repository, tests/ and the reference on sys.path)
from make_golden import REF, closed_form, closed_form_params, closed_form_pointnet, install_stubs, orc  # noqa: E402

PARAM_STRIDE = 11
MISS_SAMPLE_NUM = 24
NP_SEED = 2024
CASES = (("e0", 0, False), ("e0_hn", 0, True), ("e6", 6, False), ("e6_hn", 6, True))
FACE_FRAME = 1   # the frame in whose hole one ray's ground truth is put on a shared voxel face
HOLES = ((13, 16, 18, 24), (2, 7, 10, 17))   # per frame: rows y0:y1, columns x0:x1 of the corrupt pixels


def make_batch(shift, face):
    """g3's recipe (two slanted planes seen by two pinhole cameras) with holes that reach the last row and column of
    frame 0 (its corner rays meet no occupied voxel) and `shift` added to the depth. face = (frame, y, x, axis, value): that pixel's ground-truth point is moved along its ray to where its
    coordinate `axis` is exactly `value` (a voxel face)."""
    B, h, w = 2, 16, 24
    fx = torch.tensor([21.6, 20.0], dtype=torch.float64)
    fy = torch.tensor([21.6, 22.0], dtype=torch.float64)
    cx = torch.tensor([11.5, 12.25], dtype=torch.float64)
    cy = torch.tensor([7.5, 7.0], dtype=torch.float64)
    d, _ = orc.ray_dirs(fx.float(), fy.float(), cx.float(), cy.float(), h, w)
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    depth = torch.stack((0.9 + 0.01 * xs + 0.005 * ys, 1.3 - 0.012 * xs + 0.02 * ys), 0) + shift
    xyz = (d / d[..., 2:3] * depth.unsqueeze(-1)).permute(0, 3, 1, 2).contiguous()
    b, y, x, axis, value = face
    xyz[b, :, y, x] = d[b, y, x] / d[b, y, x, axis] * value
    hole = torch.zeros(B, 1, h, w)
    for f, (y0, y1, x0, x1) in enumerate(HOLES):   # frame 0: 18 pixels up to the last row and column; frame 1: 35
        hole[f, :, y0:y1, x0:x1] = 1
    valid = 1 - hole
    return {
        "rgb": closed_form((B, 3, h, w), 0.3819660113, 0.2, 1.5),
        "xyz": xyz, "xyz_corrupt": xyz * (1 - hole), "depth_corrupt": depth.unsqueeze(1) * (1 - hole),
        "corrupt_mask": hole.clone(), "valid_mask": valid,
        "fx": fx, "fy": fy, "cx": cx, "cy": cy, "item_path": ["a", "b"],
    }


class FixedFeatures(torch.nn.Module):
    """Stands in for the ResNet inside LIDF.get_embedding: returns the stored full_rgb_feat as a leaf."""

    def __init__(self, feat):
        super().__init__()
        self.feat = feat

    def forward(self, rgb):
        return self.feat


PNET_SEED = 41


def apply_overrides(opt, overrides):
    """overrides: {"model.imnet_gf": 32, "refine.pnet_pos_type": "abs", ...} set on the reference's Params (a
    stage-1 yaml has no refine section: those entries do not apply to it)."""
    for path, value in (overrides or {}).items():
        node = opt
        *parents, leaf = path.split(".")
        if not hasattr(opt, parents[0]):
            continue
        for name in parents:
            node = getattr(node, name)
        assert hasattr(node, leaf), path
        setattr(node, leaf, value)


def load_stage1(lidf, seeds, factor=1.0):
    """Closed-form weights at the widths the options give the three stage-1 modules; seeds = (prob_dec, offset_dec,
    pnet_model). factor: closed_form_params' factor for the two decoders."""
    m = lidf.opt.model
    D = lidf.prob_dec.inp_dim
    lidf.prob_dec.load_state_dict(closed_form_params("IMNET", D, seed=seeds[0], gf=m.imnet_gf, factor=factor))
    lidf.offset_dec.load_state_dict(closed_form_params(m.offdec_type, D, seed=seeds[1], gf=m.imnet_gf, factor=factor))
    lidf.pnet_model.load_state_dict(closed_form_pointnet(seeds[2], cin=m.pnet_in, out=m.pnet_out, gf=m.pnet_gf))


def build(seeds, hard_neg, overrides=None):
    """The reference's LIDF with train_lidf.yaml (+ overrides, see apply_overrides) and closed-form weights;
    seeds = (prob_dec, offset_dec)."""
    import models.pipeline as pl
    from opt import Params
    cfg = os.path.join(REF, "experiments", "implicit_depth")
    opt = Params(os.path.join(cfg, "default_config.yaml"))
    opt.update(os.path.join(cfg, "train_lidf.yaml"))
    opt.dist.ddp = False
    opt.grid.valid_sample_num = -1
    opt.grid.miss_sample_num = MISS_SAMPLE_NUM
    opt.loss.hard_neg, opt.loss.hard_neg_ratio = hard_neg, 0.1
    apply_overrides(opt, overrides)
    torch.manual_seed(1234)
    lidf = pl.LIDF(opt, torch.device("cpu")).eval()
    load_stage1(lidf, (seeds[0], seeds[1], PNET_SEED))
    return lidf, opt


def run_case(lidf, batch, feat, epoch, checks):
    """One LIDF.forward(batch, 'train', epoch) + loss_net.backward(); `checks` collects the asserted quantities."""
    leaf = feat.clone().requires_grad_(True)
    lidf.resnet_model = FixedFeatures(leaf)
    lidf.zero_grad()
    pre, pre_pnet = [], []
    hooks = [m.register_forward_hook(lambda mod, i, o: pre.append(o.detach().abs().min().item()))
             for net in (lidf.prob_dec, lidf.offset_dec) for m in (net.linear_1, net.linear_2, net.linear_3)]
    hooks += [m.register_forward_hook(lambda mod, i, o: pre_pnet.append(o.detach().abs().min().item()))
              for m in lidf.pnet_model.children()]
    inner = lidf.compute_loss

    def compute_loss(dd, exp_type, ep):
        dd["pred_pos"].retain_grad(), dd["pred_prob_end"].retain_grad()
        return inner(dd, exp_type, ep)
    lidf.compute_loss = compute_loss
    np.random.seed(NP_SEED)
    ok, dd, loss = lidf(batch, "train", epoch)
    lidf.compute_loss = inner
    for hk in hooks:
        hk.remove()
    assert ok
    loss["loss_net"].backward()
    checks["min_preact"], checks["min_preact_pnet"] = min(pre), min(pre_pnet)
    return dd, loss, leaf.grad


def topk_gap(v, ratio=0.1):
    k = int(v.shape[0] * ratio)
    s = torch.sort(v.double(), descending=True)[0]
    if k == 0 or k >= s.shape[0]:
        return 1.0
    return ((s[k - 1] - s[k]).abs() / max(s[k - 1].abs().item(), 1e-30)).item()


def conditions(dd, opt, epoch, hard_neg, checks):
    """The asserted properties of one case; returns a list of the violated ones."""
    bad = []
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    R = dd["total_miss_sample_num"]
    ray, label = dd["miss_ray_intersect_idx"], dd["pcl_label"]
    n_pair = torch.bincount(ray, minlength=R)
    n_lab = torch.bincount(ray, weights=label.double(), minlength=R)
    bid, flat = dd["miss_bid"], dd["miss_flat_img_id"]
    fb, fy_, fx_ = checks["face"][:3]
    face = ((bid == fb) & (flat == fy_ * w + fx_)).nonzero().reshape(-1)
    if checks["min_preact"] <= 2e-5:
        bad.append("pre-activation %.3g" % checks["min_preact"])
    if checks["min_preact_pnet"] == 0.0:   # (a ReLU exactly at its kink: its derivative is a convention)
        bad.append("a PointNet pre-activation is exactly 0")
    if face.numel() != 1 or int(n_lab[face[0]]) != 2:
        bad.append("face ray labels %s" % (n_lab[face].tolist(),))
    if int(n_lab.max()) > 2 or int(((n_lab == 2)).sum()) != 1:
        bad.append("rays with two labels: %d" % int((n_lab >= 2).sum()))
    if not bool(((n_pair > 0) & (n_lab == 0)).any()):
        bad.append("no ray with pairs and without label")
    if not bool((n_pair == 0).any()):
        bad.append("no ray without pairs")
    # distance of every gt coordinate to the voxel faces (a lattice of spacing part_size from xmin)
    part = dd["part_size"]
    g = dd["gt_pos"].double()
    off = (g - dd["xmin"].double()) / part
    dist = ((off - off.round()).abs() * part)
    keep = torch.ones(R, dtype=torch.bool)
    keep[face] = False
    if dist[keep].min().item() <= 1e-5:
        bad.append("gt_pos %.3g from a face" % dist[keep].min().item())
    if epoch >= opt.model.maxpool_label_epo:
        lg = dd["pred_prob_end"].detach()[:, 0].double()
        for r in range(R):
            v = torch.sort(lg[ray == r], descending=True)[0]
            if v.numel() > 1 and (v[0] - v[1]).item() <= 1e-4:
                bad.append("ray %d logit gap %.3g" % (r, (v[0] - v[1]).item()))
    y, x = flat // w, flat % w
    sampled = torch.zeros(bs, h * w, dtype=torch.bool)
    sampled[bid, flat] = True
    if not bool((y == h - 1).any()) or not bool((x == w - 1).any()):
        bad.append("no sampled pixel in the last row / column")
    right = sampled[bid, (flat + 1).clamp(max=h * w - 1)] | (x == w - 1)
    below = sampled[bid, (flat + w).clamp(max=h * w - 1)] | (y == h - 1)
    if bool(right.all()) or bool(below.all()):
        bad.append("every right / lower neighbour is sampled")
    # normals: recomputed here from the stored frame (the cross product before its normalisation)
    inner = (y < h - 1) & (x < w - 1)
    unit, sq = [], []
    for pos in (dd["gt_pos"], dd["pred_pos"].detach()):
        img = dd["xyz_flat"].clone()
        img[bid, flat] = pos
        img = img.reshape(bs, h, w, 3).double()
        dx = torch.zeros_like(img)
        dy = torch.zeros_like(img)
        dx[:, :, :-1] = img[:, :, 1:] - img[:, :, :-1]
        dy[:, :-1] = img[:, 1:] - img[:, :-1]
        n = torch.linalg.cross(dx, dy, dim=-1).reshape(bs, h * w, 3)[bid, flat]
        nrm = n.norm(dim=-1)
        if nrm[inner].min().item() < 1e-4:
            bad.append("normal of length %.3g" % nrm[inner].min().item())
        unit.append(n / (nrm.unsqueeze(-1) + 1e-8))
        sq = [(dx * dx).sum(-1).reshape(bs, h * w)[bid, flat], (dy * dy).sum(-1).reshape(bs, h * w)[bid, flat]]
    if hard_neg:
        d = (dd["pred_pos"].detach() - dd["gt_pos"]).abs().mean(-1)
        lsm = torch.log(orc.scatter_softmax(dd["pred_prob_end"].detach()[:, 0], ray, R))
        cos = torch.nn.functional.cosine_similarity(unit[1], unit[0], dim=-1)
        vecs = {"pos": d, "prob": -lsm[label.nonzero().reshape(-1)], "surf_norm": (1 - cos) / 2, "dx": sq[0],
                "dy": sq[1]}
        for name, v in vecs.items():
            if topk_gap(v) <= 1e-6:
                bad.append("top-k gap of %s %.3g" % (name, topk_gap(v)))
    return bad


def find_face(lidf, shift):
    """The first (pixel of FACE_FRAME's hole, voxel face) for which the reference's own compute_gt gives that ray two
    labels and every other ray at most one: the geometry part of LIDF.forward, seeded like the full run."""
    h, w = 16, 24
    y0, y1, x0, x1 = HOLES[FACE_FRAME]
    n = (y1 - y0) * (x1 - x0)
    for y in range(y0, y1):
        for x in range(x0, x1):
            if not n - MISS_SAMPLE_NUM <= (y - y0) * (x1 - x0) + (x - x0) < MISS_SAMPLE_NUM:
                continue   # (only pixels that every position of the random window contains)
            for axis, lo in ((2, -0.125), (0, -1.125), (1, -1.125)):   # the faces: lo + 0.25 k
                for k in range(10):
                    face = (FACE_FRAME, y, x, axis, lo + 0.25 * k)
                    batch = make_batch(shift, face)
                    plane = make_batch(shift, (0, 0, 0, 2, 1.0))["xyz"][FACE_FRAME, 2, y, x]
                    if not bool(((batch["xyz"][FACE_FRAME, 2, y, x] - plane).abs() < 0.25).item()):
                        continue   # (stay near the surface, where voxels are occupied)
                    with torch.no_grad():
                        dd = lidf.prepare_data(batch, "train", None)
                        lidf.get_valid_points(dd)
                        assert lidf.get_occ_vox_bound(dd)
                        np.random.seed(NP_SEED)
                        lidf.get_miss_ray(dd, "train")
                        assert lidf.compute_ray_aabb(dd)
                        lidf.compute_gt(dd)
                    R = dd["total_miss_sample_num"]
                    n_lab = torch.bincount(dd["miss_ray_intersect_idx"], weights=dd["pcl_label"].double(), minlength=R)
                    at = ((dd["miss_bid"] == FACE_FRAME) & (dd["miss_flat_img_id"] == y * w + x)).nonzero().reshape(-1)
                    if at.numel() == 1 and int(n_lab[at[0]]) == 2 and int((n_lab >= 2).sum()) == 1:
                        return face
    return None


def decoder_seeds(lidf, batch, feat):
    """Seeds of the closed-form decoder weights for which no hidden pre-activation over the step's pairs lies within
    2e-5 of 0 and (prob_dec) every ray's two largest logits are more than 1e-4 apart. The decoder input rows do not
    depend on the decoders, so the two searches are independent: the reference's own get_embedding gives the rows."""
    lidf.resnet_model = FixedFeatures(feat)
    with torch.no_grad():
        dd = lidf.prepare_data(batch, "train", None)
        lidf.get_valid_points(dd)
        assert lidf.get_occ_vox_bound(dd)
        np.random.seed(NP_SEED)
        lidf.get_miss_ray(dd, "train")
        assert lidf.compute_ray_aabb(dd)
        lidf.get_embedding(dd)
        rows = torch.cat((dd["intersect_voxel_feat"], dd["intersect_rgb_feat"], dd["intersect_enter_pos_embed"],
                          dd["intersect_leave_pos_embed"], dd["intersect_dir_embed"]), -1)
    ray, R = dd["miss_ray_intersect_idx"], dd["total_miss_sample_num"]
    D = lidf.prob_dec.inp_dim
    found = []
    for net, kind in ((lidf.prob_dec, "IMNET"), (lidf.offset_dec, lidf.opt.model.offdec_type)):
        pre = []
        hooks = [m.register_forward_hook(lambda mod, i, o: pre.append(o.abs().min().item()))
                 for m in (net.linear_1, net.linear_2, net.linear_3)]
        for seed in range(21, 6000):
            net.load_state_dict(closed_form_params(kind, D, seed=seed, gf=lidf.opt.model.imnet_gf))
            del pre[:]
            with torch.no_grad():
                out = net(rows)
            if min(pre) <= 2e-5:
                continue
            if kind == "IMNET":
                lg = out[:, 0].double()
                gaps = [torch.sort(lg[ray == r], descending=True)[0] for r in range(R)]
                if any(v.numel() > 1 and (v[0] - v[1]).item() <= 1e-4 for v in gaps):
                    continue
            found.append(seed)
            break
        else:
            raise SystemExit("g9: no %s seed keeps the pre-activations away from 0" % kind)
        for hk in hooks:
            hk.remove()
    return tuple(found)


def strided(t):
    t = t.reshape(-1)
    return t[::PARAM_STRIDE] if t.numel() > 4096 else t


def differentiable_roi_align():
    """The stub RoIAlign of make_golden.py is a numpy loop without a graph: the oracle's torch form of the same
    operator (equal to float rounding, tests/test_oracle_props.py) lets the gradient reach full_rgb_feat. That form
    is built for 2 x 2 bins; another roi_out_bbox takes its any-size counterpart, tests/roi_ref.py."""
    from roi_ref import roi_align_torch

    def roi_align(inp, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
        return orc.roi_align_fast(inp, boxes) if output_size == 2 else roi_align_torch(inp, boxes, output_size)
    sys.modules["torchvision.ops"].roi_align = roi_align


def candidates(overrides=None, verbose=True, tag="g9"):
    """(shift, face, batch, full_rgb_feat, decoder seeds) per depth shift for which a face ray exists: the geometry
    and the decoder weights of a stage-1 step at the widths of `overrides`, before the step's own conditions."""
    for shift in (0.0, 0.003, 0.007, -0.004, 0.011, -0.009, 0.014, -0.013, 0.018, 0.021):
        probe = build((21, 22), False, overrides)[0]
        face = find_face(probe, shift)
        if face is None:
            continue
        batch = make_batch(shift, face)
        with torch.no_grad():
            feat = probe.resnet_model(batch["rgb"]).detach().clone()
        seeds = decoder_seeds(probe, batch, feat)
        if verbose:
            print("%s: shift %g: face ray (frame, y, x, axis, value) = %s, decoder seeds %s" % (tag, shift, face, seeds))
        yield shift, face, batch, feat, seeds


def setup():
    torch.set_num_threads(1)   # (the scatter-adds of the backward sum in thread order: one thread, one order)
    torch.use_deterministic_algorithms(True)
    install_stubs()
    differentiable_roi_align()


def generate(verbose=True, overrides=None, cases=CASES, tag="g9"):
    setup()
    for shift, face, batch, feat, seeds in candidates(overrides, verbose, tag):
        main = {"seeds": np.array(seeds + (PNET_SEED,)), "np_seed": np.int64(NP_SEED),
                "depth_shift": np.float32(shift), "miss_sample_num": np.int64(MISS_SAMPLE_NUM),
                "face_ray": np.array(face, dtype=np.float64), "param_stride": np.int64(PARAM_STRIDE),
                "full_rgb_feat": feat.numpy()}
        for k in ("rgb", "xyz", "xyz_corrupt", "depth_corrupt", "corrupt_mask", "valid_mask"):
            main["batch_" + k] = batch[k].numpy()
        main["intr"] = torch.stack([batch[k].float() for k in ("fx", "fy", "cx", "cy")], 1).numpy()
        params, bad = {}, []
        for name, epoch, hard_neg in cases:
            lidf, opt = build(seeds, hard_neg, overrides)
            checks = {"face": face}
            dd, loss, g_feat = run_case(lidf, batch, feat, epoch, checks)
            bad += ["%s: %s" % (name, b) for b in conditions(dd, opt, epoch, hard_neg, checks)]
            if bad:
                break
            for k in ("miss_bid", "miss_flat_img_id", "gt_pos", "pcl_label", "max_pair_id",
                      "occ_vox_intersect_idx", "miss_ray_intersect_idx", "pred_pos", "pred_prob_end"):
                main["%s_%s" % (name, k)] = dd[k].detach().numpy()
            main[name + "_voxel_bound"] = dd["voxel_bound"].numpy()
            main[name + "_loss"] = np.array([float(loss[k].detach()) for k in
                                             ("pos_loss", "prob_loss", "surf_norm_loss", "smooth_loss", "loss_net",
                                              "acc", "err", "angle_err")], dtype=np.float32)
            main[name + "_min_preact"] = np.float32(checks["min_preact"])
            main[name + "_min_preact_pnet"] = np.float32(checks["min_preact_pnet"])
            main[name + "_g_pred_pos"] = dd["pred_pos"].grad.numpy()
            main[name + "_g_pred_prob_end"] = dd["pred_prob_end"].grad.numpy()
            main[name + "_g_full_rgb_feat"] = g_feat.numpy()
            for mod in ("prob_dec", "offset_dec", "pnet_model"):
                for k, p in getattr(lidf, mod).named_parameters():
                    params["%s_g_%s.%s" % (name, mod, k)] = strided(p.grad).numpy().copy()
            if verbose:
                print("%s %s: R=%d P=%d labels=%d loss_net=%.6f min|preact|=%.3g (PointNet %.3g)" % (
                    tag, name, dd["total_miss_sample_num"], dd["pcl_label"].shape[0], int(dd["pcl_label"].sum()),
                    float(loss["loss_net"]), checks["min_preact"], checks["min_preact_pnet"]))
        if not bad:
            return main, params
        if verbose:
            print("%s: shift %g rejected: %s" % (tag, shift, "; ".join(bad[:4])))
    raise SystemExit("%s: no configuration satisfies the conditions" % tag)


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member time stamp: regenerating gives the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def write(main, params):
    save_npz(os.path.join(HERE, "g9_train_step.npz"), main)
    save_npz(os.path.join(HERE, "g9_train_step_params.npz"), params)


if __name__ == "__main__":
    main, params = generate()
    write(main, params)
    for f in ("g9_train_step.npz", "g9_train_step_params.npz"):
        size = os.path.getsize(os.path.join(HERE, f))
        print("%-28s %8d bytes" % (f, size))
        assert size < (1 << 20), f
