"""make_golden_valid.py — the EVALUATION flavour of the two losses of the reference as golden vectors.

Run where the reference's sources are (make_golden.REF; it imports them):   python tests/golden/make_golden_valid.py
Runs the reference's own LIDF.forward(batch, 'valid' | 'test', epoch, pred_mask) and RefineNet.forward on the CPU with
train_refine.yaml, on the two-frame 16 x 24 batch recipe of g9 / g10 (make_golden_train.make_batch, g9's depth shift
and face ray, g9's stage-1 weight seeds, g10's stage-2 seeds), and stores the inputs the losses read and the 17- and
15-entry loss_dicts. Nothing of the reference is copied; the stubs of make_golden.py stand in for cv2 / torchvision /
torch_scatter / the two JIT extensions.

  g12_valid_loss.npz   per case: xyz, xyz_corrupt, corrupt_mask of the batch, the queried rays, the pair list in the
                       reference's voxel-major order with voxel_bound, gt_pos, pcl_label, pred_pos, pred_prob_end,
                       pred_pos_refine, loss [17], loss_refine [15], n_stat (the number of elements the nine
                       statistics are taken over); loss_opt = (pos_w, prob_w, surf_norm_w, smooth_w, hard_neg_ratio)

Cases (epoch 0):
  a  bs == 1 (frame 0 of the batch), mask_type 'all', 'valid'   the shipped validation configuration; resize branch
  b  bs == 2, mask_type 'pred' with PRED_BOXES, 'valid'         ray branch; xyz_corrupt_flat is read as the base cloud
  c  as b with hard_neg True, hard_neg_ratio 0.1                hard-negative mining at evaluation
  d  as a, 'test'
One ground-truth point per frame is the zero point (a pixel without ground-truth depth), ZERO_PIX.

The generator asserts what makes the fixture pin the algorithm and not float32 rounding, and searches the depth shifts
of make_golden_train until all of it holds:
  coverage (cases b / c, the only ones with non-queried pixels; the first four in a / d as well): a ray with gt_pos ==
  0; a ray with pairs and no label; a ray without pairs and with nonzero ground truth (its predicted depth is 0: the
  threshold is infinite); queried pixels in the last row and the last column; queried pixels whose right and whose
  lower neighbour is not queried, with xyz_corrupt != xyz at that neighbour;
  no element's threshold max(gt / pred, pred / gt), in float64, within 1e-5 (relative) of 1.05, 1.10 or 1.25;
  the k-th and (k+1)-th value of every top-k more than 1e-6 apart (relative), case c;
  every ray's two largest logits more than 1e-4 apart.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_stubs, orc  # noqa: E402
from make_golden_refine_train import LOSS_KEYS, REFINE_LOSS_KEYS, build  # noqa: E402
from make_golden_train import FixedFeatures, find_face, make_batch, save_npz, topk_gap  # noqa: E402

EPOCH = 0
METRIC_KEYS = ("a1", "a2", "a3", "rmse", "rmse_log", "log10", "abs_rel", "mae", "sq_rel")
# per frame: rows y0:y1, columns x0:x1 of pred_mask (cases b / c). Frame 0: the hole 13:16 x 18:24 plus two rows above
# it (a corrupt pixel left out of pred_mask is a valid point at the origin under mask_type 'pred', whose voxel every
# ray meets: frame 0 keeps none, so that its corner rays stay without pairs); frame 1: the hole 2:7 x 10:17 without
# its last two columns and its last row — their pixels are corrupt (xyz_corrupt = 0) and lie to the right of / below
# queried pixels
PRED_BOXES = ((11, 16, 18, 24), (1, 6, 9, 15))
ZERO_PIX = ((14, 21), (3, 12))   # per frame (y, x): ground truth without depth, inside both masks
HARD_NEG = dict(hard_neg=True, hard_neg_ratio=0.1)
# name -> (frames, mask_type, exp_type, loss overrides)
CASES = (("a", (0,), "all", "valid", {}), ("b", (0, 1), "pred", "valid", {}),
         ("c", (0, 1), "pred", "valid", HARD_NEG), ("d", (0,), "all", "test", {}))


def case_batch(batch, frames):
    out = {}
    for k, v in batch.items():
        out[k] = [v[i] for i in frames] if isinstance(v, list) else v[list(frames)].clone()
    for j, f in enumerate(frames):
        y, x = ZERO_PIX[f]
        out["xyz"][j, :, y, x] = 0.0
    return out


def pred_mask_of(frames, h, w):
    m = torch.zeros(len(frames), h, w)
    for j, f in enumerate(frames):
        y0, y1, x0, x1 = PRED_BOXES[f]
        m[j, y0:y1, x0:x1] = 1
    return m


def statistics_inputs(dd, pred_pos):
    """(gt, pred) float64 of the elements the nine statistics are taken over, by the reference's own rule."""
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    if bs != 1:
        keep = dd["gt_pos"].abs().sum(-1) != 0
        return dd["gt_pos"][keep, 2].double(), pred_pos[keep, 2].double()
    sy = torch.tensor(orc.resize_nearest_index(h, 144))
    sx = torch.tensor(orc.resize_nearest_index(w, 256))
    gt = dd["xyz_flat"].reshape(bs, h, w, 3)[0, :, :, 2][sy][:, sx]
    frame = dd["xyz_corrupt_flat"].clone()
    frame[dd["miss_bid"], dd["miss_flat_img_id"]] = pred_pos
    pred = frame.reshape(bs, h, w, 3)[0, :, :, 2][sy][:, sx]
    mask = (gt > 0) & (dd["corrupt_mask"][0].to(torch.uint8)[sy][:, sx] != 0)
    return gt[mask].double(), pred[mask].double()


def conditions(dd, mask_type, hard_neg):
    bad = []
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    R = dd["total_miss_sample_num"]
    ray, label = dd["miss_ray_intersect_idx"], dd["pcl_label"]
    bid, flat = dd["miss_bid"], dd["miss_flat_img_id"]
    n_pair = torch.bincount(ray, minlength=R)
    n_lab = torch.bincount(ray, weights=label.double(), minlength=R)
    zero = dd["gt_pos"].abs().sum(-1) == 0
    if not bool(zero.any()):
        bad.append("no ray with gt_pos == 0")
    if not bool(((n_pair > 0) & (n_lab == 0)).any()):
        bad.append("no ray with pairs and without label")
    lone = (n_pair == 0) & ~zero
    if not bool(lone.any()) or not bool((dd["pred_pos"][lone, 2] == 0).all()):
        bad.append("no ray without pairs and with nonzero ground truth")
    y, x = flat // w, flat % w
    if not bool((y == h - 1).any()) or not bool((x == w - 1).any()):
        bad.append("no queried pixel in the last row / column")
    if mask_type == "pred":
        queried = torch.zeros(bs, h * w, dtype=torch.bool)
        queried[bid, flat] = True
        differs = (dd["xyz_corrupt_flat"] != dd["xyz_flat"]).any(-1)
        right = (x < w - 1) & ~queried[bid, (flat + 1).clamp(max=h * w - 1)] & differs[bid, (flat + 1).clamp(max=h * w - 1)]
        below = (y < h - 1) & ~queried[bid, (flat + w).clamp(max=h * w - 1)] & differs[bid, (flat + w).clamp(max=h * w - 1)]
        if not bool(right.any()) or not bool(below.any()):
            bad.append("no queried pixel beside a non-queried pixel at which xyz_corrupt != xyz")
    lg = dd["pred_prob_end"].detach()[:, 0].double()
    for r in range(R):
        v = torch.sort(lg[ray == r], descending=True)[0]
        if v.numel() > 1 and (v[0] - v[1]).item() <= 1e-4:
            bad.append("ray %d logit gap %.3g" % (r, (v[0] - v[1]).item()))
    for stage, pred in (("stage 1", dd["pred_pos"]), ("stage 2", dd["pred_pos_refine"])):
        gt, p = statistics_inputs(dd, pred.detach())
        if gt.numel() == 0:
            bad.append("%s: the statistics have no element" % stage)
            continue
        thresh = torch.max(gt / p, p / gt)
        for t in (1.05, 1.10, 1.25):
            gap = ((thresh - t).abs() / t).min().item()
            if gap <= 1e-5:
                bad.append("%s: a threshold %.3g from %g" % (stage, gap, t))
    if hard_neg:
        lsm = torch.log(orc.scatter_softmax(lg.float(), ray, R))
        vecs = {"prob": -lsm[label.nonzero().reshape(-1)]}
        for stage, pred in (("1", dd["pred_pos"].detach()), ("2", dd["pred_pos_refine"].detach())):
            vecs["pos" + stage] = (pred - dd["gt_pos"]).abs().mean(-1)
            unit, sq = [], []
            for pos in (dd["gt_pos"], pred):
                img = dd["xyz_corrupt_flat"].clone()
                img[bid, flat] = pos
                img = img.reshape(bs, h, w, 3).double()
                dx, dy = torch.zeros_like(img), torch.zeros_like(img)
                dx[:, :, :-1] = img[:, :, 1:] - img[:, :, :-1]
                dy[:, :-1] = img[:, 1:] - img[:, :-1]
                n = torch.linalg.cross(dx, dy, dim=-1).reshape(bs, h * w, 3)[bid, flat]
                unit.append(n / (n.norm(dim=-1, keepdim=True) + 1e-8))
                sq = [(dx * dx).sum(-1).reshape(bs, h * w)[bid, flat], (dy * dy).sum(-1).reshape(bs, h * w)[bid, flat]]
            cos = torch.nn.functional.cosine_similarity(unit[1], unit[0], dim=-1)
            vecs.update({"surf" + stage: (1 - cos) / 2, "dx" + stage: sq[0], "dy" + stage: sq[1]})
        for name, v in vecs.items():
            if topk_gap(v) <= 1e-6:
                bad.append("top-k gap of %s %.3g" % (name, topk_gap(v)))
    return bad


def generate(verbose=True):
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    install_stubs()
    sys.modules["torchvision.ops"].roi_align = \
        lambda inp, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False: orc.roi_align_fast(inp, boxes)
    g9 = np.load(os.path.join(HERE, "g9_train_step.npz"))
    g10 = np.load(os.path.join(HERE, "g10_refine_train.npz"))
    s1 = tuple(int(v) for v in g9["seeds"])
    rseed = int(g10["seeds_refine"][0])
    feat = torch.from_numpy(g9["full_rgb_feat"]).clone()
    shifts = [float(g9["depth_shift"])] + [v for v in (0.0, 0.003, 0.007, -0.004, 0.011, -0.009, 0.014, -0.013)
                                            if abs(v - float(g9["depth_shift"])) > 1e-9]
    for shift in shifts:
        if shift == float(g9["depth_shift"]):
            f = g9["face_ray"]
            face = (int(f[0]), int(f[1]), int(f[2]), int(f[3]), float(f[4]))
        else:
            face = find_face(build(s1, rseed, {})[1], shift)
            if face is None:
                continue
        full = make_batch(shift, face)
        # (case a queries every pixel of a frame, 384 rays: g9's prob_dec seed leaves some of their logit pairs
        # closer than 1e-4, so that seed is searched here, from g9's upwards)
        why = {}
        for prob_seed in range(s1[0], s1[0] + 400):
            main, bad = run_cases((prob_seed,) + s1[1:], rseed, feat, full, verbose)
            if not bad:
                main.update({"depth_shift": np.float32(shift), "epoch": np.int64(EPOCH),
                             "seeds_stage1": np.array((prob_seed,) + s1[1:]), "seeds_refine": g10["seeds_refine"]})
                if verbose:
                    print("g12: shift %g, prob_dec seed %d (rejections on the way: %s)" % (shift, prob_seed, why))
                    for name, _, _, _, _ in CASES:
                        print("g12 %s: R=%d P=%d statistics over %d elements, loss_net %.6f / %.6f, a1 %.4f / %.4f" % (
                            name, main[name + "_gt_pos"].shape[0], main[name + "_pcl_label"].shape[0],
                            int(main[name + "_n_stat"]), main[name + "_loss"][4], main[name + "_loss_refine"][3],
                            main[name + "_loss"][8], main[name + "_loss_refine"][6]))
                return main
            key = bad[0].split(" ")[1]
            why[key] = why.get(key, 0) + 1
        if verbose:
            print("g12: shift %g rejected: %s" % (shift, why))
    raise SystemExit("g12: no configuration satisfies the conditions")


def run_cases(s1, rseed, feat, full, verbose):
    """Every case with the stage-1 seeds s1: (the fixture's arrays, the violated conditions of the first failing case)."""
    main = {}
    bad = []
    for name, frames, mask_type, exp_type, loss_kw in CASES:
        pl, lidf, refine, opt = build(s1, rseed, loss_kw)
        opt.mask_type = mask_type
        batch = case_batch(full, frames)
        h, w = batch["xyz"].shape[2:]
        lidf.resnet_model = FixedFeatures(feat[list(frames)].clone())
        pred_mask = pred_mask_of(frames, h, w) if mask_type == "pred" else None
        # the decoders' output activation has slope 0.01 outside [0, 1], and the closed-form prob_dec varies little
        # over a ray's pairs: case a has 384 rays, and some ray's two largest logits lie closer than 1e-4 at every
        # seed. The last layer is rescaled so that the case's logits fill [0.1, 0.9], where the activation is the
        # identity (a first forward measures their range)
        pre = []
        hook = lidf.prob_dec.linear_4.register_forward_hook(lambda mod, i, o: pre.append(o.detach()))
        with torch.no_grad():
            lidf(batch, exp_type, EPOCH, pred_mask)
            hook.remove()
            lo, hi = pre[-1].min(), pre[-1].max()
            scale = 0.8 / (hi - lo)
            lidf.prob_dec.linear_4.weight.mul_(scale)
            lidf.prob_dec.linear_4.bias.copy_((lidf.prob_dec.linear_4.bias - lo) * scale + 0.1)
        with torch.no_grad():
            ok, dd, loss = lidf(batch, exp_type, EPOCH, pred_mask)
            assert ok
            dd, loss_refine = refine(exp_type, EPOCH, dd)
        assert tuple(loss) == LOSS_KEYS + METRIC_KEYS and tuple(loss_refine) == REFINE_LOSS_KEYS + METRIC_KEYS
        bad = ["%s: %s" % (name, b) for b in conditions(dd, mask_type, bool(loss_kw))]
        if bad:
            break
        for k in ("xyz", "xyz_corrupt", "corrupt_mask"):
            main["%s_%s" % (name, k)] = batch[k].numpy()
        for k in ("miss_bid", "miss_flat_img_id", "miss_ray_intersect_idx", "occ_vox_intersect_idx", "voxel_bound",
                  "gt_pos", "pcl_label", "pred_pos", "pred_prob_end", "pred_pos_refine"):
            main["%s_%s" % (name, k)] = dd[k].detach().numpy()
        main[name + "_loss"] = np.array([float(loss[k]) for k in loss], dtype=np.float32)
        main[name + "_loss_refine"] = np.array([float(loss_refine[k]) for k in loss_refine], dtype=np.float32)
        main[name + "_n_stat"] = np.int64(statistics_inputs(dd, dd["pred_pos"])[0].numel())
        main[name + "_loss_opt"] = np.array([opt.loss.pos_w, opt.loss.prob_w, opt.loss.surf_norm_w,
                                             opt.loss.smooth_w, opt.loss.hard_neg_ratio or 0.0], dtype=np.float64)
        if verbose > 1:
            print("g12 %s: R=%d P=%d labels=%d statistics over %d elements, loss_net %.6f / %.6f, a1 %.4f / %.4f" % (
                name, dd["total_miss_sample_num"], dd["pcl_label"].shape[0], int(dd["pcl_label"].sum()),
                int(main[name + "_n_stat"]), float(loss["loss_net"]), float(loss_refine["loss_net"]),
                float(loss["a1"]), float(loss_refine["a1"])))
    return main, bad


if __name__ == "__main__":
    path = os.path.join(HERE, "g12_valid_loss.npz")
    save_npz(path, generate())
    print("%-24s %8d bytes" % (os.path.basename(path), os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)
