"""The float64 twins that the any-width training tests rest on, run on the inputs of the reference's own training steps
at other widths (tests/golden/g15_train_widths.npz, g16_refine_train_widths.npz; tests only, CPU).

  stage1_twin  the stage-1 composite of tests/test_train_widths_gpu.py (_oracle: orc.query with the differentiable
               RoIAlign of tests/roi_ref.py) behind orc.pointnet2stage and in front of train_loss_ref.loss_ref, under
               torch autograd from full_rgb_feat and every parameter
  stage2_twin  refine_widths_ref.chain in front of refine_loss_ref.refine_loss_ref, under autograd

Everything is rebuilt from the fixture's batch, its sampled rays and its seeds; the pair lists, voxel bounds and labels
that the twins derive on the way are asserted equal to the fixture's. tests/test_golden_widths.py holds the twins'
float32 evaluation to the fixture; tests/test_golden_widths_gpu.py then uses their float64 evaluation as the centre."""
import functools

import numpy as np
import torch

import refine_loss_ref as rl
import refine_widths_ref as rw
import train_loss_ref as tl
from util import (assert_f64_close, closed_form, closed_form_params, closed_form_pointnet, inv_out_act, k_for,
                  oracle_grads, orc)

# make_golden_widths.CONFIGS as the oracle and the product take them (r_*: stage 2)
G14 = {"A": dict(gf=32, rgb_out=16, roi_out=3, pnet_out=64, pnet_gf=16, n_iter=2, pos_rel=True,
                 r_gf=32, r_n_iter=3, r_pos_rel=True, r_pnet_pos_rel=False, r_pnet_out=64, r_pnet_gf=16),
       "B": dict(gf=128, rgb_out=32, roi_out=2, pnet_out=128, pnet_gf=32, n_iter=2, pos_rel=False,
                 r_gf=32, r_n_iter=2, r_pos_rel=False, r_pnet_pos_rel=True, r_pnet_out=128, r_pnet_gf=32)}


def strided(t, stride):
    """make_golden_train.strided: a gradient of more than 4096 elements is stored at every stride-th element."""
    t = t.reshape(-1)
    return t[::stride] if t.numel() > 4096 else t


def close_rule(got, fix):
    """tests/test_train_step_gpu.py::_close's rule as a predicate: within 2e-4 of the fixture tensor's own largest
    entry, no floor — for the tensors of a training step that have no float64 twin. Returns (ok, err, scale)."""
    scale = fix.abs().max().item()
    err = (got.detach().cpu().double() - fix.double()).abs().max().item()
    return err <= 2e-4 * scale, err, scale


def widths_D(cfg):
    roi = cfg["rgb_out"] * cfg["roi_out"] ** 2
    return cfg["pnet_out"] + roi + 2 * 51 + 27, cfg["r_pnet_out"] + roi + 51 + 27


def widths_params(cfg, seeds, factors, D):
    """(pnet, prob, off, refine pnet, refine off) closed-form state dicts of a g14 / g15 / g16 configuration; seeds and
    factors in the order (prob_dec, offset_dec, pnet_model, refine offset_dec, refine pnet_model)."""
    sp, so, spn, sr, srp = (int(v) for v in seeds)
    fp, fo, _, fr, _ = (float(v) for v in factors)
    return (closed_form_pointnet(spn, out=cfg["pnet_out"], gf=cfg["pnet_gf"]),
            closed_form_params("IMNET", int(D[0]), seed=sp, gf=cfg["gf"], factor=fp),
            closed_form_params("IEF", int(D[0]), seed=so, gf=cfg["gf"], factor=fo),
            closed_form_pointnet(srp, out=cfg["r_pnet_out"], gf=cfg["r_pnet_gf"]),
            closed_form_params("IEF", int(D[1]), seed=sr, gf=cfg["r_gf"], factor=fr))


def _geometry(g, d):
    """The train flavour of the geometry on the fixture's batch and sampled rays, through the oracle: the valid points,
    the occupied voxels, the rays' directions and pixels and the ray-major pair list. d: tl.g9_case's / rl.g10_case's
    dict. Asserts the voxel bounds and the pair list equal to the fixture's."""
    bs, h, w = d["bs"], d["h"], d["w"]
    rgb, xyzc = torch.from_numpy(g["batch_rgb"]), torch.from_numpy(g["batch_xyz_corrupt"])
    valid_mask = torch.from_numpy(g["batch_valid_mask"]).squeeze(1)
    vidx = torch.nonzero(valid_mask.reshape(bs, -1), as_tuple=False)
    valid_xyz = xyzc.permute(0, 2, 3, 1).reshape(bs, -1, 3)[vidx[:, 0], vidx[:, 1]]
    valid_rgb = rgb.permute(0, 2, 3, 1).reshape(bs, -1, 3)[vidx[:, 0], vidx[:, 1]]
    occ = orc.occupied_voxels(valid_xyz, vidx[:, 0])
    assert torch.equal(occ["voxel_bound"], d["voxel_bound"])
    intr = torch.from_numpy(g["intr"])
    dirs, pix = orc.ray_dirs(intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], h, w)
    bid, flat = d["miss_bid"], d["miss_flat"]
    ray_dir = dirs.reshape(bs, h * w, 3)[bid, flat]
    ray_pix = pix.reshape(bs, h * w, 2)[bid, flat]
    mask, dist = orc.ray_aabb(ray_dir.numpy(), occ["voxel_bound"].numpy(), bid.numpy(), occ["occ_vox_bid"].numpy())
    pair_ray, pair_vox, pair_t, pair_off = orc.pairs_from_dense(mask, dist)
    R, P = bid.shape[0], pair_ray.shape[0]
    perm = torch.argsort(pair_vox * R + pair_ray, stable=True)       # ray-major -> the reference's voxel-major order
    assert torch.equal(pair_ray[perm], d["pair_ray"]) and torch.equal(pair_vox[perm], d["pair_vox"])
    vb = occ["voxel_bound"]
    return dict(occ=occ, valid_xyz=valid_xyz, valid_rgb=valid_rgb, rgb=rgb, ray_dir=ray_dir, ray_pix=ray_pix, ray_bid=bid,
                ray_flat=flat, pair_ray=pair_ray, pair_vox=pair_vox, pair_t=pair_t, pair_off=pair_off, perm=perm, R=R,
                P=P, vox_center=((vb[:, :3] + vb[:, 3:]) / 2.0).contiguous(),
                pnet_inp=torch.cat((occ["valid_v_rel_coord"], valid_rgb[occ["valid_v_pid"]]), -1))


def _to_ray_major(mid, perm, P):
    """A max_pair_id in the reference's voxel-major pair order as an index into the ray-major list (P stays P)."""
    return torch.where(mid < P, perm[mid.clamp(max=P - 1)], torch.full_like(mid, P))


def _leaves(p, dt):
    return {k: v.detach().to(dt, copy=True).requires_grad_(True) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def stage1_twin(name, double, cfg_name="A"):
    """The stage-1 composite on one g15 case at dtype float64 / float32: {pred_pos, pred_prob_end (the reference's
    pair order), loss [8], g_pred_pos, g_pred_prob_end, g_full_rgb_feat, g_<module>.<parameter> (whole tensors)}."""
    from test_golden_widths import g15_files
    from test_train_widths_gpu import _oracle
    g, _ = g15_files()
    cfg = G14[cfg_name]
    dt = torch.float64 if double else torch.float32
    d, _ = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    geo = _geometry(g, d)
    gt_pos, label, want = tl.compute_gt_ref(d["xyz_flat"], d["miss_bid"], d["miss_flat"], d["voxel_bound"],
                                            d["pair_ray"], d["pair_vox"])
    assert torch.equal(gt_pos, d["gt_pos"]) and torch.equal(label.long(), d["pcl_label"].long())
    sp, so, sn = (int(v) for v in g["seeds"])
    pnet_p, prob_p, off_p, _, _ = widths_params(cfg, (sp, so, sn, 31, 43), (1.0,) * 5, widths_D(cfg))
    pn, pp, pq = _leaves(pnet_p, dt), _leaves(prob_p, dt), _leaves(off_p, dt)
    feat = torch.from_numpy(g["full_rgb_feat"]).to(dt, copy=True).requires_grad_(True)
    vox_feat = orc.pointnet2stage(pn, geo["pnet_inp"].to(dt), geo["occ"]["revidx"], geo["occ"]["voxel_bound"].shape[0])
    mid = _to_ray_major(d["max_pair_id"], geo["perm"], geo["P"]) if epoch < 6 else None   # (maxpool_label_epo 6)
    s = dict(ray_dir=geo["ray_dir"], ray_pix=geo["ray_pix"], ray_bid=geo["ray_bid"], pair_ray=geo["pair_ray"],
             pair_vox=geo["pair_vox"], pair_t=geo["pair_t"], pair_off=geo["pair_off"], vox_center=geo["vox_center"])
    qcfg = (cfg["rgb_out"], cfg["roi_out"], cfg["pnet_out"], cfg["gf"], "IEF", 8, 4, cfg["pos_rel"])
    res = _oracle(qcfg, s, dt, mid, cfg["n_iter"], False, leaves=(pp, pq, feat, vox_feat))
    inv = torch.empty_like(geo["perm"])
    inv[geo["perm"]] = torch.arange(geo["P"])
    got_mid = res["max_pair_id"]
    got_mid = torch.where(got_mid < geo["P"], inv[got_mid.clamp(max=geo["P"] - 1)], torch.full_like(got_mid, geo["P"]))
    assert torch.equal(got_mid, d["max_pair_id"])
    c = dict(d)
    c["pred_pos"], c["pred_prob_end"] = res["pred_pos"], res["pred_prob_end"][geo["perm"]]
    c["pred_pos"].retain_grad(), c["pred_prob_end"].retain_grad()
    loss = tl.loss_ref(c, epoch, **opt)
    loss["loss_net"].backward()
    out = {"pred_pos": c["pred_pos"].detach(), "pred_prob_end": c["pred_prob_end"].detach(),
           "loss": torch.stack([loss[k].detach().reshape(()) for k in tl.LOSS_KEYS]),
           "g_pred_pos": c["pred_pos"].grad, "g_pred_prob_end": c["pred_prob_end"].grad, "g_full_rgb_feat": feat.grad}
    for mod, leaves in (("pnet_model", pn), ("prob_dec", pp), ("offset_dec", pq)):
        out.update({"g_%s.%s" % (mod, k): v.grad for k, v in leaves.items()})
    return out


@functools.lru_cache(maxsize=None)
def stage2_twin(cfg_name, name, double):
    """refine_widths_ref.chain + refine_loss_ref on one g16 case, started from the fixture's stage-1 pred_pos and
    max_pair_id: {pred_pos_refine, end_voxel_id, loss [6], g_pred_pos_refine, g_<module>.<parameter>}."""
    from test_golden_widths import g16_files
    g, _ = g16_files(cfg_name)
    cfg = G14[cfg_name]
    dt = torch.float64 if double else torch.float32
    d, ref = rl.g10_case(g, name)
    geo = _geometry(g, d)
    occ = geo["occ"]
    seeds = tuple(int(v) for v in g["seeds_stage1"]) + tuple(int(v) for v in g["seeds_refine"])
    _, _, _, pnetr_p, offr_p = widths_params(cfg, seeds, (1.0,) * 5, widths_D(cfg))
    valid_inp = geo["pnet_inp"] if cfg["r_pnet_pos_rel"] else \
        torch.cat((geo["valid_xyz"][occ["valid_v_pid"]], geo["pnet_inp"][:, 3:]), -1)
    case = dict(cfg=(cfg["rgb_out"], cfg["roi_out"], cfg["r_pnet_out"], cfg["r_pnet_gf"], cfg["r_gf"], "IEF",
                     cfg["r_n_iter"], 8, 4),
                pnet_p=pnetr_p, off_p=offr_p, pred_pos=d["pred_pos"], feat_grid=torch.from_numpy(g["full_rgb_feat"]),
                ray_dir=geo["ray_dir"], ray_pix=geo["ray_pix"], ray_bid=geo["ray_bid"], ray_flat=geo["ray_flat"],
                noise=0.0 if ref["noise"] is None else ref["noise"], max_pair_id=d["max_pair_id"],
                pair_vox=d["pair_vox"], voxel_bound=d["voxel_bound"], voxel_bid=occ["occ_vox_bid"], rgb_img=geo["rgb"],
                valid_inp=valid_inp, valid_vox=occ["revidx"])
    leaves = {}
    pos, evs = rw.chain(case, dt, 2, cfg["r_pos_rel"], cfg["r_pnet_pos_rel"], leaves=leaves)
    c = dict(d)
    c["pred_pos_refine"] = pos
    pos.retain_grad()
    loss = rl.refine_loss_ref(c, int(g["epoch"]), **rl.G10_CASES[name])
    loss["loss_net"].backward()
    out = {"pred_pos_refine": pos.detach(), "end_voxel_id": evs[-1],
           "loss": torch.stack([loss[k].detach().reshape(()) for k in rl.REFINE_LOSS_KEYS]), "g_pred_pos_refine": pos.grad}
    for k, v in leaves.items():
        if k.startswith("pnet."):
            out["g_pnet_model." + k[5:]] = v.grad
        elif k.startswith("dec."):
            out["g_offset_dec." + k[4:]] = v.grad
    return out


def fixture_tensors(g, gp, name, keys):
    """{key: fixture tensor} of one g15 / g16 case: the listed main-file keys and every stored parameter gradient."""
    out = {k: torch.from_numpy(np.asarray(g["%s_%s" % (name, k)])) for k in keys}
    out.update({k[len(name) + 1:]: torch.from_numpy(np.asarray(v)) for k, v in gp.items() if k.startswith(name + "_g_")})
    return out


def twin_in_fixture_form(twin, stride):
    """A twin's results as the fixture stores them: parameter gradients flattened and strided."""
    return {k: (strided(v, stride) if k.startswith("g_") and "." in k else v) for k, v in twin.items()}


# ------------------------------------------------------------------------------------- the training steps' comparison
ZERO_BIAS = "g_prob_dec.linear_4.bias"


def step_form(t, tl_keys):
    """A case's tensors as hold_step takes them: the loss vector split into one entry per loss ("loss:<name>"), so that
    a small loss is not measured in units of a large one."""
    names = tl.LOSS_KEYS if tl_keys else rl.REFINE_LOSS_KEYS
    out = {k: v for k, v in t.items() if k != "loss"}
    out.update({"loss:" + n: t["loss"][i].reshape(1) for i, n in enumerate(names)})
    return out


def hold_one(what, key, got, twin64, unit, report=None):
    """assert_f64_close(got, float64 twin on the fixture's inputs, unit) for one tensor of a training step, k_for for a
    parameter gradient. unit: the reference's own float32 run (GPU tests) or the twin's float32 run (CPU tests)."""
    k = k_for(key[2:]) if key.startswith("g_") and "." in key else 4.0
    got = got.detach().cpu()
    return assert_f64_close("%s %s" % (what, key), got.reshape(twin64.shape), twin64, unit.reshape(twin64.shape),
                            k=k, report=report)


def hold_step(what, got, twin64, unit, pairs=None, report=None):
    """hold_one over every tensor of a step (dicts in step_form). prob_dec's last bias: its true value is 0, both sides
    are the rounding of a cancellation, held by tests/test_train_step_gpu.py::_zero_bias_bound over `pairs` pairs."""
    for key in sorted(k for k in twin64 if k != "end_voxel_id"):   # (every tensor the twin gives: a missing key raises)
        if key == ZERO_BIAS:
            from test_train_step_gpu import _zero_bias_bound
            bound = _zero_bias_bound(pairs)
            print("%s %s: got %.3g, unit %.3g, bound %.3g" % (what, key, float(got[key]), float(unit[key]), bound))
            assert abs(float(got[key])) <= bound and abs(float(unit[key])) <= bound
            continue
        hold_one(what, key, got[key], twin64[key], unit[key], report)


# ------------------------------------------------------------------------- g2 / g5 under the strengthened comparison
@functools.lru_cache(maxsize=None)
def g2_oracle():
    """{key: (fixture, oracle float64 output, use_sigmoid)} of g2_decoders.npz."""
    from test_oracle_golden import g2_cases, load
    g = load("g2_decoders.npz")
    out = {}
    for key, kind, d, sig, seed in g2_cases(g):
        p = closed_form_params(kind, d, seed=seed)
        x = closed_form((256, d), 0.5698402910, 0.1 * d, 1.0)
        with torch.no_grad():
            y64 = orc.decoder_forward({k: v.double() for k, v in p.items()}, x.double(), kind, 2, sig)
        out[key] = (torch.from_numpy(g[key]), y64, sig)
    return out


def g2_close(key, got, fix, y64, sig, report=None):
    """test_g2_decoders_hip's added comparison: against the float64 oracle, the reference's float32 output as the unit,
    logits (through the clamp's inverse) where there is no sigmoid."""
    through = (lambda t: t) if sig else inv_out_act
    return assert_f64_close("g2 " + key, through(got), through(y64), through(fix), report=report)


@functools.lru_cache(maxsize=None)
def g5_oracle():
    """{key: {name: (fixture, oracle float64)}} of the g5 files: y, g_input, g_<parameter>."""
    from test_oracle_golden import G5, g5_cases, g5_inputs, load
    g = load(*G5)
    out = {}
    for key, kind, d, n_iter, sig, seed in g5_cases(g):
        x, wgt = g5_inputs(d)
        y, grads = oracle_grads(closed_form_params(kind, d, seed=seed), x, kind, wgt[:, 0], torch.float64, n_iter, sig)
        case = out[key] = {"y": (torch.from_numpy(g[key + "_y"]), y)}
        case["g_input"] = (torch.from_numpy(g[key + "_g_input"]), grads.pop("input"))
        for k, v in grads.items():
            case["g_" + k] = (torch.from_numpy(g[key + "_g_" + k]), v)
    return out


def g5_close(key, name, got, fix, o64, sig, report=None):
    """test_g5_decoder_grads_hip's added comparison (parameter gradients: k_for)."""
    through = inv_out_act if (name == "y" and not sig) else (lambda t: t)
    k = k_for(name[2:]) if name.startswith("g_") and name != "g_input" else 4.0
    return assert_f64_close("g5 %s %s" % (key, name), through(got), through(o64), through(fix), k=k, report=report)

