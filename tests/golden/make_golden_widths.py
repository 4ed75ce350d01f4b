"""make_golden_widths.py — the reference's own modules at widths other than the shipped configuration.

Run in the authoring container only (it imports the reference, make_golden.REF):   python tests/golden/make_golden_widths.py
Every other fixture here was generated at imnet_gf 64 / rgb_out 32 / roi_out_bbox 2 / pnet_out 128 / pnet_gf 32; the
product also serves other widths (generic.py, lidf_decoder_chain_f32, lidf_frame_widths_f32). These fixtures pin those
routes, and the oracle they are tested with, to the reference's own runs. Nothing of the reference is copied: its
modules are imported and executed, and only inputs, outputs and settings are stored (make_golden_train.save_npz: a
rerun gives the same bytes).

  g13_decoders_widths_<case>.npz   one file per case, as g5 (together they pass 1 MiB): forward output and autograd
                            gradients (input rows, every parameter) of the reference's IMNet / IEF at gf_dim 32 and
                            128, on ROWS = 113 rows (seven 16-row sub-tiles of the chain launch plus one row;
                            three 32-row tiles and a partial one of the layered route), with g5's inputs and
                            upstream gradient. Parameter gradients of more than 4096 elements are stored at
                            every PARAM_STRIDE-th element (make_golden_train.strided).
  g14_widths_eval.npz       the evaluation trace (g3's keys for stage 1, g4's keys for two refine iterations) of the
                            reference's LIDF / RefineNet on g3's two-frame 16 x 24 batch at the two configurations of
                            CONFIGS below; closed-form PointNets in both stages. (Without g3's per-pair gathers
                            intersect_rgb_feat / intersect_voxel_feat: copies of per-ray / per-voxel rows that
                            alone pass 1 MiB.)
  g15_train_widths.npz (+ _params)         make_golden_train.generate at configuration A, cases e0 and e6_hn: g9's keys
                                           and asserted conditions.
  g16_refine_train_widths.npz (+ _params)  make_golden_refine_train.generate at A (plain, hn; stage 1 as g15 left it) and
                                           at B (plain; its own stage-1 search): g10's keys under the prefixes A_ / B_, and
                                           g10's asserted conditions.

g13's weights are closed_form_params(kind, d, seed, gf) with the linear_* weights multiplied by a per-case factor. At the
filler's own amplitude every row of every decoder case lands on ONE branch of the output clamp (argument < 0, where the
output is 0.01 x the logit), so an output pin would hold the logit a hundred times looser than it reads. The generator
searches (factor, seed) per case and asserts:
  no hidden pre-activation, in any pass, within 2e-5 of 0 (g5's rule; evaluated in float64);
  in every hidden layer of every pass at least 25 % of the entries of each sign;
  without a sigmoid: each of the clamp's three branches (argument < 0, in [0, 1], > 1) holds at least 10 % of the rows,
  and no argument lies within 2e-5 of 0 or 1;  with the sigmoid: at least 10 % of the rows below 0.4 and above 0.6.

g14 asserts g3's rule (every ray's two largest logits more than 1e-4 apart) and g10's (no position that enters a refine
iteration has a coordinate within 2e-4 of a voxel face), and searches the decoders' seeds until both hold.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_refine_train as refine_train  # noqa: E402
import make_golden_train as train  # noqa: E402
from make_golden import REF, closed_form, closed_form_params, g3_batch, install_stubs, orc  # noqa: E402
from make_golden_refine_train import load_refine  # noqa: E402
from make_golden_train import PARAM_STRIDE, FixedFeatures, apply_overrides, load_stage1, save_npz, strided  # noqa: E402

ROWS = 113
# kind, inp_dim, gf_dim, n_iter, use_sigmoid
G13_CASES = (("IMNET", 385, 32, 1, False), ("IMNET", 385, 128, 1, False), ("IEF", 385, 32, 3, False),
             ("IEF", 334, 128, 2, False), ("IEF", 337, 32, 2, True))
FACTORS = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 16.0)


def g13_key(kind, d, gf, n_iter, sig):
    return "%s_%d_%d_%d_%d" % (kind, d, gf, n_iter, int(sig))


def g13_params(kind, d, gf, seed, factor):
    """closed_form_params with the linear_* weights (not the biases, not offset_enc) times `factor` (in float32)."""
    return closed_form_params(kind, d, seed=seed, gf=gf, factor=float(factor))


def g13_inputs(d):
    """g5's recipe at ROWS rows: the input rows and the upstream gradient of sum(y * wgt)."""
    return closed_form((ROWS, d), 0.5698402910, 0.1 * d, 1.0), closed_form((ROWS, 1), 0.7390851332, 0.37, 1.0)


def g13_violations(p, x, kind, n_iter, sig):
    """The asserted conditions on a float64 evaluation of the oracle's restatement (it takes the pre-activations in
    evaluation order: three hidden layers per pass, then the output activation's argument)."""
    zs = []
    with torch.no_grad():
        y = orc.decoder_forward({k: v.double() for k, v in p.items()}, x.double(), kind, n_iter, sig, preacts=zs)
    bad = []
    for i, z in enumerate(zs[:-1]):
        if z.abs().min().item() <= 2e-5:
            bad.append("pre-activation %d: %.3g" % (i, z.abs().min().item()))
        pos = (z > 0).double().mean().item()
        if not 0.25 <= pos <= 0.75:
            bad.append("hidden layer %d: %.0f %% positive" % (i, 100 * pos))
    a = zs[-1][:, 0]
    if sig:
        if (y < 0.4).double().mean().item() < 0.1 or (y > 0.6).double().mean().item() < 0.1:
            bad.append("sigmoid output on one side")
    else:
        share = [(a < 0).double().mean().item(), ((a >= 0) & (a <= 1)).double().mean().item(),
                 (a > 1).double().mean().item()]
        if min(share) < 0.1:
            bad.append("clamp branches %s" % ["%.0f %%" % (100 * s) for s in share])
        if min(a.abs().min().item(), (a - 1).abs().min().item()) <= 2e-5:
            bad.append("clamp argument at a kink")
    return bad


def g13_decoders(verbose=True):
    import models.implicit_net as ref
    files = {}
    for c, (kind, d, gf, n_iter, sig) in enumerate(G13_CASES):
        x, wgt = g13_inputs(d)
        found = None
        for factor in FACTORS:
            for seed in range(131 + 100 * c, 131 + 100 * c + 60):
                p = g13_params(kind, d, gf, seed, factor)
                if not g13_violations(p, x, kind, n_iter, sig):
                    found = (factor, seed, p)
                    break
            if found:
                break
        if not found:
            raise SystemExit("g13: no (factor, seed) satisfies the conditions for %s" % (G13_CASES[c],))
        factor, seed, p = found
        if kind == "IEF":
            m = ref.IEF(torch.device("cpu"), d, 1, gf, n_iter=n_iter, use_sigmoid=sig)
        else:
            m = ref.IMNet(d, 1, gf, use_sigmoid=sig)
        m.load_state_dict(p)
        assert not g13_violations(p, x, kind, n_iter, sig)
        xr = x.clone().requires_grad_(True)
        y = m(xr)
        (y * wgt).sum().backward()
        key = g13_key(kind, d, gf, n_iter, sig)
        out = files[key] = {key + "_param_stride": np.int64(PARAM_STRIDE), key + "_rows": np.int64(ROWS)}
        out[key + "_seed"] = np.int64(seed)
        out[key + "_factor"] = np.float32(factor)
        out[key + "_y"] = y.detach().numpy()
        out[key + "_g_input"] = xr.grad.numpy()
        for k, v in m.named_parameters():
            out[key + "_g_" + k] = strided(v.grad).numpy().copy()
        if verbose:
            yy = y.detach()
            print("g13 %-22s factor %-4g seed %d  y in [%.3f, %.3f]  rows <0 / [0,1] / >1: %d / %d / %d" % (
                key, factor, seed, yy.min(), yy.max(), int((yy < 0).sum()), int(((yy >= 0) & (yy <= 1)).sum()),
                int((yy > 1).sum())))
    return files


# ----------------------------------------------------------------------------------------------------- g14 .. g16
# All other options as in the shipped yaml files.
CONFIGS = {
    # A, other features: every width of both stages, 'rel' decoder positions in both stages, an 'abs' refine PointNet
    "A": {"model.imnet_gf": 32, "model.rgb_out": 16, "model.roi_out_bbox": 3, "model.pnet_out": 64, "model.pnet_gf": 16,
          "model.offdec_type": "IEF", "model.n_iter": 2, "model.intersect_pos_type": "rel",
          "refine.pnet_out": 64, "refine.pnet_gf": 16, "refine.imnet_gf": 32, "refine.offdec_type": "IEF",
          "refine.n_iter": 3, "refine.intersect_pos_type": "rel", "refine.pnet_pos_type": "abs"},
    # B, other decoders only: what pipeline.FrameRunner routes to lidf_frame_widths_f32
    "B": {"model.imnet_gf": 128, "model.offdec_type": "IEF", "model.n_iter": 2,
          "refine.imnet_gf": 32, "refine.offdec_type": "IEF", "refine.n_iter": 2},
}
G14_FACTORS = (4.0, 8.0, 2.0, 16.0)   # closed_form_params' factors tried for the decoders (4: outputs of order 1)
G14_PNET_SEEDS = (41, 43)   # stage 1, stage 2


def _params(yaml, overrides):
    from opt import Params
    cfg = os.path.join(REF, "experiments", "implicit_depth")
    opt = Params(os.path.join(cfg, "default_config.yaml"))
    opt.update(os.path.join(cfg, yaml))
    opt.grid.valid_sample_num = -1   # all valid points: no random sub-sampling in the trace
    apply_overrides(opt, overrides)
    return opt


def _face_distance(dd, pos):
    """Smallest distance of a coordinate of pos [R, 3] to the voxel faces (a lattice of spacing part_size from xmin)."""
    part = dd["part_size"]
    off = (pos.double() - dd["xmin"].double()) / part
    return ((off - off.round()).abs() * part).min().item()


def _logit_gap(dd):
    lg, ray = dd["pred_prob_end"].detach()[:, 0].double(), dd["miss_ray_intersect_idx"]
    gap = 1e9
    for r in range(dd["total_miss_sample_num"]):
        v = torch.sort(lg[ray == r], descending=True)[0]
        if v.numel() > 1:
            gap = min(gap, (v[0] - v[1]).item())
    return gap


def _memo_roi_align():
    """The stub's numpy-loop RoIAlign, remembered per (boxes, output size): the seed searches call it with the same
    arguments every time."""
    ops = sys.modules["torchvision.ops"]
    real, memo = ops.roi_align, {}

    def roi_align(inp, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
        key = (inp.data_ptr(), tuple(inp.shape), boxes.numpy().tobytes(), output_size)
        if key not in memo:
            memo[key] = real(inp, boxes, output_size, spatial_scale, sampling_ratio, aligned)
        return memo[key].clone()
    ops.roi_align = roi_align


def g14_config(name, batch, verbose=True):
    """One configuration's evaluation trace: LIDF's steps as g3 takes them, then two get_pred_refine calls as g4."""
    import models.pipeline as pl
    ov = CONFIGS[name]
    dev = torch.device("cpu")
    opt = _params("test_lidf.yaml", ov)
    torch.manual_seed(1234)
    lidf = pl.LIDF(opt, dev).eval()
    with torch.no_grad():
        feat = lidf.resnet_model(batch["rgb"]).detach().clone()
    lidf.resnet_model = FixedFeatures(feat)
    load_stage1(lidf, (21, 22, G14_PNET_SEEDS[0]))
    cap = {}
    hk = lidf.pnet_model.register_forward_hook(lambda m, i, o: cap.__setitem__("occ_voxel_feat", o.detach().clone()))
    with torch.no_grad():
        dd = lidf.prepare_data(batch, "test", None)
        lidf.get_valid_points(dd)
        assert lidf.get_occ_vox_bound(dd)
        lidf.get_miss_ray(dd, "test")
        assert lidf.compute_ray_aabb(dd)
        lidf.get_embedding(dd)
        hk.remove()
        # stage-1 decoder weights: g3's rule on the logits (the prob decoder's search), g10's on the positions that
        # enter the first refine iteration (the offset decoder's search; an offset clamped to 0 leaves the point on
        # the face through which its ray enters the voxel)
        m, D = opt.model, lidf.prob_dec.inp_dim
        found = {}
        for kind, net, ok in (("IMNET", lidf.prob_dec, lambda: _logit_gap(dd) > 1e-4),
                              (m.offdec_type, lidf.offset_dec, lambda: _face_distance(dd, dd["pred_pos"]) > 2e-4)):
            for factor, seed in ((f, sd) for f in G14_FACTORS for sd in range(21, 421)):
                net.load_state_dict(closed_form_params(kind, D, seed=seed, gf=m.imnet_gf, factor=factor))
                lidf.get_pred(dd, "test", 0)
                if ok():
                    found[net] = (factor, seed)
                    break
            else:
                raise SystemExit("g14 %s: no stage-1 %s weights" % (name, kind))
        (fp, sp), (fo, so) = found[lidf.prob_dec], found[lidf.offset_dec]
        ropt = _params("test_refine.yaml", ov)
        refine = pl.RefineNet(ropt, dev).eval()
        feats, ends, real_scatter = [], [], pl.scatter

        def scatter(src, index, dim=0, out=None, dim_size=None, reduce="sum"):   # (:944: end_voxel_id, in place)
            r = real_scatter(src, index, dim=dim, out=out, dim_size=dim_size, reduce=reduce)
            if out is not None:
                ends.append(out.clone())
            return r
        pl.scatter = scatter
        hk = refine.pnet_model.register_forward_hook(lambda m, i, o: feats.append(o.detach().clone()))
        for fr, rseed in ((f, sd) for f in G14_FACTORS for sd in range(31, 431)):
            load_refine(refine, (rseed, G14_PNET_SEEDS[1]), fr)
            del feats[:], ends[:]
            p1 = refine.get_pred_refine(dd, dd["pred_pos"], "test", 0)
            if _face_distance(dd, p1) <= 2e-4:
                continue
            p2 = refine.get_pred_refine(dd, p1, "test", 1)
            break
        else:
            raise SystemExit("g14 %s: no stage-2 seed" % name)
        hk.remove()
        pl.scatter = real_scatter
        assert len(feats) == 2 and len(ends) == 2
        inp = torch.cat((dd["intersect_voxel_feat"], dd["intersect_rgb_feat"], dd["intersect_enter_pos_embed"],
                         dd["intersect_leave_pos_embed"], dd["intersect_dir_embed"]), -1)
        pred_offset = lidf.offset_dec(inp)
    assert inp.shape[1] == lidf.prob_dec.inp_dim
    keep = ["miss_bid", "miss_flat_img_id", "miss_ray_dir", "miss_img_ind", "voxel_bound", "occ_vox_bid",
            "occ_vox_intersect_idx", "miss_ray_intersect_idx", "intersect_enter_dist", "intersect_leave_dist",
            "intersect_enter_pos", "full_rgb_feat", "pair_pred_pos", "max_pair_id", "pred_prob_end",
            "pred_prob_end_softmax", "pred_pos", "valid_xyz", "valid_bid", "revidx", "valid_v_pid", "valid_v_rel_coord",
            "occ_vox_global_coord", "xmin"]
    out = {k: dd[k].detach().numpy() for k in keep}
    out["occ_voxel_feat"] = cap["occ_voxel_feat"].numpy()
    out["pred_offset"] = pred_offset.numpy()
    out["part_size"] = np.float32(dd["part_size"])
    out["offset_range"] = np.array(opt.grid.offset_range, dtype=np.float32)
    out["D"] = np.array([lidf.prob_dec.inp_dim, refine.offset_dec.inp_dim])
    # prob_dec, offset_dec, pnet_model, refine offset_dec, refine pnet_model; closed_form_params' factor of the decoders
    out["seeds"] = np.array((sp, so, G14_PNET_SEEDS[0], rseed, G14_PNET_SEEDS[1]))
    out["factors"] = np.array((fp, fo, 1.0, fr, 1.0), dtype=np.float32)
    valid_v_rgb = dd["valid_rgb"][dd["valid_v_pid"]]
    pos = dd["valid_v_rel_coord"] if ropt.refine.pnet_pos_type == "rel" else dd["valid_xyz"][dd["valid_v_pid"]]
    out["refine_valid_inp"] = torch.cat((pos, valid_v_rgb), -1).numpy()
    out["refine_offset_range"] = np.array(ropt.refine.offset_range, dtype=np.float32)
    out["pred_pos_refine_1"], out["pred_pos_refine_2"] = p1.numpy(), p2.numpy()
    out["occ_voxel_feat_refine_1"], out["occ_voxel_feat_refine_2"] = feats[0].numpy(), feats[1].numpy()
    out["end_voxel_1"], out["end_voxel_2"] = ends[0].numpy(), ends[1].numpy()
    out["min_logit_gap"] = np.float64(_logit_gap(dd))
    out["min_face_distance"] = np.float64(min(_face_distance(dd, dd["pred_pos"]), _face_distance(dd, p1)))
    if verbose:
        print("g14 %s: D %s R=%d V=%d P=%d seeds %s factors %s; logit gap %.3g, face distance %.3g" % (
            name, out["D"].tolist(), out["miss_ray_dir"].shape[0], out["voxel_bound"].shape[0],
            out["pair_pred_pos"].shape[0], out["seeds"].tolist(), out["factors"].tolist(), out["min_logit_gap"],
            out["min_face_distance"]))
    return out


def g14_widths_eval(verbose=True):
    install_stubs()
    _memo_roi_align()
    batch, (B, h, w) = g3_batch()
    out = {"hw": np.array([h, w]),
           "intr": torch.stack([batch[k].float() for k in ("fx", "fy", "cx", "cy")], 1).numpy()}
    for k in ("rgb", "xyz", "xyz_corrupt", "depth_corrupt", "corrupt_mask", "valid_mask"):
        out["batch_" + k] = batch[k].numpy()
    for name in sorted(CONFIGS):
        for k, v in g14_config(name, batch, verbose).items():
            out["%s_%s" % (name, k)] = v
    return out


# ------------------------------------------------------------------------------------------------------- g15 / g16
G15_CASES = tuple(c for c in train.CASES if c[0] in ("e0", "e6_hn"))
G16_CASES = {"A": tuple(c for c in refine_train.CASES if c[0] in ("plain", "hn")),
             "B": tuple(c for c in refine_train.CASES if c[0] == "plain")}


def g15_train_widths(verbose=True):
    """make_golden_train.generate at configuration A: the same keys and asserted conditions as g9."""
    return train.generate(verbose, CONFIGS["A"], G15_CASES, tag="g15")


def g16_refine_train_widths(g15_main, verbose=True):
    """make_golden_refine_train.generate at A (stage 1 as g15 left it) and at B (a stage-1 search of its own): the same
    keys and asserted conditions as g10, every key of a configuration under its prefix."""
    main, params = {}, {}
    for name in sorted(CONFIGS):
        ov = CONFIGS[name]
        if name == "A":
            sources = refine_train.g9_sources(g15_main, ov)
        else:
            train.setup()
            sources = ((shift, face, feat, seeds + (train.PNET_SEED,))
                       for shift, face, _, feat, seeds in train.candidates(ov, verbose, "g16 B stage 1"))
        m, p = refine_train.generate(verbose, ov, G16_CASES[name], sources, tag="g16 " + name)
        main.update(("%s_%s" % (name, k), v) for k, v in m.items())
        params.update(("%s_%s" % (name, k), v) for k, v in p.items())
    return main, params


def write_checked(name, arrays):
    path = os.path.join(HERE, name)
    save_npz(path, arrays)
    size = os.path.getsize(path)
    print("%-44s %8d bytes" % (name, size))
    assert size < (1 << 20), name


if __name__ == "__main__":
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    only = [a[7:] for a in sys.argv[1:] if a.startswith("--only-")]
    if not only or "g13" in only:
        for key, case in g13_decoders().items():
            write_checked("g13_decoders_widths_%s.npz" % key, case)
    if not only or "g14" in only:
        write_checked("g14_widths_eval.npz", g14_widths_eval())
    if not only or "g15" in only:
        main, params = g15_train_widths()
        write_checked("g15_train_widths.npz", main)
        write_checked("g15_train_widths_params.npz", params)
    if not only or "g16" in only:
        main, params = g16_refine_train_widths(np.load(os.path.join(HERE, "g15_train_widths.npz")))
        write_checked("g16_refine_train_widths.npz", main)
        write_checked("g16_refine_train_widths_params.npz", params)
