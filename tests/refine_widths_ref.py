"""Float64 / float32 references for the stage-2 refine chain at widths other than the shipped configuration (tests
only; CPU, plain torch ops through the oracle).

pointnet_ref.refine_case() — 2 frames, 20 x 24, 960 rays, 1,500 valid points, 1,458 voxels — at a configuration
    (rgb_out, roi_out_bbox, pnet_out, pnet_gf, gf_dim, decoder kind, n_iter, multires, multires_views)
with a feature map, PointNet parameters and a decoder of that configuration; the chain is pointnet_ref.refine_chain's
with the ROI feature at any output size (roi_ref.roi_align_torch) and the decoder's kind, passes and embedding widths
handed to orc.refine_step. The scene is conditioned by pointnet_ref.condition_refine's rules over that chain.
"""
import contextlib
import functools

import torch
import torch.nn.functional as F

import pointnet_ref as ref
import roi_ref
from pointnet_ref import FACE_EPS, REL, _near_face, pointnet_flags, subset_case
from util import kink_rows_of, orc

# the first five have no other route; the last three are served by query._lidf_refine_train_composed as well
CONFIGS = [(16, 3, 64, 16, 32, "IEF", 2, 8, 4), (16, 3, 64, 16, 32, "IEF", 3, 8, 4), (5, 1, 96, 32, 64, "IMNET", 1, 4, 2),
           (32, 2, 128, 32, 128, "IMNET", 1, 8, 4), (32, 2, 256, 64, 96, "IEF", 2, 8, 4),
           (32, 2, 128, 32, 32, "IEF", 2, 8, 4), (32, 2, 128, 16, 64, "IEF", 2, 8, 4), (32, 2, 128, 32, 64, "IEF", 2, 0, 0)]
NEW_ONLY, BOTH_ROUTES = CONFIGS[:5], CONFIGS[5:]
SHIPPED = (32, 2, 128, 32, 64, "IEF", 2, 8, 4)
SETTINGS = [(False, True), (True, False)]        # (pos_rel, pnet_pos_rel)
RAY_CAP, VALID_CAP = 0.15, 0.05                  # the share conditioning may drop: conditions, not measurements


def cfg_id(cfg):
    return "-".join(str(v) for v in cfg)


def inp_dim(cfg):
    rgb_out, roi_out, pnet_out, _, _, _, _, Lm, Lv = cfg
    return pnet_out + rgb_out * roi_out * roi_out + orc.embed_dim(Lm) + orc.embed_dim(Lv)


@functools.lru_cache(maxsize=None)
def widths_case(cfg):
    """refine_case() with the feature map, PointNet and decoder of cfg (host tensors; nobody writes to it)."""
    from test_train_widths_gpu import _pointnet_params
    rgb_out, roi_out, pnet_out, pnet_gf, gf, kind, n_iter, Lm, Lv = cfg
    case = dict(ref.refine_case())
    coarse = torch.randn(2, rgb_out, 5, 6, generator=torch.Generator().manual_seed(rgb_out + pnet_out))
    case["feat_grid"] = F.interpolate(coarse, size=(20, 24), mode="bilinear", align_corners=False).contiguous()
    case["pnet_p"] = _pointnet_params(6, pnet_out, pnet_gf, 5)
    case["off_p"] = orc.randomize_biases(orc.init_decoder(kind, inp_dim(cfg), 77, 5.0, gf=gf), 78)
    case["cfg"] = cfg
    return case


@contextlib.contextmanager
def _sigmoid_decoder(on):
    """orc.refine_step has no use_sigmoid argument: for the duration of the block its decoder_forward applies the
    sigmoid output (the oracle's own use_sigmoid branch)."""
    if not on:
        yield
        return
    real = orc.decoder_forward

    def decoder_forward(p, x, kind, n_iter=2, use_sigmoid=False, preacts=None):
        return real(p, x, kind, n_iter, True, preacts=preacts)
    orc.decoder_forward = decoder_forward
    try:
        yield
    finally:
        orc.decoder_forward = real


def chain(case, dt, forward_times, pos_rel=False, pnet_pos_rel=True, leaves=None, trace=None, use_sigmoid=False):
    """pointnet_ref.refine_chain at case["cfg"]: (pos, [end voxels of every iteration])."""
    _, roi_out, _, _, _, kind, n_iter, Lm, Lv = case["cfg"]
    c = lambda t: t.detach().to(dt, copy=True)  # noqa: E731
    pn = {k: c(v) for k, v in case["pnet_p"].items()}
    of = {k: c(v) for k, v in case["off_p"].items()}
    pp, fg = c(case["pred_pos"]), c(case["feat_grid"])
    if leaves is not None:
        for t in list(pn.values()) + list(of.values()) + [pp, fg]:
            t.requires_grad_(True)
        leaves.update({"pnet." + k: v for k, v in pn.items()})
        leaves.update({"dec." + k: v for k, v in of.items()})
        leaves["pred_pos"], leaves["feat_grid"] = pp, fg
    ray_dir = case["ray_dir"].to(dt)
    R = ray_dir.shape[0]
    boxes = orc.roi_boxes(case["ray_pix"].long(), case["ray_bid"].long(), fg.shape[2], fg.shape[3], 8)
    ray_rgb = roi_ref.roi_align_torch(fg, boxes, roi_out).reshape(R, -1)
    pos = pp + case["noise"] * ray_dir
    evs = []
    with _sigmoid_decoder(use_sigmoid):
        for _ in range(forward_times):
            pos, ev, _ = orc.refine_step(pos, ray_dir, case["ray_pix"], case["ray_bid"], case["ray_flat"],
                                         case["max_pair_id"], case["pair_vox"], case["voxel_bound"].to(dt),
                                         case["voxel_bid"], case["rgb_img"].to(dt), fg, case["valid_inp"].to(dt),
                                         case["valid_vox"], pn, of, off_kind=kind, n_iter=n_iter, multires=Lm,
                                         multires_views=Lv, pos_rel=pos_rel, pnet_pos_rel=pnet_pos_rel,
                                         ray_rgb=ray_rgb, trace=trace)
            evs.append(ev)
    return pos, evs


def condition(case, forward_times, pos_rel, pnet_pos_rel, use_sigmoid=False, rel=REL, max_passes=50):
    """pointnet_ref.condition_refine's rules over chain(): (keep_ray [R] bool, keep_valid [Nv] bool, passes)."""
    R, Nv = case["ray_dir"].shape[0], case["valid_inp"].shape[0]
    V = case["voxel_bound"].shape[0]
    keep_ray, keep_valid = torch.ones(R, dtype=torch.bool), torch.ones(Nv, dtype=torch.bool)
    passes = 0
    while True:
        rid, vid = torch.nonzero(keep_ray)[:, 0], torch.nonzero(keep_valid)[:, 0]
        sub = subset_case(case, keep_ray, keep_valid)
        tr = []
        with torch.no_grad():
            chain(sub, torch.float64, forward_times, pos_rel, pnet_pos_rel, trace=tr, use_sigmoid=use_sigmoid)
        bad_ray = torch.zeros(rid.numel(), dtype=torch.bool)
        bad_valid = torch.zeros(vid.numel(), dtype=torch.bool)
        for it in tr:
            bad, out_mask = pointnet_flags(it["pnet"], V, rel)
            bad_valid |= bad[:vid.numel()]
            bad_ray |= bad[vid.numel():]
            bad_ray |= out_mask.any(1)[it["end_voxel"]]
            bad_ray |= kink_rows_of(it["preacts"][:-1], it["preacts"][-1], use_sigmoid, rel=rel)
            bad_ray |= _near_face(it["pos"], sub["ray_bid"], case["voxel_bound"], case["voxel_bid"], FACE_EPS)
        if not bool(bad_ray.any() or bad_valid.any()):
            return keep_ray, keep_valid, passes
        keep_ray[rid[bad_ray]] = False
        keep_valid[vid[bad_valid]] = False
        passes += 1
        assert passes <= max_passes, "conditioning does not settle"


@functools.lru_cache(maxsize=None)
def conditioned(cfg, pos_rel=False, pnet_pos_rel=True, use_sigmoid=False):
    """widths_case(cfg) conditioned for two iterations (which covers one): (case, keep_ray, keep_valid, passes); the
    caps hold or this raises. Computed once per setting and shared; nobody writes to it."""
    case = widths_case(cfg)
    keep_ray, keep_valid, passes = condition(case, 2, pos_rel, pnet_pos_rel, use_sigmoid)
    dropped = (1.0 - keep_ray.float().mean().item(), 1.0 - keep_valid.float().mean().item())
    print("refine scene %s%s: %.1f %% of the rays, %.1f %% of the valid points dropped in %d passes"
          % (cfg_id(cfg), " pos_rel" if pos_rel else "", 100 * dropped[0], 100 * dropped[1], passes))
    assert dropped[0] <= RAY_CAP and dropped[1] <= VALID_CAP, (cfg, dropped)
    return subset_case(case, keep_ray, keep_valid), keep_ray, keep_valid, passes


def upstream(case):
    """test_f64_stage2_gpu.py::_upstream's randn."""
    return torch.randn(case["pred_pos"].shape, generator=torch.Generator().manual_seed(3))


@functools.lru_cache(maxsize=None)
def refs(cfg, forward_times, pos_rel=False, pnet_pos_rel=True, use_sigmoid=False):
    """Float64 and float32 autograd through chain() on the conditioned scene, once per configuration:
    [(pos, end voxels of the last iteration, {leaf: gradient of sum(pos * upstream)})] for float64, float32."""
    case = conditioned(cfg, pos_rel, pnet_pos_rel, use_sigmoid)[0]
    out = []
    for dt in (torch.float64, torch.float32):
        leaves = {}
        pos, evs = chain(case, dt, forward_times, pos_rel, pnet_pos_rel, leaves=leaves, use_sigmoid=use_sigmoid)
        (pos * upstream(case).to(dt)).sum().backward()
        out.append((pos.detach(), evs[-1], {k: v.grad for k, v in leaves.items()}))
    return out
