"""pipeline.py — the whole evaluation path of the reference's LIDF / RefineNet, chained on the device.

Reference counterparts (paths relative to /root/reference/src, eval flavour `exp_type='test'`):
  prepare_data        <- LIDF.prepare_data          models/pipeline.py:91-133
  get_valid_points    <- LIDF.get_valid_points      models/pipeline.py:135-160
  lidf_forward        <- LIDF.forward               models/pipeline.py:652-717
                         (get_occ_vox_bound :162-201, get_miss_ray :203-269, compute_ray_aabb
                          :271-296, get_embedding :338-425, get_pred :427-466, depth map :593-596)
  refine_forward      <- RefineNet.forward          models/pipeline.py:1032-1041
  lidf_forward_train  <- LIDF.forward, exp_type 'train'   models/pipeline.py:652-711
  refine_forward_train <- RefineNet.forward, exp_type 'train'   models/pipeline.py:1032-1041
  train_refine_step   <- the two forward calls of a stage-2 training iteration   trainers/train_refine.py:374-393
  eval_metrics        <- the bs == 1 statistics of LIDF.compute_loss   models/pipeline.py:577-627

Every compute step is a call into liblidf_hip.so through implicit_depth_amd.query / .pointnet;
what is written here in torch is plumbing only (views, index_select of inputs, dict handling).
The ResNet that produces `full_rgb_feat` is upstream of the path (out of scope): the
caller passes its output. Keys of the returned data_dict are the reference's.
"""
import torch

from . import _lib
from . import query as Q


class LidfOptions:
    """The options of the shipped configs that the path reads (experiments/implicit_depth/
    default_config.yaml + test_lidf.yaml / test_refine.yaml)."""

    def __init__(self, **kw):
        self.mask_type = "all"                 # 'all' | 'pred'
        self.multires, self.multires_views = 8, 4
        self.roi_inp_bbox = 8
        self.roi_out_bbox = 2                  # model.roi_out_bbox (2 in every shipped config)
        self.intersect_pos_type = "abs"
        self.offset_range = (0.0, 1.0)
        self.grid_res = 8
        self.xmin, self.xmax = (-1.0, -1.0, 0.0), (1.0, 1.0, 2.0)   # utils/constants.py:15-16
        self.valid_stride = None               # None = every valid point (valid_sample_num == -1)
        # grid.valid_sample_num (10000 in every shipped config): None or -1 = every valid point; n > 0 = the random
        # block sample of n valid points per image (query.sample_valid_points) wherever no valid_idx is passed
        self.valid_sample_num = None
        self.sampler_state = None              # query.sampler_state(seed, device); None = the device's default state
        # training (train_lidf.yaml): rays per image of the random window, label-selected pairs before this epoch
        self.miss_sample_num = 20000
        # who draws that window: 'numpy' = get_miss_ray + sample_miss_rays (np.random.choice per image, the reference's
        # own call); 'device' = query.sample_miss_window (one library call, starts drawn from sampler_state). miss_starts:
        # device int32 [bs], the window starts of the 'device' route instead of a draw (None = draw)
        self.miss_sample = "numpy"
        self.miss_starts = None
        # RoIAlign's adjoint to full_rgb_feat in the training calls: 'atomic' (default; its border boxes are summed with
        # float atomics, equal to rounding between runs) or 'ordered' (a fixed-order gather, bit-reproducible;
        # query.lidf_query_train). torch.use_deterministic_algorithms is not consulted
        self.roi_backward = "atomic"
        self.maxpool_label_epo = 6
        # stage 2 (test_refine.yaml)
        self.refine_forward_times = 2
        self.refine_offset_range = (-0.2, 0.2)
        self.refine_use_all_pix = True
        self.refine_pnet_pos_type = "rel"
        self.refine_intersect_pos_type = "abs"
        # stage-2 training (train_refine.yaml:66-67): the perturbation of the first iteration's input
        self.refine_perturb = True
        self.refine_perturb_prob = 0.8
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown option %s" % k)
            setattr(self, k, v)
        self.sample_num()
        self.miss_route()
        self.roi_route()

    def miss_route(self):
        """miss_sample, checked: 'numpy' or 'device'."""
        if self.miss_sample not in ("numpy", "device"):
            raise ValueError("miss_sample must be 'numpy' or 'device', not %r" % (self.miss_sample,))
        return self.miss_sample

    def roi_route(self):
        """roi_backward, checked: 'atomic' or 'ordered'."""
        if self.roi_backward not in ("atomic", "ordered"):
            raise ValueError("roi_backward must be 'atomic' or 'ordered', not %r" % (self.roi_backward,))
        return self.roi_backward

    def sample_num(self):
        """valid_sample_num as the sampler takes it: n > 0, or 0 for every valid point (None / -1)."""
        n = self.valid_sample_num
        if n is None or n == -1:
            return 0
        if int(n) != n or n < 1:
            raise ValueError("valid_sample_num must be None, -1 (every valid point) or a positive count, not %r" % (n,))
        if self.valid_stride and self.valid_stride > 1:
            raise ValueError("valid_sample_num and valid_stride are two different selections of the valid points: "
                             "set one of them")
        return int(n)


def prepare_data(batch, opt, pred_mask=None, exp_type="test"):
    """LIDF.prepare_data (models/pipeline.py:91-133). exp_type 'train': the batch's own valid_mask (or
    1 - corrupt_mask), no pred_mask override (:126)."""
    rgb_img = batch["rgb"]
    bs, _, h, w = rgb_img.shape
    corrupt_mask = batch["corrupt_mask"].squeeze(1)
    valid_mask = batch["valid_mask"].squeeze(1) if "valid_mask" in batch else 1 - corrupt_mask
    dd = {
        "bs": bs, "h": h, "w": w, "rgb_img": rgb_img, "corrupt_mask": corrupt_mask,
        "valid_mask": valid_mask,
        "xyz_flat": batch["xyz"].permute(0, 2, 3, 1).contiguous().reshape(bs, -1, 3),
        "xyz_corrupt_flat": batch["xyz_corrupt"].permute(0, 2, 3, 1).contiguous().reshape(bs, -1, 3),
        "fx": batch["fx"].float(), "fy": batch["fy"].float(),
        "cx": batch["cx"].float(), "cy": batch["cy"].float(),
        "item_path": batch.get("item_path"),
    }
    if exp_type == "train":
        return dd
    if opt.mask_type == "pred":
        dd["pred_mask"] = pred_mask
        dd["valid_mask"] = 1 - pred_mask
    elif opt.mask_type == "all":
        dd["pred_mask"] = torch.ones_like(corrupt_mask)
        dd["valid_mask"] = 1 - (batch["depth_corrupt"] == 0).squeeze(1).float()
    else:
        raise NotImplementedError("mask_type %s" % opt.mask_type)
    return dd


def get_valid_points(dd, opt, valid_idx=None):
    """LIDF.get_valid_points (models/pipeline.py:135-160). valid_idx [Nv,2] (image, flat pixel)
    may be supplied and wins; otherwise opt.valid_sample_num > 0 draws the reference's random block sample
    (utils/point_utils.py:79-125) on the device, query.sample_valid_points — an image without a valid pixel
    raises RuntimeError, the reference's assertion; otherwise every valid pixel, optionally every
    opt.valid_stride-th."""
    bs = dd["bs"]
    if valid_idx is None and opt.sample_num():
        valid_idx = Q.sample_valid_points(dd["valid_mask"], opt.sample_num(), state=opt.sampler_state)
    if valid_idx is None:
        nz = Q.nonzero_pixels(dd["valid_mask"])
        valid_bid, valid_flat = nz["bid"], nz["flat"]
        if opt.valid_stride and opt.valid_stride > 1:
            valid_bid, valid_flat = valid_bid[::opt.valid_stride], valid_flat[::opt.valid_stride]
    else:
        valid_bid, valid_flat = valid_idx[:, 0].long(), valid_idx[:, 1].long()
    lin = valid_bid * (dd["h"] * dd["w"]) + valid_flat
    rgb_flat = dd["rgb_img"].permute(0, 2, 3, 1).contiguous().reshape(-1, 3)
    dd.update({
        "valid_bid": valid_bid, "valid_flat_img_id": valid_flat,
        "valid_xyz": dd["xyz_corrupt_flat"].reshape(-1, 3).index_select(0, lin),
        "valid_rgb": rgb_flat.index_select(0, lin),
    })
    return dd


def _mark(marks, name):
    """Benchmarks only: record a CUDA event named `name` on the current stream."""
    if marks is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((name, ev))


def lidf_forward(batch, full_rgb_feat, pnet_model, prob_dec, offset_dec, opt=None, pred_mask=None,
                 valid_idx=None, precision="f32", workspace=None, marks=None, offsets="all"):
    """LIDF.forward for evaluation (models/pipeline.py:652-717): returns (success, data_dict).
    success False = one of the reference's early exits (no occupied voxel / no miss ray / no
    intersecting pair); data_dict then holds what was computed up to that point."""
    opt = opt or LidfOptions()
    Q._refuse_autograd("pipeline.lidf_forward", "pipeline.lidf_forward_train (the stage-1 training step; its "
                       "differentiable core is query.lidf_query_train)",
                       (("full_rgb_feat", full_rgb_feat),),
                       (("pnet_model", pnet_model), ("prob_dec", prob_dec), ("offset_dec", offset_dec)))
    _mark(marks, "start")
    dd = prepare_data(batch, opt, pred_mask)
    get_valid_points(dd, opt, valid_idx)
    _mark(marks, "valid_points")
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    # occupied voxels (get_occ_vox_bound)
    occ = Q.get_occ_vox_bound(dd["valid_xyz"].contiguous(), dd["valid_bid"].to(torch.int32).contiguous(),
                              bs, opt.xmin, opt.xmax, opt.grid_res)
    dd.update(occ)
    V = occ["voxel_bound"].shape[0]
    _mark(marks, "occupied_voxels")
    if V == 0:
        return False, dd
    # miss rays
    dd.update(Q.get_miss_ray(dd["pred_mask"], dd["fx"], dd["fy"], dd["cx"], dd["cy"]))
    _mark(marks, "miss_rays")
    if dd["total_miss_sample_num"] == 0:
        return False, dd
    # ray / voxel pairs (compact, ray-major)
    vox_bid = occ["occ_vox_bid"].to(torch.int32).contiguous()
    # densely occupied grids take the cell walk (bit-identical; measured on MI355X, 76,800 rays per
    # frame: 0.34 -> 0.22 ms at 729 voxels per frame, but 0.066 -> 0.082 ms at 74, where the
    # voxel-by-voxel loop is already shorter than the walk's two extra launches)
    grid = dict(voxel_coord=occ["voxel_coord"], grid_dims=occ["grid_dims"], batch=bs) if V > 256 * bs else {}
    pair_off, pair_ray, pair_vox, pair_t = Q.compute_ray_aabb(
        dd["miss_ray_dir"], occ["voxel_bound"], dd["ray_bid"], vox_bid, **grid)
    dd.update({"pair_off": pair_off, "pair_ray": pair_ray, "pair_vox": pair_vox, "pair_t": pair_t,
               "voxel_bid": vox_bid})
    _mark(marks, "ray_aabb")
    if pair_ray.shape[0] == 0:
        return False, dd
    # voxel embedding: PointNet over the valid points of every occupied voxel
    valid_v_rgb = dd["valid_rgb"].index_select(0, occ["valid_v_pid"])
    pnet_inp = torch.cat((occ["valid_v_rel_coord"], valid_v_rgb), -1)
    dd["pnet_inp"] = pnet_inp
    dd["occ_voxel_feat"] = pnet_model(pnet_inp, occ["revidx"], n_vox=V)
    dd["full_rgb_feat"] = full_rgb_feat
    _mark(marks, "pointnet")
    # get_embedding + get_pred + depth map (pred_xyz = xyz_corrupt with the rays' pixels replaced)
    depth = dd["xyz_corrupt_flat"][:, :, 2].reshape(bs, h, w).clone()
    vox_center = None
    if opt.intersect_pos_type == "rel":
        vb = occ["voxel_bound"]
        vox_center = ((vb[:, :3] + vb[:, 3:]) / 2.0).contiguous()
    out = Q.lidf_query(dd["miss_ray_dir"], dd["ray_pix"], dd["ray_bid"], pair_off, pair_ray, pair_vox,
                       pair_t, full_rgb_feat, dd["occ_voxel_feat"], prob_dec, offset_dec,
                       multires=opt.multires, multires_views=opt.multires_views,
                       roi_inp_bbox=opt.roi_inp_bbox, roi_out_bbox=opt.roi_out_bbox, offset_range=opt.offset_range,
                       part_size=occ["part_size"], vox_center=vox_center,
                       pos_rel=opt.intersect_pos_type == "rel", ray_flat=dd["ray_flat"], depth=depth,
                       want_rayfeat=True, precision=precision, workspace=workspace, offsets=offsets)
    dd.update(out)
    dd["pred_depth"] = depth
    _mark(marks, "query")
    return True, dd


def _train_geometry(batch, full_rgb_feat, opt, valid_idx):
    """LIDF.forward(batch, 'train', epoch) up to and including compute_gt (models/pipeline.py:652-704): (success,
    data_dict). success False = one of the reference's three early exits."""
    from .losses import compute_gt
    if opt.intersect_pos_type not in ("abs", "rel"):
        raise NotImplementedError("intersect_pos_type %s" % opt.intersect_pos_type)
    _lib.require_cuda(batch["rgb"], batch["xyz"], full_rgb_feat, names=["batch['rgb']", "batch['xyz']", "full_rgb_feat"])
    dd = prepare_data(batch, opt, exp_type="train")
    get_valid_points(dd, opt, valid_idx)
    bs = dd["bs"]
    if dd["valid_xyz"].shape[0] == 0:   # (no valid point at all: no occupied voxel)
        return False, dd
    occ = Q.get_occ_vox_bound(dd["valid_xyz"].contiguous(), dd["valid_bid"].to(torch.int32).contiguous(),
                              bs, opt.xmin, opt.xmax, opt.grid_res)
    dd.update(occ)
    V = occ["voxel_bound"].shape[0]
    if V == 0:
        return False, dd
    if opt.miss_route() == "device" and opt.miss_sample_num != -1:
        dd.update(Q.sample_miss_window(dd["corrupt_mask"], dd["fx"], dd["fy"], dd["cx"], dd["cy"], opt.miss_sample_num,
                                       state=opt.sampler_state, starts=opt.miss_starts))
    else:
        miss = Q.get_miss_ray(dd["corrupt_mask"], dd["fx"], dd["fy"], dd["cx"], dd["cy"])
        dd.update(Q.sample_miss_rays(miss, bs, opt.miss_sample_num))
    if dd["total_miss_sample_num"] == 0:
        return False, dd
    vox_bid = occ["occ_vox_bid"].to(torch.int32).contiguous()
    grid = dict(voxel_coord=occ["voxel_coord"], grid_dims=occ["grid_dims"], batch=bs) if V > 256 * bs else {}
    pair_off, pair_ray, pair_vox, pair_t = Q.compute_ray_aabb(
        dd["miss_ray_dir"], occ["voxel_bound"], dd["ray_bid"], vox_bid, **grid)
    dd.update({"pair_off": pair_off, "pair_ray": pair_ray, "pair_vox": pair_vox, "pair_t": pair_t,
               "voxel_bid": vox_bid})
    if pair_ray.shape[0] == 0:
        return False, dd
    compute_gt(dd)
    valid_v_rgb = dd["valid_rgb"].index_select(0, occ["valid_v_pid"])
    dd["pnet_inp"] = torch.cat((occ["valid_v_rel_coord"], valid_v_rgb), -1)
    dd["full_rgb_feat"] = full_rgb_feat
    return True, dd


def _vox_center(dd, opt):
    if opt.intersect_pos_type != "rel":
        return None
    vb = dd["voxel_bound"]
    return ((vb[:, :3] + vb[:, 3:]) / 2.0).contiguous()


def lidf_forward_train(batch, full_rgb_feat, pnet_model, prob_dec, offset_dec, opt=None, loss_opt=None, epoch=0,
                       valid_idx=None):
    """LIDF.forward(batch, 'train', epoch) (models/pipeline.py:652-711) as one call: returns (success, data_dict,
    loss_dict). prepare_data in the train flavour (the miss rays come from corrupt_mask), get_valid_points,
    get_occ_vox_bound, get_miss_ray + the random window of opt.miss_sample_num rays per image (np.random, as the
    reference draws it; opt.miss_sample = 'device': query.sample_miss_window, drawn on the device from opt.sampler_state
    or taken from opt.miss_starts, with the windows in data_dict['miss_window']), compute_ray_aabb, compute_gt, the PointNet and the query under autograd
    (query.lidf_query_train, pairs selected by the labels while epoch < opt.maxpool_label_epo) and
    losses.lidf_loss. loss_dict['loss_net'].backward() reaches full_rgb_feat and every parameter of the three
    modules. success False = one of the reference's three early exits (no occupied voxel / no miss ray / no
    intersecting pair): loss_dict is then {} and data_dict holds what was computed up to that point. The DDP
    success-flag handshake of :662-701 stays with the trainer."""
    from .losses import lidf_loss
    opt = opt or LidfOptions()
    ok, dd = _train_geometry(batch, full_rgb_feat, opt, valid_idx)
    if not ok:
        return False, dd, {}
    dd["occ_voxel_feat"] = pnet_model(dd["pnet_inp"], dd["revidx"], n_vox=dd["voxel_bound"].shape[0])
    dd.update(Q.lidf_query_train(
        dd["miss_ray_dir"], dd["ray_pix"], dd["ray_bid"], dd["pair_off"], dd["pair_ray"], dd["pair_vox"],
        dd["pair_t"], full_rgb_feat,
        dd["occ_voxel_feat"], prob_dec, offset_dec, multires=opt.multires, multires_views=opt.multires_views,
        roi_inp_bbox=opt.roi_inp_bbox, roi_out_bbox=opt.roi_out_bbox, offset_range=opt.offset_range,
        part_size=dd["part_size"], vox_center=_vox_center(dd, opt), pos_rel=opt.intersect_pos_type == "rel",
        max_pair_id=dd["gt_max_pair_id"] if epoch < opt.maxpool_label_epo else None, roi_backward=opt.roi_route()))
    return True, dd, lidf_loss(dd, loss_opt, "train", epoch)


def refine_forward_train(dd, pnet_model_refine, offset_dec_refine, opt=None, loss_opt=None, epoch=0):
    """RefineNet.forward('train', epoch, data_dict) (models/pipeline.py:1032-1041) on the data_dict of the frozen
    stage 1 (train_refine_step's, or lidf_forward_train's): returns (data_dict, loss_dict_refine).
    opt.refine_forward_times x get_pred_refine under autograd (query.lidf_refine_train: one node, two library
    calls at the shipped widths, generic.refine_train at another rgb_out / roi_out_bbox / pnet_out), the perturbation of the first iteration drawn with the reference's own np.random calls — only when
    opt.refine_perturb is set, as the reference's `and` short-circuits — then losses.refine_loss. Adds
    pred_pos_refine [R,3], end_voxel_id [R] and refine_perturb_noise (the scalar drawn, None for none) to data_dict;
    loss_dict_refine['loss_net'].backward() reaches every parameter of the two modules. The end voxels go through
    the cell table when data_dict holds get_occ_vox_bound's grid."""
    from .losses import refine_loss
    opt = opt or LidfOptions()
    noise = Q.refine_perturb_noise(opt.refine_perturb_prob) if opt.refine_perturb else None
    valid_inp = dd["pnet_inp"]                     # cat(valid_v_rel_coord, valid_v_rgb), pipeline.py:1000
    if opt.refine_pnet_pos_type == "abs":          # :1001-1003
        valid_inp = torch.cat((dd["valid_xyz"].index_select(0, dd["valid_v_pid"]), dd["pnet_inp"][:, 3:]), -1)
    pos, end_voxel = Q.lidf_refine_train(
        dd["miss_ray_dir"], dd["ray_pix"], dd["ray_bid"], dd["ray_flat"], dd["pred_pos"], dd["max_pair_id"],
        dd["pair_vox"], dd["voxel_bound"], dd["voxel_bid"], dd["rgb_img"], dd["full_rgb_feat"],
        valid_inp.contiguous(), dd["revidx"].to(torch.int32).contiguous(), pnet_model_refine, offset_dec_refine,
        forward_times=opt.refine_forward_times, multires=opt.multires, multires_views=opt.multires_views,
        roi_inp_bbox=opt.roi_inp_bbox, roi_out_bbox=opt.roi_out_bbox, offset_range=opt.refine_offset_range,
        pos_rel=opt.refine_intersect_pos_type == "rel", pnet_pos_rel=opt.refine_pnet_pos_type == "rel",
        perturb_noise=noise, roi_backward=opt.roi_route(),
        grid=dd if all(k in dd for k in ("voxel_coord", "grid_dims", "xmin", "part_size")) else None)
    dd["pred_pos_refine"], dd["end_voxel_id"] = pos, end_voxel
    dd["refine_perturb_noise"] = noise
    return dd, refine_loss(dd, loss_opt, "train", epoch)


def train_refine_step(batch, full_rgb_feat, pnet_model, prob_dec, offset_dec, pnet_model_refine, offset_dec_refine,
                      opt=None, loss_opt=None, epoch=0, valid_idx=None):
    """The two forward calls of a stage-2 training iteration (trainers/train_refine.py:374-393): the frozen
    LIDF.forward(batch, 'train', epoch), then RefineNet.forward('train', epoch, data_dict). Returns (success,
    data_dict, loss_dict, loss_dict_refine); loss_dict is stage 1's (the trainer logs its prob_loss and acc), and
    loss_dict_refine['loss_net'].backward() is the step's backward. success False = one of stage 1's three early
    exits: the result is then (False, data_dict, {}, {}).

    Stage 1 is frozen (train_refine.py:71-73): it runs under torch.no_grad() whatever the requires_grad flags of
    full_rgb_feat, pnet_model, prob_dec and offset_dec say, and never receives a gradient. It takes the train
    flavour of the geometry (the corrupt_mask rays, the opt.miss_sample_num window, compute_gt) and then the
    inference query (query.lidf_query) and losses.lidf_loss — nothing of it is differentiated. While
    epoch < opt.maxpool_label_epo the pair of every ray is selected by the labels, as in the reference (not the
    shipped stage-2 configuration: train_refine*.yaml set maxpool_label_epo 0; pass LidfOptions(maxpool_label_epo=0)).
    loss_opt serves both losses, as the reference's one `loss` section does (train_refine.yaml: prob_w 0).
    The DDP success-flag handshake and the optimiser stay with the trainer."""
    from .losses import lidf_loss
    opt = opt or LidfOptions()
    with torch.no_grad():
        ok, dd = _train_geometry(batch, full_rgb_feat.detach(), opt, valid_idx)
        if not ok:
            return False, dd, {}, {}
        dd["occ_voxel_feat"] = pnet_model(dd["pnet_inp"], dd["revidx"], n_vox=dd["voxel_bound"].shape[0])
        dd.update(Q.lidf_query(
            dd["miss_ray_dir"], dd["ray_pix"], dd["ray_bid"], dd["pair_off"], dd["pair_ray"], dd["pair_vox"],
            dd["pair_t"], dd["full_rgb_feat"], dd["occ_voxel_feat"], prob_dec, offset_dec, multires=opt.multires,
            multires_views=opt.multires_views, roi_inp_bbox=opt.roi_inp_bbox, roi_out_bbox=opt.roi_out_bbox,
            offset_range=opt.offset_range, part_size=dd["part_size"], vox_center=_vox_center(dd, opt),
            pos_rel=opt.intersect_pos_type == "rel", want_rayfeat=False))
        if epoch < opt.maxpool_label_epo:   # the label-selected pair of every ray (models/pipeline.py:444-454)
            dd["max_pair_id"] = dd["gt_max_pair_id"]
            dd["pred_pos"] = torch.cat((dd["pair_pred_pos"], dd["pair_pred_pos"].new_zeros((1, 3))), 0)[dd["max_pair_id"]]
        loss_dict = lidf_loss(dd, loss_opt, "train", epoch)
    dd, loss_dict_refine = refine_forward_train(dd, pnet_model_refine, offset_dec_refine, opt, loss_opt, epoch)
    return True, dd, loss_dict, loss_dict_refine


def refine_forward(dd, pnet_model_refine, offset_dec_refine, opt=None, precision="f32", cell_lookup=True):
    """RefineNet.forward for evaluation (models/pipeline.py:1032-1041) on lidf_forward's data_dict:
    opt.refine_forward_times x get_pred_refine; adds pred_pos_refine and pred_depth_refine.
    cell_lookup: the end voxel of a ray through the cell table of get_occ_vox_bound's grid (the same ids as
    the reference's every-ray x every-voxel pcl_aabb, lidf_refine(grid=)); False tests every voxel."""
    opt = opt or LidfOptions()
    Q._refuse_autograd("pipeline.refine_forward", "pipeline.refine_forward_train (the stage-2 training step; its "
                       "differentiable core is query.lidf_refine_train)",
                       (("pred_pos", dd.get("pred_pos")),),
                       (("pnet_model_refine", pnet_model_refine), ("offset_dec_refine", offset_dec_refine)))
    bs, h, w = dd["bs"], dd["h"], dd["w"]
    occ_rev = dd["revidx"].to(torch.int32).contiguous()
    sel = None
    if opt.mask_type == "all" and not opt.refine_use_all_pix:
        inp_zero = (1 - dd["valid_mask"]).reshape(-1)
        sel = inp_zero.index_select(0, dd["miss_bid"] * (h * w) + dd["miss_flat_img_id"])
    valid_inp = dd["pnet_inp"]                     # cat(valid_v_rel_coord, valid_v_rgb), pipeline.py:1000
    if opt.refine_pnet_pos_type == "abs":          # :1001-1003
        valid_inp = torch.cat((dd["valid_xyz"].index_select(0, dd["valid_v_pid"]), dd["pnet_inp"][:, 3:]), -1)
    pos, end_voxel = Q.lidf_refine(
        dd["miss_ray_dir"], dd["ray_pix"], dd["ray_bid"], dd["ray_flat"], dd["pred_pos"],
        dd["max_pair_id"], dd["pair_vox"], dd["voxel_bound"], dd["voxel_bid"], dd["rgb_img"],
        dd["full_rgb_feat"], valid_inp.contiguous(), occ_rev, pnet_model_refine, offset_dec_refine,
        forward_times=opt.refine_forward_times, multires=opt.multires,
        multires_views=opt.multires_views, roi_inp_bbox=opt.roi_inp_bbox, roi_out_bbox=opt.roi_out_bbox,
        offset_range=opt.refine_offset_range, pos_rel=opt.refine_intersect_pos_type == "rel",
        pnet_pos_rel=opt.refine_pnet_pos_type == "rel", rayfeat=dd.get("rayfeat"),
        precision=precision, pnet_select=sel,
        grid=dd if (cell_lookup and all(k in dd for k in ("voxel_coord", "grid_dims", "xmin", "part_size"))) else None)
    dd["pred_pos_refine"], dd["end_voxel_id"] = pos, end_voxel
    depth = dd["xyz_corrupt_flat"][:, :, 2].reshape(-1).clone()
    depth[dd["miss_bid"] * (h * w) + dd["miss_flat_img_id"]] = pos[:, 2]
    dd["pred_depth_refine"] = depth.reshape(bs, h, w)
    return dd


def eval_metrics(dd, key="pred_depth", frame=0):
    """The nine ClearGrasp statistics of LIDF.compute_loss's bs == 1 branch
    (models/pipeline.py:577-627) for one frame, on the device. frame=None: every frame of the batch in one call
    (query.depth_metrics_frames), [bs] tensors whose entry b is the frame=b call's, bit for bit."""
    h, w = dd["h"], dd["w"]
    if frame is None:
        bs = dd["bs"]
        gt = dd["xyz_flat"][:, :, 2].reshape(bs, h, w).contiguous()
        return Q.depth_metrics_frames(dd[key].contiguous(), gt, dd["corrupt_mask"].reshape(bs, h, w))
    gt = dd["xyz_flat"][frame, :, 2].reshape(h, w).contiguous()
    return Q.depth_metrics(dd[key][frame].contiguous(), gt, dd["corrupt_mask"][frame])


def eval_loss(dd, loss_opt=None, exp_type="valid", epoch=0, stage=1, per_frame=False):
    """loss_dict of LIDF.forward(batch, 'valid' | 'test', epoch) (stage=1, models/pipeline.py:704-710) or of
    RefineNet.forward (stage=2, :1032-1041) on the data_dict of lidf_forward / refine_forward: compute_gt where its
    entries are missing, then losses.lidf_loss / losses.refine_loss in the evaluation flavour — the number a
    trainer's validate() picks its best checkpoint by. Every entry is a detached 0-dim device tensor.
    per_frame=True: every entry a [bs] tensor, entry b the loss_dict of frame b alone at bs == 1 — what the
    reference's test() reports per frame (losses.lidf_loss; losses.frame_slice(dd, b) is that frame's dict)."""
    from .losses import lidf_loss, refine_loss
    if stage not in (1, 2):
        raise ValueError("stage must be 1 or 2, not %r" % (stage,))
    if exp_type not in ("valid", "test"):
        raise ValueError("eval_loss is the evaluation flavour: exp_type 'valid' or 'test', not %r" % (exp_type,))
    return (lidf_loss if stage == 1 else refine_loss)(dd, loss_opt, exp_type, epoch, per_frame=per_frame)


# ------------------------------------------------------------------------------------------------
# The same evaluation path as ONE library call per batch, without a host round trip
# ------------------------------------------------------------------------------------------------
_FC = {"R": 0, "P": 1, "V": 2, "NV": 3, "NV0": 4, "NVS": 5, "NPN": 6, "OVERFLOW": 7}


class FrameRunner:
    """LIDF.forward (+ RefineNet.forward) for evaluation through lidf_frame_f32: every compacted list
    (valid points, occupied voxels, rays, ray/voxel pairs) lives in a buffer sized for the worst case
    and its length stays on the device, so a frame is enqueued without a single .item() / nonzero()
    size read (the reference — and lidf_forward above — stall the stream four times per frame), and
    the launch sequence depends on (batch, h, w, max_pairs) only: `capture()` records it into a HIP
    graph that `run()` replays.

        runner = FrameRunner(bs, h, w, device, pnet, prob_dec, offset_dec, opt,
                             pnet_refine=..., offset_dec_refine=...)
        runner.run(batch, full_rgb_feat)      # enqueue only (optionally: runner.capture(...) once)
        dd = runner.result()                  # ONE sync: reads the counts, returns the data_dict

    result() gives the reference's data_dict keys as views of the capacity buffers (int32 index
    tensors; `reference_dtypes=True` adds the int64 forms). mask_type 'all' / 'pred', every valid
    pixel, every opt.valid_stride-th, or — opt.valid_sample_num = n > 0, the shipped configs' 10000 — the random
    block sample of n valid pixels per image, drawn on the device at the head of the frame from `sampler_state`
    (query.sampler_state; default: opt.sampler_state, else the device's default state) without a sync and
    recorded into the graph, so every replay draws a fresh sample; result() raises on an image without a valid
    pixel; intersect_pos_type / refine_intersect_pos_type / refine_pnet_pos_type 'abs' or
    'rel'; precision "f32"
    or "f16x3" (as lidf_query / lidf_refine).
    max_pairs bounds the pair list (default 32 per pixel: a ray crosses at most 25 cells of the default 9^3
    grid); a frame with more pairs raises in result(). The default is a statement about the default grid: with
    opt.grid_res / xmin / xmax single rays exceed 32 pairs (at full occupancy up to 38 on 17^3, grid_res 16, and
    up to 44 in a 3 x 3 x 41 box — the kernel handles such rays), while the mean per pixel, which is what the
    capacity bounds, stays below (25.2 and 8.8 there); pass max_pairs for a finer grid that is densely occupied.
    offsets="selected" (opt-in; see query.lidf_query): the offset decoder runs on the arg-max pair of every ray
    only — pred_pos, the depth maps, stage 2 and the statistics are bit-identical, pred_offset / pair_pred_pos
    are meaningful at the selected pairs only (other rows: NaN, or a previous frame's selected values). With
    precision="f16x3" the statement holds for counts, voxel and ray features, pred_prob_end, the softmax and
    max_pair_id against the f16x3 frame with offsets="all"; positions and what follows from them are held to
    float64 by the split criterion instead (query.lidf_query).

    Decoder widths: prob_dec / offset_dec / offset_dec_refine of gf_dim 64 (every shipped config) run lidf_frame_f32.
    As soon as one of them has another width — each gf_dim 32, 64 or 128 with the reference's layers 4 gf -> 2 gf ->
    gf -> 1 (generic.chain_ok), IMNet or IEF, any n_iter, the three may differ — the frame runs
    lidf_frame_widths_f32: the same call, counts, graph capture and buffers, every decoder ONE register-chained
    launch per slab of pe_slab pairs (default generic.QUERY_SLAB; slab boundaries do not change a bit) / per refine
    iteration. Stage 1 equals lidf_forward at the same widths bit for bit, stage 2 within float rounding (its layer 1
    is factorised). That route is f32, offsets='all', one stream: precision="f16x3", offsets="selected" and
    side_stream=True are refused there, as is any other gf_dim / out_dim and LIDF_CHAIN16=0. The feature widths stay
    the shipped ones (rgb_out 32, roi_out_bbox 2, PointNet 6 -> 32 -> 128). chain_route=True sends gf_dim 64 decoders
    through that route as well (the A/B of the two routes at one width, scripts/frame_widths_time.py).

    Weight streams: the runner owns ONE blob with the packed streams of all its modules and the
    device-side fingerprints they were built from (nothing of it lives in the per-module caches, so a
    captured graph never references memory another call can free). Every frame re-validates them with one
    fingerprint launch over all parameter buffers (+ two early-exit pack launches, ~20 us) — in-place
    updates, `p.data` writes and load_state_dict are picked up by the next frame. guard_every = N > 1
    validates every N-th frame only and trusts the blob in between (evaluation loops whose parameters do
    not change: the reference's eval runs under torch.no_grad() with the modules in eval());
    `invalidate()` forces the check on the next frame; modules frozen with _lib.freeze_packed are
    validated once."""

    def __init__(self, bs, h, w, device, pnet_model, prob_dec, offset_dec, opt=None, pnet_model_refine=None,
                 offset_dec_refine=None, max_pairs=None, lds_voxels=None,
                 precision="f32", guard_every=1, offsets="all", side_stream=None, sampler_state=None, pe_slab=None,
                 chain_route=False):
        import ctypes as C
        import math
        from .decoders import is_shipped
        from .generic import chain_ok
        from .pointnet import check_pointnet
        self.C = C
        self.opt = opt = opt or LidfOptions()
        if opt.intersect_pos_type not in ("abs", "rel"):
            raise NotImplementedError("intersect_pos_type %s" % opt.intersect_pos_type)
        if opt.mask_type not in ("all", "pred"):
            raise NotImplementedError("mask_type %s" % opt.mask_type)
        if precision not in Q.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(Q.PRECISIONS))
        self.precision = precision
        if offsets not in ("all", "selected"):
            raise ValueError("offsets must be 'all' or 'selected'")
        self.offsets = offsets      # 'selected': offset_dec on the arg-max pair of every ray only (lidf_query)
        self.bs, self.h, self.w, self.dev = bs, h, w, torch.device(device)
        self.mods = (pnet_model, prob_dec, offset_dec, pnet_model_refine, offset_dec_refine)
        what = "FrameRunner (use lidf_forward / refine_forward, which run other widths layer by layer)"
        check_pointnet(pnet_model, what)
        if opt.roi_out_bbox != 2:
            raise RuntimeError("lidf_hip: %s is built for roi_out_bbox = 2" % what)
        self.refine = pnet_model_refine is not None
        if self.refine:
            check_pointnet(pnet_model_refine, what)
        # the decoders: the shipped gf_dim 64 (lidf_frame_f32), or gf_dim 32 / 64 / 128 each, one register-chained
        # launch per decoder (lidf_frame_widths_f32) as soon as one of them is not the shipped width
        decs = [prob_dec, offset_dec] + ([offset_dec_refine] if self.refine else [])
        self.widths = bool(chain_route) or not all(is_shipped(m) for m in decs)
        if self.widths:
            for m in decs:
                if not chain_ok(m):
                    raise RuntimeError(
                        "lidf_hip: FrameRunner takes decoders of gf_dim 32, 64 or 128 with the reference's layers "
                        "4 gf -> 2 gf -> gf -> 1 (out_dim 1; LIDF_CHAIN16=0 switches their one-launch kernel off); got "
                        "gf_dim=%d out_dim=%d. Use lidf_forward / refine_forward, which run other widths layer by layer"
                        % (m.gf_dim, m.linear_4.out_features))
            for bad, why in ((precision != "f32", "precision %r" % precision),
                             (offsets != "all", "offsets=%r" % offsets), (bool(side_stream), "side_stream=True")):
                if bad:
                    raise RuntimeError("lidf_hip: FrameRunner: %s is built for the shipped widths (gf_dim 64 in all "
                                       "three decoders); at gf_dim %s the frame runs f32, offsets='all', on the "
                                       "caller's stream alone" % (why, "/".join(str(m.gf_dim) for m in decs)))
            E = 3 + 6 * opt.multires
            D1, D2 = 256 + 2 * E + 3 + 6 * opt.multires_views, 256 + E + 3 + 6 * opt.multires_views
            for m, d in zip(decs, (D1, D1, D2)):
                if m.inp_dim != d:
                    raise RuntimeError("lidf_hip: FrameRunner: decoder inp_dim must be %d for this configuration "
                                       "(got %d)" % (d, m.inp_dim))
        if pe_slab is not None and int(pe_slab) < 1:
            raise ValueError("pe_slab must be a positive number of pairs")
        # the widened grid of LIDF.get_occ_vox_bound (models/pipeline.py:167-173), in the reference's f32
        t32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
        lo, hi = t32(opt.xmin), t32(opt.xmax)
        self.part_size = float(torch.min(hi - lo).item()) / opt.grid_res
        lo, hi = lo - 0.5 * self.part_size, hi + 0.5 * self.part_size
        self.xmin = [float(v) for v in lo.tolist()]
        self.res = [int(v) for v in torch.ceil((hi - lo) / self.part_size).tolist()]
        N, Cc = bs * h * w, bs * self.res[0] * self.res[1] * self.res[2]
        self.N, self.Cc = N, Cc
        self.max_pairs = int(max_pairs) if max_pairs else 32 * N
        # bound of the PointNet's LDS pooling tables. One frame: 288 (the largest table that fits; a frame
        # with more occupied voxels falls to per-point global atomics, +0.3 ms) at 1.5 % over the 128 that
        # lets two workgroups share a CU; batches: 128 (their larger tables take the voxel-sorted walk)
        self.lds_voxels = int(lds_voxels) if lds_voxels else (288 if bs == 1 else 128)
        Ed = 3 + 6 * opt.multires_views
        dev = self.dev
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        P = self.max_pairs
        self.buf = {
            "counts": torch.zeros((8,), **i32),
            "valid_bid": torch.empty((N,), **i32), "valid_flat": torch.empty((N,), **i32),
            "valid_xyz": torch.empty((N, 3), **f32), "valid_rgb": torch.empty((N, 3), **f32),
            "occ_bid_coord": torch.empty((Cc, 4), **i32), "voxel_bound": torch.empty((Cc, 6), **f32),
            "valid_v_pid": torch.empty((2 * N,), **i32), "revidx": torch.empty((2 * N,), **i32),
            "valid_v_rel_coord": torch.empty((N, 3), **f32), "pnet_inp": torch.empty((2 * N, 6), **f32),
            "occ_voxel_feat": torch.empty((Cc, 128), **f32),
            "ray_bid": torch.empty((N,), **i32), "ray_flat": torch.empty((N,), **i32),
            "ray_pix": torch.empty((N, 2), **i32), "ray_dir": torch.empty((N, 3), **f32),
            "pair_off": torch.zeros((N + 1,), **i32), "pair_ray": torch.empty((P,), **i32),
            "pair_vox": torch.empty((P,), **i32), "pair_t": torch.empty((P, 2), **f32),
            "pred_offset": torch.empty((P,), **f32), "pred_prob": torch.empty((P,), **f32),
            "pred_prob_softmax": torch.empty((P,), **f32), "pair_pred_pos": torch.empty((P, 3), **f32),
            "max_pair_id": torch.empty((N,), dtype=torch.int64, device=dev),
            "pred_pos": torch.empty((N, 3), **f32), "rayfeat": torch.empty((N, 128 + Ed), **f32),
            "pred_depth": torch.empty((bs, h, w), **f32),
        }
        if self.offsets == "selected":   # rows of the per-pair outputs that no frame writes must not look like results
            self.buf["pred_offset"].fill_(float("nan"))
            self.buf["pair_pred_pos"].fill_(float("nan"))
        if self.refine:
            self.buf.update({"pred_pos_refine": torch.empty((N, 3), **f32),
                             "end_voxel_id": torch.empty((N,), **i32),
                             "pred_depth_refine": torch.empty((bs, h, w), **f32)})
        L = _lib.lib()
        self.times = opt.refine_forward_times if self.refine else 0
        res = (C.c_int32 * 3)(*self.res)
        wsb = L.lidf_frame_workspace_bytes(bs, h, w, res, self.max_pairs, self.lds_voxels, self.times)
        self.ws = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=dev)
        # static inputs (a captured graph replays fixed addresses): load() copies a batch into them
        self.inp = {
            "rgb": torch.empty((bs, 3, h, w), **f32), "xyz_corrupt": torch.empty((bs, 3, h, w), **f32),
            "valid_mask": torch.empty((bs, h, w), **f32), "intr": torch.empty((bs, 4), **f32),
            "feat_grid": torch.empty((bs, 32, h, w), **f32),
            "miss_mask": torch.empty((bs, h, w), **f32) if opt.mask_type == "pred" else None,
        }
        self.graph = None
        self.graph_trusted = None                  # the same launch sequence without the guard (guard_every > 1)
        self._keep = None
        self.guard_every = max(1, int(guard_every))
        self._frames_since_guard = None            # None: the next frame validates
        # side_stream (lidf_hip.h: LidfFrameArgs.aux_stream): the weight-stream guard, the box sums and the
        # per-ray features of a frame run on a second stream beside its head, voxel list, pairs and PointNet;
        # bit-identical results. None (default) = for eager calls only: a replayed graph pays more for the
        # cross-stream edges than they save, and frames pipelined over several streams fill each other's gaps
        # already (FramePipeline passes False). True / False force it.
        # In a process that also runs a process group (RCCL creates streams of its own) HIP's default of 4 hardware
        # queues can put this side stream and the caller's stream on ONE queue: the fork then runs in sequence and a
        # frame is 6 % slower than without the group (A/B in one session, profiles/r06_ab_pg.txt: 1.660 ms plain,
        # 1.766 under a 1-rank nccl group, 1.675 with GPU_MAX_HW_QUEUES=8, 1.700 without the side stream). Export
        # GPU_MAX_HW_QUEUES=8 before the first HIP call of such a process (bench.py --workload e2e --gpus N does).
        self.side_mode = side_stream
        self.side = None                           # (stream, ev_fork, ev_join): created by the first frame that forks
        self._fail_after = 0                       # LidfFrameArgs.fail_after (test hook: a mid-frame failure)
        self.profile_events = None                 # benchmarks: six hipEvent_t recorded around the matrix launches
        self.pack_blob = torch.empty((L.lidf_frame_pack_bytes(),), dtype=torch.uint8, device=dev)
        self.pack_guard = torch.zeros((L.lidf_frame_pack_guard_bytes(),), dtype=torch.uint8, device=dev)
        self.wd = None
        if self.widths:
            # LidfFrameWidths: the runner's second workspace (layer-1 tables, the slab of embedding rows), the three
            # chain streams and their fingerprints — owned here like pack_blob / pack_guard above. The bias rows
            # (b1 + an IEF's W1[:, enc] benc) are formed by generic._bias_row inside every frame — captured with it —
            # so that a row's bits are the stepwise path's
            wd = _lib.LidfFrameWidths()
            wd.prob_gf, wd.off_gf = int(prob_dec.gf_dim), int(offset_dec.gf_dim)
            wd.refine_gf = int(offset_dec_refine.gf_dim) if self.refine else 0
            wd.pe_slab_pairs = int(pe_slab) if pe_slab else 0
            wwb = L.lidf_frame_widths_workspace_bytes(bs, h, w, res, self.max_pairs, self.times, opt.multires,
                                                      opt.multires_views, C.byref(wd))
            wpb = L.lidf_frame_widths_pack_bytes(opt.multires, opt.multires_views, C.byref(wd))
            if not wwb or not wpb:
                raise RuntimeError("lidf_hip: FrameRunner: multires %d / multires_views %d outside the frame's range"
                                   % (opt.multires, opt.multires_views))
            self.ws_widths = torch.empty((wwb,), dtype=torch.uint8, device=dev)
            self.pack_blob_widths = torch.empty((wpb,), dtype=torch.uint8, device=dev)
            self.pack_guard_widths = torch.zeros((L.lidf_frame_widths_pack_guard_bytes(),), dtype=torch.uint8,
                                                 device=dev)
            self.bias_rows = [torch.empty((4 * int(m.gf_dim),), **f32) for m in decs]
            wd.workspace, wd.workspace_bytes = self.ws_widths.data_ptr(), wwb
            wd.pack_blob, wd.pack_blob_bytes = self.pack_blob_widths.data_ptr(), wpb
            wd.pack_guard = self.pack_guard_widths.data_ptr()
            for name, t in zip(("prob_bias", "off_bias", "refine_bias"), self.bias_rows):
                setattr(wd, name, t.data_ptr())
            self.wd = wd
        self.vidx, self.n_valid_idx = None, 0      # explicit valid points (load(valid_idx=))
        # opt.valid_sample_num > 0: every frame starts with query.sample_valid_launch on the frame's valid mask,
        # straight into vidx (no sync; part of the captured graph) unless load() was handed an explicit valid_idx
        self.sample_n = opt.sample_num()
        self._sample_now = bool(self.sample_n)
        if self.sample_n:
            if h % 8 or w % 8:
                raise ValueError("valid_sample_num needs h = %d and w = %d to be multiples of the 8 x 8 block" % (h, w))
            if self.sample_n > h * w:
                raise ValueError("valid_sample_num = %d exceeds the %d pixels of an image" % (self.sample_n, h * w))
            self.vidx = torch.empty((2, N), **i32)
            self.sample_cnt = torch.ones((bs,), **i32)
            self.sample_ws = Q.sample_valid_workspace(bs, h, w, dev)
            st = sampler_state if sampler_state is not None else opt.sampler_state
            self.sampler_state = Q.default_sampler_state(dev) if st is None else st
            Q._check_sampler_state(self.sampler_state, dev)
            self.n_valid_idx = bs * self.sample_n
        self.src = dict(self.inp)
        math.isfinite(self.part_size)

    # -- inputs -----------------------------------------------------------------------------------
    def load(self, batch, full_rgb_feat, pred_mask=None, copy=None, valid_idx=None):
        """Hand a batch (the reference's dataset item keys) to the runner. mask_type 'all': valid <=>
        the measured depth is non-zero (prepare_data, pipeline.py:119-121), so depth_corrupt itself is
        the valid mask; 'pred': valid_mask = 1 - pred_mask, rays where pred_mask is non-zero.
        valid_idx [M,2] (image, flat pixel; any integer dtype, M <= bs*h*w): the valid points as the
        code upstream sampled them (LIDF.get_valid_points with grid.valid_sample_num != -1 keeps the
        output of utils/point_utils.py sample_valid_points) instead of every opt.valid_stride-th valid
        pixel; copied into the runner's static index buffers without a sync. A captured graph replays
        the M it was captured with. A runner with opt.valid_sample_num > 0 draws its own sample on the device
        at the head of every frame; an explicit valid_idx replaces the draw for that frame (eager frames only:
        a captured graph holds the sampler launch).
        copy=True (the default once a graph is captured: a graph replays fixed addresses) copies the
        tensors into the runner's static input buffers — device-to-device, no sync; copy=False passes
        the caller's own contiguous float32 tensors to the library as they lie (kept alive by the
        runner until the next load)."""
        copy = (self.graph is not None) if copy is None else copy
        bs, h, w = self.bs, self.h, self.w
        i = self.inp
        intr = [batch[k].reshape(bs) for k in ("fx", "fy", "cx", "cy")]
        if all(t.dtype == torch.float32 for t in intr):
            torch.stack(intr, 1, out=i["intr"])
        else:
            i["intr"].copy_(torch.stack(intr, 1), non_blocking=True)
        if self.opt.mask_type == "all":
            valid, miss = batch["depth_corrupt"].reshape(bs, h, w), None
        else:
            miss = pred_mask.reshape(bs, h, w)
            valid = None
        srcs = {"rgb": batch["rgb"], "xyz_corrupt": batch["xyz_corrupt"], "feat_grid": full_rgb_feat,
                "valid_mask": valid, "miss_mask": miss}
        direct = not copy and all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                                                and t.device == self.dev) for t in srcs.values())
        if direct:
            self.src = dict(srcs, intr=i["intr"])
        else:
            if self.graph is None and not copy:
                copy = True   # (not plain contiguous float32 device tensors: go through the static buffers)
            for k in ("rgb", "xyz_corrupt", "feat_grid"):
                i[k].copy_(srcs[k], non_blocking=True)
            if valid is not None:
                i["valid_mask"].copy_(valid, non_blocking=True)
            if miss is not None:
                i["miss_mask"].copy_(miss, non_blocking=True)
            self.src = dict(i)
        if miss is not None:   # valid_mask = 1 - pred_mask (prepare_data, pipeline.py:116-117)
            torch.sub(1.0, self.src["miss_mask"], out=i["valid_mask"])
            self.src["valid_mask"] = i["valid_mask"]
        m = 0
        if self.sample_n:
            if valid_idx is not None and self.graph is not None:
                raise RuntimeError("the captured graph draws its valid points itself (valid_sample_num = %d); it "
                                   "cannot take an explicit valid_idx" % self.sample_n)
            self._sample_now = valid_idx is None
            m = self.bs * self.sample_n
        if valid_idx is not None:
            if valid_idx.dim() != 2 or valid_idx.shape[1] != 2:
                raise RuntimeError("valid_idx must be [M,2] (image, flat pixel)")
            m = int(valid_idx.shape[0])
            if m > self.N:
                raise RuntimeError("valid_idx holds %d points, the frame buffers %d" % (m, self.N))
            if self.vidx is None:
                self.vidx = torch.empty((2, self.N), dtype=torch.int32, device=self.dev)
            if m:
                self.vidx[:, :m].copy_(valid_idx.t(), non_blocking=True)
        if self.graph is not None and m != self.n_valid_idx:
            raise RuntimeError("the captured graph replays %d listed valid points, this batch has %d"
                               % (self.n_valid_idx, m))
        self.n_valid_idx = m

    # -- the launch sequence ------------------------------------------------------------------------
    def invalidate(self):
        """The next frame re-validates the packed weight streams (guard_every > 1, frozen modules)."""
        self._frames_since_guard = None

    def _guard_due(self):
        """Whether the coming frame fingerprints the parameters (and re-packs what changed)."""
        n = self._frames_since_guard
        if n is None:
            return True
        if all(m is None or m in _lib.FROZEN for m in self.mods):
            return False
        return n >= self.guard_every

    def enqueue(self, guard=True):
        """lidf_frame_f32 on the static inputs: one fingerprint launch over every module's parameters +
        the early-exit packs (guard=True) + the frame; nothing here reads a size or waits for the device."""
        from .decoders import _decoder_struct
        from .pointnet import pointnet_struct
        C = self.C
        pnet, prob, off, pnet_r, off_r = self.mods
        opt, b, i = self.opt, self.buf, self.src
        keep = []
        if self._sample_now:   # ahead of the frame and of its side-stream fork, on the caller's stream
            Q.sample_valid_launch(i["valid_mask"], self.sample_n, self.sampler_state, self.vidx[0], self.vidx[1],
                                  None, self.sample_cnt, self.sample_ws)
        dp, do = _decoder_struct(prob, keep), _decoder_struct(off, keep)
        pn = pointnet_struct(pnet, keep)
        a = _lib.LidfFrameArgs()
        a.batch, a.height, a.width = self.bs, self.h, self.w
        for k in ("rgb", "xyz_corrupt", "valid_mask", "intr", "feat_grid"):
            setattr(a, k, i[k].data_ptr())
        a.miss_mask = i["miss_mask"].data_ptr() if i["miss_mask"] is not None else None
        a.xmin = (C.c_float * 3)(*self.xmin)
        a.res = (C.c_int32 * 3)(*self.res)
        a.part_size = self.part_size
        a.valid_stride = int(opt.valid_stride) if opt.valid_stride and opt.valid_stride > 1 else 1
        a.pnet, a.prob, a.off = C.pointer(pn), C.pointer(dp), C.pointer(do)
        a.packed_query = None
        a.multires, a.multires_views, a.roi_inp_bbox = opt.multires, opt.multires_views, opt.roi_inp_bbox
        a.pos_rel = int(opt.intersect_pos_type == "rel")
        a.offset_range0, a.offset_range1 = float(opt.offset_range[0]), float(opt.offset_range[1])
        a.refine_times = self.times
        a.precision = Q.PRECISIONS[self.precision]
        if self.refine:
            dr = _decoder_struct(off_r, keep)
            pr = pointnet_struct(pnet_r, keep)
            a.pnet_refine, a.off_refine, a.packed_refine = C.pointer(pr), C.pointer(dr), None
            a.refine_pos_rel = int(opt.refine_intersect_pos_type == "rel")
            a.refine_pnet_pos_rel = int(opt.refine_pnet_pos_type == "rel")
            a.refine_use_all_pix = int(bool(opt.refine_use_all_pix) or opt.mask_type != "all")
            a.refine_offset_range0 = float(opt.refine_offset_range[0])
            a.refine_offset_range1 = float(opt.refine_offset_range[1])
        a.max_pairs, a.lds_voxels = self.max_pairs, self.lds_voxels
        for k, t in b.items():
            setattr(a, k, t.data_ptr())
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        if self.n_valid_idx > 0:
            a.valid_idx_bid, a.valid_idx_flat = self.vidx[0].data_ptr(), self.vidx[1].data_ptr()
            a.n_valid_idx = self.n_valid_idx
        # the runner's own packed streams + fingerprints (lidf_hip.h: LIDF_FRAME_PACK_GUARDED / _TRUSTED)
        a.pack_blob, a.pack_blob_bytes = self.pack_blob.data_ptr(), self.pack_blob.numel()
        a.pack_guard = self.pack_guard.data_ptr()
        a.pack_mode = 1 if guard else 2
        a.offsets_selected = int(self.offsets == "selected")
        if self.widths:   # the any-width route runs on the caller's stream alone; its bias rows are part of the frame
            from .generic import _bias_row
            if guard:   # (a trusted frame keeps the rows of the last validated one, as it keeps the streams)
                for t, m in zip(self.bias_rows, (prob, off, off_r)):
                    t.copy_(_bias_row(m))
        elif self.side_mode or (self.side_mode is None and not torch.cuda.is_current_stream_capturing()):
            if self.side is None:   # the side stream and its two events exist only for runners that fork
                with torch.cuda.device(self.dev):
                    self.side = (torch.cuda.Stream(self.dev), _lib.hip_event(), _lib.hip_event())
            a.aux_stream, a.ev_fork, a.ev_join = self.side[0].cuda_stream, self.side[1], self.side[2]
        a.fail_after = int(self._fail_after)
        if self.profile_events is not None:   # (benchmarks: six hipEvent_t, LidfFrameArgs.profile_events)
            self._pev = (C.c_void_p * 6)(*[e if isinstance(e, C.c_void_p) else C.c_void_p(e)
                                           for e in self.profile_events])
            a.profile_events = C.cast(self._pev, C.POINTER(C.c_void_p))
        try:
            with torch.cuda.device(self.dev):
                if self.widths:
                    _lib.check(_lib.lib().lidf_frame_widths_f32(C.byref(a), C.byref(self.wd),
                                                                _lib.current_stream(self.dev)))
                else:
                    _lib.check(_lib.lib().lidf_frame_f32(C.byref(a), _lib.current_stream(self.dev)))
        except RuntimeError:
            self._frames_since_guard = None   # (the library reset the fingerprints; validate again)
            raise
        self._keep = keep

    def __del__(self):
        # the two raw events of the side stream are the runner's (created through the library)
        side, self.side = getattr(self, "side", None), None
        if side is not None:
            try:
                self.graph = self.graph_trusted = None   # (a captured graph may reference them)
                torch.cuda.synchronize(self.dev)
                _lib.hip_event_destroy(side[1]), _lib.hip_event_destroy(side[2])
            except Exception:   # interpreter shutdown: the process releases them
                pass

    def capture(self):
        """Record enqueue() into a HIP graph (torch.cuda.CUDAGraph) after one eager warm-up call; run()
        then replays it. The graph holds the parameters' CURRENT storage pointers: in-place updates are
        picked up by the fingerprint check inside the graph, a replaced `.data` needs a new capture.
        With guard_every > 1 (or frozen modules) a second graph without the check is recorded as well."""
        for k, t in self.src.items():        # a batch handed over in place moves into the static buffers:
            if t is not None and self.inp.get(k) is not None and t is not self.inp[k]:
                self.inp[k].copy_(t)         # the graph reads those
        self.src = dict(self.inp)
        # warm-up on the stream the capture will use: kernel attributes are set, the packed weight
        # streams exist (and are valid), nothing is allocated during the capture
        st = torch.cuda.Stream(self.dev)
        st.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(st):
            self.enqueue(True)
        torch.cuda.synchronize(self.dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            self.enqueue(True)
        self.graph = g
        self.graph_trusted = None
        if self.guard_every > 1 or all(m is None or m in _lib.FROZEN for m in self.mods):
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, stream=st):
                self.enqueue(False)
            self.graph_trusted = g2
        self._frames_since_guard = None
        return self

    def run(self, batch=None, full_rgb_feat=None, pred_mask=None, valid_idx=None):
        """load() (when a batch is given) + the frame (graph replay if captured). No sync."""
        Q._refuse_autograd("pipeline.FrameRunner.run", "query.lidf_query_train (stage-1 training step)",
                           (("full_rgb_feat", full_rgb_feat),),
                           tuple(zip(("pnet_model", "prob_dec", "offset_dec", "pnet_model_refine",
                                      "offset_dec_refine"), self.mods)))
        if batch is not None:
            self.load(batch, full_rgb_feat, pred_mask, valid_idx=valid_idx)
        guard = self._guard_due()
        if self.graph is not None:
            (self.graph if guard or self.graph_trusted is None else self.graph_trusted).replay()
        else:
            self.enqueue(guard)
        self._frames_since_guard = 1 if guard else self._frames_since_guard + 1
        return self

    # -- outputs ------------------------------------------------------------------------------------
    def counts(self):
        """The list lengths (ONE device -> host copy; the only sync of a frame)."""
        c = self.buf["counts"].tolist()
        return {k: c[i] for k, i in _FC.items()}

    def result(self, reference_dtypes=False):
        """(success, data_dict) as lidf_forward / refine_forward return them: views of the capacity
        buffers cut to the frame's counts. success False = one of the reference's early exits (no
        occupied voxel / no ray / no pair: the launches ran on empty lists)."""
        c = self.counts()
        if c["OVERFLOW"]:
            raise RuntimeError("FrameRunner: the frame has more than max_pairs = %d ray/voxel pairs; "
                               "construct the runner with a larger max_pairs" % self.max_pairs)
        if self._sample_now:
            Q.raise_on_empty_image(self.sample_cnt.tolist(), "FrameRunner (valid_sample_num = %d)" % self.sample_n)
        b, R, P, V, NV, NVS = self.buf, c["R"], c["P"], c["V"], c["NV"], c["NVS"]
        dd = {
            "bs": self.bs, "h": self.h, "w": self.w, "part_size": self.part_size,
            "xmin": torch.tensor(self.xmin, device=self.dev), "grid_dims": tuple(self.res),
            "valid_bid": b["valid_bid"][:NVS], "valid_flat_img_id": b["valid_flat"][:NVS],
            "valid_xyz": b["valid_xyz"][:NVS], "valid_rgb": b["valid_rgb"][:NVS],
            "occ_vox_bid": b["occ_bid_coord"][:V, 0], "occ_vox_global_coord": b["occ_bid_coord"][:V, 1:],
            "voxel_bound": b["voxel_bound"][:V], "valid_v_pid": b["valid_v_pid"][:NV],
            "revidx": b["revidx"][:NV], "valid_v_rel_coord": b["valid_v_rel_coord"][:NV],
            "pnet_inp": b["pnet_inp"][:NV], "occ_voxel_feat": b["occ_voxel_feat"][:V],
            "ray_bid": b["ray_bid"][:R], "ray_flat": b["ray_flat"][:R], "ray_pix": b["ray_pix"][:R],
            "miss_ray_dir": b["ray_dir"][:R], "total_miss_sample_num": R,
            "pair_off": b["pair_off"][:R + 1], "pair_ray": b["pair_ray"][:P], "pair_vox": b["pair_vox"][:P],
            "pair_t": b["pair_t"][:P], "pred_offset": b["pred_offset"][:P].unsqueeze(1),
            "pred_prob_end": b["pred_prob"][:P].unsqueeze(1), "pair_pred_pos": b["pair_pred_pos"][:P],
            "pred_prob_end_softmax": b["pred_prob_softmax"][:P], "max_pair_id": b["max_pair_id"][:R],
            "pred_pos": b["pred_pos"][:R], "rayfeat": b["rayfeat"][:R], "pred_depth": b["pred_depth"],
            "full_rgb_feat": self.src["feat_grid"], "rgb_img": self.src["rgb"], "counts": c,
        }
        if reference_dtypes:   # the reference's int64 index tensors (torch.nonzero / torch.unique)
            dd["miss_bid"], dd["miss_flat_img_id"] = dd["ray_bid"].long(), dd["ray_flat"].long()
            dd["miss_img_ind"] = dd["ray_pix"].long()
            for k in ("valid_bid", "valid_flat_img_id", "occ_vox_bid", "occ_vox_global_coord", "valid_v_pid",
                      "revidx"):
                dd[k] = dd[k].long()
        ok = V > 0 and R > 0 and P > 0
        if self.refine and ok:
            dd["pred_pos_refine"] = b["pred_pos_refine"][:R]
            dd["end_voxel_id"] = b["end_voxel_id"][:R]
            dd["pred_depth_refine"] = b["pred_depth_refine"]
        return ok, dd

    def loss_dict(self, batch, loss_opt=None, exp_type="valid", epoch=0, per_frame=False):
        """What a trainer's validate() / test() reads after a frame: eval_loss on result()'s data_dict plus what it
        lacks — xyz_flat, xyz_corrupt_flat and corrupt_mask of `batch`. Returns (success, loss_dict of stage 1,
        loss_dict of stage 2 — {} without refinement); success False (an early exit of the frame): two empty dicts.
        It reads the frame's counts as result() does and touches neither the frame call, its graph nor its
        workspace. per_frame=True: [bs] tensors, entry b the bs == 1 loss_dict of frame b (eval_loss), with no host
        read beyond the counts."""
        ok, dd = self.result()
        if not ok:
            return False, {}, {}
        bs = self.bs
        dd["xyz_flat"] = batch["xyz"].permute(0, 2, 3, 1).contiguous().reshape(bs, -1, 3)
        dd["xyz_corrupt_flat"] = batch["xyz_corrupt"].permute(0, 2, 3, 1).contiguous().reshape(bs, -1, 3)
        dd["corrupt_mask"] = batch["corrupt_mask"].reshape(bs, self.h, self.w)
        loss1 = eval_loss(dd, loss_opt, exp_type, epoch, stage=1, per_frame=per_frame)
        return True, loss1, (eval_loss(dd, loss_opt, exp_type, epoch, stage=2, per_frame=per_frame)
                             if self.refine else {})

    def metrics(self, batch, key=None, frame=0):
        """The nine ClearGrasp statistics (models/pipeline.py:577-627) of frame `frame` on the device:
        xyz[frame, 2] of the NCHW batch is the ground-truth depth map as it lies (no copy). frame=None: every frame
        in one call (query.depth_metrics_frames; the depth planes are gathered into one [bs,h,w] tensor), [bs]
        tensors whose entry b is the frame=b call's, bit for bit."""
        key = key or ("pred_depth_refine" if self.refine else "pred_depth")
        if frame is None:
            return Q.depth_metrics_frames(self.buf[key], batch["xyz"][:, 2].contiguous(),
                                          batch["corrupt_mask"].reshape(self.bs, self.h, self.w))
        seg = batch["corrupt_mask"].reshape(self.bs, self.h, self.w)[frame]
        return Q.depth_metrics(self.buf[key][frame], batch["xyz"][frame, 2], seg)


class FramePipeline:
    """Independent frames pipelined over S streams (2.09 -> 1.61 ms per 240x320 frame at
    S = 3 on one MI355X): S FrameRunners, each with its own buffers, packed-weight entries and HIP
    stream, take the batches in turn, so that one frame's low-occupancy stretches (PointNet chains, the
    per-voxel layers, scans, the partial last round of the matrix kernels) are filled by its neighbours'
    kernels. Frames come back in submission order, each with its one size read. opt.valid_sample_num and
    sampler_state are FrameRunner's (every lane samples from its own state).

        pipe = FramePipeline(3, bs, h, w, device, pnet, prob_dec, offset_dec, opt, pnet_refine, offset_refine)
        for batch in loader:
            if pipe.full:
                ok, data_dict, metrics = pipe.collect()            # the oldest frame; frees its runner
                ...                                                # use (or clone) data_dict here
            pipe.submit(batch, lidf.resnet_model(batch['rgb']))   # enqueue only
        while pipe.pending:
            ok, data_dict, metrics = pipe.collect()

    data_dict holds views of a runner's buffers, valid until the submit() that reuses the runner (the one
    after S - 1 further submits). A runner's stream waits for the caller's current stream before it starts
    a frame: inputs produced there and reads of the previous result enqueued there are ordered before it.
    metrics_frame: the frame whose statistics submit() records (FrameRunner.metrics' `frame`; default 0); None
    records every frame of the batch in one call, [bs] tensors."""

    def __init__(self, streams, bs, h, w, device, *models, with_metrics=True, metrics_frame=0, **kw):
        if streams < 1:
            raise ValueError("streams must be >= 1")
        self.dev = torch.device(device)
        if streams > 1:
            kw.setdefault("side_stream", False)   # (the lanes fill each other's gaps: see FrameRunner)
        # opt.valid_sample_num: every lane draws from a state of its own (the base state with the lane number added
        # to the seed) — lanes run on different streams, and one shared counter would be advanced by all of them
        opt = kw.get("opt") or (models[3] if len(models) > 3 else None)
        states = [kw.pop("sampler_state", None)] * streams
        if opt is not None and opt.sample_num() and streams > 1:
            base = states[0] if states[0] is not None else opt.sampler_state
            base = Q.default_sampler_state(self.dev) if base is None else base
            states = [base.clone() for _ in range(streams)]
            for k, st in enumerate(states):
                st[0] += k
        self.runners = [FrameRunner(bs, h, w, device, *models, sampler_state=states[k], **kw) for k in range(streams)]
        self.lanes = [torch.cuda.Stream(self.dev) for _ in range(streams)]
        self.with_metrics = with_metrics
        self.metrics_frame = metrics_frame   # FrameRunner.metrics' frame: None records every frame ([bs] tensors)
        self.pending = []          # [(slot, metrics)] in submission order
        self.n = 0

    @property
    def full(self):
        return len(self.pending) == len(self.runners)

    def submit(self, batch, full_rgb_feat, pred_mask=None, valid_idx=None):
        if self.full:
            raise RuntimeError("FramePipeline: %d frames in flight — collect() the oldest first" % len(self.pending))
        slot = self.n % len(self.runners)
        self.n += 1
        lane = self.lanes[slot]
        lane.wait_stream(torch.cuda.current_stream(self.dev))
        # the lane reads the caller's tensors (copies into the runner's static buffers, the library call when
        # they are handed over in place, the metrics kernel): tell the caching allocator, or a tensor the
        # caller drops on its next loop iteration could be handed out again on the caller's stream while the
        # lane's reads are still queued
        for t in list(batch.values()) + [full_rgb_feat, pred_mask, valid_idx]:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(lane)
        with torch.cuda.stream(lane), torch.no_grad():
            self.runners[slot].run(batch, full_rgb_feat, pred_mask, valid_idx=valid_idx)
            m = self.runners[slot].metrics(batch, frame=self.metrics_frame) if self.with_metrics else None
        self.pending.append((slot, m))

    def collect(self):
        """(success, data_dict, metrics) of the oldest frame in flight (waits for that frame only)."""
        if not self.pending:
            raise RuntimeError("FramePipeline: nothing in flight")
        slot, m = self.pending.pop(0)
        with torch.cuda.stream(self.lanes[slot]):
            ok, dd = self.runners[slot].result()
        return ok, dd, m
