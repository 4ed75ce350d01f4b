"""GPU: the evaluation path on voxel grids other than the shipped 9 x 9 x 9 one (tests/grids.py) against the oracle.
On the shipped grid the cell edge is 0.25, so no operation of the voxel arithmetic rounds, every ray crosses at most
25 cells, a column of cells has one mask word and the cell table fits the grid walk's LDS. Here: cell edges that
are no binary fraction (v / crop, c * crop + crop / 2, xmin + c * crop and lo + crop round), per-axis cell counts that
differ, rays with more than the 32 hits lidf_ray_aabb_onepass_kernel keeps in LDS, columns of two mask words, a
cell table read from global memory, and a pair list cut inside a ray's run. Geometry is compared bit for bit;
predictions within the tolerances of test_frame_gpu.test_frame_vs_oracle_and_reference_dtypes. What each grid is
there for is asserted on the CPU in tests/test_grids.py."""
import pytest
import torch

import grids
from test_frame_gpu import _compare, _dev, _models, _stepwise
from test_voxelize_gpu import check
from util import TOL, orc

pytestmark = pytest.mark.gpu

NAMES = [g[0] for g in grids.ALL]


# ------------------------------------------------------------------------------------------------
# a. voxel build
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_voxel_build(cuda, name, B):
    """get_occ_vox_bound against orc.occupied_voxels, bit for bit (test_voxelize_gpu.check): uniform points reaching
    outside the grid, points exactly on computed cell faces, their nextafter neighbours on both sides, one far
    point — and, in a second pass, the first pass' stored voxel_bound values fed back in as points."""
    from implicit_depth_amd.query import get_occ_vox_bound
    grid = grids.BY_NAME[name]
    dims = grids.widened(*grid[1:])[2]
    stored = None
    for rnd in range(2):
        xyz, bid = grids.voxel_points(grid, B, 20000, seed=10 * B + rnd, stored=stored)
        ref = orc.occupied_voxels(xyz, bid, *grid[1:])
        res = get_occ_vox_bound(xyz.to(cuda), bid.int().to(cuda), B, *grid[1:])
        assert tuple(res["grid_dims"]) == dims
        assert 0 < ref["valid_v_pid"].numel() < xyz.shape[0]          # points inside and outside
        check(res, ref)
        assert torch.equal(res["voxel_coord"].cpu().long(), ref["occ_vox_global_coord"])
        stored = res["voxel_bound"]


# ------------------------------------------------------------------------------------------------
# b. ray / voxel lists: dense, compact and the grid walk
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one", "frames", "shuffled"])
@pytest.mark.parametrize("name", NAMES)
def test_ray_voxel_lists(cuda, name, mode):
    """ray_aabb.forward (dense), compute_ray_aabb (compact) and compute_ray_aabb(voxel_coord=, grid_dims=, batch=)
    (the grid walk) on the voxels get_occ_vox_bound builds, against orc.ray_aabb + orc.pairs_from_dense: mask,
    distances and the ray-major lists bit for bit. 969 rays (no multiple of the 256-ray workgroups): the camera
    rays of a 24 x 32 image, random directions, the axes, a reversed pair, one pointing away.
    'one': a single frame. 'frames': three frames, frame-major rays — the workgroups on a frame boundary read the
    grid walk's tables from global memory, the others stage them in LDS (where they fit: not on res20).
    'shuffled': three frames, random frame per ray — every workgroup on the global route."""
    from implicit_depth_amd.extensions import ray_aabb
    from implicit_depth_amd.query import compute_ray_aabb, get_occ_vox_bound
    grid = grids.BY_NAME[name]
    B = 1 if mode == "one" else 3
    # about 1000 voxels (the oracle's dense V x R form stays small); the long box full (369 cells a frame), the
    # 21^3 grid at 8 %
    fill = {"long_box": 1.0, "res20": 0.08}.get(name, min(1.0, 1000.0 / (B * grids.cells_of(grid))))
    d, rb, occ, pts, pbid = grids.grid_scene(grid, B, fill, seed=len(name) + B,
                                             ray_order="shuffled" if mode == "shuffled" else "frames")
    dev_occ = get_occ_vox_bound(pts.to(cuda), pbid.int().to(cuda), B, *grid[1:])
    check(dev_occ, occ)
    vb, vbid = dev_occ["voxel_bound"], dev_occ["occ_vox_bid"].int().contiguous()
    V, R = vb.shape[0], d.shape[0]
    assert R % 256 != 0 and R <= 1000
    m_ref, t_ref = orc.ray_aabb(d.numpy(), occ["voxel_bound"].numpy(), rb.numpy(), occ["occ_vox_bid"].numpy())
    pr_ref, pv_ref, pt_ref, off_ref = orc.pairs_from_dense(m_ref, t_ref)
    if name == "long_box":   # every cell occupied: the central camera rays cross more than 32 cells
        assert fill == 1.0 and int((off_ref[1:] - off_ref[:-1]).max()) > grids.AABB_HITS
    t = [d.to(cuda), vb, rb.to(cuda), vbid]
    mask, dist = ray_aabb.forward(*t)
    assert mask.shape == (V, R) and (mask.cpu().numpy() == m_ref).all()
    assert (dist.cpu().numpy() == t_ref).all()
    compact = compute_ray_aabb(*t)
    walk = compute_ray_aabb(*t, voxel_coord=dev_occ["voxel_coord"], grid_dims=dev_occ["grid_dims"], batch=B)
    for a, b in zip(walk, compact):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for got in (compact, walk):
        assert torch.equal(got[0].cpu().long(), off_ref)
        assert torch.equal(got[1].cpu().long(), pr_ref) and torch.equal(got[2].cpu().long(), pv_ref)
        assert torch.equal(got[3].cpu(), pt_ref)
    assert pr_ref.numel() > 0


# ------------------------------------------------------------------------------------------------
# c. the end voxel of stage 2 through the cell table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frames,occupancy", [("res10", 2, 0.4), ("res12", 2, 0.4), ("flat", 3, 0.4),
                                                   ("offset", 2, 1.0), ("res20", 1, 0.1), ("long_box", 2, 1.0)])
def test_refine_end_voxel_on_other_grids(cuda, name, frames, occupancy):
    """test_refine_gpu.test_refine_end_voxel_through_the_cell_table on the grids whose stored bounds are rounded
    (the 27-cell neighbourhood is tested against the stored bounds because the cell estimate is only right to within
    one cell there) and on the long box: lidf_refine(grid=) against the every-voxel route (ids equal, positions
    bit-equal) and both against the definition on the CPU. The query points also hold the nextafter neighbours of the
    stored bounds."""
    from test_refine_gpu import check_end_voxel_lookup
    check_end_voxel_lookup(cuda, frames, occupancy, grids.BY_NAME[name], neighbours=True)


# ------------------------------------------------------------------------------------------------
# d. the whole path: frame call against stepwise path against oracle
# ------------------------------------------------------------------------------------------------
def _oracle_stage1(batch, feat, grid, pos_rel):
    """orc.lidf_forward on the grid; intersect_pos_type 'rel' (which lidf_forward does not restate): its geometry,
    then orc.query with the voxel centres."""
    from implicit_depth_amd.synthetic import init_decoder_params
    pnet_p = orc.init_pointnet(3, 1.5)                                   # test_frame_gpu._models' parameters
    prob_p, off_p = init_decoder_params("IMNET", 385, 7, 5.0), init_decoder_params("IEF", 385, 8, 5.0)
    ok, ref = orc.lidf_forward(batch, feat, pnet_p, prob_p, off_p, xmin=grid[1], xmax=grid[2], grid_res=grid[3])
    assert ok
    if pos_rel:
        vb = ref["voxel_bound"]
        out = orc.query(ref["miss_ray_dir"], ref["miss_img_ind"], ref["miss_bid"], ref["pair_ray"], ref["pair_vox"],
                        ref["pair_t"], ref["pair_off"], feat, ref["occ_voxel_feat"], prob_p, off_p,
                        part_size=ref["part_size"], fast_roi=True, vox_center=(vb[:, :3] + vb[:, 3:]) / 2.0,
                        pos_rel=True)
        ref.update(out)
        xyz = batch["xyz_corrupt"].permute(0, 2, 3, 1).contiguous().reshape(ref["bs"], -1, 3).clone()
        xyz[ref["miss_bid"], ref["miss_flat_img_id"]] = out["pred_pos"]
        ref["pred_depth"] = xyz[:, :, 2].reshape(ref["bs"], ref["h"], ref["w"])
    return ref


def _against_oracle(dd, ref):
    """Stage 1 of the frame call against the oracle chain: geometry bit for bit, predictions within TOL (2e-5 for
    the PointNet's features), another arg-max only where the two softmax values are within 1e-6."""
    P = ref["pair_ray"].shape[0]
    assert dd["counts"]["P"] == P and dd["counts"]["V"] == ref["voxel_bound"].shape[0]
    for k in ("voxel_bound", "valid_v_rel_coord"):
        assert torch.equal(dd[k].cpu(), ref[k]), k
    for k, kr in (("revidx", "revidx"), ("valid_v_pid", "valid_v_pid"), ("ray_flat", "miss_flat_img_id"),
                  ("ray_bid", "miss_bid"), ("pair_ray", "pair_ray"), ("pair_vox", "pair_vox"),
                  ("pair_off", "pair_off"), ("occ_vox_bid", "occ_vox_bid"),
                  ("occ_vox_global_coord", "occ_vox_global_coord")):
        assert torch.equal(dd[k].cpu().long(), ref[kr]), k
    # (the rays themselves: lidf_device.h forms their length as the reference's torch.norm does, so the slab test
    # sees the oracle's rays and t_enter / t_leave are its values)
    assert torch.equal(dd["miss_ray_dir"].cpu(), ref["miss_ray_dir"])
    assert torch.equal(dd["pair_t"].cpu(), ref["pair_t"])
    err = {"occ_voxel_feat": (dd["occ_voxel_feat"].cpu() - ref["occ_voxel_feat"]).abs().max().item()}
    for k in ("pred_offset", "pred_prob_end", "pair_pred_pos"):
        err[k] = (dd[k].cpu() - ref[k]).abs().max().item()
    print("against the oracle:", {k: "%.3g" % v for k, v in err.items()})
    assert err["occ_voxel_feat"] <= 2e-5, err
    for k in ("pred_offset", "pred_prob_end", "pair_pred_pos"):
        assert err[k] <= TOL, (k, err)
    gid, rid = dd["max_pair_id"].cpu(), ref["max_pair_id"]
    sm = ref["pred_prob_end_softmax"]
    for r in (gid != rid).nonzero().flatten().tolist():   # only float-noise ties may differ
        assert gid[r] < P and rid[r] < P and abs(sm[gid[r]] - sm[rid[r]]) <= 1e-6, r
    same = gid == rid
    assert (dd["pred_depth"].cpu() - ref["pred_depth"]).abs().reshape(-1)[same].mean().item() <= TOL


def _centre_on_a_pixel(batch, h, w):
    """Integer principal point: the ray of pixel (w / 2, h / 2) is (0, 0, 1), two direction components exactly
    zero — it runs along the z axis through the middle column of the long box, through all its 41 cells."""
    batch["cx"] = torch.full_like(batch["cx"], float(w // 2))
    batch["cy"] = torch.full_like(batch["cy"], float(h // 2))


CASES = {
    # name: (grid, (B, h, w), occupied cells, options, captured graph)
    "long_box": ("long_box", (2, 24, 32), grids.every_cell, {}, False),
    "long_box_graph": ("long_box", (2, 24, 32), grids.every_cell, {}, True),
    "res10_sparse": ("res10", (2, 48, 64), None, {}, False),
    "res10_rel_abs": ("res10", (2, 48, 64), None, {"intersect_pos_type": "rel", "refine_pnet_pos_type": "abs"}, False),
    "res16_dense": ("res16", (1, 66, 88), grids.every_cell, {}, False),
    "flat_checkerboard": ("flat", (2, 30, 40), grids.checkerboard, {}, False),
    "offset_checkerboard": ("offset", (2, 30, 40), grids.checkerboard, {}, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_equals_stepwise_equals_oracle(cuda, case):
    """FrameRunner and lidf_forward + refine_forward with LidfOptions(xmin=, xmax=, grid_res=): bit-equal lists and
    predictions (test_frame_gpu.test_frame_equals_stepwise_path's pattern, a second batch through the same runner
    included), and stage 1 against orc.lidf_forward on the same grid.
    long_box: every one of the 3 x 3 x 41 cells occupied and an integer principal point — rays with more than 32
    pairs (asserted from the stepwise pair_off): the branch of lidf_ray_aabb_onepass_kernel that walks the voxel list
    again, which only the frame call reaches; the stepwise path takes the grid walk with two mask words per column.
    res16_dense: 4913 voxels in one frame (66 x 88: the smallest 4:3 image with that many valid pixels) — the scan of
    lidf_frame_cells_kernel takes five rounds, V is far above lds_voxels, some rays exceed 32 pairs.
    flat / offset: per-axis cell counts that differ, cell edges that round, cells occupied in a checkerboard.
    res10: the synthetic batch as it comes (sparse), cell edge 0.2; once with the positions relative to the voxel
    centre in stage 1 and absolute in the stage-2 PointNet.
    res16_dense is the case that found the rays' length one unit in the last place off the reference's (eight rays
    grazing a cell corner: 145,572 pairs against the oracle's 145,568; ray_norm in lidf_device.h)."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    name, (B, h, w), cells, opt_kw, graph = CASES[case]
    grid = grids.BY_NAME[name]
    models = _models(cuda)
    opt = pl.LidfOptions(xmin=grid[1], xmax=grid[2], grid_res=grid[3], **opt_kw)
    runner = pl.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], opt, models[3], models[4])
    assert tuple(runner.res) == grids.widened(*grid[1:])[2]
    batch, feat = synthetic_batch(B, h, w, seed=77)
    V = grids.occupy(batch, cells(grid), grid) if cells else None
    if name == "long_box":
        _centre_on_a_pixel(batch, h, w)
    ora = _oracle_stage1(batch, feat, grid, opt.intersect_pos_type == "rel")
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    with torch.no_grad():
        runner.load(batch, feat)
        if graph:
            runner.capture()
        runner.run()
    ok, dd = runner.result()
    ok_ref, ref = _stepwise(batch, feat, models, opt)
    assert ok and ok_ref
    c = dd["counts"]
    assert (c["R"], c["P"], c["V"]) == (ref["miss_ray_dir"].shape[0], ref["pair_ray"].shape[0],
                                        ref["voxel_bound"].shape[0])
    assert c["NV"] == ref["revidx"].shape[0] and c["NPN"] == c["NV"] + c["R"] and c["OVERFLOW"] == 0
    assert V is None or c["V"] == V
    per_ray = (ref["pair_off"][1:] - ref["pair_off"][:-1]).long()
    print(case, "R %d P %d V %d, pairs per ray max %d mean %.1f, rays with more than 32: %d"
          % (c["R"], c["P"], c["V"], int(per_ray.max()), per_ray.float().mean().item(),
             int((per_ray > grids.AABB_HITS).sum())))
    if name in ("long_box", "res16"):
        assert int((per_ray > grids.AABB_HITS).sum()) >= 1
    if name == "long_box":   # the ray along the z axis crosses every cell of its column
        assert int(per_ray.max()) >= 41
    _compare(dd, ref)
    _against_oracle(dd, ora)
    # a second, different batch through the same runner (and the same graph): nothing stale
    batch2, feat2 = synthetic_batch(B, h, w, seed=78, hole_frac=1.3)
    if cells:
        grids.occupy(batch2, grids.checkerboard(grid, parity=1), grid)    # (other cells than the first batch's)
    batch2, feat2 = _dev(batch2, cuda), feat2.to(cuda)
    with torch.no_grad():
        runner.run(batch2, feat2)
    ok2, dd2 = runner.result()
    ok_ref2, ref2 = _stepwise(batch2, feat2, models, opt)
    assert ok2 and ok_ref2 and dd2["counts"]["P"] != c["P"] and dd2["counts"]["OVERFLOW"] == 0
    assert dd2["counts"]["P"] == ref2["pair_ray"].shape[0] and dd2["counts"]["V"] == ref2["voxel_bound"].shape[0]
    _compare(dd2, ref2)


# ------------------------------------------------------------------------------------------------
# e. the pair list cut at its capacity
# ------------------------------------------------------------------------------------------------
def test_capacity_cut_keeps_the_head_of_the_list(cuda):
    """max_pairs below the need: the lists hold the first max_pairs pairs of the uncut lists, pair_off is the uncut
    one clamped, P == max_pairs and the overflow flag is set — with the cut strictly inside the run of a ray with
    more than 32 pairs (past its 32nd: the walk over the voxel list stops in the middle), and inside the run of a
    ray of a later 256-ray workgroup than the first. max_pairs == P exactly: no flag, the whole lists. Long box,
    every cell occupied, two frames (1536 rays, six workgroups); the buffers are read directly (result() raises on
    overflow)."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    grid = grids.BY_NAME["long_box"]
    B, h, w = 2, 24, 32
    models = _models(cuda)
    opt = pl.LidfOptions(xmin=grid[1], xmax=grid[2], grid_res=grid[3])
    batch, feat = synthetic_batch(B, h, w, seed=77)
    grids.occupy(batch, grids.every_cell(grid), grid)
    _centre_on_a_pixel(batch, h, w)
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    ok_ref, ref = _stepwise(batch, feat, models, opt)
    assert ok_ref
    off = ref["pair_off"].long().cpu()
    cnt = off[1:] - off[:-1]
    R, P = cnt.numel(), int(off[-1])
    long_rays = torch.nonzero(cnt > grids.AABB_HITS).flatten()
    assert long_rays.numel() >= 2
    # (the last of them with room for the cut: the long rays before it lie whole in front of the cut)
    r1 = int(torch.nonzero(cnt >= grids.AABB_HITS + 4).flatten()[-1])
    assert r1 > int(long_rays[0])
    later = torch.nonzero((cnt >= 3) & (cnt <= grids.AABB_HITS) & (torch.arange(R) >= R // 2 + 256)).flatten()
    r2 = int(later[0])
    cuts = (int(off[r1]) + grids.AABB_HITS + 2, int(off[r2]) + 1)
    assert off[r1] + grids.AABB_HITS < cuts[0] < off[r1 + 1] and off[r2] < cuts[1] < off[r2 + 1] and r2 >= 256
    for mp in cuts:
        small = pl.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], opt, models[3], models[4],
                               max_pairs=mp)
        with torch.no_grad():
            small.run(batch, feat)
        c = small.counts()
        assert c["P"] == mp and c["OVERFLOW"] == 1 and c["R"] == R, (mp, c)
        b = small.buf
        assert torch.equal(b["pair_off"][:R + 1].long().cpu(), off.clamp(max=mp)), mp
        for k in ("pair_ray", "pair_vox", "pair_t"):
            assert b[k].shape[0] == mp and torch.equal(b[k], ref[k][:mp].to(b[k].dtype)), (k, mp)
        with pytest.raises(RuntimeError, match="max_pairs"):
            small.result()
    exact = pl.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], opt, models[3], models[4], max_pairs=P)
    with torch.no_grad():
        exact.run(batch, feat)
    ok, dd = exact.result()
    assert ok and dd["counts"]["P"] == P and dd["counts"]["OVERFLOW"] == 0
    _compare(dd, ref)
