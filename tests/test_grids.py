"""CPU: what tests/test_grids_gpu.py rests on, checked with the oracle alone — each grid of tests/grids.py reaches
the branch it is there for (a change of a fixture must not quietly leave a branch unreached), and the oracle's
new grid arguments leave the default grid's results as they were."""
import numpy as np
import pytest
import torch

import grids
from util import orc


def test_grid_table_matches_its_comments():
    dims = {g[0]: grids.widened(*g[1:])[2] for g in grids.ALL}
    assert dims == {"default": (9, 9, 9), "res10": (11, 11, 11), "res12": (13, 13, 13), "res16": (17, 17, 17),
                    "long_box": (3, 3, 41), "flat": (13, 7, 13), "offset": (8, 11, 10), "res20": (21, 21, 21)}
    # per-axis counts that differ, in two ways (x == z != y; all three different)
    assert len(set(dims["flat"])) == 2 and len(set(dims["offset"])) == 3 and len(set(dims["long_box"])) == 2


def test_widened_is_the_oracles_grid():
    """grids.widened against orc.occupied_voxels: the widened corner and the cell edge, bit for bit; the cell
    counts by the cells the oracle accepts (a point in the last cell of every axis is in, one cell further out)."""
    for g in grids.ALL:
        lo, part, dims = grids.widened(*g[1:])
        n = dims[0] * dims[1] * dims[2]
        last = torch.tensor([n - 1])
        pts = torch.cat((grids.cell_centres(last, g), grids.cell_centres(last, g) + part))
        occ = orc.occupied_voxels(pts, torch.zeros(2, dtype=torch.long), *g[1:])
        assert occ["part_size"] == part and torch.equal(occ["xmin"], lo), g[0]
        assert occ["valid_v_pid"].tolist() == [0], g[0]
        assert occ["occ_vox_global_coord"].tolist() == [[dims[0] - 1, dims[1] - 1, dims[2] - 1]], g[0]


def test_long_box_has_a_camera_ray_with_more_hits_than_the_lds_list():
    """lidf_ray_aabb_onepass_kernel keeps AABB_HITS = 32 hits per ray in LDS; a ray with more walks the voxel
    list again. The fully occupied long box reaches that branch with the pixel rays of the 24 x 32 image."""
    n = grids.hits_per_ray(grids.BY_NAME["long_box"], grids.camera_rays())
    assert int(n.max()) > grids.AABB_HITS and int((n > grids.AABB_HITS).sum()) >= 1
    # res16 at full occupancy reaches it too; the default grid never does
    h, w = grids.smallest_image(grids.cells_of(grids.BY_NAME["res16"]), seed=77)
    assert int(grids.hits_per_ray(grids.BY_NAME["res16"], grids.camera_rays(h, w)).max()) > grids.AABB_HITS
    assert int(grids.hits_per_ray(grids.BY_NAME["default"], grids.camera_rays()).max()) <= grids.AABB_HITS


def test_long_box_needs_two_mask_words_per_column():
    assert grids.widened(*grids.BY_NAME["long_box"][1:])[2][2] > 32      # mw = (rz + 31) / 32 = 2
    assert all(grids.widened(*g[1:])[2][2] <= 32 for g in grids.ALL if g[0] != "long_box")


def test_large_grid_exceeds_the_grid_walks_lds_table():
    assert grids.cells_of(grids.LARGE) > grids.GRID_LDS_CELLS
    assert all(grids.cells_of(g) <= grids.GRID_LDS_CELLS for g in grids.GRIDS)


def test_inexact_grids_have_a_cell_edge_that_rounds():
    for g in grids.ALL:
        part = grids.widened(*g[1:])[1]
        exact = float(np.float32(part)) == part
        assert exact == (g[0] not in grids.INEXACT), (g[0], part)
    # ... and the voxel arithmetic does round there: some lower bound lo + c * part is no exact f32 product
    for name in grids.INEXACT:
        lo, part, dims = grids.widened(*grids.BY_NAME[name][1:])
        c = torch.arange(max(dims), dtype=torch.float64)
        assert bool(((lo[0].double() + c * float(np.float32(part))).float().double()
                     != lo[0].double() + c * float(np.float32(part))).any()), name


def test_occupy_fills_the_chosen_cells():
    from implicit_depth_amd.synthetic import synthetic_batch
    for name, cells in (("long_box", grids.every_cell), ("flat", grids.checkerboard), ("offset", grids.checkerboard)):
        g = grids.BY_NAME[name]
        batch, _ = synthetic_batch(2, 30, 40, seed=77)
        want = cells(g)
        V = grids.occupy(batch, want, g)
        xyz = batch["xyz_corrupt"].permute(0, 2, 3, 1).reshape(2, -1, 3)
        valid = (batch["depth_corrupt"] != 0).reshape(2, -1)
        idx = torch.nonzero(valid)
        occ = orc.occupied_voxels(xyz[idx[:, 0], idx[:, 1]], idx[:, 0], *g[1:])
        dims = grids.widened(*g[1:])[2]
        assert occ["voxel_bound"].shape[0] == V == 2 * want.numel()
        assert torch.equal(occ["occ_vox_global_coord"][: want.numel()], grids.cell_coords(want, dims))
        assert occ["valid_v_pid"].numel() == idx.shape[0]                 # every valid point inside the grid


def test_occupy_on_the_default_grid_is_test_frame_gpus():
    """The generalised helper gives the 9^3 tests the inputs they always had."""
    from implicit_depth_amd.synthetic import synthetic_batch
    batch, _ = synthetic_batch(2, 25, 33, seed=77)
    old = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
    cells = torch.arange(729)
    V = grids.occupy(batch, cells, grids.BY_NAME["default"])
    B, _, h, w = old["xyz_corrupt"].shape
    valid = (old["depth_corrupt"] != 0).reshape(B, h * w)
    cell = cells[(torch.cumsum(valid.long(), 1) - 1) % 729]
    c = torch.stack((cell // 81, (cell // 9) % 9, cell % 9), 1).float()
    pts = torch.tensor([-1.125, -1.125, -0.125]).reshape(1, 3, 1) + (c + 0.5) * 0.25
    assert V == 2 * 729
    assert torch.equal(batch["xyz_corrupt"], (pts * valid.unsqueeze(1).float()).reshape(B, 3, h, w))


def test_oracle_default_grid_arguments_change_nothing():
    """orc.lidf_forward on the batch of the g9 fixture (the reference's own training step on the default grid,
    every valid pixel kept): the voxel bounds are the reference's, with the grid arguments left out and with the
    default values spelled out; another grid gives another list."""
    import train_loss_ref as tl
    g, _ = tl.g9_files()
    batch, feat = tl.g9_batch(g)
    from implicit_depth_amd.synthetic import init_decoder_params
    pnet_p = orc.init_pointnet(3, 1.5)
    prob_p, off_p = init_decoder_params("IMNET", 385, 7, 5.0), init_decoder_params("IEF", 385, 8, 5.0)
    ok, a = orc.lidf_forward(batch, feat, pnet_p, prob_p, off_p)
    ok2, b = orc.lidf_forward(batch, feat, pnet_p, prob_p, off_p, xmin=(-1.0, -1.0, 0.0), xmax=(1.0, 1.0, 2.0),
                              grid_res=8)
    assert ok and ok2
    want = torch.from_numpy(g["e0_voxel_bound"])
    assert torch.equal(a["voxel_bound"], want) and torch.equal(b["voxel_bound"], want)
    assert a["part_size"] == 0.25
    for k in ("revidx", "valid_v_rel_coord", "pair_ray", "pair_vox", "pair_t", "occ_voxel_feat", "pred_offset",
              "pred_prob_end", "pair_pred_pos", "max_pair_id", "pred_depth"):
        assert torch.equal(a[k], b[k]), k
    ok3, c = orc.lidf_forward(batch, feat, pnet_p, prob_p, off_p, grid_res=10)
    assert c["part_size"] == 0.2 and c["voxel_bound"].shape != want.shape
