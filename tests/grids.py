"""Voxel grids other than the shipped 9 x 9 x 9 one, shared by tests/test_grids.py (CPU: the preconditions) and
tests/test_grids_gpu.py (the kernels against the oracle on them). A plain module: tables and input builders only.

A grid is (name, xmin, xmax, grid_res) as LidfOptions / get_occ_vox_bound / orc.occupied_voxels take it; the
cells per axis and the cell edge follow from LIDF.get_occ_vox_bound's widening (models/pipeline.py:167-173)."""
import torch

from util import orc

DEFAULT_BOX = ((-1.0, -1.0, 0.0), (1.0, 1.0, 2.0))   # utils/constants.py:15-16

# name, xmin, xmax, grid_res                                             cells per axis   cell edge
GRIDS = (
    ("default", DEFAULT_BOX[0], DEFAULT_BOX[1], 8),                     # 9, 9, 9         0.25 (exact)
    ("res10", DEFAULT_BOX[0], DEFAULT_BOX[1], 10),                      # 11, 11, 11      0.2
    ("res12", DEFAULT_BOX[0], DEFAULT_BOX[1], 12),                      # 13, 13, 13      1/6
    ("res16", DEFAULT_BOX[0], DEFAULT_BOX[1], 16),                      # 17, 17, 17      0.125 (exact)
    ("long_box", (-0.25, -0.25, 0.0), (0.25, 0.25, 10.0), 2),           # 3, 3, 41        0.25 (exact)
    ("flat", (-1.0, -0.5, 0.0), (1.0, 0.5, 2.0), 6),                    # 13, 7, 13       1/6
    ("offset", (-0.7, -0.9, 0.1), (0.6, 0.8, 1.7), 7),                  # 8, 11, 10       ~0.2286
)
# one cubic grid whose cell table does not fit the grid walk's LDS (GRID_LDS_CELLS = 8192 in lidf_aux.hip)
LARGE = ("res20", DEFAULT_BOX[0], DEFAULT_BOX[1], 20)                   # 21, 21, 21      0.1
ALL = GRIDS + (LARGE,)
BY_NAME = {g[0]: g for g in ALL}
# grids whose cell edge is no binary fraction: v / crop, c * crop + crop / 2 and xmin + c * crop round
INEXACT = ("res10", "res12", "flat", "offset", "res20")

GRID_LDS_CELLS = 8192   # lidf_aux.hip
AABB_HITS = 32          # lidf_aux.hip: hits per ray that lidf_ray_aabb_onepass_kernel keeps in LDS
CAMERA = (24, 32)       # the image whose pixel rays the long box is crossed by (768 rays)


def widened(xmin, xmax, res):
    """(lo [3] f32, part_size (a Python float), cells per axis) of the widened grid, with the operations of
    query.get_occ_vox_bound and orc.occupied_voxels: f32 corners, the cell edge formed in double."""
    lo = torch.tensor(xmin, dtype=torch.float32)
    hi = torch.tensor(xmax, dtype=torch.float32)
    part_size = torch.min(hi - lo).item() / res
    lo = lo - 0.5 * part_size
    hi = hi + 0.5 * part_size
    dims = tuple(int(v) for v in torch.ceil((hi - lo) / part_size).tolist())
    return lo, part_size, dims


def cells_of(grid):
    lo, part, dims = widened(*grid[1:])
    return dims[0] * dims[1] * dims[2]


def cell_coords(cells, dims):
    """[n, 3] integer cell of every key ((x * ry) + y) * rz + z."""
    return torch.stack((cells // (dims[1] * dims[2]), (cells // dims[2]) % dims[1], cells % dims[2]), -1)


def cell_centres(cells, grid):
    """[n, 3] f32 centres of the cells `cells` (keys into one image's grid): half a cell from every face, so the
    point lies in its cell whichever way the voxel arithmetic rounds."""
    lo, part, dims = widened(*grid[1:])
    return lo + (cell_coords(cells, dims).float() + 0.5) * part


def occupy(batch, cells, grid):
    """Moves the valid points of a synthetic batch so that the cells `cells` (keys into one image's grid) of every
    image are occupied: the j-th valid pixel of an image lies at the centre of chosen cell j % len(cells). Returns
    the number of voxels."""
    B, _, h, w = batch["xyz_corrupt"].shape
    valid = (batch["depth_corrupt"] != 0).reshape(B, h * w)
    assert int(valid.sum(1).min()) >= cells.numel()
    cell = cells[(torch.cumsum(valid.long(), 1) - 1) % cells.numel()]              # [B, h w]
    pts = cell_centres(cell, grid).permute(0, 2, 1)                                # [B, 3, h w]
    batch["xyz_corrupt"] = (pts * valid.unsqueeze(1).float()).reshape(B, 3, h, w).contiguous()
    return B * cells.numel()


def every_cell(grid):
    return torch.arange(cells_of(grid))


def checkerboard(grid, parity=0):
    """Every second cell (coordinate sum even, or odd with parity=1)."""
    lo, part, dims = widened(*grid[1:])
    k = torch.arange(dims[0] * dims[1] * dims[2])
    return k[cell_coords(k, dims).sum(1) % 2 == parity]


def smallest_image(n_valid, seed, B=1, hole_frac=1.0):
    """The smallest 4:3 image (3k x 4k) of synthetic_batch(B, ., ., seed) with at least n_valid valid pixels in
    every frame."""
    from implicit_depth_amd.synthetic import synthetic_batch
    k = 1
    while True:
        if 12 * k * k >= n_valid:
            batch, _ = synthetic_batch(B, 3 * k, 4 * k, seed=seed, hole_frac=hole_frac)
            if int((batch["depth_corrupt"] != 0).reshape(B, -1).sum(1).min()) >= n_valid:
                return 3 * k, 4 * k
        k += 1


def special_rays(R, gen):
    """[R, 3] unit directions of test_boxes_gpu.grid_scene's kind: random ones, the axes (zero components: the
    d + 1e-12 path), in a cell-boundary plane, through cell corners, pointing away from the grid, a line and its
    reverse."""
    d = torch.randn(R, 3, generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    if R >= 8:
        d[0], d[1], d[2] = torch.tensor([0.0, 0, 1]), torch.tensor([1.0, 0, 0]), torch.tensor([0.0, -1, 0])
        d[3] = torch.tensor([0.0, 0.6, 0.8])
        d[4] = torch.tensor([-0.125, -0.125, 0.125]) / 0.2165063509
        d[5] = torch.tensor([0.6, 0.0, -0.8])
        d[6] = -d[7]
    return d.contiguous()


def camera_rays(h=CAMERA[0], w=CAMERA[1]):
    """[h w, 3] pixel rays of synthetic.pixel_rays (fx = fy = 0.9 w, principal point between the pixels)."""
    from implicit_depth_amd.synthetic import pixel_rays
    return pixel_rays(1, h, w)[0]


def grid_scene(grid, B, fill, seed, n_special=201, ray_order="frames"):
    """test_boxes_gpu.grid_scene on any grid: occupied cells (each with probability `fill`) of B frames as the
    oracle's voxel list — sorted by (frame, x, y, z), bounds from orc.occupied_voxels on the cells' centres — and
    rays through, beside and along the grid: the camera rays of CAMERA followed by special_rays. ray_order
    'frames': frame-major ray_bid (every frame gets a contiguous run of the rays); 'shuffled': random frames.
    Returns (ray_dir [R,3], ray_bid [R] i32, occ: the oracle's dict, points [V,3], point frames [V])."""
    g = torch.Generator().manual_seed(seed)
    n = cells_of(grid)
    key = torch.nonzero(torch.rand(B * n, generator=g) < fill).squeeze(1)
    if key.numel() == 0:
        key = torch.tensor([n // 2])
    bid = key // n
    pts = cell_centres(key % n, grid)
    occ = orc.occupied_voxels(pts, bid, *grid[1:])
    assert occ["voxel_bound"].shape[0] == key.numel() and (occ["revidx"] == torch.arange(key.numel())).all()
    d = torch.cat((camera_rays(), special_rays(n_special, g)), 0).contiguous()
    R = d.shape[0]
    if ray_order == "frames":
        rb = (torch.arange(R) * B) // R
    else:
        rb = torch.randint(0, B, (R,), generator=g)
    return d, rb.int().contiguous(), occ, pts, bid


def hits_per_ray(grid, d):
    """[R] number of cells of the fully occupied grid each direction of d crosses (one frame), from the oracle."""
    n = cells_of(grid)
    occ = orc.occupied_voxels(cell_centres(torch.arange(n), grid), torch.zeros(n, dtype=torch.long), *grid[1:])
    mask, _ = orc.ray_aabb(d.numpy(), occ["voxel_bound"].numpy(), torch.zeros(d.shape[0]).numpy(),
                           occ["occ_vox_bid"].numpy())
    return torch.from_numpy(mask).sum(0)


def voxel_points(grid, B, n, seed, stored=None):
    """About n points for the voxel build on `grid`: uniform ones reaching outside the grid; points exactly on
    computed cell faces (lo + k * part_size in f32 for k from -1 to dims + 1, the three coordinates drawn
    independently); the torch.nextafter neighbours of those on both sides (whole points, and each coordinate on a
    side of its own); `stored` — voxel_bound [V,6] of a first pass — as points (lower corners, upper corners, mixed);
    one far point. Returns (xyz [N,3] f32, bid [N] int64)."""
    g = torch.Generator().manual_seed(seed)
    lo, part, dims = widened(*grid[1:])
    ext = torch.tensor(dims, dtype=torch.float32) * part
    k = n // 5
    uni = lo - 0.15 * ext + torch.rand(2 * k, 3, generator=g) * (1.3 * ext)
    face = torch.empty(k, 3)
    for a in range(3):
        ks = torch.randint(-1, dims[a] + 2, (k,), generator=g).float()
        face[:, a] = lo[a] + ks * part             # f32: the oracle's (and the kernels') bound_min expression
    inf = torch.tensor(float("inf"))
    up, down = torch.nextafter(face, inf), torch.nextafter(face, -inf)
    side = torch.randint(0, 3, (k, 3), generator=g)
    mixed = torch.where(side == 0, down, torch.where(side == 1, face, up))
    parts = [uni, face, up[: k // 2], down[: k // 2], mixed]
    if stored is not None and stored.shape[0] > 0:
        s = stored.cpu()
        pick = torch.randint(0, 2, (s.shape[0], 3), generator=g)
        parts += [s[:, :3], s[:, 3:], torch.where(pick == 0, s[:, :3], s[:, 3:])]
    parts.append(torch.tensor([[1e6, -3e5, 2e7]]))
    xyz = torch.cat(parts, 0).contiguous()
    bid = torch.randint(0, B, (xyz.shape[0],), generator=g)
    return xyz, bid
