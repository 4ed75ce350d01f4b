"""Voxel-index layouts for the PointNet inference tests, and a census that replays the pooling walk of
csrc/lidf_pointnet.hip on the CPU (tests only; tests/test_pointnet_layouts.py, tests/test_pointnet_routes_gpu.py).

Which pooling mechanism runs is decided by the number of voxels and by the caller, never by the data; which of
a mechanism's branches decide a result is decided by how the voxel indices lie in the point list. The layouts
below put the indices where those branches sit, and the census says, for one layout instance, how many 32-point
groups, tiles and workgroups meet each branch, so that a test can assert that its input reaches the branch it is
about instead of hoping so."""
import numpy as np
import torch

# The walk's constants, named once (lines of implicit_depth_amd/csrc/lidf_pointnet.hip unless said otherwise)
TILE = 128            # points of a tile: `ntile = (AN + 127) / 128` (:218), `p = tile * 128 + wave * 32 + col` (:241)
WAVE = 32             # points a wavefront pools together: the 32 columns of `wave * 32 + col` (:241, pn_pool's ballot :91)
WINDOW = 32           # rows of the windowed LDS table of the voxel-sorted walk: PN_WINDOW (:416), `vox - vbase < tab_rows` (:263)
ROUNDS = 4            # distinct voxels of a wavefront that pn_pool reduces by shuffles before the per-lane fallback: `rounds < 4` (:93)
LDS_MAX_VOX = 288     # largest table that lives in LDS: PN_LDS_LIMIT = 288 * 129 * 4 (:418), lidf_pointnet_lds_max_voxels (:520)
SORT_MAX_VOX = 16384  # largest table the counting sort takes: lidf_sort_idx_ws_bytes returns 0 beyond it (lidf_train.hip:1590)
SORTED_GRID = 512     # workgroups of the sorted walk: min(tiles, 2 x compute units) (:628), 256 compute units on an MI355X

RUN_LENGTHS = (1, 1, 1, 2, 2, 3, 5, 9, 17, 40, 48, 64)   # `runs`: from single points to two whole wavefronts
TAIL_ROWS = 40        # `tail_rows`: the voxels [V - 40, V)
LEFT_OUT = 0.3        # `left_out`: share of entries set to -1
HEAVY = 0.9           # `heavy`: share of the points in voxel V - 1

LAYOUTS = ("singles", "runs", "heavy", "tail_rows", "left_out", "all_left_out", "uniform")


def route_of(V):
    """The mechanism lidf_pointnet_f32 pools V voxels with: "a" one LDS table per workgroup, "d" the voxel-sorted
    walk over a 32-row window, "b" unsorted global maxima (lidf_api.hip:1141-1171)."""
    return "a" if V <= LDS_MAX_VOX else ("d" if V <= SORT_MAX_VOX else "b")


def _live(V, g):
    """The voxels a layout may draw from: all but an eighth (at least one) of the table, so that every layout on more
    than one voxel leaves voxels without points."""
    if V <= 1:
        return torch.zeros(1, dtype=torch.int64)
    return torch.randperm(V, generator=g)[:V - max(1, V // 8)]


def _runs(n, V, g):
    live = _live(V, g)
    lens = torch.tensor(RUN_LENGTHS)[torch.randint(0, len(RUN_LENGTHS), (n,), generator=g)]   # n runs always suffice
    k = int((torch.cumsum(lens, 0) < n).sum().item()) + 1
    vox = live[torch.randint(0, live.numel(), (k,), generator=g)]
    return torch.repeat_interleave(vox, lens[:k])[:n].contiguous()


def layout(name, n, V, seed):
    """vox int64 [n] in [0, V) (-1: the point is left out of the pooling), seeded.
    singles       n <= V, every point in its own voxel: a random subset of the voxels in random order
    runs          consecutive points share a voxel (the pixels of a depth image do), run lengths from RUN_LENGTHS,
                  voxels drawn at random with repeats
    heavy         about 90 % of the points in voxel V - 1, the others one per voxel elsewhere
    tail_rows     every point in the voxels [V - 40, V)
    left_out      `runs` with 30 % of the entries -1;  all_left_out: every entry -1
    uniform       independent uniform indices"""
    g = torch.Generator().manual_seed(seed)
    if name == "uniform":
        return torch.randint(0, V, (n,), generator=g)
    if name == "singles":
        assert n <= V, (n, V)
        return torch.randperm(V, generator=g)[:n].contiguous()
    if name == "runs":
        return _runs(n, V, g)
    if name == "left_out":
        vox = _runs(n, V, g)
        vox[torch.rand(n, generator=g) < LEFT_OUT] = -1
        return vox
    if name == "all_left_out":
        return torch.full((n,), -1, dtype=torch.int64)
    if name == "heavy":
        vox = torch.full((n,), V - 1, dtype=torch.int64)
        k = min(n - int(HEAVY * n), max(V - 1 - max(1, V // 8), 0))   # (a small table holds fewer single voxels)
        if k > 0:
            vox[torch.randperm(n, generator=g)[:k]] = torch.randperm(V - 1, generator=g)[:k]
        return vox
    if name == "tail_rows":
        lo = max(V - TAIL_ROWS, 0)
        return lo + torch.randint(0, V - lo, (n,), generator=g)
    raise KeyError(name)


def wave_classes(vox):
    """The unsorted walk (route b; input order): shares of the 32-point groups that hold kept points with 1, with 2 to
    ROUNDS and with more than ROUNDS distinct voxels — one shuffle round, several, and rounds plus the per-lane
    fallback of pn_pool — and the number of groups in which a round combines two or more points ("shared")."""
    v = vox.numpy()
    one = few = many = shared = groups = 0
    for s in range(0, v.shape[0], WAVE):
        w = v[s:s + WAVE]
        w = w[w >= 0]
        if w.size == 0:
            continue
        groups += 1
        _, first, cnt = np.unique(w, return_index=True, return_counts=True)
        d = cnt.size
        one += d == 1
        few += 1 < d <= ROUNDS
        many += d > ROUNDS
        in_rounds = cnt[np.argsort(first)][:ROUNDS]          # pn_pool takes the voxels in the order of their first lanes
        shared += bool((in_rounds > 1).any())
    t = max(groups, 1)
    return {"groups": groups, "one": one / t, "few": few / t, "many": many / t, "shared": shared}


def sorted_walk(vox, V, grid=SORTED_GRID):
    """The voxel-sorted walk (routes d and e2) of `grid` workgroups at most over the kept points in ascending voxel
    order: workgroup b walks the tiles [tb, te) (:218-222) with a WINDOW-row table anchored at the voxel of its first
    point (:235); a point WINDOW or more rows past the anchor goes to the global table per lane.
    spill          int [tiles]: such points of every tile;  points: int [tiles] kept points of the tile
    spilled        bool [n]: the same per input point
    multi_tile     workgroups that walk more than one tile
    later_tile_all_spill   workgroups one of whose tiles after the first spills entirely
    windows_past_end       workgroups whose window reaches beyond row V - 1 (`row < a.V` in the flush, :358)"""
    v = vox.numpy()
    kept = np.flatnonzero(v >= 0)
    order = kept[np.argsort(v[kept], kind="stable")]
    sv = v[order]
    an = sv.shape[0]
    ntile = (an + TILE - 1) // TILE
    g = min(grid, (v.shape[0] + TILE - 1) // TILE)              # the launch is sized by the capacity, not by *n_perm
    spill = np.zeros(ntile, dtype=np.int64)
    points = np.zeros(ntile, dtype=np.int64)
    spilled = np.zeros(v.shape[0], dtype=bool)
    multi = later_all = past_end = 0
    per, rem = (ntile // g, ntile % g) if g else (0, 0)
    for b in range(g):
        tb = b * per + min(b, rem)
        te = tb + per + (1 if b < rem else 0)
        if tb >= te or tb * TILE >= an:
            continue
        anchor = sv[tb * TILE]
        multi += te - tb > 1
        past_end += anchor + WINDOW > V
        for t in range(tb, te):
            seg = slice(t * TILE, min((t + 1) * TILE, an))
            out = sv[seg] - anchor >= WINDOW
            spill[t], points[t] = out.sum(), out.size
            spilled[order[seg][out]] = True
        later_all += bool((spill[tb + 1:te] == points[tb + 1:te]).any())
    return {"spill": spill, "points": points, "spilled": torch.from_numpy(spilled), "multi_tile": int(multi),
            "later_tile_all_spill": int(later_all), "windows_past_end": int(past_end)}


# ---------------------------------------------------------------------------------------------------------------
# The cases of tests/test_pointnet_routes_gpu.py: (layout, n, V). Listed here so that the CPU tests hold every one
# of them to its route (tests/test_pointnet_layouts.py) without importing a GPU module.
# ---------------------------------------------------------------------------------------------------------------
ROUTE_V = {"a": (1, 40, 288), "d": (289, 3000, 16384), "b": (16385, 20000)}
SMALL_N = (1, 31, 33, 127, 128, 129, 257)      # around one wavefront, one tile, two tiles
LARGE_N = 4000                                  # 32 tiles: every workgroup of the sorted walk one tile
MANY_TILES = ("uniform", 70000, 16000)          # 547 tiles on 512 workgroups: 35 of them walk two


def singles_n(V):
    return min(V - max(1, V // 8), 3000)


def matrix():
    """[(route, layout, n, V)]: every table size of every route at every small row count with `runs`, and at LARGE_N
    (`singles`: singles_n) with every layout that fits the table and leaves voxels without points."""
    out = []
    for route, vs in ROUTE_V.items():
        for V in vs:
            assert route_of(V) == route
            out += [(route, "runs", n, V) for n in SMALL_N]
            if V == 1:
                out.append((route, "uniform", LARGE_N, V))
                continue
            out.append((route, "singles", singles_n(V), V))
            out += [(route, name, LARGE_N, V) for name in ("runs", "heavy", "left_out")]
            if V >= 3000:                          # (uniform indices leave voxels empty only on a table this sparse)
                out.append((route, "uniform", LARGE_N, V))
            if V > TAIL_ROWS:
                out.append((route, "tail_rows", LARGE_N, V))
    out.append(("d",) + MANY_TILES)
    return out


# One input under table sizes on both sides of each threshold: (layout, n, V used by the layout); n_vox = pads(V)
CROSS = [("singles", 180, 200), ("runs", LARGE_N, 200), ("heavy", LARGE_N, 200), ("tail_rows", LARGE_N, 200),
         ("left_out", LARGE_N, 200), ("uniform", LARGE_N, 200),
         ("singles", 2500, 3000), ("runs", LARGE_N, 3000), ("heavy", LARGE_N, 3000), ("tail_rows", LARGE_N, 3000),
         ("left_out", LARGE_N, 3000), ("uniform", LARGE_N, 3000)]


def pads(V):
    """Table sizes a cross-route input of V used voxels runs under: the last of route (a) and the first of (d) where
    it fits, the last of (d) and the first of (b)."""
    return tuple(p for p in (LDS_MAX_VOX, LDS_MAX_VOX + 1, SORT_MAX_VOX, SORT_MAX_VOX + 1) if p >= V)


def case_seed(name, n, V):
    return 1000003 * LAYOUTS.index(name) + 7919 * n + V
