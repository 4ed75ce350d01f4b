"""CPU: what tests/test_pointnet_routes_gpu.py rests on. The layouts of tests/pointnet_layouts.py reach the branches
of the PointNet's pooling they are built for (conditions on the inputs, asserted through the census of the kernel's
walk), every (n, V) of the GPU matrix lies on the route it is listed under (read from the exported size function
alone), and the float64 comparison the GPU tests use refuses a pooling that drops or misplaces a point."""
import pytest
import torch

import pointnet_layouts as pl
from util import assert_f64_close, orc


def _case(name, n, V):
    return pl.layout(name, n, V, pl.case_seed(name, n, V))


# ------------------------------------------------------------------------------------------------ layout conditions
def test_layouts_are_seeded_and_in_range():
    for route, name, n, V in pl.matrix():
        vox = _case(name, n, V)
        assert vox.dtype == torch.int64 and tuple(vox.shape) == (n,) and int(vox.max()) < V and int(vox.min()) >= -1
        assert torch.equal(vox, _case(name, n, V))
        kept = vox[vox >= 0]
        assert kept.numel() > 0
        if V > 1:   # every case on more than one voxel has voxels without points
            assert int((torch.bincount(kept, minlength=V) == 0).sum()) > 0, (name, n, V)
    assert int(pl.layout("all_left_out", 300, 289, 0).max()) == -1
    left = _case("left_out", pl.LARGE_N, 3000)
    assert 0.25 < (left < 0).double().mean().item() < 0.35
    heavy = _case("heavy", pl.LARGE_N, 3000)
    rest = heavy[heavy != 2999]
    assert rest.numel() == pl.LARGE_N - int(pl.HEAVY * pl.LARGE_N) and rest.unique().numel() == rest.numel()
    singles = _case("singles", pl.singles_n(3000), 3000)
    assert singles.unique().numel() == singles.numel() < 3000


@pytest.mark.parametrize("V", [v for vs in pl.ROUTE_V.values() for v in vs if v > 1])
def test_runs_meets_every_branch_of_the_wave_reduction(V):
    """One distinct voxel in a 32-point group: one shuffle round; 2 to 4: several rounds; 5 or more: four rounds, then
    the per-lane fallback with members on both sides. At least 5 % of the groups each, and the rounds combine points."""
    for name in ("runs", "left_out"):
        c = pl.wave_classes(_case(name, pl.LARGE_N, V))
        assert c["groups"] >= 100 and min(c["one"], c["few"], c["many"]) >= 0.05, (name, c)
        assert c["shared"] >= 0.9 * c["groups"]
    # what the suite fed route (b) before: every lane its own voxel, no round ever combines two points
    c = pl.wave_classes(torch.randint(0, 16385, (600,), generator=torch.Generator().manual_seed(16385)))
    assert c["many"] == 1.0 and c["shared"] <= 2


@pytest.mark.parametrize("V", [3000, 16384])
def test_singles_spills_most_of_every_tile_on_the_sorted_walk(V):
    n = pl.singles_n(V)
    assert n >= 512
    s = pl.sorted_walk(_case("singles", n, V), V)
    full = s["points"] == pl.TILE
    assert int(full.sum()) >= 4 and bool((s["spill"][full] >= pl.TILE // 2).all()), s["spill"]
    assert bool((s["spill"][full] < pl.TILE).all())          # and the window holds the rest: both sides decide rows
    assert int(s["spilled"].sum()) == int(s["spill"].sum())


def test_many_tiles_case_has_second_tiles_beyond_the_window():
    name, n, V = pl.MANY_TILES
    vox = _case(name, n, V)
    s = pl.sorted_walk(vox, V, pl.SORTED_GRID)
    assert s["points"].shape[0] == 547 and s["multi_tile"] == 547 - pl.SORTED_GRID
    assert s["later_tile_all_spill"] >= 2, s["later_tile_all_spill"]
    # and second tiles that straddle the window's end
    assert int(((s["spill"] > 0) & (s["spill"] < s["points"])).sum()) >= 2


@pytest.mark.parametrize("V", [289, 3000, 16384])
def test_tail_rows_has_windows_that_cross_the_table_end(V):
    vox = _case("tail_rows", pl.LARGE_N, V)
    assert int(vox.min()) >= V - pl.TAIL_ROWS
    s = pl.sorted_walk(vox, V)
    assert s["windows_past_end"] >= 1 and s["windows_past_end"] < s["points"].shape[0]


def test_left_out_shortens_the_sorted_walk():
    vox = _case("left_out", pl.LARGE_N, 3000)
    s = pl.sorted_walk(vox, 3000)
    kept = int((vox >= 0).sum())
    assert int(s["points"].sum()) == kept and s["points"].shape[0] == (kept + pl.TILE - 1) // pl.TILE < pl.LARGE_N // pl.TILE
    assert pl.sorted_walk(pl.layout("all_left_out", 300, 3000, 0), 3000)["points"].shape[0] == 0


def test_census_on_a_hand_made_list():
    """Three workgroups over 5 tiles of sorted points: anchors, spill counts and the table end, counted by hand."""
    vox = torch.cat([torch.full((128,), 0), torch.arange(100, 228),                  # workgroup 0: tiles 0, 1
                     torch.full((100,), 300), torch.full((28,), 331), torch.full((128,), 332),   # workgroup 1: tiles 2, 3
                     torch.full((60,), 990), torch.full((10,), -1)])                 # workgroup 2: tile 4 (60 points)
    s = pl.sorted_walk(vox[torch.randperm(vox.numel(), generator=torch.Generator().manual_seed(1))], 1000, grid=3)
    assert s["points"].tolist() == [128, 128, 128, 128, 60] and s["spill"].tolist() == [0, 128, 0, 128, 0]
    assert (s["multi_tile"], s["later_tile_all_spill"], s["windows_past_end"]) == (2, 2, 1)
    s = pl.sorted_walk(vox, 1000, grid=512)                                          # one tile each: nothing spills but 100..227
    assert s["spill"].tolist() == [0, 96, 0, 0, 0] and s["multi_tile"] == 0
    assert int(s["spilled"].sum()) == 96 and bool(s["spilled"][128 + 32:256].all()) and not bool(s["spilled"][:128 + 32].any())
    w = pl.wave_classes(torch.tensor([3] * 32 + [1, 2] * 16 + list(range(32)) + [-1] * 32 + [0, 0, 1, 2, 3, 4, 5, 5]))
    assert (w["groups"], w["one"], w["few"], w["many"], w["shared"]) == (4, 0.25, 0.25, 0.5, 3)


# ------------------------------------------------------------------------------------------------- route signature
def test_every_gpu_case_lies_on_its_route():
    """lidf_pointnet_workspace_bytes(n, V) alone tells the route: only the voxel-sorted walk has scratch that grows
    with the number of points (its permutation), and the first table beyond LDS brings the copies of the unsorted
    path's table. A changed threshold moves these, and a case of the GPU matrix with them, onto another route."""
    from implicit_depth_amd import _lib
    L = _lib.lib()   # loads without a GPU (no compute call is made here)
    ws = L.lidf_pointnet_workspace_bytes
    shapes = sorted({(n, V) for _, _, n, V in pl.matrix()} | {(n, pad) for _, n, V in pl.CROSS for pad in pl.pads(V)})
    assert len(shapes) >= 30
    for n, V in shapes:
        # twice the points, and at least 64 more: the scratch is sized in 256-byte steps, which one point more does
        # not cross
        more = max(2 * n, n + 64)
        if pl.LDS_MAX_VOX < V <= pl.SORT_MAX_VOX:
            assert pl.route_of(V) == "d" and ws(more, V) > ws(n, V), (n, V)
        else:
            assert pl.route_of(V) in "ab" and ws(more, V) == ws(n, V), (n, V)
    routes = {V: r for r, vs in pl.ROUTE_V.items() for V in vs}
    assert all(pl.route_of(V) == r for V, r in routes.items()) and pl.route_of(pl.MANY_TILES[2]) == "d"
    for n in (1, 257, pl.LARGE_N):
        assert ws(n, 289) - ws(n, 288) >= 289 * 128 * 4          # at least one more [V, 128] table
        assert ws(2 * n + 64, 16385) == ws(n, 16385) and ws(2 * n + 64, 16384) > ws(n, 16384)


# ------------------------------------------------------------------------------- the comparison refuses a wrong pooling
def _refs(p, inp, vox, V):
    keep = vox >= 0
    with torch.no_grad():
        r64 = orc.pointnet2stage({k: v.double() for k, v in p.items()}, inp[keep].double(), vox[keep], V)
        r32 = orc.pointnet2stage(p, inp[keep], vox[keep], V)
    return r64, r32


def _refused(what, got, r64, r32):
    try:
        assert_f64_close(what, got, r64, r32)
    except AssertionError:
        return True
    return False


def test_comparison_refuses_a_wrong_pooling():
    """The float32 oracle on a damaged input stands in for a kernel with that defect; util.assert_f64_close, as the
    GPU tests call it, must refuse each."""
    p = orc.init_pointnet(3, 1.5)
    n, V = 600, 700
    vox = pl.layout("singles", n, V, 11)
    inp = torch.randn(n, 6, generator=torch.Generator().manual_seed(12))
    r64, r32 = _refs(p, inp, vox, V)
    assert not _refused("undamaged", r32, r64, r32)
    # (i) one point dropped
    keep = torch.ones(n, dtype=torch.bool)
    keep[n // 3] = False
    assert _refused("one point dropped", _refs(p, inp[keep], vox[keep], V)[1], r64, r32)
    # (ii) the points beyond the window dropped (a spill that never reaches the global table)
    s = pl.sorted_walk(vox, V)
    assert int(s["spilled"].sum()) >= n // 2
    assert _refused("spill dropped", _refs(p, inp[~s["spilled"]], vox[~s["spilled"]], V)[1], r64, r32)
    # ... and in a layout where most dropped points hide behind their voxel's other points
    vr = pl.layout("runs", 4000, V, 13)
    ir = torch.randn(4000, 6, generator=torch.Generator().manual_seed(14))
    sr = pl.sorted_walk(vr, V, grid=8)
    assert 0 < int(sr["spilled"].sum()) < 4000
    assert _refused("spill dropped (runs)", _refs(p, ir[~sr["spilled"]], vr[~sr["spilled"]], V)[1], *_refs(p, ir, vr, V))
    # (iii) one point pooled into the next voxel
    j = int(torch.nonzero(vox < V - 1)[5])
    moved = vox.clone()
    moved[j] += 1
    assert _refused("pooled into v + 1", _refs(p, inp, moved, V)[1], r64, r32)
    # (iv) an empty voxel's row replaced by its neighbour's
    cnt = torch.bincount(vox, minlength=V)
    e = int(torch.nonzero((cnt[:-1] == 0) & (cnt[1:] > 0))[0])
    bad = r32.clone()
    bad[e] = r32[e + 1]
    assert not torch.equal(bad[e], r32[e])
    assert _refused("empty row <- neighbour", bad, r64, r32)
    # the empty voxel's row itself: vox_lin2 of a zero pool
    assert torch.equal(r32[e], torch.relu(p["vox_lin2.bias"]))
