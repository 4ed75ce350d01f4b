"""PointNet2Stage inference (lidf_pointnet_f32, and its device-count twin inside the frame call) on every pooling
route and voxel layout, against the float64 oracle.

The pooled maxima reach the voxel table through five mechanisms, chosen by the number of voxels and by the caller:
(a) one LDS table per workgroup (V <= 288), (d) the voxel-sorted walk over a 32-row LDS window (V <= 16384),
(b) unsorted global maxima with a per-wave shuffle reduction (beyond), and in the frame call (e1) the LDS table for
the first `lds_voxels` voxels with per-lane maxima for the others, (e2) the grouped walk over the window. The
layouts of tests/pointnet_layouts.py put the voxel indices where each mechanism's branches sit;
tests/test_pointnet_layouts.py asserts, without a GPU, that they do and that every (n, V) here lies on its route.

Criterion of the matrix: util.assert_f64_close, no worse than 4 x the float32 oracle's own error against float64.
Largest ratios measured on an MI355X (elementwise / normwise), per route over its cases:
    (a) LDS table      1.55 / 1.22   (31 cases)
    (d) sorted walk    1.68 / 1.21   (39 cases)
    (b) unsorted       1.54 / 1.02   (26 cases)
The remaining tests are exact: rows of voxels without points, one input under table sizes on both sides of each
threshold, the frame call against the stepwise path.
"""
import pytest
import torch

import pointnet_layouts as pl
from test_frame_gpu import DENSE_SHAPE, _compare, _dev as _batch_dev, _models, _occupy_all, _stepwise
from util import assert_f64_close, make_pointnet, orc

pytestmark = pytest.mark.gpu

PARAMS = orc.init_pointnet(3, 1.5)
REPORT = {}


def _dev(p, dev, dt):
    return {k: v.to(dev, dt) for k, v in p.items()}


def _inputs(name, n, V, cuda):
    seed = pl.case_seed(name, n, V)
    vox = pl.layout(name, n, V, seed)
    inp = torch.randn(n, 6, generator=torch.Generator().manual_seed(seed + 1))
    return inp.to(cuda), vox.to(cuda)


_MODEL = []


def _run(inp, vox, n_vox, cuda):
    if not _MODEL:
        _MODEL.append(make_pointnet(PARAMS, cuda))   # eval mode, as test_f64_gpu.py::test_pointnet_forward builds it
    with torch.no_grad():
        return _MODEL[0](inp, vox, n_vox)


def _empty_row(cuda):
    """A voxel without points: pool 0 -> vox_lin2(0) -> relu(vox_lin2.bias)."""
    return torch.relu(PARAMS["vox_lin2.bias"]).to(cuda)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_rows_are_empty(got, rows, cuda):
    """Exactly relu(vox_lin2.bias), no tolerance. The one freedom is the sign of a zero: the per-voxel kernel's ReLU
    is fmaxf(x, 0 * x) (lidf_linear.hip:96, :142; it passes a NaN on), which writes -0 for a negative bias where
    torch writes +0. torch.equal takes the two for equal; all such rows must be the same bits as each other."""
    assert rows.numel() > 0
    g = got[rows]
    assert torch.equal(g, _empty_row(cuda).expand(rows.numel(), -1)), "a voxel without points is not relu(bias)"
    assert torch.equal(_bits(g), _bits(g[:1]).expand(rows.numel(), -1)), "rows of voxels without points differ"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for route in sorted(REPORT):
        rows = REPORT[route]
        print("route (%s): %d cases, largest ratio %.2f elementwise / %.2f normwise"
              % (route, len(rows), max(r["ratio_max"] for r in rows), max(r["ratio_nrm"] for r in rows)))


# ------------------------------------------------------------------------------------------------- float64 matrix
@pytest.mark.parametrize("route,name,n,V", pl.matrix(), ids=lambda v: str(v))
def test_pointnet_route_against_float64(cuda, route, name, n, V):
    inp, vox = _inputs(name, n, V, cuda)
    keep = vox >= 0
    got = _run(inp, vox, V, cuda)
    with torch.no_grad():   # left-out points: the reference sees the kept rows only
        r64 = orc.pointnet2stage(_dev(PARAMS, cuda, torch.float64), inp[keep].double(), vox[keep], V)
        r32 = orc.pointnet2stage(_dev(PARAMS, cuda, torch.float32), inp[keep], vox[keep], V)
    rows = REPORT.setdefault(route, [])
    assert_f64_close("pointnet (%s) %s n=%d V=%d" % (route, name, n, V), got, r64, r32, report=rows)
    if V > 1:
        empty = torch.nonzero(torch.bincount(vox[keep], minlength=V) == 0).flatten()
        _assert_rows_are_empty(got, empty, cuda)


# ------------------------------------------------------------------------------------------------------ exact rows
@pytest.mark.parametrize("V", [40, 288, 289, 16384, 16385])
@pytest.mark.parametrize("n", [1, 129, 4000])
def test_all_points_left_out_gives_the_empty_row_everywhere(cuda, n, V):
    """Every index negative: route (a) flushes an untouched table, (d) walks a permutation of length 0, (b) finds no
    lane to pool. Every voxel's row is relu(vox_lin2.bias), exactly (_assert_rows_are_empty)."""
    inp = torch.randn(n, 6, generator=torch.Generator().manual_seed(n + V)).to(cuda)
    vox = pl.layout("all_left_out", n, V, 0).to(cuda)
    got = _run(inp, vox, V, cuda)
    assert tuple(got.shape) == (V, 128)
    _assert_rows_are_empty(got, torch.arange(V, device=cuda), cuda)


# -------------------------------------------------------------------------------------- the same input on every route
@pytest.mark.parametrize("name,n,V", pl.CROSS, ids=lambda v: str(v))
def test_routes_agree_bit_for_bit(cuda, name, n, V):
    """One (inp, vox) under table sizes on both sides of each threshold. A point's chain reads its own column alone,
    wherever the point stands in a tile, and the pooling is an integer maximum of positive float bits: the rows of
    the used voxels are the same bits on every route, the padding rows are the empty row."""
    inp, vox = _inputs(name, n, V, cuda)
    pads = pl.pads(V)
    assert len(pads) == (4 if V <= pl.LDS_MAX_VOX else 2) and len({pl.route_of(p) for p in pads}) >= 2
    outs = [_run(inp, vox, pad, cuda) for pad in pads]
    for pad, out in zip(pads, outs):
        assert tuple(out.shape) == (pad, 128)
        diff = torch.nonzero((_bits(out[:V]) != _bits(outs[0][:V])).any(1)).flatten()
        assert diff.numel() == 0, "n_vox %d (route %s) differs from n_vox %d (route %s) in rows %s" % (
            pad, pl.route_of(pad), pads[0], pl.route_of(pads[0]), diff[:8].tolist())
        if pad > V:
            _assert_rows_are_empty(out, torch.arange(V, pad, device=cuda), cuda)


# -------------------------------------------------------------------------------------------------- frame routes
FRAMES = {"one frame": (1, 48, 64), "two frames": (2, 48, 64), "dense": DENSE_SHAPE}


@pytest.mark.parametrize("k", [1, 8, 32, 33])
@pytest.mark.parametrize("case", list(FRAMES))
def test_frame_overflow_routes_equal_the_stepwise_path(cuda, case, k):
    """FrameRunner(lds_voxels=k) with more occupied voxels than k: one frame pools the first k voxels through the
    workgroup's table and the others per lane (e1), a batch walks its points grouped by voxel over the 32-row window
    (e2; "dense": every cell occupied, about one point per voxel). Both PointNets (the refine one with its tail
    layer) take that route; everything from occ_voxel_feat to pred_pos_refine is bit-equal to the stepwise path."""
    from implicit_depth_amd import pipeline
    from implicit_depth_amd.synthetic import synthetic_batch
    shape = FRAMES[case]
    B, h, w = shape[:3]
    models = _models(cuda)
    opt = pipeline.LidfOptions(valid_stride=None, refine_use_all_pix=case != "two frames")
    batch, feat = synthetic_batch(B, h, w, seed=77)
    V = _occupy_all(batch) if case == "dense" else None
    batch, feat = _batch_dev(batch, cuda), feat.to(cuda)
    runner = pipeline.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], opt, models[3], models[4],
                                  lds_voxels=k)
    assert runner.lds_voxels == k
    with torch.no_grad():
        runner.run(batch, feat)
    ok, dd = runner.result()
    ok_ref, ref = _stepwise(batch, feat, models, opt)
    assert ok and ok_ref
    c = dd["counts"]
    assert c["V"] > k and c["V"] == ref["voxel_bound"].shape[0] and c["OVERFLOW"] == 0
    assert V is None or c["V"] == V
    _compare(dd, ref)
