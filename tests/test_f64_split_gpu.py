"""precision="f16x3" against float64 (lidf_rows_h.hip, lidf_points_h.hip): the float64 yardstick of tests/test_f64_gpu.py
with the split path's unit. The float32 oracle's error alone is no unit for these kernels — the scheme has a
representation error of its own — so split_f16_ref.assert_split_close takes the error of a twin of the f16 pieces
(tests/split_f16_ref.py, float64 products and sums) plus the float32 oracle's, both against the float64 oracle on the
same inputs, and concedes the kernel F64_K = 4 times that, elementwise and normwise. tests/test_split_f16_ref.py
shows on the CPU that one lost, stale or flushed low piece is rejected by it.

References and twin are evaluated on the GPU with torch's own ops (TF32 off). Forward only: no kink masks, no element
is left out of any comparison. Decoder outputs are compared as logits (util.inv_out_act). The product's own arg-max is
fed to the references and checked on its own (util.check_selection)."""
import functools
import gc

import pytest
import torch

import pointnet_ref as ref
import split_f16_ref as sp
from util import (check_selection, decoder_preacts, inv_out_act, make_module, make_pointnet, orc, tf32_off,
                  to_dev)

pytestmark = pytest.mark.gpu

REPORT = {"decoders": [], "query": [], "range edge": [], "stage 2": []}


@pytest.fixture(autouse=True)
def _full_precision_references():
    with tf32_off():
        yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _print_report():
    yield
    for group, rows in REPORT.items():
        if rows:
            worst = max(rows, key=lambda r: r["ratio_max"])
            print("\nf16x3 vs float64, %s: %d tensors, worst ratio elementwise %.2f (%s) / normwise %.2f"
                  % (group, len(rows), worst["ratio_max"], worst["what"], max(r["ratio_nrm"] for r in rows)))


def _dev(p, dev, dt):
    return {k: v.to(dev, dt) for k, v in p.items()}


def _logits(v, sig):
    return v.double() if sig else inv_out_act(v)


# ---------------------------------------------------------------------------------------------------------------
# the decoder boundary (lidf_rows_h.hip)
# ---------------------------------------------------------------------------------------------------------------
N_ROWS = 1000


@functools.lru_cache(maxsize=None)
def _decoder_case(kind, d, scale):
    p = orc.randomize_biases(orc.init_decoder(kind, d, 81, scale), 82)
    return p, torch.randn(N_ROWS, d, generator=torch.Generator().manual_seed(N_ROWS + d))


def _split_forward(x, kind, m):
    from implicit_depth_amd.decoders import decoders_forward
    kw = {"prob_dec": m} if kind == "IMNET" else {"offset_dec": m}
    with torch.no_grad():
        return [o for o in decoders_forward(x, precision="f16x3", **kw) if o is not None][0]


def _check_decoder(what, got, p, x, kind, n_iter, sig, group="decoders"):
    with torch.no_grad():
        r64 = orc.decoder_forward(_dev(p, x.device, torch.float64), x.double(), kind, n_iter, sig)
        r32 = orc.decoder_forward(_dev(p, x.device, torch.float32), x, kind, n_iter, sig)
        twin = sp.split_decoder(p, x, kind, n_iter, sig)
    sp.assert_split_close(what, _logits(got, sig), _logits(r64, sig), _logits(r32, sig), _logits(twin, sig),
                          report=REPORT[group])


# D = 385 and 334: the k-step tail and the bias column (386 = 24 x 16 + 2, 335 = 20 x 16 + 15); D = 17: two k-steps
@pytest.mark.parametrize("scale", [1.0, 5.0, 20.0])
@pytest.mark.parametrize("kind,d", [("IMNET", 385), ("IEF", 385), ("IMNET", 334), ("IEF", 334), ("IMNET", 17),
                                    ("IEF", 17)])
def test_decoder_boundary(cuda, kind, d, scale):
    """1,000 rows (8 tiles of 128, the last one of 104 rows: two full wave tiles, one of 8 rows, one empty)."""
    p, x = _decoder_case(kind, d, scale)
    x = x.to(cuda)
    got = _split_forward(x, kind, make_module(kind, p, d, cuda))
    _check_decoder("%s D=%d x%g" % (kind, d, scale), got, p, x, kind, 2, False)


@pytest.mark.parametrize("n", [1, 31, 33, 127, 129])
@pytest.mark.parametrize("kind", ["IMNET", "IEF"])
def test_decoder_boundary_row_edges(cuda, kind, n):
    """Wave-tile (32 rows) and workgroup (128 rows) edges: the first n of the 1,000 rows. A row's result does not
    depend on its neighbours (a row is a column of the matrix instruction's operand, rows past the end are
    clamped), so it is also bit-identical to the same row of the 1,000-row call."""
    p, x = _decoder_case(kind, 385, 5.0)
    x = x.to(cuda)
    m = make_module(kind, p, 385, cuda)
    got = _split_forward(x[:n].contiguous(), kind, m)
    assert got.shape == (n, 1)
    assert torch.equal(got, _split_forward(x, kind, m)[:n])
    _check_decoder("%s n=%d" % (kind, n), got, p, x[:n], kind, 2, False)


@pytest.mark.parametrize("kind,d,n,n_iter,sig", [("IEF", 334, 333, 2, True), ("IMNET", 385, 129, 1, True),
                                                 ("IEF", 385, 1000, 3, False), ("IEF", 334, 333, 3, True)])
def test_decoder_boundary_sigmoid_and_three_iterations(cuda, kind, d, n, n_iter, sig):
    p, x = _decoder_case(kind, d, 5.0)
    x = x[:n].to(cuda)
    got = _split_forward(x, kind, make_module(kind, p, d, cuda, n_iter=n_iter, use_sigmoid=sig))
    _check_decoder("%s D=%d n=%d x%d%s" % (kind, d, n, n_iter, " sigmoid" if sig else ""), got, p, x, kind, n_iter, sig)


def test_decoder_boundary_pair_on_strided_view(cuda):
    """Both decoders in one call on a view of a wider tensor (row stride 404, first column 7)."""
    from implicit_depth_amd.decoders import decoders_forward
    d = 385
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 83, 5.0), 84)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 85, 5.0), 86)
    wide = torch.randn(700, d + 19, generator=torch.Generator().manual_seed(9)).to(cuda)
    x = wide[:, 7:7 + d]
    with torch.no_grad():
        gp, go = decoders_forward(x, make_module("IMNET", pp, d, cuda), make_module("IEF", po, d, cuda),
                                  precision="f16x3")
    xc = x.contiguous()
    _check_decoder("pair strided prob", gp, pp, xc, "IMNET", 2, False)
    _check_decoder("pair strided off", go, po, xc, "IEF", 2, False)


def test_decoder_range_edge(cuda):
    """Weights x55: the largest float64 hidden pre-activation lies in [2^13, 2^15], the activations that are split
    reach 1,100 — inside the f16 range, where the header of lidf_points_h.hip promises unchanged relative accuracy."""
    kind, d = "IMNET", 385
    p, x = _decoder_case(kind, d, 55.0)
    x = x.to(cuda)
    zs, _ = decoder_preacts(_dev(p, cuda, torch.float64), x.double(), kind)
    top = max(z.abs().max().item() for z in zs)
    assert 2.0 ** 13 <= top <= 2.0 ** 15, top
    got = _split_forward(x, kind, make_module(kind, p, d, cuda))
    assert torch.isfinite(got).all()
    _check_decoder("IMNET D=385 x55 (max |z| %.0f)" % top, got, p, x, kind, 2, False, group="range edge")


# ---------------------------------------------------------------------------------------------------------------
# the fused query (lidf_points_h.hip)
# ---------------------------------------------------------------------------------------------------------------
def _scene(B, h, w, N, seed, scale=5.0, ragged=False, off_kind="IEF", **kw):
    s = orc.synthetic_scene(B, h, w, N, seed=seed, ragged=ragged, weight_scale=scale, **kw)
    if off_kind != "IEF":
        s["off_p"] = orc.init_decoder(off_kind, s["D"], 8, scale)
    orc.randomize_biases(s["prob_p"], seed + 1)
    orc.randomize_biases(s["off_p"], seed + 2)
    return s


def _check_query(tag, scene, cuda, off_kind="IEF", n_iter=2, sig=False, **kw):
    """run the product at precision="f16x3" and hold every output to float64; kw: multires, multires_views, pos_rel."""
    from implicit_depth_amd.query import lidf_query
    s = to_dev(scene, cuda)
    D = scene["D"]
    prob = make_module("IMNET", scene["prob_p"], D, cuda, use_sigmoid=sig)
    off = make_module(off_kind, scene["off_p"], D, cuda, n_iter=n_iter, use_sigmoid=sig)
    if kw.get("pos_rel"):
        kw["vox_center"] = s["vox_center"]
    with torch.no_grad():
        got = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                         s["pair_t"], s["feat_grid"], s["vox_feat"], prob, off, ray_flat=s["ray_flat"],
                         precision="f16x3", **kw)
        mid = got["max_pair_id"].long()
        common = dict(off_kind=off_kind, n_iter=n_iter, use_sigmoid=sig, fast_roi=True, max_pair_id=mid, **kw)
        args = lambda c, dt: (c(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(),  # noqa: E731
                              s["pair_vox"].long(), c(s["pair_t"]), s["pair_off"], c(s["feat_grid"]),
                              c(s["vox_feat"]), _dev(scene["prob_p"], cuda, dt), _dev(scene["off_p"], cuda, dt))
        if "vox_center" in kw:
            common64 = dict(common, vox_center=s["vox_center"].double())
        else:
            common64 = common
        r64 = orc.query(*args(lambda v: v.double(), torch.float64), **common64)
        r32 = orc.query(*args(lambda v: v, torch.float32), **common)
        twin = sp.split_query(*args(lambda v: v, torch.float32), **common)
    for k in ("pred_offset", "pred_prob_end"):
        sp.assert_split_close("%s %s logit" % (tag, k), _logits(got[k], sig), _logits(r64[k], sig),
                              _logits(r32[k], sig), _logits(twin[k], sig), report=REPORT["query"])
    for k in ("pair_pred_pos", "pred_pos", "pred_prob_end_softmax"):
        sp.assert_split_close("%s %s" % (tag, k), got[k], r64[k], r32[k], twin[k], report=REPORT["query"])
    if not sig:
        check_selection(scene, got, r64, r32)


@pytest.mark.parametrize("scale", [1.0, 5.0, 20.0])
@pytest.mark.parametrize("ragged", [False, True])
def test_query_small_scene(cuda, ragged, scale):
    """1 x 24 x 32 rays x 16 candidates (12,288 pairs dense; 0-16 per ray ragged: tiles straddle up to a dozen rays)."""
    _check_query("%s x%g" % ("ragged" if ragged else "dense", scale), _scene(1, 24, 32, 16, 42, scale, ragged), cuda)


def test_query_one_pair_per_ray(cuda):
    """N = 1: a 32-point tile has 32 rays, round 0 covers two, 15 more rank-1 rounds go through the todo loop."""
    _check_query("one pair per ray", _scene(1, 16, 24, 1, 41), cuda)


def test_query_second_grab_and_single_tile_tail(cuda):
    """148,255 pairs = 1,159 tiles of 128 (the last one of 31 points). The grid is min(tiles, 2 x CUs) workgroups
    which grab two tiles at a time: above 4 x CUs tiles a workgroup comes back for a second grab and runs the
    weight stream across it, and an odd count makes the last grab a single tile."""
    scene = _scene(1, 96, 128, 24, 7, ragged=True)
    P = scene["P"]
    tiles = (P + 127) // 128
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert 140000 <= P <= 200000 and P % 128 != 0, P
    assert tiles == 1159 and tiles % 2 == 1 and tiles > 4 * cus, (tiles, cus)
    _check_query("1,159 tiles", scene, cuda)


def test_query_fewer_octaves(cuda):
    """multires = 4, multires_views = 2: the kernel is built for 8 octaves, the unused ones carry zero weights."""
    _check_query("4 octaves", _scene(1, 12, 16, 8, 45, multires=4, multires_views=2), cuda, multires=4,
                 multires_views=2)


def test_query_relative_positions(cuda):
    _check_query("pos_rel", _scene(1, 12, 16, 8, 46, ragged=True), cuda, pos_rel=True)


def test_query_imnet_as_offset_decoder(cuda):
    _check_query("IMNet offsets", _scene(1, 12, 16, 8, 47, off_kind="IMNET"), cuda, off_kind="IMNET")


def test_query_sigmoid_three_iterations(cuda):
    _check_query("sigmoid x3", _scene(1, 12, 16, 8, 48), cuda, n_iter=3, sig=True)


# ---------------------------------------------------------------------------------------------------------------
# stage 2: lidf_refine at f16x3 (the IEF on whole rows through lidf_rows_h.hip; the PointNet stays f32)
# ---------------------------------------------------------------------------------------------------------------
REFINE_KEYS = ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pred_pos", "max_pair_id", "pair_vox", "voxel_bound",
               "voxel_bid", "rgb_img", "feat_grid", "valid_inp", "valid_vox")


@functools.lru_cache(maxsize=None)
def _refine_refs(forward_times):
    """The conditioned scene of tests/test_f64_stage2_gpu.py through orc.refine_step on the CPU (it goes through numpy):
    (float64 positions, end voxels, float32 positions, twin positions). The twin applies to the IEF only: the last
    iteration's float64 decoder rows (the trace's "rows") through split_decoder, on the float64 incoming position."""
    case = ref.conditioned_refine_case()[0]
    with torch.no_grad():
        tr = []
        p64, e64 = ref.refine_chain(case, torch.float64, forward_times, trace=tr)
        p32, e32 = ref.refine_chain(case, torch.float32, forward_times)
        off = sp.split_decoder(case["off_p"], tr[-1]["rows"], "IEF")
    assert torch.equal(e64[-1], e32[-1])
    return p64, e64[-1], p32, tr[-1]["pos"] + (off * 0.4 - 0.2) * case["ray_dir"].double()


@pytest.mark.parametrize("forward_times", [1, 2])
def test_refine_inference(cuda, forward_times):
    from implicit_depth_amd.query import lidf_refine
    case = ref.conditioned_refine_case()[0]
    p64, e64, p32, twin = _refine_refs(forward_times)
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    t["pred_pos"] = (case["pred_pos"] + case["noise"] * case["ray_dir"]).contiguous().to(cuda)
    pnet, dec = make_pointnet(case["pnet_p"], cuda), make_module("IEF", case["off_p"], 334, cuda)
    with torch.no_grad():
        pos, ev = lidf_refine(*[t[k] for k in REFINE_KEYS], pnet, dec, forward_times=forward_times, precision="f16x3")
    assert torch.equal(ev.cpu().long(), e64)
    sp.assert_split_close("refine x%d pos" % forward_times, pos, p64, p32, twin, report=REPORT["stage 2"])
