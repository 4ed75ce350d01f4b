"""precision="f16x3" together with offsets="selected" at the shipped widths: prob_dec on every pair through the one-net
form of lidf_points_h_kernel, the per-ray arg-max, offset_dec on the one-pair-per-ray list through the kernel's list
form (every row gathers its own ray's row of the layer-1 table, no rank-1 ray rounds).

The contract: pred_prob_end, the softmax and max_pair_id — in the frame also the counts and the voxel / ray features —
are bit-identical to the f16x3 run with offsets="all"; the selected pairs' offsets, pred_pos and what follows are held
to float64 through the twin of this data flow (tests/split_selected_ref.py) at the project's own F64_K /
F64_FLOOR_ULPS; the other rows of pred_offset / pair_pred_pos are NaN; a list row's result depends on that row alone,
which is why the frame call (device-side counts, capacity-sized launches) and the stepwise path agree bit for bit."""
import functools
import gc
import os
import zlib

import pytest
import torch

import split_f16_ref as sp
import split_selected_ref as ss
import stream_order as so
import ws_poison
from entry_cases import QUERY_KEYS, Entry, _scene_inputs, query_scene, same
from test_f64_split_gpu import _dev as _cast, _logits, _scene
from test_frame_gpu import DENSE_SHAPE, OCCUPY, SAME, SAME_INT, _dev, _models
from util import TOL, check_selection, make_module, orc, run_query, tf32_off, to_dev

pytestmark = pytest.mark.gpu

MODE = dict(precision="f16x3", offsets="selected")
PER_PAIR_SELECTED = ("pred_offset", "pair_pred_pos")


@pytest.fixture(autouse=True)
def _full_precision_references():
    with tf32_off():
        yield
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------
# (a) the query against float64
# ---------------------------------------------------------------------------------------------------------------
def _call(s, prob, off, **kw):
    from implicit_depth_amd.query import lidf_query
    with torch.no_grad():
        return lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                          s["pair_t"], s["feat_grid"], s["vox_feat"], prob, off, ray_flat=s["ray_flat"], **kw)


def _check_query(tag, scene, cuda, off_kind="IEF", n_iter=2, sig=False, **kw):
    s = to_dev(scene, cuda)
    D, P, R = scene["D"], scene["P"], scene["R"]
    prob = make_module("IMNET", scene["prob_p"], D, cuda, use_sigmoid=sig)
    off = make_module(off_kind, scene["off_p"], D, cuda, n_iter=n_iter, use_sigmoid=sig)
    if kw.get("pos_rel"):
        kw["vox_center"] = s["vox_center"]
    got = _call(s, prob, off, **MODE, **kw)
    every = _call(s, prob, off, precision="f16x3", **kw)
    # the prob side: the bits of the two-net launch
    for k in ("pred_prob_end", "pred_prob_end_softmax", "max_pair_id"):
        assert torch.equal(got[k], every[k]), (tag, k)
    mid = got["max_pair_id"].long()
    has = mid < P
    rows = mid[has]
    assert (mid[~has] == P).all() and (got["pred_pos"][~has] == 0).all()
    rest = torch.ones(P, dtype=torch.bool, device=cuda)
    rest[rows] = False
    assert torch.isnan(got["pred_offset"][rest]).all() and torch.isnan(got["pair_pred_pos"][rest]).all()
    assert torch.isfinite(got["pred_offset"][rows]).all() and torch.isfinite(got["pair_pred_pos"][rows]).all()
    assert torch.equal(got["pred_pos"][has], got["pair_pred_pos"][rows])
    # the offset side against float64, the twin of the list form as the scheme's own error
    with torch.no_grad():
        common = dict(off_kind=off_kind, n_iter=n_iter, use_sigmoid=sig, fast_roi=True, max_pair_id=mid, **kw)
        args = lambda c, dt: (c(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(),  # noqa: E731
                              s["pair_vox"].long(), c(s["pair_t"]), s["pair_off"], c(s["feat_grid"]),
                              c(s["vox_feat"]), _cast(scene["prob_p"], cuda, dt), _cast(scene["off_p"], cuda, dt))
        common64 = dict(common, vox_center=s["vox_center"].double()) if "vox_center" in kw else common
        r64 = orc.query(*args(lambda v: v.double(), torch.float64), **common64)
        r32 = orc.query(*args(lambda v: v, torch.float32), **common)
        twin = ss.split_selected_query(*args(lambda v: v, torch.float32), **common)
    assert torch.equal(twin["selected_rows"], rows)
    sp.assert_split_close("%s pred_offset logit (selected rows)" % tag, _logits(got["pred_offset"][rows], sig),
                          _logits(r64["pred_offset"][rows], sig), _logits(r32["pred_offset"][rows], sig),
                          _logits(twin["pred_offset"][rows], sig))
    sp.assert_split_close("%s pair_pred_pos (selected rows)" % tag, got["pair_pred_pos"][rows],
                          r64["pair_pred_pos"][rows], r32["pair_pred_pos"][rows], twin["pair_pred_pos"][rows])
    sp.assert_split_close("%s pred_pos" % tag, got["pred_pos"], r64["pred_pos"], r32["pred_pos"], twin["pred_pos"])
    sp.assert_split_close("%s pred_prob_end logit" % tag, _logits(got["pred_prob_end"], sig),
                          _logits(r64["pred_prob_end"], sig), _logits(r32["pred_prob_end"], sig),
                          _logits(twin["pred_prob_end"], sig))
    if not sig:
        check_selection(scene, got, r64, r32)
    return got


@pytest.mark.parametrize("ragged", [True, False])
def test_query_partial_tiles(cuda, ragged):
    """1 x 37 x 53 x 16. Ragged: R = 1,961 list rows = 15 workgroup tiles + 41 rows = one full wave tile + 9 rows, 113
    rays without a pair, P = 16,061 = 61 mod 128 pairs in the prob launch."""
    scene = _scene(1, 37, 53, 16, 42, ragged=ragged)
    R, P = scene["R"], scene["P"]
    assert R == 1961 and R % 128 == 41 and R % 32 == 9
    if ragged:
        assert P == 16061 and int((scene["pair_off"][1:] == scene["pair_off"][:-1]).sum()) == 113
    else:
        assert P == 16 * R
    _check_query("37 x 53 %s" % ("ragged" if ragged else "dense"), scene, cuda)


@pytest.mark.parametrize("shape", [(1, 3, 5, 4), (1, 1, 1, 3)])
def test_query_fewer_rows_than_a_wave_tile(cuda, shape):
    """R = 15 and R = 1: the list is one partial wave tile, every other lane is clamped to its last row."""
    scene = _scene(*shape, 43)
    assert scene["R"] == shape[1] * shape[2]
    _check_query("R = %d" % scene["R"], scene, cuda)


@pytest.mark.parametrize("scale", [1.0, 20.0])
def test_query_weight_scales(cuda, scale):
    """The scale edges of tests/test_f64_split_gpu.py: N(0, 0.02) weights (every low weight piece an f16 subnormal)
    and 20 x that."""
    _check_query("x%g" % scale, _scene(1, 24, 32, 16, 42, scale, ragged=True), cuda)


def test_query_second_grab_on_the_list(cuda):
    """2 x 240 x 320 x 1 ragged: R = 153,600 list rows = 1,200 tiles of 128. The list launch is min(tiles, 2 x CUs)
    workgroups grabbing two tiles at a time from its own counter: above 4 x CUs tiles a workgroup comes back for a
    second grab and runs offset_dec's weight stream across it."""
    scene = _scene(2, 240, 320, 1, 7, ragged=True)
    R = scene["R"]
    tiles = (R + 127) // 128
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert R == 153600 and tiles == 1200 and tiles > 4 * cus, (R, tiles, cus)
    _check_query("1,200 list tiles", scene, cuda)


def test_query_relative_positions(cuda):
    _check_query("pos_rel", _scene(1, 12, 16, 8, 46, ragged=True), cuda, pos_rel=True)


def test_query_imnet_as_offset_decoder(cuda):
    _check_query("IMNet offsets", _scene(1, 12, 16, 8, 47, off_kind="IMNET"), cuda, off_kind="IMNET")


def test_query_sigmoid_three_iterations(cuda):
    _check_query("sigmoid x3", _scene(1, 12, 16, 8, 48), cuda, n_iter=3, sig=True)


def test_query_fewer_octaves(cuda):
    _check_query("4 octaves", _scene(1, 12, 16, 8, 45, multires=4, multires_views=2), cuda, multires=4,
                 multires_views=2)


# ---------------------------------------------------------------------------------------------------------------
# (b) a list row depends on that row alone
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _independence_case():
    return _scene(1, 37, 53, 16, 42, ragged=True)


@pytest.mark.parametrize("n", [1, 31, 33, 127, 129])
def test_list_rows_do_not_depend_on_their_neighbours(cuda, n):
    """The first n rays of the ragged 1 x 37 x 53 x 16 scene on their own (wave-tile and workgroup-tile edges of the
    list) against the same rays of the full call: the same bits."""
    scene = _independence_case()
    s = to_dev(scene, cuda)
    D = scene["D"]
    prob, off = make_module("IMNET", scene["prob_p"], D, cuda), make_module("IEF", scene["off_p"], D, cuda)
    full = _call(s, prob, off, **MODE)
    pn = int(scene["pair_off"][n])
    part = dict(s)
    for k in ("ray_dir", "ray_pix", "ray_bid", "ray_flat"):
        part[k] = s[k][:n].contiguous()
    part["pair_off"] = s["pair_off"][:n + 1].contiguous()
    for k in ("pair_ray", "pair_vox", "pair_t"):
        part[k] = s[k][:pn].contiguous()
    got = _call(part, prob, off, **MODE)
    mid_f, mid = full["max_pair_id"][:n], got["max_pair_id"]
    has = mid < pn
    assert torch.equal(has, mid_f < scene["P"]) and torch.equal(mid[has], mid_f[has]) and (mid[~has] == pn).all()
    rows = mid[has]
    assert rows.numel() > 0 or n == 1
    assert torch.equal(got["pred_pos"], full["pred_pos"][:n])
    for k in PER_PAIR_SELECTED:
        assert torch.equal(got[k][rows], full[k][rows]), k


# ---------------------------------------------------------------------------------------------------------------
# (c) the frame
# ---------------------------------------------------------------------------------------------------------------
def _stepwise(batch, feat, models, opt):
    from implicit_depth_amd import pipeline as pl
    pnet, prob, off, pnet_r, offr = models
    with torch.no_grad():
        ok, dd = pl.lidf_forward(batch, feat, pnet, prob, off, opt, **MODE)
        if ok:
            pl.refine_forward(dd, pnet_r, offr, opt, precision="f16x3")
    return ok, dd


def _compare_selected(dd, ref, first_frame):
    """test_frame_gpu._compare with the per-pair offset outputs taken at the selected pairs (the stepwise path's
    other rows are NaN; the frame's are NaN in a runner's first frame and may be an earlier frame's afterwards)."""
    P = ref["pair_ray"].shape[0]
    m = ref["max_pair_id"].long()
    m = m[m < P]
    assert m.numel() > 0
    for k in SAME:
        if k in PER_PAIR_SELECTED:
            assert torch.equal(dd[k][m], ref[k][m]) and torch.isfinite(dd[k][m]).all(), k
            rest = torch.ones(P, dtype=torch.bool, device=m.device)
            rest[m] = False
            assert torch.isnan(ref[k][rest]).all(), k
            assert not first_frame or torch.isnan(dd[k][rest]).all(), k
        else:
            assert torch.equal(dd[k], ref[k]), k
    for k in SAME_INT:
        assert torch.equal(dd[k].long(), ref[k].long()), k


def _against_all_pairs(a, b, tag):
    """b: this mode, a: the f16x3 frame with offsets='all' on the same inputs."""
    assert a["counts"] == b["counts"]
    for k in ("pred_prob_end", "pred_prob_end_softmax", "max_pair_id", "occ_voxel_feat", "rayfeat"):
        assert torch.equal(a[k], b[k]), k
    assert (a["pred_pos"] - b["pred_pos"]).abs().max().item() <= TOL
    eq = a["end_voxel_id"] == b["end_voxel_id"]
    share = eq.float().mean().item()
    print("%s: end voxels equal on %.4f of %d rays" % (tag, share, eq.numel()))
    assert share >= 0.99
    assert (a["pred_pos_refine"] - b["pred_pos_refine"])[eq].abs().max().item() <= 2 * TOL


@pytest.mark.parametrize("shape,graph", [((3, 37, 53), False), ((2, 48, 64), True), (DENSE_SHAPE, False)])
def test_frame_equals_stepwise_and_the_all_pairs_frame(cuda, shape, graph):
    """Two batches through one runner (and one graph): the second has another P, so nothing is stale. The dense
    layout (every cell occupied, P > 8 R) feeds the list from the 64-lane reduce on the stepwise path and from the
    8-lane one in the frame."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = shape[:3]
    dense = shape[3:] == ("dense",)
    models = _models(cuda)
    opt = pl.LidfOptions()
    sel = pl.FrameRunner(B, h, w, cuda, *models[:3], opt, models[3], models[4], **MODE)
    every = pl.FrameRunner(B, h, w, cuda, *models[:3], opt, models[3], models[4], precision="f16x3")
    counts = []
    # (the dense layout needs 729 valid pixels per image: its second batch has smaller holes, the others' larger ones)
    for it, kw in enumerate((dict(seed=77), dict(seed=78, hole_frac=0.7 if dense else 1.3))):
        batch, feat = synthetic_batch(B, h, w, **kw)
        if dense:
            OCCUPY["dense"](batch)
        batch, feat = _dev(batch, cuda), feat.to(cuda)
        with torch.no_grad():
            every.run(batch, feat)
            sel.load(batch, feat)
            if graph and it == 0:
                sel.capture()
            sel.run()
        ok, b = sel.result()
        ok_a, a = every.result()
        ok_ref, ref = _stepwise(batch, feat, models, opt)
        assert ok and ok_a and ok_ref
        c = b["counts"]
        assert (c["R"], c["P"]) == (ref["miss_ray_dir"].shape[0], ref["pair_ray"].shape[0]) and c["OVERFLOW"] == 0
        assert not dense or c["P"] > 8 * c["R"]
        counts.append(c["P"])
        _compare_selected(b, ref, first_frame=it == 0)
        _against_all_pairs(a, b, "%s frame %d" % (shape, it))
    # (with every cell occupied every pixel's ray crosses the same cells: the dense frames differ in their data only)
    assert dense or counts[0] != counts[1]


def test_frame_with_a_side_stream(cuda):
    """side_stream=True, eager: the same kernels on the same data, every output bit-equal to the one-stream call."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = 2, 48, 64
    models = _models(cuda)
    opt = pl.LidfOptions()
    one = pl.FrameRunner(B, h, w, cuda, *models[:3], opt, models[3], models[4], side_stream=False, **MODE)
    two = pl.FrameRunner(B, h, w, cuda, *models[:3], opt, models[3], models[4], side_stream=True, **MODE)
    batch, feat = synthetic_batch(B, h, w, seed=5)
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    with torch.no_grad():
        one.run(batch, feat)
        two.run(batch, feat)
    ok, a = one.result()
    ok2, b = two.result()
    assert ok and ok2 and a["counts"] == b["counts"]
    for k in SAME + SAME_INT:
        same(b[k], a[k], k, ref="the one-stream call")     # (bit for bit, the NaN rows included)


# ---------------------------------------------------------------------------------------------------------------
# (d) arbitrary workspace contents, the caller's stream
# ---------------------------------------------------------------------------------------------------------------
def _check_against_oracle(scene, ref, got):
    """entry_cases.check_query at the rows this mode writes."""
    P = scene["P"]
    mid = got["max_pair_id"].cpu()
    rows = mid[mid < P]
    for k in ("pred_prob_end", "pred_pos"):
        assert (got[k].cpu() - ref[k]).abs().max().item() <= TOL, k
    for k in PER_PAIR_SELECTED:
        assert (got[k].cpu()[rows] - ref[k][rows]).abs().max().item() <= TOL, k
    assert (got["pred_prob_end_softmax"].cpu() - ref["pred_prob_end_softmax"]).abs().max().item() <= 1e-5


def test_query_on_a_poisoned_workspace(cuda, monkeypatch, request):
    """Every byte of the workspace 0xFF on entry (the two tile counters -1, the tables and the list NaN): equal bits."""
    poison = ws_poison.Poisoner("zeros", seed=zlib.crc32(request.node.nodeid.encode())).install(monkeypatch)
    scene, ref = query_scene()

    def run():
        out = run_query(scene, cuda, want_rayfeat=True, **MODE)
        torch.cuda.synchronize()
        return {k: out[k] for k in QUERY_KEYS}

    base = run()
    assert poison.handed
    poison.begin("ones")
    got = run()
    assert poison.handed
    _check_against_oracle(scene, ref, got)
    same(got, base)


def test_frame_on_a_poisoned_workspace(cuda):
    """Batch A, then batch B through the same runner with its workspace and buffers filled with 0xFF in between: B's
    outputs equal a fresh runner's."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = 2, 48, 64
    models = _models(cuda)
    opt = pl.LidfOptions()
    batch_a, feat_a = synthetic_batch(B, h, w, seed=77)
    batch_b, feat_b = synthetic_batch(B, h, w, seed=78, hole_frac=1.9)
    batch_a, feat_a, batch_b, feat_b = _dev(batch_a, cuda), feat_a.to(cuda), _dev(batch_b, cuda), feat_b.to(cuda)
    fresh = pl.FrameRunner(B, h, w, cuda, *models[:3], opt, models[3], models[4], **MODE)
    runner = pl.FrameRunner(B, h, w, cuda, *models[:3], opt, models[3], models[4], **MODE)
    with torch.no_grad():
        fresh.run(batch_b, feat_b)
        runner.run(batch_a, feat_a)
    torch.cuda.synchronize()
    ok, ref = fresh.result()
    ws_poison.poison_tensor(runner.ws, "ones")
    for t in runner.buf.values():
        ws_poison.poison_tensor(t, "ones")
    with torch.no_grad():
        runner.run(batch_b, feat_b)
    torch.cuda.synchronize()
    ok2, dd = runner.result()
    assert ok and ok2 and dd["counts"] == ref["counts"]
    # (the rows no frame wrote are NaN in both, as the runner's own fill in one and as 0xFF bytes in the other:
    # the per-pair offset outputs are compared at the selected pairs, everything else bit for bit)
    P = ref["counts"]["P"]
    m = ref["max_pair_id"].long()
    m = m[m < P]
    rest = torch.ones(P, dtype=torch.bool, device=cuda)
    rest[m] = False
    assert m.numel() > 0 and bool(rest.any())
    for k in SAME + SAME_INT:
        if k in PER_PAIR_SELECTED:
            same(dd[k][m], ref[k][m], k + " at the selected pairs", ref="a fresh runner")
            assert torch.isfinite(dd[k][m]).all() and torch.isnan(dd[k][rest]).all() and torch.isnan(ref[k][rest]).all(), k
        else:
            same(dd[k], ref[k], k, ref="a fresh runner")


def _entry(dev):
    """entry_cases.entry_lidf_query in this mode."""
    from implicit_depth_amd.query import lidf_query
    scene, ref = query_scene()
    D = scene["D"]
    prob, off = make_module("IMNET", scene["prob_p"], D, dev), make_module("IEF", scene["off_p"], D, dev)

    def call(live):
        depth = torch.zeros((scene["B"], scene["h"], scene["w"]), device=dev)
        with torch.no_grad():
            out = lidf_query(live["ray_dir"], live["ray_pix"], live["ray_bid"], live["pair_off"], live["pair_ray"],
                             live["pair_vox"], live["pair_t"], live["feat_grid"], live["vox_feat"], prob, off,
                             ray_flat=live["ray_flat"], depth=depth, want_rayfeat=True, **MODE)
        out["depth"] = depth
        return {k: out[k] for k in QUERY_KEYS}

    keys = ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pair_off", "pair_ray", "pair_vox", "pair_t", "feat_grid",
            "vox_feat")
    return Entry(_scene_inputs(scene, keys), call, lambda got: _check_against_oracle(scene, ref, got),
                 modules=(prob, off))


def test_query_on_the_callers_stream_with_late_inputs(cuda, monkeypatch):
    """tests/stream_order.py: the call on a fresh stream behind a delay, its inputs and weights arriving on that stream
    only; whatever ran on another queue saw NaN decoys."""
    rec = so.Recorder().install(monkeypatch)
    entry = _entry(cuda)
    base = so.baseline(entry, cuda)
    entry.check(base)
    host_ms, fresh = so.enqueue_ms(entry, cuda)
    so.compare(fresh, base, entry, "on a fresh stream, no delay")
    ms = so.delay_ms(host_ms, "lidf_query f16x3 selected", "late inputs")
    got, running = so.late_inputs(entry, cuda, ms, rec)
    so.compare(got, base, entry, "with late inputs")
    assert running, "inconclusive: the %g ms delay had ended when the enqueue returned" % ms


# ---------------------------------------------------------------------------------------------------------------
# (e) the pybind shim
# ---------------------------------------------------------------------------------------------------------------
def test_shim_equals_ctypes(cuda):
    from implicit_depth_amd import torch_ext
    assert os.path.exists(torch_ext.EXT_PATH), "the pybind shim was not built"
    m = torch_ext.ext()
    scene = orc.synthetic_scene(2, 12, 16, 6, seed=6, ragged=True)
    s = to_dev(scene, cuda)
    D = scene["D"]
    prob, off = make_module("IMNET", scene["prob_p"], D, cuda), make_module("IEF", scene["off_p"], D, cuda)
    pw, ow = torch_ext.decoder_weights(prob), torch_ext.decoder_weights(off)
    depth = torch.zeros(2, 12, 16, device=cuda)
    out = m.forward_query(s["ray_dir"], s["ray_pix"].long(), s["ray_bid"].long(), s["ray_flat"].long(),
                          s["pair_off"], s["pair_ray"], s["pair_vox"], s["pair_t"], s["feat_grid"], s["vox_feat"],
                          None, pw, ow, 2, 0.001, False, 8, 4, 8, False, 0.0, 1.0, 0.25, depth, 1, True)
    d2 = torch.zeros(2, 12, 16, device=cuda)
    ref = _call(s, prob, off, depth=d2, **MODE)
    keys = ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_prob_end_softmax", "max_pair_id", "pred_pos")
    for got, k in zip(out, keys):
        same(got, ref[k], k, ref="the ctypes call")
    assert torch.equal(depth, d2)
    assert torch.isnan(ref["pred_offset"]).any() and not torch.isnan(ref["pred_offset"]).all()
    # by name, the same; left out, offsets='all'
    out_kw = m.forward_query(s["ray_dir"], s["ray_pix"].long(), s["ray_bid"].long(), s["ray_flat"].long(),
                             s["pair_off"], s["pair_ray"], s["pair_vox"], s["pair_t"], s["feat_grid"], s["vox_feat"],
                             None, pw, ow, 2, 0.001, False, 8, 4, 8, False, 0.0, 1.0, 0.25, None, 1,
                             offsets_selected=True)
    same(out_kw[0], ref["pred_offset"], "pred_offset by keyword", ref="the ctypes call")
    out_all = m.forward_query(s["ray_dir"], s["ray_pix"].long(), s["ray_bid"].long(), s["ray_flat"].long(),
                              s["pair_off"], s["pair_ray"], s["pair_vox"], s["pair_t"], s["feat_grid"],
                              s["vox_feat"], None, pw, ow, 2, 0.001, False, 8, 4, 8, False, 0.0, 1.0, 0.25, None, 1)
    assert torch.isfinite(out_all[0]).all() and torch.equal(out_all[1], ref["pred_prob_end"])
