"""The evaluation frame as ONE library call with decoders of gf_dim 32 / 64 / 128 (lidf_frame_widths_f32 through
pipeline.FrameRunner: device-side list lengths, HIP-graph replay, one register-chained launch per decoder) against
the stepwise path at the same widths (pipeline.lidf_forward + refine_forward: generic.query / generic.refine) and
against the oracle chain.

Stage 1 runs the stepwise path's kernels on the same rows, so it is compared bit for bit. Stage 2 runs the factorised
layer 1 (per-voxel and per-ray tables + the embed(pos) columns) where the stepwise path multiplies whole rows: two
f32 routes that differ at 1e-6 m while a cell is 0.25 m, so end_voxel_id has to agree on >= 99 % of the rays (expected
share of differing rays < 1e-4) and the refined positions on those rays within 2e-4, the bound
test_generic_gpu.py::test_eval_chain_at_other_widths applies to stage 2 at other widths."""
import pytest
import torch

from test_frame_gpu import DENSE_SHAPE, OCCUPY, SAME, SAME_INT, _dev, _stepwise
from util import make_pointnet, orc

pytestmark = pytest.mark.gpu

STAGE1 = tuple(k for k in SAME if k not in ("pred_pos_refine", "pred_depth_refine"))
STAGE1_INT = tuple(k for k in SAME_INT if k != "end_voxel_id")
TRIPLES = [(32, 32, 32), (128, 128, 128), (32, 128, 64)]
D1, D2 = 385, 334


def _decoder(kind, D, seed, gf, dev, n_iter=2):
    from implicit_depth_amd import IEF, IMNet
    p = orc.init_decoder(kind, D, seed, 5.0, gf=gf)
    m = IMNet(D, 1, gf) if kind == "IMNET" else IEF(dev, D, 1, gf, n_iter=n_iter)
    m.load_state_dict({k: v.clone() for k, v in p.items()})
    return m.to(dev).eval(), p


def _models(dev, triple, params=False):
    """(pnet, prob_dec, offset_dec, pnet_refine, offset_dec_refine) of test_frame_gpu._models at the decoder widths
    `triple`: the shipped PointNets, IMNet / IEF / IEF decoders with the reference's initialisation x 5."""
    pnet_p, pnetr_p = orc.init_pointnet(3, 1.5), orc.init_pointnet(4, 1.5)
    prob, prob_p = _decoder("IMNET", D1, 7, triple[0], dev)
    off, off_p = _decoder("IEF", D1, 8, triple[1], dev)
    offr, offr_p = _decoder("IEF", D2, 9, triple[2], dev)
    models = (make_pointnet(pnet_p, dev), prob, off, make_pointnet(pnetr_p, dev), offr)
    return (models, (pnet_p, prob_p, off_p, pnetr_p, offr_p)) if params else models


def _runner(dev, shape, models, opt, **kw):
    from implicit_depth_amd import pipeline as pl
    return pl.FrameRunner(shape[0], shape[1], shape[2], dev, models[0], models[1], models[2], opt, models[3],
                          models[4], **kw)


def _compare_stage1(dd, ref):
    for k in STAGE1:
        assert torch.equal(dd[k], ref[k]), k                 # the same kernels on the same rows: bit-equal
    for k in STAGE1_INT:
        assert torch.equal(dd[k].long(), ref[k].long()), k


def _compare(dd, ref):
    _compare_stage1(dd, ref)
    same = dd["end_voxel_id"].long() == ref["end_voxel_id"].long()
    share = float(same.float().mean())
    d = (dd["pred_pos_refine"] - ref["pred_pos_refine"])[same].abs().max().item()
    hw = dd["h"] * dd["w"]
    pix = (dd["ray_bid"].long() * hw + dd["ray_flat"].long())[same]
    dz = (dd["pred_depth_refine"].reshape(-1)[pix] - ref["pred_depth_refine"].reshape(-1)[pix]).abs().max().item()
    print("stage 2: end voxel equal on %.5f of %d rays, max |d pos| %.3g, max |d depth| %.3g"
          % (share, same.numel(), d, dz))
    assert share >= 0.99
    assert d <= 2e-4 and dz <= 2e-4
    # the pixels no ray replaces are the input's depth in both
    keep = torch.ones(dd["pred_depth_refine"].numel(), dtype=torch.bool, device=pix.device)
    keep[dd["ray_bid"].long() * hw + dd["ray_flat"].long()] = False
    assert torch.equal(dd["pred_depth_refine"].reshape(-1)[keep], ref["pred_depth_refine"].reshape(-1)[keep])


def _check_counts(c, ref):
    assert (c["R"], c["P"], c["V"]) == (ref["miss_ray_dir"].shape[0], ref["pair_ray"].shape[0],
                                        ref["voxel_bound"].shape[0])
    assert c["NV"] == ref["revidx"].shape[0] and c["NPN"] == c["NV"] + c["R"] and c["OVERFLOW"] == 0


CASES = [((2, 48, 64), t, True, False, None) for t in TRIPLES] + \
        [((3, 37, 53), t, False, True, 997) for t in TRIPLES] + [(DENSE_SHAPE, (32, 128, 64), False, True, None)]


@pytest.mark.parametrize("shape,triple,graph,use_all_pix,pe_slab", CASES)
def test_frame_widths_equals_stepwise_path(cuda, shape, triple, graph, use_all_pix, pe_slab):
    """Graph replay at (2, 48, 64) without refine_use_all_pix; eager at (3, 37, 53) with slabs of 997 pairs (several
    slabs live, no boundary a multiple of the 16-row sub-tile); every cell occupied (P > 8 R) for one triple. A second
    batch through the same runner / graph gives a different P: nothing stale."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = shape[:3]
    models = _models(cuda, triple)
    opt = pl.LidfOptions(refine_use_all_pix=use_all_pix)
    runner = _runner(cuda, shape, models, opt, pe_slab=pe_slab)
    assert runner.widths
    batch, feat = synthetic_batch(B, h, w, seed=77)
    V = OCCUPY[shape[3]](batch) if len(shape) > 3 else None
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
    _check_counts(c, ref)
    assert V is None or c["V"] == V
    assert shape[3:] != ("dense",) or c["P"] > 8 * c["R"]
    assert pe_slab is None or c["P"] > 3 * pe_slab
    _compare(dd, ref)
    batch2, feat2 = synthetic_batch(B, h, w, seed=78, hole_frac=1.3)
    batch2, feat2 = _dev(batch2, cuda), feat2.to(cuda)
    with torch.no_grad():
        runner.run(batch2, feat2)
    ok2, dd2 = runner.result()
    ok_ref2, ref2 = _stepwise(batch2, feat2, models, opt)
    assert ok2 and ok_ref2 and dd2["counts"]["P"] != c["P"]
    _check_counts(dd2["counts"], ref2)
    _compare(dd2, ref2)


def test_frame_widths_vs_oracle(cuda):
    """gf 32 / 32 / 32 at (2, 48, 64) against orc.lidf_forward + 2 x orc.refine_step with the assertions and numbers
    of test_generic_gpu.py::test_eval_chain_at_other_widths — made on the stepwise result first, so that a miss
    there points at the inputs and not at the frame call."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = 2, 48, 64
    models, (pnet_p, prob_p, off_p, pnetr_p, offr_p) = _models(cuda, (32, 32, 32), params=True)
    batch, feat = synthetic_batch(B, h, w, seed=77)
    ok_ref, ref = orc.lidf_forward(batch, feat, pnet_p, prob_p, off_p, fast_roi=False)
    assert ok_ref
    cur = ref["pred_pos"]
    for _ in range(2):
        cur, end_ref, _ = orc.refine_step(cur, ref["miss_ray_dir"], ref["miss_img_ind"], ref["miss_bid"],
                                          ref["miss_flat_img_id"], ref["max_pair_id"], ref["pair_vox"],
                                          ref["voxel_bound"], ref["occ_vox_bid"], batch["rgb"], feat, ref["pnet_inp"],
                                          ref["revidx"], pnetr_p, offr_p, ray_rgb=ref["ray_rgb"])
    opt = pl.LidfOptions()
    dev_batch, dev_feat = _dev(batch, cuda), feat.to(cuda)
    ok, step = _stepwise(dev_batch, dev_feat, models, opt)
    runner = _runner(cuda, (B, h, w), models, opt)
    with torch.no_grad():
        runner.run(dev_batch, dev_feat)
    ok2, dd = runner.result()
    assert ok and ok2
    for name, got in (("stepwise", step), ("frame", dd)):
        assert (got["pair_ray"].cpu().long() == ref["pair_ray"]).all(), name
        assert (got["pair_vox"].cpu().long() == ref["pair_vox"]).all(), name
        assert float((got["occ_voxel_feat"].cpu() - ref["occ_voxel_feat"]).abs().max()) <= 2e-5, name
        for k in ("pred_offset", "pred_prob_end", "pair_pred_pos"):
            assert float((got[k].cpu() - ref[k]).abs().max()) <= 1e-4, (name, k)
        same = got["max_pair_id"].cpu() == ref["max_pair_id"]
        assert float(same.float().mean()) >= 0.99, name
        assert float((got["pred_pos"].cpu() - ref["pred_pos"])[same].abs().max()) <= 1e-4, name
        end_same = got["end_voxel_id"].cpu().long() == end_ref
        if name == "stepwise":
            assert end_same[same].all(), name
        else:   # (the factorised layer 1: a position within 1e-6 m of a cell face may fall on the other side)
            assert float(end_same[same].float().mean()) >= 0.99, name
        both = same & end_same
        assert float((got["pred_pos_refine"].cpu() - cur)[both].abs().max()) <= 2e-4, name


def test_frame_widths_short_and_empty_lists(cuda):
    """A 'pred' mask that selects 5 rays (fewer rows than one 16-row sub-tile), one that selects none, a frame
    without a valid point — what lidf_frame_f32 returns in test_frame_pred_mask_early_exits_and_overflow — and a
    max_pairs below P."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = 1, 24, 32
    models = _models(cuda, (32, 32, 32))
    batch, feat = synthetic_batch(B, h, w, seed=5)
    b, feat = _dev(batch, cuda), feat.to(cuda)
    opt = pl.LidfOptions(mask_type="pred")
    pm = torch.zeros(B, h, w)
    pm.view(-1)[torch.tensor([266, 267, 400, 401, 500])] = 1.0    # interior pixels of rows 8, 12 and 15
    pm = pm.to(cuda)
    runner = _runner(cuda, (B, h, w), models, opt)
    with torch.no_grad():
        runner.run(b, feat, pm)
        ok, dd = runner.result()
        ok_ref, ref = pl.lidf_forward(b, feat, models[0], models[1], models[2], opt, pred_mask=pm)
        pl.refine_forward(ref, models[3], models[4], opt)
    assert ok and ok_ref and dd["counts"]["R"] == 5
    _check_counts(dd["counts"], ref)
    _compare(dd, ref)
    with torch.no_grad():
        runner.run(b, feat, torch.zeros(B, h, w, device=cuda))            # no miss ray
        ok, d0 = runner.result()
        assert not ok and d0["counts"]["R"] == 0 and d0["counts"]["P"] == 0
        far = dict(b)
        far["xyz_corrupt"] = b["xyz_corrupt"] + 50.0                      # no occupied voxel
        runner.run(far, feat, pm)
        ok, d0 = runner.result()
        assert not ok and d0["counts"]["V"] == 0 and d0["counts"]["P"] == 0 and d0["counts"]["NV"] == 0
        runner.run(b, feat, pm)                                           # and a good frame through the same buffers
        ok, dd = runner.result()
        assert ok
        _compare(dd, ref)
    small = pl.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], pl.LidfOptions(), max_pairs=100)
    with torch.no_grad():
        small.run(b, feat)
    assert small.counts()["OVERFLOW"] == 1 and small.counts()["P"] == 100
    with pytest.raises(RuntimeError, match="max_pairs"):
        small.result()


def test_frame_widths_weight_streams_follow_parameter_updates(cuda):
    """A p.data write to offset_dec (gf 32) and to offset_dec_refine between two frames of a captured graph changes
    the next frame; stage 1 still equals the stepwise path."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = 2, 48, 64
    models = _models(cuda, (32, 32, 32))
    opt = pl.LidfOptions()
    batch, feat = synthetic_batch(B, h, w, seed=77)
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    runner = _runner(cuda, (B, h, w), models, opt)
    with torch.no_grad():
        runner.load(batch, feat)
        runner.capture()

    def frame():
        with torch.no_grad():
            runner.run(batch, feat)
        ok, dd = runner.result()
        assert ok
        return {k: dd[k].clone() for k in ("pred_offset", "pred_prob_end", "pred_pos", "pred_pos_refine")}, dd

    first, _ = frame()
    again, _ = frame()
    for k in first:
        assert torch.equal(first[k], again[k]), k
    for p in models[2].parameters():                       # offset_dec, every layer and the offset encoder
        p.data.mul_(1.25)
    second, dd = frame()
    assert not torch.equal(second["pred_offset"], first["pred_offset"])
    assert torch.equal(second["pred_prob_end"], first["pred_prob_end"])
    ok_ref, ref = _stepwise(batch, feat, models, opt)
    assert ok_ref
    _compare(dd, ref)
    models[4].linear_1.bias.data.add_(0.05)               # offset_dec_refine: the bias row and the guard follow
    models[4].linear_3.weight.data.mul_(1.5)
    third, dd = frame()
    assert torch.equal(third["pred_pos"], second["pred_pos"])
    assert not torch.equal(third["pred_pos_refine"], second["pred_pos_refine"])
    ok_ref, ref = _stepwise(batch, feat, models, opt)
    assert ok_ref
    _compare(dd, ref)


def test_frame_widths_position_types(cuda):
    """intersect_pos_type 'rel', refine.intersect_pos_type 'rel', refine.pnet_pos_type 'abs' at gf 128."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = 2, 30, 40
    models = _models(cuda, (128, 128, 128))
    opt = pl.LidfOptions(intersect_pos_type="rel", refine_intersect_pos_type="rel", refine_pnet_pos_type="abs")
    batch, feat = synthetic_batch(B, h, w, seed=21)
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    runner = _runner(cuda, (B, h, w), models, opt)
    with torch.no_grad():
        runner.run(batch, feat)
    ok, dd = runner.result()
    ok_ref, ref = _stepwise(batch, feat, models, opt)
    assert ok and ok_ref
    _check_counts(dd["counts"], ref)
    _compare(dd, ref)


def _poison(runner):
    """Both workspaces (the slab of embedding rows included) and every float output NaN; every index buffer 0 — an
    in-range value, so that a launch that reads beyond a count shows as a wrong number and not as a fault."""
    runner.ws.fill_(0xFF)
    runner.ws_widths.fill_(0xFF)
    for k, t in runner.buf.items():
        if k == "counts":
            continue
        if t.is_floating_point():
            t.fill_(float("nan"))
        else:
            t.zero_()


def test_frame_widths_workspace_contents_and_stream(cuda):
    """Arbitrary workspace contents and a non-default stream with late inputs (tests/stream_order.py) give the bits
    of the plain run."""
    import stream_order as so
    from entry_cases import Entry
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w = 2, 48, 64
    models = _models(cuda, (32, 128, 64))
    opt = pl.LidfOptions(refine_use_all_pix=False)
    batch, feat = synthetic_batch(B, h, w, seed=78, hole_frac=1.9)
    keys = ("rgb", "xyz_corrupt", "depth_corrupt", "fx", "fy", "cx", "cy")
    runner = _runner(cuda, (B, h, w), models, opt, pe_slab=4000)
    out_keys = STAGE1 + STAGE1_INT + ("pred_pos_refine", "pred_depth_refine", "end_voxel_id", "counts")

    def call(live):
        with torch.no_grad():
            runner.run({k: live[k] for k in keys}, live["feat"])
        return dict(runner.buf)

    def finish(res):
        real, runner.buf = runner.buf, res
        try:
            ok, dd = runner.result()
        finally:
            runner.buf = real
        assert ok, dd["counts"]
        return {k: dd[k] for k in out_keys}

    inputs = {k: batch[k] for k in keys}
    inputs["feat"] = feat
    entry = Entry(inputs, call, lambda got: None, modules=models, zero=("depth_corrupt",), finish=finish)
    base = so.baseline(entry, cuda)
    assert base["counts"]["P"] > 4000 and base["counts"]["OVERFLOW"] == 0
    _poison(runner)
    got = so.baseline(entry, cuda)
    so.compare(got, base, entry, "poisoned workspaces and buffers")
    host_ms, fresh = so.enqueue_ms(entry, cuda)
    so.compare(fresh, base, entry, "a fresh stream, no delay")
    _poison(runner)
    ms = so.delay_ms(host_ms, "frame_widths", "late inputs")
    got, running = so.late_inputs(entry, cuda, ms)
    so.compare(got, base, entry, "late inputs on a non-default stream")
    assert running, "the delay had ended when the frame returned to the host: inconclusive"


def test_frame_widths_refusals(cuda, monkeypatch):
    """What the one-call route is not built for raises with the reason, naming FrameRunner."""
    from implicit_depth_amd import PointNet2Stage, pipeline as pl
    models = _models(cuda, (32, 32, 32))
    opt = pl.LidfOptions()
    for kw in (dict(offsets="selected"), dict(precision="f16x3"), dict(side_stream=True)):
        with pytest.raises(RuntimeError, match="FrameRunner.*shipped widths"):
            _runner(cuda, (1, 24, 32), models, opt, **kw)
    narrow, _ = _decoder("IMNET", D1, 7, 16, cuda)
    with pytest.raises(RuntimeError, match="FrameRunner.*gf_dim 32, 64 or 128"):
        _runner(cuda, (1, 24, 32), (models[0], narrow) + models[2:], opt)
    pnet64 = PointNet2Stage(6, 64, 32).to(cuda).eval()
    with pytest.raises(RuntimeError, match="FrameRunner"):
        _runner(cuda, (1, 24, 32), (pnet64,) + models[1:], opt)
    monkeypatch.setenv("LIDF_CHAIN16", "0")
    with pytest.raises(RuntimeError, match="FrameRunner.*LIDF_CHAIN16"):
        _runner(cuda, (1, 24, 32), models, opt)
