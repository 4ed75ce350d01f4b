"""The per-frame evaluation losses and depth statistics of a whole batch on the device
(lidf_stage1_eval_loss_frames_f32 / lidf_refine_eval_loss_frames_f32 / lidf_depth_metrics_frames_f32).

The contract: row b of a per_frame=True call IS the existing bs == 1 call on frame b alone, bit for bit, NaN positions
included; a frame without a ray is all NaN. The batches (tests/eval_frames.py) are joined FROM bs == 1 frames, so every
yardstick — the bs == 1 call, the float64 restatement, the reference's fixture — comes from code that exists without
the feature.

Findings recorded here: none — every entry of every row came out bit-equal on an MI355X."""
import pytest
import torch

import eval_frames as ef
import eval_loss_ref as el
from test_eval_loss_gpu import _check, _product_dd, _run

pytestmark = pytest.mark.gpu


def _keys(stage):
    return el.EVAL_LOSS_KEYS if stage == 1 else el.REFINE_EVAL_LOSS_KEYS


def _frames(dd, stage, exp_type="test", **opt):
    from implicit_depth_amd import LidfLossOptions, lidf_loss, refine_loss
    return (lidf_loss if stage == 1 else refine_loss)(dd, LidfLossOptions(**opt), exp_type, 0, per_frame=True)


def _same(a, b):
    """Bit-equal where a number stands, NaN at the same positions."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _mismatches(out, refs, stage):
    """[(frame, key)] at which row b of `out` is not, bit for bit, refs[b] (None: a frame without a ray — all NaN)."""
    bad = []
    for b, ref in enumerate(refs):
        for k in _keys(stage):
            got = out[k][b]
            if not (torch.isnan(got) if ref is None else _same(got, ref[k])):
                bad.append((b, k))
    return bad


@pytest.fixture(scope="module")
def cases(cuda):
    """name -> (frames, options, product dict of the joined batch, {(stage, exp_type): the bs == 1 call per frame});
    computed once, never modified."""
    out = {}
    fa, opt_a, _ = ef.batch_a()
    fb, opt_b = ef.batch_b()
    for name, frames, opt in (("A", fa, opt_a), ("B", fb, opt_b)):
        refs = {}
        for stage in (1, 2):
            for exp_type in ("valid", "test"):
                refs[stage, exp_type] = [_run(_product_dd(d, cuda), stage, exp_type, **opt)
                                         if d["miss_bid"].shape[0] else None for d in frames]
        out[name] = (frames, opt, _product_dd(ef.concat_frames(frames), cuda), refs)
    return out


@pytest.mark.parametrize("exp_type", ("valid", "test"))
@pytest.mark.parametrize("stage", (1, 2))
@pytest.mark.parametrize("name", ("A", "B"))
def test_row_is_the_one_frame_call(cases, name, stage, exp_type):
    frames, opt, dd, refs = cases[name]
    out = _frames(dd, stage, exp_type, **opt)
    assert tuple(out) == _keys(stage)
    for k, v in out.items():
        assert v.shape == (len(frames),) and v.dtype == torch.float32 and v.is_cuda and not v.requires_grad, k
    ref = refs[stage, exp_type]
    for b, r in enumerate(ref):
        for k in _keys(stage):
            print(name, stage, exp_type, b, k, float(out[k][b]), "all NaN" if r is None else float(r[k]))
    assert _mismatches(out, ref, stage) == []
    if name == "A":   # the NaN positions the frames were built for
        nan = {b: {k for k in _keys(stage) if torch.isnan(out[k][b])} for b in range(5)}
        assert nan[0] == nan[1] == set() and nan[2] == set(_keys(stage)) and nan[3] == set(el.METRIC_KEYS)
        assert nan[4] == ({"prob_loss", "loss_net"} if stage == 1 else set())
        assert float(out["err"][3]) == 0.0


@pytest.mark.parametrize("stage", (1, 2))
@pytest.mark.parametrize("name", ("A", "B"))
def test_finite_rows_against_float64_and_the_reference_run(cases, name, stage):
    frames, opt, dd, _ = cases[name]
    out = _frames(dd, stage, "test", **opt)
    fixture = ef.batch_a()[2]
    checked = []
    for b, d in enumerate(frames):
        row = {k: out[k][b] for k in _keys(stage)}
        if not all(torch.isfinite(v) for v in row.values()):
            continue
        ref32 = (fixture["loss"] if stage == 1 else fixture["loss_refine"]) if (name, b) == ("A", 1) else None
        _check("%s frame %d" % (name, b), row, d, stage, ref32, **opt)
        checked.append(b)
    assert checked == ({"A": [0, 1] if stage == 1 else [0, 1, 4], "B": [0, 1, 2]}[name])


@pytest.mark.parametrize("stage", (1, 2))
def test_negative_controls(cases, stage):
    """The comparison of test_row_is_the_one_frame_call tells frames apart, and the per-frame flavour from the
    existing bs != 1 one."""
    frames, opt, dd, refs = cases["B"]
    ref = refs[stage, "test"]
    out = _frames(dd, stage, "test", **opt)
    assert _mismatches(out, ref, stage) == []
    swapped = {k: v[[2, 1, 0]] for k, v in out.items()}
    assert _mismatches(swapped, ref, stage) != [] and _mismatches(swapped, [ref[2], ref[1], ref[0]], stage) == []
    whole = _run(dd, stage, "test", **opt)   # (one mean over the rays of all frames, the statistics over the rays)
    bad = _mismatches({k: v.reshape(1).expand(len(frames)) for k, v in whole.items()}, ref, stage)
    # (means over other populations; a2 / a3 are 1 in both flavours on this generator, so they are not asked for)
    assert {b for b, _ in bad} == {0, 1, 2}
    assert {k for _, k in bad} >= {"pos_loss", "surf_norm_loss", "err", "rmse", "mae", "abs_rel"}


def _maps(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    gt = 0.4 + 1.2 * torch.rand(B, h, w, generator=g)
    pred = gt * (1.0 + 0.08 * torch.randn(B, h, w, generator=g))
    seg = torch.rand(B, h, w, generator=g) < 0.6
    gt[torch.rand(B, h, w, generator=g) < 0.1] = 0.0
    gt[0, 3, 5], gt[0, 7, 9], gt[0, 11, 2] = float("nan"), float("inf"), -0.5
    gt[1] = -gt[1].abs()   # no positive pixel: NaN, count 0
    return pred, gt, seg


@pytest.mark.parametrize("h,w", ((16, 24), (48, 64)))
def test_statistics_of_every_frame(cuda, h, w):
    """144 x 256 from 16 x 24 resizes up, from 48 x 64 down (9 x and 3 x in height, 10.67 x and 4 x in width)."""
    from implicit_depth_amd import query as Q
    B = 3
    pred, gt, seg = (t.to(cuda) for t in _maps(B, h, w, seed=h + w))
    for mask in (None, seg, seg.to(torch.uint8), seg.float() * 3.0):
        one = [Q.depth_metrics(pred[b], gt[b], None if mask is None else mask[b]) for b in range(B)]
        got = Q.depth_metrics_frames(pred, gt, mask)
        ws = Q._METRICS_FRAMES_WS[cuda.index, torch.cuda.current_stream(cuda).cuda_stream, B]
        assert not ws.any()
        again = Q.depth_metrics_frames(pred, gt, mask)   # (the same workspace)
        assert not ws.any()
        assert tuple(got) == Q.METRIC_NAMES + ("count",)
        for k in got:
            assert got[k].shape == (B,) and _same(got[k], again[k]), k
            for b in range(B):
                assert _same(got[k][b], one[b][k]), (k, b, float(got[k][b]), float(one[b][k]))
        assert float(got["count"][1]) == 0 and all(torch.isnan(got[k][1]) for k in Q.METRIC_NAMES)
        assert float(got["count"][0]) > 0 and float(got["count"][0]) != float(got["count"][2])
    assert Q.depth_metrics_frames(pred[:0], gt[:0])["a1"].shape == (0,)


def test_eval_metrics_of_every_frame(cuda, cases):
    from implicit_depth_amd import pipeline as pl
    frames, _, dd, _ = cases["B"]
    dd = dict(dd)
    depth = dd["xyz_corrupt_flat"][:, :, 2].reshape(-1).clone()
    depth[dd["ray_bid"].long() * (dd["h"] * dd["w"]) + dd["ray_flat"].long()] = dd["pred_pos"][:, 2]
    dd["pred_depth"] = depth.reshape(dd["bs"], dd["h"], dd["w"])
    got = pl.eval_metrics(dd, frame=None)
    for b in range(dd["bs"]):
        one = pl.eval_metrics(dd, frame=b)
        for k in one:
            assert _same(got[k][b], one[k]), (k, b)


def test_runner_rows_and_pipeline_metrics(cuda):
    from implicit_depth_amd import frame_slice
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    from test_frame_gpu import _dev, _models
    B, h, w = 2, 24, 32
    models = _models(cuda)
    opt = pl.LidfOptions()
    batch, feat = synthetic_batch(B, h, w, seed=77)
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    runner = pl.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], opt, models[3], models[4])
    with torch.no_grad():
        runner.run(batch, feat)
    ok, l1, l2 = runner.loss_dict(batch, per_frame=True)
    assert ok and tuple(l1) == el.EVAL_LOSS_KEYS and tuple(l2) == el.REFINE_EVAL_LOSS_KEYS
    _, dd = runner.result()
    dd["xyz_flat"] = batch["xyz"].permute(0, 2, 3, 1).contiguous().reshape(B, -1, 3)
    dd["xyz_corrupt_flat"] = batch["xyz_corrupt"].permute(0, 2, 3, 1).contiguous().reshape(B, -1, 3)
    dd["corrupt_mask"] = batch["corrupt_mask"].reshape(B, h, w)
    for b in range(B):
        fd = frame_slice(dd, b)
        assert fd["pred_pos"].shape[0] > 0
        for stage, got in ((1, l1), (2, l2)):
            one = pl.eval_loss(fd, stage=stage)
            for k in one:
                assert got[k].shape == (B,) and _same(got[k][b], one[k]), (b, stage, k)
    every = runner.metrics(batch, frame=None)
    for b in range(B):
        one = runner.metrics(batch, frame=b)
        for k in one:
            assert _same(every[k][b], one[k]), (b, k)
    for frame, shape in ((None, (B,)), (0, ())):
        pipe = pl.FramePipeline(2, B, h, w, cuda, *models[:3], opt, models[3], models[4],
                                **({} if frame == 0 else {"metrics_frame": frame}))
        pipe.submit(batch, feat)
        ok, _, m = pipe.collect()
        assert ok
        for k in every:
            assert m[k].shape == shape and _same(m[k], every[k] if frame is None else every[k][0]), (frame, k)


@pytest.mark.parametrize("stage", (1, 2))
def test_hygiene(cuda, cases, stage, monkeypatch):
    from implicit_depth_amd import LidfLossOptions, lidf_loss, refine_loss
    from ws_poison import Poisoner
    frames, opt, dd, refs = cases["B"]
    base = _frames(dd, stage, "test", **opt)
    again = _frames(dd, stage, "test", **opt)
    for k in base:
        assert torch.equal(base[k], again[k]), k                       # run-to-run identical
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        other = _frames(dd, stage, "test", **opt)
    side.synchronize()
    for k in base:
        assert torch.equal(base[k], other[k]), k                       # the caller's stream, the same bits
    poison = Poisoner().install(monkeypatch)
    for mode in ("ones", "high", "random"):
        poison.begin(mode)
        got = _frames(dd, stage, "test", **opt)
        assert len(poison.handed) == 1
        for k in base:
            assert torch.equal(base[k], got[k]), (mode, k)             # any workspace contents
    monkeypatch.undo()
    # bs == 1 with per_frame: the plain call as [1]
    d0 = _product_dd(frames[0], cuda)
    one, plain = _frames(d0, stage, "test", **opt), refs[stage, "test"][0]
    for k in plain:
        assert one[k].shape == (1,) and torch.equal(one[k][0], plain[k]), k
    # no ray in the whole batch: all NaN, no error (the plain call raises, as before)
    empty = _product_dd(ef.concat_frames([ef.without_rays(f) for f in frames[:2]]), cuda)
    got = _frames(empty, stage, "test", **opt)
    assert tuple(got) == _keys(stage)
    assert all(v.shape == (2,) and v.is_cuda and bool(torch.isnan(v).all()) for v in got.values())
    with pytest.raises(RuntimeError, match="no ray"):
        (lidf_loss if stage == 1 else refine_loss)(empty, LidfLossOptions(**opt), "test", 0)


def test_zero_rays_through_the_c_abi(cuda):
    """n_rays == 0 with batch > 0: LIDF_OK, loss filled with NaN on the stream, no launch (NULL lists are fine)."""
    import ctypes as C
    from implicit_depth_amd import _lib
    L = _lib.lib()
    for fn, n in ((L.lidf_stage1_eval_loss_frames_f32, 17), (L.lidf_refine_eval_loss_frames_f32, 15)):
        loss = torch.zeros((3, n), device=cuda)
        a = _lib.LidfEvalLossArgs()
        a.batch, a.height, a.width, a.loss = 3, 4, 4, loss.data_ptr()
        assert fn(C.byref(a), _lib.current_stream(cuda)) == 0
        assert bool(torch.isnan(loss).all())
