"""The evaluation flavour ('valid' / 'test') of lidf_loss / refine_loss on the device (lidf_stage1_eval_loss_f32 /
lidf_refine_eval_loss_f32) against the float64 restatement tests/eval_loss_ref.py, with the float32 fixture
(tests/golden/g12_valid_loss.npz, the reference's own run) or the float32 restatement as the yardstick
(util.assert_f64_close); a1 - a3 as exact counts."""
import pytest
import torch

import eval_loss_ref as el
import train_loss_ref as tl
from util import assert_f64_close

pytestmark = pytest.mark.gpu

STAT = ("a1", "a2", "a3")


def _product_dd(d, dev):
    """The product's data_dict from a restatement dict: pairs ray-major (a stable sort keeps each ray's order),
    compute_gt's entries built on the host."""
    bs, h, w = d["bs"], d["h"], d["w"]
    R = d["miss_bid"].shape[0]
    lin = d["miss_bid"] * (h * w) + d["miss_flat"]
    table = torch.full((bs * h * w,), -1, dtype=torch.int32)
    table[lin] = torch.arange(R, dtype=torch.int32)
    dd = {"bs": bs, "h": h, "w": w, "xyz_flat": d["xyz_flat"].to(dev), "xyz_corrupt_flat": d["xyz_corrupt_flat"].to(dev),
          "corrupt_mask": d["corrupt_mask"].to(dev), "ray_bid": d["miss_bid"].int().to(dev),
          "ray_flat": d["miss_flat"].int().to(dev), "gt_pos": d["gt_pos"].to(dev), "pix2ray": table.to(dev),
          "pred_pos": d["pred_pos"].to(dev), "pred_pos_refine": d["pred_pos_refine"].to(dev)}
    if "pair_ray" in d:
        order = torch.argsort(d["pair_ray"], stable=True)
        ray, label = d["pair_ray"][order], d["pcl_label"][order]
        off = torch.zeros(R + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.bincount(ray, minlength=R), 0)
        dd.update({"pair_off": off.int().to(dev), "pcl_label": label.to(dev),
                   "gt_max_pair_id": tl.segment_argmax(label.float(), ray, R).to(dev),
                   "n_label": torch.tensor([int(label.sum())], dtype=torch.int32, device=dev)[0],
                   "pred_prob_end": d["pred_prob_end"][order].contiguous().to(dev)})
    return dd


def _run(dd, stage, exp_type="valid", **opt):
    from implicit_depth_amd import LidfLossOptions, lidf_loss, refine_loss
    return (lidf_loss if stage == 1 else refine_loss)(dd, LidfLossOptions(**opt), exp_type, 0)


def _check(what, out, d, stage, ref32=None, **opt):
    """out against the float64 restatement; ref32: the fixture's vector (default: the float32 restatement)."""
    keys = el.EVAL_LOSS_KEYS if stage == 1 else el.REFINE_EVAL_LOSS_KEYS
    assert tuple(out) == keys
    r64 = el.eval_loss_ref(d, torch.float64, stage, 0, **opt)
    r32 = el.eval_loss_ref(d, torch.float32, stage, 0, **opt)
    n = float(r64["count"])
    for i, k in enumerate(keys):
        got = out[k]
        assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32 and not got.requires_grad, k
        y32 = r32[k] if ref32 is None else ref32[i]
        print(what, stage, k, float(got), float(r64[k]), float(y32))
        if k in STAT:
            assert round(float(got) * n) == round(float(r64[k]) * n) == round(float(y32) * n), (what, k)
        else:
            assert_f64_close("%s stage %d %s" % (what, stage, k), got.reshape(1), r64[k].reshape(1),
                             y32.reshape(1).float())


def _opt(g, name):
    pos_w, prob_w, surf_w, smooth_w, _ = (float(v) for v in g[name + "_loss_opt"])
    return dict(pos_w=pos_w, prob_w=prob_w, surf_norm_w=surf_w, smooth_w=smooth_w, **el.G12_CASES[name][1])


@pytest.mark.parametrize("stage", (1, 2))
@pytest.mark.parametrize("name", sorted(el.G12_CASES))
def test_fixture_cases(cuda, name, stage):
    g = el.g12_file()
    d, ref = el.g12_case(g, name)
    opt = _opt(g, name)
    out = _run(_product_dd(d, cuda), stage, el.G12_CASES[name][0], **opt)
    _check(name, out, d, stage, ref["loss"] if stage == 1 else ref["loss_refine"], **opt)


@pytest.fixture(scope="module")
def sized():
    """B = 3, 20 x 27, hole fraction about 0.6: R is no multiple of 256 and more than 512 (several blocks, a ragged
    last one); the same generated frame 0 alone is the B = 1 case."""
    d3 = el.random_case(3, 20, 27, 0.6, seed=5)
    assert d3["miss_bid"].shape[0] > 512 and d3["miss_bid"].shape[0] % 256 != 0
    R0 = int((d3["miss_bid"] == 0).sum())   # (the rays come in (frame, pixel) order)
    pk = d3["pair_ray"] < R0
    d1 = dict(d3, bs=1, pair_ray=d3["pair_ray"][pk], pred_prob_end=d3["pred_prob_end"][pk], pcl_label=d3["pcl_label"][pk])
    for k in ("xyz_flat", "xyz_corrupt_flat", "corrupt_mask"):
        d1[k] = d3[k][:1].contiguous()
    for k in ("miss_bid", "miss_flat", "gt_pos", "pred_pos", "pred_pos_refine"):
        d1[k] = d3[k][:R0].contiguous()
    return d3, d1


@pytest.mark.parametrize("stage", (1, 2))
def test_ragged_blocks_against_float64(cuda, sized, stage):
    d = sized[0]
    opt = dict(smooth_w=0.5)
    _check("3x20x27", _run(_product_dd(d, cuda), stage, **opt), d, stage, **opt)


@pytest.mark.parametrize("stage", (1, 2))
def test_one_frame_takes_the_resize_branch(cuda, sized, stage):
    from implicit_depth_amd import pipeline as pl
    d = sized[1]
    dd = _product_dd(d, cuda)
    out = _run(dd, stage, "test", smooth_w=0.5)
    _check("1x20x27", out, d, stage, smooth_w=0.5)
    # the nine statistics: bit-equal to pipeline.eval_metrics on the same depth image
    pred = d["pred_pos"] if stage == 1 else d["pred_pos_refine"]
    depth = d["xyz_corrupt_flat"][0, :, 2].clone()
    depth[d["miss_flat"]] = pred[:, 2]
    dd["pred_depth"] = depth.reshape(1, d["h"], d["w"]).to(cuda)
    m = pl.eval_metrics(dd)
    for k in el.METRIC_KEYS:
        assert torch.equal(out[k], m[k]), k


@pytest.mark.parametrize("stage", (1, 2))
def test_hard_neg_routes_agree_and_runs_are_bit_identical(cuda, stage):
    g = el.g12_file()
    d, _ = el.g12_case(g, "c")
    opt = _opt(g, "c")
    dd = _product_dd(d, cuda)
    a = _run(dd, stage, hard_neg_select="torch", **opt)
    b = _run(dd, stage, hard_neg_select="device", **opt)
    c = _run(dd, stage, hard_neg_select="device", **opt)
    for k in a:
        assert torch.equal(b[k], c[k]), k
        # (the two selects sum the same k values in different orders: one float32 rounding of the mean, and of
        # loss_net its weighted sum)
        assert abs(float(a[k]) - float(b[k])) <= 4 * 2.0 ** -23 * abs(float(a[k])), (k, float(a[k]), float(b[k]))
    d3 = el.random_case(3, 20, 27, 0.6, seed=5)
    dd3 = _product_dd(d3, cuda)
    x, y = _run(dd3, stage, smooth_w=0.5), _run(dd3, stage, smooth_w=0.5)
    for k in x:
        assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("stage", (1, 2))
def test_no_term_buffers_no_autograd_no_sync(cuda, sized, stage, monkeypatch):
    from implicit_depth_amd import losses
    d = sized[0]
    dd = _product_dd(d, cuda)
    dd["pred_pos"].requires_grad_(True), dd["pred_pos_refine"].requires_grad_(True)
    dd["pred_prob_end"].requires_grad_(True)
    R, P = d["miss_bid"].shape[0], d["pair_ray"].shape[0]
    shapes, real = [], torch.empty

    def empty(shape, *a, **kw):
        shapes.append(tuple(shape))
        return real(shape, *a, **kw)
    monkeypatch.setattr(losses.torch, "empty", empty)
    _run(dd, stage)   # (warm: library load and allocator)
    del shapes[:]
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _run(dd, stage)
        out_dev = _run(dd, stage, hard_neg=True, hard_neg_ratio=0.1, hard_neg_select="device")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(not v.requires_grad and v.grad_fn is None for v in list(out.values()) + list(out_dev.values()))
    plain = shapes[:shapes.index((17 if stage == 1 else 15,), 1)]
    assert (R,) not in plain and (P,) not in plain and (R, 2) not in plain, plain
    assert shapes.count((R,)) == 4 and shapes.count((P,)) == (1 if stage == 1 else 0)   # (the hard_neg call's)


@pytest.mark.parametrize("stage", (1, 2))
@pytest.mark.parametrize("bs", (1, 2))
def test_empty_selection_gives_nan_statistics_and_zero_err(cuda, stage, bs):
    d = el.random_case(bs, 12, 20, 0.5, seed=2, zero_gt=True)
    out = _run(_product_dd(d, cuda), stage)
    assert float(out["err"]) == 0.0
    for k in el.METRIC_KEYS:
        assert torch.isnan(out[k]), k
    assert torch.isfinite(out["pos_loss"]) and torch.isfinite(out["angle_err"])


def test_frame_runner_loss_dict_equals_the_stepwise_losses(cuda):
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    from test_frame_gpu import _dev, _models, _stepwise
    models = _models(cuda)
    for B in (1, 2):
        opt = pl.LidfOptions()
        batch, feat = synthetic_batch(B, 24, 32, seed=77)
        batch, feat = _dev(batch, cuda), feat.to(cuda)
        runner = pl.FrameRunner(B, 24, 32, cuda, models[0], models[1], models[2], opt, models[3], models[4])
        with torch.no_grad():
            runner.run(batch, feat)
        ok, l1, l2 = runner.loss_dict(batch)
        ok_ref, dd = _stepwise(batch, feat, models, opt)
        assert ok and ok_ref
        r1, r2 = pl.eval_loss(dd, stage=1), pl.eval_loss(dd, stage=2)
        _, fd = runner.result()
        same = all(torch.equal(fd[k], dd[k]) for k in ("pred_pos", "pred_prob_end", "pred_pos_refine", "pair_off"))
        for got, ref in ((l1, r1), (l2, r2)):
            assert tuple(got) == tuple(ref)
            for k in got:
                if same:
                    assert torch.equal(got[k], ref[k]) or (torch.isnan(got[k]) and torch.isnan(ref[k])), (B, k)
                else:
                    assert abs(float(got[k]) - float(ref[k])) <= 1e-4 * max(abs(float(ref[k])), 1.0), (B, k)


def test_training_flavour_reads_xyz_flat_as_before(cuda):
    """The training kernels are the <.., EVAL = false> instantiations of the same templates, instruction for
    instruction those of the parent commit (compared at build time); here: the g9 losses against their fixture with
    an xyz_corrupt_flat present that must not be read."""
    from implicit_depth_amd import LidfLossOptions, lidf_loss
    from test_train_step_gpu import _ray_major
    g, _ = tl.g9_files()
    for name in sorted(tl.G9_CASES):
        d, ref = tl.g9_case(g, name)
        epoch, opt = tl.g9_opt(name)
        dd, _ = _ray_major(d, cuda)
        a = lidf_loss(dict(dd), LidfLossOptions(**opt), "train", epoch)
        dd["xyz_corrupt_flat"] = torch.zeros_like(dd["xyz_flat"])
        b = lidf_loss(dict(dd), LidfLossOptions(**opt), "train", epoch)
        for i, k in enumerate(tl.LOSS_KEYS):
            assert torch.equal(a[k].detach(), b[k].detach()), (name, k)
            assert abs(float(a[k]) - float(ref["loss"][i])) <= 2e-5 * max(abs(float(ref["loss"][i])), 1e-30), (name, k)
