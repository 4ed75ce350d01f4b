"""GPU: every route that serves widths other than the shipped configuration against the fixtures generated from the
reference at those widths (tests/golden/make_golden_widths*.py).

Yardstick: assert_f64_close(got, float64 oracle on the fixture's inputs, fixture) — the reference's own float32 run is
the unit: the product may be F64_K (bias gradients: K_BIAS) times less accurate than the code it replaces, and no more.
tests/test_golden_widths.py holds the oracle to the same fixtures on the CPU and shows that these comparisons refuse a
zeroed tensor, a row mean and two exchanged rows."""
import pytest
import torch

import golden_widths_ref as gw
from golden_widths_ref import strided
from test_golden_widths import G13_KEYS, g13_case, g13_tensors
from util import assert_f64_close, make_module

pytestmark = pytest.mark.gpu


def _show(report):
    for row in report:
        print("  %-60s ratio %.2f elementwise / %.2f normwise" % (row["what"], row["ratio_max"], row["ratio_nrm"]))
    if report:
        print("  largest: %.2f elementwise / %.2f normwise" % (max(r["ratio_max"] for r in report),
                                                              max(r["ratio_nrm"] for r in report)))


def _g13_module(c, cuda):
    return make_module(c["kind"], c["p"], c["d"], cuda, n_iter=c["n_iter"], use_sigmoid=c["sig"], gf=c["gf"])


def _g13_output(c, route, got, report):
    name, fix, o64, _, k, through = next(t for t in g13_tensors(c) if t[0] == "y")
    assert_f64_close("g13 %s %s y" % (c["key"], route), through(got), through(o64), through(fix), k=k, report=report)


@pytest.mark.parametrize("key", G13_KEYS)
def test_g13_forward_chain(cuda, key):
    """Module forward without autograd: lidf_decoder_chain_f32, one launch (113 rows: seven 16-row sub-tiles + 1 row)."""
    from implicit_depth_amd import generic
    c = g13_case(key)
    mod = _g13_module(c, cuda)
    assert generic.chain_ok(mod)
    with torch.no_grad():
        got = mod(c["x"].to(cuda))
    report = []
    _g13_output(c, "chain", got, report)
    _show(report)


@pytest.mark.parametrize("key", G13_KEYS)
def test_g13_forward_layers(cuda, monkeypatch, key):
    """The same forward with LIDF_CHAIN16=0: the layered route, one lidf_linear_f32 launch per layer and pass."""
    from implicit_depth_amd import generic
    c = g13_case(key)
    mod = _g13_module(c, cuda)
    monkeypatch.setenv("LIDF_CHAIN16", "0")
    assert not generic.chain_ok(mod)
    with torch.no_grad():
        got = mod(c["x"].to(cuda))
    report = []
    _g13_output(c, "layers", got, report)
    _show(report)


@pytest.mark.parametrize("key", G13_KEYS)
def test_g13_autograd(cuda, key):
    """The module under autograd (generic.decoder_forward_train): output, input-row and parameter gradients."""
    c = g13_case(key)
    mod = _g13_module(c, cuda).train()
    x = c["x"].to(cuda).requires_grad_(True)
    y = mod(x)
    assert y.requires_grad
    (y * c["wgt"].to(cuda)).sum().backward()
    got = {"y": y.detach(), "g_input": x.grad}
    for k, v in mod.named_parameters():
        got["g_" + k] = strided(v.grad, c["stride"])
    report = []
    for name, fix, o64, _, k, through in g13_tensors(c):
        assert_f64_close("g13 %s autograd %s" % (key, name), through(got[name].cpu()), through(o64), through(fix), k=k,
                         report=report)
    assert len(report) == len(got)
    _show(report)


# ------------------------------------------------------------------------------------------------------------- g14
def _dev(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _g14_setup(name, cuda):
    """(fixture, float64 oracle, float32 oracle's integer results, product modules, LidfOptions keywords)."""
    from test_golden_widths import g14_fixture, g14_oracle
    from util import make_pointnet
    cfg, fix = gw.G14[name], g14_fixture(name)
    pnet_p, prob_p, off_p, pnetr_p, offr_p = gw.widths_params(cfg, fix["seeds"], fix["factors"], fix["D"])
    D1, D2 = (int(v) for v in fix["D"])
    models = (make_pointnet(pnet_p, cuda, out=cfg["pnet_out"], gf=cfg["pnet_gf"]),
              make_module("IMNET", prob_p, D1, cuda, gf=cfg["gf"]),
              make_module("IEF", off_p, D1, cuda, n_iter=cfg["n_iter"], gf=cfg["gf"]),
              make_pointnet(pnetr_p, cuda, out=cfg["r_pnet_out"], gf=cfg["r_pnet_gf"]),
              make_module("IEF", offr_p, D2, cuda, n_iter=cfg["r_n_iter"], gf=cfg["r_gf"]))
    kw = dict(roi_out_bbox=cfg["roi_out"], intersect_pos_type="rel" if cfg["pos_rel"] else "abs",
              refine_intersect_pos_type="rel" if cfg["r_pos_rel"] else "abs",
              refine_pnet_pos_type="rel" if cfg["r_pnet_pos_rel"] else "abs",
              offset_range=tuple(float(v) for v in fix["offset_range"]),
              refine_offset_range=tuple(float(v) for v in fix["refine_offset_range"]))
    return fix, g14_oracle(name, True), models, kw


def _g14_stage1(what, dd, fix, o64, report):
    """The stage-1 half of a data_dict against the fixture: lists equal, floats held to the float64 oracle."""
    from implicit_depth_amd.query import to_reference_order
    from test_golden_widths import G14_PAIR_KEYS
    for got, ref in (("occ_vox_bid", "occ_vox_bid"), ("revidx", "revidx"), ("valid_v_pid", "valid_v_pid"),
                     ("ray_bid", "miss_bid"), ("ray_flat", "miss_flat_img_id")):
        assert torch.equal(dd[got].long().cpu(), fix[ref].long()), (what, got)
    assert torch.equal(dd["voxel_bound"].cpu(), fix["voxel_bound"]), what
    assert (dd["miss_ray_dir"].cpu() - fix["miss_ray_dir"]).abs().max().item() <= 2e-7, what
    pr, pv = dd["pair_ray"], dd["pair_vox"]
    P = pr.shape[0]
    assert P == fix["pair_pred_pos"].shape[0], what
    perm = to_reference_order(pr, pv)
    assert torch.equal(pv[perm].long().cpu(), fix["occ_vox_intersect_idx"].long()), what
    assert torch.equal(pr[perm].long().cpu(), fix["miss_ray_intersect_idx"].long()), what
    assert_f64_close("%s occ_voxel_feat" % what, dd["occ_voxel_feat"].cpu(), o64["occ_voxel_feat"],
                     fix["occ_voxel_feat"], report=report)
    for k in G14_PAIR_KEYS:
        assert_f64_close("%s %s" % (what, k), dd[k][perm].cpu().reshape(fix[k].shape), o64[k], fix[k], report=report)
    assert_f64_close("%s pred_pos" % what, dd["pred_pos"].cpu(), o64["pred_pos"], fix["pred_pos"], report=report)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(P, device=perm.device)
    gid = dd["max_pair_id"].long()
    gid_ref = torch.where(gid < P, inv[gid.clamp(max=P - 1)], torch.full_like(gid, P))
    assert torch.equal(gid_ref.cpu(), fix["max_pair_id"].long()), what


def _g14_stage2(what, dd, it, fix, o64, report):
    assert torch.equal(dd["end_voxel_id"].long().cpu(), fix["end_voxel_%d" % it].long()), (what, it)
    k = "pred_pos_refine_%d" % it
    assert_f64_close("%s %s" % (what, k), dd["pred_pos_refine"].cpu(), o64[k], fix[k], report=report)


def _g14_pairs_bit_equal(fix, cuda):
    """compute_ray_aabb on the reference's own ray directions: the pair lists and the t values bit for bit."""
    from implicit_depth_amd.query import compute_ray_aabb, to_reference_order
    off, pr, pv, pt = compute_ray_aabb(fix["miss_ray_dir"].to(cuda), fix["voxel_bound"].to(cuda),
                                       fix["miss_bid"].int().to(cuda), fix["occ_vox_bid"].int().to(cuda))
    perm = to_reference_order(pr, pv)
    assert torch.equal(pv[perm].long().cpu(), fix["occ_vox_intersect_idx"].long())
    assert torch.equal(pr[perm].long().cpu(), fix["miss_ray_intersect_idx"].long())
    assert torch.equal(pt[perm, 0].cpu(), fix["intersect_enter_dist"])
    assert torch.equal(pt[perm, 1].cpu(), fix["intersect_leave_dist"])


def _g14_stepwise(name, cuda, report):
    from implicit_depth_amd import pipeline as pl
    fix, o64, models, kw = _g14_setup(name, cuda)
    _g14_pairs_bit_equal(fix, cuda)
    batch, feat = _dev(fix["batch"], cuda), fix["full_rgb_feat"].to(cuda)
    pnet, prob, off, pnetr, offr = models
    first = None
    for it in (1, 2):
        opt = pl.LidfOptions(refine_forward_times=it, **kw)
        with torch.no_grad():
            ok, dd = pl.lidf_forward(batch, feat, pnet, prob, off, opt)
            assert ok
            pl.refine_forward(dd, pnetr, offr, opt)
        if first is None:
            first = dd
            _g14_stage1("g14 %s stepwise" % name, dd, fix, o64, report)
        _g14_stage2("g14 %s stepwise" % name, dd, it, fix, o64, report)
    return fix, o64, models, kw, batch, feat, first


def test_g14_a_stepwise(cuda):
    """Configuration A (every feature width other than shipped, roi_out_bbox 3, 'rel' positions in both stages, an
    'abs' refine PointNet) through pipeline.lidf_forward + refine_forward."""
    report = []
    _g14_stepwise("A", cuda, report)
    _show(report)


def test_g14_b_stepwise_and_frame(cuda):
    """Configuration B (decoders of gf_dim 128 / 128 / 32, shipped features) stepwise and through FrameRunner, which
    routes it to lidf_frame_widths_f32: eagerly and as a graph replay, both refine iterations."""
    from implicit_depth_amd import pipeline as pl
    report = []
    fix, o64, models, kw, batch, feat, step = _g14_stepwise("B", cuda, report)
    B, (h, w) = batch["rgb"].shape[0], fix["hw"]
    for it, graph in ((1, False), (2, False), (2, True)):
        opt = pl.LidfOptions(refine_forward_times=it, **kw)
        runner = pl.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], opt, models[3], models[4],
                                chain_route=False)
        assert runner.widths
        with torch.no_grad():
            runner.load(batch, feat)
            if graph:
                runner.capture()
            runner.run()
        ok, dd = runner.result()
        assert ok
        what = "g14 B frame %s" % ("graph" if graph else "eager")
        if it == 2:
            _g14_stage1(what, dd, fix, o64, report)
            for k in ("occ_voxel_feat", "pred_offset", "pred_prob_end", "pair_pred_pos", "pred_prob_end_softmax",
                      "pred_pos", "pair_t"):
                assert torch.equal(dd[k], step[k]), (what, k)        # the stepwise stage 1's bits
            for k in ("pair_ray", "pair_vox", "max_pair_id"):
                assert torch.equal(dd[k].long(), step[k].long()), (what, k)
        _g14_stage2(what, dd, it, fix, o64, report)
    _show(report)


# ------------------------------------------------------------------------------------------------------ g15 / g16
def _hold(got, fix, what, bad):
    """gw.close_rule (test_train_step_gpu.py::_close's rule: 2e-4 of the fixture tensor's own largest entry, no floor)
    for the tensors without a float64 twin on the fixture's inputs: the frozen stage 1 of a g16 step."""
    ok, err, scale = gw.close_rule(got, fix)
    print("  %-64s err %.3g scale %.3g err/scale %.3g" % (what, err, scale, err / scale if scale else float("inf")))
    if not ok:   # (collected, so that one run reports every tensor that misses)
        bad.append((what, err, scale))


def _train_modules(cfg, seeds, D, cuda):
    """Stage-1 and stage-2 modules of a g15 / g16 configuration in training mode (factor 1: g9's / g10's weights)."""
    from util import make_pointnet
    pnet_p, prob_p, off_p, pnetr_p, offr_p = gw.widths_params(cfg, seeds, (1.0,) * 5, D)
    stage1 = (make_pointnet(pnet_p, cuda, out=cfg["pnet_out"], gf=cfg["pnet_gf"]).train(),
              make_module("IMNET", prob_p, D[0], cuda, gf=cfg["gf"]).train(),
              make_module("IEF", off_p, D[0], cuda, n_iter=cfg["n_iter"], gf=cfg["gf"]).train())
    stage2 = (make_pointnet(pnetr_p, cuda, out=cfg["r_pnet_out"], gf=cfg["r_pnet_gf"]).train(),
              make_module("IEF", offr_p, D[1], cuda, n_iter=cfg["r_n_iter"], gf=cfg["r_gf"]).train())
    return stage1, stage2


def _param_grads(got, mods, names, stride):
    for mod, m in zip(names, mods):
        for k, p in m.named_parameters():
            got["g_%s.%s" % (mod, k)] = strided(p.grad.detach().cpu(), stride)


@pytest.mark.parametrize("name", ["e0", "e6_hn"])
def test_g15_train_step(cuda, name):
    """pipeline.lidf_forward_train at configuration A (generic.query_train: rgb_out 16, roi_out_bbox 3, pnet_out 64,
    gf 32, 'rel' positions) against the reference's own LIDF.forward(batch, 'train', epoch) + backward: the float64
    stage-1 composite on the fixture's inputs (gw.stage1_twin, held to the fixture on the CPU) is the centre, the
    reference's float32 run the unit."""
    import numpy as np
    import train_loss_ref as tl
    from implicit_depth_amd import LidfLossOptions, LidfOptions, lidf_forward_train
    from implicit_depth_amd.query import to_reference_order
    from test_golden_widths import g15_files, g15_step
    g, gp = g15_files()
    cfg = gw.G14["A"]
    fix, t64, _ = g15_step(name)
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    batch, feat = tl.g9_batch(g)
    batch, feat = _dev(batch, cuda), feat.to(cuda).requires_grad_(True)
    sp, so, sn = (int(v) for v in g["seeds"])
    mods, _ = _train_modules(cfg, (sp, so, sn, 31, 43), gw.widths_D(cfg), cuda)
    np.random.seed(int(g["np_seed"]))   # (sample_miss_rays draws the window as the reference does)
    ok, dd, loss = lidf_forward_train(
        batch, feat, *mods, opt=LidfOptions(miss_sample_num=int(g["miss_sample_num"]), roi_out_bbox=cfg["roi_out"],
                                            intersect_pos_type="rel"),
        loss_opt=LidfLossOptions(**opt), epoch=epoch)
    assert ok
    dd["pred_pos"].retain_grad(), dd["pred_prob_end"].retain_grad()
    loss["loss_net"].backward()
    assert torch.equal(dd["miss_bid"].cpu(), d["miss_bid"]) and torch.equal(dd["miss_flat_img_id"].cpu(), d["miss_flat"])
    P = d["pair_ray"].shape[0]
    perm = to_reference_order(dd["pair_ray"], dd["pair_vox"])
    assert torch.equal(dd["pair_ray"][perm].long().cpu(), d["pair_ray"]) and torch.equal(dd["pair_vox"][perm].long().cpu(),
                                                                                        d["pair_vox"])
    assert torch.equal(dd["gt_pos"].cpu(), d["gt_pos"])
    assert torch.equal(dd["pcl_label"][perm].long().cpu(), d["pcl_label"].long())
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(P, device=perm.device)
    gid = dd["max_pair_id"].long()
    assert torch.equal(torch.where(gid < P, inv[gid.clamp(max=P - 1)], torch.full_like(gid, P)).cpu(), d["max_pair_id"])
    assert tuple(loss) == tl.LOSS_KEYS
    got = {"pred_pos": dd["pred_pos"], "pred_prob_end": dd["pred_prob_end"][perm], "g_pred_pos": dd["pred_pos"].grad,
           "g_pred_prob_end": dd["pred_prob_end"].grad[perm], "g_full_rgb_feat": feat.grad}
    got.update({"loss:" + k: loss[k].reshape(1) for k in tl.LOSS_KEYS})
    _param_grads(got, mods, ("pnet_model", "prob_dec", "offset_dec"), int(g["param_stride"]))
    assert set(got) == set(fix)
    report = []
    gw.hold_step("g15 %s" % name, got, t64, fix, pairs=P, report=report)
    assert len(report) == len(fix) - 1
    _show(report)


@pytest.mark.parametrize("cfg_name,name,factorised", [("A", "plain", None), ("A", "hn", None), ("B", "plain", None),
                                                      ("B", "plain", True)])
def test_g16_refine_train_step(cuda, monkeypatch, cfg_name, name, factorised):
    """pipeline.train_refine_step against the reference's stage-2 iteration: at A through generic.refine_train (the
    only route there), at B through the composed route and through generic.refine_train (factorised=True). Stage 2 is
    held to the float64 refine chain on the fixture's inputs (gw.stage2_twin, held to the fixture on the CPU) with the
    reference's float32 run as the unit; the frozen stage 1, which only feeds it, by gw.close_rule."""
    import functools
    import numpy as np
    import refine_loss_ref as rl
    import train_loss_ref as tl
    from implicit_depth_amd import LidfLossOptions, LidfOptions, query as Q, train_refine_step
    from test_golden_widths import g16_files, g16_step
    g, gp = g16_files(cfg_name)
    cfg = gw.G14[cfg_name]
    fix, t64, _ = g16_step(cfg_name, name)
    d, ref = rl.g10_case(g, name)
    batch, feat = rl.g10_batch(g)
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    seeds = tuple(int(v) for v in g["seeds_stage1"]) + tuple(int(v) for v in g["seeds_refine"])
    mods, mods_r = _train_modules(cfg, seeds, gw.widths_D(cfg), cuda)
    opt = LidfOptions(miss_sample_num=int(g["miss_sample_num"]), maxpool_label_epo=0, roi_out_bbox=cfg["roi_out"],
                      intersect_pos_type="rel" if cfg["pos_rel"] else "abs",
                      refine_intersect_pos_type="rel" if cfg["r_pos_rel"] else "abs",
                      refine_pnet_pos_type="rel" if cfg["r_pnet_pos_rel"] else "abs")
    loss_opt = LidfLossOptions(prob_w=0.0, **rl.G10_CASES[name])   # (train_refine.yaml: one loss section, prob_w 0)
    if factorised is not None:
        monkeypatch.setattr(Q, "lidf_refine_train", functools.partial(Q.lidf_refine_train, factorised=factorised))
    np.random.seed(ref["np_seed"])
    ok, dd, loss1, loss = train_refine_step(batch, feat, *mods, *mods_r, opt=opt, loss_opt=loss_opt,
                                            epoch=int(g["epoch"]))
    assert ok
    dd["pred_pos_refine"].retain_grad()
    loss["loss_net"].backward()
    what = "g16 %s %s%s" % (cfg_name, name, "" if factorised is None else " factorised")
    assert torch.equal(dd["miss_bid"].cpu(), d["miss_bid"]) and torch.equal(dd["miss_flat_img_id"].cpu(), d["miss_flat"])
    assert dd["pair_ray"].shape[0] == d["pair_ray"].shape[0]
    assert dd["refine_perturb_noise"] == ref["noise"]   # the same draw, bit for bit
    assert torch.equal(dd["end_voxel_id"].cpu().long(), ref["end_voxel_id"])
    bad = []
    _hold(dd["pred_pos"], d["pred_pos"], what + " stage 1 pred_pos", bad)
    for i, k in enumerate(tl.LOSS_KEYS):
        _hold(loss1[k], ref["loss_stage1"][i], "%s stage 1 %s" % (what, k), bad)
    assert not bad, bad
    assert tuple(loss) == rl.REFINE_LOSS_KEYS
    got = {"pred_pos_refine": dd["pred_pos_refine"], "g_pred_pos_refine": dd["pred_pos_refine"].grad}
    got.update({"loss:" + k: loss[k].reshape(1) for k in rl.REFINE_LOSS_KEYS})
    _param_grads(got, mods_r, rl.G10_MODULES, int(g["param_stride"]))
    assert set(got) == set(fix)
    report = []
    gw.hold_step(what, got, t64, fix, report=report)
    assert len(report) == len(fix)
    _show(report)
    assert all(p.grad is None for m in mods for p in m.parameters())   # stage 1 is frozen
