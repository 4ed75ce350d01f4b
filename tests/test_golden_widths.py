"""CPU: the oracle against the fixtures generated from the reference AT OTHER WIDTHS (tests/golden/make_golden_widths.py),
and a proof that the comparisons the GPU tests make with those fixtures bite.

Oracle against fixture: assert_f64_close(fixture, oracle float64, oracle float32) — the unit is the oracle's own
float32-against-float64 rounding, which a structural disagreement with the reference cannot inflate. That is the guard
for tests/test_golden_widths_gpu.py, which turns the roles round: there the fixture (the reference's own float32 run)
is the unit, and the float64 oracle on the fixture's inputs the centre.

The pins bite: every fixture tensor replaced by zeros, by its mean over rows, and by itself with two rows exchanged is
rejected by the comparison the GPU test applies to it (g2_decoders.npz and the g5 files included, under the comparisons
test_golden_gpu.py gained with this module). The float64 twins of the two training steps and the comparison helpers
shared with the GPU tests live in tests/golden_widths_ref.py."""
import functools

import numpy as np
import pytest
import torch

import golden_widths_ref as gw
from golden_widths_ref import G14, g2_close, g2_oracle, g5_close, g5_oracle, strided, widths_params  # noqa: F401
from test_oracle_golden import load
from util import TOL, assert_f64_close, closed_form, closed_form_params, inv_out_act, k_for, oracle_grads, orc

# kind, inp_dim, gf_dim, n_iter, use_sigmoid (make_golden_widths.G13_CASES)
G13_CASES = (("IMNET", 385, 32, 1, False), ("IMNET", 385, 128, 1, False), ("IEF", 385, 32, 3, False),
             ("IEF", 334, 128, 2, False), ("IEF", 337, 32, 2, True))
G13_KEYS = tuple("%s_%d_%d_%d_%d" % (k, d, gf, n, int(s)) for k, d, gf, n, s in G13_CASES)


@functools.lru_cache(maxsize=None)
def g13_case(key):
    """One g13 case: its settings, the regenerated inputs, the fixture's tensors and the oracle's float64 / float32
    output and gradients on the same inputs (computed once, shared by every test that needs them; read-only)."""
    kind, d, gf, n_iter, sig = G13_CASES[G13_KEYS.index(key)]
    g = load("g13_decoders_widths_%s.npz" % key)
    rows, stride = int(g[key + "_rows"]), int(g[key + "_param_stride"])
    p = closed_form_params(kind, d, seed=int(g[key + "_seed"]), gf=gf, factor=float(g[key + "_factor"]))
    x = closed_form((rows, d), 0.5698402910, 0.1 * d, 1.0)
    wgt = closed_form((rows, 1), 0.7390851332, 0.37, 1.0)
    c = dict(key=key, kind=kind, d=d, gf=gf, n_iter=n_iter, sig=sig, p=p, x=x, wgt=wgt, stride=stride,
             fix={k[len(key) + 1:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(key + "_")})
    for name, dt in (("o64", torch.float64), ("o32", torch.float32)):
        y, grads = oracle_grads(p, x, kind, wgt[:, 0], dt, n_iter, sig)
        c[name] = {"y": y}
        c[name]["g_input"] = grads.pop("input")
        for k, v in grads.items():
            c[name]["g_" + k] = v
    return c


def g13_tensors(c):
    """(name, fixture, oracle64, oracle32, k, through) for every float tensor of a g13 case, in the form the fixture
    stores it. through: the map both sides go through before they are compared (the clamp's inverse for the output of a
    decoder without a sigmoid: outside [0, 1] the clamp divides a logit's error by 100)."""
    ident = (lambda t: t)
    for name in sorted(c["o64"]):
        if name == "y":
            yield name, c["fix"]["y"], c["o64"]["y"], c["o32"]["y"], 4.0, (ident if c["sig"] else inv_out_act)
        elif name == "g_input":
            yield name, c["fix"][name], c["o64"][name], c["o32"][name], 4.0, ident
        else:
            yield (name, c["fix"][name], strided(c["o64"][name], c["stride"]), strided(c["o32"][name], c["stride"]),
                   k_for(name[2:]), ident)


def variants(t):
    """The three altered tensors a comparison must reject: zeros, the mean over rows (over all entries of a vector),
    two rows exchanged (the rows holding the largest and the smallest entry of one column)."""
    t = t.clone()
    if t.shape[0] < 2:   # (a one-element gradient, linear_4.bias: it is its own mean and has no second row)
        return (("zeros", torch.zeros_like(t)),)
    flat = t.reshape(t.shape[0], -1)
    col = int((flat.max(0)[0] - flat.min(0)[0]).argmax())   # (the column with the widest spread: a ReLU's may be all 0)
    i, j = int(flat[:, col].argmax()), int(flat[:, col].argmin())
    assert i != j and not torch.equal(t[i], t[j])
    swapped = t.clone()
    swapped[i], swapped[j] = t[j], t[i]
    return (("zeros", torch.zeros_like(t)), ("row mean", t.double().mean(0, keepdim=True).expand_as(t).to(t.dtype).clone()),
            ("rows exchanged", swapped))


def rejects(what, got, ref64, unit, k, through=lambda t: t):
    """True if the GPU tests' comparison (the fixture as the unit) refuses `got`."""
    try:
        assert_f64_close(what, through(got), through(ref64), through(unit), k=k)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------- g13
@pytest.mark.parametrize("key", G13_KEYS)
def test_g13_oracle_matches_reference_modules(key):
    c = g13_case(key)
    assert set(c["fix"]) - {"seed", "factor", "rows", "param_stride"} == set(c["o64"])
    report = []
    for name, fix, o64, o32, k, through in g13_tensors(c):
        assert_f64_close("%s %s" % (key, name), through(fix), through(o64), through(o32), k=k, report=report)
        if through is inv_out_act:   # and as stored
            assert_f64_close("%s %s (clamped)" % (key, name), fix, o64, o32, k=k, report=report)
    assert len(report) >= 10


@pytest.mark.parametrize("key", G13_KEYS)
def test_g13_conditions_hold(key):
    """What the generator asserted, re-read from the float64 oracle: no hidden pre-activation within 2e-5 of 0, at
    least 25 % of every hidden layer on each side of its kink, and (no sigmoid) at least 10 % of the rows on each of the
    clamp's three branches with no argument within 2e-5 of 0 or 1."""
    c = g13_case(key)
    zs = []
    with torch.no_grad():
        orc.decoder_forward({k: v.double() for k, v in c["p"].items()}, c["x"].double(), c["kind"], c["n_iter"],
                            c["sig"], preacts=zs)
    assert len(zs) == 3 * c["n_iter"] + 1
    for z in zs[:-1]:
        assert z.abs().min().item() > 2e-5
        assert 0.25 <= (z > 0).double().mean().item() <= 0.75
    if not c["sig"]:
        a = zs[-1][:, 0]
        n = a.shape[0]
        assert min(int((a < 0).sum()), int(((a >= 0) & (a <= 1)).sum()), int((a > 1).sum())) >= 0.1 * n
        assert min(a.abs().min().item(), (a - 1).abs().min().item()) > 2e-5


@pytest.mark.parametrize("key", G13_KEYS)
def test_g13_pins_bite(key):
    c = g13_case(key)
    n = 0
    for name, fix, o64, _, k, through in g13_tensors(c):
        assert not rejects("%s %s itself" % (key, name), fix, o64, fix, k, through)
        for vname, v in variants(fix):
            assert rejects("%s %s <- %s" % (key, name, vname), v, o64, fix, k, through), (key, name, vname)
            n += 1
    assert n >= 28


# ------------------------------------------------------------------------- g2 / g5 under the strengthened comparison
def _raises(fn, *a):
    try:
        fn(*a)
    except AssertionError:
        return True
    return False


def test_g2_g5_pins_bite_and_the_old_tolerances_did_not():
    """Under the added comparisons every altered tensor is refused. The absolute 1e-4 of g2 and the
    2e-4 max(1, max|ref|) of g5 accepted some of them: with closed_form_params at amplitude 0.14 every g2 row sits on
    the clamp's y < 0 branch (output = 0.01 x logit, whole tensors below 1e-3), and several g5 gradients are smaller
    than the floor of 2e-4."""
    old_accepted = []
    for key, (fix, y64, sig) in g2_oracle().items():
        g2_close(key, fix, fix, y64, sig)
        for vname, v in variants(fix):
            assert _raises(g2_close, key, v, fix, y64, sig), (key, vname)
            if (v - fix).abs().max().item() <= TOL:
                old_accepted.append(("g2", key, vname))
    for key, case in g5_oracle().items():
        sig = key.endswith("_1")
        for name, (fix, o64) in case.items():
            g5_close(key, name, fix, fix, o64, sig)
            for vname, v in variants(fix):
                assert _raises(g5_close, key, name, v, fix, o64, sig), (key, name, vname)
                old = TOL if name == "y" else 2e-4 * max(1.0, fix.abs().max().item())
                if (v - fix).abs().max().item() <= old:
                    old_accepted.append(("g5", key, name, vname))
    print("altered tensors the old tolerances accepted:", old_accepted)
    assert ("g2", "IMNET_265_0", "row mean") in old_accepted
    assert ("g5", "IEF_334_3_1", "g_offset_enc.weight", "zeros") in old_accepted


# ------------------------------------------------------------------------------------------------------------- g14
G14_INT_KEYS = ("revidx", "valid_v_pid", "occ_vox_bid", "occ_vox_global_coord", "miss_bid", "miss_flat_img_id",
                "miss_img_ind", "occ_vox_intersect_idx", "miss_ray_intersect_idx", "max_pair_id", "end_voxel_1",
                "end_voxel_2")
G14_PAIR_KEYS = ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_prob_end_softmax")
G14_FLOAT_KEYS = ("occ_voxel_feat",) + G14_PAIR_KEYS + ("pred_pos", "occ_voxel_feat_refine_1", "pred_pos_refine_1",
                                                         "occ_voxel_feat_refine_2", "pred_pos_refine_2")


def g14_batch(g):
    b = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("batch_")}
    intr = torch.from_numpy(g["intr"]).double()
    b.update(fx=intr[:, 0], fy=intr[:, 1], cx=intr[:, 2], cy=intr[:, 3])
    return b


@functools.lru_cache(maxsize=None)
def g14_fixture(name):
    g = load("g14_widths_eval.npz")
    fix = {k[len(name) + 1:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith(name + "_")}
    fix["hw"] = tuple(int(v) for v in g["hw"])
    fix["batch"] = g14_batch(g)
    return fix


@functools.lru_cache(maxsize=None)
def g14_oracle(name, double):
    """The oracle chain on a g14 configuration's inputs, in float64 or float32: the occupied voxels, the pair lists,
    the PointNet, the query and two refine steps. Per-pair tensors in the fixture's (voxel-major) order. The float32
    run pools the ROI features with the oracle's numpy loop (what the generator's stub ran), the float64 run with its
    float64 twin (tests/roi_ref.py)."""
    import contextlib
    import roi_ref
    cfg, fix = G14[name], g14_fixture(name)
    dt = torch.float64 if double else torch.float32
    c = (lambda t: t.to(dt))
    b = fix["batch"]
    bs, (h, w) = b["rgb"].shape[0], fix["hw"]
    valid_mask = 1 - (b["depth_corrupt"] == 0).squeeze(1).float()
    vidx = torch.nonzero(valid_mask.reshape(bs, -1), as_tuple=False)
    valid_xyz = b["xyz_corrupt"].permute(0, 2, 3, 1).reshape(bs, -1, 3)[vidx[:, 0], vidx[:, 1]]
    valid_rgb = b["rgb"].permute(0, 2, 3, 1).reshape(bs, -1, 3)[vidx[:, 0], vidx[:, 1]]
    occ = orc.occupied_voxels(valid_xyz, vidx[:, 0])
    intr = b["fx"].float(), b["fy"].float(), b["cx"].float(), b["cy"].float()
    mr = orc.get_miss_ray(torch.ones(bs, h, w), *intr)
    mask, dist = orc.ray_aabb(mr["miss_ray_dir"].numpy(), occ["voxel_bound"].numpy(), mr["miss_bid"].numpy(),
                              occ["occ_vox_bid"].numpy())
    pair_ray, pair_vox, pair_t, pair_off = orc.pairs_from_dense(mask, dist)
    R, P, V = mr["miss_ray_dir"].shape[0], pair_ray.shape[0], occ["voxel_bound"].shape[0]
    perm = torch.argsort(pair_vox * R + pair_ray, stable=True)
    pnet_p, prob_p, off_p, pnetr_p, offr_p = (
        {k: c(v) for k, v in p.items()} for p in widths_params(cfg, fix["seeds"], fix["factors"], fix["D"]))
    out = {"ints": {"revidx": occ["revidx"], "valid_v_pid": occ["valid_v_pid"], "occ_vox_bid": occ["occ_vox_bid"],
                    "occ_vox_global_coord": occ["occ_vox_global_coord"], "miss_bid": mr["miss_bid"],
                    "miss_flat_img_id": mr["miss_flat_img_id"], "miss_img_ind": mr["miss_img_ind"],
                    "occ_vox_intersect_idx": pair_vox[perm], "miss_ray_intersect_idx": pair_ray[perm]},
           "exact": {"valid_xyz": valid_xyz, "valid_v_rel_coord": occ["valid_v_rel_coord"], "xmin": occ["xmin"],
                     "voxel_bound": occ["voxel_bound"], "miss_ray_dir": mr["miss_ray_dir"],
                     "intersect_enter_dist": pair_t[perm, 0], "intersect_leave_dist": pair_t[perm, 1]},
           "perm": perm, "pairs": (pair_ray, pair_vox, pair_t, pair_off), "rays": mr, "occ": occ}
    pnet_inp = torch.cat((occ["valid_v_rel_coord"], valid_rgb[occ["valid_v_pid"]]), -1)
    out["occ_voxel_feat"] = orc.pointnet2stage(pnet_p, c(pnet_inp), occ["revidx"], V)
    vb = occ["voxel_bound"]
    feat = c(fix["full_rgb_feat"])
    with (roi_ref.patched(orc) if double else contextlib.nullcontext()):
        res = orc.query(c(mr["miss_ray_dir"]), mr["miss_img_ind"], mr["miss_bid"], pair_ray, pair_vox, c(pair_t),
                        pair_off, feat, out["occ_voxel_feat"], prob_p, off_p, off_kind="IEF", n_iter=cfg["n_iter"],
                        offset_range=tuple(float(v) for v in fix["offset_range"]), part_size=float(fix["part_size"]),
                        vox_center=c((vb[:, :3] + vb[:, 3:]) / 2.0) if cfg["pos_rel"] else None,
                        pos_rel=cfg["pos_rel"], roi_out_bbox=cfg["roi_out"])
    for k in G14_PAIR_KEYS:
        out[k] = res[k][perm]
    out["pred_pos"], out["ray_rgb"] = res["pred_pos"], res["ray_rgb"]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(P)
    mid = res["max_pair_id"]
    out["ints"]["max_pair_id"] = torch.where(mid < P, inv[mid.clamp(max=P - 1)], torch.full_like(mid, P))
    valid_inp = pnet_inp if cfg["r_pnet_pos_rel"] else torch.cat((valid_xyz[occ["valid_v_pid"]], pnet_inp[:, 3:]), -1)
    out["exact"]["refine_valid_inp"] = valid_inp
    pos = res["pred_pos"]
    for it in (1, 2):
        pos, ev, vfeat = orc.refine_step(
            pos, c(mr["miss_ray_dir"]), mr["miss_img_ind"], mr["miss_bid"], mr["miss_flat_img_id"], mid, pair_vox, vb,
            occ["occ_vox_bid"], c(b["rgb"]), feat, c(valid_inp), occ["revidx"], pnetr_p, offr_p, n_iter=cfg["r_n_iter"],
            offset_range=tuple(float(v) for v in fix["refine_offset_range"]), pos_rel=cfg["r_pos_rel"],
            pnet_pos_rel=cfg["r_pnet_pos_rel"], ray_rgb=res["ray_rgb"])
        out["pred_pos_refine_%d" % it], out["occ_voxel_feat_refine_%d" % it] = pos, vfeat
        out["ints"]["end_voxel_%d" % it] = ev
    return out


@pytest.mark.parametrize("name", sorted(G14))
def test_g14_oracle_matches_reference_trace(name):
    fix, o64, o32 = g14_fixture(name), g14_oracle(name, True), g14_oracle(name, False)
    for k in G14_INT_KEYS:   # (a key missing on either side raises)
        assert torch.equal(o32["ints"][k].long(), fix[k].long()), k
    assert torch.equal(o64["ints"]["max_pair_id"], o32["ints"]["max_pair_id"])
    for it in (1, 2):   # (the fixture's conditions keep every end voxel out of rounding's reach)
        assert torch.equal(o64["ints"]["end_voxel_%d" % it], o32["ints"]["end_voxel_%d" % it])
    for k, v in o32["exact"].items():
        assert torch.equal(v, fix[k]), k
    assert float(fix["min_logit_gap"]) > 1e-4 and float(fix["min_face_distance"]) > 2e-4
    report = []
    for k in G14_FLOAT_KEYS:
        assert_f64_close("g14 %s %s" % (name, k), fix[k], o64[k], o32[k], report=report)
    print("g14 %s: largest ratio %.2f elementwise / %.2f normwise" % (
        name, max(r["ratio_max"] for r in report), max(r["ratio_nrm"] for r in report)))


@pytest.mark.parametrize("name", sorted(G14))
def test_g14_pins_bite(name):
    fix, o64 = g14_fixture(name), g14_oracle(name, True)
    for k in G14_FLOAT_KEYS:
        assert not rejects("g14 %s %s itself" % (name, k), fix[k], o64[k], fix[k], 4.0)
        for vname, v in variants(fix[k]):
            assert rejects("g14 %s %s <- %s" % (name, k, vname), v, o64[k], fix[k], 4.0), (name, k, vname)


# ------------------------------------------------------------------------------------------------------ g15 / g16
G15_CASES = ("e0", "e6_hn")
G16_CASES = (("A", "plain"), ("A", "hn"), ("B", "plain"))




@functools.lru_cache(maxsize=None)
def g15_files():
    return load("g15_train_widths.npz"), load("g15_train_widths_params.npz")


@functools.lru_cache(maxsize=None)
def g16_files(cfg):
    """Configuration cfg's part of the g16 files, under g10's key names."""
    cut = lambda g: {k[2:]: v for k, v in g.items() if k.startswith(cfg + "_")}  # noqa: E731
    return cut(load("g16_refine_train_widths.npz")), cut(load("g16_refine_train_widths_params.npz"))


@pytest.mark.parametrize("name", G15_CASES)
def test_g15_labels_and_loss_twin_match_the_reference(name):
    """tests/train_loss_ref.py (compute_gt and the loss, the float64 twin the GPU loss tests rest on) on the
    reference's own predictions at configuration A: labels equal, its float32 losses and gradients held to the
    reference's by its own float32-against-float64 rounding."""
    import train_loss_ref as tl
    g, _ = g15_files()
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    gt_pos, label, want = tl.compute_gt_ref(d["xyz_flat"], d["miss_bid"], d["miss_flat"], d["voxel_bound"],
                                            d["pair_ray"], d["pair_vox"])
    assert torch.equal(gt_pos, d["gt_pos"]) and torch.equal(label.long(), d["pcl_label"].long())
    if epoch < 6:
        assert torch.equal(want, d["max_pair_id"])
    l64, gp64, gl64 = tl.loss_and_grads(d, torch.float64, epoch, **opt)
    l32, gp32, gl32 = tl.loss_and_grads(d, torch.float32, epoch, **opt)
    for i, k in enumerate(tl.LOSS_KEYS):
        assert_f64_close("g15 %s %s" % (name, k), ref["loss"][i].reshape(1), l64[i].reshape(1), l32[i].reshape(1))
    assert_f64_close("g15 %s g_pred_pos" % name, ref["g_pred_pos"], gp64, gp32)
    assert_f64_close("g15 %s g_pred_prob_end" % name, ref["g_pred_prob_end"], gl64, gl32)


@pytest.mark.parametrize("cfg,name", G16_CASES)
def test_g16_loss_twin_matches_the_reference(cfg, name):
    """tests/refine_loss_ref.py on the reference's own pred_pos_refine at configurations A and B."""
    import refine_loss_ref as rl
    g, _ = g16_files(cfg)
    d, ref = rl.g10_case(g, name)
    l64, g64 = rl.loss_and_grad(d, torch.float64, int(g["epoch"]), **rl.G10_CASES[name])
    l32, g32 = rl.loss_and_grad(d, torch.float32, int(g["epoch"]), **rl.G10_CASES[name])
    for i, k in enumerate(rl.REFINE_LOSS_KEYS):
        assert_f64_close("g16 %s %s %s" % (cfg, name, k), ref["loss"][i].reshape(1), l64[i].reshape(1),
                         l32[i].reshape(1))
    assert_f64_close("g16 %s %s g_pred_pos_refine" % (cfg, name), ref["g_pred_pos_refine"], g64, g32)



STAGE1_KEYS = ("pred_pos", "pred_prob_end", "loss", "g_pred_pos", "g_pred_prob_end", "g_full_rgb_feat")
STAGE2_KEYS = ("pred_pos_refine", "loss", "g_pred_pos_refine")


def g15_step(name):
    """(fixture tensors in hold_step's form, float64 twin, float32 twin) of one g15 case."""
    g, gp = g15_files()
    stride = int(g["param_stride"])
    return (gw.step_form(gw.fixture_tensors(g, gp, name, STAGE1_KEYS), tl_keys=True),
            gw.step_form(gw.twin_in_fixture_form(gw.stage1_twin(name, True), stride), tl_keys=True),
            gw.step_form(gw.twin_in_fixture_form(gw.stage1_twin(name, False), stride), tl_keys=True))


def g16_step(cfg, name):
    g, gp = g16_files(cfg)
    stride = int(g["param_stride"])
    return (gw.step_form(gw.fixture_tensors(g, gp, name, STAGE2_KEYS), tl_keys=False),
            gw.step_form(gw.twin_in_fixture_form(gw.stage2_twin(cfg, name, True), stride), tl_keys=False),
            gw.step_form(gw.twin_in_fixture_form(gw.stage2_twin(cfg, name, False), stride), tl_keys=False))


@pytest.mark.parametrize("name", G15_CASES)
def test_g15_stage1_composite_twin_matches_the_reference(name):
    """The stage-1 composite that tests/test_train_widths_gpu.py rests on (its _oracle: orc.query with the
    differentiable RoIAlign) behind orc.pointnet2stage and in front of train_loss_ref, on the g15 inputs at A: the pair
    lists, labels and max_pair_id it derives equal the reference's (asserted inside), and its float32 pred_pos,
    pred_prob_end, eight losses, g_pred_pos, g_pred_prob_end, g_full_rgb_feat and every (strided) parameter gradient
    are held to the reference's by its own float32-against-float64 rounding."""
    fix, t64, t32 = g15_step(name)
    assert set(fix) == set(t64) == set(t32)
    report = []
    gw.hold_step("g15 %s twin" % name, fix, t64, t32, pairs=fix["pred_prob_end"].shape[0], report=report)
    assert len(report) == len(fix) - 1        # (prob_dec's last bias goes by its bound)
    print("g15 %s: largest ratio %.2f elementwise / %.2f normwise" % (
        name, max(r["ratio_max"] for r in report), max(r["ratio_nrm"] for r in report)))


@pytest.mark.parametrize("cfg,name", G16_CASES)
def test_g16_refine_chain_twin_matches_the_reference(cfg, name):
    """refine_widths_ref.chain (what tests/test_refine_widths_gpu.py rests on) in front of refine_loss_ref on the g16
    inputs at A and B, started from the reference's stage-1 pred_pos and max_pair_id: end voxels equal, pred_pos_refine,
    the six losses, g_pred_pos_refine and every (strided) parameter gradient held to the reference's."""
    g, _ = g16_files(cfg)
    fix, t64, t32 = g16_step(cfg, name)
    assert set(fix) == set(t64) - {"end_voxel_id"}
    for t in (t64, t32):
        assert torch.equal(t["end_voxel_id"], torch.from_numpy(g[name + "_end_voxel_id"]))
    report = []
    gw.hold_step("g16 %s %s twin" % (cfg, name), fix, t64, t32, report=report)
    assert len(report) == len(fix)
    print("g16 %s %s: largest ratio %.2f elementwise / %.2f normwise" % (
        cfg, name, max(r["ratio_max"] for r in report), max(r["ratio_nrm"] for r in report)))


def test_g15_g16_pins_bite():
    """gw.hold_one — the comparison the GPU tests of the two training steps call, with the float64 twin as the centre
    and the fixture as the unit — refuses the three altered forms of every stored prediction, loss and gradient
    (prob_dec's last bias aside: its true value is 0, tests/test_train_step_gpu.py::_zero_bias_bound); gw.close_rule,
    which holds the frozen stage 1 of a g16 step, refuses them for its tensors."""
    n = 0
    for fix, t64, _ in [g15_step(name) for name in G15_CASES] + [g16_step(cfg, name) for cfg, name in G16_CASES]:
        for k, f in fix.items():
            if k == gw.ZERO_BIAS or float(f.abs().max()) == 0.0:
                continue
            gw.hold_one("itself", k, f, t64[k], f)
            for vname, v in variants(f):
                assert _raises(gw.hold_one, vname, k, v, t64[k], f), (k, vname)
                n += 1
    assert n > 300
    for cfg, name in G16_CASES:
        g, _ = g16_files(cfg)
        for k in ("pred_pos", "loss_stage1"):
            f = torch.from_numpy(g["%s_%s" % (name, k)])
            assert gw.close_rule(f, f)[0]
            for vname, v in variants(f.reshape(-1, 1) if f.dim() == 1 else f):
                assert not gw.close_rule(v.reshape(f.shape), f)[0], (cfg, name, k, vname)
