"""GPU: the ordered RoIAlign adjoint (lidf_ray_features_backward_ordered_f32, roi_backward="ordered").

Every case is torch.equal to the numpy twin of its summation order (roi_backward_ref.py) and to a second run, and is
held to float64 (autograd of the oracle's RoIAlign in torch ops) with the default route's own error as the unit
(util.assert_f64_close, F64_K): the ordered route may be no less accurate than the route it stands in for."""
import numpy as np
import pytest
import torch

import roi_backward_ref as rb
from util import F64_K, assert_f64_close, make_module, make_pointnet

pytestmark = pytest.mark.gpu

LV = 4                      # multires_views: rows of 128 + 27 columns
LD = 128 + 3 + 6 * LV


def _adjoint(entry, g, pix, bid, B, H, W, bbox, dev, poison=False, ws_bytes=None):
    """One call of `entry` ('ordered' or 'atomic') on device tensors, with the whole workspace."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    need = L.lidf_ray_features_backward_ordered_workspace_bytes(B, H, W)
    assert need == B * 129 * H * W * 4
    fn = L.lidf_ray_features_backward_ordered_f32 if entry == "ordered" else L.lidf_ray_features_backward_f32
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF if poison else 0)                         # 0xFFFFFFFF: a NaN as float, -1 as a ray count
    out = torch.full((B, 32, H, W), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(fn(_lib.ptr(g) if g.numel() else None, _lib.ptr(pix) if pix.numel() else None,
                      _lib.ptr(bid) if bid.numel() else None, pix.shape[0], B, H, W, bbox, LV, _lib.ptr(out),
                      _lib.ptr(ws), need, _lib.current_stream(dev)))
    return out


def _check(what, g, pix, bid, B, H, W, bbox, dev, poison=False):
    """twin, second run, and the float64 criterion against the default route; returns the ordered result."""
    gd = torch.from_numpy(g).to(dev)
    pd, bd = torch.from_numpy(pix).to(dev).contiguous(), torch.from_numpy(bid).to(dev).contiguous()
    got = _adjoint("ordered", gd, pd, bd, B, H, W, bbox, dev, poison)
    again = _adjoint("ordered", gd, pd, bd, B, H, W, bbox, dev, poison)
    default = _adjoint("atomic", gd, pd, bd, B, H, W, bbox, dev)
    twin = torch.from_numpy(rb.roi_backward_ordered(g, pix, bid, B, H, W, bbox))
    got_c = got.cpu()
    assert bool(torch.isfinite(got_c).all()), what          # every element written, nothing of the workspace read
    differ = (got_c != twin).nonzero()
    assert torch.equal(got_c, twin), (what, "twin", differ.shape[0], differ[:4].tolist())
    assert torch.equal(got, again), (what, "second run")
    r64 = rb.torch_adjoint(g, pix, bid, B, H, W, bbox, torch.float64)
    assert_f64_close(what, got_c, r64, default.cpu(), k=F64_K)
    return got


def _grad_rows(R, seed):
    return np.random.default_rng(seed).standard_normal((R, LD)).astype(np.float32)


# every box clamped on both sides; the smallest image the ring path of the default route takes; last tiles 2 and 3
# pixels wide; several tiles a side with partial last tiles
@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (2, 9, 9), (1, 18, 35), (3, 37, 53)])
def test_every_pixel_a_ray(cuda, B, H, W):
    pix, bid = rb.pixel_rays(B, H, W)
    _check("%dx%dx%d" % (B, H, W), _grad_rows(pix.shape[0], 21), pix, bid, B, H, W, 8, cuda)


def _sparse(name):
    B, H, W = 2, 24, 32
    if name == "corners+interior":
        pts = [(0, 0, 0), (0, 31, 0), (1, 0, 23), (1, 31, 23), (0, 17, 11)]       # (frame, x, y)
    elif name == "border_row":
        pts = [(0, x, 0) for x in range(W)]
    elif name == "frame1_only":
        pts = [(1, x, y) for y in range(0, H, 3) for x in range(0, W, 2)]
    else:
        pts = []
    a = np.array(pts, dtype=np.int32).reshape(-1, 3)
    return B, H, W, np.ascontiguousarray(a[:, 1:3]), np.ascontiguousarray(a[:, 0])


@pytest.mark.parametrize("name", ["corners+interior", "border_row", "frame1_only", "empty"])
def test_sparse_ray_sets(cuda, name):
    B, H, W, pix, bid = _sparse(name)
    got = _check(name, _grad_rows(pix.shape[0], 22), pix, bid, B, H, W, 8, cuda, poison=(name == "empty"))
    if name == "empty":
        assert not bool(got.any())                           # R = 0 writes zeros
    if name == "frame1_only":
        assert not bool(got[0].any()) and bool(got[1].any())


@pytest.mark.parametrize("bbox", [2, 6, 8])
def test_roi_inp_bbox(cuda, bbox):
    B, H, W = 2, 19, 23
    pix, bid = rb.pixel_rays(B, H, W)
    _check("bbox %d" % bbox, _grad_rows(pix.shape[0], 23), pix, bid, B, H, W, bbox, cuda)


def test_two_rays_on_one_pixel(cuda):
    """A two-term float add is commutative: the parked sum, and with it the result, has the twin's bits."""
    B, H, W = 1, 16, 20
    idx = np.array([105, 105, 106, 0, 0, 19, 319, 319, 150])        # an interior pair, two border pairs
    pix = np.stack((idx % W, idx // W), 1).astype(np.int32)
    _check("shared pixels", _grad_rows(len(idx), 24), pix, np.zeros(len(idx), dtype=np.int32), B, H, W, 8, cuda)


def test_workspace_filled_with_nan(cuda):
    B, H, W = 2, 18, 35
    pix, bid = rb.pixel_rays(B, H, W)
    keep = np.random.default_rng(25).random(pix.shape[0]) < 0.4     # most pixels named by no ray
    pix, bid = np.ascontiguousarray(pix[keep]), np.ascontiguousarray(bid[keep])
    _check("poisoned workspace", _grad_rows(pix.shape[0], 26), pix, bid, B, H, W, 8, cuda, poison=True)


def test_non_default_stream(cuda):
    B, H, W = 2, 18, 35
    pix, bid = rb.pixel_rays(B, H, W)
    g = _grad_rows(pix.shape[0], 27)
    gd, pd, bd = torch.from_numpy(g).to(cuda), torch.from_numpy(pix).to(cuda), torch.from_numpy(bid).to(cuda)
    ref = _adjoint("ordered", gd, pd, bd, B, H, W, 8, cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        got = _adjoint("ordered", gd, pd, bd, B, H, W, 8, cuda, poison=True)
    side.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(got.cpu(), torch.from_numpy(rb.roi_backward_ordered(g, pix, bid, B, H, W, 8)))


def test_autograd_node_routes(cuda):
    """query._RayFeaturesFn with the argument: 'ordered' has the entry's bits, the default and no argument agree."""
    from implicit_depth_amd.query import _RayFeaturesFn
    B, H, W = 2, 12, 16
    pix, bid = rb.pixel_rays(B, H, W)
    g = _grad_rows(pix.shape[0], 28)
    gd, pd, bd = torch.from_numpy(g).to(cuda), torch.from_numpy(pix).to(cuda), torch.from_numpy(bid).to(cuda)
    ray_dir = torch.nn.functional.normalize(torch.randn(pix.shape[0], 3, generator=torch.Generator().manual_seed(29)),
                                            dim=1).to(cuda)
    grads = {}
    for route in ("ordered", "atomic", None):
        fg = torch.zeros(B, 32, H, W, device=cuda, requires_grad=True)
        extra = () if route is None else (route,)
        (_RayFeaturesFn.apply(fg, ray_dir, pd, bd, 8, LV, *extra) * gd).sum().backward()
        grads[route] = fg.grad
    assert torch.equal(grads["ordered"].cpu(), torch.from_numpy(rb.roi_backward_ordered(g, pix, bid, B, H, W, 8)))
    assert (grads["atomic"] - grads[None]).abs().max().item() <= 1e-5 * max(1.0, grads[None].abs().max().item())
    with pytest.raises(ValueError):
        _RayFeaturesFn.apply(torch.zeros(B, 32, H, W, device=cuda, requires_grad=True), ray_dir, pd, bd, 8, LV, "x")


# ---- end to end -----------------------------------------------------------------------------------------------------
def _modules(dev):
    from implicit_depth_amd.synthetic import init_decoder_params
    from util import orc
    pnet = make_pointnet(orc.init_pointnet(3, 1.5), dev).train()
    prob = make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, dev).train()
    off = make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, dev).train()
    return pnet, prob, off


def _batch(dev):
    from implicit_depth_amd.synthetic import synthetic_batch
    batch, feat = synthetic_batch(2, 24, 32, seed=3)
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}, feat.to(dev)


def _clamped_rays(dd, half=4):
    x, y = dd["ray_pix"][:, 0], dd["ray_pix"][:, 1]
    return int(((x < half) | (x > dd["w"] - 1 - half) | (y < half) | (y > dd["h"] - 1 - half)).sum())


def _same_bits(a, b, what):
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, (what, differ)


def test_lidf_forward_train_ordered(cuda):
    from implicit_depth_amd import LidfOptions, lidf_forward_train
    batch, feat = _batch(cuda)

    def run(route):
        mods = _modules(cuda)
        f = feat.clone().requires_grad_()
        np.random.seed(31)
        ok, dd, loss = lidf_forward_train(batch, f, *mods, opt=LidfOptions(roi_backward=route), epoch=0)
        assert ok and _clamped_rays(dd) > 0 and dd["total_miss_sample_num"] > _clamped_rays(dd)
        loss["loss_net"].backward()
        out = {"loss_net": loss["loss_net"].detach().clone()}
        for name, m in zip(("pnet", "prob", "off"), mods):
            out.update({"%s.%s" % (name, k): p.grad.clone() for k, p in m.named_parameters()})
        return f.grad.clone(), out
    g1, p1 = run("ordered")
    g2, p2 = run("ordered")
    g0, p0 = run("atomic")
    assert bool(g1.any()) and torch.equal(g1, g2)
    _same_bits(p1, p2, "ordered, second run")
    _same_bits(p1, p0, "ordered against the default route")       # every parameter gradient and loss_net
    assert (g1 - g0).abs().max().item() <= 1e-5 * max(1.0, g0.abs().max().item())


def test_refine_forward_train_ordered(cuda):
    from implicit_depth_amd import LidfOptions, train_refine_step
    from implicit_depth_amd.pipeline import refine_forward_train
    from implicit_depth_amd.synthetic import init_decoder_params
    from util import orc
    batch, feat = _batch(cuda)
    mods = _modules(cuda)

    def modules_r():
        return (make_pointnet(orc.init_pointnet(4, 1.5), cuda).train(),
                make_module("IEF", init_decoder_params("IEF", 334, 9, 5.0), 334, cuda).train())
    np.random.seed(32)
    ok, dd0, _, _ = train_refine_step(batch, feat, *mods, *modules_r(), opt=LidfOptions(maxpool_label_epo=0))
    assert ok and _clamped_rays(dd0) > 0

    def run(route):
        mods_r = modules_r()
        dd = dict(dd0)
        dd["full_rgb_feat"] = feat.clone().requires_grad_()
        np.random.seed(33)
        dd, loss = refine_forward_train(dd, *mods_r, opt=LidfOptions(maxpool_label_epo=0, roi_backward=route))
        loss["loss_net"].backward()
        out = {"loss_net": loss["loss_net"].detach().clone()}
        for name, m in zip(("pnet_refine", "off_refine"), mods_r):
            out.update({"%s.%s" % (name, k): p.grad.clone() for k, p in m.named_parameters()})
        return dd["full_rgb_feat"].grad.clone(), out
    g1, p1 = run("ordered")
    g2, p2 = run("ordered")
    g0, p0 = run("atomic")
    assert bool(g1.any()) and torch.equal(g1, g2)
    _same_bits(p1, p2, "ordered, second run")
    _same_bits(p1, p0, "ordered against the default route")
    assert (g1 - g0).abs().max().item() <= 1e-5 * max(1.0, g0.abs().max().item())
