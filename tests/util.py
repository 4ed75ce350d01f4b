"""Shared helpers for the parity tests (tests only)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import lidf_oracle as orc  # noqa: E402  (the checker; never used by the product)

TOL = 1e-4  # north_star: outputs within 1e-4 fp32 of the reference decoder


def make_module(kind, params, inp_dim, device, n_iter=2, use_sigmoid=False, gf=64):
    """Product module (implicit_depth_amd.decoders) carrying the oracle's parameters."""
    from implicit_depth_amd import IEF, IMNet
    if kind == "IEF":
        m = IEF(device, inp_dim, 1, gf, n_iter=n_iter, use_sigmoid=use_sigmoid)
    else:
        m = IMNet(inp_dim, 1, gf, use_sigmoid=use_sigmoid)
    m.load_state_dict({k: v.clone() for k, v in params.items()})
    return m.to(device).eval()


def to_dev(scene, device):
    out = {}
    for k, v in scene.items():
        out[k] = v.to(device) if torch.is_tensor(v) else v
    return out


def run_query(scene, device, **kw):
    """Product path on `device` for an oracle synthetic_scene dict."""
    from implicit_depth_amd.query import lidf_query
    s = to_dev(scene, device)
    D = 256 + 2 * orc.embed_dim(8) + orc.embed_dim(4)
    prob = make_module("IMNET", scene["prob_p"], D, device)
    off = make_module("IEF", scene["off_p"], D, device)
    depth = torch.zeros((scene["B"], scene["h"], scene["w"]), device=device)
    with torch.no_grad():
        out = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"],
                         s["pair_vox"], s["pair_t"], s["feat_grid"], s["vox_feat"], prob, off,
                         ray_flat=s["ray_flat"], depth=depth, **kw)
    out["depth"] = depth
    return out


def oracle_query(scene, **kw):
    return orc.query(scene["ray_dir"], scene["ray_pix"], scene["ray_bid"], scene["pair_ray"].long(),
                     scene["pair_vox"].long(), scene["pair_t"], scene["pair_off"],
                     scene["feat_grid"], scene["vox_feat"], scene["prob_p"], scene["off_p"], **kw)


def closed_form(shape, a, b, amp):
    """Deterministic pseudo-random tensor amp*sin(i*a + b) (float64 sin, cast to f32): lets the
    golden fixtures carry only outputs — weights and inputs are regenerated from this formula."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float64)
    return (amp * torch.sin(i * a + b)).float().reshape(shape)


def closed_form_params(kind, inp_dim, seed, gf=64, factor=1.0):
    """State dict with reference parameter names, weights ~ amplitude 0.14 (std 0.1), biases 0.05. factor: the
    linear_* weights (not the biases, not offset_enc) times it, in float32 — at amplitude 0.14 the decoders' outputs
    stay on one branch of the output clamp (tests/golden/make_golden_widths.py searches a factor per case)."""
    dims = [("linear_1", inp_dim + (16 if kind == "IEF" else 0), 4 * gf), ("linear_2", 4 * gf, 2 * gf),
            ("linear_3", 2 * gf, gf), ("linear_4", gf, 1)]
    p = {}
    if kind == "IEF":
        p["offset_enc.weight"] = closed_form((16, 1), 0.9, seed + 0.5, 0.3)
        p["offset_enc.bias"] = closed_form((16,), 1.3, seed + 0.7, 0.1)
    for j, (name, din, dout) in enumerate(dims):
        p[name + ".weight"] = closed_form((dout, din), 0.6180339887 + 0.01 * j, seed + j, 0.14)
        if factor != 1.0:
            p[name + ".weight"] = p[name + ".weight"] * torch.tensor(factor, dtype=torch.float32)
        p[name + ".bias"] = closed_form((dout,), 0.7236067977, seed + 10 + j, 0.05)
    return p


def closed_form_pointnet(seed, cin=6, out=128, gf=32):
    """PointNet2Stage(cin, out, gf) state dict from the closed-form filler (default: the shipped 6 / 128 / 32)."""
    shapes = {"point_lin1": (gf, cin), "point_lin2": (out // 2, gf), "vox_lin1": (out // 2, out // 2),
              "point_lin3": (out, out), "point_lin4": (out, out), "vox_lin2": (out, out)}
    p = {}
    for j, (name, (dout, din)) in enumerate(shapes.items()):
        amp = 1.4 / (din ** 0.5)
        p[name + ".weight"] = closed_form((dout, din), 0.6180339887 + 0.013 * j, seed + j, amp)
        p[name + ".bias"] = closed_form((dout,), 0.7236067977, seed + 20 + j, 0.1)
    return p


def make_pointnet(params, device, out=128, gf=32):
    from implicit_depth_amd import PointNet2Stage
    m = PointNet2Stage(input_channels=params["point_lin1.weight"].shape[1], output_channels=out, gf_dim=gf)
    m.load_state_dict({k: v.clone() for k, v in params.items()})
    return m.to(device).eval()


# ----------------------------------------------------------------------------------------------
# float64 yardstick: the HIP f32 path against a float64 evaluation of the oracle, with the oracle's own
# float32 error on the same inputs as the unit (tests/test_f64_gpu.py, tests/test_f64_criterion.py)
# ----------------------------------------------------------------------------------------------
F64_K = 4.0          # the kernel may be this many times less accurate than the f32 torch evaluation
F64_FLOOR_ULPS = 4   # plus this many units of 2^-24 of the tensor's largest magnitude

# Bias gradients are column sums of dZ over the rows. The training kernels sum them serially per lane over a
# slice's rows (lidf_train.hip, asum / bs2 of the weight-gradient kernel) where torch's reference reduces with a
# tree; on an MI355X that costs 2-4.3x the f32 reference's error (largest: off.linear_3.bias of the 614,400-pair
# query-training step, 4.26 elementwise / 3.65 normwise; prob.linear_4.bias of the pair node at 320 rows, 4.16).
# Weight gradients and every other tensor keep the shared F64_K.
K_BIAS = 6.0


def k_for(name):
    """The factor of assert_f64_close for the gradient of parameter `name`."""
    return K_BIAS if name.endswith(".bias") else F64_K


def f64(obj, device=None):
    """float64 copy of a tensor or of a dict of tensors (integer tensors keep their type)."""
    if isinstance(obj, dict):
        return {k: f64(v, device) for k, v in obj.items()}
    if not torch.is_tensor(obj):
        return obj
    t = obj.detach().to(device) if device is not None else obj.detach()
    return t.double() if t.is_floating_point() else t


def inv_out_act(v):
    """Exact inverse of the decoders' output activation max(min(y, 0.01y + 0.99), 0.01y) (implicit_net.py:96),
    in float64: v < 0 -> 100 v, v > 1 -> 100 (v - 0.99). The activation divides any logit error by 100 outside
    [0, 1]; comparing logits keeps that error visible."""
    v = v.double()
    return torch.where(v < 0, 100.0 * v, torch.where(v > 1, 100.0 * (v - 0.99), v))


def f64_errors(got, ref64, ref32):
    """(max|got - ref64|, max|ref32 - ref64|, ||got - ref64|| / ||ref64||, ||ref32 - ref64|| / ||ref64||, max|ref64|)."""
    r = ref64.double().reshape(-1)
    g = got.detach().double().to(r.device).reshape(-1)
    s = ref32.detach().double().to(r.device).reshape(-1)
    nr = max(r.norm().item(), 1e-300)
    return ((g - r).abs().max().item(), (s - r).abs().max().item(), (g - r).norm().item() / nr,
            (s - r).norm().item() / nr, r.abs().max().item())


def assert_f64_close(what, got, ref64, ref32, k=F64_K, floor_ulps=F64_FLOOR_ULPS, report=None):
    """The HIP result must be no less accurate than the float32 oracle it replaces, within a factor k, both
    elementwise and normwise, against the float64 oracle on the same inputs:
        max|got - ref64|          <= k max|ref32 - ref64|           + floor_ulps 2^-24 max|ref64|
        ||got - ref64|| / ||ref64|| <= k ||ref32 - ref64|| / ||ref64|| + floor_ulps 2^-24
    Returns (and appends to `report`, a list) the measured errors; the assertion message carries both errors
    and their ratio."""
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(ref32.shape), (what, got.shape, ref64.shape, ref32.shape)
    if ref64.numel() == 0:
        return None
    e_max, e32_max, e_nrm, e32_nrm, scale = f64_errors(got, ref64, ref32)
    u = 2.0 ** -24
    row = {"what": what, "max": e_max, "max32": e32_max, "ratio_max": e_max / max(e32_max, u * scale, 1e-300),
           "nrm": e_nrm, "nrm32": e32_nrm, "ratio_nrm": e_nrm / max(e32_nrm, u, 1e-300)}
    if report is not None:
        report.append(row)
    msg = ("%s: HIP vs float64 max %.3g / normwise %.3g; f32 oracle vs float64 max %.3g / normwise %.3g; "
           "ratio %.2f / %.2f (k = %g)" % (what, e_max, e_nrm, e32_max, e32_nrm, row["ratio_max"],
                                           row["ratio_nrm"], k))
    print(msg)
    assert e_max == e_max and e_max <= k * e32_max + floor_ulps * u * scale, msg
    assert e_nrm <= k * e32_nrm + floor_ulps * u, msg
    return row


def check_selection(scene, got, r64, r32):
    """The product's arg-max is a maximum of its ray's float64 logits, to within the rounding the f32 path
    is allowed (k x the f32 oracle's largest logit error)."""
    R = scene["R"]
    pr = scene["pair_ray"].long().to(got["max_pair_id"].device)
    l64 = r64["pred_prob_end"][:, 0]
    tol = 4 * (r32["pred_prob_end"][:, 0].double() - l64).abs().max().item() + 2.0 ** -22
    mx = torch.full((R,), -float("inf"), dtype=torch.float64, device=l64.device)
    mx = mx.scatter_reduce(0, pr, l64, reduce="amax", include_self=True)
    mid = got["max_pair_id"].long()
    has = mid < scene["P"]
    assert bool((mx[~has] == -float("inf")).all())                  # a ray without pairs selects the dummy row
    chosen = l64[mid[has]]
    assert (pr[mid[has]] == torch.arange(R, device=mid.device)[has]).all()
    gap = (mx[has] - chosen).max().item()
    print("arg-max: largest float64 logit gap of a selected pair %.3g (tolerance %.3g)" % (gap, tol))
    assert gap <= tol, (gap, tol)


def decoder_preacts(p, x, kind, n_iter=2):
    """Every kink-bearing pre-activation of orc.decoder_forward(p, x, kind, n_iter), taken from the oracle itself
    (its preacts list): the three hidden layers of every pass, and the output clamp's argument (the IEF's running
    offset, the IMNet's logit)."""
    zs = []
    with torch.no_grad():
        orc.decoder_forward(p, x, kind, n_iter, preacts=zs)
    return zs[:-1], zs[-1]


def kink_rows(p, x, kind, n_iter=2, use_sigmoid=False, rel=1.5e-6):
    """[n] bool: rows of the float64 evaluation where any hidden pre-activation lies within rel x (its layer's
    max|z|) of the leaky-ReLU kink at 0, or the output clamp's argument within rel x max|y| of its kinks at 0
    and 1. Such a row's gradient depends on which side of the kink rounding puts it (slope 1 or 0.02), in
    any precision; gradient checks give it zero upstream gradient on both sides. (rel: the f32 oracle's own
    pre-activation error against float64 is 0.5-0.9e-6 x max|z| on the IEF at 385 inputs.)"""
    zs, y = decoder_preacts(p, x, kind, n_iter)
    return kink_rows_of(zs, y, use_sigmoid, rel)


def kink_rows_of(zs, y, use_sigmoid=False, rel=1.5e-6):
    """kink_rows' rule on pre-activations already taken (decoder_forward's preacts list, split as
    decoder_preacts does)."""
    bad = torch.zeros(y.shape[0], dtype=torch.bool, device=y.device)
    for z in zs:
        bad |= (z.abs() < rel * z.abs().max()).any(1)
    if not use_sigmoid:
        d = rel * max(y.abs().max().item(), 1.0)
        bad |= ((y.abs() < d) | ((y - 1.0).abs() < d)).any(1)
    return bad


def oracle_grads(p, x, kind, w, dt, n_iter=2, use_sigmoid=False):
    """Oracle decoder output and gradients of sum(y * w) at dtype dt, on x's device: {param: grad, "input": grad}.
    Parameters and input are fresh leaves (a copy even where x already has dtype dt), so two calls on the same x
    never share an input gradient."""
    pc = {k: v.detach().to(x.device, dt, copy=True).requires_grad_(True) for k, v in p.items()}
    xc = x.detach().to(dt, copy=True).requires_grad_(True)
    y = orc.decoder_forward(pc, xc, kind, n_iter, use_sigmoid)
    (y.reshape(-1) * w.to(dt)).sum().backward()
    g = {k: v.grad for k, v in pc.items()}
    g["input"] = xc.grad
    return y.detach(), g


def tf32_off():
    """Context manager: full-precision float32 matmuls (no TF32) for the references, restored on exit."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        old = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        try:
            yield
        finally:
            torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old
    return cm()
