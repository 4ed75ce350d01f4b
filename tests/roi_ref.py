"""RoIAlign at any output size as differentiable torch (tests only).

oracle.lidf_oracle.roi_align is the statement of torchvision's roi_align (aligned, sampling_ratio -1) the product is
held to, but it is a numpy loop: float32 only and outside autograd. Its vectorised twin roi_align_fast follows the
tensors' dtype and is differentiable, for 2 x 2 bins only. `roi_align_torch` is that twin at any output size, sample
for sample the loop's arithmetic (separable bilinear taps per axis, the same edge rules); `check_against_oracle`
holds its float32 values to the numpy loop, so that its float64 / float32 autograd gradients are the gradients of
orc.roi_align. `patched(orc)` puts it in the oracle's place for the duration of a `with` block, so that orc.query
differentiates through the ROI feature at any roi_out_bbox.
"""
import contextlib

import torch


def _axis_taps(start, binsz, g, S, size):
    """orc._axis_taps with S bins: (lo, hi) int64 [n, S, g] and (wlo, whi) [n, S, g]."""
    ph = torch.arange(S, dtype=start.dtype, device=start.device).view(1, S, 1)
    i = (torch.arange(g, dtype=start.dtype, device=start.device) + 0.5).view(1, 1, g)
    c = (start.view(-1, 1, 1) + ph * binsz.view(-1, 1, 1)) + (i * binsz.view(-1, 1, 1)) / float(g)
    dead = (c < -1.0) | (c > float(size))
    c = c.clamp(min=0.0)
    lo = c.floor().long()
    edge = lo >= size - 1
    lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    c = torch.where(edge, lo.to(c.dtype), c)
    l = c - lo.to(c.dtype)
    wlo, whi = 1.0 - l, l
    wlo = torch.where(dead, torch.zeros_like(wlo), wlo)
    whi = torch.where(dead, torch.zeros_like(whi), whi)
    return lo, hi, wlo, whi


def roi_align_torch(feat, boxes, output_size=2, chunk=4096):
    """feat [B, C, H, W], boxes [K, 5] (bid, x1, y1, x2, y2): [K, C, S, S] in feat's dtype, differentiable in feat."""
    S = int(output_size)
    B, C, H, W = feat.shape
    K = boxes.shape[0]
    boxes = boxes.to(device=feat.device, dtype=feat.dtype)   # (integer corners: exact in any float type)
    bid = boxes[:, 0].long()
    rsw, rsh = boxes[:, 1] - 0.5, boxes[:, 2] - 0.5
    roi_w, roi_h = (boxes[:, 3] - 0.5) - rsw, (boxes[:, 4] - 0.5) - rsh
    bw, bh = roi_w / float(S), roi_h / float(S)
    gw, gh = torch.ceil(roi_w / float(S)).long(), torch.ceil(roi_h / float(S)).long()
    pieces, order = [], []
    for g_h in torch.unique(gh).tolist():
        for g_w in torch.unique(gw).tolist():
            sel = ((gh == g_h) & (gw == g_w)).nonzero().flatten()
            if sel.numel() == 0:
                continue
            if g_h == 0 or g_w == 0:           # an empty box: no sample, the bin is 0
                pieces.append(feat.new_zeros((sel.numel(), C, S, S)) + 0.0 * feat.sum())
                order.append(sel)
                continue
            for s0 in range(0, sel.numel(), chunk):
                ids = sel[s0:s0 + chunk]
                ylo, yhi, wyl, wyh = _axis_taps(rsh[ids], bh[ids], g_h, S, H)
                xlo, xhi, wxl, wxh = _axis_taps(rsw[ids], bw[ids], g_w, S, W)
                n = ids.numel()
                bsel = bid[ids].view(n, 1, 1, 1)
                csel = torch.arange(C, device=feat.device).view(1, C, 1, 1)
                acc = torch.zeros(n, C, S, S, dtype=feat.dtype, device=feat.device)
                for yi, wy in ((ylo, wyl), (yhi, wyh)):
                    for xi, wx in ((xlo, wxl), (xhi, wxh)):
                        v = feat[bsel, csel, yi.reshape(n, 1, S * g_h, 1), xi.reshape(n, 1, 1, S * g_w)]
                        v = v * wy.reshape(n, 1, S * g_h, 1) * wx.reshape(n, 1, 1, S * g_w)
                        acc = acc + v.reshape(n, C, S, g_h, S, g_w).sum((3, 5))
                pieces.append(acc / float(max(g_h * g_w, 1)))
                order.append(ids)
    if not pieces:
        return torch.zeros(K, C, S, S, dtype=feat.dtype, device=feat.device)
    inv = torch.empty(K, dtype=torch.long, device=feat.device)
    cat_ids = torch.cat(order)
    inv[cat_ids] = torch.arange(K, device=feat.device)
    return torch.cat(pieces, 0)[inv]


def check_against_oracle(orc, feat, boxes, output_size):
    """The float32 values against the numpy loop (re-associated sums: a few units of 2^-24 of the largest value)."""
    got = roi_align_torch(feat.float(), boxes, output_size)
    ref = orc.roi_align(feat.float().cpu(), boxes.float().cpu(), output_size=output_size)
    tol = 16 * 2.0 ** -24 * max(float(feat.abs().max()), 1e-30)
    assert float((got.cpu() - ref).abs().max()) <= tol, (float((got.cpu() - ref).abs().max()), tol)


@contextlib.contextmanager
def patched(orc):
    """orc.roi_align replaced by roi_align_torch (same signature for the arguments orc.query passes)."""
    real = orc.roi_align

    def roi_align(feat, boxes, output_size=2, spatial_scale=1.0, aligned=True):
        assert spatial_scale == 1.0 and aligned
        return roi_align_torch(feat, boxes, output_size)
    orc.roi_align = roi_align
    try:
        yield
    finally:
        orc.roi_align = real
