"""The ordered RoIAlign adjoint (lidf_ray_features_backward_ordered_f32) as numpy float32, operation for operation
(tests only): 32 channels, 2 x 2 bins, `half` = roi_inp_bbox // 2.

The order is the one include/lidf_hip.h states, written out literally:

  park     every ray adds its 128 gradient columns to gimg[b, c*4 + ph*2 + pw, qy, qx] (rays in their own order; the
           device's order among more than two rays of one pixel is not fixed, a two-term add is commutative).
  interior lidf_rayfeat_gather_kernel's order. Per destination pixel acc = 0, then for the bins (ph, pw) = (0,0) (0,1)
           (1,0) (1,1), for the source rows yy ascending (ph = 0: y+1 .. y+half; ph = 1: y-half+1 .. y), for the source
           columns xx ascending (alike): acc += gimg[b, bin, yy, xx], only sources with an unclamped box
           (half <= xx <= W-1-half, half <= yy <= H-1-half). The value is 0 + acc / half^2.
  border   onto it, the clamped boxes: source pixels in raster order (row, then column), bins 0..3 within a source
           pixel, each term ((g / (gh gw)) * wy) * wx added on its own, with roi_tap's sample positions and
           roi_axis_weight's summed tap weights. No product is fused with a sum.

Every array is float32 and every numpy operation rounds once, so the result has the kernel's bits (adding a zero term
changes no bit of a sum that is never -0, so the masked vector adds below equal the kernel's skipped terms).
`mutate` builds the wrong adjoints the CPU test must tell from the right one."""
import numpy as np

F = np.float32


def _tap(x, lim):
    """roi_tap: (lo, hi, l, ok) of one sample position."""
    ok = not (x < F(-1.0) or x > F(lim))
    if x <= F(0):
        x = F(0)
    lo = int(x)
    if lo >= lim - 1:
        hi = lo = lim - 1
        x = F(lo)
    else:
        hi = lo + 1
    return lo, hi, F(x - F(lo)), ok


def _axis_weights(start, binsz, n, lim):
    """roi_axis_weight for every pixel of the axis at once: float32 [lim]; the taps are added in sample order."""
    w = np.zeros(lim, dtype=F)
    for i in range(n):
        pos = F(start + F(F(F(i) + F(0.5)) * binsz) / F(n))
        lo, hi, l, ok = _tap(pos, lim)
        if not ok:
            continue
        w[lo] = F(w[lo] + F(F(1.0) - l))
        w[hi] = F(w[hi] + l)
    return w


def _axis(q, half, lim, unclamped_count=False):
    """(n, [weights of bin 0, weights of bin 1]) of the box of centre q along an axis of `lim` pixels."""
    c1, c2 = min(max(q - half, 0), lim - 1), min(max(q + half, 0), lim - 1)
    start = F(F(c1) - F(0.5))
    roi = F(F(F(c2) - F(0.5)) - start)
    binsz = F(roi / F(2.0))
    n = int(np.ceil(F(roi / F(2.0))))
    ws = [_axis_weights(F(start + F(F(p) * binsz)), binsz, n, lim) if n > 0 else np.zeros(lim, dtype=F)
          for p in range(2)]
    return (half if unclamped_count else n), ws


def park(d_rayfeat, ray_pix, ray_bid, B, H, W):
    """gimg [B, 128, H, W] float32: the first 128 columns of every ray's row at its pixel."""
    g = np.ascontiguousarray(np.asarray(d_rayfeat, dtype=F)[:, :128])
    pix, bid = np.asarray(ray_pix).astype(np.int64), np.asarray(ray_bid).astype(np.int64)
    gimg = np.zeros((B, H, W, 128), dtype=F)
    np.add.at(gimg, (bid, pix[:, 1], pix[:, 0]), g)
    return np.ascontiguousarray(gimg.transpose(0, 3, 1, 2))


def interior(gimg, half):
    """The interior gather: [B, 32, H, W]."""
    B, _, H, W = gimg.shape
    g = gimg.reshape(B, 32, 4, H, W)
    src = np.zeros((H, W), dtype=bool)
    src[half:H - half, half:W - half] = True        # sources with an unclamped box (empty on a narrow image)
    acc = np.zeros((B, 32, H, W), dtype=F)
    for ph in range(2):
        for pw in range(2):
            gm = np.where(src, g[:, :, ph * 2 + pw], F(0))
            for dy in (range(1 - half, 1) if ph else range(1, half + 1)):      # source row yy = y + dy, ascending
                for dx in (range(1 - half, 1) if pw else range(1, half + 1)):
                    ys0, ys1 = max(0, dy), min(H, H + dy)                        # source rows that have a destination
                    xs0, xs1 = max(0, dx), min(W, W + dx)
                    if ys0 >= ys1 or xs0 >= xs1:
                        continue
                    acc[:, :, ys0 - dy:ys1 - dy, xs0 - dx:xs1 - dx] += gm[:, :, ys0:ys1, xs0:xs1]
    return (F(0) + acc / F(half * half)).astype(F)


def border(gimg, half, out, mutate=None):
    """The clamped boxes' terms added onto `out` [B, 32, H, W] in place, source by source in raster order."""
    B, _, H, W = gimg.shape
    g = gimg.reshape(B, 32, 4, H, W)
    if mutate == "drop_clamped":
        return out
    unc = mutate == "unclamped_count"
    ax_y = {qy: _axis(qy, half, H, unc) for qy in range(H) if qy < half or qy > H - 1 - half}
    ax_x = {qx: _axis(qx, half, W, unc) for qx in range(W) if qx < half or qx > W - 1 - half}
    for qy in range(H):
        rowc = qy < half or qy > H - 1 - half
        for qx in range(W):
            if not (rowc or qx < half or qx > W - 1 - half):
                continue
            gs = g[:, :, :, qy, qx]                                  # [B, 32, 4]
            if not gs.any():
                continue
            gh, wys = ax_y[qy] if qy in ax_y else _cached(ax_y, qy, half, H, unc)
            gw, wxs = ax_x[qx] if qx in ax_x else _cached(ax_x, qx, half, W, unc)
            if gh <= 0 or gw <= 0:
                continue
            ny, nx = np.nonzero(wys[0] + wys[1])[0], np.nonzero(wxs[0] + wxs[1])[0]
            y0, y1, x0, x1 = ny.min(), ny.max() + 1, nx.min(), nx.max() + 1
            scaled = gs / F(gh * gw)
            for b in range(4):
                ph, pw = (b & 1, b >> 1) if mutate == "swap_bins" else (b >> 1, b & 1)
                term = scaled[:, :, b, None, None] * wys[ph][None, None, y0:y1, None]       # (g / (gh gw)) * wy
                out[:, :, y0:y1, x0:x1] += term * wxs[pw][None, None, None, x0:x1]          # ... * wx, then the add
    return out


def _cached(table, q, half, lim, unc):
    """The axis data of an unclamped coordinate of a source that is clamped along the other axis."""
    table[q] = _axis(q, half, lim, unc)
    return table[q]


def roi_backward_ordered(d_rayfeat, ray_pix, ray_bid, B, H, W, roi_inp_bbox, mutate=None):
    """d_feat_grid [B, 32, H, W] float32 of the ordered route. d_rayfeat [R, >= 128] (any float type, rounded to
    float32 first), ray_pix [R, 2] (x, y), ray_bid [R]."""
    half = roi_inp_bbox // 2
    assert 1 <= half <= 16
    gimg = park(d_rayfeat, ray_pix, ray_bid, B, H, W)
    out = interior(gimg, half)
    return border(gimg, half, out, mutate)


# ---- shared by the CPU and the GPU tests ----------------------------------------------------------------------------
def pixel_rays(B, H, W):
    """Every pixel of every frame a ray, frame-major raster order: (ray_pix [R, 2] int32 (x, y), ray_bid [R] int32)."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pix = np.tile(np.stack((xs.reshape(-1), ys.reshape(-1)), 1), (B, 1)).astype(np.int32)
    return pix, np.repeat(np.arange(B), H * W).astype(np.int32)


def torch_adjoint(d_rayfeat, ray_pix, ray_bid, B, H, W, roi_inp_bbox, dtype):
    """Autograd of the oracle's RoIAlign in torch ops (roi_ref.roi_align_torch) in `dtype`: d_feat_grid [B,32,H,W]."""
    import torch
    from roi_ref import roi_align_torch
    from util import orc
    pix = torch.as_tensor(np.asarray(ray_pix)).long()
    bid = torch.as_tensor(np.asarray(ray_bid)).long()
    g = torch.as_tensor(np.asarray(d_rayfeat, dtype=F)[:, :128]).to(dtype)
    feat = torch.zeros(B, 32, H, W, dtype=dtype, requires_grad=True)
    if pix.shape[0] == 0:
        return torch.zeros(B, 32, H, W, dtype=dtype)
    boxes = orc.roi_boxes(pix, bid, H, W, roi_inp_bbox)
    (roi_align_torch(feat, boxes, 2).reshape(pix.shape[0], -1) * g).sum().backward()
    return feat.grad.detach()
