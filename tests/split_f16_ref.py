"""A twin of the split-f16 arithmetic of lidf_points_h.hip / lidf_rows_h.hip, and the criterion built on it (tests only).

precision="f16x3" evaluates every product of decoder layers 1-3 as  wh*xh + wh*xl + wl*xh  on f16 pieces with f32
accumulation. The float32 oracle's error alone is no unit for that path: the scheme carries a representation error
of its own (the dropped wl*xl term, the 22 bits of a two-piece operand, f16 subnormal low pieces at small weights)
which an exact-f32 evaluation does not have. The twin restates the scheme with plain torch ops, on CPU or GPU
tensors: every operand is rounded to f16 pieces where the kernels and their packers do (lidf_mma.h: hpiece, split1,
split2; stream_value_h, stream_value_r, decoder_pass_h) and nowhere else, exactly the three products are kept, products and
sums are float64, and a value is rounded to f32 only where the kernel holds an f32 value (layer outputs, the voxpart /
raypart tables, u, the running offset). Layer 4 and the output activation are float64. What remains between the twin
and the kernel is f32 accumulation, which is what the float32 oracle has: assert_split_close takes the sum of both
errors as its unit.

defect= (CPU tests only) makes the twin wrong the way these kernels can be wrong: a low piece lost, stale or flushed
is an error of 2^-11 on a few operands, not a wrong answer.
    "act2" / "act3"  low pieces of one activation pair (two features of one tile) dropped ahead of layer 2 / layer 3
    "wlo"            low weight pieces of one k-sub-step of layer 2 dropped (8 columns x 32 outputs)
    "emb"            low pieces of the layer-1 operand of one k-step dropped (query: 4 (octave, coordinate) combos,
                     sin and cos, enter and leave; rows: 16 columns)
    "ulvh"           the ul*vh product of the IEF term dropped
    "ray"            the low piece of the ray row dropped (query only)
    "flush"          f16 subnormal pieces flushed to zero"""
import numpy as np
import torch
import torch.nn.functional as F

from util import F64_FLOOR_ULPS, F64_K, f64_errors, orc

DEFECTS = ("act2", "act3", "wlo", "emb", "ulvh", "ray", "flush")
ROW_DEFECTS = ("act2", "act3", "wlo", "emb", "ulvh", "flush")     # "ray" exists in the factorised layer 1 only


def tile_feature(r, half):
    """Feature of result register r of a 32x32 tile in lane half `half` (lidf_mma.h:tile_feature)."""
    return (r & 3) + 8 * (r >> 2) + 4 * half


# where the defects sit: pair 5 of tile 3 (H1) / tile 2 (H2), lane half 0; output tile 1, input tile 4, sub-step 1
ACT2_FEATURES = [32 * 3 + tile_feature(10, 0), 32 * 3 + tile_feature(11, 0)]
ACT3_FEATURES = [32 * 2 + tile_feature(10, 0), 32 * 2 + tile_feature(11, 0)]
WLO_OUTPUTS = slice(32, 64)
WLO_COLUMNS = [32 * 4 + tile_feature(8 + i, 0) for i in range(8)]
EMB_KSTEP = 2


def pieces(x, n=2, flush=False):
    """x -> its n f16 pieces (lidf_mma.h: hpiece / split1 / split2), as float64 tensors. The operand is an f32 value in the
    kernel, the residual x - hi is exact in f32. flush: pieces below the f16 normal range read as zero."""
    r = x.float()
    out = []
    for _ in range(n):
        h = r.half()
        r = r - h.float()
        if flush:
            h = torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)
        out.append(h.double())
    return out


def _drop(t, cols, rows=slice(None)):
    t = t.clone()
    t[rows, cols] = 0
    return t


def prod3(W, X, flush=False, wl_drop=None, xl_drop=None):
    """[n, out] float64: X W^T as wh*xh + wh*xl + wl*xh. wl_drop (rows, cols) / xl_drop cols: low pieces read as 0."""
    wh, wl = pieces(W, 2, flush)
    xh, xl = pieces(X, 2, flush)
    if wl_drop is not None:
        wl = _drop(wl, wl_drop[1], wl_drop[0])
    if xl_drop is not None:
        xl = _drop(xl, xl_drop)
    return (xh + xl) @ wh.t() + xh @ wl.t()


def _lrelu32(z32):
    return torch.maximum(z32, z32 * 0.02)        # lrelu1: v_max_f32(x, x * 0.02f)


def _hidden(z32, W, b, flush, xl_drop=None, wl_drop=None):
    """One of layers 2, 3 on the f32 pre-activations of the layer before: f32 pre-activations."""
    z = prod3(W, _lrelu32(z32), flush, wl_drop, xl_drop) + sum(pieces(b, 3, flush))
    return z.float()


def _tail(p, z1_32, defect):
    """Layers 2-4 on layer 1's f32 pre-activations: the pass's output [n, 1] in float64."""
    fl = defect == "flush"
    z2 = _hidden(z1_32, p["linear_2.weight"], p["linear_2.bias"], fl,
                 xl_drop=ACT2_FEATURES if defect == "act2" else None,
                 wl_drop=(WLO_OUTPUTS, WLO_COLUMNS) if defect == "wlo" else None)
    z3 = _hidden(z2, p["linear_3.weight"], p["linear_3.bias"], fl, xl_drop=ACT3_FEATURES if defect == "act3" else None)
    return F.linear(F.leaky_relu(z3.double(), 0.02), p["linear_4.weight"].double(), p["linear_4.bias"].double())


def _ief_parts(p, D):
    """(u, c) of an IEF: W1[:, enc] wenc as the f32 the packer holds, W1[:, enc] benc in float64."""
    We = p["linear_1.weight"][:, D:].double()
    return ((We @ p["offset_enc.weight"].double()[:, 0]).float(), We @ p["offset_enc.bias"].double())


def _passes(p, base32, kind, n_iter, D, defect):
    """The passes behind layer 1's constant part base32 [n, 256] (f32): the logit (IMNet) / the running offset after
    the last pass (IEF) in float64. The offset enters a pass as the f32 the kernel holds, in two pieces."""
    fl = defect == "flush"
    if kind != "IEF":
        return _tail(p, base32, defect)
    uh, ul = pieces(_ief_parts(p, D)[0], 2, fl)
    val = torch.full((base32.shape[0], 1), 0.001, dtype=torch.float32, device=base32.device)
    for _ in range(n_iter):
        vh, vl = pieces(val, 2, fl)
        t = (vh + vl) * uh.view(1, -1)
        if defect != "ulvh":
            t = t + vh * ul.view(1, -1)
        off = val.double() + _tail(p, (base32.double() + t).float(), defect)
        val = off.float()
    return off


def _check_defect(defect, allowed):
    if defect is not None and defect not in allowed:
        raise ValueError("defect %r: one of %s" % (defect, allowed))


def split_decoder(p, x, kind, n_iter=2, use_sigmoid=False, defect=None):
    """lidf_rows_h.hip on materialised rows x [n, D]: layer 1 over all D columns, b1 (+ c) riding as column D in
    two pieces. Returns the decoder's output [n, 1] in float64 on x's device."""
    _check_defect(defect, ROW_DEFECTS)
    fl = defect == "flush"
    p = {k: v.to(x.device) for k, v in p.items()}
    D = x.shape[1]
    W1 = p["linear_1.weight"]
    b = p["linear_1.bias"].double()
    if kind == "IEF":
        b = b + _ief_parts(p, D)[1]
    cols = list(range(16 * EMB_KSTEP, 16 * EMB_KSTEP + 16)) if defect == "emb" else None
    base = prod3(W1[:, :D], x, fl, xl_drop=cols) + sum(pieces(b, 2, fl))
    return orc._out_act(_passes(p, base.float(), kind, n_iter, D, defect), use_sigmoid)


def _emb_kstep_columns(ks, E):
    """Columns of cat(embed(enter), embed(leave)) that k-step ks of the factorised layer 1 covers
    (stream_value_h, K_L1): combos 4ks..4ks+3 = (octave c // 3, coordinate c % 3), sin and cos, both positions."""
    cols = []
    for c in range(4 * ks, 4 * ks + 4):
        for sc in (0, 1):
            col = 3 + 6 * (c // 3) + 3 * sc + c % 3
            cols += [col, E + col]
    return cols


def split_query(ray_dir, ray_pix, ray_bid, pair_ray, pair_vox, pair_t, pair_off, feat_grid, vox_feat, prob_p, off_p,
                off_kind="IEF", n_iter=2, use_sigmoid=False, multires=8, multires_views=4, roi_inp_bbox=8,
                offset_range=(0.0, 1.0), part_size=0.25, vox_center=None, pos_rel=False, chunk=65536,
                fast_roi=True, roi_out_bbox=2, max_pair_id=None, defect=None):
    """orc.query's signature and result keys (float64), layer 1 factorised as lidf_points_h.hip has it:
        z1 = voxpart[voxel] + (hi + lo of raypart[ray]) + W1[:, enter | leave] embed(position) (+ u val)
    voxpart = W1[:, 0:128] vox_feat + b1 (+ c) is an exact-f32 table (float64 here, rounded to f32); raypart =
    W1[:, rgb | dir] rayfeat comes from lidf_rows_h.hip's layer 1 (three products on the f32 per-ray rows, rounded
    to f32); the embedding's sin / cos values and the raw x, y, z are operands in two pieces."""
    _check_defect(defect, DEFECTS)
    fl = defect == "flush"
    dev = vox_feat.device
    c64 = lambda t: t.to(dev).double()  # noqa: E731
    ray_dir, pair_t, feat_grid, vox_feat = c64(ray_dir), c64(pair_t), c64(feat_grid), c64(vox_feat)
    R, P = ray_dir.shape[0], pair_ray.shape[0]
    E, Ed = orc.embed_dim(multires), orc.embed_dim(multires_views)
    boxes = orc.roi_boxes(ray_pix.long(), ray_bid.long(), feat_grid.shape[2], feat_grid.shape[3], roi_inp_bbox)
    if fast_roi and roi_out_bbox == 2:
        ray_rgb = orc.roi_align_fast(feat_grid, boxes).reshape(R, -1)
    else:
        ray_rgb = orc.roi_align(feat_grid, boxes, output_size=roi_out_bbox).reshape(R, -1).to(dev).double()
    rayfeat = torch.cat((ray_rgb, orc.embed(ray_dir, multires_views)), -1).float()
    ray_cols = list(range(128, 256)) + list(range(256 + 2 * E, 256 + 2 * E + Ed))
    emb_drop = _emb_kstep_columns(EMB_KSTEP, E) if defect == "emb" else None

    nets = []
    for p, kind in ((off_p, off_kind), (prob_p, "IMNET")):
        p = {k: v.to(dev) for k, v in p.items()}
        W1 = p["linear_1.weight"]
        D = 256 + 2 * E + Ed
        b = p["linear_1.bias"].double()
        if kind == "IEF":
            b = b + _ief_parts(p, D)[1]
        voxpart = (vox_feat @ W1[:, :128].double().t() + b).float()
        raypart = prod3(W1[:, ray_cols], rayfeat, fl).float()
        rp = pieces(raypart, 2, fl)
        nets.append((p, kind, voxpart, rp[0] if defect == "ray" else rp[0] + rp[1], W1[:, 256:256 + 2 * E], D))

    pred_offset = torch.empty(P, 1, dtype=torch.float64, device=dev)
    pred_prob = torch.empty(P, 1, dtype=torch.float64, device=dev)
    pair_pred_pos = torch.empty(P, 3, dtype=torch.float64, device=dev)
    for s in range(0, P, chunk):
        sl = slice(s, min(P, s + chunk))
        pr, pv, pt = pair_ray[sl].long(), pair_vox[sl].long(), pair_t[sl]
        d = ray_dir[pr]
        enter = d * pt[:, 0:1]
        leave = d * pt[:, 1:2]
        if pos_rel:
            c = c64(vox_center)[pv]
            ie, il = enter - c, leave - c
        else:
            ie, il = enter, leave
        emb = torch.cat((orc.embed(ie, multires), orc.embed(il, multires)), -1)
        outs = []
        for p, kind, voxpart, ray_rows, Wpe, D in nets:
            base = voxpart[pv].double() + ray_rows[pr] + prod3(Wpe, emb, fl, xl_drop=emb_drop)
            outs.append(orc._out_act(_passes(p, base.float(), kind, n_iter, D, defect), use_sigmoid))
        po, pp = outs
        sc = po * (offset_range[1] - offset_range[0]) + offset_range[0]
        sc = sc * np.sqrt(3) * part_size
        pred_offset[sl], pred_prob[sl] = po, pp
        pair_pred_pos[sl] = enter + sc * d
    pair_ray = pair_ray.long()
    sm = orc.scatter_softmax(pred_prob[:, 0], pair_ray, dim_size=R) if P > 0 else pred_prob[:, 0]
    if max_pair_id is None:
        _, max_pair_id = orc.scatter_max(sm, pair_ray, dim_size=R)
    dummy = torch.cat((pair_pred_pos, torch.zeros(1, 3, dtype=torch.float64, device=dev)), 0)
    return {"pred_offset": pred_offset, "pred_prob_end": pred_prob, "pair_pred_pos": pair_pred_pos,
            "pred_prob_end_softmax": sm, "max_pair_id": max_pair_id, "pred_pos": dummy[max_pair_id]}


def assert_split_close(what, got, ref64, ref32, twin, k=F64_K, floor_ulps=F64_FLOOR_ULPS, report=None):
    """util.assert_f64_close with the split path's unit. The kernel carries two errors independently — the scheme's
    representation error, which the twin has, and f32 accumulation, which the float32 oracle has — so the unit is
    their sum, elementwise and normwise, against the float64 oracle on the same inputs:
        max|got - ref64|            <= k (max|twin - ref64| + max|ref32 - ref64|)                 + floor_ulps 2^-24 max|ref64|
        ||got - ref64|| / ||ref64|| <= k (||twin - ref64|| + ||ref32 - ref64||) / ||ref64||       + floor_ulps 2^-24
    Returns (and appends to `report`, a list) the measured errors, both units and both ratios."""
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(ref32.shape) == tuple(twin.shape), \
        (what, got.shape, ref64.shape, ref32.shape, twin.shape)
    if ref64.numel() == 0:
        return None
    e_max, e32_max, e_nrm, e32_nrm, scale = f64_errors(got, ref64, ref32)
    et_max, _, et_nrm, _, _ = f64_errors(twin, ref64, ref32)
    u = 2.0 ** -24
    row = {"what": what, "max": e_max, "max32": e32_max, "max_twin": et_max,
           "ratio_max": e_max / max(et_max + e32_max, u * scale, 1e-300),
           "nrm": e_nrm, "nrm32": e32_nrm, "nrm_twin": et_nrm, "ratio_nrm": e_nrm / max(et_nrm + e32_nrm, u, 1e-300)}
    if report is not None:
        report.append(row)
    msg = ("%s: f16x3 vs float64 max %.3g / normwise %.3g; twin vs float64 max %.3g / normwise %.3g; f32 oracle vs "
           "float64 max %.3g / normwise %.3g; ratio %.2f / %.2f (k = %g)"
           % (what, e_max, e_nrm, et_max, et_nrm, e32_max, e32_nrm, row["ratio_max"], row["ratio_nrm"], k))
    print(msg)
    assert e_max == e_max and e_max <= k * (et_max + e32_max) + floor_ulps * u * scale, msg
    assert e_nrm <= k * (et_nrm + e32_nrm) + floor_ulps * u, msg
    return row
