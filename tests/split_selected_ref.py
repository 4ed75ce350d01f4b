"""The float64 twin of precision="f16x3" with offsets="selected" (tests only): split_f16_ref's pieces in the data flow
of the list form of lidf_points_h_kernel.

prob_dec runs on every pair exactly as in the all-pairs launch (a net's arithmetic does not see the other net), so
pred_prob_end, the softmax and the arg-max are split_f16_ref.split_query's. offset_dec runs on the arg-max pair of every
ray that has one. There every row is its own ray, and the kernel gathers the ray's row of the raypart table beside the
voxel's row of the voxpart table and starts layer 1 from their f32 sum:
    z1 = f32(voxpart[voxel] + raypart[ray]) + W1[:, enter | leave] embed(position) (+ u val)
— the ray row is added WHOLE, it is not an operand in two f16 pieces as in the all-pairs launch (split_query), whose
rank-1 ray rounds the list form does not run. raypart itself is still the f32 table of lidf_rows_h.hip's layer 1 (three
products on the f32 per-ray rows, rounded to f32), voxpart the exact-f32 table. Everything behind layer 1's constant
part is split_f16_ref._passes.

Rows of pred_offset / pair_pred_pos that are no selected pair are NaN; a ray without a pair has max_pair_id == P and
pred_pos = (0, 0, 0).

ray_row= (CPU tests only) makes the twin wrong the way the list form can be wrong about the ray row:
    "wrong"  the row of the next ray (r + 1, wrapping)
    "drop"   no ray row
    "h1"     the ray row rounded to one f16 piece
defect= is split_f16_ref's, applied to the offset net (the prob net stays honest): "act2", "act3", "wlo", "emb", "ulvh",
"flush"."""
import numpy as np
import torch

import split_f16_ref as sp
from util import orc

RAY_ROWS = ("wrong", "drop", "h1")


def split_selected_query(ray_dir, ray_pix, ray_bid, pair_ray, pair_vox, pair_t, pair_off, feat_grid, vox_feat, prob_p,
                         off_p, off_kind="IEF", n_iter=2, use_sigmoid=False, multires=8, multires_views=4,
                         roi_inp_bbox=8, offset_range=(0.0, 1.0), part_size=0.25, vox_center=None, pos_rel=False,
                         chunk=65536, fast_roi=True, roi_out_bbox=2, max_pair_id=None, defect=None, ray_row=None):
    """split_query's signature and result keys (float64). max_pair_id given: that selection (P = no pair)."""
    sp._check_defect(defect, sp.ROW_DEFECTS)
    if ray_row is not None and ray_row not in RAY_ROWS:
        raise ValueError("ray_row %r: one of %s" % (ray_row, RAY_ROWS))
    fl = defect == "flush"
    full = sp.split_query(ray_dir, ray_pix, ray_bid, pair_ray, pair_vox, pair_t, pair_off, feat_grid, vox_feat, prob_p,
                          off_p, off_kind, n_iter, use_sigmoid, multires, multires_views, roi_inp_bbox, offset_range,
                          part_size, vox_center, pos_rel, chunk, fast_roi, roi_out_bbox, max_pair_id)
    dev = vox_feat.device
    c64 = lambda t: t.to(dev).double()  # noqa: E731
    ray_dir, pair_t, feat_grid, vox_feat = c64(ray_dir), c64(pair_t), c64(feat_grid), c64(vox_feat)
    R, P = ray_dir.shape[0], pair_ray.shape[0]
    E, Ed = orc.embed_dim(multires), orc.embed_dim(multires_views)
    mid = full["max_pair_id"].to(dev).long()
    has = (mid >= 0) & (mid < P)
    rays, rows = torch.nonzero(has)[:, 0], mid[has]

    # the per-ray feature rows and the offset net's two layer-1 tables, as in split_query
    boxes = orc.roi_boxes(ray_pix.long(), ray_bid.long(), feat_grid.shape[2], feat_grid.shape[3], roi_inp_bbox)
    if fast_roi and roi_out_bbox == 2:
        ray_rgb = orc.roi_align_fast(feat_grid, boxes).reshape(R, -1)
    else:
        ray_rgb = orc.roi_align(feat_grid, boxes, output_size=roi_out_bbox).reshape(R, -1).to(dev).double()
    rayfeat = torch.cat((ray_rgb, orc.embed(ray_dir, multires_views)), -1).float()
    ray_cols = list(range(128, 256)) + list(range(256 + 2 * E, 256 + 2 * E + Ed))
    p = {k: v.to(dev) for k, v in off_p.items()}
    W1 = p["linear_1.weight"]
    D = 256 + 2 * E + Ed
    b = p["linear_1.bias"].double()
    if off_kind == "IEF":
        b = b + sp._ief_parts(p, D)[1]
    voxpart = (vox_feat @ W1[:, :128].double().t() + b).float()
    raypart = sp.prod3(W1[:, ray_cols], rayfeat, fl).float()

    pv, pt, d = pair_vox.to(dev).long()[rows], pair_t[rows], ray_dir[rays]
    enter, leave = d * pt[:, 0:1], d * pt[:, 1:2]
    if pos_rel:
        c = c64(vox_center)[pv]
        ie, il = enter - c, leave - c
    else:
        ie, il = enter, leave
    emb = torch.cat((orc.embed(ie, multires), orc.embed(il, multires)), -1)
    if ray_row == "wrong":
        const32 = voxpart[pv] + raypart[(rays + 1) % R]
    elif ray_row == "drop":
        const32 = voxpart[pv]
    elif ray_row == "h1":
        const32 = voxpart[pv] + raypart[rays].half().float()
    else:
        const32 = voxpart[pv] + raypart[rays]          # ONE f32 sum per feature, the accumulator's initial value
    emb_drop = sp._emb_kstep_columns(sp.EMB_KSTEP, E) if defect == "emb" else None
    base = const32.double() + sp.prod3(W1[:, 256:256 + 2 * E], emb, fl, xl_drop=emb_drop)
    po = orc._out_act(sp._passes(p, base.float(), off_kind, n_iter, D, defect), use_sigmoid)
    sc = po * (offset_range[1] - offset_range[0]) + offset_range[0]
    sc = sc * np.sqrt(3) * part_size

    nan = float("nan")
    pred_offset = torch.full((P, 1), nan, dtype=torch.float64, device=dev)
    pair_pred_pos = torch.full((P, 3), nan, dtype=torch.float64, device=dev)
    pred_pos = torch.zeros(R, 3, dtype=torch.float64, device=dev)
    pred_offset[rows] = po
    pair_pred_pos[rows] = enter + sc * d
    pred_pos[rays] = pair_pred_pos[rows]
    return {"pred_offset": pred_offset, "pred_prob_end": full["pred_prob_end"], "pair_pred_pos": pair_pred_pos,
            "pred_prob_end_softmax": full["pred_prob_end_softmax"], "max_pair_id": full["max_pair_id"],
            "pred_pos": pred_pos, "selected_rows": rows, "selected_rays": rays}
