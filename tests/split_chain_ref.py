"""A twin of the split-f16 decoder chain (csrc/lidf_chain16_h.hip, precision="f16x3" at gf_dim 32 / 64 / 128), tests
only. The method, the pieces and the criterion are tests/split_f16_ref.py's (pieces, prod3, assert_split_close,
util.F64_K); this file restates the NEW kernel with plain torch ops, on CPU or GPU tensors, float64 products and sums,
with a rounding only where the kernel holds a rounded value:

    tables                      voxpart / raypart rows are f32 (exact-f32 launches made them); their sum is f32
    base                        gathered rows + prod3(W1[:, per-row columns], X), rounded to f32 (the kernel's layer-1
                                accumulator starts from the rows' f32 sum and takes the three piece products of every
                                16-column group on the f16 matrix instruction, f32 accumulation)
    u * offset                  f32: u = W1[:, enc columns] wenc as the f32 the packer holds, the running offset f32,
                                base + u * offset on the f32 matrix instruction, rounded to f32 (NOT in pieces)
    layers 2, 3                 prod3 on the leaky-ReLU'd f32 pre-activations (max(z, 0.02 z) in f32), + the f32 bias
                                (exact: it seeds the accumulator through the f32 matrix instruction), rounded to f32
    layer 4, the activation     float64; the running offset is rounded to f32 after every pass

defect= makes the twin wrong the way THIS kernel can be wrong; the places follow its 16 x 16 tiles (lane = row j,
group g; register r of tile T = feature 16 T + 4 g + r):
    "act2" / "act3"  low pieces of one activation quad (features 16 T + 4 g + 0..3) dropped ahead of layer 2 / layer 3
    "wlo"            low weight pieces of one (output tile, input tile) block of layer 2 dropped (16 x 16 weights)
    "emb"            low pieces of one 16-column k-group of the layer-1 operand dropped
    "flush"          f16 subnormal pieces flushed to zero"""
import numpy as np
import torch
import torch.nn.functional as F

from split_f16_ref import assert_split_close, pieces, prod3  # noqa: F401  (assert_split_close: re-exported)
from util import orc

DEFECTS = ("act2", "act3", "wlo", "emb", "flush")

# where the defects sit (inside every width: layer 2 reads 4 gf >= 128 features, layer 3 2 gf >= 64):
# quad g = 2 of tile 3 (layer 2's input) / quad g = 1 of tile 2 (layer 3's input); output tile 1 x input tile 4;
# k-group 1
ACT2_FEATURES = [16 * 3 + 4 * 2 + r for r in range(4)]
ACT3_FEATURES = [16 * 2 + 4 * 1 + r for r in range(4)]
WLO_OUTPUTS = slice(16, 32)
WLO_COLUMNS = list(range(16 * 4, 16 * 5))
EMB_KGROUP = 1


def _check_defect(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError("defect %r: one of %s" % (defect, DEFECTS))


def _gf_of(p, gf):
    g = p["linear_3.weight"].shape[0]
    if gf is not None and int(gf) != g:
        raise ValueError("gf %r does not match the parameters (gf_dim %d)" % (gf, g))
    if g not in (32, 64, 128) or p["linear_4.weight"].shape[0] != 1:
        raise ValueError("the chain takes gf_dim 32 / 64 / 128 with a 1-wide head")
    return g


def _lrelu32(z32):
    return torch.maximum(z32, z32 * 0.02)        # v_med3_f32(z, 0.02f * z, +inf)


def _hidden(z32, W, b, flush, xl_drop=None, wl_drop=None):
    """One of layers 2, 3 on the f32 pre-activations of the layer before: f32 pre-activations."""
    return (prod3(W, _lrelu32(z32), flush, wl_drop, xl_drop) + b.double()).float()


def _tail(p, z1_32, defect):
    """Layers 2-4 on layer 1's f32 pre-activations: the pass's output [n, 1] in float64."""
    fl = defect == "flush"
    z2 = _hidden(z1_32, p["linear_2.weight"], p["linear_2.bias"], fl,
                 xl_drop=ACT2_FEATURES if defect == "act2" else None,
                 wl_drop=(WLO_OUTPUTS, WLO_COLUMNS) if defect == "wlo" else None)
    z3 = _hidden(z2, p["linear_3.weight"], p["linear_3.bias"], fl, xl_drop=ACT3_FEATURES if defect == "act3" else None)
    return F.linear(F.leaky_relu(z3.double(), 0.02), p["linear_4.weight"].double(), p["linear_4.bias"].double())


def ief_parts(p, D):
    """(u, c) of an IEF: W1[:, enc] wenc as the f32 the packer holds, W1[:, enc] benc in float64."""
    We = p["linear_1.weight"][:, D:D + 16].double()
    return ((We @ p["offset_enc.weight"].double()[:, 0]).float(), We @ p["offset_enc.bias"].double())


def bias_row(p, kind, D):
    """The one-row voxpart table of a launch without per-voxel columns: b1 (+ the IEF's constant), f32."""
    b = p["linear_1.bias"].double()
    if kind == "IEF":
        b = b + ief_parts(p, D)[1]
    return b.float()


def chain_passes(p, base32, kind, n_iter, D, defect=None, init_offset=0.001):
    """The passes behind layer 1's f32 accumulators base32 [n, 4 gf]: the logit (IMNet) / the running offset after
    the last pass (IEF), float64."""
    if kind != "IEF":
        return _tail(p, base32, defect)
    u = ief_parts(p, D)[0].double().view(1, -1)
    val = torch.full((base32.shape[0], 1), init_offset, dtype=torch.float32, device=base32.device)
    for _ in range(n_iter):
        off = val.double() + _tail(p, (base32.double() + u * val.double()).float(), defect)
        val = off.float()
    return off


def chain_rows(p, x, kind, n_iter=2, sig=False, gf=None, w1_col0=0, vox_rows=None, ray_rows=None, defect=None):
    """lidf_decoder_chain_split_f32 on per-row operand columns x [n, k] (they multiply W1[:, w1_col0 : w1_col0 + k])
    plus the already gathered f32 table rows vox_rows / ray_rows [n, 4 gf] (or [1, 4 gf]; either may be None).
    Returns the output [n, 1] in float64 on x's device."""
    _check_defect(defect)
    p = {k: v.to(x.device) for k, v in p.items()}
    _gf_of(p, gf)
    fl = defect == "flush"
    k = x.shape[1]
    D = p["linear_1.weight"].shape[1] - (16 if kind == "IEF" else 0)
    cols = None
    if defect == "emb":
        cols = [c for c in range(16 * EMB_KGROUP, 16 * EMB_KGROUP + 16) if c < k]
    rows = torch.zeros((1, p["linear_1.weight"].shape[0]), dtype=torch.float32, device=x.device)
    if vox_rows is not None:
        rows = vox_rows.float()
    if ray_rows is not None:
        rows = (rows + ray_rows.float()) if vox_rows is not None else ray_rows.float()   # the f32 sum of both rows
    base = rows.double() + prod3(p["linear_1.weight"][:, w1_col0:w1_col0 + k], x, fl, xl_drop=cols)
    return orc._out_act(chain_passes(p, base.float(), kind, n_iter, D, defect), sig)


def chain_decoder(p, x, kind, n_iter=2, sig=False, gf=None, defect=None):
    """decoders_forward(precision="f16x3") / generic.decoder_forward on materialised rows x [n, D]: every column is a
    per-row operand, the bias row the one-row voxpart."""
    D = x.shape[1]
    pd = {k: v.to(x.device) for k, v in p.items()}
    return chain_rows(p, x, kind, n_iter, sig, gf, 0, bias_row(pd, kind, D).view(1, -1), None, defect)


def chain_query(ray_dir, ray_pix, ray_bid, pair_ray, pair_vox, pair_t, pair_off, feat_grid, vox_feat, prob_p, off_p,
                off_kind="IEF", n_iter=2, use_sigmoid=False, multires=8, multires_views=4, roi_inp_bbox=8,
                offset_range=(0.0, 1.0), part_size=0.25, vox_center=None, pos_rel=False, chunk=65536,
                fast_roi=True, roi_out_bbox=2, max_pair_id=None, defect=None):
    """orc.query's signature and result keys (float64) with layer 1 factorised as generic.query has it at any width:
        z1 = voxpart[voxel] + raypart[ray] + W1[:, enter | leave] embed(position)
    voxpart = W1[:, voxel columns] vox_feat + b1 (+ c) and raypart = W1[:, ROI | direction columns] rayfeat are
    exact-f32 tables (float64 here, rounded to f32); the 2 E embedding columns are the chain launch's operand."""
    _check_defect(defect)
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
    Cv, Cr = vox_feat.shape[1], ray_rgb.shape[1]
    rayfeat = torch.cat((ray_rgb, orc.embed(ray_dir, multires_views)), -1)
    ray_cols = list(range(Cv, Cv + Cr)) + list(range(Cv + Cr + 2 * E, Cv + Cr + 2 * E + Ed))
    D = Cv + Cr + 2 * E + Ed

    nets = []
    for p, kind in ((off_p, off_kind), (prob_p, "IMNET")):
        p = {k: v.to(dev) for k, v in p.items()}
        W1 = p["linear_1.weight"].double()
        voxpart = (vox_feat @ W1[:, :Cv].t() + bias_row(p, kind, D).double()).float()
        raypart = (rayfeat @ W1[:, ray_cols].t()).float()
        nets.append((p, kind, voxpart, raypart))

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
        emb = torch.cat((orc.embed(ie, multires), orc.embed(il, multires)), -1).float()   # lidf_pe_rows_f32's f32 rows
        outs = []
        for p, kind, voxpart, raypart in nets:
            outs.append(chain_rows(p, emb, kind, n_iter, use_sigmoid, None, Cv + Cr, voxpart[pv], raypart[pr], defect))
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
