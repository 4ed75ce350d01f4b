"""generic.py — the reference's modules at widths other than the shipped configuration.

The register-chained kernels of liblidf_hip are built for the widths every shipped config uses
(imnet_gf 64, pnet_gf 32, pnet_out 128, rgb_out 32, roi_out_bbox 2: models/pipeline.py:56-85 with
experiments/implicit_depth/*.yaml). The reference's constructors take other values
(IMNet / IEF gf_dim and out_dim, PointNet2Stage input_channels / gf_dim / output_channels, the
ROI feature's channels and bins); those run here layer by layer: every nn.Linear is one
lidf_linear_f32 launch (the same f32 matrix-instruction kernel, 256 output columns per launch,
fused bias / activation / gathered term / scatter-max), the ROI pooling is lidf_roi_align_f32.
Same results as the reference's modules to the tolerance of the fast path (the summation order
inside a dot product differs from cuBLAS as it does there). The decoders also train at other
widths: every layer is an autograd function whose backward runs lidf_linear_f32 (input gradient)
and lidf_wgrad_f32 (weight and bias gradients), the PointNet's two poolings and its gather are
torch indexing that autograd differentiates itself. The stage-1 query trains at other widths through
query_train below (query.lidf_query_train sends every configuration its fixed-width kernels are not
built for here): the factorised layer 1 under autograd, with lidf_roi_align_backward_f32 and
lidf_gather2_backward_f32 as the adjoints of the ROI pooling and of the two gathered tables; stage 2 trains through refine_train (a decoder row is a
stage-1 pair with one pair per ray: the same factorised layer 1, and lidf_refine_step_forward_f32 / _backward_f32 for
the per-ray step of an iteration). The fused single-launch training kernels stay at the shipped widths.

Round 6: a decoder of gf_dim 32, 64 or 128 with a 1-wide head runs its inference as ONE register-chained launch
(lidf_decoder_chain_f32, csrc/lidf_chain16.hip: 16-row sub-tiles of the 16 x 16 x 4 matrix instruction, activations
in registers from layer 1 to the output) instead of one launch per layer and pass — the query and decoder_forward
take it; LIDF_CHAIN16=0 keeps the layer-by-layer path (A/B, and the definition the chain is tested against).
precision="f16x3" exists in that launch only (lidf_decoder_chain_split_f32, csrc/lidf_chain16_h.hip: the products of
layers 1-3 on f16 pieces): decoder_chain, decoder_forward, query and refine take it and refuse, with the reason, a
decoder the chain is not built for (split_refusal).

Nothing here is used when the widths are the shipped ones.
"""
import ctypes
import os

import torch

from . import _lib


def chain_ok(mod):
    """A decoder lidf_decoder_chain_f32 is built for: gf_dim 32 / 64 / 128, the reference's 4 gf -> 2 gf -> gf -> 1."""
    if os.environ.get("LIDF_CHAIN16", "1") == "0":
        return False
    gf = int(mod.gf_dim)
    return (gf in (32, 64, 128) and mod.linear_1.out_features == 4 * gf and mod.linear_2.out_features == 2 * gf
            and mod.linear_3.out_features == gf and mod.linear_4.out_features == 1)


def split_refusal(mod):
    """Why precision "f16x3" does not take this decoder at a configuration other than the shipped one (the split-f16
    products exist in the one-launch chain only: lidf_decoder_chain_split_f32), or None when it does."""
    if chain_ok(mod):
        return None
    if os.environ.get("LIDF_CHAIN16", "1") == "0":
        return ("LIDF_CHAIN16=0 switches the one-launch decoder chain off, and precision 'f16x3' at other widths "
                "exists in that chain only (there is no layer-by-layer split path)")
    if mod.linear_4.out_features != 1:
        return ("precision 'f16x3' takes decoders with a 1-wide head (the chain's 4 gf -> 2 gf -> gf -> 1); got "
                "out_dim=%d" % mod.linear_4.out_features)
    return ("precision 'f16x3' is built for gf_dim 32 / 64 / 128 (the one-launch decoder chain; there is no "
            "layer-by-layer split path); got gf_dim=%d" % int(mod.gf_dim))


def _check_precision(precision, *mods):
    if precision not in ("f32", "f16x3"):
        raise ValueError("precision must be 'f32' or 'f16x3'")
    if precision == "f16x3":
        for mod in mods:
            why = split_refusal(mod)
            if why:
                raise RuntimeError(why)


def _bias_row(mod):
    """b1 (+ the IEF's constant W1[:, enc columns] benc) as the one-row voxpart table of a chain launch."""
    from .decoders import IEF
    b = mod.linear_1.bias.detach().float()
    if isinstance(mod, IEF):
        d = mod.inp_dim
        b = b + mod.linear_1.weight.detach()[:, d:d + 16].float() @ mod.offset_enc.bias.detach().float()
    return b


def decoder_chain(mod, x, k, w1_col0=0, voxpart=None, vox_idx=None, raypart=None, ray_idx=None, out=None,
                  padded=False, packed=None, precision="f32"):
    """The whole decoder on per-row operand columns x[:, :k] (they multiply W1[:, w1_col0 : w1_col0 + k]) plus two
    gathered table rows — lidf_decoder_chain_f32. voxpart must carry b1 (+ the IEF constant: _bias_row). padded: x's
    buffer is readable up to column 16 ceil(k / 16) of its last row (otherwise the trailing rows go through a
    padded copy). packed: a dict the caller keeps over the slabs of one query — the first call leaves its workspace
    (the packed weight stream) there, the later ones skip the pack launch; the state is kept per precision (the two
    streams differ). precision "f16x3": lidf_decoder_chain_split_f32 — the products of layers 1-3 on f16 pieces, the
    tables, biases, the IEF's rank-1 term and layer 4 in f32. Returns [n, 1]."""
    from .decoders import _decoder_struct
    import ctypes as C
    _check_precision(precision, mod)
    split = precision == "f16x3"
    n = x.shape[0]
    dev = x.device
    if out is None:
        out = torch.empty((n, 1), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if x.stride(1) != 1:
        x = x.contiguous()
    ldx = x.stride(0) if n > 1 else x.shape[1]
    kq16 = (k + 15) // 16 * 16
    L = _lib.lib()
    gf = int(mod.gf_dim)
    wsb = (L.lidf_decoder_chain_split_workspace_bytes if split else L.lidf_decoder_chain_workspace_bytes)(gf, k)
    entry = L.lidf_decoder_chain_split_f32 if split else L.lidf_decoder_chain_f32
    state = packed.setdefault(precision, {}) if packed is not None else {}
    ws = state.get("ws")
    if ws is None:
        ws = state["ws"] = _lib.workspace(wsb, dev)
        state["ready"] = 0
    keep = []
    dec = _decoder_struct(mod, keep)

    def run(xs, ld, rows, o, vi, ri, rp):
        with torch.cuda.device(dev):
            _lib.check(entry(
                C.byref(dec), gf, int(mod.inp_dim), _lib.ptr(xs), ld, k, w1_col0, rows, _lib.ptr(voxpart), _lib.ptr(vi),
                _lib.ptr(rp), _lib.ptr(ri), _lib.ptr(o), state["ready"], _lib.ptr(ws), wsb,
                _lib.current_stream(dev)))
        state["ready"] = 1

    # rows whose 16-column groups would read past the end of x's buffer: through a padded copy
    tail = 0 if (padded or kq16 <= k) else min(n, (kq16 - k + max(ldx, 1) - 1) // max(ldx, 1))
    head = n - tail
    if head:
        run(x, ldx, head, out, vox_idx, ray_idx, raypart)
    if tail:
        xt = torch.zeros((tail, kq16), dtype=torch.float32, device=dev)
        xt[:, :k] = x[head:, :k]
        # (the tail's rows of a ray table without an index array are rows head.. of it)
        rp_t = raypart[head:] if (raypart is not None and ray_idx is None) else raypart
        run(xt, kq16, tail, out[head:], vox_idx[head:] if vox_idx is not None else None,
            ray_idx[head:] if ray_idx is not None else None, rp_t)
    return out


def linear_hip(x, weight, bias=None, act=0, slope=0.0, addrows=None, addidx=None, out=None,
               pool=None, poolidx=None, w_col0=0, k=None, addrows2=None, addidx2=None):
    """out = act(x @ weight[:, w_col0:w_col0+k].T + bias (+ addrows[addidx]) (+ addrows2[addidx2])) through
    lidf_linear_f32 / lidf_linear_gather2_f32.
    x [n, >=k] f32 (row stride free), weight [nout, ldw] f32; act 0 none / 1 max(v, slope*v).
    pool [V, nout] (zero-initialised) receives the scatter-max over poolidx instead of / beside out."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise RuntimeError("linear_hip: x must be a CUDA float32 matrix (no CPU path)")
    w = weight.detach()
    if w.dtype != torch.float32 or w.dim() != 2 or (w.shape[1] > 1 and w.stride(1) != 1):
        raise RuntimeError("linear_hip: weight must be float32 [nout, k] with unit column stride")
    n = x.shape[0]
    k = int(k if k is not None else w.shape[1] - w_col0)
    nout = int(w.shape[0])
    if x.shape[1] < k:
        raise RuntimeError("linear_hip: x has %d columns, the layer contracts over %d" % (x.shape[1], k))
    if x.stride(1) != 1:
        x = x.contiguous()
    ldx = x.stride(0) if n > 1 else x.shape[1]   # (a single row: its real width, never a fabricated stride)
    b = bias.detach().contiguous() if bias is not None else None
    if out is None and pool is None:
        out = torch.empty((n, nout), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    wsb = L.lidf_linear_workspace_bytes(k)
    ws = _lib.workspace(wsb, x.device)
    if n == 0:
        return out
    if addrows2 is not None:
        if addrows is None or pool is not None:
            raise RuntimeError("linear_hip: a second gathered term needs the first one and no pooling")
        with torch.cuda.device(x.device):
            _lib.check(L.lidf_linear_gather2_f32(
                _lib.ptr(x), ldx, n, k, w.data_ptr() + 4 * w_col0, max(w.stride(0), w.shape[1]) if nout > 1 else w.shape[1],
                _lib.ptr(b), nout, act, float(slope),
                _lib.ptr(addrows), _lib.ptr(addidx), addrows.stride(0),
                _lib.ptr(addrows2), _lib.ptr(addidx2), addrows2.stride(0),
                _lib.ptr(out), out.stride(0), _lib.ptr(ws), wsb, _lib.current_stream(x.device)))
        return out
    with torch.cuda.device(x.device):
        _lib.check(L.lidf_linear_f32(
            _lib.ptr(x), ldx, n, k, w.data_ptr() + 4 * w_col0, max(w.stride(0), w.shape[1]) if nout > 1 else w.shape[1],
            _lib.ptr(b), nout, act, float(slope),
            _lib.ptr(addrows), _lib.ptr(addidx), addrows.stride(0) if addrows is not None else 0,
            _lib.ptr(out), out.stride(0) if out is not None else 0,
            _lib.ptr(pool), _lib.ptr(poolidx), pool.stride(0) if pool is not None else 0,
            _lib.ptr(ws), wsb, _lib.current_stream(x.device)))
    return out


def _out_act(mod, y):
    # implicit_net.py:93-96 / :148-151 on the [n, out_dim] output
    if mod.use_sigmoid:
        return torch.sigmoid(y)
    return torch.max(torch.min(y, y * 0.01 + 0.99), y * 0.01)


def _decoder_from_layer1(mod, n, dev, layer1):
    """The decoder behind its first layer. layer1(act) -> [n, 4 gf]: W1[:, :inp_dim] x + b1, activated (act True: the
    IMNet's layer 1 in one launch) or not (the IEF's pass-independent part, to which every pass adds the 16
    offset-encoding columns)."""
    from .decoders import IEF
    l1, l2, l3, l4 = mod.linear_1, mod.linear_2, mod.linear_3, mod.linear_4
    if not isinstance(mod, IEF):
        h = layer1(True)
        h = linear_hip(h, l2.weight, l2.bias, act=1, slope=0.02)
        h = linear_hip(h, l3.weight, l3.bias, act=1, slope=0.02)
        return _out_act(mod, linear_hip(h, l4.weight, l4.bias))
    if l4.out_features != 1:
        raise RuntimeError("IEF feeds its output back through offset_enc = Linear(1, 16): out_dim must be 1")
    # layer 1 = W1[:, :d] x + b1 (the same in every pass) + W1[:, d:] enc(off)
    d = mod.inp_dim
    base = layer1(False)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    from .decoders import _init_offset_value
    off = torch.full((n, 1), _init_offset_value(mod), dtype=torch.float32, device=dev)
    for _ in range(int(mod.n_iter)):
        enc = linear_hip(off, mod.offset_enc.weight, mod.offset_enc.bias)
        h = linear_hip(enc, l1.weight, None, act=1, slope=0.02, addrows=base, addidx=rows, w_col0=d, k=16)
        h = linear_hip(h, l2.weight, l2.bias, act=1, slope=0.02)
        h = linear_hip(h, l3.weight, l3.bias, act=1, slope=0.02)
        off = off + linear_hip(h, l4.weight, l4.bias)
    return _out_act(mod, off)


def decoder_forward(mod, x, precision="f32"):
    """IMNet.forward / IEF.forward (models/implicit_net.py:81-98 / :131-152) at any gf_dim / out_dim
    on [n, inp_dim] rows. precision "f16x3": the split chain (chain_ok decoders only)."""
    _check_precision(precision, mod)
    x = x.detach()
    n, d = x.shape
    if d != mod.inp_dim:
        raise RuntimeError("decoder inp_dim %d != input width %d" % (mod.inp_dim, d))
    l1 = mod.linear_1
    if chain_ok(mod):   # one launch: every input column is a per-row operand, the bias a one-row table
        return decoder_chain(mod, x, d, voxpart=_bias_row(mod).reshape(1, -1).contiguous(), precision=precision)
    return _decoder_from_layer1(
        mod, n, x.device,
        lambda act: linear_hip(x, l1.weight, l1.bias, act=1 if act else 0, slope=0.02 if act else 0.0, k=d))


def pointnet_forward(mod, inp_feat, vox2point_idx, n_vox):
    """PointNet2Stage.forward (models/pointnet.py:22-38) at any input_channels / gf_dim /
    output_channels: torch_scatter's max becomes the scatter-max epilogue of the producing layer
    (values are post-ReLU, a voxel without points keeps 0)."""
    x = inp_feat.detach().contiguous()
    idx = vox2point_idx.detach().to(torch.int32).contiguous()
    dev = x.device
    half, outc = mod.point_lin2.out_features, mod.point_lin4.out_features
    if half % 32 or outc % 32:
        raise RuntimeError("PointNet2Stage: output_channels must be a multiple of 64 on this path "
                           "(the scatter-max epilogue raises whole 32-column tiles)")
    f1 = linear_hip(x, mod.point_lin1.weight, mod.point_lin1.bias, act=1)
    pool1 = torch.zeros((max(n_vox, 1), half), dtype=torch.float32, device=dev)
    f2 = linear_hip(f1, mod.point_lin2.weight, mod.point_lin2.bias, act=1, pool=pool1, poolidx=idx,
                    out=torch.empty((x.shape[0], half), dtype=torch.float32, device=dev))
    g1 = linear_hip(pool1[:n_vox], mod.vox_lin1.weight, mod.vox_lin1.bias, act=1)
    # point_lin3 on cat(g1[idx], f2): the voxel half once per voxel, gathered into the point half
    gpart = linear_hip(g1, mod.point_lin3.weight, mod.point_lin3.bias, k=half)
    f4 = linear_hip(f2, mod.point_lin3.weight, None, act=1, addrows=gpart, addidx=idx, w_col0=half, k=half)
    pool2 = torch.zeros((max(n_vox, 1), outc), dtype=torch.float32, device=dev)
    linear_hip(f4, mod.point_lin4.weight, mod.point_lin4.bias, act=1, pool=pool2, poolidx=idx)
    return linear_hip(pool2[:n_vox], mod.vox_lin2.weight, mod.vox_lin2.bias, act=1)


def roi_align_rays(feat_grid, ray_pix, ray_bid, roi_inp_bbox=8, roi_out_bbox=2):
    """The per-ray ROI feature (models/pipeline.py:374-391) at any channel count / output size:
    [R, C * roi_out_bbox^2] through lidf_roi_align_f32."""
    B, Cn, h, w = feat_grid.shape
    R = ray_pix.shape[0]
    out = torch.empty((R, Cn * roi_out_bbox * roi_out_bbox), dtype=torch.float32, device=feat_grid.device)
    fg = feat_grid.detach().contiguous()
    with torch.cuda.device(fg.device):
        _lib.check(_lib.lib().lidf_roi_align_f32(_lib.ptr(fg), B, Cn, h, w, _lib.ptr(ray_pix), _lib.ptr(ray_bid), R,
                                                 int(roi_inp_bbox), int(roi_out_bbox), _lib.ptr(out), out.shape[1],
                                                 _lib.current_stream(fg.device)))
    return out


QUERY_SLAB = 614400   # pairs per slab of the layer-by-layer query (rows [slab, D]: 0.95 GB at D = 385)
CHAIN_SLAB_FACTOR = 16


def query(ray_dir, ray_pix, ray_bid, pair_off, pair_ray, pair_vox, pair_t, feat_grid, vox_feat, prob_dec,
          offset_dec, multires, multires_views, roi_inp_bbox, roi_out_bbox, offset_range, part_size,
          vox_center, pos_rel, ray_flat, depth, want_rayfeat, precision="f32"):
    """get_embedding + get_pred (models/pipeline.py:338-466) at widths other than the shipped ones:
    the decoder input rows are materialised as the reference does ([P, pnet_out + rgb_out * roi^2 +
    2E + Ed]) and the decoders run layer by layer. The pieces: lidf_roi_align_f32, lidf_embed_f32,
    lidf_pe_rows_f32, lidf_linear_f32 per layer, lidf_query_tail_f32 (pair positions, per-ray softmax /
    arg-max, select); gathers and the concat are torch indexing on the device. precision "f16x3": the slabs run the
    split chain (lidf_decoder_chain_split_f32, both decoders chain_ok); the layer-1 tables stay exact f32."""
    from .decoders import get_embedder
    _check_precision(precision, prob_dec, offset_dec)
    dev = ray_dir.device
    R, P = ray_dir.shape[0], pair_ray.shape[0]
    E = 3 + 6 * multires
    L = _lib.lib()
    roi = roi_align_rays(feat_grid, ray_pix, ray_bid, roi_inp_bbox, roi_out_bbox)
    edir = get_embedder(multires_views)[0](ray_dir.detach().contiguous())
    D = vox_feat.shape[1] + roi.shape[1] + 2 * E + edir.shape[1]
    if D != prob_dec.inp_dim or D != offset_dec.inp_dim:
        raise RuntimeError("decoder inp_dim must be %d for this configuration" % D)
    # The reference materialises cat(...) [P, D] and every activation [P, 4 gf] at once (7.6 GB at the
    # configs[1] shape for D = 385 alone). Here the pairs go through in slabs of QUERY_SLAB rows (the slab the
    # CPU baseline uses): rows, positional encodings and activations of one slab are live at a time — about
    # 1 GB at D = 385, gf_dim = 64 —, the per-pair outputs [P, 1] are the only full-length arrays.
    # lidf_query_tail_f32 reads both arrays as [P]: the reference's own use (pred_prob_end[:, 0] and a 1-wide
    # offset, pipeline.py:437-442). A wider head would be read interleaved, so it is refused here.
    if prob_dec.linear_4.out_features != 1 or offset_dec.linear_4.out_features != 1:
        raise RuntimeError("the query takes decoders with out_dim == 1 (got prob_dec %d, offset_dec %d)"
                           % (prob_dec.linear_4.out_features, offset_dec.linear_4.out_features))
    vf = vox_feat.detach().contiguous()
    pred_prob = torch.empty((P, prob_dec.linear_4.out_features), dtype=torch.float32, device=dev)
    pred_offset = torch.empty((P, offset_dec.linear_4.out_features), dtype=torch.float32, device=dev)
    # Layer 1 in its factorised form (the algebra of the fixed-width kernels): of the D
    # columns of a row only the 2E position-embedding columns depend on the pair — the voxel columns give one
    # [V, 4 gf] table per decoder (with the bias), the ROI and direction columns one [R, 4 gf] table, and per pair
    # layer 1 is W1[:, pair columns] PE(p) + the two gathered table rows (lidf_linear_gather2_f32): 2E = 102 of the
    # 385 columns are multiplied per pair and the [P, D] rows of the reference are never formed.
    Cv, Cr, Ed = vf.shape[1], roi.shape[1], edir.shape[1]
    ray_rows = torch.arange(R, dtype=torch.int32, device=dev)
    tables = []
    chained = chain_ok(prob_dec) and chain_ok(offset_dec)
    packs = ({}, {})   # the chain launches' packed weight streams, one pack per decoder and query
    for dec in (prob_dec, offset_dec):
        l1 = dec.linear_1
        # (the chain launch takes the IEF's constant W1[:, enc] benc inside the per-voxel table, as the fixed-width
        # kernels do; the layer-by-layer path adds the encoded offset explicitly in every pass)
        voxpart = linear_hip(vf, l1.weight, _bias_row(dec) if chained else l1.bias, k=Cv)
        rp = linear_hip(roi, l1.weight, None, w_col0=Cv, k=Cr)
        raypart = linear_hip(edir, l1.weight, None, w_col0=Cv + Cr + 2 * E, k=Ed, addrows=rp, addidx=ray_rows)
        tables.append((voxpart, raypart))
    # (the chain launch keeps nothing per pair but the 2E position-embedding columns — 408 B at L = 8: the whole
    # configs[1] frame is 2 GB. At gf 128 longer slabs pay — one pack and one ramp-up per decoder and frame: 97.8 ->
    # 99.2 Mpoints/s —, at gf 32 they do not: 588 -> 578, a 614,400-pair slab of embedding rows is 250 MB and is
    # read back twice out of the 256 MB last-level cache instead of HBM)
    slab = QUERY_SLAB * (CHAIN_SLAB_FACTOR if (chained and prob_dec.gf_dim >= 128) else 1)
    for p0 in range(0, P, slab):
        p1 = min(P, p0 + slab)
        n = p1 - p0
        pr_s, pv_s, pt_s = pair_ray[p0:p1], pair_vox[p0:p1], pair_t[p0:p1]
        # (16 floats of slack behind the rows: the chain launch reads whole 16-column groups of the last row)
        pe = torch.empty((n * 2 * E + 16,), dtype=torch.float32, device=dev)[:n * 2 * E].view(n, 2 * E)
        with torch.cuda.device(dev):
            _lib.check(L.lidf_pe_rows_f32(_lib.ptr(pr_s), _lib.ptr(pv_s), _lib.ptr(pt_s), _lib.ptr(ray_dir),
                                          _lib.ptr(vox_center), 1 if pos_rel else 0, multires, n, _lib.ptr(pe),
                                          _lib.current_stream(dev)))
        pr_i, pv_i = pr_s.contiguous(), pv_s.contiguous()
        for dec, (voxpart, raypart), dst, pk in ((prob_dec, tables[0], pred_prob, packs[0]),
                                                  (offset_dec, tables[1], pred_offset, packs[1])):
            w1 = dec.linear_1.weight
            if chained:   # the whole decoder in one launch, straight into its slab of the output
                decoder_chain(dec, pe, 2 * E, w1_col0=Cv + Cr, voxpart=voxpart, vox_idx=pv_i, raypart=raypart,
                              ray_idx=pr_i, out=dst[p0:p1], padded=True, packed=pk, precision=precision)
                continue

            def layer1(act, w1=w1, voxpart=voxpart, raypart=raypart):
                return linear_hip(pe, w1, None, act=1 if act else 0, slope=0.02 if act else 0.0, w_col0=Cv + Cr,
                                  k=2 * E, addrows=voxpart, addidx=pv_i, addrows2=raypart, addidx2=pr_i)
            dst[p0:p1] = _decoder_from_layer1(dec, n, dev, layer1)
        del pe
    f32 = dict(dtype=torch.float32, device=dev)
    pos, sm = torch.empty((P, 3), **f32), torch.empty((P,), **f32)
    mid, pred = torch.empty((R,), dtype=torch.int64, device=dev), torch.empty((R, 3), **f32)
    off1, prob1 = pred_offset.reshape(-1).contiguous(), pred_prob.reshape(-1).contiguous()
    with torch.cuda.device(dev):
        _lib.check(L.lidf_query_tail_f32(_lib.ptr(off1), _lib.ptr(prob1), _lib.ptr(pair_off), _lib.ptr(pair_ray),
                                         _lib.ptr(pair_t), _lib.ptr(ray_dir), R, P, float(offset_range[0]),
                                         float(offset_range[1]), float(part_size), None, _lib.ptr(pos), _lib.ptr(sm),
                                         _lib.ptr(mid), _lib.ptr(pred), _lib.current_stream(dev)))
    if depth is not None:   # pipeline.py:593-596: the queried pixels take the predicted z
        hw = depth.shape[1] * depth.shape[2]
        depth.view(-1)[ray_bid.long() * hw + ray_flat.long()] = pred[:, 2]
    out = {"pred_offset": pred_offset, "pred_prob_end": pred_prob, "pair_pred_pos": pos,
           "pred_prob_end_softmax": sm, "max_pair_id": mid, "pred_pos": pred, "workspace": None}
    if want_rayfeat:
        out["rayfeat"] = torch.cat((roi, edir), 1)
    return out


def refine(ray_dir, ray_pix, ray_bid, ray_flat, pred_pos, max_pair_id, pair_vox, voxel_bound, voxel_bid, rgb_img,
           feat_grid, valid_inp, valid_vox, pnet_model, offset_dec, forward_times, multires, multires_views,
           roi_inp_bbox, roi_out_bbox, offset_range, pos_rel, pnet_pos_rel, ray_rgb, pnet_select, precision="f32"):
    """forward_times x RefineNet.get_pred_refine (models/pipeline.py:922-1030, eval flavour) at widths other
    than the shipped ones, step by step as the reference writes it: the end voxel of every ray
    (lidf_pcl_aabb_last_f32 over the arg-max pair's voxel), the PointNet over valid + predicted points,
    the decoder rows [R, pnet_out + rgb_out * roi^2 + E + Ed], the decoder, the offset along the ray. The
    modules run through their own forward (layer by layer where a width differs). precision "f16x3": the decoder
    goes through decoders_forward(rows, offset_dec=..., precision=...), the PointNet stays f32."""
    from .decoders import decoders_forward, get_embedder
    from .extensions import pcl_aabb
    if precision not in ("f32", "f16x3"):
        raise ValueError("precision must be 'f32' or 'f16x3'")
    dev = ray_dir.device
    R, P, V = ray_dir.shape[0], pair_vox.shape[0], voxel_bound.shape[0]
    hw = rgb_img.shape[2] * rgb_img.shape[3]
    if ray_rgb is None:
        ray_rgb = roi_align_rays(feat_grid, ray_pix, ray_bid, roi_inp_bbox, roi_out_bbox)
    edir = get_embedder(multires_views)[0](ray_dir.detach().contiguous())
    embed = get_embedder(multires)[0]
    miss_rgb = rgb_img.permute(0, 2, 3, 1).reshape(-1, 3)[ray_bid.long() * hw + ray_flat.long()]
    pv = torch.cat((pair_vox.long(), torch.zeros(1, dtype=torch.long, device=dev)))
    first = pv[max_pair_id.clamp(max=P)]                       # the dummy row's voxel is 0 (pipeline.py:933)
    sel = None
    if pnet_select is not None:
        sel = torch.nonzero(pnet_select.reshape(-1) != 0, as_tuple=False)[:, 0]
    cur = pred_pos.detach().contiguous()
    end_voxel = first.int()
    for _ in range(int(forward_times)):
        last = pcl_aabb.last_voxel(cur, voxel_bound, ray_bid, voxel_bid).long()     # -1: in no voxel
        end = torch.maximum(first, last)                       # (:939-944: scatter of the containing voxels)
        end_voxel = end.int()
        eb = voxel_bound[end]
        center = (eb[:, :3] + eb[:, 3:]) / 2.0
        pred_inp = torch.cat(((cur - center) if pnet_pos_rel else cur, miss_rgb), 1)
        if sel is not None:
            pn_inp, pn_vox = torch.cat((valid_inp, pred_inp[sel]), 0), torch.cat((valid_vox.long(), end[sel]), 0)
        else:
            pn_inp, pn_vox = torch.cat((valid_inp, pred_inp), 0), torch.cat((valid_vox.long(), end), 0)
        occ = pnet_model(pn_inp.contiguous(), pn_vox.int(), n_vox=V)
        enter = (cur - center) if pos_rel else cur
        rows = torch.cat((occ[end], ray_rgb, embed(enter.contiguous()), edir), 1)
        off = offset_dec(rows) if precision == "f32" else decoders_forward(rows, offset_dec=offset_dec,
                                                                           precision=precision)[1]
        cur = (cur + (off * (offset_range[1] - offset_range[0]) + offset_range[0]) * ray_dir).contiguous()
    return cur, end_voxel


class _LinearFn(torch.autograd.Function):
    """act(x W^T + b) through lidf_linear_f32 with a backward through the library: d x = (g * act') W
    (lidf_linear_f32 on W^T), d W = (g * act')^T x and d b = its column sums (lidf_wgrad_f32: fixed
    summation order for layers of >= 32 outputs and >= 4 inputs; the 1-wide output layer and offset_enc =
    Linear(1, 16) add their row slices with float atomics — correct to rounding, not bit-reproducible run
    to run, lidf_hip.h). act' is read off the output (leaky ReLU keeps the sign)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        out = linear_hip(x.detach(), weight, bias, act=act, slope=slope)
        ctx.cfg = (act, slope, bias is not None)
        ctx.save_for_backward(x, weight, out if act else None)   # (version counters catch in-place updates)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        x, w = x.detach(), w.detach()
        act, slope, has_bias = ctx.cfg
        g = g.detach().contiguous().float()
        if act:
            g = g * torch.where(out > 0, torch.ones((), device=g.device), torch.full((), slope, device=g.device))
        n, nout, k = x.shape[0], w.shape[0], w.shape[1]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = linear_hip(g, w.t().contiguous())
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            L = _lib.lib()
            dw = torch.zeros((nout, k), dtype=torch.float32, device=g.device)
            db = torch.zeros((nout,), dtype=torch.float32, device=g.device) if has_bias else None
            xc = x if x.stride(1) == 1 else x.contiguous()
            wsb = L.lidf_wgrad_workspace_bytes()
            ws = _lib.workspace(wsb, g.device)
            if n:
                with torch.cuda.device(g.device):
                    _lib.check(L.lidf_wgrad_f32(_lib.ptr(g), g.stride(0), nout, _lib.ptr(xc), xc.stride(0) if n > 1 else k,
                                                k, n, _lib.ptr(dw), k, _lib.ptr(db), _lib.ptr(ws), wsb,
                                                _lib.current_stream(g.device)))
        return dx, dw, db if has_bias else None, None, None


def _lin(x, layer, act=0, slope=0.0):
    return _LinearFn.apply(x, layer.weight, layer.bias, act, slope)


def decoder_forward_train(mod, x):
    """IMNet / IEF forward under autograd at any gf_dim / out_dim: the reference's own sequence of
    operations (implicit_net.py:81-98 / :131-152) with every nn.Linear as a _LinearFn; the concat, the
    running offset and the output activation are torch ops that autograd differentiates itself."""
    from .decoders import IEF, _init_offset_value
    if x.shape[1] != mod.inp_dim:
        raise RuntimeError("decoder inp_dim %d != input width %d" % (mod.inp_dim, x.shape[1]))

    def trunk(h):
        for layer in (mod.linear_1, mod.linear_2, mod.linear_3):
            h = _lin(h, layer, 1, 0.02)
        return _lin(h, mod.linear_4)
    if not isinstance(mod, IEF):
        return _out_act(mod, trunk(x))
    if mod.linear_4.out_features != 1:
        raise RuntimeError("IEF feeds its output back through offset_enc = Linear(1, 16): out_dim must be 1")
    off = torch.full((x.shape[0], 1), _init_offset_value(mod), dtype=torch.float32, device=x.device)
    for _ in range(int(mod.n_iter)):
        off = off + trunk(torch.cat((x, _lin(off, mod.offset_enc)), 1))
    return _out_act(mod, off)


def pointnet_forward_train(mod, inp_feat, vox2point_idx, n_vox):
    """PointNet2Stage.forward under autograd at any width: the reference's sequence (models/pointnet.py:
    22-38) with every nn.Linear as a _LinearFn. The scatter-max and the gather are device-side torch
    indexing (scatter_reduce 'amax' / index): their backward routes a voxel's gradient to its maximal
    point as torch_scatter does (exactly equal positive maxima — ties — share it instead). A layer of fewer than 32
    outputs (point_lin1 at gf_dim 16) takes the column-sum form of its weight gradient (_train_lin), so that the
    whole training step at other widths gives the same bits in every run."""
    from .pointnet import _segment_max
    idx = vox2point_idx.long()
    f2 = _train_lin(_train_lin(inp_feat, mod.point_lin1, 1), mod.point_lin2, 1)
    g1 = _train_lin(_segment_max(f2, idx, n_vox), mod.vox_lin1, 1)
    f5 = _train_lin(_train_lin(torch.cat((g1[idx], f2), -1), mod.point_lin3, 1), mod.point_lin4, 1)
    return _train_lin(_segment_max(f5, idx, n_vox), mod.vox_lin2, 1)


# ------------------------------------------------------------------------------------------------------------------
# The query under autograd at any width (get_embedding + get_pred for the stage-1 training step)
# ------------------------------------------------------------------------------------------------------------------
def _leaky_mask(g, out, slope):
    return g * torch.where(out > 0, torch.ones((), device=g.device), torch.full((), slope, device=g.device))


def _wgrad_into(a, b, c, col0=0, db=None):
    """c[:, col0 : col0 + b.shape[1]] += a^T b, db += column sums of a (lidf_wgrad_f32 straight into the column
    block of a wider gradient through ldc)."""
    n, m, k = a.shape[0], a.shape[1], b.shape[1]
    if n == 0:
        return
    L = _lib.lib()
    b = b if b.stride(1) == 1 else b.contiguous()
    wsb = L.lidf_wgrad_workspace_bytes()
    ws = _lib.workspace(wsb, a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.lidf_wgrad_f32(_lib.ptr(a), a.stride(0) if n > 1 else m, m, _lib.ptr(b),
                                    b.stride(0) if n > 1 else k, k, n, c.data_ptr() + 4 * col0, c.stride(0),
                                    _lib.ptr(db), _lib.ptr(ws), wsb, _lib.current_stream(a.device)))


def gather2_backward(dz, seg_off=None, n_seg=0, idx=None, n_idx_rows=0):
    """(d_addrows2 [n_seg, F], d_addrows [n_idx_rows, F]) of dz [n, F] through lidf_gather2_backward_f32: sums over
    the row ranges of the CSR offsets seg_off and sums by the row index idx; either may be left out (None)."""
    n, F = dz.shape
    dev = dz.device
    L = _lib.lib()
    d2 = torch.empty((n_seg, F), dtype=torch.float32, device=dev) if seg_off is not None else None
    d1 = torch.empty((n_idx_rows, F), dtype=torch.float32, device=dev) if idx is not None else None
    wsb = L.lidf_gather2_backward_workspace_bytes(n, n_idx_rows, F) if idx is not None else 0
    ws = _lib.workspace(wsb, dev)
    with torch.cuda.device(dev):
        _lib.check(L.lidf_gather2_backward_f32(_lib.ptr(dz), n, F, _lib.ptr(seg_off), n_seg, _lib.ptr(d2),
                                               _lib.ptr(idx), n_idx_rows, _lib.ptr(d1), _lib.ptr(ws), wsb,
                                               _lib.current_stream(dev)))
    return d2, d1


class _RoiAlignFn(torch.autograd.Function):
    """The per-ray ROI feature [R, C S^2] (lidf_roi_align_f32) with its adjoint to the feature map
    (lidf_roi_align_backward_f32: a gather, bit-reproducible for rays on distinct pixels). The backward runs only
    when feat_grid needs a gradient."""

    @staticmethod
    def forward(ctx, feat_grid, ray_pix, ray_bid, roi_inp_bbox, roi_out_bbox):
        ctx.save_for_backward(ray_pix, ray_bid)
        ctx.cfg = (tuple(feat_grid.shape), int(roi_inp_bbox), int(roi_out_bbox))
        return roi_align_rays(feat_grid, ray_pix, ray_bid, roi_inp_bbox, roi_out_bbox)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        ray_pix, ray_bid = ctx.saved_tensors
        (B, Cn, h, w), inp, outb = ctx.cfg
        g = g.detach().contiguous().float()
        dev = g.device
        d_feat = torch.empty((B, Cn, h, w), dtype=torch.float32, device=dev)
        L = _lib.lib()
        wsb = L.lidf_roi_align_backward_workspace_bytes(B, h, w)
        ws = _lib.workspace(wsb, dev)
        with torch.cuda.device(dev):
            _lib.check(L.lidf_roi_align_backward_f32(_lib.ptr(g), g.shape[1], _lib.ptr(ray_pix), _lib.ptr(ray_bid),
                                                     g.shape[0], B, Cn, h, w, inp, outb, _lib.ptr(d_feat),
                                                     _lib.ptr(ws), wsb, _lib.current_stream(dev)))
        return d_feat, None, None, None, None


class _Layer1Fn(torch.autograd.Function):
    """Layer 1 of a decoder in its factorised form, per pair: act(W1[:, pair columns] PE(p) + voxpart[voxel(p)] +
    raypart[ray(p)]) with voxpart = W1[:, voxel columns] vox_feat + b1 [V, 4 gf] and raypart = W1[:, ROI columns] roi +
    W1[:, direction columns] embed(dir) [R, 4 gf] (lidf_linear_f32 / lidf_linear_gather2_f32). No [P, D] row is formed,
    and no row gradient: the backward reduces dZ1 to the two tables (lidf_gather2_backward_f32, fixed order) before it
    meets a weight, forms the pair-column block of dW1 straight from the embedding rows (lidf_wgrad_f32 into the
    column block) and the other blocks, d vox_feat and d roi from the tables."""

    @staticmethod
    def forward(ctx, vox_feat, roi, w1, b1, edir, pe, pair_off, pair_ray, pair_vox, act):
        vf, rf = vox_feat.detach().contiguous(), roi.detach().contiguous()
        Cv, Cr, E2, Ed = vf.shape[1], rf.shape[1], pe.shape[1], edir.shape[1]
        R = rf.shape[0]
        ray_rows = torch.arange(R, dtype=torch.int32, device=vf.device)
        voxpart = linear_hip(vf, w1, b1, k=Cv)
        rp = linear_hip(rf, w1, None, w_col0=Cv, k=Cr)
        raypart = linear_hip(edir, w1, None, w_col0=Cv + Cr + E2, k=Ed, addrows=rp, addidx=ray_rows)
        out = linear_hip(pe, w1, None, act=1 if act else 0, slope=0.02 if act else 0.0, w_col0=Cv + Cr, k=E2,
                         addrows=voxpart, addidx=pair_vox, addrows2=raypart, addidx2=pair_ray)
        ctx.act = act
        ctx.save_for_backward(vox_feat, roi, w1, edir, pe, pair_off, pair_vox, out if act else None)
        return out

    @staticmethod
    def backward(ctx, g):
        vox_feat, roi, w1, edir, pe, pair_off, pair_vox, out = ctx.saved_tensors
        vf, rf, w = vox_feat.detach().contiguous(), roi.detach().contiguous(), w1.detach()
        Cv, Cr, E2, Ed = vf.shape[1], rf.shape[1], pe.shape[1], edir.shape[1]
        V, R = vf.shape[0], rf.shape[0]
        dz = g.detach().contiguous().float()
        if ctx.act:
            dz = _leaky_mask(dz, out, 0.02)
        d_ray, d_vox = gather2_backward(dz, pair_off, R, pair_vox, V)
        dvf = droi = dw = db = None
        if ctx.needs_input_grad[0]:
            dvf = linear_hip(d_vox, w[:, :Cv].t().contiguous())
        if ctx.needs_input_grad[1]:
            droi = linear_hip(d_ray, w[:, Cv:Cv + Cr].t().contiguous())
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dw = torch.zeros(w.shape, dtype=torch.float32, device=dz.device)
            db = torch.zeros((w.shape[0],), dtype=torch.float32, device=dz.device)
            _wgrad_into(d_vox, vf, dw, 0, db)          # (b1 enters once per voxel row: its gradient is the tables' sum)
            _wgrad_into(d_ray, rf, dw, Cv)
            _wgrad_into(dz, pe, dw, Cv + Cr)
            _wgrad_into(d_ray, edir, dw, Cv + Cr + E2)
        return dvf, droi, dw, db, None, None, None, None, None, None


class _EncLayer1Fn(torch.autograd.Function):
    """One pass of an IEF's layer 1: leaky(base + W1[:, enc columns] enc) — the 16 offset-encoding columns as their
    own small product added to the kept pass-independent base (lidf_linear_f32 with the base as its gathered term)."""

    @staticmethod
    def forward(ctx, enc, w1, base, col0, rows):
        e = enc.detach().contiguous()
        out = linear_hip(e, w1, None, act=1, slope=0.02, addrows=base.detach(), addidx=rows, w_col0=col0,
                         k=e.shape[1])
        ctx.col0 = col0
        ctx.save_for_backward(enc, w1, out)
        return out

    @staticmethod
    def backward(ctx, g):
        enc, w1, out = ctx.saved_tensors
        e, w = enc.detach().contiguous(), w1.detach()
        c0, k = ctx.col0, enc.shape[1]
        dz = _leaky_mask(g.detach().contiguous().float(), out, 0.02)
        denc = dw = None
        if ctx.needs_input_grad[0]:
            denc = linear_hip(dz, w[:, c0:c0 + k].t().contiguous())
        if ctx.needs_input_grad[1]:
            dw = torch.zeros(w.shape, dtype=torch.float32, device=dz.device)
            _wgrad_into(dz, e, dw, c0)
        return denc, dw, dz if ctx.needs_input_grad[2] else None, None, None


class _NarrowLinearFn(torch.autograd.Function):
    """act(x W^T + b) for the layers lidf_wgrad_f32's fixed-order block path does not take (fewer than 32 outputs or fewer
    than 4 inputs: the 1-wide output layer, offset_enc = Linear(1, 16)): the weight and bias gradients are the column
    sums of the per-row products [g_o x_j | g_o], formed by lidf_gather2_backward_f32 onto a single destination row —
    chunk sums in row order, chunks in order — so that these gradients too are bit-identical from run to run."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        out = linear_hip(x.detach(), weight, bias, act=act, slope=slope)
        ctx.cfg = (act, slope)
        ctx.save_for_backward(x, weight, out if act else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        x, w = x.detach(), w.detach()
        g = g.detach().contiguous().float()
        if ctx.cfg[0]:
            g = _leaky_mask(g, out, ctx.cfg[1])
        n, nout, k = x.shape[0], w.shape[0], w.shape[1]
        dx = linear_hip(g, w.t().contiguous()) if ctx.needs_input_grad[0] else None
        F = (nout * k + nout + 3) // 4 * 4
        prod = torch.zeros((n, F), dtype=torch.float32, device=g.device)
        prod[:, :nout * k] = (g[:, :, None] * x[:, None, :]).reshape(n, nout * k)
        prod[:, nout * k:nout * k + nout] = g
        _, s = gather2_backward(prod, idx=torch.zeros((n,), dtype=torch.int32, device=g.device), n_idx_rows=1)
        return dx, s[0, :nout * k].reshape(nout, k).clone(), s[0, nout * k:nout * k + nout].clone(), None, None


def _train_lin(x, layer, act=0, slope=0.0):
    """A layer under autograd: _LinearFn where lidf_wgrad_f32 sums in a fixed order, the column-sum form for the
    narrow ones."""
    nout, k = layer.weight.shape
    if (nout < 32 or k < 4) and layer.bias is not None and nout * (k + 1) <= 1024:
        return _NarrowLinearFn.apply(x, layer.weight, layer.bias, act, slope)
    return _LinearFn.apply(x, layer.weight, layer.bias, act, slope)


def _decoder_train_from_layer1(mod, layer1, n, dev):
    """decoder_forward_train behind the factorised layer 1. layer1(act) -> [n, 4 gf] under autograd."""
    from .decoders import IEF, _init_offset_value

    def rest(h):
        h = _train_lin(h, mod.linear_2, 1, 0.02)
        h = _train_lin(h, mod.linear_3, 1, 0.02)
        return _train_lin(h, mod.linear_4)
    if not isinstance(mod, IEF):
        return _out_act(mod, rest(layer1(True)))
    base = layer1(False)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    off = torch.full((n, 1), _init_offset_value(mod), dtype=torch.float32, device=dev)
    for _ in range(int(mod.n_iter)):   # (the passes share every parameter: autograd adds their gradients up)
        enc = _train_lin(off, mod.offset_enc)
        off = off + rest(_EncLayer1Fn.apply(enc, mod.linear_1.weight, base, int(mod.inp_dim), rows))
    return _out_act(mod, off)


def query_train(ray_dir, ray_pix, ray_bid, pair_off, pair_ray, pair_vox, pair_t, feat_grid, vox_feat, prob_dec,
                offset_dec, multires=8, multires_views=4, roi_inp_bbox=8, roi_out_bbox=2, offset_range=(0.0, 1.0),
                part_size=0.25, vox_center=None, pos_rel=False, max_pair_id=None, offsets="all",
                roi_backward="atomic"):
    """get_embedding + get_pred (models/pipeline.py:338-466) under autograd at any rgb_out / roi_out_bbox / pnet_out /
    gf_dim / multires: what query.lidf_query_train is at the shipped widths. Gradients reach feat_grid (through
    _RoiAlignFn), vox_feat and every parameter of both decoders. Layer 1 keeps the factorised form of `query` — the
    per-voxel and per-ray tables, only the 2E position-embedding columns per pair (_Layer1Fn) —, the layers behind it
    are one autograd function each, an IEF's passes add their 16 encoded-offset columns to the kept base
    (_EncLayer1Fn), and the tail is query._QueryTailFn (pair positions, per-ray softmax / arg-max over the detached
    logits, the max_pair_id override). Every launch goes to the caller's current stream.
    Run-to-run: bit-identical gradients when the rays are distinct pixels, both decoders have gf_dim >= 32 and
    multires_views >= 1 (lidf_roi_align_backward_f32, lidf_gather2_backward_f32 and lidf_wgrad_f32's block path sum
    in fixed orders; a 3-column direction block or a layer of fewer than 32 outputs falls to lidf_wgrad_f32's
    atomics beyond 512 rows) and at most 16,384 voxel rows.
    roi_backward ("atomic" / "ordered", query.lidf_query_train's argument) is checked and changes nothing here: this
    route's adjoint to feat_grid is the ordered gather lidf_roi_align_backward_f32 already.
    Returns lidf_query_train's dict."""
    from .decoders import get_embedder
    from .query import _QueryTailFn, _roi_backward_arg
    _roi_backward_arg(roi_backward)
    if offsets != "all":
        raise RuntimeError("offsets=%r runs inside the fixed-width training kernel only (gf_dim 64, rgb_out 32, "
                           "roi_out_bbox 2, pnet_out 128); at other widths the offset decoder runs on every pair"
                           % (offsets,))
    if prob_dec.linear_4.out_features != 1 or offset_dec.linear_4.out_features != 1:
        raise RuntimeError("the query takes decoders with out_dim == 1 (got prob_dec %d, offset_dec %d)"
                           % (prob_dec.linear_4.out_features, offset_dec.linear_4.out_features))
    dev = ray_dir.device
    R, P = ray_dir.shape[0], pair_ray.shape[0]
    E = 3 + 6 * multires
    L = _lib.lib()
    roi = _RoiAlignFn.apply(feat_grid, ray_pix, ray_bid, roi_inp_bbox, roi_out_bbox)
    edir = get_embedder(multires_views)[0](ray_dir.detach().contiguous()).detach()   # a constant of the step
    D = vox_feat.shape[1] + roi.shape[1] + 2 * E + edir.shape[1]
    for dec in (prob_dec, offset_dec):
        if D != dec.inp_dim or dec.linear_1.in_features < D:
            raise RuntimeError("decoder inp_dim must be %d for this configuration" % D)
    pe = torch.empty((P, 2 * E), dtype=torch.float32, device=dev)
    if P:
        with torch.cuda.device(dev):
            _lib.check(L.lidf_pe_rows_f32(_lib.ptr(pair_ray), _lib.ptr(pair_vox), _lib.ptr(pair_t), _lib.ptr(ray_dir),
                                          _lib.ptr(vox_center), 1 if pos_rel else 0, multires, P, _lib.ptr(pe),
                                          _lib.current_stream(dev)))
    outs = []
    for dec in (prob_dec, offset_dec):
        l1 = dec.linear_1

        def layer1(act, l1=l1):
            return _Layer1Fn.apply(vox_feat, roi, l1.weight, l1.bias, edir, pe, pair_off, pair_ray, pair_vox, act)
        outs.append(_decoder_train_from_layer1(dec, layer1, P, dev))
    pred_prob, pred_offset = outs
    pair_pred_pos, sm, mid, pred_pos = _QueryTailFn.apply(
        pred_offset, pred_prob, pair_off, pair_ray, pair_t, ray_dir, float(offset_range[0]), float(offset_range[1]),
        float(part_size), max_pair_id)
    return {"pred_offset": pred_offset, "pred_prob_end": pred_prob, "pair_pred_pos": pair_pred_pos,
            "pred_prob_end_softmax": sm, "max_pair_id": mid, "pred_pos": pred_pos}


# ------------------------------------------------------------------------------------------------------------------
# Stage 2 under autograd at any width (forward_times x get_pred_refine for the stage-2 training step)
# ------------------------------------------------------------------------------------------------------------------
def refine_step_forward(pos, st, table_ready=False):
    """lidf_refine_step_forward_f32 on the step constants st (refine_train builds them): (end_voxel [R] i32,
    pnet_inp [Nv + R, 6], pnet_vox [Nv + R] i32, pe [R, E]) — the valid points' rows copied in front."""
    dev = pos.device
    R, Nv, E = pos.shape[0], st["valid_inp"].shape[0], 3 + 6 * st["multires"]
    B, _, h, w = st["rgb_img"].shape
    pn_inp = torch.empty((Nv + R, 6), dtype=torch.float32, device=dev)
    pn_vox = torch.empty((Nv + R,), dtype=torch.int32, device=dev)
    pn_inp[:Nv] = st["valid_inp"]
    pn_vox[:Nv] = st["valid_vox"]
    end_voxel = torch.empty((R,), dtype=torch.int32, device=dev)
    pe = torch.empty((R, E), dtype=torch.float32, device=dev)
    cells = st["cells"]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lidf_refine_step_forward_f32(
            _lib.ptr(pos), _lib.ptr(st["max_pair_id"]), _lib.ptr(st["pair_vox"]), st["pair_vox"].shape[0],
            _lib.ptr(st["voxel_bound"]), _lib.ptr(st["voxel_bid"]), st["voxel_bound"].shape[0], _lib.ptr(st["ray_bid"]),
            _lib.ptr(st["ray_flat"]), _lib.ptr(st["rgb_img"]), B, h, w, R, Nv, 1 if st["pnet_pos_rel"] else 0,
            1 if st["pos_rel"] else 0, st["multires"],
            _lib.ptr(cells["coord"]) if cells else None, cells["res"] if cells else None,
            cells["xmin"] if cells else None, cells["part"] if cells else 0.0, 1 if (cells and table_ready) else 0,
            _lib.ptr(end_voxel), _lib.ptr(pn_inp), _lib.ptr(pn_vox), _lib.ptr(pe), E,
            _lib.ptr(cells["table"]) if cells else None, 4 * cells["table"].numel() if cells else 0,
            _lib.current_stream(dev)))
    return end_voxel, pn_inp, pn_vox, pe


def refine_step_backward(g_pos, st, d_off=False, pos=None, end_voxel=None, d_pe=None, d_rows=None, d_pos=False):
    """lidf_refine_step_backward_f32: (d_off [R] or None, d_pos [R, 3] or None). d_rows: the gradient of the whole
    pnet_inp [Nv + R, 6] (its predicted rows are read)."""
    dev = g_pos.device
    R, Nv = g_pos.shape[0], st["valid_inp"].shape[0]
    o = torch.empty((R,), dtype=torch.float32, device=dev) if d_off else None
    dp = torch.empty((R, 3), dtype=torch.float32, device=dev) if d_pos else None
    r0, r1 = st["offset_range"]
    rows = ctypes.c_void_p(d_rows.data_ptr() + 24 * Nv) if d_rows is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().lidf_refine_step_backward_f32(
            _lib.ptr(g_pos), _lib.ptr(st["ray_dir"]), float(r0), float(r1), _lib.ptr(o), _lib.ptr(pos),
            _lib.ptr(end_voxel), _lib.ptr(st["voxel_bound"]), 1 if st["pos_rel"] else 0, _lib.ptr(d_pe),
            st["multires"], rows, _lib.ptr(dp), R, _lib.current_stream(dev)))
    return o, dp


def _f32c(g):
    """An incoming gradient as a dense float32 tensor (None stays None)."""
    return None if g is None else g.detach().contiguous().float()


class _RayStepFn(torch.autograd.Function):
    """The per-ray step of one iteration (lidf_refine_step_forward_f32): from the position entering the iteration the
    end voxels, the PointNet rows of valid + predicted points and embed(pos (- centre)). The position itself is
    handed through as the first output, so that the gradient of the additive update (_FinishFn) arrives here together
    with those of the rows and of the embedding and d pos = g + embed'(x)^T d_pe + d_rows[:, 0:3] is ONE launch
    (lidf_refine_step_backward_f32), no row gradient gathered or added by torch."""

    @staticmethod
    def forward(ctx, cur, st, table_ready):
        x = cur.detach().contiguous()
        end_voxel, pn_inp, pn_vox, pe = refine_step_forward(x, st, table_ready)
        ctx.st = st
        ctx.save_for_backward(x, end_voxel)
        ctx.mark_non_differentiable(end_voxel, pn_vox)
        return x.view_as(x), pn_inp, pe, end_voxel, pn_vox

    @staticmethod
    def backward(ctx, g_pos, g_rows, g_pe, _g_end, _g_vox):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        x, end_voxel = ctx.saved_tensors
        g = _f32c(g_pos) if g_pos is not None else torch.zeros_like(x)
        _, d_pos = refine_step_backward(g, ctx.st, pos=x, end_voxel=end_voxel, d_pe=_f32c(g_pe), d_rows=_f32c(g_rows),
                                        d_pos=True)
        return d_pos, None, None


class _FinishFn(torch.autograd.Function):
    """pos + (off (r1 - r0) + r0) dir (pipeline.py:1028-1029); backward: d off = (r1 - r0) <g, dir>
    (lidf_refine_step_backward_f32), d pos = g."""

    @staticmethod
    def forward(ctx, pos, off, st):
        r0, r1 = st["offset_range"]
        ctx.st = st
        return pos.detach() + (off.detach() * (r1 - r0) + r0) * st["ray_dir"]

    @staticmethod
    def backward(ctx, g):
        g = g.detach().contiguous().float()
        d_off = None
        if ctx.needs_input_grad[1]:
            d_off = refine_step_backward(g, ctx.st, d_off=True)[0].view(-1, 1)
        return g if ctx.needs_input_grad[0] else None, d_off, None


TABLE_CHUNK = 16   # columns per launch of a layer-1 table product


def _table_product(x, w, bias, col0, k, addrows=None, addidx=None):
    """x[:, :k] W[:, col0 : col0 + k]^T (+ bias) (+ addrows[addidx]) for a layer-1 table of the refine step, the
    contraction split into runs of TABLE_CHUNK columns: every launch starts its matrix-instruction sums at zero and
    adds the previous runs' result in its epilogue. lidf_linear_f32 carries ONE accumulator chain over k, whose
    rounding grows with the chain's length and the running sum's size; a table row is shared by every iteration (the
    per-ray table) or by every ray of a voxel (the per-voxel table), so its rounding does not average out over the rows
    of a gradient sum the way a per-row product's does, and the second iteration's 2^7 octave multiplies it. Measured at
    (32, 2, 128, 16, 64, IEF): dec.linear_4.weight 4.04 x the float32 oracle's error with one chain of 128 columns;
    runs of 16 hold every case of tests/test_refine_widths_gpu.py, the worst at 3.46."""
    rows = None
    out = None
    for c0 in range(0, k, TABLE_CHUNK):
        kk = min(TABLE_CHUNK, k - c0)
        if out is None:
            out = linear_hip(x[:, c0:], w, bias, w_col0=col0 + c0, k=kk, addrows=addrows, addidx=addidx)
        else:
            if rows is None:
                rows = torch.arange(x.shape[0], dtype=torch.int32, device=x.device)
            out = linear_hip(x[:, c0:], w, None, w_col0=col0 + c0, k=kk, addrows=out, addidx=rows)
    return out


class _RayPartFn(torch.autograd.Function):
    """raypart = W1[:, ROI columns] roi + W1[:, direction columns] embed(dir) [R, 4 gf]: the part of a stage-2
    decoder's layer 1 that depends on feat_grid and W1 only — formed once per step, shared by the iterations. Its
    gradient is the iterations' dZ1 summed (by autograd); from it d roi and the two column blocks of dW1."""

    @staticmethod
    def forward(ctx, roi, w1, edir, col_roi, col_dir):
        rf = roi.detach().contiguous()
        rows = torch.arange(rf.shape[0], dtype=torch.int32, device=rf.device)
        rp = _table_product(rf, w1, None, col_roi, rf.shape[1])
        ctx.cols = (col_roi, col_dir)
        ctx.save_for_backward(roi, w1, edir)
        return _table_product(edir, w1, None, col_dir, edir.shape[1], addrows=rp, addidx=rows)

    @staticmethod
    def backward(ctx, g):
        roi, w1, edir = ctx.saved_tensors
        rf, w = roi.detach().contiguous(), w1.detach()
        col_roi, col_dir = ctx.cols
        d_ray = g.detach().contiguous().float()
        droi = dw = None
        if ctx.needs_input_grad[0]:
            droi = linear_hip(d_ray, w[:, col_roi:col_roi + rf.shape[1]].t().contiguous())
        if ctx.needs_input_grad[1]:
            dw = torch.zeros(w.shape, dtype=torch.float32, device=d_ray.device)
            _wgrad_into(d_ray, rf, dw, col_roi)
            _wgrad_into(d_ray, edir, dw, col_dir)
        return droi, dw, None, None, None


class _RefineLayer1Fn(torch.autograd.Function):
    """Layer 1 of a stage-2 decoder, factorised as _Layer1Fn with exactly one pair per ray:
    act(W1[:, position columns] embed(pos) + voxpart[end_voxel] + raypart) with voxpart = W1[:, voxel columns]
    occ_voxel_feat + b1 [V, 4 gf]. No [R, D] row and no row gradient: the backward sums dZ1 by end voxel
    (lidf_gather2_backward_f32: sorted, fixed order) for d occ_voxel_feat and the voxel block of dW1, hands dZ1 itself to
    raypart, and — unlike stage 1, where the per-row operand is a constant — forms d embed = dZ1 W1[:, position
    columns] for the position's gradient."""

    @staticmethod
    def forward(ctx, occ, raypart, w1, b1, pe, end_voxel, col_pos, act):
        vf = occ.detach().contiguous()
        rows = torch.arange(pe.shape[0], dtype=torch.int32, device=pe.device)
        voxpart = _table_product(vf, w1, b1, 0, vf.shape[1])
        out = linear_hip(pe.detach(), w1, None, act=1 if act else 0, slope=0.02 if act else 0.0, w_col0=col_pos,
                         k=pe.shape[1], addrows=voxpart, addidx=end_voxel, addrows2=raypart.detach(), addidx2=rows)
        ctx.cfg = (col_pos, act)
        ctx.save_for_backward(occ, w1, pe, end_voxel, out if act else None)
        return out

    @staticmethod
    def backward(ctx, g):
        occ, w1, pe, end_voxel, out = ctx.saved_tensors
        vf, w, x = occ.detach().contiguous(), w1.detach(), pe.detach()
        col_pos, act = ctx.cfg
        Cv, E = vf.shape[1], x.shape[1]
        dz = g.detach().contiguous().float()
        if act:
            dz = _leaky_mask(dz, out, 0.02)
        _, d_vox = gather2_backward(dz, idx=end_voxel, n_idx_rows=vf.shape[0])
        docc = dpe = dw = db = None
        if ctx.needs_input_grad[0]:
            docc = linear_hip(d_vox, w[:, :Cv].t().contiguous())
        if ctx.needs_input_grad[4]:
            dpe = linear_hip(dz, w[:, col_pos:col_pos + E].t().contiguous())
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dw = torch.zeros(w.shape, dtype=torch.float32, device=dz.device)
            db = torch.zeros((w.shape[0],), dtype=torch.float32, device=dz.device)
            _wgrad_into(d_vox, vf, dw, 0, db)          # (b1 enters once per voxel row: its gradient is the table's sum)
            _wgrad_into(dz, x, dw, col_pos)
        return docc, dz if ctx.needs_input_grad[1] else None, dw, db, dpe, None, None, None


def refine_train(ray_dir, ray_pix, ray_bid, ray_flat, pred_pos, max_pair_id, pair_vox, voxel_bound, voxel_bid, rgb_img,
                 feat_grid, valid_inp, valid_vox, pnet_model, offset_dec, forward_times=2, multires=8, multires_views=4,
                 roi_inp_bbox=8, roi_out_bbox=2, offset_range=(-0.2, 0.2), pos_rel=False, pnet_pos_rel=True,
                 perturb_noise=None, grid=None, roi_backward="atomic"):
    """forward_times x RefineNet.get_pred_refine (models/pipeline.py:922-1030, exp_type 'train') under autograd at any
    rgb_out / roi_out_bbox / roi_inp_bbox, PointNet2Stage(6, pnet_out, pnet_gf), IEF (any n_iter) or IMNet of any
    gf_dim with a 1-wide head, use_sigmoid on or off, multires / multires_views 0..16: what query.lidf_refine_train is
    at the shipped widths, with its arguments, returns and gradient targets (every parameter of pnet_model and
    offset_dec, pred_pos and feat_grid when they require grad; valid_inp carries none).
    A decoder row is a stage-1 pair with one pair per ray, so layer 1 keeps the factorised form (_RefineLayer1Fn /
    _RayPartFn): a per-voxel table gathered by end_voxel, a per-ray table formed once per step, and the E columns of
    embed(pos) as the per-row operand — no [R, D] row and no row gradient, forward or backward. Per iteration the rays
    take one call each way (lidf_refine_step_forward_f32 / _backward_f32: end voxel, PointNet rows, embedding; d off,
    d pos); the PointNet runs the module's own training path (generic.pointnet_forward_train where a width differs),
    layers 2-4 and an IEF's passes are query_train's (_decoder_train_from_layer1). Every launch goes to the caller's
    current stream. Run-to-run: as query_train — bit-identical gradients for rays on distinct pixels, gf_dim >= 32,
    multires_views >= 1 and at most 16,384 voxels. roi_backward ("atomic" / "ordered", query.lidf_refine_train's
    argument) is checked and changes nothing here: the adjoint to feat_grid is the ordered gather already.
    Returns pred_pos_refine [R, 3] (with grad) and the last end_voxel_id [R] i32."""
    from .decoders import get_embedder
    from .query import _as_i32, _cell_lookup, _f32, _roi_backward_arg
    _roi_backward_arg(roi_backward)
    if offset_dec.linear_4.out_features != 1:
        raise RuntimeError("the refine step takes a decoder with out_dim == 1 (got %d): its output is the offset "
                           "along the ray" % offset_dec.linear_4.out_features)
    if pnet_model.input_channels != 6:
        raise RuntimeError("pnet_model.input_channels must be 6 (the predicted points' rows are xyz + rgb), got %d"
                           % pnet_model.input_channels)
    E, Ed = 3 + 6 * multires, 3 + 6 * multires_views
    if not (0 <= multires <= 16 and 0 <= multires_views <= 16):
        raise RuntimeError("multires / multires_views must lie in 0..16")
    if feat_grid.dim() != 4:
        raise RuntimeError("feat_grid must be [B,rgb_out,h,w]")
    Cv, Cr = pnet_model.vox_lin2.out_features, feat_grid.shape[1] * roi_out_bbox * roi_out_bbox
    D = Cv + Cr + E + Ed
    if offset_dec.inp_dim != D or offset_dec.linear_1.in_features < D:
        raise RuntimeError("refine offset_dec inp_dim must be %d (pnet_out %d + rgb_out %d x roi_out_bbox^2 %d + "
                           "E %d + Ed %d), got %d" % (D, Cv, feat_grid.shape[1], roi_out_bbox * roi_out_bbox, E, Ed,
                                                      offset_dec.inp_dim))
    ray_pix, ray_bid = _as_i32(ray_pix, "ray_pix"), _as_i32(ray_bid, "ray_bid")
    ray_flat, voxel_bid = _as_i32(ray_flat, "ray_flat"), _as_i32(voxel_bid, "voxel_bid")
    pair_vox, valid_vox = _as_i32(pair_vox, "pair_vox"), _as_i32(valid_vox, "valid_vox")
    ts = dict(ray_dir=ray_dir, ray_pix=ray_pix, ray_bid=ray_bid, ray_flat=ray_flat, max_pair_id=max_pair_id,
              pair_vox=pair_vox, voxel_bound=voxel_bound, voxel_bid=voxel_bid, rgb_img=rgb_img, valid_inp=valid_inp,
              valid_vox=valid_vox)
    _lib.require_cuda(pred_pos, feat_grid, *ts.values(), names=["pred_pos", "feat_grid"] + list(ts))
    for n in ("ray_dir", "voxel_bound", "rgb_img", "valid_inp"):
        _f32(ts[n], n)
    _f32(pred_pos, "pred_pos"), _f32(feat_grid, "feat_grid")
    if max_pair_id.dtype != torch.int64:
        raise RuntimeError("max_pair_id must be int64")
    R, V, Nv = ray_dir.shape[0], voxel_bound.shape[0], valid_inp.shape[0]
    if (tuple(ray_dir.shape) != (R, 3) or tuple(pred_pos.shape) != (R, 3) or tuple(max_pair_id.shape) != (R,)
            or tuple(ray_bid.shape) != (R,) or tuple(ray_flat.shape) != (R,) or tuple(ray_pix.shape) != (R, 2)):
        raise RuntimeError("ray_dir / pred_pos must be [R,3]; ray_pix [R,2]; ray_bid / ray_flat / max_pair_id [R]")
    if tuple(voxel_bound.shape) != (V, 6) or tuple(voxel_bid.shape) != (V,):
        raise RuntimeError("voxel_bound / voxel_bid must be [V,6] / [V]")
    if tuple(valid_inp.shape) != (Nv, 6) or tuple(valid_vox.shape) != (Nv,):
        raise RuntimeError("valid_inp / valid_vox must be [Nv,6] / [Nv]")
    if rgb_img.dim() != 4 or rgb_img.shape[1] != 3:
        raise RuntimeError("rgb_img must be [B,3,h,w]")
    if valid_inp.requires_grad:
        raise RuntimeError("refine_train: valid_inp carries no gradient (the valid points are inputs of the frozen "
                           "stage 1, trainers/train_refine.py:73)")
    dev = ray_dir.device
    cur = pred_pos
    if perturb_noise is not None:
        cur = cur + float(perturb_noise) * ray_dir
    if R == 0:   # nothing to refine: empty outputs that still carry a graph to every parameter
        zero = sum(q.sum() for m in (pnet_model, offset_dec) for q in m.parameters()) * 0.0
        return cur + zero + 0.0 * feat_grid.sum(), torch.empty((0,), dtype=torch.int32, device=dev)
    st = {k: v.detach() for k, v in ts.items()}
    st.update(multires=int(multires), pos_rel=bool(pos_rel), pnet_pos_rel=bool(pnet_pos_rel),
              offset_range=(float(offset_range[0]), float(offset_range[1])),
              cells=_cell_lookup(grid, V, rgb_img.shape[0], dev, voxel_bound))
    l1 = offset_dec.linear_1
    roi = _RoiAlignFn.apply(feat_grid, ray_pix, ray_bid, roi_inp_bbox, roi_out_bbox)
    edir = get_embedder(multires_views)[0](ray_dir.detach().contiguous()).detach()   # a constant of the step
    raypart = _RayPartFn.apply(roi, l1.weight, edir, Cv, Cv + Cr + E)
    end_voxel = None
    for it in range(int(forward_times)):
        pos, pn_inp, pe, end_voxel, pn_vox = _RayStepFn.apply(cur, st, it > 0)
        occ = pnet_model(pn_inp, pn_vox, n_vox=V)

        def layer1(act, occ=occ, pe=pe, end_voxel=end_voxel):
            return _RefineLayer1Fn.apply(occ, raypart, l1.weight, l1.bias, pe, end_voxel, Cv + Cr, act)
        off = _decoder_train_from_layer1(offset_dec, layer1, R, dev)
        cur = _FinishFn.apply(pos, off, st)
    return cur, end_voxel
