"""precision="f16x3" at decoders of gf_dim 32 / 64 / 128 (csrc/lidf_chain16_h.hip, lidf_decoder_chain_split_f32) against
float64: the yardstick of tests/test_f64_split_gpu.py with the twin of THIS kernel (tests/split_chain_ref.py). The unit
of split_f16_ref.assert_split_close is the twin's error plus the float32 oracle's, both against the float64 oracle on
the same inputs; the kernel may be F64_K = 4 times that, elementwise and normwise. tests/test_chain_split_ref.py shows on
the CPU that a lost or flushed low piece is rejected by it.

References and twin are evaluated on the GPU with torch's own ops (TF32 off). Forward only: no element is left out of
any comparison. Decoder outputs are compared as logits (util.inv_out_act); the product's own arg-max is fed to the
references and checked on its own (util.check_selection)."""
import functools
import gc

import pytest
import torch

import pointnet_ref as ref
import roi_ref
import split_chain_ref as sc
import stream_order as so
import ws_poison
from util import check_selection, decoder_preacts, inv_out_act, make_module, make_pointnet, orc, tf32_off, to_dev

pytestmark = pytest.mark.gpu

REPORT = {"decoders": [], "tables": [], "query": [], "range edge": [], "stage 2": [], "reference runs": []}
WIDTHS = (32, 64, 128)
KINDS = (("IMNET", 1), ("IEF", 1), ("IEF", 2), ("IEF", 3))


@pytest.fixture(autouse=True)
def _full_precision_references():
    with tf32_off():
        yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _print_report():
    yield
    for group, rows in REPORT.items():
        if rows:
            worst = max(rows, key=lambda r: r["ratio_max"])
            print("\nf16x3 chain vs float64, %s: %d tensors, worst ratio elementwise %.2f (%s) / normwise %.2f"
                  % (group, len(rows), worst["ratio_max"], worst["what"], max(r["ratio_nrm"] for r in rows)))


def _dev(p, dev, dt):
    return {k: v.to(dev, dt) for k, v in p.items()}


def _logits(v, sig):
    return v.double() if sig else inv_out_act(v)


@functools.lru_cache(maxsize=None)
def _params(kind, d, gf, scale):
    return orc.randomize_biases(orc.init_decoder(kind, d, 81, scale, gf=gf), 82)


@functools.lru_cache(maxsize=None)
def _rows(n, d):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(n + d))


def _chain(mod, x, precision="f16x3", **kw):
    """generic.decoder_chain on rows whose every column is a per-row operand (k = D, the bias row as voxpart)."""
    from implicit_depth_amd import generic
    with torch.no_grad():
        return generic.decoder_chain(mod, x, x.shape[1], voxpart=generic._bias_row(mod).reshape(1, -1).contiguous(),
                                     precision=precision, **kw)


def _forward(mod, x, kind):
    from implicit_depth_amd.decoders import decoders_forward
    kw = {"prob_dec": mod} if kind == "IMNET" else {"offset_dec": mod}
    with torch.no_grad():
        return [o for o in decoders_forward(x, precision="f16x3", **kw) if o is not None][0]


F16_MAX = 65504.0


def _split_top(p, x, kind, n_iter):
    """The largest magnitude the kernel splits into f16 pieces, by the float64 oracle: the per-row operand and the
    pre-activations of layers 1 and 2 of every pass (layer 3's go to the f32 layer 4)."""
    zs, _ = decoder_preacts(_dev(p, x.device, torch.float64), x.double(), kind, n_iter)
    return max([x.abs().max().item()] + [z.abs().max().item() for i, z in enumerate(zs) if i % 3 != 2])


def _check_decoder(what, got, p, x, kind, n_iter, sig, gf, group="decoders"):
    with torch.no_grad():
        r64 = orc.decoder_forward(_dev(p, x.device, torch.float64), x.double(), kind, n_iter, sig)
        r32 = orc.decoder_forward(_dev(p, x.device, torch.float32), x, kind, n_iter, sig)
        twin = sc.chain_decoder(p, x, kind, n_iter, sig, gf)
    assert torch.isfinite(got).all(), what
    sc.assert_split_close(what, _logits(got, sig), _logits(r64, sig), _logits(r32, sig), _logits(twin, sig),
                          report=REPORT[group])


# ---------------------------------------------------------------------------------------------------------------
# the decoder boundary
# ---------------------------------------------------------------------------------------------------------------
N_BOUNDARY = 257       # sixteen 16-row sub-tiles and one row: five workgroups, an odd sub-tile


def _strided(x):
    """The rows as a view of a wider NaN-filled buffer: row stride 404, first column 7."""
    wide = torch.full((x.shape[0], 404), float("nan"), device=x.device)
    wide[:, 7:7 + x.shape[1]] = x
    return wide[:, 7:7 + x.shape[1]]


def _boundary(cuda, gf, k, run):
    """Every kind x activation x weight scale at one (gf, k): a strided view and plain rows (padded=False both: the
    trailing rows go through the padded copy), each held to float64 and bit-equal to each other."""
    x = _rows(N_BOUNDARY, k).to(cuda)
    xs = _strided(x)
    for kind, n_iter in KINDS:
        for sig in (False, True):
            for scale in (1.0, 5.0, 20.0):
                p = _params(kind, k, gf, scale)
                mod = make_module(kind, p, k, cuda, n_iter=n_iter, use_sigmoid=sig, gf=gf)
                got = run(mod, x, kind)
                what = "gf %d k %d %s x%d%s x%g" % (gf, k, kind, n_iter, " sigmoid" if sig else "", scale)
                assert got.shape == (N_BOUNDARY, 1)
                assert torch.equal(run(mod, xs, kind).view(torch.int32), got.view(torch.int32)), what + ": the strided view"
                top = _split_top(p, x, kind, n_iter)
                if top >= F16_MAX:
                    # outside the accuracy contract (lidf_hip.h: |activations| < 65504) by the float64 oracle's own
                    # values: a high piece is infinite, the twin is NaN there as well. Only the widest weights over
                    # three iterations get there (layer 2's pre-activations at 9e4 .. 1.5e6); nothing else may.
                    assert scale == 20.0 and n_iter == 3, (what, top)
                    print("%s: split activations reach %.3g, outside the f16 range: bits compared, not values" % (what, top))
                    continue
                _check_decoder(what, got, p, x, kind, n_iter, sig, gf)


# k = 51 / 102: the refine and query operand widths; 385: more k-groups than the prefetched seven and a one-column
# tail; 17: two groups
@pytest.mark.parametrize("k", [17, 51, 102, 385])
@pytest.mark.parametrize("gf", WIDTHS)
def test_decoder_chain_boundary(cuda, gf, k):
    _boundary(cuda, gf, k, lambda mod, x, kind: _chain(mod, x, padded=False))


@pytest.mark.parametrize("k", [17, 51, 102, 385])
@pytest.mark.parametrize("gf", [32, 128])
def test_decoders_forward_boundary(cuda, gf, k):
    _boundary(cuda, gf, k, _forward)


@pytest.mark.parametrize("gf", WIDTHS)
def test_row_edges(cuda, gf):
    """Sub-tile (16 rows), sub-tile pair and odd remainder: a row's result does not depend on its neighbours, so the
    first n rows of the 1,000-row call are the n-row call bit for bit."""
    k = 102
    p = _params("IEF", k, gf, 5.0)
    mod = make_module("IEF", p, k, cuda, gf=gf)
    x = _rows(1000, k).to(cuda)
    whole = _chain(mod, x)
    _check_decoder("gf %d 1,000 rows" % gf, whole, p, x, "IEF", 2, False, gf)
    for n in (1, 15, 16, 17, 31, 32, 33, 47):
        got = _chain(mod, x[:n].contiguous())
        assert got.shape == (n, 1)
        assert torch.equal(got, whole[:n]), (gf, n)


@pytest.mark.parametrize("gf", [32, 128])
def test_a_wavefront_walks_several_tiles(cuda, gf):
    """40,001 rows = 2,501 sub-tiles against at most 4 x 256 SIMD ranges: every wavefront's ring runs on from a pass
    section into layer 1 of its next tile."""
    k, n = 102, 40001
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert (n + 15) // 16 > 2 * 4 * cus, cus
    p = _params("IEF", k, gf, 5.0)
    mod = make_module("IEF", p, k, cuda, gf=gf)
    x = torch.randn(n, k, generator=torch.Generator().manual_seed(7)).to(cuda)
    x[:1000] = _rows(1000, k).to(cuda)
    got = _chain(mod, x)
    assert torch.equal(got[:1000], _chain(mod, x[:1000].contiguous()))
    pick = torch.randperm(n, generator=torch.Generator().manual_seed(8))[:2000].to(cuda)
    _check_decoder("gf %d 40,001 rows, 2,000 of them" % gf, got[pick], p, x[pick], "IEF", 2, False, gf)


@pytest.mark.parametrize("gf", WIDTHS)
def test_range_edge(cuda, gf):
    """Weights x55 (test_f64_split_gpu.py::test_decoder_range_edge): the activations that are split reach the
    thousands, inside the f16 range, where the header promises unchanged relative accuracy."""
    kind, d = "IMNET", 385
    p = _params(kind, d, gf, 55.0)
    x = _rows(1000, d).to(cuda)
    zs, _ = decoder_preacts(_dev(p, cuda, torch.float64), x.double(), kind)
    top = max(z.abs().max().item() for z in zs[:2])          # the pre-activations of layers 1 and 2 are split
    assert 2.0 ** 9 <= top < 65504, top
    got = _chain(make_module(kind, p, d, cuda, gf=gf), x)
    _check_decoder("gf %d x55 (max split |z| %.0f)" % (gf, top), got, p, x, kind, 1, False, gf, group="range edge")


@pytest.mark.parametrize("gf", WIDTHS)
def test_not_the_f32_kernel_by_accident(cuda, gf):
    p = _params("IEF", 102, gf, 5.0)
    mod = make_module("IEF", p, 102, cuda, gf=gf)
    x = _rows(1000, 102).to(cuda)
    split, exact = _chain(mod, x), _chain(mod, x, precision="f32")
    assert not torch.equal(split, exact)
    assert (split - exact).abs().max().item() <= 1e-3         # (and no other function either)


# ---------------------------------------------------------------------------------------------------------------
# gathered tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["both, indexed", "ray rows in order", "voxpart alone"])
@pytest.mark.parametrize("gf", WIDTHS)
def test_gathered_tables(cuda, gf, tables):
    """A decoder row is [per-voxel columns | per-row columns | per-ray columns]: the outer blocks arrive as rows of two
    exact-f32 tables. Repeated and out-of-order indices; ray_idx=None (row i takes table row i); voxpart alone."""
    from implicit_depth_amd.generic import _bias_row, decoder_chain, linear_hip
    kv, k, kr = 24, 51, (0 if tables == "voxpart alone" else 19)
    n, V = 333, 11
    R = n if tables == "ray rows in order" else 40
    g = torch.Generator().manual_seed(gf + len(tables))
    D = kv + k + kr
    p = _params("IEF", D, gf, 5.0)
    mod = make_module("IEF", p, D, cuda, gf=gf)
    fv, gr, x = (torch.randn(V, kv, generator=g).to(cuda), torch.randn(R, max(kr, 1), generator=g).to(cuda),
                 torch.randn(n, k, generator=g).to(cuda))
    vi = torch.randint(0, V, (n,), generator=g).to(cuda)                  # repeated, out of order
    ri = torch.arange(n).to(cuda) if tables == "ray rows in order" else torch.randint(0, R, (n,), generator=g).to(cuda)
    w1 = mod.linear_1.weight
    voxpart = linear_hip(fv, w1, _bias_row(mod), k=kv)
    raypart = linear_hip(gr, w1, None, w_col0=kv + k, k=kr) if kr else None
    with torch.no_grad():
        got = decoder_chain(mod, x, k, w1_col0=kv, voxpart=voxpart, vox_idx=vi.int(), raypart=raypart,
                            ray_idx=ri.int() if tables == "both, indexed" else None, precision="f16x3")
        rows = torch.cat([fv[vi], x] + ([gr[ri]] if kr else []), 1)
        r64 = orc.decoder_forward(_dev(p, cuda, torch.float64), rows.double(), "IEF", 2)
        r32 = orc.decoder_forward(_dev(p, cuda, torch.float32), rows, "IEF", 2)
        twin = sc.chain_rows(p, x, "IEF", 2, False, gf, kv, voxpart[vi], raypart[ri] if kr else None)
    sc.assert_split_close("gf %d %s" % (gf, tables), inv_out_act(got), inv_out_act(r64), inv_out_act(r32),
                          inv_out_act(twin), report=REPORT["tables"])


# ---------------------------------------------------------------------------------------------------------------
# the query
# ---------------------------------------------------------------------------------------------------------------
# (gf, feat_grid channels, roi_out_bbox, vox_feat width, pos_rel): gf 32 and 128 at the shipped features; configuration A
# of the width goldens; gf 64 decoders at rgb_out 16 (the 64-wide chain: the shipped kernels need rgb_out 32)
QUERY_CONFIGS = {"gf32": (32, 32, 2, 128, False), "gf128": (128, 32, 2, 128, False), "A": (32, 16, 3, 64, True),
                 "gf64_rgb16": (64, 16, 2, 128, False)}


@functools.lru_cache(maxsize=None)
def _query_scene(name, scale=5.0):
    import torch.nn.functional as F
    gf, Cr, roi_out, Co, pos_rel = QUERY_CONFIGS[name]
    s = orc.synthetic_scene(2, 13, 17, 6, seed=40 + gf, ragged=True, weight_scale=scale)
    g = torch.Generator().manual_seed(Cr + Co)
    s["vox_feat"] = torch.relu(torch.randn(s["V"], Co, generator=g))
    coarse = torch.randn(2, Cr, 4, 5, generator=g)
    s["feat_grid"] = F.interpolate(coarse, size=(13, 17), mode="bilinear", align_corners=False).contiguous()
    s["D"] = Co + Cr * roi_out * roi_out + 2 * orc.embed_dim(8) + orc.embed_dim(4)
    s["prob_p"] = orc.randomize_biases(orc.init_decoder("IMNET", s["D"], 7, scale, gf=gf), 41)
    s["off_p"] = orc.randomize_biases(orc.init_decoder("IEF", s["D"], 8, scale, gf=gf), 42)
    assert (s["pair_off"][1:] == s["pair_off"][:-1]).any()               # rays without pairs
    return s


def _run_query(name, cuda, precision="f16x3"):
    from implicit_depth_amd.query import lidf_query
    gf, _, roi_out, _, pos_rel = QUERY_CONFIGS[name]
    scene = _query_scene(name)
    s = to_dev(scene, cuda)
    prob = make_module("IMNET", scene["prob_p"], scene["D"], cuda, gf=gf)
    off = make_module("IEF", scene["off_p"], scene["D"], cuda, gf=gf)
    depth = torch.zeros((2, 13, 17), device=cuda)
    with torch.no_grad():
        got = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                         s["pair_t"], s["feat_grid"], s["vox_feat"], prob, off, ray_flat=s["ray_flat"], depth=depth,
                         roi_out_bbox=roi_out, vox_center=s["vox_center"], pos_rel=pos_rel, precision=precision)
    got["depth"] = depth
    return scene, s, got


@pytest.mark.parametrize("name", list(QUERY_CONFIGS))
def test_query(cuda, name):
    gf, _, roi_out, _, pos_rel = QUERY_CONFIGS[name]
    scene, s, got = _run_query(name, cuda)
    with torch.no_grad():
        common = dict(n_iter=2, fast_roi=True, roi_out_bbox=roi_out, pos_rel=pos_rel,
                      max_pair_id=got["max_pair_id"].long())
        args = lambda c, dt: (c(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(),  # noqa: E731
                              s["pair_vox"].long(), c(s["pair_t"]), s["pair_off"], c(s["feat_grid"]),
                              c(s["vox_feat"]), _dev(scene["prob_p"], cuda, dt), _dev(scene["off_p"], cuda, dt))
        with roi_ref.patched(orc):       # (roi_out_bbox 3: the RoIAlign in torch ops, on the device, in the run's dtype)
            r64 = orc.query(*args(lambda v: v.double(), torch.float64), vox_center=s["vox_center"].double(), **common)
            r32 = orc.query(*args(lambda v: v, torch.float32), vox_center=s["vox_center"], **common)
            twin = sc.chain_query(*args(lambda v: v, torch.float32), vox_center=s["vox_center"], **common)
    for k in ("pred_offset", "pred_prob_end"):
        sc.assert_split_close("%s %s logit" % (name, k), inv_out_act(got[k]), inv_out_act(r64[k]), inv_out_act(r32[k]),
                              inv_out_act(twin[k]), report=REPORT["query"])
    for k in ("pair_pred_pos", "pred_pos"):
        sc.assert_split_close("%s %s" % (name, k), got[k], r64[k], r32[k], twin[k], report=REPORT["query"])
    check_selection(scene, got, r64, r32)
    z = got["depth"].view(-1)[(s["ray_bid"].long() * 13 * 17 + s["ray_flat"].long())]
    assert torch.equal(z, got["pred_pos"][:, 2])                        # the depth write-back


def test_query_in_slabs_reuses_the_packed_stream(cuda, monkeypatch):
    """Slabs of 64 pairs: one pack per decoder and query, every later slab runs prepacked; the same bits as one slab."""
    from implicit_depth_amd import generic
    _, _, whole = _run_query("gf32", cuda)
    assert whole["pred_offset"].shape[0] > 300
    monkeypatch.setattr(generic, "QUERY_SLAB", 64)
    _, _, part = _run_query("gf32", cuda)
    for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_prob_end_softmax", "pred_pos", "max_pair_id", "depth"):
        assert torch.equal(part[k], whole[k]), k


def test_query_without_pairs(cuda):
    from implicit_depth_amd.query import lidf_query
    scene = orc.synthetic_scene(1, 6, 8, 4, seed=3)
    R, D = scene["R"], scene["D"]
    s = to_dev(scene, cuda)
    prob = make_module("IMNET", orc.init_decoder("IMNET", D, 7, 5.0, gf=32), D, cuda, gf=32)
    off = make_module("IEF", orc.init_decoder("IEF", D, 8, 5.0, gf=32), D, cuda, gf=32)
    empty_i = torch.zeros((0,), dtype=torch.int32, device=cuda)
    with torch.no_grad():
        out = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], torch.zeros((R + 1,), dtype=torch.int32, device=cuda),
                         empty_i, empty_i, torch.zeros((0, 2), device=cuda), s["feat_grid"], s["vox_feat"], prob, off,
                         precision="f16x3")
    assert out["pred_offset"].shape == (0, 1) and out["pair_pred_pos"].shape == (0, 3)
    assert (out["max_pair_id"] == 0).all() and float(out["pred_pos"].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# stage 2: lidf_refine at f16x3 with an IEF of gf_dim 32 / 128 (the PointNet stays f32)
# ---------------------------------------------------------------------------------------------------------------
REFINE_KEYS = ("ray_dir", "ray_pix", "ray_bid", "ray_flat", "pred_pos", "max_pair_id", "pair_vox", "voxel_bound",
               "voxel_bid", "rgb_img", "feat_grid", "valid_inp", "valid_vox")


@functools.lru_cache(maxsize=None)
def _refine_refs(gf):
    """The 960-ray scene of tests/test_f64_stage2_gpu.py with an IEF of gf_dim `gf`, conditioned for it (rays at a
    decoder kink or a voxel face dropped), through orc.refine_step on the CPU, two iterations: (case, float64
    positions, end voxels, float32 positions, twin positions). The twin applies to the IEF only: the last iteration's
    float64 decoder rows, as the f32 rows the kernel reads, through chain_decoder, on the float64 incoming position."""
    case = ref.refine_case()
    case["off_p"] = orc.randomize_biases(orc.init_decoder("IEF", 334, 77, 5.0, gf=gf), 78)
    keep_ray, keep_valid, _ = ref.condition_refine(case, 2)
    case = ref.subset_case(case, keep_ray, keep_valid)
    with torch.no_grad():
        tr = []
        p64, e64 = ref.refine_chain(case, torch.float64, 2, trace=tr)
        p32, e32 = ref.refine_chain(case, torch.float32, 2)
        off = sc.chain_decoder(case["off_p"], tr[-1]["rows"].float(), "IEF", 2, False, gf)
    assert torch.equal(e64[-1], e32[-1])
    return case, p64, e64[-1], p32, tr[-1]["pos"] + (off * 0.4 - 0.2) * case["ray_dir"].double()


@pytest.mark.parametrize("gf", [32, 128])
def test_refine_inference(cuda, gf):
    from implicit_depth_amd.query import lidf_refine
    case, p64, e64, p32, twin = _refine_refs(gf)
    t = {k: case[k].to(cuda) for k in REFINE_KEYS}
    t["pred_pos"] = (case["pred_pos"] + case["noise"] * case["ray_dir"]).contiguous().to(cuda)
    pnet, dec = make_pointnet(case["pnet_p"], cuda), make_module("IEF", case["off_p"], 334, cuda, gf=gf)
    with torch.no_grad():
        pos, ev = lidf_refine(*[t[k] for k in REFINE_KEYS], pnet, dec, forward_times=2, precision="f16x3")
        pos32, ev32 = lidf_refine(*[t[k] for k in REFINE_KEYS], pnet, dec, forward_times=2)
    assert torch.equal(ev, ev32) and torch.equal(ev.cpu().long(), e64)
    assert not torch.equal(pos, pos32)
    sc.assert_split_close("refine gf %d x2 pos" % gf, pos, p64, p32, twin, report=REPORT["stage 2"])


# ---------------------------------------------------------------------------------------------------------------
# the reference's own runs at other widths (tests/golden/g13_*, g14_widths_eval.npz)
# ---------------------------------------------------------------------------------------------------------------
def _g13_keys():
    from test_golden_widths import G13_KEYS
    return G13_KEYS


@pytest.mark.parametrize("key", _g13_keys())
def test_g13_forward_split_chain(cuda, key):
    """The five decoder fixtures through the split chain: the fixture is the float32 side, as test_golden_widths_gpu.py
    takes it for the f32 chain."""
    from test_golden_widths import g13_case, g13_tensors
    c = g13_case(key)
    mod = make_module(c["kind"], c["p"], c["d"], cuda, n_iter=c["n_iter"], use_sigmoid=c["sig"], gf=c["gf"])
    x = c["x"].to(cuda)
    got = _forward(mod, x, c["kind"]).cpu()
    with torch.no_grad():
        twin = sc.chain_decoder(c["p"], x, c["kind"], c["n_iter"], c["sig"], c["gf"]).cpu()
    _, fix, o64, _, _, through = next(t for t in g13_tensors(c) if t[0] == "y")
    sc.assert_split_close("g13 %s split chain y" % key, through(got), through(o64), through(fix), through(twin),
                          report=REPORT["reference runs"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_g14_stepwise_f16x3(cuda, name):
    """pipeline.lidf_forward + refine_forward(precision="f16x3") on the evaluation fixture, configurations A and B,
    under the comparisons test_golden_widths_gpu.py applies to the stepwise f32 route (its own helpers)."""
    import test_golden_widths_gpu as tg
    from implicit_depth_amd import pipeline as pl
    fix, o64, models, kw = tg._g14_setup(name, cuda)
    batch, feat = tg._dev(fix["batch"], cuda), fix["full_rgb_feat"].to(cuda)
    pnet, prob, off, pnetr, offr = models
    report = []
    for it in (1, 2):
        opt = pl.LidfOptions(refine_forward_times=it, **kw)
        with torch.no_grad():
            ok, dd = pl.lidf_forward(batch, feat, pnet, prob, off, opt, precision="f16x3")
            assert ok
            pl.refine_forward(dd, pnetr, offr, opt, precision="f16x3")
        if it == 1:
            tg._g14_stage1("g14 %s stepwise f16x3" % name, dd, fix, o64, report)
        tg._g14_stage2("g14 %s stepwise f16x3" % name, dd, it, fix, o64, report)
    tg._show(report)


# ---------------------------------------------------------------------------------------------------------------
# workspace and stream hygiene of the new entry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gf", WIDTHS)
def test_workspace_contents_do_not_matter(cuda, monkeypatch, gf):
    """A workspace of 0xFF bytes (prepacked = 0: the first call of a fresh state) gives the clean run's bits."""
    p = _params("IEF", 102, gf, 5.0)
    mod = make_module("IEF", p, 102, cuda, gf=gf)
    x = _rows(1000, 102).to(cuda)
    poison = ws_poison.Poisoner("zeros", seed=gf).install(monkeypatch)
    base = _chain(mod, x)
    torch.cuda.synchronize()
    assert poison.handed, "the entry took no workspace from _lib.workspace"
    for mode in ("ones", "high", "random"):
        poison.begin(mode)
        got = _chain(mod, x)
        torch.cuda.synchronize()
        assert len(poison.handed) == 1 and torch.equal(got, base), mode


@pytest.mark.parametrize("gf", WIDTHS)
def test_late_inputs_on_another_stream(cuda, monkeypatch, gf):
    """The call on a non-default stream whose inputs and parameters arrive behind a bounded delay: the default-stream
    run's bits (every launch, the pack included, goes to the caller's stream)."""
    from entry_cases import Entry
    p = _params("IEF", 102, gf, 5.0)
    mod = make_module("IEF", p, 102, cuda, gf=gf)

    def call(live):
        return _chain(mod, live["x"])

    entry = Entry({"x": _rows(2049, 102)}, call, lambda got: None, modules=(mod,))
    rec = so.Recorder().install(monkeypatch)
    base = so.baseline(entry, cuda)
    _check_decoder("gf %d default stream" % gf, base, p, entry.inputs["x"].to(cuda), "IEF", 2, False, gf)
    host_ms, fresh = so.enqueue_ms(entry, cuda)
    so.compare(fresh, base, entry, "split chain gf %d on a fresh stream, no delay" % gf)
    ms = so.delay_ms(host_ms, "split chain gf %d" % gf, "late inputs")
    got, running = so.late_inputs(entry, cuda, ms, rec)
    so.compare(got, base, entry, "split chain gf %d with late inputs" % gf)
    assert running, "inconclusive: the %g ms delay had ended when the enqueue returned" % ms


# ---------------------------------------------------------------------------------------------------------------
# refusals that remain
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(cuda, monkeypatch):
    from implicit_depth_amd import IMNet, generic
    from implicit_depth_amd import query as Q
    from implicit_depth_amd.decoders import decoders_forward
    x = _rows(33, 51).to(cuda)
    narrow = make_module("IMNET", orc.init_decoder("IMNET", 51, 7, 5.0, gf=48), 51, cuda, gf=48)
    with pytest.raises(RuntimeError, match="gf_dim 32 / 64 / 128.*got gf_dim=48"):
        decoders_forward(x, prob_dec=narrow, precision="f16x3")
    wide_head = IMNet(51, 2, 32).to(cuda).eval()
    with pytest.raises(RuntimeError, match="1-wide head"):
        decoders_forward(x, prob_dec=wide_head, precision="f16x3")
    ok = make_module("IMNET", _params("IMNET", 51, 32, 5.0), 51, cuda, gf=32)
    with pytest.raises(ValueError):
        decoders_forward(x, prob_dec=ok, precision="bf16")
    monkeypatch.setenv("LIDF_CHAIN16", "0")
    with pytest.raises(RuntimeError, match="LIDF_CHAIN16=0.*no layer-by-layer split path"):
        decoders_forward(x, prob_dec=ok, precision="f16x3")
    with pytest.raises(RuntimeError, match="LIDF_CHAIN16=0"):
        _chain(ok, x)
    monkeypatch.delenv("LIDF_CHAIN16")
    assert decoders_forward(x, prob_dec=ok, precision="f16x3")[0].shape == (33, 1)
    # the training entries have no precision argument
    import inspect
    for fn in (Q.lidf_query_train, generic.query_train, generic.decoder_forward_train):
        assert "precision" not in inspect.signature(fn).parameters, fn.__name__


def test_query_refusals(cuda, monkeypatch):
    """offsets='selected' at other widths, and a query whose decoders the chain does not take."""
    from implicit_depth_amd.query import lidf_query
    scene = _query_scene("gf32")
    s = to_dev(scene, cuda)
    prob = make_module("IMNET", scene["prob_p"], scene["D"], cuda, gf=32)
    off = make_module("IEF", scene["off_p"], scene["D"], cuda, gf=32)
    args = (s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"], s["pair_t"],
            s["feat_grid"], s["vox_feat"], prob, off)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="offsets='selected'.*shipped widths"):
            lidf_query(*args, precision="f16x3", offsets="selected")
        monkeypatch.setenv("LIDF_CHAIN16", "0")
        with pytest.raises(RuntimeError, match="LIDF_CHAIN16=0"):
            lidf_query(*args, precision="f16x3")
