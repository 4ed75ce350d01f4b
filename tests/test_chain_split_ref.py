"""The twin of the split-f16 decoder chain (tests/split_chain_ref.py) and the criterion it feeds, on the CPU: the honest
twin is as accurate as the float32 oracle to within util.F64_K at gf_dim 32 / 64 / 128, and assert_split_close rejects
every way this kernel can lose a low piece. Decoder outputs are compared as logits (util.inv_out_act)."""
import functools

import pytest
import torch

import split_chain_ref as sc
from util import F64_K, f64, f64_errors, inv_out_act, orc

N_ROWS = 2000
D_ROWS = 385
WIDTHS = (32, 64, 128)


@functools.lru_cache(maxsize=None)
def _decoder_case(kind, gf, scale, n_iter):
    """(p, x, float64 output, float32 output) of the oracle on N_ROWS random rows; computed once, written by nobody."""
    p = orc.randomize_biases(orc.init_decoder(kind, D_ROWS, 11, scale, gf=gf), 12)
    x = torch.randn(N_ROWS, D_ROWS, generator=torch.Generator().manual_seed(gf))
    with torch.no_grad():
        return (p, x, orc.decoder_forward(f64(p), x.double(), kind, n_iter), orc.decoder_forward(p, x, kind, n_iter))


def _query(fn, s, cast=lambda v: v, **kw):
    return fn(cast(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(), s["pair_vox"].long(),
              cast(s["pair_t"]), s["pair_off"], cast(s["feat_grid"]), cast(s["vox_feat"]), cast(s["prob_p"]),
              cast(s["off_p"]), fast_roi=True, **kw)


@functools.lru_cache(maxsize=None)
def _scene_case(gf, scale):
    """A 1 x 16 x 24 x 16 scene (6,144 pairs) with decoders of gf_dim `gf` at weight scale `scale`, random biases, and
    the oracle's float64 / float32 query on it (the float64 arg-max given to both)."""
    s = orc.synthetic_scene(1, 16, 24, 16, seed=1234, weight_scale=scale)
    s["prob_p"] = orc.randomize_biases(orc.init_decoder("IMNET", s["D"], 7, scale, gf=gf), 5)
    s["off_p"] = orc.randomize_biases(orc.init_decoder("IEF", s["D"], 8, scale, gf=gf), 6)
    with torch.no_grad():
        r64 = _query(orc.query, s, cast=f64)
        r32 = _query(orc.query, s, max_pair_id=r64["max_pair_id"])
    return s, r64, r32


def _rejected(what, bad, r64, r32, twin):
    try:
        sc.assert_split_close(what, inv_out_act(bad), inv_out_act(r64), inv_out_act(r32), inv_out_act(twin))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("scale", [1.0, 5.0])
@pytest.mark.parametrize("kind,n_iter", [("IMNET", 1), ("IEF", 1), ("IEF", 2), ("IEF", 3)])
@pytest.mark.parametrize("gf", WIDTHS)
def test_honest_twin_within_k_of_the_f32_oracle(gf, kind, n_iter, scale):
    """defect=None: the twin computes something other than float64 and is within F64_K x the float32 oracle's error
    of float64, elementwise and normwise — the unit of assert_split_close is neither vacuous nor out of reach."""
    p, x, r64, r32 = _decoder_case(kind, gf, scale, n_iter)
    twin = sc.chain_decoder(p, x, kind, n_iter, False, gf)
    assert twin.dtype == torch.float64 and twin.shape == r64.shape
    l64, l32, lt = inv_out_act(r64), inv_out_act(r32), inv_out_act(twin)
    e_t, e_32, n_t, n_32, _ = f64_errors(lt, l64, l32)
    print("gf %d %s n_iter %d x%g: twin vs float64 %.3g / %.3g, f32 oracle %.3g / %.3g"
          % (gf, kind, n_iter, scale, e_t, n_t, e_32, n_32))
    assert 0 < e_t <= F64_K * e_32 and 0 < n_t <= F64_K * n_32, (e_t, e_32, n_t, n_32)
    sc.assert_split_close("gf %d %s" % (gf, kind), lt, l64, l32, lt, k=1.0)


def test_honest_query_twin():
    """chain_query (the factorised layer 1, gf 32) under the same condition on both decoders of a scene."""
    s, r64, r32 = _scene_case(32, 5.0)
    twin = _query(sc.chain_query, s, max_pair_id=r64["max_pair_id"])
    for k in ("pred_offset", "pred_prob_end"):
        l64, l32, lt = inv_out_act(r64[k]), inv_out_act(r32[k]), inv_out_act(twin[k])
        e_t, e_32, n_t, n_32, _ = f64_errors(lt, l64, l32)
        assert 0 < e_t <= F64_K * e_32 and 0 < n_t <= F64_K * n_32, (k, e_t, e_32, n_t, n_32)
    for k in ("pair_pred_pos", "pred_pos", "pred_prob_end_softmax"):
        sc.assert_split_close(k, twin[k], r64[k], r32[k], twin[k], k=1.0)


def test_unknown_defects_and_widths_are_refused():
    p, x, _, _ = _decoder_case("IEF", 32, 5.0, 2)
    with pytest.raises(ValueError):
        sc.chain_decoder(p, x, "IEF", defect="ulvh")     # u * offset is f32 in this kernel: no such piece
    with pytest.raises(ValueError):
        sc.chain_decoder(p, x, "IEF", gf=64)


@pytest.mark.parametrize("defect", sc.DEFECTS)
@pytest.mark.parametrize("gf", WIDTHS)
def test_rows_defect_rejected_at_scale_5(gf, defect):
    """The chain's ways of losing a low piece, on 2,000 rows at 385 inputs: rejected on both decoder kinds."""
    for kind in ("IMNET", "IEF"):
        p, x, r64, r32 = _decoder_case(kind, gf, 5.0, 2)
        twin = sc.chain_decoder(p, x, kind, 2, False, gf)
        bad = sc.chain_decoder(p, x, kind, 2, False, gf, defect=defect)
        assert not torch.equal(bad, twin), "the defect changes nothing"
        assert _rejected("gf %d %s %s" % (gf, kind, defect), bad, r64, r32, twin), (gf, kind, defect)


@pytest.mark.parametrize("defect", sc.DEFECTS)
def test_query_defect_rejected_at_scale_5(defect):
    """The same for the factorised layer 1 of the query at gf 32."""
    s, r64, r32 = _scene_case(32, 5.0)
    mid = r64["max_pair_id"]
    twin = _query(sc.chain_query, s, max_pair_id=mid)
    bad = _query(sc.chain_query, s, max_pair_id=mid, defect=defect)
    for k in ("pred_offset", "pred_prob_end"):
        assert not torch.equal(bad[k], twin[k]), "the defect changes nothing"
        assert _rejected("%s %s" % (k, defect), bad[k], r64[k], r32[k], twin[k]), (k, defect)
