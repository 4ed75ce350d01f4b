"""The twin of the split-f16 arithmetic (tests/split_f16_ref.py) and its criterion, on the CPU: the honest twin is
as accurate as the scheme promises, and assert_split_close rejects every way of losing a low piece that the fixed
output tolerance (util.TOL) and the 2e-5 closeness of tests/test_split_f16_gpu.py let through. Decoder outputs are
compared as logits (util.inv_out_act), as the f32 tests do."""
import functools

import pytest
import torch

import split_f16_ref as sp
from util import TOL, f64, f64_errors, inv_out_act, orc

N_ROWS = 2000
DECODER_CASES = [("IMNET", 385), ("IEF", 385), ("IEF", 334)]


@functools.lru_cache(maxsize=None)
def _decoder_case(kind, d, scale, n_iter=2):
    """(p, x, float64 output, float32 output) of the oracle on N_ROWS random rows; computed once, written by nobody."""
    p = orc.randomize_biases(orc.init_decoder(kind, d, 11, scale), 12)
    x = torch.randn(N_ROWS, d, generator=torch.Generator().manual_seed(d))
    with torch.no_grad():
        return p, x, orc.decoder_forward(f64(p), x.double(), kind, n_iter), orc.decoder_forward(p, x, kind, n_iter)


@functools.lru_cache(maxsize=None)
def _scene_case(scale, n_iter=2):
    """A 1 x 16 x 24 x 16 scene (6,144 pairs) at weight scale `scale` with random biases, and the oracle's float64 /
    float32 query on it (the float64 arg-max given to both)."""
    s = orc.synthetic_scene(1, 16, 24, 16, seed=1234, weight_scale=scale)
    orc.randomize_biases(s["prob_p"], 5)
    orc.randomize_biases(s["off_p"], 6)
    with torch.no_grad():
        r64 = _query(orc.query, s, cast=f64, n_iter=n_iter)
        r32 = _query(orc.query, s, max_pair_id=r64["max_pair_id"], n_iter=n_iter)
    return s, r64, r32


def _query(fn, s, cast=lambda v: v, **kw):
    return fn(cast(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(), s["pair_vox"].long(),
              cast(s["pair_t"]), s["pair_off"], cast(s["feat_grid"]), cast(s["vox_feat"]), cast(s["prob_p"]),
              cast(s["off_p"]), fast_roi=True, **kw)


def _rejected(what, bad, r64, r32, twin):
    try:
        sp.assert_split_close(what, inv_out_act(bad), inv_out_act(r64), inv_out_act(r32), inv_out_act(twin))
    except AssertionError:
        return True
    return False


def _old_criteria_accept(bad, r32, r64=None):
    """What tests/test_split_f16_gpu.py asserts of a post-activation output: (within TOL of the oracle, within 2e-5
    of the exact-f32 result). r64 given: on the outputs behind the clamp only (outside [0, 1] by 1e-3; 45-97 % of
    the outputs of the scale-5 cases here) — there the activation divides a logit error by 100. Inside [0, 1] a
    defect of 1e-4 on the logit is a defect of 1e-4 on the output, and TOL does see the largest of these there."""
    e = (bad.float() - r32).abs()
    if r64 is not None:
        behind = (r64 < -1e-3) | (r64 > 1 + 1e-3)
        assert behind.float().mean().item() > 0.4
        e = e[behind]
    return e.max().item() <= TOL, e.max().item() <= 2e-5


# ---------------------------------------------------------------------------------------------------------------
# the honest twin
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 5.0, 20.0])
@pytest.mark.parametrize("kind,d", DECODER_CASES)
def test_honest_twin_is_as_accurate_as_the_scheme_promises(kind, d, scale):
    """The twin meets its own criterion with k = 1, computes something other than float64, and is within 8 x the f32
    oracle's error of float64 (a simplified emulation of the scheme gave at most 2.9 x; at scale 1 the low
    pieces are f16 subnormals with an absolute error of 2^-25, which the f32 oracle does not have)."""
    p, x, r64, r32 = _decoder_case(kind, d, scale)
    twin = sp.split_decoder(p, x, kind)
    assert twin.dtype == torch.float64 and twin.shape == r64.shape
    l64, l32, lt = inv_out_act(r64), inv_out_act(r32), inv_out_act(twin)
    sp.assert_split_close("%s %d x%g" % (kind, d, scale), lt, l64, l32, lt, k=1.0)
    e_t, e_32, n_t, n_32, _ = f64_errors(lt, l64, l32)
    print("%s %d x%g: twin / f32 oracle error against float64: %.2f elementwise, %.2f normwise"
          % (kind, d, scale, e_t / e_32, n_t / n_32))
    assert 0 < e_t <= 8 * e_32 and 0 < n_t <= 8 * n_32, (e_t, e_32, n_t, n_32)


@pytest.mark.parametrize("scale", [1.0, 5.0, 20.0])
def test_honest_query_twin(scale):
    """split_query (the factorised layer 1) under the same three conditions, on both decoders of a scene, and equal to
    split_decoder on the oracle's own rows to f32 rounding of layer 1 (the tables are rounded where the rows are not)."""
    s, r64, r32 = _scene_case(scale)
    twin = _query(sp.split_query, s, max_pair_id=r64["max_pair_id"])
    for k in ("pred_offset", "pred_prob_end"):
        l64, l32, lt = inv_out_act(r64[k]), inv_out_act(r32[k]), inv_out_act(twin[k])
        sp.assert_split_close("%s x%g" % (k, scale), lt, l64, l32, lt, k=1.0)
        e_t, e_32, n_t, n_32, _ = f64_errors(lt, l64, l32)
        print("%s x%g: twin / f32 oracle error against float64: %.2f elementwise, %.2f normwise"
              % (k, scale, e_t / e_32, n_t / n_32))
        assert 0 < e_t <= 8 * e_32 and 0 < n_t <= 8 * n_32, (k, e_t, e_32, n_t, n_32)
    for k in ("pair_pred_pos", "pred_pos", "pred_prob_end_softmax"):
        sp.assert_split_close("%s x%g" % (k, scale), twin[k], r64[k], r32[k], twin[k], k=1.0)
    rows = []
    _query(orc.query, s, cast=f64, rows=rows)
    by_rows = sp.split_decoder(s["off_p"], torch.cat(rows, 0), "IEF")
    e = (inv_out_act(by_rows) - inv_out_act(twin["pred_offset"])).abs().max().item()
    assert e <= 64 * 2.0 ** -24 * max(1.0, inv_out_act(r64["pred_offset"]).abs().max().item()), e


def test_range_at_tiny_weights():
    """Scale 0.05, for range only: every weight's low piece and most activations' are f16 subnormals or zero, the
    twin stays finite and meets its own criterion. The biases (std 0.05) dominate every pre-activation there, a lost
    low piece of a product moves nothing that the bias pieces' own rounding does not, and no defect separates."""
    for kind, d in DECODER_CASES:
        p, x, r64, r32 = _decoder_case(kind, d, 0.05)
        twin = sp.split_decoder(p, x, kind)
        assert torch.isfinite(twin).all()
        sp.assert_split_close("%s %d x0.05" % (kind, d), inv_out_act(twin), inv_out_act(r64), inv_out_act(r32),
                              inv_out_act(twin), k=1.0)


def test_unknown_defects_are_refused():
    p, x, _, _ = _decoder_case("IEF", 385, 5.0)
    with pytest.raises(ValueError):
        sp.split_decoder(p, x, "IEF", defect="ray")          # the ray row exists in the factorised layer 1 only
    with pytest.raises(ValueError):
        sp.split_decoder(p, x, "IEF", defect="nothing")


# ---------------------------------------------------------------------------------------------------------------
# detection
# ---------------------------------------------------------------------------------------------------------------
# The ul*vh product scales with the running offset, which enters pass 1 as 0.001: at two iterations one pass carries
# it and the defect is 3.3 x the unit, under k = 4. It is shown at three iterations (8.5 x).
def _n_iter(defect):
    return 3 if defect == "ulvh" else 2


def _decoder_detection(kind, d, scale, defect):
    """(rejected by assert_split_close, accepted by TOL, accepted by the 2e-5 closeness)."""
    n_iter = _n_iter(defect)
    p, x, r64, r32 = _decoder_case(kind, d, scale, n_iter)
    twin = sp.split_decoder(p, x, kind, n_iter)
    bad = sp.split_decoder(p, x, kind, n_iter, defect=defect)
    assert not torch.equal(bad, twin), "the defect changes nothing"
    return (_rejected("%s %d x%g %s" % (kind, d, scale, defect), bad, r64, r32, twin),
            *_old_criteria_accept(bad, r32, r64 if scale > 1 else None))


def _query_detection(scale, defect):
    n_iter = _n_iter(defect)
    s, r64, r32 = _scene_case(scale, n_iter)
    mid = r64["max_pair_id"]
    twin = _query(sp.split_query, s, max_pair_id=mid, n_iter=n_iter)
    bad = _query(sp.split_query, s, max_pair_id=mid, n_iter=n_iter, defect=defect)
    keys = ("pred_offset",) if defect == "ulvh" else ("pred_offset", "pred_prob_end")
    assert all(not torch.equal(bad[k], twin[k]) for k in keys), "the defect changes nothing"
    rej = [_rejected("%s x%g %s" % (k, scale, defect), bad[k], r64[k], r32[k], twin[k]) for k in keys]
    old = [_old_criteria_accept(bad[k], r32[k], r64[k] if scale > 1 else None) for k in ("pred_offset", "pred_prob_end")]
    return all(rej), all(o[0] for o in old), all(o[1] for o in old)


# At scale 5 the subnormal flush is the one defect large enough for the 2e-5 closeness to see behind the clamp
# (2.1e-5 to 3.0e-5 there); TOL accepts it. At scale 1, where the low weight pieces are subnormals and the flush is what
# the case is about, both accept it (4.6e-6 on the logit).
def _assert_blind(defect, scale, tol_accepts, close_accepts):
    assert tol_accepts, defect
    assert close_accepts or (defect == "flush" and scale == 5.0), defect


@pytest.mark.parametrize("defect", sp.ROW_DEFECTS)
def test_rows_defect_rejected_at_scale_5(defect):
    """lidf_rows_h.hip's ways of losing a low piece, on 2,000 rows at 385 inputs: rejected on every decoder they
    touch, while the post-activation output stays within TOL of the oracle and within 2e-5 of exact f32."""
    for kind in ("IEF",) if defect == "ulvh" else ("IMNET", "IEF"):
        rejected, tol_accepts, close_accepts = _decoder_detection(kind, 385, 5.0, defect)
        assert rejected, (kind, defect)
        _assert_blind(defect, 5.0, tol_accepts, close_accepts)


@pytest.mark.parametrize("defect", sp.DEFECTS)
def test_query_defect_rejected_at_scale_5(defect):
    """The same for the factorised layer 1 of lidf_points_h.hip, the ray row's low piece included."""
    rejected, tol_accepts, close_accepts = _query_detection(5.0, defect)
    assert rejected, defect
    _assert_blind(defect, 5.0, tol_accepts, close_accepts)


@pytest.mark.parametrize("defect", ["flush", "act2", "act3", "ray"])
def test_defect_rejected_at_the_reference_initialisation(defect):
    """Scale 1 (N(0, 0.02) weights: the low weight pieces are f16 subnormals): the subnormal flush, the activation
    pairs and the ray row are still rejected, and no output moves by more than 5e-6. The header of lidf_points_h.hip
    promises that subnormal operands are honoured; this is the criterion that holds it to that."""
    if defect == "ray":
        rejected, tol_accepts, close_accepts = _query_detection(1.0, defect)
    else:
        rejected, tol_accepts, close_accepts = _decoder_detection("IEF", 385, 1.0, defect)
        assert _decoder_detection("IMNET", 385, 1.0, defect)[0], defect
    assert rejected, defect
    _assert_blind(defect, 1.0, tol_accepts, close_accepts)
