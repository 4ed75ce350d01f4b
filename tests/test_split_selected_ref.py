"""The twin of precision="f16x3" with offsets="selected" (tests/split_selected_ref.py) on the CPU: its prob side is
split_query's, its offset side agrees with split_query's where every ray has one pair (the two differ in how the ray
row enters layer 1: whole, or as two f16 pieces), and assert_split_close rejects every way the list form of
lidf_points_h_kernel can get the ray row wrong as well as split_f16_ref's defects on the offset net. Decoder outputs
are compared as logits (util.inv_out_act) on the selected rows."""
import functools

import pytest
import torch

import split_f16_ref as sp
import split_selected_ref as ss
from util import f64, inv_out_act, orc


def _query(fn, s, cast=lambda v: v, **kw):
    return fn(cast(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(), s["pair_vox"].long(),
              cast(s["pair_t"]), s["pair_off"], cast(s["feat_grid"]), cast(s["vox_feat"]), cast(s["prob_p"]),
              cast(s["off_p"]), fast_roi=True, **kw)


@functools.lru_cache(maxsize=None)
def _scene_case(N, n_iter=2, ragged=False):
    """A 1 x 12 x 16 x N scene at weight scale 5 with random biases, the oracle's float64 / float32 query on it (the
    float64 arg-max given to everything) and the honest twin; computed once, written by nobody."""
    s = orc.synthetic_scene(1, 12, 16, N, seed=4321, weight_scale=5.0, ragged=ragged)
    orc.randomize_biases(s["prob_p"], 5)
    orc.randomize_biases(s["off_p"], 6)
    with torch.no_grad():
        r64 = _query(orc.query, s, cast=f64, n_iter=n_iter)
        mid = r64["max_pair_id"]
        r32 = _query(orc.query, s, max_pair_id=mid, n_iter=n_iter)
        twin = _query(ss.split_selected_query, s, max_pair_id=mid, n_iter=n_iter)
    return s, r64, r32, twin


def _rejected(what, bad, r64, r32, twin):
    try:
        sp.assert_split_close(what, inv_out_act(bad), inv_out_act(r64), inv_out_act(r32), inv_out_act(twin))
    except AssertionError:
        return True
    return False


def test_prob_side_is_split_query():
    s, r64, _, twin = _scene_case(8, ragged=True)
    full = _query(sp.split_query, s, max_pair_id=r64["max_pair_id"])
    for k in ("pred_prob_end", "pred_prob_end_softmax", "max_pair_id"):
        assert torch.equal(twin[k], full[k]), k
    # rows outside the selection are NaN, rays without a pair select P and sit at the origin
    P, R = s["P"], s["R"]
    rows, rays = twin["selected_rows"], twin["selected_rays"]
    other = torch.ones(P, dtype=torch.bool)
    other[rows] = False
    assert torch.isnan(twin["pred_offset"][other]).all() and torch.isnan(twin["pair_pred_pos"][other]).all()
    assert torch.isfinite(twin["pred_offset"][rows]).all() and torch.isfinite(twin["pair_pred_pos"][rows]).all()
    empty = torch.ones(R, dtype=torch.bool)
    empty[rays] = False
    assert empty.any() and (twin["max_pair_id"][empty] == P).all() and (twin["pred_pos"][empty] == 0).all()
    assert torch.equal(twin["pred_pos"][rays], twin["pair_pred_pos"][rows])


def test_offset_side_agrees_with_split_query_on_one_pair_per_ray():
    """N = 1: every pair is selected. The whole ray row against its two f16 pieces is a difference of 2^-22 of that
    row: the selected twin meets the criterion with split_query as the twin (and is itself honest: k = 1 against its
    own error), on the logits and on the positions."""
    s, r64, r32, twin = _scene_case(1)
    assert s["P"] == s["R"] and torch.equal(twin["selected_rows"], torch.arange(s["P"]))
    full = _query(sp.split_query, s, max_pair_id=r64["max_pair_id"])
    assert not torch.equal(twin["pred_offset"], full["pred_offset"])
    l64, l32 = inv_out_act(r64["pred_offset"]), inv_out_act(r32["pred_offset"])
    sp.assert_split_close("selected twin, split_query as twin", inv_out_act(twin["pred_offset"]), l64, l32,
                          inv_out_act(full["pred_offset"]))
    sp.assert_split_close("selected twin, own", inv_out_act(twin["pred_offset"]), l64, l32,
                          inv_out_act(twin["pred_offset"]), k=1.0)
    for k in ("pair_pred_pos", "pred_pos"):
        sp.assert_split_close("selected twin %s" % k, twin[k], r64[k], r32[k], full[k])


def _detection(n_iter, **wrong):
    s, r64, r32, twin = _scene_case(8, n_iter)
    rows = twin["selected_rows"]
    assert rows.numel() == s["R"]
    bad = _query(ss.split_selected_query, s, max_pair_id=r64["max_pair_id"], n_iter=n_iter, **wrong)
    assert torch.equal(bad["pred_prob_end"], twin["pred_prob_end"])     # the prob net stays honest
    assert not torch.equal(bad["pred_offset"][rows], twin["pred_offset"][rows]), "the defect changes nothing"
    # the honest twin passes where the wrong one is rejected
    sp.assert_split_close("honest", inv_out_act(twin["pred_offset"][rows]), inv_out_act(r64["pred_offset"][rows]),
                          inv_out_act(r32["pred_offset"][rows]), inv_out_act(twin["pred_offset"][rows]), k=1.0)
    return _rejected(str(wrong), bad["pred_offset"][rows], r64["pred_offset"][rows], r32["pred_offset"][rows],
                     twin["pred_offset"][rows])


@pytest.mark.parametrize("ray_row", ss.RAY_ROWS)
def test_wrong_ray_row_rejected(ray_row):
    """1 x 12 x 16 x 8 at weight scale 5: the row of ray r + 1, no ray row, the ray row in one f16 piece."""
    assert _detection(2, ray_row=ray_row), ray_row


# (ul*vh scales with the running offset, 0.001 into pass 1: shown at three iterations, as in test_split_f16_ref.py)
@pytest.mark.parametrize("defect", sp.ROW_DEFECTS)
def test_offset_net_defect_rejected(defect):
    assert _detection(3 if defect == "ulvh" else 2, defect=defect), defect


def test_unknown_modes_are_refused():
    s, r64, _, _ = _scene_case(8)
    with pytest.raises(ValueError):
        _query(ss.split_selected_query, s, max_pair_id=r64["max_pair_id"], defect="ray")   # no pieces of the ray row here
    with pytest.raises(ValueError):
        _query(ss.split_selected_query, s, max_pair_id=r64["max_pair_id"], ray_row="nothing")
