"""The float64 yardstick of tests/test_f64_gpu.py, on the CPU: the oracle's float64 mode agrees with its
float32 default to float32 rounding, and assert_f64_close catches small deliberate errors that the fixed
output tolerance (util.TOL) and the fixed gradient tolerance (2e-4 x max|g|) let through."""
import pytest
import torch

from util import (TOL, assert_f64_close, decoder_preacts, f64, f64_errors, inv_out_act, kink_rows, oracle_grads,
                  orc)


def _scene():
    return orc.synthetic_scene(1, 32, 32, 16, seed=1234)


def _query(s, prob_p=None, off_p=None, cast=lambda v: v):
    return orc.query(cast(s["ray_dir"]), s["ray_pix"], s["ray_bid"], s["pair_ray"].long(), s["pair_vox"].long(),
                     cast(s["pair_t"]), s["pair_off"], cast(s["feat_grid"]), cast(s["vox_feat"]),
                     cast(prob_p or s["prob_p"]), cast(off_p or s["off_p"]), fast_roi=True)


def _grads(p, x, w, n_iter=2):
    pc = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xc = x.clone().requires_grad_(True)
    (orc.ief_forward(pc, xc, n_iter).reshape(-1) * w).sum().backward()
    g = {k: v.grad for k, v in pc.items()}
    g["input"] = xc.grad
    return g


def test_float64_oracle_agrees_with_float32_default():
    """Same functions, same inputs: float64 and float32 differ by float32 rounding only, the arg-max aside."""
    s = _scene()
    r32, r64 = _query(s), _query(s, cast=f64)
    for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_prob_end_softmax"):
        assert r64[k].dtype == torch.float64 and r32[k].dtype == torch.float32, k
        e_max, _, e_nrm, _, scale = f64_errors(r32[k], r64[k], r32[k])
        # (measured: max 3.1e-6, normwise 2.4e-6 = 40 units of 2^-24 — rounding through four layers and two
        # passes; and non-zero: the float64 mode does compute in float64)
        assert 0 < e_max <= 256 * 2.0 ** -24 * max(scale, 1.0) and e_nrm <= 128 * 2.0 ** -24, (k, e_max, e_nrm)
    agree = (r32["max_pair_id"] == r64["max_pair_id"]).float().mean().item()
    assert agree >= 0.99, agree
    # (that the float32 default itself is unchanged is guarded by the pinned goldens, tests/test_oracle_golden.py)


def test_oracle_grads_gives_each_call_its_own_leaves():
    """Two reference gradients on the same float32 input (the pair node's two decoders) must not share an input
    gradient: each equals the one computed alone, and their sum is the pair's."""
    d, n = 385, 300
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 21, 5.0), 22)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 23, 5.0), 24)
    gen = torch.Generator().manual_seed(1)
    x, w = torch.randn(n, d, generator=gen), torch.randn(n, generator=gen)
    _, gp = oracle_grads(pp, x, "IMNET", w, torch.float32)
    _, go = oracle_grads(po, x, "IEF", w, torch.float32)
    assert gp["input"] is not go["input"] and x.grad is None and not x.requires_grad
    _, go_alone = oracle_grads(po, x.clone(), "IEF", w, torch.float32)
    assert torch.equal(go["input"], go_alone["input"])
    xc = x.clone().requires_grad_(True)
    ((orc.imnet_forward(pp, xc).reshape(-1) + orc.ief_forward(po, xc, 2).reshape(-1)) * w).sum().backward()
    assert (gp["input"] + go["input"] - xc.grad).abs().max().item() <= 1e-5 * xc.grad.abs().max().item()


def test_kink_mask_reads_the_oracles_own_preactivations():
    """The pre-activations behind util.kink_rows come from the oracle's preacts hook: 3 hidden layers per pass
    and the clamp's argument, which the activation maps onto the oracle's output."""
    d, n = 385, 50
    p = orc.randomize_biases(orc.init_decoder("IEF", d, 11, 5.0), 12)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    zs, y = decoder_preacts(f64(p), x, "IEF", 3)
    assert len(zs) == 9 and [z.shape[1] for z in zs[:3]] == [256, 128, 64] and y.shape == (n, 1)
    assert torch.equal(torch.max(torch.min(y, y * 0.01 + 0.99), y * 0.01), orc.ief_forward(f64(p), x, 3))


def test_logit_check_rejects_a_bias_shift_the_output_tolerance_accepts():
    """offset_dec.linear_4.bias + 4e-5: each of the IEF's two passes adds it to the running offset (8.2e-5 on the
    logit). Outside [0, 1] the output activation divides that by 100 (97 % of the rows here), inside it stays below
    TOL; in logit space it is ~20x the f32 oracle's own error."""
    s = _scene()
    r32, r64 = _query(s), _query(s, cast=f64)
    po = dict(s["off_p"])
    po["linear_4.bias"] = po["linear_4.bias"] + 4e-5
    bad = _query(s, off_p=po)
    clamped = ((r32["pred_offset"] < 0) | (r32["pred_offset"] > 1)).float().mean().item()
    assert clamped > 0.9, clamped
    for k in ("pred_offset", "pair_pred_pos", "pred_pos"):     # the existing criterion passes it
        assert (bad[k] - r32[k]).abs().max().item() <= TOL, k
    with pytest.raises(AssertionError):
        assert_f64_close("pred_offset logit", inv_out_act(bad["pred_offset"]), inv_out_act(r64["pred_offset"]),
                         inv_out_act(r32["pred_offset"]))
    # and the unperturbed f32 oracle meets the helper with k = 1
    assert_f64_close("pred_offset logit", inv_out_act(r32["pred_offset"]), inv_out_act(r64["pred_offset"]),
                     inv_out_act(r32["pred_offset"]), k=1.0)


@pytest.mark.parametrize("layer", ["linear_1", "linear_2", "linear_3"])
def test_gradient_check_rejects_a_weight_scale_the_fixed_tolerance_accepts(layer):
    """One layer's weights x (1 + 3e-6) on a 5,000-row IEF gradient (kink rows masked): every gradient tensor is
    within 2e-4 x max|g| (tests/test_train_gpu.py::_close), the float64 yardstick rejects it."""
    d, n = 385, 5000
    p = orc.randomize_biases(orc.init_decoder("IEF", d, 11, 5.0), 12)
    gen = torch.Generator().manual_seed(n)
    x, w = torch.randn(n, d, generator=gen), torch.randn(n, generator=gen)
    bad_rows = kink_rows(f64(p), f64(x), "IEF")
    assert bad_rows.float().mean().item() < 0.01, bad_rows.sum().item()
    w = torch.where(bad_rows, torch.zeros_like(w), w)
    g32, g64 = _grads(p, x, w), _grads(f64(p), f64(x), f64(w))
    pp = dict(p)
    pp[layer + ".weight"] = pp[layer + ".weight"] * (1 + 3e-6)
    gp = _grads(pp, x, w)
    rejected = []
    for k in g64:
        assert (gp[k] - g32[k]).abs().max().item() <= 2e-4 * max(1.0, g32[k].abs().max().item()), k
        try:
            assert_f64_close(k, gp[k], g64[k], g32[k])
        except AssertionError:
            rejected.append(k)
        assert_f64_close(k, g32[k], g64[k], g32[k], k=1.0)
    assert "input" in rejected and len(rejected) >= 5, rejected


def test_inv_out_act_is_the_exact_inverse():
    y = torch.tensor([-300.0, -1.5, -1e-3, 0.0, 0.25, 1.0, 1.0 + 1e-3, 2.5, 300.0], dtype=torch.float64)
    v = torch.max(torch.min(y, y * 0.01 + 0.99), y * 0.01)
    assert torch.allclose(inv_out_act(v), y, rtol=0, atol=1e-12)
