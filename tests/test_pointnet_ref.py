"""The float64 references of tests/test_f64_stage2_gpu.py, on the CPU (tests/pointnet_ref.py): the conditioning
reaches its fixed point quickly and drops little, it is what makes the float32 oracle's error a usable unit,
pointnet2stage_argrouted is the oracle with torch_scatter's gradient, and on conditioned inputs
util.assert_f64_close rejects small deliberate errors of the kinds a PointNet backward can make."""
import contextlib
import io

import pytest
import torch

import pointnet_ref as ref
from util import assert_f64_close, f64, f64_errors, orc

U = 2.0 ** -24


def _subset(c):
    return c["inp"][c["keep"]], c["vox"][c["keep"]]


def _grads(fn, c, dt, inp=None, vox=None, w=None):
    x, vx = _subset(c) if inp is None else (inp, vox)
    return ref.pointnet_grads(fn, c["p"], x, vx, c["V"], c["w"] if w is None else w, dt)[1]


def _normwise(g32, g64):
    return max(f64_errors(g32[k], g64[k], g32[k])[3] for k in g64)


def test_rel_is_above_the_float32_oracles_preactivation_error():
    """REL >= 4 x the float32 oracle's largest pre-activation error against float64, relative to its layer's
    max|z|, over every shape (measured: 6.5e-7 at (70000, 300), vox_lin2)."""
    worst = 0.0
    for n, V in ref.SHAPES:
        c = ref.pointnet_case(n, V)
        x, vx = _subset(c)
        t32, t64 = [], []
        with torch.no_grad():
            orc.pointnet2stage(c["p"], x, vx, V, trace=t32)
            orc.pointnet2stage(f64(c["p"]), x.double(), vx, V, trace=t64)
        for k in ref.LAYERS:
            e = ((t32[0][k].double() - t64[0][k]).abs().max() / t64[0][k].abs().max()).item()
            print("(%d, %d) %s: float32 pre-activation error %.3g x max|z|" % (n, V, k, e))
            worst = max(worst, e)
    assert 0 < worst and ref.REL >= 4 * worst, worst


@pytest.mark.parametrize("n,V", ref.SHAPES)
def test_pointnet_conditioning(n, V):
    """Fixed point in <= 10 passes, <= 2 % of the points dropped, <= 0.1 % of the output entries masked (measured:
    0 / 0 / 0.80 / 0.40 / 0.73 / 0.55 % of the points in 0-2 passes, at most 9 of 640,000 entries); nothing is
    flagged on the result; the float32 oracle's gradients are then within 64 x 2^-24 of float64 normwise
    (measured: <= 4.9e-7)."""
    c = ref.pointnet_case(n, V)
    dropped = 1.0 - c["keep"].float().mean().item()
    print("(%d, %d): %d points dropped (%.2f %%) in %d passes, %d output entries masked"
          % (n, V, int((~c["keep"]).sum()), 100 * dropped, c["passes"], c["masked"]))
    assert c["passes"] <= 10 and dropped <= 0.02 and c["masked"] <= 1e-3 * V * 128
    x, vx = _subset(c)
    keep, _, passes = ref.condition_pointnet(f64(c["p"]), x, vx, V)
    assert passes == 0 and bool(keep.all())
    e = _normwise(_grads(orc.pointnet2stage, c, torch.float32), _grads(orc.pointnet2stage, c, torch.float64))
    print("(%d, %d): float32 oracle's gradients vs float64, normwise %.3g" % (n, V, e))
    assert e <= 64 * U, e


def test_unconditioned_inputs_give_no_yardstick():
    """(20000, 5000) as drawn: float32 and float64 route some gradients differently, the float32 oracle is
    7e-4 normwise / 1.1e-2 x max|g| off float64 — the conditioning is what makes its error a unit."""
    c = ref.pointnet_case(20000, 5000)
    g32 = _grads(orc.pointnet2stage, c, torch.float32, c["inp"], c["vox"])
    g64 = _grads(orc.pointnet2stage, c, torch.float64, c["inp"], c["vox"])
    e = _normwise(g32, g64)
    print("unconditioned (20000, 5000): normwise %.3g" % e)
    assert e > 64 * U, e


@pytest.mark.parametrize("n,V", [(257, 9), (3000, 40), (20000, 5000)])
def test_argrouted_equals_the_oracle_without_ties(n, V):
    c = ref.pointnet_case(n, V)
    x, vx = _subset(c)
    for dt in (torch.float32, torch.float64):
        a = ref.pointnet_grads(ref.pointnet2stage_argrouted, c["p"], x, vx, V, c["w"], dt)
        o = ref.pointnet_grads(orc.pointnet2stage, c["p"], x, vx, V, c["w"], dt)
        assert torch.equal(a[0], o[0])                                  # in value, bit for bit
        # in gradient: one row per entry on both sides, to the rounding of sums taken in another order (the bound
        # of the float32 oracle against float64 above, 64 units of the type's rounding)
        for k in o[1]:
            assert (a[1][k] - o[1][k]).abs().max().item() <= 64 * (U if dt == torch.float32 else 2.0 ** -53) * \
                o[1][k].abs().max().item(), k


def test_argrouted_puts_a_tied_gradient_on_the_lowest_row():
    """Every row twice (rows i and i + n): the values are the oracle's, the second copies get no gradient at all
    and the first copies the whole of it — the oracle's amax autograd gives each half. The routing is taken with
    ref.rowwise_linear, under which the two copies of a row are equal bit for bit on any CPU (a matrix product
    does not promise that, and then there is no tie to route)."""
    c = ref.pointnet_case(257, 9)
    x, vx = _subset(c)
    n = x.shape[0]
    x2, v2 = torch.cat((x, x)), torch.cat((vx, vx))
    rowwise = lambda p, inp, vox, V: ref.pointnet_forward(p, inp, vox, V, linear=ref.rowwise_linear)  # noqa: E731
    out_a, _ = ref.pointnet_grads(ref.pointnet2stage_argrouted, c["p"], x2, v2, 9, c["w"], torch.float64)
    out_r, ga = ref.pointnet_grads(rowwise, c["p"], x2, v2, 9, c["w"], torch.float64)
    out_o, go = ref.pointnet_grads(orc.pointnet2stage, c["p"], x2, v2, 9, c["w"], torch.float64)
    _, g1 = ref.pointnet_grads(orc.pointnet2stage, c["p"], x, vx, 9, c["w"], torch.float64)
    assert torch.equal(out_a, out_o)
    assert (out_r - out_o).abs().max().item() <= 1e-12 * out_o.abs().max().item()
    assert not ga["inp"][n:].any() and ga["inp"][:n].any()
    assert (ga["inp"][:n] - g1["inp"]).abs().max().item() <= 1e-12 * g1["inp"].abs().max().item()
    assert go["inp"][n:].any()                                          # (the even split the product does not make)
    for k in g1:
        if k != "inp":
            assert (ga[k] - g1[k]).abs().max().item() <= 1e-12 * g1[k].abs().max().item(), k


# ----------------------------------------------------------------------------------------------------------------
# the criterion bites
# ----------------------------------------------------------------------------------------------------------------
def _old_bound_ratio(got, g32):
    """Largest error in units of test_train_gpu.py::test_pointnet_gradients' bound, 5e-4 x max(1e-2, max|g|)."""
    return max((got[k] - g32[k]).abs().max().item() / (5e-4 * max(1e-2, g32[k].abs().max().item())) for k in g32)


def _rejected(got, g64, g32):
    out = []
    for k in g64:
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                assert_f64_close(k, got[k], g64[k], g32[k])
        except AssertionError:
            out.append(k)
    return out


def test_f64_criterion_rejects_pointnet_errors_the_fixed_tolerance_accepts():
    """(70000, 300) conditioned, three deliberate errors in a float32 evaluation, each within the old bound of
    5e-4 x max|g| in every tensor and each rejected by assert_f64_close:
      * one pooled entry's gradient routed to the runner-up row instead of the arg row;
      * the last 256-row chunk of one voxel (the rows past its 256th) left out of the per-voxel row sum behind
        vox_lin1's output gradient;
      * a 1e-5 relative error in one weight gradient.
    The first two are made in a voxel whose upstream gradient is 1e-3 of the others'. With an upstream gradient
    like every other voxel's they would not need this file: a pooled entry of the second pooling feeds one row's
    whole input gradient, and such a row sum is carried by at most 128 arg rows, so either error is then 20-500 x
    the old bound in the input gradient (measured) — the old bound passes them only where the loss weighs the
    voxel lightly, which is where the float64 yardstick still sees them."""
    n, V = 70000, 300
    c = ref.pointnet_case(n, V)
    x, vx = _subset(c)
    cnt = torch.bincount(vx, minlength=V)
    # a voxel with a tail chunk (more than 256 rows) that holds an arg row of the second pooling, i.e. whose
    # rows past the 256th carry some of the voxel's sum
    tr = []
    with torch.no_grad():
        orc.pointnet2stage(f64(c["p"]), x.double(), vx, V, trace=tr)
    _, arg2 = ref.pool_args(*tr[0]["pool2"], V)
    v = tail = None
    for cand in torch.nonzero(cnt > 256)[:, 0].tolist():
        rows = torch.nonzero(vx == cand)[:, 0]
        t = rows[(rows.numel() - 1) // 256 * 256:]
        if torch.isin(arg2[cand], t).any():
            v, tail = cand, t
            break
    assert v is not None
    print("voxel %d: %d rows, the last %d left out of its row sum" % (v, int(cnt[v]), tail.numel()))
    w = c["w"].clone()
    w[v] *= 1e-3
    g64 = _grads(orc.pointnet2stage, c, torch.float64, w=w)
    g32 = _grads(orc.pointnet2stage, c, torch.float32, w=w)
    assert not _rejected(g32, g64, g32)

    f = int(torch.nonzero(arg2[v] < x.shape[0])[0, 0])       # a pooled entry of the voxel that has an arg row

    def runner_up_pool(xx, vv, VV):
        out = ref._gather_pool(xx, vv, VV)
        if xx.shape[1] != 128:
            return out
        _, arg = ref.pool_args(xx.detach(), vv, VV)
        rest = xx.detach().clone()
        rest[arg[v, f], f] = 0.0
        _, second = ref.pool_args(rest, vv, VV)
        assert second[v, f] < xx.shape[0] and second[v, f] != arg[v, f]
        arg[v, f] = second[v, f]
        wrong = torch.gather(torch.cat((xx, xx.new_zeros(1, 128)), 0), 0, arg)
        return wrong + (out - wrong).detach()                # the right value, the wrong row's gradient

    def short_sum(g1, vv):
        rows = g1[vv]
        cut = torch.zeros(vv.shape[0], 1, dtype=torch.bool)
        cut[tail] = True
        return torch.where(cut, rows.detach(), rows)

    wrong = {"runner-up row": _grads(lambda *a: ref.pointnet_forward(*a, pool=runner_up_pool), c, torch.float32, w=w),
             "short row sum": _grads(lambda *a: ref.pointnet_forward(*a, spread=short_sum), c, torch.float32, w=w),
             "dW x (1 + 1e-5)": dict(g32, **{"point_lin3.weight": g32["point_lin3.weight"] * (1 + 1e-5)})}
    for what, got in wrong.items():
        old, rej = _old_bound_ratio(got, g32), _rejected(got, g64, g32)
        print("%s: %.3g of the old bound; rejected: %s" % (what, old, ", ".join(rej)))
        assert 0 < old <= 1.0, (what, old)
        assert rej, what


# ----------------------------------------------------------------------------------------------------------------
# the refine scene
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_rel,pnet_pos_rel", [(False, True), (True, False)])
def test_refine_conditioning(pos_rel, pnet_pos_rel):
    """R = 960, V = 1458, 1500 valid points, two iterations: fixed point in <= 10 passes, <= 10 % of the rays and
    <= 2 % of the valid points dropped (measured: 45 rays / 17 points in 4 passes; relative positions 53 / 11 in
    8); on the result the float32 and float64 chains choose the same end voxels and nothing is flagged."""
    case, keep_ray, keep_valid, passes = ref.conditioned_refine_case(pos_rel, pnet_pos_rel)
    R, Nv = keep_ray.numel(), keep_valid.numel()
    assert (R, Nv, case["voxel_bound"].shape[0]) == (960, 1500, 1458)
    print("refine scene (pos_rel %s): %d of %d rays, %d of %d valid points dropped in %d passes"
          % (pos_rel, int((~keep_ray).sum()), R, int((~keep_valid).sum()), Nv, passes))
    assert passes <= 10
    assert (~keep_ray).float().mean().item() <= 0.10 and (~keep_valid).float().mean().item() <= 0.02
    again = ref.condition_refine(case, 2, pos_rel, pnet_pos_rel)
    assert again[2] == 0 and bool(again[0].all()) and bool(again[1].all())
    with torch.no_grad():
        p64, e64 = ref.refine_chain(case, torch.float64, 2, pos_rel, pnet_pos_rel)
        p32, e32 = ref.refine_chain(case, torch.float32, 2, pos_rel, pnet_pos_rel)
    assert all(torch.equal(a, b) for a, b in zip(e64, e32))
    assert p64.dtype == torch.float64 and 0 < (p32.double() - p64).abs().max().item() <= 1e-4


def test_refine_trace_follows_the_chain():
    """The trace hooks: one entry per iteration, the position entering it, the PointNet's and the decoder's
    pre-activations (3 hidden layers x 2 passes + the running offset); without a trace the values are the same
    bits."""
    case = ref.conditioned_refine_case()[0]
    tr = []
    with torch.no_grad():
        pos_t, _ = ref.refine_chain(case, torch.float32, 2, trace=tr)
        pos, _ = ref.refine_chain(case, torch.float32, 2)
    R, Nv = case["ray_dir"].shape[0], case["valid_inp"].shape[0]
    assert torch.equal(pos, pos_t) and len(tr) == 2
    assert torch.equal(tr[0]["pos"], case["pred_pos"] + case["noise"] * case["ray_dir"])
    for it in tr:
        assert len(it["preacts"]) == 7 and it["preacts"][-1].shape == (R, 1)
        assert set(it["pnet"]) == set(ref.LAYERS) | {"pool1", "pool2"}
        assert it["pnet"]["point_lin4"].shape == (Nv + R, 128) and it["pnet"]["vox_lin2"].shape == (1458, 128)
        assert torch.equal(it["pnet"]["pool2"][1][Nv:], it["end_voxel"])
