"""GPU: lidf_ray_reduce_kernel on its own (through lidf_ray_reduce_f32) against its float64 twin
(tests/ray_reduce_ref.py), at both lane widths. A list as given holds more than 8 pairs per ray and runs the 64-lane
form; followed by empty rays until P <= 8 R' it runs the 8-lane form, the one every frame call takes. Every list
runs both ways, with all outputs (softmax, ids, positions, a depth map scattered through ray_bid / ray_flat) and with
the ids alone.

Measured on an MI355X: the softmax error against float64 is at most 1.73 (elementwise) / 1.59 (normwise) times the
float32 twin's (util.assert_f64_close, F64_K = 4; both on the one ray of 200 pairs with logits spread over +-80,
the same at both widths since they give the same bits; every other list is below 1.5), and |sum - 1| of a finite
ray reaches 0.46 of its bound (6 + ceil(n / 64)) 2^-24."""
import pytest
import torch

import ray_reduce_ref as rr
from util import assert_f64_close

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _pixels(R8, seed):
    """A pixel of its own for every ray of the padded list, in 2 images of R8 pixels: half the pixels stay unnamed."""
    g = torch.Generator().manual_seed(seed)
    pix = torch.randperm(2 * R8, generator=g)[:R8]
    return (pix // R8).int(), (pix % R8).int()


def _run(cuda, lst, off, R, bid, flat, hw, full):
    """One call of lidf_ray_reduce_f32 on `R` rays of `lst` with offsets `off`; outputs pre-filled with NaN / -1 /
    the sentinel so that anything the kernel leaves unwritten shows."""
    from implicit_depth_amd import _lib
    P = lst["P"]
    prob, pos, offd = lst["prob"].to(cuda), lst["pos"].to(cuda), off.to(cuda)
    mid = torch.full((R,), -1, dtype=torch.int64, device=cuda)
    out = {"max_pair_id": mid}
    if full:
        out["softmax"] = torch.full((P,), float("nan"), device=cuda)
        out["pred_pos"] = torch.full((R, 3), float("nan"), device=cuda)
        out["depth"] = torch.full((2, hw), SENTINEL, device=cuda)
        bd, fd = bid.to(cuda), flat.to(cuda)
        args = (_lib.ptr(bd), _lib.ptr(fd), hw, _lib.ptr(out["softmax"]), _lib.ptr(mid), _lib.ptr(out["pred_pos"]),
                _lib.ptr(out["depth"]))
    else:
        args = (None, None, 0, None, _lib.ptr(mid), None, None)
    _lib.check(_lib.lib().lidf_ray_reduce_f32(_lib.ptr(prob), _lib.ptr(pos), _lib.ptr(offd), R, P, *args,
                                              _lib.current_stream(cuda)))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.fixture(scope="module")
def runs(cuda):
    """Every list of ray_reduce_ref.all_lists() through the kernel at both widths and both launch forms, and the
    twin's float64 and float32 evaluations; computed once, read by every test below."""
    out = {}
    for lst in rr.all_lists():
        off8, R8 = rr.padded(lst)
        bid, flat = _pixels(R8, lst["P"])
        r = {"lst": lst, "R8": R8, "bid": bid, "flat": flat,
             "w64": _run(cuda, lst, lst["off"], lst["R"], bid, flat, R8, True),
             "w8": _run(cuda, lst, off8, R8, bid, flat, R8, True),
             "w64_ids": _run(cuda, lst, lst["off"], lst["R"], None, None, 0, False),
             "w8_ids": _run(cuda, lst, off8, R8, None, None, 0, False),
             "ref64": rr.reduce_ref(lst["prob"], lst["off"], lst["pos"], torch.float64),
             "ref32": rr.reduce_ref(lst["prob"], lst["off"], lst["pos"], torch.float32)}
        out[lst["name"]] = r
    return out


def _same_bits(a, b):
    """Bit-equal, NaN counting as equal to NaN (the payload of a NaN is nobody's contract)."""
    if a.is_floating_point():
        return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
    return torch.equal(a, b)


def test_both_widths_give_the_same_bits(runs):
    """The regression test of the canonical summation order: softmax, ids, positions and the depth map of the 8-lane
    form equal the 64-lane form's on every list."""
    bad = []
    for name, r in runs.items():
        R, P = r["lst"]["R"], r["lst"]["P"]
        a, b = r["w64"], r["w8"]
        if not _same_bits(a["softmax"], b["softmax"]):
            d = (a["softmax"] != b["softmax"]) & ~(torch.isnan(a["softmax"]) & torch.isnan(b["softmax"]))
            bad.append("%s: %d of %d softmax values differ, by up to %.3g" % (
                name, int(d.sum()), P, (a["softmax"] - b["softmax"])[d].abs().max().item()))
        if not torch.equal(a["max_pair_id"], b["max_pair_id"][:R]):
            bad.append("%s: %d ids differ" % (name, int((a["max_pair_id"] != b["max_pair_id"][:R]).sum())))
        if not _same_bits(a["pred_pos"], b["pred_pos"][:R]):
            bad.append("%s: pred_pos differs" % name)
        # the depth maps agree outside the padding rays' pixels, which only the padded run names (and zeroes)
        pad = torch.zeros(2, r["R8"], dtype=torch.bool)
        pad[r["bid"][R:].long(), r["flat"][R:].long()] = True
        if not _same_bits(a["depth"][~pad], b["depth"][~pad]):
            bad.append("%s: depth differs" % name)
        assert (a["depth"][pad] == SENTINEL).all() and (b["depth"][pad] == 0).all(), name
        assert (b["max_pair_id"][R:] == P).all() and (b["pred_pos"][R:] == 0).all(), name
    print("\n".join(bad))
    assert not bad, "%d differences between the lane widths, e.g. %s" % (len(bad), bad[0])


def test_ids_alone_equal_the_full_call(runs):
    """NULL softmax, pred_pos and depth: the same ids."""
    for name, r in runs.items():
        assert torch.equal(r["w64_ids"]["max_pair_id"], r["w64"]["max_pair_id"]), name
        assert torch.equal(r["w8_ids"]["max_pair_id"], r["w8"]["max_pair_id"]), name


def test_outputs_are_consistent(runs):
    """Every output of a call belongs to the same selection: positions are the selected pairs' rows (or 0), the depth
    map holds their z at the rays' pixels and the sentinel elsewhere, every softmax entry was written."""
    for name, r in runs.items():
        lst = r["lst"]
        for key, R in (("w64", lst["R"]), ("w8", r["R8"])):
            o = r[key]
            mid = o["max_pair_id"]
            assert ((mid >= 0) & (mid <= lst["P"])).all(), name
            exp = torch.cat((lst["pos"], torch.zeros(1, 3)))[mid]
            assert torch.equal(o["pred_pos"], exp), (name, key)
            named = torch.zeros(2, r["R8"], dtype=torch.bool)
            named[r["bid"][:R].long(), r["flat"][:R].long()] = True
            assert torch.equal(o["depth"][r["bid"][:R].long(), r["flat"][:R].long()], exp[:, 2]), (name, key)
            assert (o["depth"][~named] == SENTINEL).all(), (name, key)
            if lst["pattern"] != "nonfinite":
                assert not torch.isnan(o["softmax"]).any(), (name, key)
            # a selected pair lies in its own ray
            off = lst["off"].long()
            has = mid[:lst["R"]] < lst["P"]
            assert ((mid[:lst["R"]] >= off[:-1]) & (mid[:lst["R"]] < off[1:]))[has].all(), (name, key)


def test_softmax_against_float64(runs):
    """Both widths against the float64 twin, the float32 twin's error as the unit (F64_K and the floor as everywhere
    else), list by list."""
    report = []
    for name, r in runs.items():
        if r["lst"]["pattern"] == "nonfinite":
            continue
        for key in ("w64", "w8"):
            assert_f64_close("%s %s" % (name, key), r[key]["softmax"], r["ref64"][0], r["ref32"][0], report=report)
    worst_max = max(report, key=lambda x: x["ratio_max"])
    worst_nrm = max(report, key=lambda x: x["ratio_nrm"])
    print("largest ratios: elementwise %.2f (%s), normwise %.2f (%s)" % (
        worst_max["ratio_max"], worst_max["what"], worst_nrm["ratio_nrm"], worst_nrm["what"]))


def test_finite_rays_sum_to_one(runs):
    """|sum - 1| <= (6 + ceil(n / 64)) 2^-24 on every non-empty finite ray (ray_reduce_ref.unit_sum_bound)."""
    worst = 0.0
    for name, r in runs.items():
        lst = r["lst"]
        ray = rr.ray_of(lst["off"])
        n = torch.tensor(lst["counts"])
        bound = torch.tensor([rr.unit_sum_bound(int(k)) for k in n], dtype=torch.float64)
        finite = n > 0
        if lst["pattern"] == "nonfinite":
            finite &= ~lst["dummy"]
        for key in ("w64", "w8"):
            s = torch.zeros(lst["R"], dtype=torch.float64).index_add_(0, ray, r[key]["softmax"].double())
            err = (s - 1.0).abs()
            assert (err[finite] <= bound[finite]).all(), (name, key, (err / bound)[finite].max().item())
            worst = max(worst, (err / bound)[finite].max().item())
    print("largest |sum - 1| / bound: %.3f" % worst)


def test_equal_logits_give_exactly_one_nth(runs):
    """expf(0) is 1 and a sum of n <= 200 ones is exact: every value is float32(1) / float32(n), whoever's expf."""
    seen = 0
    for name, r in runs.items():
        lst = r["lst"]
        if lst["pattern"] != "equal":
            continue
        n = torch.tensor(lst["counts"])[rr.ray_of(lst["off"])].float()
        exp = torch.ones_like(n) / n
        first = lst["off"][:-1].long()
        first = torch.where(torch.tensor(lst["counts"]) > 0, first, torch.full_like(first, lst["P"]))
        for key in ("w64", "w8"):
            assert torch.equal(r[key]["softmax"], exp), (name, key)
            assert torch.equal(r[key]["max_pair_id"][:lst["R"]], first), (name, key)     # all tied: the first pair
        seen += 1
    assert seen == len(rr.STRUCTURES)


def test_argmax_on_exact_duplicates(runs):
    """Two exact copies of the maximum, in another lane, in the same lane one stride on, in the last pair: the
    lowest copy's index, and both copies carry the same softmax bits."""
    r = runs["duplicates"]
    lst = r["lst"]
    for key in ("w64", "w8"):
        mid = r[key]["max_pair_id"][:lst["R"]]
        assert torch.equal(mid, lst["expect"]), (key, (mid != lst["expect"]).nonzero().flatten().tolist())
        sm = r[key]["softmax"]
        top = torch.zeros(lst["R"]).scatter_reduce(0, rr.ray_of(lst["off"]), sm, reduce="amax")
        assert torch.equal(sm[mid], top)
        assert ((sm == top[rr.ray_of(lst["off"])]).long().bincount(minlength=2)[1]) == 2 * lst["R"]


def test_argmax_against_float64(runs):
    """On a random list the id is the float64 arg-max wherever the float64 softmax decides it (the two largest values
    differ by more than 4 max|ref32 - ref64| + 2^-22, relative to the larger: util.check_selection's rule); on the
    other rays, at most 1 % of the non-empty ones, the selected pair's float64 value lies within that of the
    maximum."""
    for name, r in runs.items():
        lst = r["lst"]
        if lst["pattern"] not in rr.RANDOM_PATTERNS:
            continue
        sm64, id64, _ = r["ref64"]
        decided, tol = rr.decided_rays(sm64, r["ref32"][0], lst["off"])
        nonempty = torch.tensor(lst["counts"]) > 0
        weak = nonempty & ~decided
        assert int(weak.sum()) <= rr.MAX_WEAK_FRACTION * int(nonempty.sum()), (name, int(weak.sum()))
        top, _ = rr.top_two(sm64, lst["off"])
        for key in ("w64", "w8"):
            mid = r[key]["max_pair_id"][:lst["R"]]
            assert torch.equal(mid[decided], id64[decided]), (name, key)
            assert (mid[~nonempty] == lst["P"]).all() and (mid[nonempty] < lst["P"]).all(), (name, key)
            if weak.any():
                assert ((top[weak] - sm64[mid[weak]]) <= tol * top[weak]).all(), (name, key)


def test_empty_and_nonfinite_rays_select_the_dummy_row(runs):
    """No pair, a NaN or +inf logit, all -inf: id P, position exactly 0, depth 0 at the ray's pixel; the ray's
    softmax entries are NaN where the twin's are, and its finite neighbours in the group are untouched by it."""
    r = runs["nonfinite"]
    lst = r["lst"]
    sm64, id64, pp64 = r["ref64"]
    dummy = lst["dummy"]
    assert torch.equal(id64 == lst["P"], dummy)
    for key in ("w64", "w8"):
        o = r[key]
        mid = o["max_pair_id"][:lst["R"]]
        assert torch.equal(mid, id64), (key, mid.tolist(), id64.tolist())
        assert (o["pred_pos"][:lst["R"]][dummy] == 0).all()
        assert (o["depth"][r["bid"][:lst["R"]].long(), r["flat"][:lst["R"]].long()][dummy] == 0).all()
        assert torch.equal(torch.isnan(o["softmax"]), torch.isnan(sm64)), key
        fin = ~torch.isnan(sm64)
        assert_f64_close("nonfinite %s, finite rays" % key, o["softmax"][fin], sm64[fin], r["ref32"][0][fin])
    # every list's empty rays
    for name, q in runs.items():
        empty = torch.tensor(q["lst"]["counts"]) == 0
        for key in ("w64", "w8"):
            assert (q[key]["max_pair_id"][:q["lst"]["R"]][empty] == q["lst"]["P"]).all(), (name, key)
            assert (q[key]["pred_pos"][:q["lst"]["R"]][empty] == 0).all(), (name, key)
