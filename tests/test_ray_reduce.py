"""CPU: the twin of lidf_ray_reduce_kernel (tests/ray_reduce_ref.py) against the oracle's scatter_softmax /
scatter_max, the two lane widths' summation orders against each other, and the caps of the lists the GPU test
(tests/test_ray_reduce_gpu.py) runs."""
import numpy as np
import pytest
import torch

import ray_reduce_ref as rr
from util import orc


def _exponentials(n, seed, pattern):
    """What the kernel sums for a ray of n pairs: float32 exp(p - max), numpy's exp standing in for the device's."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.05, 1.05, n) if pattern == "uniform" else rng.normal(0.0, 3.0, n)
    p = p.astype(np.float32)
    return np.exp(p - p.max()).astype(np.float32)


def _sum_serial_8(e):
    """The order the 8-lane form had before it took the canonical one: one accumulator per lane, then the butterfly."""
    s = np.zeros(8, dtype=np.float32)
    for k in range(e.shape[0]):
        s[k % 8] = s[k % 8] + e[k]
    lane = np.arange(8)
    for stride in (4, 2, 1):
        s = s + s[lane ^ stride]
    return s[0]


def test_both_widths_sum_in_one_order():
    """sum_order_8 and sum_order_64 agree bit for bit on every length from 1 to 200 (8 draws each, two patterns);
    the one-accumulator order does not, so the comparison can tell the orders apart."""
    differ_old = 0
    for n in range(1, 201):
        for k in range(8):
            e = _exponentials(n, 1000 * n + k, ("uniform", "normal")[k % 2])
            a, b = rr.sum_order_8(e), rr.sum_order_64(e)
            assert a.dtype == b.dtype == np.float32
            assert a.tobytes() == b.tobytes(), (n, k, float(a), float(b))
            differ_old += _sum_serial_8(e).tobytes() != b.tobytes()
            if n <= 8:
                assert _sum_serial_8(e).tobytes() == b.tobytes()       # zeros in the missing slots add exactly
    print("one accumulator per lane differs from the canonical order on %d of 1600 rays" % differ_old)
    assert differ_old > 0


def test_summation_orders_propagate_nonfinite():
    e = np.ones(70, dtype=np.float32)
    e[69] = np.nan
    assert np.isnan(rr.sum_order_8(e)) and np.isnan(rr.sum_order_64(e))
    assert rr.sum_order_8(np.ones(200, np.float32)) == rr.sum_order_64(np.ones(200, np.float32)) == 200.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_twin_matches_the_oracle_on_finite_lists(dtype):
    for lst in rr.random_lists():
        if lst["R"] > 200 and lst["pattern"] != "uniform":
            continue                                     # (scatter_max is a Python loop over the pairs)
        ray = rr.ray_of(lst["off"])
        sm, mid, pp = rr.reduce_ref(lst["prob"], lst["off"], lst["pos"], dtype)
        sm_ref = orc.scatter_softmax(lst["prob"].to(dtype), ray, lst["R"])
        assert sm.dtype == dtype and torch.equal(sm, sm_ref), lst["name"]
        _, id_ref = orc.scatter_max(sm_ref, ray, lst["R"])
        assert torch.equal(mid, id_ref), lst["name"]
        exp = torch.cat((lst["pos"].to(dtype), torch.zeros(1, 3, dtype=dtype)))[id_ref]
        assert torch.equal(pp, exp), lst["name"]


def test_twin_on_ties_empties_and_nonfinite_rays():
    lst = rr.duplicate_list()
    sm, mid, _ = rr.reduce_ref(lst["prob"], lst["off"], lst["pos"], torch.float64)
    assert torch.equal(mid, lst["expect"])
    lst = rr.nonfinite_list()
    for dtype in (torch.float32, torch.float64):
        sm, mid, pp = rr.reduce_ref(lst["prob"], lst["off"], lst["pos"], dtype)
        assert torch.equal(mid == lst["P"], lst["dummy"])
        assert (pp[lst["dummy"]] == 0).all()
        ray = rr.ray_of(lst["off"])
        nonempty = torch.tensor(lst["counts"]) > 0
        assert torch.equal(torch.isnan(sm), (lst["dummy"] & nonempty)[ray])     # a ray is NaN as a whole or not at all
    # the rays of tests/test_edge_gpu.py::test_ray_reduce_nonfinite_logits
    inf, nan = float("inf"), float("nan")
    prob = torch.tensor([0.1, 0.5, 0.2, nan, nan, nan, -inf, -inf, -inf, inf, 1.0, 2.0])
    off = torch.tensor([0, 3, 6, 9, 9, 12])
    _, mid, pp = rr.reduce_ref(prob, off, torch.ones(12, 3), torch.float32)
    assert mid.tolist() == [1, 12, 12, 12, 12] and (pp[1:] == 0).all()


def test_lists_stay_inside_their_caps():
    lists = rr.all_lists()
    assert len({l["name"] for l in lists}) == len(lists)
    seen = set()
    for lst in lists:
        assert lst["P"] <= (rr.MAX_PAIRS if lst["R"] > 1000 else rr.MAX_PAIRS_SMALL), (lst["name"], lst["P"])
        assert lst["P"] > 8 * lst["R"]                          # the 64-lane form as given ...
        off8, R8 = rr.padded(lst)
        assert lst["P"] <= 8 * R8 and torch.equal(off8[:lst["R"] + 1], lst["off"])   # ... the 8-lane form padded
        seen |= set(lst["counts"])
        if lst["pattern"] in rr.RANDOM_PATTERNS:
            sm64 = rr.reduce_ref(lst["prob"], lst["off"], lst["pos"], torch.float64)[0]
            sm32 = rr.reduce_ref(lst["prob"], lst["off"], lst["pos"], torch.float32)[0]
            decided, tol = rr.decided_rays(sm64, sm32, lst["off"])
            nonempty = int((torch.tensor(lst["counts"]) > 0).sum())
            weak = nonempty - int(decided.sum())
            assert tol < 1e-5, (lst["name"], tol)
            assert weak <= rr.MAX_WEAK_FRACTION * nonempty, (lst["name"], weak, nonempty)
    assert seen >= set(rr.LENGTHS)
    assert {l["R"] for l in lists} >= set(rr.RAY_COUNTS)
    groups = rr.STRUCTURES["groups"]
    quads = [groups[i:i + 4] for i in range(0, len(groups), 4)]
    assert any(max(q) <= 8 for q in quads) and any(8 < max(q) <= 64 and min(q) <= 8 for q in quads)
    assert any(max(q) > 64 and min(q) <= 8 for q in quads)     # a short ray beside a long one, in the loop with it
