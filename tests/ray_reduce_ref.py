"""A plain twin of lidf_ray_reduce_kernel (csrc/lidf_aux.hip) for the tests: the per-ray softmax, arg-max and
selected position of a CSR pair list at float64 or float32, a float32 replay of the order in which each lane
width sums a ray's exponentials, and the pair lists tests/test_ray_reduce.py (CPU) and
tests/test_ray_reduce_gpu.py share. numpy / torch on the CPU only; never used by the product."""
import math

import numpy as np
import torch


def ray_of(off):
    """[P] int64: the ray of every pair of the CSR offsets `off` [R + 1]."""
    off = torch.as_tensor(off).long()
    return torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])


def reduce_ref(prob, off, pos, dtype):
    """(softmax [P], max_pair_id [R] int64, pred_pos [R, 3]) of f32 logits `prob` [P], offsets `off` [R + 1] and
    positions `pos` [P, 3], evaluated in `dtype`. The exponent argument is p - max of the ray; ties go to the lowest
    pair index; a ray without a pair, or without a softmax value that compares greater than -inf (any NaN or +inf
    logit, or all -inf: every value of the ray is NaN then), selects the dummy row: id P, position 0."""
    off = torch.as_tensor(off).long()
    R, P = off.numel() - 1, int(off[-1])
    ray = ray_of(off)
    p = prob.detach().cpu().to(dtype)
    ninf = torch.full((R,), -float("inf"), dtype=dtype)
    mx = ninf.scatter_reduce(0, ray, p, reduce="amax", include_self=True)
    e = (p - mx[ray]).exp()
    sm = e / torch.zeros(R, dtype=dtype).index_add_(0, ray, e)[ray]
    v = torch.where(torch.isnan(sm), torch.full_like(sm, -float("inf")), sm)      # a NaN never compares greater
    top = ninf.scatter_reduce(0, ray, v, reduce="amax", include_self=True)
    cand = torch.where((v == top[ray]) & (v > -float("inf")), torch.arange(P), torch.full((P,), P))
    mid = torch.full((R,), P, dtype=torch.long).scatter_reduce(0, ray, cand, reduce="amin", include_self=True)
    pp = torch.cat((pos.detach().cpu().to(dtype), torch.zeros(1, 3, dtype=dtype)))[mid]
    return sm, mid, pp


# ----------------------------------------------------------------------------------------------
# the summation order, replayed in float32 (numpy float32 addition is IEEE, like the device's v_add_f32)
# ----------------------------------------------------------------------------------------------
def sum_order_64(e):
    """The canonical order, as the 64-lane form runs it: lane = slot j adds e[j], e[j + 64], ... in ascending order
    from 0.f; then every lane adds its partner's value at strides 32, 16, 8, 4, 2, 1."""
    e = np.asarray(e, dtype=np.float32)
    s = np.zeros(64, dtype=np.float32)
    for k in range(e.shape[0]):
        s[k % 64] = s[k % 64] + e[k]
    lane = np.arange(64)
    for stride in (32, 16, 8, 4, 2, 1):
        s = s + s[lane ^ stride]
    return s[0]


def sum_order_8(e):
    """The 8-lane form: lane l keeps eight accumulators a[l, q] for the slots l + 8 q (pair k of the ray goes to
    lane k % 8, q = (k / 8) % 8), adds them up in-lane as q ^ 4, q ^ 2, q ^ 1, then the lanes' butterfly 4, 2, 1."""
    e = np.asarray(e, dtype=np.float32)
    a = np.zeros((8, 8), dtype=np.float32)
    for k in range(e.shape[0]):
        l, q = k % 8, (k // 8) % 8
        a[l, q] = a[l, q] + e[k]
    for h in (4, 2, 1):
        a = a[:, :h] + a[:, h:2 * h]
    s = a[:, 0]
    lane = np.arange(8)
    for stride in (4, 2, 1):
        s = s + s[lane ^ stride]
    return s[0]


# ----------------------------------------------------------------------------------------------
# the pair lists of the kernel's own tests
# ----------------------------------------------------------------------------------------------
# the smallest lengths at which each path and boundary exists: the fast paths end at 8 and 64 pairs, a lane's second
# element starts at 9 and 65, its accumulator q wraps at 65 (8 lanes) and the third element starts at 129 (64 lanes)
LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)

# groups of four rays (one group of the kernel): all four within 8 (fast at both widths), all within 64 (fast at 64
# lanes, the loop at 8), and short rays beside one beyond 64 (the loop at both widths)
GROUPS = ((0, 1, 2, 7), (8, 8, 7, 1),
          (9, 0, 8, 64), (63, 15, 16, 17), (1, 9, 2, 7),
          (65, 0, 1, 8), (127, 64, 9, 2), (128, 129, 7, 63), (200, 16, 0, 17), (15, 200, 65, 128))

# ray counts: 1, 3, 4, 5 (below, at and above one group of four), 127 and 129 (around the 128 rays of an 8-lane
# workgroup, 8 workgroups of the 64-lane form's 16), 1001 (8 and 63 workgroups, not a multiple of 4)
_CYCLE = (9, 0, 17, 1, 8, 65, 2, 7, 16, 15, 63, 0)          # mean 16.9
_CYCLE_1001 = (9, 8, 7, 9, 17, 2, 9, 0, 16, 9, 1, 15)       # mean 8.5: just above the 8 pairs per ray of the switch
_LONG = (63, 64, 65, 127, 128, 129, 200)


def _counts(R):
    if R <= 5:
        return {1: (200,), 3: (9, 0, 65), 4: (17, 1, 129, 8), 5: (64, 0, 9, 2, 15)}[R]
    if R < 1000:
        return tuple(_CYCLE[r % len(_CYCLE)] for r in range(R))
    c = [_CYCLE_1001[r % len(_CYCLE_1001)] for r in range(R)]
    for j, r in enumerate(range(50, R, 97)):                 # a long ray now and then, every length once or twice
        c[r] = _LONG[j % len(_LONG)]
    return tuple(c)


RAY_COUNTS = (1, 3, 4, 5, 127, 129, 1001)
STRUCTURES = dict([("groups", tuple(n for g in GROUPS for n in g))] + [("R%d" % R, _counts(R)) for R in RAY_COUNTS])
PATTERNS = ("normal", "uniform", "spread", "equal")
RANDOM_PATTERNS = ("normal", "uniform", "spread")

# The caps of the lists (tests/test_ray_reduce.py asserts them): a list forces the 64-lane form by holding more than
# 8 pairs per ray, so the 1,001-ray list needs more than 8,008 pairs; every other list stays below 4,000.
MAX_PAIRS = 10000
MAX_PAIRS_SMALL = 4000
MAX_WEAK_FRACTION = 0.01     # rays of a random list whose arg-max the float64 reference does not decide


def _off(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    return torch.from_numpy(off).int()


def _pos(P, g):
    return torch.randn(P, 3, generator=g)


def _logits(pattern, P, g):
    if pattern == "normal":
        return 3.0 * torch.randn(P, generator=g)
    if pattern == "uniform":                                 # what the decoders' output clamp leaves
        return torch.rand(P, generator=g) * 1.1 - 0.05
    if pattern == "spread":                                  # exponentials underflow below the maximum - 87.3
        return torch.rand(P, generator=g) * 160.0 - 80.0
    assert pattern == "equal"
    return torch.full((P,), 0.37)


def _list(name, counts, prob, g, **extra):
    off = _off(counts)
    P = int(off[-1])
    assert prob.shape == (P,) and prob.dtype == torch.float32
    assert P > 8 * len(counts), (name, P, len(counts))       # as given, the launcher takes the 64-lane form
    d = {"name": name, "counts": tuple(counts), "off": off, "prob": prob.contiguous(), "pos": _pos(P, g), "P": P,
         "R": len(counts)}
    d.update(extra)
    return d


def random_lists():
    """Every structure with every logit pattern."""
    out = []
    for si, (sname, counts) in enumerate(STRUCTURES.items()):
        for pi, pat in enumerate(PATTERNS):
            g = torch.Generator().manual_seed(1000 + 10 * si + pi)
            out.append(_list("%s-%s" % (sname, pat), counts, _logits(pat, sum(counts), g), g, pattern=pat))
    return out


def duplicate_list():
    """Rays whose maximum occurs twice, exactly: the second copy in the next lane, in the same lane one stride on
    (+8 at 8 lanes, +64 at 64 lanes, where +8 is another lane) and in the ray's last pair. `expect` holds the lowest
    copy's pair index per ray."""
    g = torch.Generator().manual_seed(77)
    counts, chunks, expect, beg = [], [], [], 0
    for n in (9, 17, 65, 129, 200):
        for a in (0, 3):
            for b in (a + 1, a + 8, a + 64, n - 1):
                if b >= n or b == a:
                    continue
                p = torch.rand(n, generator=g) * 1.1 - 0.05
                p[a] = p[b] = 1.25
                counts.append(n)
                chunks.append(p)
                expect.append(beg + a)
                beg += n
    d = _list("duplicates", counts, torch.cat(chunks), g, pattern="duplicates")
    d["expect"] = torch.tensor(expect, dtype=torch.long)
    return d


NONFINITE_LENGTHS = (3, 9, 64, 70)     # the fast path at both widths; the loop at 8 and fast at 64 (twice); both loops


def nonfinite_list():
    """The rays of test_ray_reduce_nonfinite_logits at every length of NONFINITE_LENGTHS, eight rays (two groups)
    per length so that a group's path depends on its length alone: finite, all NaN, all -inf, +inf among finite;
    then empty, one NaN as the last pair, -inf among finite (a finite ray: those pairs weigh 0), finite."""
    g = torch.Generator().manual_seed(78)
    inf, nan = float("inf"), float("nan")
    counts, chunks, dummy = [], [], []
    for n in NONFINITE_LENGTHS:
        def fin():
            return torch.rand(n, generator=g) * 2.0 - 0.5
        rays = [fin(), torch.full((n,), nan), torch.full((n,), -inf), fin(), None, fin(), fin(), fin()]
        rays[3][0] = inf
        rays[5][n - 1] = nan
        rays[6][1::2] = -inf
        want = [False, True, True, True, True, True, False, False]
        for r, w in zip(rays, want):
            counts.append(0 if r is None else n)
            dummy.append(w)
            if r is not None:
                chunks.append(r)
    d = _list("nonfinite", counts, torch.cat(chunks), g, pattern="nonfinite")
    d["dummy"] = torch.tensor(dummy)
    return d


def all_lists():
    return random_lists() + [duplicate_list(), nonfinite_list()]


def padded(lst):
    """The same rays followed by empty ones until P <= 8 R': the launcher takes the 8-lane form. Returns (off', R')."""
    Rp = -(-lst["P"] // 8)
    off = torch.cat((lst["off"], torch.full((Rp - lst["R"],), lst["P"], dtype=torch.int32)))
    assert Rp > lst["R"] and lst["P"] <= 8 * Rp and off.numel() == Rp + 1
    return off, Rp


def selection_tolerance(sm64, sm32):
    """util.check_selection's rule on the softmax: 4 x the float32 twin's largest error plus 2^-22."""
    return 4.0 * (sm32.double() - sm64).abs().max().item() + 2.0 ** -22


def top_two(sm64, off):
    """Per ray: the largest float64 softmax value and the runner-up (0 where the ray has fewer than two pairs)."""
    off = torch.as_tensor(off).long()
    R = off.numel() - 1
    ray = ray_of(off)
    top = torch.zeros(R, dtype=torch.float64).scatter_reduce(0, ray, sm64, reduce="amax", include_self=True)
    first = torch.full((R,), sm64.numel(), dtype=torch.long).scatter_reduce(
        0, ray, torch.where(sm64 == top[ray], torch.arange(sm64.numel()), torch.full_like(ray, sm64.numel())),
        reduce="amin", include_self=True)
    rest = sm64.clone()
    rest[first[first < sm64.numel()]] = 0.0
    second = torch.zeros(R, dtype=torch.float64).scatter_reduce(0, ray, rest, reduce="amax", include_self=True)
    return top, second


def decided_rays(sm64, sm32, off):
    """[R] bool: non-empty rays whose two largest float64 softmax values differ by more than the tolerance, relative
    to the larger; and the tolerance."""
    tol = selection_tolerance(sm64, sm32)
    top, second = top_two(sm64, off)
    off = torch.as_tensor(off).long()
    nonempty = off[1:] > off[:-1]
    return nonempty & ((top - second) > tol * top), tol


def unit_sum_bound(n):
    """|sum of a finite ray's softmax - 1| in units of 2^-24: the butterfly's 6 levels, the ceil(n / 64) - 1 serial
    additions of a slot, and the division."""
    return (6 + math.ceil(n / 64)) * 2.0 ** -24
