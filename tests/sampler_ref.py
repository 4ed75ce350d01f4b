"""numpy twin of implicit_depth_amd/csrc/lidf_sample.hip (lidf_sample_valid_points) — the same Philox4x32-10,
the same Feistel bijection with cycle walking, the same multiply-high, bit for bit — and check_sample(), the
structural checker of the sampler's semantics (include/lidf_hip.h; utils/point_utils.py:79-125 of the
reference), which judges the reference's own outputs, the twin's and the device's alike."""
import numpy as np

M32 = 0xFFFFFFFF
ROUNDS = 6
KEY_WORD = 0x80000000


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """One Philox4x32-10 block. c3 may be a numpy uint64 array (values < 2^32): the block of every slot at once."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    m = np.uint64(M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m, p1 >> np.uint64(32), p1 & m
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _mix(v):
    m = np.uint64(M32)
    v = v ^ (v >> np.uint64(16)); v = (v * np.uint64(0x7FEB352D)) & m
    v = v ^ (v >> np.uint64(15)); v = (v * np.uint64(0x846CA68B)) & m
    return v ^ (v >> np.uint64(16))


def perm(x, N, key):
    """The keyed bijection of [0, N) at every element of x (uint64 array, values < N)."""
    N = int(N)
    bits = (N - 1).bit_length() if N > 1 else 0
    h = np.uint64((bits + 1) >> 1)
    m = np.uint64((1 << int(h)) - 1)
    x = np.array(x, dtype=np.uint64)
    out = np.empty_like(x)
    todo = np.arange(x.shape[0])
    while todo.size:
        L, R = x >> h, x & m
        for r in range(ROUNDS):
            t = L ^ (_mix((R + np.uint64(key[r])) & np.uint64(M32)) & m)
            L, R = R, t
        x = (L << h) | R
        done = x < np.uint64(N)
        out[todo[done]] = x[done]
        todo, x = todo[~done], x[~done]
    return out


def block_order(mask_img):
    """Flat pixel ids y*w+x of the non-zero pixels of one [h,w] image in block order (NaN is non-zero)."""
    h, w = mask_img.shape
    nz = np.asarray(mask_img != 0)
    ids = np.arange(h * w).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    return ids[nz.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)]


def image_ranks(cnt, n, b, seed, counter):
    """The block-order rank of every slot of image b (int64 [n]); cnt > 0."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    k0, k1, c0, c1 = seed & M32, seed >> 32, counter & M32, counter >> 32
    key = [int(v) for v in philox4x32_10(c0, c1, b, KEY_WORD, k0, k1)]
    key += [int(v) for v in philox4x32_10(c0, c1, b, KEY_WORD + 1, k0, k1)]
    slots = np.arange(n, dtype=np.uint64)
    if cnt >= n:
        step = cnt // n
        inum = cnt // step
        j = perm(slots, inum, key)
        off = np.zeros(n, dtype=np.uint64)
        if step > 1:
            r0 = philox4x32_10(c0, c1, b, slots, k0, k1)[0]
            off = (r0 * np.uint64(step)) >> np.uint64(32)
        return (j * np.uint64(step) + off).astype(np.int64)
    M = ((n + cnt - 1) // cnt - 1) * cnt
    rank = np.arange(n, dtype=np.int64)
    rank[cnt:] = (perm(slots[: n - cnt], M, key) % np.uint64(cnt)).astype(np.int64)
    return rank


def sample_valid_points(mask, n, seed, counter):
    """(idx int64 [bs*n,2], valid_cnt int32 [bs]) exactly as lidf_sample_valid_points writes them."""
    mask = np.asarray(mask)
    bs = mask.shape[0]
    idx = np.zeros((bs * n, 2), dtype=np.int64)
    cnts = np.zeros(bs, dtype=np.int32)
    for b in range(bs):
        order = block_order(mask[b])
        cnts[b] = order.shape[0]
        idx[b * n:(b + 1) * n, 0] = b
        if order.shape[0]:
            idx[b * n:(b + 1) * n, 1] = order[image_ranks(order.shape[0], n, b, seed, counter)]
    return idx, cnts


def check_sample(mask, n, out):
    """Assert that out [bs*n,2] is a possible result of the sampler for mask [bs,h,w] (every image non-empty):
    dense images hold n points of n distinct intervals of `step` consecutive block-order ranks, none at a rank
    >= inum*step; sparse images hold every valid point in block order first, then n - cnt points whose
    multiplicities do not exceed the pool's ceil(n/cnt) - 1 copies. Returns the per-image ranks."""
    mask, out = np.asarray(mask), np.asarray(out)
    bs = mask.shape[0]
    assert out.shape == (bs * n, 2), out.shape
    ranks = []
    for b in range(bs):
        o = out[b * n:(b + 1) * n]
        assert (o[:, 0] == b).all(), "image ids of image %d" % b
        order = block_order(mask[b])
        cnt = order.shape[0]
        assert cnt > 0, "image %d has no valid pixel" % b
        pos = np.full(mask.shape[1] * mask.shape[2], -1, dtype=np.int64)
        pos[order] = np.arange(cnt)
        assert ((o[:, 1] >= 0) & (o[:, 1] < pos.shape[0])).all()
        r = pos[o[:, 1]]
        assert (r >= 0).all(), "image %d: a sampled pixel is not valid" % b
        if cnt >= n:
            step = cnt // n
            inum = cnt // step
            assert (r < inum * step).all(), "image %d: rank beyond inum*step" % b
            assert np.unique(r // step).shape[0] == n, "image %d: intervals not distinct" % b
        else:
            assert (r[:cnt] == np.arange(cnt)).all(), "image %d: head is not every valid point in order" % b
            mult = -(-n // cnt) - 1
            assert np.bincount(r[cnt:], minlength=cnt).max() <= mult, "image %d: more copies than the pool" % b
        ranks.append(r)
    return ranks


def chi_square(mask_img, n, sampler, calls):
    """Pearson's chi-square of the per-rank inclusion counts over `calls` samples of one image against the
    uniform expectation over the live ranks. sampler(k) -> flat ids [n] of call k. Returns (statistic, dof,
    counts of the dead ranks >= inum*step summed). For sparse images only the n - cnt drawn slots count."""
    order = block_order(mask_img)
    cnt = order.shape[0]
    pos = np.full(mask_img.size, -1, dtype=np.int64)
    pos[order] = np.arange(cnt)
    live = (cnt // (cnt // n)) * (cnt // n) if cnt >= n else cnt
    counts = np.zeros(cnt, dtype=np.int64)
    for k in range(calls):
        r = pos[np.asarray(sampler(k))]
        counts += np.bincount(r[cnt:] if cnt < n else r, minlength=cnt)
    exp = counts[:live].sum() / live
    stat = float(((counts[:live] - exp) ** 2 / exp).sum())
    return stat, live - 1, int(counts[live:].sum())


def chi_bound(dof):
    """Mean of the chi-square distribution plus six standard deviations."""
    return dof + 6.0 * (2.0 * dof) ** 0.5
