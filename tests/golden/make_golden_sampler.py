"""make_golden_sampler.py — g11_sample_valid.npz: the REFERENCE's own utils/point_utils.py sample_valid_points on
a handful of small masks, for tests/test_sample_valid.py to validate tests/sampler_ref.py's check_sample on (and
to pin the parts of the sampler that are deterministic in the reference: block order, the head of a sparse
image, the cnt == n image).

Per case k: mask_k (the [bs,h,w] 0/1 mask, np.packbits of its flat form), shape_k, n_k, ref_k int32 [bs*n] (the flat
pixel column of the reference's output; its image column is b for slots b*n .. b*n+n-1, asserted here). Plus the reference's chi-square statistics of the
two uniformity set-ups (chi_dense, chi_sparse with their masks and n) over CHI_CALLS calls, and empty_raises: the
reference dies with an AssertionError on a batch that holds an all-zero image.

The reference module imports cv2 and matplotlib (not installed, not used by the sampler): stubbed, as
make_golden.py does. Its sparse branch hands a 0-dim tensor to np.random.choice as the size, which today's numpy
refuses: np.random.choice is wrapped so that the size becomes an int — nothing else about the call changes.

    python tests/golden/make_golden_sampler.py
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/src"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "utils"))

import sampler_ref as sr  # noqa: E402

CHI_CALLS = 2000


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def reference_sampler():
    _stub("cv2")
    mpl = _stub("matplotlib")
    mpl.pyplot = _stub("matplotlib.pyplot")
    tk = _stub("mpl_toolkits")
    tk.mplot3d = _stub("mpl_toolkits.mplot3d")
    import point_utils
    choice = np.random.choice

    def choice_int_size(a, size=None, replace=True, p=None):
        return choice(a, int(size) if size is not None else None, replace=replace, p=p)

    point_utils.np.random.choice = choice_int_size
    return point_utils.sample_valid_points


def density_mask(rng, shape, density):
    return (rng.random(shape) < density).astype(np.uint8)


def exact_mask(rng, shape, cnt):
    """One image with exactly cnt valid pixels."""
    m = np.zeros(int(np.prod(shape)), dtype=np.uint8)
    m[rng.choice(m.shape[0], cnt, replace=False)] = 1
    return m.reshape(shape)


def uniformity_masks():
    rng = np.random.default_rng(1107)
    return exact_mask(rng, (1, 16, 24), 344), 40, exact_mask(rng, (1, 16, 24), 45), 100


def main():
    ref = reference_sampler()
    rng = np.random.default_rng(20261018)
    np.random.seed(11)
    torch.manual_seed(11)
    few = np.zeros((1, 8, 8), dtype=np.uint8)
    few.reshape(-1)[[3, 17, 40, 63]] = 1
    # density 0.5 with one image on either side of n = 128: image 0 sparse (cnt 100), image 1 dense (cnt 150)
    mixed = np.concatenate((exact_mask(rng, (1, 16, 16), 100), exact_mask(rng, (1, 16, 16), 150)), 0)
    cases = [
        (density_mask(rng, (2, 16, 24), 0.9), 40),
        (density_mask(rng, (2, 16, 24), 0.3), 100),
        (np.ones((1, 8, 8), dtype=np.uint8), 64),
        (few, 64),
        (mixed, 128),
        (density_mask(rng, (3, 240, 320), 0.7), 10000),
    ]
    out = {"n_cases": np.int64(len(cases))}
    for k, (mask, n) in enumerate(cases):
        got = ref(torch.from_numpy(mask.astype(np.float32)), n).numpy()
        sr.check_sample(mask, n, got)
        out["mask_%d" % k] = np.packbits(mask.reshape(-1))
        out["shape_%d" % k] = np.array(mask.shape, dtype=np.int64)
        out["n_%d" % k] = np.int64(n)
        out["ref_%d" % k] = got[:, 1].astype(np.int32)   # (the image column is b for slots b*n .. b*n+n-1: checked)
        assert (got[:, 0] == np.repeat(np.arange(mask.shape[0]), n)).all()
        cnts = [int(m.sum()) for m in mask]
        print("case %d: shape %s n %d cnt %s" % (k, mask.shape, n, cnts))
    md, nd, ms, ns = uniformity_masks()
    for name, mask, n in (("dense", md, nd), ("sparse", ms, ns)):
        t = torch.from_numpy(mask.astype(np.float32))
        stat, dof, dead = sr.chi_square(mask[0], n, lambda k: ref(t, n).numpy()[:, 1], CHI_CALLS)
        print("chi %s: %.1f (dof %d, bound %.1f), dead-rank count %d" % (name, stat, dof, sr.chi_bound(dof), dead))
        out["chi_%s" % name] = np.float64(stat)
        out["chi_%s_dof" % name] = np.int64(dof)
        out["chi_%s_dead" % name] = np.int64(dead)
        out["chi_%s_mask" % name] = mask
        out["chi_%s_n" % name] = np.int64(n)
    try:
        ref(torch.zeros((2, 8, 8)).index_put_((torch.tensor([0]), torch.tensor([1]), torch.tensor([2])),
                                              torch.tensor(1.0)), 4)
        out["empty_raises"] = np.bool_(False)
    except AssertionError:
        out["empty_raises"] = np.bool_(True)
    print("all-zero image raises AssertionError in the reference:", bool(out["empty_raises"]))
    path = os.path.join(HERE, "g11_sample_valid.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
