"""GPU: lidf_sample_valid_points (the device-side valid-point sampler) against its numpy twin, bit for bit, and
through every layer that takes LidfOptions.valid_sample_num: query.sample_valid_points, pipeline.lidf_forward /
lidf_forward_train and FrameRunner (eager and as a captured graph). The twin itself is held to the reference's
outputs and to the uniformity bound in tests/test_sample_valid.py."""
import numpy as np
import pytest
import torch

import sampler_ref as sr
from test_sample_valid import g11_cases
from util import make_module, make_pointnet, orc

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15   # a 64-bit seed with the top bit set: both halves of both state words matter


def _state(dev, counter=5):
    from implicit_depth_amd.query import sampler_state
    return sampler_state(SEED, dev, counter)


def _run(mask_t, n, state):
    """One raw launch: (bid, flat, idx, valid_cnt) as numpy."""
    from implicit_depth_amd import query as Q
    bs, h, w = mask_t.shape
    dev = mask_t.device
    bid = torch.full((bs * n,), -7, dtype=torch.int32, device=dev)
    flat = torch.full((bs * n,), -7, dtype=torch.int32, device=dev)
    idx = torch.full((bs * n, 2), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((bs,), -7, dtype=torch.int32, device=dev)
    Q.sample_valid_launch(mask_t, n, state, bid, flat, idx, cnt, Q.sample_valid_workspace(bs, h, w, dev))
    return bid.cpu().numpy(), flat.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()


def _equals_twin(mask_np, mask_t, n, dev, counter=5, check=True):
    state = _state(dev, counter)
    bid, flat, idx, cnt = _run(mask_t, n, state)
    want, want_cnt = sr.sample_valid_points(mask_np, n, SEED, counter)
    assert (cnt == want_cnt).all()
    assert (idx == want).all()
    assert (bid == want[:, 0]).all() and (flat == want[:, 1]).all()
    assert state.tolist() == _state(dev, counter + 1).tolist()   # the counter advanced on the device
    if check:
        sr.check_sample(mask_np, n, idx)
    return idx


@pytest.mark.parametrize("case", range(6))
def test_equals_twin_on_the_golden_masks(cuda, case):
    mask, n, _ = g11_cases()[case]
    _equals_twin(mask, torch.from_numpy(mask.astype(np.float32)).to(cuda), n, cuda)


def test_equals_twin_one_valid_pixel(cuda):
    mask = np.zeros((1, 8, 8), dtype=np.uint8)
    mask[0, 5, 2] = 1
    idx = _equals_twin(mask, torch.from_numpy(mask).to(cuda), 64, cuda)
    assert (idx[:, 1] == 5 * 8 + 2).all()


def test_equals_twin_more_blocks_than_threads(cuda):
    """(2,64,2048): 2,048 blocks per image, two chunks of the workgroup's scan; dense and sparse image."""
    rng = np.random.default_rng(8)
    mask = (rng.random((2, 64, 2048)) < 0.6).astype(np.uint8)
    mask[1] &= (rng.random((64, 2048)) < 0.05).astype(np.uint8)    # ~3,900 valid: sparse for n = 5000
    _equals_twin(mask, torch.from_numpy(mask).to(cuda), 5000, cuda)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.bool, torch.int32, torch.int64])
def test_mask_dtypes(cuda, dtype):
    rng = np.random.default_rng(9)
    mask = (rng.random((2, 16, 24)) < 0.5).astype(np.uint8)
    t = torch.from_numpy(mask).to(dtype)
    if dtype == torch.float32:          # NaN and a negative value count as non-zero
        zeros = np.argwhere(mask == 0)[:2]
        for (b, y, x), v in zip(zeros, (float("nan"), -2.5)):
            t[b, y, x] = v
            mask[b, y, x] = 1
    elif dtype in (torch.int32, torch.int64):
        ones = np.argwhere(mask == 1)[:2]
        t[tuple(ones[0])] = -1
        t[tuple(ones[1])] = 1 << 30 if dtype == torch.int32 else 1 << 40   # (int64: the low word alone is zero)
    _equals_twin(mask, t.to(cuda), 50, cuda)


def test_same_state_same_sample_and_identical_images_differ(cuda):
    mask, n, _ = g11_cases()[0]
    mask = np.stack((mask[0], mask[0]))
    t = torch.from_numpy(mask).to(cuda)
    state = _state(cuda, 40)
    a = _run(t, n, state)[2]
    b = _run(t, n, _state(cuda, 40))[2]
    c = _run(t, n, state)[2]                      # the state moved on: counter 41
    assert (a == b).all() and (a != c).any()
    assert (c == sr.sample_valid_points(mask, n, SEED, 41)[0]).all()
    assert (a[:n, 1] != a[n:, 1]).any()           # two identical images of one batch get different samples


def test_image_without_a_valid_pixel(cuda):
    from implicit_depth_amd import query as Q
    mask, n, _ = g11_cases()[0]
    mask = mask.copy()
    mask[1] = 0
    t = torch.from_numpy(mask.astype(np.float32)).to(cuda)
    bid, flat, idx, cnt = _run(t, n, _state(cuda))
    want, want_cnt = sr.sample_valid_points(mask, n, SEED, 5)
    assert cnt.tolist() == [int(mask[0].sum()), 0] == want_cnt.tolist()
    assert (idx == want).all() and (idx[n:] == np.array([1, 0])).all()
    sr.check_sample(mask[:1], n, idx[:n])         # the other image is unaffected
    with pytest.raises(RuntimeError, match="image 1"):
        Q.sample_valid_points(t, n, state=_state(cuda))
    got, c = Q.sample_valid_points(t, n, state=_state(cuda), return_counts=True, check=False)
    assert (got.cpu().numpy() == want).all() and c.tolist() == cnt.tolist()


def test_python_surface(cuda):
    from implicit_depth_amd import query as Q
    mask, n, _ = g11_cases()[4]
    t = torch.from_numpy(mask).to(cuda)
    state = _state(cuda, 0)
    got = Q.sample_valid_points(t.unsqueeze(1), n, state=state)
    assert got.dtype == torch.int64 and got.shape == (2 * n, 2) and got.device == t.device
    assert (got.cpu().numpy() == sr.sample_valid_points(mask, n, SEED, 0)[0]).all()
    assert state.tolist()[1] == 1
    # the default state: one per device, seeded from torch.initial_seed(), advanced by every call
    st = Q.default_sampler_state(cuda)
    assert st is Q.default_sampler_state(cuda)
    assert st.tolist()[0] == Q.sampler_state(torch.initial_seed(), cuda).tolist()[0]
    c0 = st.tolist()[1]
    got = Q.sample_valid_points(t, n)
    assert (got.cpu().numpy() == sr.sample_valid_points(mask, n, torch.initial_seed(), c0)[0]).all()
    assert st.tolist()[1] == c0 + 1
    with pytest.raises(RuntimeError):
        Q.sample_valid_points(t, n, state=torch.zeros(2, dtype=torch.int64))          # state on the host


# ---- the layers above ----------------------------------------------------------------------------------------------
def _dev(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _same(a, b, path=""):
    """Every tensor of two (nested) results bit-equal (NaN equal to NaN); 'workspace' is the query's scratch buffer,
    handed back for reuse, not a result."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype, path
        assert torch.equal(torch.nan_to_num(a.detach().float(), nan=12345.0),
                           torch.nan_to_num(b.detach().float(), nan=12345.0)) if a.is_floating_point() \
            else torch.equal(a, b), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            if k != "workspace":
                _same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, i))


def _g9(dev):
    """The 2 x 16 x 24 batch of the stage-1 training fixture (366 and 349 valid pixels) with its modules."""
    import train_loss_ref as tl
    from util import closed_form_params, closed_form_pointnet
    g, _ = tl.g9_files()
    batch, feat = tl.g9_batch(g)
    sp, so, sn = (int(v) for v in g["seeds"])
    mods = (make_pointnet(closed_form_pointnet(sn), dev),
            make_module("IMNET", closed_form_params("IMNET", 385, sp), 385, dev),
            make_module("IEF", closed_form_params("IEF", 385, so), 385, dev))
    return _dev(batch, dev), feat.to(dev), mods, int(g["miss_sample_num"])


@pytest.mark.parametrize("n", [100, 400])     # dense (step 3) and sparse
def test_lidf_forward_with_valid_sample_num(cuda, n):
    """lidf_forward with valid_sample_num = the same call given valid_idx = the twin's sample for the same state.
    (The fixture batch is the training fixture's: the g3 trace holds no images to build a batch from.)"""
    from implicit_depth_amd import pipeline as pl
    batch, feat, mods, _ = _g9(cuda)
    mask = (batch["depth_corrupt"][:, 0] != 0).cpu().numpy().astype(np.uint8)   # mask_type 'all'
    want, _ = sr.sample_valid_points(mask, n, SEED, 17)
    with torch.no_grad():
        ok, dd = pl.lidf_forward(batch, feat, *mods, opt=pl.LidfOptions(valid_sample_num=n,
                                                                          sampler_state=_state(cuda, 17)))
        ok_ref, ref = pl.lidf_forward(batch, feat, *mods, opt=pl.LidfOptions(),
                                      valid_idx=torch.from_numpy(want).to(cuda))
        # an explicit valid_idx still wins over the option
        ok_x, dx = pl.lidf_forward(batch, feat, *mods, opt=pl.LidfOptions(valid_sample_num=n),
                                   valid_idx=torch.from_numpy(want).to(cuda))
    assert ok and ok_ref and ok_x
    assert dd["valid_bid"].shape[0] == 2 * n
    _same(dd, ref)
    _same(dx, ref)
    empty = dict(batch, depth_corrupt=batch["depth_corrupt"].clone())
    empty["depth_corrupt"][1] = 0
    with pytest.raises(RuntimeError, match="image 1"), torch.no_grad():
        pl.lidf_forward(empty, feat, *mods, opt=pl.LidfOptions(valid_sample_num=n))


def test_lidf_forward_train_with_valid_sample_num(cuda):
    from implicit_depth_amd import LidfLossOptions, pipeline as pl
    batch, feat, mods, miss_n = _g9(cuda)
    mods = tuple(m.train() for m in mods)
    n = 100
    mask = (batch["valid_mask"][:, 0] != 0).cpu().numpy().astype(np.uint8)      # the train flavour's mask
    want, _ = sr.sample_valid_points(mask, n, SEED, 3)
    out = []
    for kw in (dict(opt=pl.LidfOptions(miss_sample_num=miss_n, valid_sample_num=n, sampler_state=_state(cuda, 3))),
               dict(opt=pl.LidfOptions(miss_sample_num=miss_n), valid_idx=torch.from_numpy(want).to(cuda))):
        np.random.seed(4)                          # (sample_miss_rays draws its window from numpy)
        ok, dd, loss = pl.lidf_forward_train(batch, feat, *mods, loss_opt=LidfLossOptions(), epoch=0, **kw)
        assert ok
        out.append((dd, loss))
    assert out[0][0]["valid_bid"].shape[0] == 2 * n
    _same(out[0], out[1])


def _frame_models(cuda):
    from implicit_depth_amd.synthetic import init_decoder_params
    return (make_pointnet(orc.init_pointnet(3, 1.5), cuda),
            make_module("IMNET", init_decoder_params("IMNET", 385, 7, 5.0), 385, cuda),
            make_module("IEF", init_decoder_params("IEF", 385, 8, 5.0), 385, cuda))


FRAME_KEYS = ("valid_bid", "valid_flat_img_id", "valid_xyz", "voxel_bound", "revidx", "valid_v_pid", "occ_voxel_feat",
              "ray_bid", "ray_flat", "pair_off", "pair_ray", "pair_vox", "pair_t", "pred_offset", "pred_prob_end",
              "pair_pred_pos", "max_pair_id", "pred_pos", "pred_depth")


def test_frame_runner_with_valid_sample_num(cuda):
    """enqueue() samples on the device into the runner's index buffers: the frame equals a runner fed the twin's
    sample through load(valid_idx=); captured, every replay draws the next counter's sample. The capture succeeding
    is the evidence that nothing on the way reads a size or waits."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    B, h, w, n = 2, 64, 64, 500
    models = _frame_models(cuda)
    batch, feat = synthetic_batch(B, h, w, seed=77)
    batch, feat = _dev(batch, cuda), feat.to(cuda)
    mask = (batch["depth_corrupt"][:, 0] != 0).cpu().numpy().astype(np.uint8)
    assert all(int(m.sum()) > n for m in mask)
    state = _state(cuda, 100)
    runner = pl.FrameRunner(B, h, w, cuda, *models, pl.LidfOptions(valid_sample_num=n), sampler_state=state)
    plain = pl.FrameRunner(B, h, w, cuda, *models, pl.LidfOptions())

    def reference(counter):
        want, _ = sr.sample_valid_points(mask, n, SEED, counter)
        with torch.no_grad():
            plain.run(batch, feat, valid_idx=torch.from_numpy(want).to(cuda))
        ok, ref = plain.result()
        assert ok
        return want, {k: ref[k].clone() for k in FRAME_KEYS}

    def check(dd, counter):
        want, ref = reference(counter)
        assert dd["counts"]["NVS"] == B * n
        assert (dd["valid_bid"].cpu().numpy() == want[:, 0]).all()
        assert (dd["valid_flat_img_id"].cpu().numpy() == want[:, 1]).all()
        for k in FRAME_KEYS:
            assert torch.equal(dd[k], ref[k]), k

    with torch.no_grad():
        runner.run(batch, feat)
    ok, dd = runner.result()
    assert ok
    check(dd, 100)
    with torch.no_grad():
        runner.capture()
    c = state.tolist()[1]
    assert c > 101                                # the warm-up frame of capture() drew a sample as well
    for k in range(2):
        with torch.no_grad():
            runner.run()
        ok, dd = runner.result()
        assert ok and state.tolist()[1] == c + k + 1
        check(dd, c + k)
    with pytest.raises(RuntimeError, match="captured graph"):
        runner.load(batch, feat, valid_idx=torch.zeros((4, 2), dtype=torch.int64, device=cuda))
    # an image without a valid pixel: result() names it
    empty = dict(batch, depth_corrupt=batch["depth_corrupt"].clone())
    empty["depth_corrupt"][0] = 0
    with torch.no_grad():
        runner.run(empty, feat)
    with pytest.raises(RuntimeError, match="image 0"):
        runner.result()
    with pytest.raises(ValueError):
        pl.FrameRunner(B, 60, 64, cuda, *models, pl.LidfOptions(valid_sample_num=n))
