"""GPU: every caller-workspace entry point on arbitrary workspace contents.

include/lidf_hip.h: "scratch memory comes from the caller". Except for lidf_depth_metrics_f32 (workspace zero-filled
once by the caller; a call leaves it zero) no entry states a precondition on what the workspace holds, so each must
give the same answer whatever bytes it finds. Every case here runs an entry with its workspaces pre-filled by
tests/ws_poison.py (`zeros` = the clean run; `ones` = 0xFF: NaN floats, -1 ints, all-bits status words; `high` = 0x7F:
huge finite floats, large positive ints, status words that read as finished aggregates; `random` bytes; `replay` = what the kernels left behind on another, larger input) and asserts
  * the reference of the entry's existing test, with that test's bound (imported, not restated), and
  * torch.equal (bit for bit, NaN included) with the `zeros` run — except on the paths the documents name as not
    bit-reproducible: lidf_wgrad_f32 without its workspace and lidf_ray_features_backward_f32 without a workspace
    (lidf_hip.h), and feat_grid's gradient where boxes clamp at the image border (RoIAlign backward's
    border taps are float atomics even with the workspace). Those are held to the reference, and to the run-to-run
    bound their existing tests state.
lidf_depth_metrics_f32 has the opposite contract and is checked for it. FrameRunner's persistent workspace and
buffers are poisoned in place between two batches.

Regions a kernel reads before it writes them, the call site that initialises each, and the extent (read from
csrc/ before the first poisoned run; word = 4 bytes):

  region (carve-up)                           read by                          initialised by                      extent
  ------------------------------------------  -------------------------------  ----------------------------------  ---------------------------
  frame lb_head: 2 tickets, stA/stB/stL       lidf_frame_head_kernel           lidf_frame_f32 step 0,              f.lb_bytes / 4 + C words from
   (FrameWs.lb_head, lidf_frame_head_lb_bytes)  lb_ticket / lb_exclusive (spin)   lidf_launch_zero_segments seg 0     lb_head: lb_head, lb_pairs
  frame lb_pairs: ticket + status per 256     lidf_ray_aabb_onepass_kernel      the same segment (adjacent)         (both 256-aligned) and
   rays of CAPACITY (..._onepass_lb_bytes)      lb_ticket / lb_exclusive (spin)                                      cell_flag [C], contiguous
  frame cell_flag [C]                         lidf_frame_cells_kernel (scan)    the same segment (frame_ws carves   C words
                                                                                it right behind the f.lb_bytes)
  frame pool1 [C,64] / pool2 [C,128]          pointnet chains (integer max)     step 0 segs 1, 2; per refine        C*64, C*128 words
                                                                                iteration lidf_launch_refine_step
                                                                                (zero0 / zero1) or, split-f16,
                                                                                zero_segments {end_voxel, pools}
  frame query tile counter (FrameWs.q.counter) lidf_points(_h) atomicAdd        step 0 seg 3                        1 word
  frame box list length (q.box + grid_floats) lidf_rayfeat(_border)_kernel      step 0 seg 4                        1 word
  frame group counts (FrameWs.pnet.sort, B>=2) lidf_group_count_kernel atomics  step 0 seg 5; lidf_group_scan_      C words
                                                                                kernel leaves them zero again
  frame counts[0..7], pair_off[0..R]          every later launch (n_dev)        lidf_frame_head_kernel :205-209,    all eight / R + 1 entries
                                                                                lidf_frame_cells_kernel :242,
                                                                                onepass kernel :1048-1054
  query tile counter (stepwise)               lidf_points(_h) atomicAdd         query_impl, hipMemsetAsync          4 bytes
  query box list length (stepwise)            lidf_rayfeat(_border)_kernel      lidf_launch_rayfeat_phase           4 bytes
  scan `sums` (n > 32768)                     lidf_scan_top / _final_kernel     lidf_scan_sums_kernel writes        nb words, all written
                                                                                every block's word first
  voxelize cell_flag [ncell]                  lidf_launch_scan(cell_flag)       lidf_voxelize_f32 hipMemsetAsync    ncell words
  grid cell / colmask / tab                   lidf_ray_aabb_grid_kernel         lidf_grid_init_kernel               ncell, ncol, 2*ntab: all
  refine cell table [B*rx*ry*rz]              lidf_refine_endvox_cells_kernel   lidf_launch_refine_prep_dev         nc words of 0xff (first
                                                                                hipMemsetAsync(0xff)                iteration; later: ready)
  refine end_voxel [R] (no cell table)        lidf_refine_endvox_kernel max     hipMemsetAsync                      R words
  pointnet pool1 / pool2 (stepwise)           chains / run_linear scatter-max   pointnet_impl zero_words            V*64, V*128 words
  pointnet `part` copies (V*129*4 > LDS)      global atomic max + poolmax       lidf_launch_pointnet_chain          copies * V * F words, per
                                                                                hipMemsetAsync                      stage
  pointnet sort hist / scanned / perm         lidf_seg_place_kernel, chains     lidf_seg_hist_kernel writes every   V * nblk words, all written
                                                                                [voxel][block] word; scan; place
  select histograms [n_jobs * SEL_HIST]       lidf_select_hist_kernel atomics   lidf_launch_select hipMemsetAsync   hist_bytes (aligned, whole)
  select state / partial / tie_cnt / tie_pre  lidf_select_final / _weights      written by the hist / partial /     nslab entries, all written
                                                                                final kernels of the same call      before read
  decoder train `small` [512]                 lidf_ief_finish_kernel sums       decoder_backward_core /             512 words
                                                                                qdec backward hipMemsetAsync
  wgrad slabs (WG_SCRATCH_FLOATS)             lidf_wgrad_reduce_kernel          lidf_wgrad2_kernel writes the       sp * mb * nb slabs, only
                                                                                slabs the reduce reads              those read
  packed weight streams (head of workspaces)  every matrix kernel               lidf_launch_pack* of the same call  the whole stream + aux
  depth metrics ticket + partial sums         lidf_depth_metrics_kernel         THE CALLER, once; the last          whole workspace
                                                                                workgroup clears the ticket and
                                                                                the partial sums it read

The two spin-waits of the library (lb_exclusive, lidf_device.h) read only the frame path's status words, which the
first row covers for the full capacity (R_cap, not the device-side R), so no poisoned word can be mistaken for a
predecessor's aggregate. Reading found no read-before-write region uncovered or short. The first run found the one
departure from the stated contracts: lidf_depth_metrics_kernel reset its ticket but left the partial sums in the
workspace it promises to leave as it found it (harmless to the next call, which overwrites them before reading, but
not what the header says); the last workgroup now clears them too.
"""
import zlib

import numpy as np
import pytest
import torch

import ws_poison
from entry_cases import (QUERY_KEYS, check_query as _check_query, close_rel as _close_rel, intr as _intr,
                         mask_2x16x24 as _mask_2x16x24, pointnet_case as _pointnet_case,
                         pointnet_train_case as _pointnet_train_case, query_loss as _query_loss,
                         query_scene as _query_scene, query_scene_gf32 as _query_scene_gf32,
                         query_train_case as _query_train_case, refine_case as _refine_case,
                         refine_oracle as _refine_oracle, refine_train_scene, same, scan_values as values, step_result as _step_result,
                         voxel_points as _voxel_points, voxel_ref as _voxel_ref)
from util import (K_BIAS, TOL, assert_f64_close, k_for, make_module, make_pointnet, oracle_grads, orc, run_query,
                  tf32_off, to_dev)

pytestmark = pytest.mark.gpu

MODES = ("ones", "high", "random", "replay")


@pytest.fixture
def poison(monkeypatch, request):
    """_lib.workspace replaced for this test; the random bytes are seeded by the test's id."""
    with tf32_off():
        yield ws_poison.Poisoner("zeros", seed=zlib.crc32(request.node.nodeid.encode())).install(monkeypatch)


def drive(poison, mode, run, donor=None):
    """`run()` on zero-filled workspaces, then on workspaces poisoned by `mode` (replay: with what `donor()` — by
    default run() itself — left in its workspaces). Returns (clean result, poisoned result)."""
    poison.begin("zeros")
    base = run()
    torch.cuda.synchronize()
    assert poison.handed, "the entry took no workspace from _lib.workspace"
    if mode == "replay":
        poison.begin("zeros")
        (donor or run)()
        assert poison.snapshot()
    poison.begin(mode)
    got = run()
    torch.cuda.synchronize()
    return base, got


# ------------------------------------------------------------------------------------------------------------------
# Geometry
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1025, 32768, 32769])     # 32769: the first three-launch length (`sums` in the workspace)
def test_exclusive_scan(cuda, poison, n, mode):
    from implicit_depth_amd import _lib
    L = _lib.lib()

    def scan(m):
        xd = values(m).to(cuda)
        out = torch.full((m + 1,), -7, dtype=torch.int32, device=cuda)
        wsb = L.lidf_exclusive_scan_workspace_bytes(m)
        ws = _lib.workspace(wsb, cuda)
        _lib.check(L.lidf_exclusive_scan_i32(_lib.ptr(xd), m, _lib.ptr(out), _lib.ptr(ws), wsb,
                                             _lib.current_stream(cuda)))
        torch.cuda.synchronize()
        return out

    base, got = drive(poison, mode, lambda: scan(n), donor=lambda: scan(300000 if n >= 32768 else 32769))
    ref = torch.zeros(n + 1, dtype=torch.int64)
    ref[1:] = torch.cumsum(values(n).long(), 0)
    assert (got.cpu().long() == ref).all()
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,B", [(5000, 1), (20000, 3)])
def test_get_occ_vox_bound(cuda, poison, n, B, mode):
    from implicit_depth_amd.query import get_occ_vox_bound
    from test_voxelize_gpu import check

    def run(n=n, B=B):
        xyz, bid = _voxel_points(n, B)
        return get_occ_vox_bound(xyz.to(cuda), bid.int().to(cuda), batch=B)

    base, got = drive(poison, mode, run, donor=lambda: run(*((20000, 3) if n == 5000 else (40000, 4))))
    check(got, _voxel_ref(n, B))
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_ray_aabb_voxel_list(cuda, poison, mode):
    from implicit_depth_amd.query import compute_ray_aabb
    from test_boxes_gpu import scene

    def run(R=257, V=300):
        return compute_ray_aabb(*[torch.from_numpy(a).to(cuda) for a in scene(R, V, R + V)])

    base, got = drive(poison, mode, run, donor=lambda: run(40000, 300))   # (a donor beyond the one-workgroup scan)
    d, vb, rb, vbid = scene(257, 300, 557)
    m_ref, t_ref = orc.ray_aabb(d, vb, rb, vbid)
    pr_ref, pv_ref, pt_ref, off_ref = orc.pairs_from_dense(m_ref, t_ref)
    off, pr, pv, pt = got
    assert (off.cpu().long() == off_ref).all() and (pr.cpu().long() == pr_ref).all()
    assert (pv.cpu().long() == pv_ref).all() and (pt.cpu() == pt_ref).all()
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_ray_aabb_grid_walk(cuda, poison, mode):
    from implicit_depth_amd.query import compute_ray_aabb
    from test_boxes_gpu import grid_scene

    def run(R=700, B=2, fill=0.3):
        d, vb, rb, vbid, coord = grid_scene(R, B, 9, fill, seed=R + B)
        return compute_ray_aabb(*[a.to(cuda) for a in (d, vb, rb, vbid)], voxel_coord=coord.to(cuda),
                                grid_dims=(9, 9, 9), batch=B)

    base, got = drive(poison, mode, run, donor=lambda: run(40000, 3, 0.6))
    d, vb, rb, vbid, coord = grid_scene(700, 2, 9, 0.3, seed=702)
    assert vb.shape[0] <= 600
    m_ref, t_ref = orc.ray_aabb(d.numpy(), vb.numpy(), rb.numpy(), vbid.numpy())
    pr_ref, pv_ref, pt_ref, off_ref = orc.pairs_from_dense(m_ref, t_ref)
    assert (got[0].cpu().long() == off_ref).all() and (got[1].cpu().long() == pr_ref).all()
    assert (got[2].cpu().long() == pv_ref).all() and (got[3].cpu() == pt_ref).all()
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_get_miss_ray(cuda, poison, mode):
    from implicit_depth_amd.query import get_miss_ray
    from test_miss_ray_gpu import _check

    def run(shape=(2, 16, 24)):
        B, h, w = shape
        mask = torch.from_numpy((np.random.default_rng(h * w).random(shape) < 0.4).astype(np.uint8))
        res = get_miss_ray(mask.to(cuda), *_intr(B, h, w, cuda))
        return mask, res

    (_, base), (mask, got) = drive(poison, mode, run, donor=lambda: run((4, 240, 320)))   # (a three-launch scan)
    ref = orc.get_miss_ray(mask, *[t.cpu() for t in _intr(2, 16, 24, cuda)])
    _check(got, {k: v.numpy() for k, v in ref.items() if torch.is_tensor(v)}, ref["total_miss_sample_num"])
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_sample_valid_points(cuda, poison, mode):
    import sampler_ref as sr
    from implicit_depth_amd import query as Q
    from test_sample_valid_gpu import SEED

    def run(mask_np=None, n=40):
        mask_np = _mask_2x16x24() if mask_np is None else mask_np
        bs, h, w = mask_np.shape
        mask = torch.from_numpy(mask_np).to(cuda)
        state = Q.sampler_state(SEED, cuda, 5)
        out = {"bid": torch.full((bs * n,), -7, dtype=torch.int32, device=cuda),
               "flat": torch.full((bs * n,), -7, dtype=torch.int32, device=cuda),
               "idx": torch.full((bs * n, 2), -7, dtype=torch.int64, device=cuda),
               "cnt": torch.full((bs,), -7, dtype=torch.int32, device=cuda)}
        Q.sample_valid_launch(mask, n, state, out["bid"], out["flat"], out["idx"], out["cnt"],
                              Q.sample_valid_workspace(bs, h, w, cuda))
        out["state"] = state
        return out

    big = (np.random.default_rng(8).random((2, 64, 2048)) < 0.6).astype(np.uint8)
    base, got = drive(poison, mode, run, donor=lambda: run(big, 5000))
    want, want_cnt = sr.sample_valid_points(_mask_2x16x24(), 40, SEED, 5)
    assert (got["cnt"].cpu().numpy() == want_cnt).all() and (got["idx"].cpu().numpy() == want).all()
    assert (got["bid"].cpu().numpy() == want[:, 0]).all() and (got["flat"].cpu().numpy() == want[:, 1]).all()
    sr.check_sample(_mask_2x16x24(), 40, got["idx"].cpu().numpy())
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_miss_ray_window(cuda, poison, mode):
    import miss_window_ref as mw
    from implicit_depth_amd import query as Q
    from test_miss_window_gpu import _check

    def run(mask_np=None, n=60):
        mask_np = _mask_2x16x24(seed=7) if mask_np is None else mask_np
        bs, h, w = mask_np.shape
        return Q.sample_miss_window(torch.from_numpy(mask_np).to(cuda), *_intr(bs, h, w, cuda), n,
                                    state=Q.sampler_state(3, cuda, 1))

    big = (np.random.default_rng(9).random((3, 40, 56)) < 0.5).astype(np.uint8)
    base, got = drive(poison, mode, run, donor=lambda: run(big, 100))
    mask_np = _mask_2x16x24(seed=7)
    poison.begin("zeros")                         # (_check compares with get_miss_ray's rows: a clean call)
    _check(got, mask_np, torch.from_numpy(mask_np).to(cuda), _intr(2, 16, 24, cuda), 60,
           mw.select(mask_np, 60, seed=3, counter=1))
    same(got, base)


# ------------------------------------------------------------------------------------------------------------------
# Decoders
# ------------------------------------------------------------------------------------------------------------------
def _dev(p, dev, dt):
    return {k: v.to(dev, dt) for k, v in p.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_decoders_300_rows(cuda, poison, precision, mode):
    from implicit_depth_amd import decoders_forward
    d = 385
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 1, 5.0), 2)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 3, 5.0), 4)
    mp, mo = make_module("IMNET", pp, d, cuda), make_module("IEF", po, d, cuda)

    def run(n=300):
        x = torch.randn(n, d, generator=torch.Generator().manual_seed(5))
        with torch.no_grad():
            return decoders_forward(x.to(cuda), mp, mo, precision=precision)

    base, got = drive(poison, mode, run, donor=lambda: run(5000))
    x = torch.randn(300, d, generator=torch.Generator().manual_seed(5))
    assert (got[0].cpu() - orc.imnet_forward(pp, x)).abs().max().item() <= TOL
    assert (got[1].cpu() - orc.ief_forward(po, x, 2)).abs().max().item() <= TOL
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [17, 2049])
@pytest.mark.parametrize("gf", [32, 64, 128])
def test_decoder_chain(cuda, poison, monkeypatch, gf, n, mode):
    """lidf_decoder_chain_f32 as test_decoder_chain_matches_the_layers holds it: the layer-by-layer path's own
    distance from float64 is the yardstick."""
    import copy
    from implicit_depth_amd import IEF, generic
    inp = 385
    torch.manual_seed(gf + inp)
    mod = IEF("cpu", inp, 1, gf, n_iter=2)
    for p in mod.parameters():
        p.data.mul_(6.0)
    ref_mod = copy.deepcopy(mod).double()
    ref_mod.init_offset = ref_mod.init_offset.double()
    mod = mod.to(cuda).eval()
    mod.device, mod.init_offset = cuda, mod.init_offset.to(cuda)

    assert generic.chain_ok(mod)

    def run(rows=n):
        x = torch.randn(rows, inp, generator=torch.Generator().manual_seed(rows))
        with torch.no_grad():
            return generic.decoder_forward(mod, x.to(cuda))     # (the chain launch at every gf, 64 included)

    base, got = drive(poison, mode, run, donor=lambda: run(2049 if n == 17 else 40000))
    x = torch.randn(n, inp, generator=torch.Generator().manual_seed(n))
    with torch.no_grad():
        ref = ref_mod.forward_composite(x.double())
        poison.begin("zeros")
        monkeypatch.setenv("LIDF_CHAIN16", "0")
        layers = generic.decoder_forward(mod, x.to(cuda))
        monkeypatch.delenv("LIDF_CHAIN16")
    e_chain = float((got.double().cpu() - ref).abs().max())
    e_layers = float((layers.double().cpu() - ref).abs().max())
    assert e_chain <= max(1e-5, 1.5 * e_layers), (e_chain, e_layers)
    assert float((got - layers).abs().max()) <= 4e-5
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_decoder_training_320_rows(cuda, poison, mode):
    """Forward with kept activations + backward of one IEF (tests/test_f64_gpu.py::test_decoder_module_backward at
    320 rows: every weight gradient is one slice, the workspace's slab area is present)."""
    from test_f64_gpu import _masked_weights
    d = 385
    p = orc.randomize_biases(orc.init_decoder("IEF", d, 31, 5.0), 32)
    m = make_module("IEF", p, d, cuda).train()

    def case(n):
        gen = torch.Generator().manual_seed(n)
        x = torch.randn(n, d, generator=gen).to(cuda)
        return x, _masked_weights(p, x, "IEF", n, gen, cuda)

    def run(n=320):
        x, w = case(n)
        for q in m.parameters():
            q.grad = None
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        (y.reshape(-1) * w).sum().backward()
        out = {k: q.grad.clone() for k, q in m.named_parameters()}
        out.update(input=xg.grad, y=y.detach())
        return out

    base, got = drive(poison, mode, run, donor=lambda: run(5000))
    x, w = case(320)
    _, g64 = oracle_grads(p, x, "IEF", w, torch.float64)
    _, g32 = oracle_grads(p, x, "IEF", w, torch.float32)
    for k in g64:
        assert_f64_close("IEF n=320 d%s" % k, got[k], g64[k], g32[k], k=k_for(k))
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_decoder_pair_node_320_rows(cuda, poison, mode):
    """decoders_forward_train (tests/test_f64_gpu.py::test_decoder_pair_node_backward at 320 rows)."""
    from implicit_depth_amd import decoders_forward_train
    from test_f64_gpu import _check_decoder_out, _masked_weights
    d = 385
    pp = orc.randomize_biases(orc.init_decoder("IMNET", d, 21, 5.0), 22)
    po = orc.randomize_biases(orc.init_decoder("IEF", d, 23, 5.0), 24)
    prob, off = make_module("IMNET", pp, d, cuda).train(), make_module("IEF", po, d, cuda).train()

    def case(n):
        gen = torch.Generator().manual_seed(n + d)
        x = torch.randn(n, d, generator=gen).to(cuda)
        return x, _masked_weights(pp, x, "IMNET", n, gen, cuda), _masked_weights(po, x, "IEF", n, gen, cuda)

    def run(n=320):
        x, wp, wo = case(n)
        for q in list(prob.parameters()) + list(off.parameters()):
            q.grad = None
        xg = x.clone().requires_grad_(True)
        yp, yo = decoders_forward_train(xg, prob, off)
        ((yp.reshape(-1) * wp).sum() + (yo.reshape(-1) * wo).sum()).backward()
        out = {"prob." + k: q.grad.clone() for k, q in prob.named_parameters()}
        out.update({"off." + k: q.grad.clone() for k, q in off.named_parameters()})
        out.update(input=xg.grad, yp=yp.detach(), yo=yo.detach())
        return out

    base, got = drive(poison, mode, run, donor=lambda: run(5000))
    x, wp, wo = case(320)
    refs = {}
    for dt in (torch.float64, torch.float32):
        yp_r, gp = oracle_grads(pp, x, "IMNET", wp, dt)
        yo_r, go = oracle_grads(po, x, "IEF", wo, dt)
        g = {"prob." + k: v for k, v in gp.items() if k != "input"}
        g.update({"off." + k: v for k, v in go.items() if k != "input"})
        g["input"] = gp["input"] + go["input"]
        refs[dt] = (yp_r, yo_r, g)
    _check_decoder_out("pair prob", got["yp"], refs[torch.float64][0], refs[torch.float32][0], False)
    _check_decoder_out("pair off", got["yo"], refs[torch.float64][1], refs[torch.float32][1], False)
    for k in refs[torch.float64][2]:
        assert_f64_close("pair d%s" % k, got[k], refs[torch.float64][2][k], refs[torch.float32][2][k], k=k_for(k))
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_wgrad_with_workspace(cuda, poison, mode):
    """lidf_wgrad_f32 with its workspace at the decoders' layer-1 shape, 5,000 rows: the slab reduction (at 320 rows
    every block is one slice and the slabs are not used)."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    M, N = 256, 385

    def run(n=5000):
        g = torch.Generator().manual_seed(n)
        a, b = torch.randn(n, M, generator=g).to(cuda), torch.randn(n, N, generator=g).to(cuda)
        wsb = L.lidf_wgrad_workspace_bytes()
        ws = _lib.workspace(wsb, cuda)
        c, db = torch.zeros(M, N, device=cuda), torch.zeros(M, device=cuda)
        _lib.check(L.lidf_wgrad_f32(_lib.ptr(a), M, M, _lib.ptr(b), N, N, n, _lib.ptr(c), N, _lib.ptr(db),
                                    _lib.ptr(ws), wsb, _lib.current_stream(cuda)))
        torch.cuda.synchronize()
        return {"a": a, "b": b, "c": c, "db": db}

    base, got = drive(poison, mode, run, donor=lambda: run(160000))
    a, b = got["a"], got["b"]
    assert_f64_close("wgrad dW", got["c"], a.double().t() @ b.double(), a.t() @ b)
    assert_f64_close("wgrad db", got["db"], a.double().sum(0), a.sum(0), k=K_BIAS)
    same(got, base)


def test_wgrad_without_workspace_reference_only(cuda):
    """The column kernel's float atomics (lidf_hip.h: NOT bit-reproducible run to run): no workspace to poison, the
    reference bound alone."""
    from implicit_depth_amd import _lib
    L = _lib.lib()
    M, N, n = 256, 385, 5000
    with tf32_off():
        g = torch.Generator().manual_seed(n)
        a, b = torch.randn(n, M, generator=g).to(cuda), torch.randn(n, N, generator=g).to(cuda)
        c, db = torch.zeros(M, N, device=cuda), torch.zeros(M, device=cuda)
        _lib.check(L.lidf_wgrad_f32(_lib.ptr(a), M, M, _lib.ptr(b), N, N, n, _lib.ptr(c), N, _lib.ptr(db), None, 0,
                                    _lib.current_stream(cuda)))
        assert_f64_close("wgrad atomics dW", c, a.double().t() @ b.double(), a.t() @ b)
        assert_f64_close("wgrad atomics db", db, a.double().sum(0), a.sum(0), k=K_BIAS)


# ------------------------------------------------------------------------------------------------------------------
# Query
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_lidf_query(cuda, poison, precision, mode):
    scene, ref = _query_scene()

    def run(s=scene):
        out = run_query(s, cuda, precision=precision, want_rayfeat=True)
        return {k: out[k] for k in QUERY_KEYS}

    big = orc.synthetic_scene(2, 24, 32, 16, seed=99, ragged=True)
    base, got = drive(poison, mode, run, donor=lambda: run(big))
    _check_query(scene, ref, got)
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_lidf_query_generic_gf32(cuda, poison, mode):
    from implicit_depth_amd import IEF, IMNet, generic
    from implicit_depth_amd.query import lidf_query
    scene, ref = _query_scene_gf32()
    D = scene["D"]
    prob, off = IMNet(D, 1, 32), IEF(cuda, D, 1, 32, n_iter=2)
    prob.load_state_dict(scene["prob_p"]), off.load_state_dict(scene["off_p"])
    prob, off = prob.to(cuda).eval(), off.to(cuda).eval()
    assert generic.chain_ok(prob) and generic.chain_ok(off)

    def run(sc=scene):
        s = to_dev(sc, cuda)
        depth = torch.zeros((sc["B"], sc["h"], sc["w"]), device=cuda)
        with torch.no_grad():
            out = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                             s["pair_t"], s["feat_grid"], s["vox_feat"], prob, off, ray_flat=s["ray_flat"], depth=depth)
        out["depth"] = depth
        return {k: out[k] for k in QUERY_KEYS if k in out}

    big = dict(orc.synthetic_scene(2, 24, 32, 16, seed=99, ragged=True))
    base, got = drive(poison, mode, run, donor=lambda: run(big))
    _check_query(scene, ref, got)
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("factorised,offsets", [(True, "all"), (True, "selected"), (False, "all")])   # ('selected' is
def test_lidf_query_train(cuda, poison, factorised, offsets, mode):                                  # factorised only)
    from implicit_depth_amd.query import lidf_query_train
    sel = offsets == "selected"
    scene, w, ref, gref = _query_train_case(sel)
    D = scene["D"]
    kw = dict(offset_range=(-0.2, 0.2), part_size=0.25, pos_rel=True, factorised=factorised, offsets=offsets)

    def run(sc=scene, wts=w):
        s = to_dev(sc, cuda)
        prob = make_module("IMNET", sc["prob_p"], D, cuda).train()
        off = make_module("IEF", sc["off_p"], D, cuda).train()
        fgd = s["feat_grid"].clone().requires_grad_(True)
        vfd = s["vox_feat"].clone().requires_grad_(True)
        out = lidf_query_train(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                               s["pair_t"], fgd, vfd, prob, off, vox_center=s["vox_center"], **kw)
        _query_loss(out, {k: v.to(cuda) for k, v in wts.items()}, sel).backward()
        res = {k: out[k].detach() for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_pos", "max_pair_id")}
        res.update({"feat_grid": fgd.grad, "vox_feat": vfd.grad})
        res.update({"prob." + k: v.grad for k, v in prob.named_parameters()})
        res.update({"off." + k: v.grad for k, v in off.named_parameters()})
        return res

    def donor():
        big = orc.synthetic_scene(1, 24, 32, 16, seed=91, ragged=True)
        gen = torch.Generator().manual_seed(92)
        run(big, {"prob": torch.randn(big["P"], generator=gen), "off": torch.randn(big["P"], generator=gen),
                  "pos": torch.randn(big["R"], 3, generator=gen)})

    base, got = drive(poison, mode, run, donor=donor)
    mid = got["max_pair_id"].cpu()
    live = mid[mid < scene["P"]]
    for k in ("pred_prob_end", "pred_pos"):
        assert (got[k].cpu() - ref[k]).abs().max().item() <= TOL, k
    for k in ("pred_offset", "pair_pred_pos"):
        rows = live if sel else slice(None)
        assert (got[k].cpu()[rows] - ref[k][rows]).abs().max().item() <= TOL, k
    for k, g in gref.items():
        _close_rel(got[k].cpu(), g, k, 5e-4, 1e-2)
    # feat_grid: every RoI box of a 12 x 16 frame is clamped at the border — float atomics; held to
    # the reference above and to rounding here, everything else bit for bit
    a, b = got.pop("feat_grid"), base.pop("feat_grid")
    assert (a - b).abs().max().item() <= 16 * 2.0 ** -24 * b.abs().max().item()
    if not factorised:     # lidf_rows_backward_f32 (no workspace): "d vox_feat [V,128] (float atomics)", lidf_hip.h —
        got.pop("vox_feat"), base.pop("vox_feat")     # the reference bound above is what holds it
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_ray_features_backward_with_workspace(cuda, poison, mode):
    """lidf_ray_features_backward_f32 with its whole workspace (parked-gradient image + rays-per-pixel table) on rays
    whose boxes stay inside the image, one ray per pixel: stored, then gathered per pixel, no atomics — bit for
    bit. (Two rays of one pixel are added atomically and clamped boxes keep float atomics with the workspace too,
    DESIGN.md 5.9: test_lidf_query_train above holds those to the reference.)"""
    from implicit_depth_amd.query import _RayFeaturesFn

    def case(B, h, w, R):
        gen = torch.Generator().manual_seed(h * w)
        feat = torch.randn(B, 32, h, w, generator=gen)
        iw, ih = w - 16, h - 16                                   # pixels at least 8 from every border
        pick = torch.randperm(B * ih * iw, generator=gen)[:R]     # distinct (image, pixel)
        bid, rest = pick // (ih * iw), pick % (ih * iw)
        pix = torch.stack((8 + rest % iw, 8 + rest // iw), 1).int()
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=1)
        return feat, pix, bid.int(), d, torch.randn(R, 128, generator=gen)

    # (40 x 56 and 60 x 88: the last 16-pixel tile row / column is at least half a box wide, so the rays-per-pixel
    # table is used — lidf_launch_rayfeat_backward)
    def run(B=2, h=40, w=56, R=900):
        feat, pix, bid, d, wgt = case(B, h, w, R)
        fgd = feat.to(cuda).requires_grad_(True)
        got = _RayFeaturesFn.apply(fgd, d.to(cuda), pix.to(cuda), bid.to(cuda), 8, 4)
        (got[:, :128] * wgt.to(cuda)).sum().backward()
        return fgd.grad

    base, got = drive(poison, mode, run, donor=lambda: run(3, 60, 88, 4000))
    feat, pix, bid, d, wgt = case(2, 40, 56, 900)
    fg = feat.clone().requires_grad_(True)
    boxes = orc.roi_boxes(pix.long(), bid.long(), 40, 56, 8)
    (orc.roi_align_fast(fg, boxes).reshape(900, -1) * wgt).sum().backward()
    assert (got.cpu() - fg.grad).abs().max().item() <= 1e-5 * max(1.0, fg.grad.abs().max().item())
    same(got, base)


def test_ray_features_backward_without_workspace_reference_only(cuda):
    """workspace NULL: every ray adds its samples' shares with float atomics (lidf_hip.h) — the reference alone."""
    from implicit_depth_amd import _lib
    scene = orc.synthetic_scene(2, 12, 16, 1, seed=73)
    s = to_dev(scene, cuda)
    R = scene["R"]
    wgt = torch.randn(R, 128, generator=torch.Generator().manual_seed(74))
    fg = scene["feat_grid"].clone().requires_grad_(True)
    boxes = orc.roi_boxes(scene["ray_pix"].long(), scene["ray_bid"].long(), 12, 16, 8)
    (orc.roi_align_fast(fg, boxes).reshape(R, -1) * wgt).sum().backward()
    g = torch.zeros((R, 128 + 27), device=cuda)
    g[:, :128] = wgt.to(cuda)
    d_feat = torch.empty((2, 32, 12, 16), device=cuda)
    _lib.check(_lib.lib().lidf_ray_features_backward_f32(
        _lib.ptr(g), _lib.ptr(s["ray_pix"]), _lib.ptr(s["ray_bid"]), R, 2, 12, 16, 8, 4, _lib.ptr(d_feat), None, 0,
        _lib.current_stream(cuda)))
    assert (d_feat.cpu() - fg.grad).abs().max().item() <= 1e-5 * max(1.0, fg.grad.abs().max().item())


# ------------------------------------------------------------------------------------------------------------------
# PointNet
# ------------------------------------------------------------------------------------------------------------------
# (3000, 40): the LDS table; (2000, 300): sorted walk with a 32-row window, V > 288; (600, 16385): the global-atomic
# tables beyond 16,384 voxels
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,v,donor", [(3000, 40, (5000, 60)), (2000, 300, (9000, 400)), (600, 16385, (1500, 17000))])
def test_pointnet_inference(cuda, poison, n, v, donor, mode):
    p = _pointnet_case(n, v)[0]
    m = make_pointnet(p, cuda)

    def run(n=n, v=v):
        g = torch.Generator().manual_seed(n + v)
        inp = torch.randn(n, 6, generator=g)
        vox = torch.randint(0, v, (n,), generator=g)
        with torch.no_grad():
            return m(inp.to(cuda), vox.to(cuda), n_vox=v)

    base, got = drive(poison, mode, run, donor=lambda: run(*donor))
    ref = _pointnet_case(n, v)[3]
    assert got.shape == ref.shape and (got.cpu() - ref).abs().max().item() <= 2e-5
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,v,donor", [(3000, 40, (5000, 60)), (2000, 300, (9000, 400))])
def test_pointnet_training(cuda, poison, n, v, donor, mode):
    """tests/test_train_gpu.py::test_pointnet_gradients' reference and bounds."""
    p = orc.init_pointnet(7, 1.5)

    def run(n=n, v=v):
        g = torch.Generator().manual_seed(n + v)
        inp = torch.randn(n, 6, generator=g)
        vox = torch.randint(0, v, (n,), generator=g)
        wgt = torch.randn(v, 128, generator=g)
        m = make_pointnet(p, cuda).train()
        xd = inp.to(cuda).requires_grad_(True)
        out = m(xd, vox.to(cuda), n_vox=v)
        (out * wgt.to(cuda)).sum().backward()
        res = {k: q.grad for k, q in m.named_parameters()}
        res.update(inp=xd.grad, out=out.detach())
        return res

    base, got = drive(poison, mode, run, donor=lambda: run(*donor))
    _, _, _, _, ref, grads = _pointnet_train_case(n, v)
    assert (got["out"].cpu() - ref).abs().max().item() <= 2e-5
    for k, g in grads.items():
        _close_rel(got[k].cpu(), g, k, 5e-4, 1e-2)
    same(got, base)


# ------------------------------------------------------------------------------------------------------------------
# Stage 2
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cell_table", [False, True])
def test_lidf_refine_two_iterations(cuda, poison, cell_table, mode):
    from implicit_depth_amd.query import lidf_query, lidf_refine
    from implicit_depth_amd.synthetic import GRID_RES, GRID_XMIN, PART_SIZE
    scene, vb, vbid, rgb, valid_inp, valid_vox, pnet_p, offr_p = _refine_case()
    s = to_dev(scene, cuda)
    D = scene["D"]
    prob, off = make_module("IMNET", scene["prob_p"], D, cuda), make_module("IEF", scene["off_p"], D, cuda)
    pnet, offr = make_pointnet(pnet_p, cuda), make_module("IEF", offr_p, 334, cuda)
    poison.begin("zeros")
    with torch.no_grad():
        s1 = lidf_query(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["pair_off"], s["pair_ray"], s["pair_vox"],
                        s["pair_t"], s["feat_grid"], s["vox_feat"], prob, off)
    ci = torch.arange(GRID_RES)
    coord = torch.stack(torch.meshgrid(ci, ci, ci, indexing="ij"), -1).reshape(-1, 3).repeat(2, 1).int().contiguous()
    grid = {"xmin": torch.tensor(GRID_XMIN), "grid_dims": (GRID_RES,) * 3, "part_size": PART_SIZE,
            "voxel_coord": coord.to(cuda)} if cell_table else None

    def run(extra=0):
        vi, vv = valid_inp, valid_vox
        if extra:          # (the donor: more valid points through the same voxels)
            g = torch.Generator().manual_seed(extra)
            vi = torch.randn(500 + extra, 6, generator=g) * 0.2
            vv = torch.randint(0, scene["V"], (500 + extra,), generator=g).int()
        with torch.no_grad():
            return lidf_refine(s["ray_dir"], s["ray_pix"], s["ray_bid"], s["ray_flat"], s1["pred_pos"],
                               s1["max_pair_id"], s["pair_vox"], vb.to(cuda), vbid.to(cuda), rgb.to(cuda),
                               s["feat_grid"], vi.to(cuda), vv.to(cuda), pnet, offr, forward_times=2, grid=grid)

    base, got = drive(poison, mode, run, donor=lambda: run(3000))
    pos, ev = _refine_oracle(s1["pred_pos"].cpu(), s1["max_pair_id"].cpu())
    assert (got[0].cpu() - pos).abs().max().item() <= TOL
    assert (got[1].cpu().long() == ev).all()
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_lidf_refine_train(cuda, poison, mode):
    """tests/test_train_gpu.py::test_refine_train_fused_step_vs_composed's scene (cell table on): the fused step,
    forward and backward, against the step composed from the modules' own autograd functions."""
    from implicit_depth_amd.query import _lidf_refine_train_composed, lidf_refine_train
    poison.begin("zeros")
    sc = refine_train_scene(cuda)
    occ, vb, vbid, V, bid, pos0, ray_dir, flat, ray_pix, pair_vox, mid, rgb, feat, valid_inp, valid_vox = (
        sc[k] for k in ("occ", "vb", "vbid", "V", "bid", "pos0", "ray_dir", "flat", "ray_pix", "pair_vox", "mid", "rgb",
                        "feat", "valid_inp", "valid_vox"))
    wgt, pnet_p, dec_p = sc["wgt"].to(cuda), sc["pnet_p"], sc["dec_p"]

    def step(fn, n_valid=500, **kw):
        pnet, dec = make_pointnet(pnet_p, cuda).train(), make_module("IEF", dec_p, 334, cuda).train()
        pp = pos0.to(cuda).requires_grad_(True)
        fg = feat.to(cuda).requires_grad_(True)
        vi, vv = valid_inp, valid_vox
        if n_valid != 500:
            gg = torch.Generator().manual_seed(n_valid)
            vi = torch.randn(n_valid, 6, generator=gg) * 0.2
            vv = torch.randint(0, V, (n_valid,), generator=gg).int()
        got, ev = fn(ray_dir.to(cuda), ray_pix.to(cuda), bid.int().to(cuda), flat.int().to(cuda), pp, mid.to(cuda),
                     pair_vox.to(cuda), vb, vbid, rgb.to(cuda), fg, vi.to(cuda), vv.to(cuda), pnet, dec,
                     forward_times=3, pos_rel=True, pnet_pos_rel=False, perturb_noise=0.03, **kw)
        (got * wgt).sum().backward()
        res = {"pos": got.detach(), "ev": ev, "pred_pos": pp.grad, "feat_grid": fg.grad}
        res.update({"pnet." + k: q.grad for k, q in pnet.named_parameters()})
        res.update({"dec." + k: q.grad for k, q in dec.named_parameters()})
        return res

    ref = step(_lidf_refine_train_composed)
    torch.cuda.synchronize()
    base, got = drive(poison, mode, lambda: step(lidf_refine_train, grid=occ),
                      donor=lambda: step(lidf_refine_train, n_valid=4000, grid=occ))
    assert torch.equal(got["ev"], ref["ev"])
    assert (got["pos"] - ref["pos"]).abs().max().item() <= TOL
    for k, gr in ref.items():
        if k not in ("pos", "ev"):
            err = (got[k] - gr).abs().max().item()
            assert err <= 1e-3 * max(gr.abs().max().item(), 1e-3), (k, err, gr.abs().max().item())
    # feat_grid's border taps are float atomics: the existing test's two-run bound; the rest bit for bit
    a, b = got.pop("feat_grid"), base.pop("feat_grid")
    assert (a - b).abs().max().item() <= 1e-5 * max(b.abs().max().item(), 1e-3)
    same(got, base)


# ------------------------------------------------------------------------------------------------------------------
# Losses
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_stage1_training_step(cuda, poison, mode):
    """pipeline.lidf_forward_train on the g9 fixture (test_train_step_gpu::test_whole_step_against_the_reference)."""
    import train_loss_ref as tl
    from test_train_step_gpu import _close, _g9_step, _synthetic_step, _zero_bias_bound
    g, gp = tl.g9_files()
    name = "e0"
    d, ref = tl.g9_case(g, name)
    keep = {}

    def run():
        dd, loss, feat, mods = _g9_step(g, name, cuda)
        keep.update(dd=dd, loss=loss, feat=feat, mods=mods)
        return _step_result(dd, loss, feat, mods, ("pred_pos", "pred_prob_end", "miss_bid", "miss_flat_img_id"))

    def donor():           # (a larger frame batch through the same step)
        _synthetic_step(2, 48, 64, 1.0, cuda)[2]["loss_net"].backward()

    base, got = drive(poison, mode, run, donor=donor)
    dd, loss, feat, mods = keep["dd"], keep["loss"], keep["feat"], keep["mods"]
    assert torch.equal(dd["miss_bid"].cpu(), d["miss_bid"]) and torch.equal(dd["miss_flat_img_id"].cpu(), d["miss_flat"])
    bad = []
    for i, k in enumerate(tl.LOSS_KEYS):
        _close(loss[k].detach().cpu(), ref["loss"][i], (name, k), bad)
    _close(feat.grad.cpu(), ref["g_full_rgb_feat"], (name, "full_rgb_feat"), bad)
    stride = int(g["param_stride"])
    for mod, m in zip(("pnet_model", "prob_dec", "offset_dec"), mods):
        for k, p in m.named_parameters():
            want = torch.from_numpy(gp["%s_g_%s.%s" % (name, mod, k)])
            have = p.grad.detach().cpu().reshape(-1)
            have = have[::stride] if have.numel() > 4096 else have
            if (mod, k) == ("prob_dec", "linear_4.bias"):
                assert abs(float(have)) <= _zero_bias_bound(d["pair_ray"].shape[0])
                continue
            _close(have, want, (name, mod, k), bad)
    assert not bad, bad
    # full_rgb_feat: on this 16 x 24 frame every RoI box is clamped — the same sum in another order (DESIGN.md 5.9,
    # test_whole_step_is_bit_identical_and_trains' bound); everything else bit for bit
    a, b = got.pop("full_rgb_feat"), base.pop("full_rgb_feat")
    assert (a - b).abs().max().item() <= 16 * 2.0 ** -24 * b.abs().max().item()
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_refine_training_step(cuda, poison, mode):
    """pipeline.train_refine_step on the g10 fixture (test_refine_train_step_gpu::test_whole_step_against_the_reference)."""
    import refine_loss_ref as rl
    from test_refine_train_step_gpu import _check_step, _g10_step
    g, gp = rl.g10_files()
    name = "plain"
    d, ref = rl.g10_case(g, name)
    keep = {}

    def run():
        dd, loss1, loss, feat, mods, mods_r = _g10_step(g, name, cuda)
        keep.update(dd=dd, loss=loss, mods_r=mods_r)
        res = _step_result(dd, loss, None, mods_r, ("pred_pos", "pred_pos_refine", "end_voxel_id"))
        res.update({"loss1." + k: v.detach() for k, v in loss1.items()})
        return res

    base, got = drive(poison, mode, run)
    assert (keep["dd"]["pred_pos"].cpu() - d["pred_pos"]).abs().max().item() <= TOL
    _check_step(g, gp, name, keep["dd"], keep["loss"], keep["mods_r"], ref, d)
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_stage1_loss_with_device_select(cuda, poison, mode):
    """lidf_loss forward + backward with hard-negative mining on the device: the loss kernels' and the select
    kernel's workspaces (test_hard_neg_gpu::test_lidf_loss_device_route_on_the_fixture)."""
    import train_loss_ref as tl
    from implicit_depth_amd import LidfLossOptions, lidf_loss
    from implicit_depth_amd.losses import compute_gt
    from test_hard_neg_gpu import _stage1_dd
    g, _ = tl.g9_files()
    name = "e0_hn"
    d, ref = tl.g9_case(g, name)
    epoch, opt = tl.g9_opt(name)
    order = {}

    def run():
        dd, order["o"] = _stage1_dd(d, cuda)
        compute_gt(dd)
        out = lidf_loss(dd, LidfLossOptions(hard_neg_select="device", **opt), "train", epoch)
        out["loss_net"].backward()
        res = {k: v.detach() for k, v in out.items()}
        res.update(g_pred_pos=dd["pred_pos"].grad, g_logit=dd["pred_prob_end"].grad)
        return res

    base, got = drive(poison, mode, run)
    loss64, gp64, gl64 = tl.loss_and_grads(d, torch.float64, epoch, **opt)
    inv = torch.empty_like(order["o"])
    inv[order["o"]] = torch.arange(inv.shape[0])
    for i, k in enumerate(tl.LOSS_KEYS):
        assert_f64_close("g9 %s %s" % (name, k), got[k].cpu().reshape(1), loss64[i].reshape(1), ref["loss"][i].reshape(1))
    assert_f64_close("g9 g_pred_pos", got["g_pred_pos"].cpu(), gp64, ref["g_pred_pos"])
    assert_f64_close("g9 g_pred_prob_end", got["g_logit"].cpu()[inv], gl64, ref["g_pred_prob_end"])
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_refine_loss_with_device_select(cuda, poison, mode):
    import refine_loss_ref as rl
    from implicit_depth_amd import LidfLossOptions, refine_loss
    from test_hard_neg_gpu import _refine_dd
    g, _ = rl.g10_files()
    d, ref = rl.g10_case(g, "hn")
    epoch, opt = int(g["epoch"]), rl.G10_CASES["hn"]

    def run():
        dd = _refine_dd(d, cuda)
        out = refine_loss(dd, LidfLossOptions(hard_neg_select="device", **opt), "train", epoch)
        out["loss_net"].backward()
        res = {k: v.detach() for k, v in out.items()}
        res["g_pred_pos_refine"] = dd["pred_pos_refine"].grad
        return res

    def donor():
        big = _refine_dd(rl.random_case(600, bs=3), cuda)
        refine_loss(big, LidfLossOptions(hard_neg_select="device", hard_neg=True, hard_neg_ratio=0.1, smooth_w=0.5),
                    "train", 0)["loss_net"].backward()

    base, got = drive(poison, mode, run, donor=donor)
    loss64, gp64 = rl.loss_and_grad(d, torch.float64, epoch, 1.0, **opt)
    for i, k in enumerate(rl.REFINE_LOSS_KEYS):
        assert_f64_close("g10 hn %s" % k, got[k].cpu().reshape(1), loss64[i].reshape(1), ref["loss"][i].reshape(1))
    assert_f64_close("g10 hn g_pred_pos_refine", got["g_pred_pos_refine"].cpu(), gp64, ref["g_pred_pos_refine"])
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["3x20x27", "1x20x27", "g12c_hard_neg"])
@pytest.mark.parametrize("stage", (1, 2))
def test_eval_losses(cuda, poison, stage, case, mode):
    """The evaluation-flavour losses (tests/test_eval_loss_gpu.py: several ragged blocks, the one-frame resize
    branch with the depth statistics, and the fixture case with hard-negative mining on the device)."""
    import eval_loss_ref as el
    from test_eval_loss_gpu import _check, _opt, _product_dd, _run
    ref32 = None
    if case == "g12c_hard_neg":
        g = el.g12_file()
        d, ref = el.g12_case(g, "c")
        opt, exp = dict(_opt(g, "c")), el.G12_CASES["c"][0]
        ref32 = ref["loss"] if stage == 1 else ref["loss_refine"]
        run_opt = dict(opt, hard_neg_select="device")
    else:
        d3 = el.random_case(3, 20, 27, 0.6, seed=5)
        d, exp = d3, "valid"
        if case == "1x20x27":
            R0 = int((d3["miss_bid"] == 0).sum())
            pk = d3["pair_ray"] < R0
            d = dict(d3, bs=1, pair_ray=d3["pair_ray"][pk], pred_prob_end=d3["pred_prob_end"][pk], pcl_label=d3["pcl_label"][pk])
            for k in ("xyz_flat", "xyz_corrupt_flat", "corrupt_mask"):
                d[k] = d3[k][:1].contiguous()
            for k in ("miss_bid", "miss_flat", "gt_pos", "pred_pos", "pred_pos_refine"):
                d[k] = d3[k][:R0].contiguous()
            exp = "test"
        opt = run_opt = dict(smooth_w=0.5)
    base, got = drive(poison, mode, lambda: _run(_product_dd(d, cuda), stage, exp, **run_opt),
                      donor=lambda: _run(_product_dd(el.random_case(4, 40, 54, 0.6, seed=6), cuda), stage, exp, **run_opt))
    _check(case, got, d, stage, ref32, **opt)
    same(got, base)


@pytest.mark.parametrize("mode", MODES)
def test_topk_mean_five_jobs(cuda, poison, mode):
    """lidf_topk_mean_f32, five jobs in one call (tests/test_hard_neg_gpu.py::test_five_jobs_in_one_call): the
    histograms, states, partial sums and tie tables all live in the workspace."""
    from test_hard_neg_gpu import _check, _pattern, _raw_jobs
    ns = [1, 257, 4097, 10000, 65]
    pats = ["uniform", "five_values", "last_digit", "uniform", "signed_zeros"]
    ratio = 0.3

    def values(scale=1):
        vals = [_pattern(p, n * scale) for p, n in zip(pats, ns)]
        vals[3][np.random.default_rng(5).random(ns[3] * scale) < 0.8] = -np.inf
        return vals, [None, None, None, int(np.isfinite(vals[3]).sum()), None]

    def run(scale=1):
        vals, counts = values(scale)
        dv = [torch.from_numpy(v).to(cuda) for v in vals]
        dc = [None if c is None else torch.tensor([c], dtype=torch.int32, device=cuda) for c in counts]
        dw = [torch.full((v.shape[0],), 5.0, device=cuda) for v in vals]
        means = _raw_jobs(cuda, list(zip(dv, dc, dw)), ratio)
        return {"means": means, "weights": dw}

    base, got = drive(poison, mode, run, donor=lambda: run(7))
    vals, counts = values()
    for i in range(5):
        _check(got["means"][i], got["weights"][i], vals[i], ratio, counts[i], what="job %d" % i)
    same(got, base)


# ------------------------------------------------------------------------------------------------------------------
# Metrics: the opposite contract — zero-filled once by the caller, left zero by every call
# ------------------------------------------------------------------------------------------------------------------
def test_depth_metrics_leaves_its_workspace_zero(cuda, monkeypatch):
    from implicit_depth_amd import query as Q
    from test_metrics_gpu import _maps
    h, w = 37, 53
    a, b = _maps(h, w, seed=h + w), _maps(h, w, seed=7)

    def call(m):
        return Q.depth_metrics(m[0].to(cuda), m[1].to(cuda), m[2].to(cuda), None)

    def fresh(m):
        monkeypatch.setattr(Q, "_METRICS_WS", {})
        return call(m)

    ref_a, ref_b = fresh(a), fresh(b)
    monkeypatch.setattr(Q, "_METRICS_WS", {})
    got_a = call(a)
    (ws,) = Q._METRICS_WS.values()
    torch.cuda.synchronize()
    assert not bool(ws.any()), "lidf_depth_metrics_f32 left %d non-zero workspace bytes" % int((ws != 0).sum())
    got_b = call(b)                                   # a different map through the same workspace
    torch.cuda.synchronize()
    assert list(Q._METRICS_WS.values())[0] is ws and not bool(ws.any())
    same(got_a, ref_a)
    same(got_b, ref_b)
    for got, m in ((got_a, a), (got_b, b)):
        ref = orc.depth_metrics(m[0], m[1], m[2], None)
        assert float(got["count"]) == float(ref["count"])
        for k in Q.METRIC_NAMES:
            r, v = float(ref[k]), float(got[k])
            assert abs(v - r) <= 2e-6 * max(1.0, abs(r)), (k, v, r)


# ------------------------------------------------------------------------------------------------------------------
# Frame: the runner's persistent workspace and buffers poisoned between two batches
# ------------------------------------------------------------------------------------------------------------------
PER_RAY = ("ray_bid", "ray_flat", "ray_pix", "ray_dir", "max_pair_id", "pred_pos", "rayfeat", "pred_pos_refine",
           "end_voxel_id")
PER_PAIR = ("pair_ray", "pair_vox", "pair_t", "pred_offset", "pred_prob", "pred_prob_softmax", "pair_pred_pos")


@pytest.mark.parametrize("graph", [False, True])
def test_frame_runner(cuda, poison, graph):
    """(2, 48, 64) of test_frame_equals_stepwise_path. Batch A, then batch B through the same runner with
    runner.ws and every runner.buf tensor poisoned in between (ones, high, random); then A (more valid points, more
    pairs) followed by B with nothing poisoned, so that B meets A's
    finished tickets, status words and tails. B's outputs equal a fresh runner's up to the device-side counts, rows
    beyond the counts keep the poison, and the fresh runner equals the stepwise path."""
    from implicit_depth_amd import pipeline as pl
    from implicit_depth_amd.synthetic import synthetic_batch
    from test_frame_gpu import _compare, _dev, _models, _stepwise
    B, h, w = 2, 48, 64
    models = _models(cuda)
    opt = pl.LidfOptions(valid_stride=None, refine_use_all_pix=False)
    batch_a, feat_a = synthetic_batch(B, h, w, seed=77)
    batch_b, feat_b = synthetic_batch(B, h, w, seed=78, hole_frac=1.9)
    batch_a, feat_a, batch_b, feat_b = _dev(batch_a, cuda), feat_a.to(cuda), _dev(batch_b, cuda), feat_b.to(cuda)

    def new_runner(batch, feat):
        r = pl.FrameRunner(B, h, w, cuda, models[0], models[1], models[2], opt, models[3], models[4])
        with torch.no_grad():
            r.load(batch, feat)
            if graph:
                r.capture()
            r.run()
        torch.cuda.synchronize()
        return r

    poison.begin("zeros")
    fresh = new_runner(batch_b, feat_b)
    ok, ref = fresh.result()
    ok_s, step = _stepwise(batch_b, feat_b, models, opt)
    assert ok and ok_s
    _compare(ref, step)
    cb = ref["counts"]

    runner = new_runner(batch_a, feat_a)
    ca = runner.counts()
    assert ca["NV"] > cb["NV"] and ca["P"] > cb["P"] and ca["V"] >= cb["V"], (ca, cb)   # A is the larger problem
    gen = torch.Generator().manual_seed(4864)
    for mode in ("ones", "high", "random"):
        torch.cuda.synchronize()
        ws_poison.poison_tensor(runner.ws, mode, gen=gen)
        for t in runner.buf.values():
            ws_poison.poison_tensor(t, mode, gen=gen)
        # (pack_blob and its guard are persistent state of another kind — the packed weights with the fingerprint
        # they were built from; invalidate() re-validates the fingerprint, not the blob's bytes — and stay as they are)
        before = {k: runner.buf[k].clone() for k in PER_RAY + PER_PAIR}
        with torch.no_grad():
            runner.run(batch_b, feat_b)
        torch.cuda.synchronize()
        ok2, dd = runner.result()
        assert ok2 and dd["counts"] == cb, (mode, dd["counts"], cb)
        _compare(dd, ref)
        for keys, n in ((PER_RAY, cb["R"]), (PER_PAIR, cb["P"])):
            for k in keys:
                same(runner.buf[k][n:], before[k][n:], "%s rows beyond the count (%s poison)" % (k, mode))

    # A, then B, nothing poisoned in between
    runner2 = new_runner(batch_a, feat_a)
    with torch.no_grad():
        runner2.run(batch_b, feat_b)
    torch.cuda.synchronize()
    ok3, dd3 = runner2.result()
    assert ok3 and dd3["counts"] == cb
    _compare(dd3, ref)
