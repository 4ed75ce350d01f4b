"""GPU: every entry point held to its caller's stream — late inputs, slow side.

Every other GPU test enqueues on the default stream and synchronises the whole device (the exceptions: FrameRunner /
FramePipeline in test_frame_gpu.py, two graph captures). tests/stream_order.py describes what passes unseen under that
regime and the two stress modes that show it; this file drives the inventory of tests/test_workspace_gpu.py through
them, on that file's scenes (tests/entry_cases.py). Per case:
  * the default-stream run is held to the reference of the entry's existing test, with that test's bound;
  * an un-delayed run on a fresh stream and the stressed run on another are bit-equal to it — except the results the
    documents name as not bit-reproducible (lidf_wgrad_f32 / lidf_ray_features_backward_f32 without workspace are not
    part of this inventory; feat_grid's gradient at clamped boxes; lidf_rows_backward_f32's d vox_feat), which keep
    the run-to-run bounds test_workspace_gpu.py states;
  * the delay was still running when the enqueue returned to the host — except for the entries below.

Entries that read a size back make the host wait for their stream inside the call, so the "delay still running"
assertion cannot hold for them and is skipped (their late inputs still arrive behind the delay on `s`, and every
launch before the read still has to be on `s` to see them): READS_BACK below names each with the call site of its read.

Stream departures of the library, where each forks and joins, and the case that covers it:

  frame aux stream (FrameRunner.side[0], LidfFrameArgs.aux_stream)
      fork   lidf_frame_f32 records ev_fork on the caller's stream (start of the frame, rays exist, layer-1 launch
             done); the aux stream waits for it
      join   ev_join recorded on the aux stream (guard done, per-ray features done, stage-2 table done), awaited by the
             caller's stream before the first consumer; on every error exit
      case   frame_runner_side: late inputs and slow side
  training side stream, forward (query._train_side_stream)
      fork   lidf_query_train: side.wait_stream(caller) before lidf_pe_rows_f32
      join   caller.wait_stream(side) before _QueryTrainFn.apply reads pe
      case   query_train_factorised_all / _selected: late inputs and slow side; test_two_callers_share_...
  training side stream, backward
      fork   _QueryTrainFn.backward: side.wait_stream(caller) once the structs, ws2, d_vox2 and d_ray2 exist
      join   caller.wait_stream(side) before d_vox += d_vox2 and d_ray += d_ray2
      case   the same cases (backward() runs under the same stream); test_one_training_stream_equals_two
  pack cache (_lib.packed_entry)
      fork   none: one blob and guard per (module, stream), touched by launches of that stream only
      join   none needed
      case   test_per_stream_weight_entries_follow_an_update_across_streams, test_eviction_of_per_stream_weight_entries

Calibration and delays, measured on one MI355X: torch.cuda._sleep runs 2,385,000 cycles per millisecond (two
calibrations in one process: 2,385,082 and 2,387,168). The delay is max(20 ms, 3 x the host time of one enqueue on a
fresh stream); every case's enqueue took under 6.7 ms, so EVERY case — late inputs, slow side, LIDF_TRAIN_STREAMS=1,
two callers — ran with the 20.0 ms floor, a twelfth of the 250 ms cap. Host milliseconds of one enqueue (the largest;
entries that read a size back include their wait for the device): get_occ_vox_bound 6.0, exclusive_scan_32769 5.8
(its first three-launch call on a stream), stage1_training_step 3.3, refine_training_step 2.5, the three
query_train cases 1.5-1.7, decoder_training / decoder_pair_node 1.2-1.5, lidf_query_generic_gf32 and
decoder_chain_gf32 0.9, the PointNet training cases 0.8, lidf_refine_voxel_list 0.7, everything else 0.05-0.65
(frame_runner_captured 0.16, depth_metrics 0.05). The tests print the figures of their own run.

What the controls showed: all three fail the comparison, as asserted — work under another pool stream and a read on
the null stream see the NaN decoy (torch's pool streams are non-blocking streams: the null stream does not wait for
them, so null-stream launches are visible on this runtime), a fork without its join leaves the zero fill in the clone.
The second of them did NOT trip in one early run: its two streams had landed on one hardware queue, which runs them
in submission order. stream_order.fresh_stream() therefore picks the caller's stream with a bounded probe so that it
shares no hardware queue with the null stream or the entry's side stream; since then the controls trip in every run.
No library entry failed any case.
"""
import pytest
import torch

import entry_cases as ec
import stream_order as so
from util import assert_f64_close, check_selection, inv_out_act, tf32_off

pytestmark = pytest.mark.gpu

# name -> the call site of the host read (query.py unless another file is named)
READS_BACK = {
    "get_occ_vox_bound": "get_occ_vox_bound: counts.tolist() (V, Nv)",
    "ray_aabb_voxel_list": "compute_ray_aabb: pair_off[-1].item() (P)",
    "ray_aabb_grid_walk": "compute_ray_aabb: pair_off[-1].item() (P)",
    "get_miss_ray": "_compact_mask: cnt.item() (R)",
    "sample_miss_window": "sample_miss_window: buf.pop('n_rays').tolist() (R_out, T), its one read",
    "stage1_training_step": "pipeline._train_geometry: the reads of _compact_mask, get_occ_vox_bound, compute_ray_aabb",
    "refine_training_step": "pipeline._train_geometry: the reads of _compact_mask, get_occ_vox_bound, compute_ray_aabb",
}

CASES = {
    # geometry and samplers
    "exclusive_scan_32769": lambda d: ec.entry_exclusive_scan(d),
    "get_occ_vox_bound": lambda d: ec.entry_get_occ_vox_bound(d),
    "ray_aabb_voxel_list": lambda d: ec.entry_ray_aabb_voxel_list(d),
    "ray_aabb_grid_walk": lambda d: ec.entry_ray_aabb_grid_walk(d),
    "pcl_aabb": lambda d: ec.entry_pcl_aabb(d),
    "get_miss_ray": lambda d: ec.entry_get_miss_ray(d),
    "sample_valid_points": lambda d: ec.entry_sample_valid_points(d),
    "sample_miss_window": lambda d: ec.entry_sample_miss_window(d),
    # inference
    "embed_forward": lambda d: ec.entry_embed(d),
    "decoders_300_rows_f32": lambda d: ec.entry_decoders_300_rows(d, "f32"),
    "decoders_300_rows_f16x3": lambda d: ec.entry_decoders_300_rows(d, "f16x3"),
    "decoder_chain_gf32": lambda d: ec.entry_decoder_chain(d, 32),
    "decoder_chain_gf64": lambda d: ec.entry_decoder_chain(d, 64),
    "decoder_chain_gf128": lambda d: ec.entry_decoder_chain(d, 128),
    "lidf_query_f32": lambda d: ec.entry_lidf_query(d, "f32"),
    "lidf_query_f16x3": lambda d: ec.entry_lidf_query(d, "f16x3"),
    "lidf_query_generic_gf32": lambda d: ec.entry_lidf_query_generic_gf32(d),
    "lidf_query_shim": lambda d: ec.entry_lidf_query_shim(d),
    "pointnet_inference_3000_40": lambda d: ec.entry_pointnet_inference(d, 3000, 40),
    "pointnet_inference_2000_300": lambda d: ec.entry_pointnet_inference(d, 2000, 300),
    "lidf_refine_voxel_list": lambda d: ec.entry_lidf_refine(d, False),
    "lidf_refine_cell_table": lambda d: ec.entry_lidf_refine(d, True),
    "depth_metrics": lambda d: ec.entry_depth_metrics(d),
    "frame_runner_one_stream": lambda d: ec.entry_frame_runner(d, False, False),
    "frame_runner_side": lambda d: ec.entry_frame_runner(d, True, False),
    "frame_runner_captured": lambda d: ec.entry_frame_runner(d, None, True),
    # training
    "embed_backward": lambda d: ec.entry_embed_backward(d),
    "decoder_training_320_rows": lambda d: ec.entry_decoder_training_320_rows(d),
    "decoder_pair_node_320_rows": lambda d: ec.entry_decoder_pair_node_320_rows(d),
    "query_train_factorised_all": lambda d: ec.entry_lidf_query_train(d, True, "all"),
    "query_train_factorised_selected": lambda d: ec.entry_lidf_query_train(d, True, "selected"),
    "query_train_rows_all": lambda d: ec.entry_lidf_query_train(d, False, "all"),
    "pointnet_training_3000_40": lambda d: ec.entry_pointnet_training(d, 3000, 40),
    "pointnet_training_2000_300": lambda d: ec.entry_pointnet_training(d, 2000, 300),
    "eval_loss_stage1_3x20x27": lambda d: ec.entry_eval_loss(d, 1),
    "eval_loss_stage2_3x20x27": lambda d: ec.entry_eval_loss(d, 2),
    "topk_mean_five_jobs": lambda d: ec.entry_topk_mean_five_jobs(d),
    "lidf_refine_train": lambda d: ec.entry_lidf_refine_train(d),
    "stage1_training_step": lambda d: ec.entry_stage1_training_step(d),
    "refine_training_step": lambda d: ec.entry_refine_training_step(d),
    "stage1_loss_device_select": lambda d: ec.entry_stage1_loss_device_select(d),
    "refine_loss_device_select": lambda d: ec.entry_refine_loss_device_select(d),
}
SLOW_SIDE = ("query_train_factorised_all", "query_train_factorised_selected", "frame_runner_side")


@pytest.fixture
def rec(monkeypatch):
    with tf32_off():
        yield so.Recorder().install(monkeypatch)


def _prepared(name, dev):
    """The case's entry, its default-stream run held to the reference, and the delay for its stressed runs, sized by
    an un-delayed run on a fresh stream that must equal the default-stream run as well."""
    entry = CASES[name](dev)
    assert (entry.reads_back is not None) == (name in READS_BACK), name
    base = so.baseline(entry, dev)
    entry.check(base)
    host_ms, fresh = so.enqueue_ms(entry, dev)
    so.compare(fresh, base, entry, name + " on a fresh stream, no delay")
    return entry, base, host_ms


@pytest.mark.parametrize("name", list(CASES))
def test_late_inputs(cuda, rec, name):
    entry, base, host_ms = _prepared(name, cuda)
    ms = so.delay_ms(host_ms, name, "late inputs")
    got, running = so.late_inputs(entry, cuda, ms, rec)
    so.compare(got, base, entry, name + " with late inputs")
    if name not in READS_BACK:
        assert running, "inconclusive: the %g ms delay had ended when the enqueue of %s returned" % (ms, name)


@pytest.mark.parametrize("name", SLOW_SIDE)
def test_slow_side(cuda, rec, name):
    entry, base, host_ms = _prepared(name, cuda)
    ms = so.delay_ms(host_ms, name, "slow side")
    got, running = so.slow_side(entry, cuda, ms, entry.side(), rec)
    so.compare(got, base, entry, name + " with a slow side stream")
    assert running, "inconclusive: the %g ms delay had ended when the enqueue of %s returned" % (ms, name)


# ------------------------------------------------------------------------------------------------------------------
# Controls: plain torch ops, no library call. Each must FAIL the comparison.
# ------------------------------------------------------------------------------------------------------------------
def _toy(call):
    x = torch.arange(1, 4097, dtype=torch.float32)
    return ec.Entry({"x": x}, call, lambda got: None)


def test_control_work_on_another_stream_is_seen(cuda):
    """An "entry" that multiplies under torch.cuda.stream(other) while its input arrives on `s`: reads the decoy."""
    other = torch.cuda.Stream(cuda)

    def call(live):
        with torch.cuda.stream(other):
            return live["x"] * 2

    entry = _toy(call)
    base = so.baseline(entry, cuda)
    assert torch.equal(base.cpu(), entry.inputs["x"] * 2)
    got, running = so.late_inputs(entry, cuda, so.MIN_MS, apart_from=(other,))
    other.synchronize()
    assert running
    with pytest.raises(AssertionError, match="differs from the default-stream run"):
        so.compare(got, base, entry, "control 1")


def test_control_missing_join_is_seen(cuda):
    """A two-stream toy that forks and never joins, under "slow side": the clone on `s` finds the zero fill."""
    side = torch.cuda.Stream(cuda)

    def call(live):
        y = torch.zeros_like(live["x"])
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            torch.mul(live["x"], 2, out=y)
        return y                                   # (no current_stream.wait_stream(side))

    entry = _toy(call)
    base = so.baseline(entry, cuda)
    assert torch.equal(base.cpu(), entry.inputs["x"] * 2)
    got, running = so.slow_side(entry, cuda, so.MIN_MS, side)
    assert running
    with pytest.raises(AssertionError, match="differs from the default-stream run"):
        so.compare(got, base, entry, "control 2")


def test_control_null_stream_read_is_seen(cuda):
    """A toy that reads its input on the default stream while the input arrives on `s`. torch's pool streams are
    non-blocking streams: the null stream does not wait for them, so the toy reads the decoy. (Were this control to
    stop tripping on some runtime, the harness would be blind to null-stream launches there, and only to those.)"""
    def call(live):
        with torch.cuda.stream(torch.cuda.default_stream(cuda)):
            return live["x"] * 2

    entry = _toy(call)
    base = so.baseline(entry, cuda)
    got, running = so.late_inputs(entry, cuda, so.MIN_MS)
    torch.cuda.synchronize(cuda)
    assert running
    with pytest.raises(AssertionError, match="differs from the default-stream run"):
        so.compare(got, base, entry, "control 3")


# ------------------------------------------------------------------------------------------------------------------
# Cases without a counterpart in test_workspace_gpu.py
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", ["all", "selected"])
def test_one_training_stream_equals_two(cuda, rec, monkeypatch, offsets):
    """LIDF_TRAIN_STREAMS=1 (everything on the caller's stream: the launch order a graph capture takes) against the
    default: query.py's "every sum keeps its fixed order" as an assertion — outputs and gradients bit-identical, on
    the default stream and on `s` with late inputs. feat_grid's gradient keeps its float-atomic bound."""
    name = "query_train_factorised_" + offsets
    entry, two, host_ms = _prepared(name, cuda)
    monkeypatch.setenv("LIDF_TRAIN_STREAMS", "1")
    one = so.baseline(entry, cuda)
    entry.check(one)
    so.compare(one, two, entry, name + ", one stream against two, default stream")
    ms = so.delay_ms(host_ms, name, "late inputs, LIDF_TRAIN_STREAMS=1")
    got, running = so.late_inputs(entry, cuda, ms, rec)
    so.compare(got, two, entry, name + ", one stream with late inputs against two on the default stream")
    assert running


def test_two_callers_share_the_training_side_stream(cuda, rec):
    """Two factorised training steps on two streams, enqueued back to back with a delay in front of each: both fork to
    the one query._TRAIN_SIDE stream. Each equals its own default-stream run."""
    names = ("query_train_factorised_all", "query_train_factorised_selected")
    prepared = [_prepared(n, cuda) for n in names]
    ms = [so.delay_ms(p[2], n, "two callers") for n, p in zip(names, prepared)]
    runs = [so.LateRun(p[0], cuda) for p in prepared]
    torch.cuda.synchronize(cuda)
    side = prepared[0][0].side()
    s1 = so.fresh_stream(cuda, (side,))
    s2 = so.fresh_stream(cuda, (side, s1))
    torch.cuda.synchronize(cuda)
    runs[0].enqueue(ms[0], s1, rec)
    runs[1].enqueue(ms[1], s2, rec)
    for n, run, (entry, base, _) in zip(names, runs, prepared):
        got, running = run.finish()
        so.compare(got, base, entry, n + " beside another caller")
        assert running, n


def _query_call(scene, prob, off, live, dev):
    from implicit_depth_amd.query import lidf_query
    with torch.no_grad():
        out = lidf_query(live["ray_dir"], live["ray_pix"], live["ray_bid"], live["pair_off"], live["pair_ray"],
                         live["pair_vox"], live["pair_t"], live["feat_grid"], live["vox_feat"], prob, off)
    return {k: out[k] for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_pos", "pred_prob_end_softmax",
                                "max_pair_id")}


def test_per_stream_weight_entries_follow_an_update_across_streams(cuda):
    """One decoder pair through lidf_query on s1, then on s2: two packed entries (_lib.packed_entry keeps a blob and
    its guard per stream). After an in-place parameter update queued on s1 behind a delay and s2.wait_stream(s1), the
    call on s2 must answer with the NEW weights — its guard reads the parameters in stream order — held to the
    float64 oracle of the new weights, not to the code; s1's entry is left alone by the call on s2."""
    from implicit_depth_amd import _lib
    from test_f64_gpu import _oracle_query_on
    from util import make_module
    scene, _ = ec.query_scene()
    D = scene["D"]
    with tf32_off():
        prob, off = make_module("IMNET", scene["prob_p"], D, cuda), make_module("IEF", scene["off_p"], D, cuda)
        live = {k: scene[k].to(cuda) for k in ec._SCENE_KEYS[:-1]}
        s1 = so.fresh_stream(cuda)
        s2 = so.fresh_stream(cuda, (s1,))
        torch.cuda.synchronize(cuda)
        with torch.cuda.stream(s1):
            old1 = so.tree_map(torch.clone, _query_call(scene, prob, off, live, cuda))
        with torch.cuda.stream(s2):
            old2 = so.tree_map(torch.clone, _query_call(scene, prob, off, live, cuda))
        torch.cuda.synchronize(cuda)
        ec.same(old2, old1, "s2 against s1, same weights", ref="the run on s1")
        entries = _lib.packed_entries(_lib.PACK_CACHE, prob)
        assert len(entries) == 2 and entries[0].blob.data_ptr() != entries[1].blob.data_ptr()
        e1 = entries[0]
        blob1, guard1 = e1.blob.clone(), e1.guard.clone()
        torch.cuda.synchronize(cuda)
        behind = torch.cuda.Event()
        with torch.cuda.stream(s1):             # the update: late, in place, on s1
            so.spin(so.MIN_MS, cuda)
            behind.record(s1)
            for p in list(prob.parameters()) + list(off.parameters()):
                p.data.mul_(1.25)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            new2 = so.tree_map(torch.clone, _query_call(scene, prob, off, live, cuda))
        running = not behind.query()
        s2.synchronize()
        assert running, "inconclusive: the update had landed before the call on s2 was enqueued"
        # s1's entry: untouched by the call on s2 (still the old weights' streams and fingerprint)
        assert torch.equal(e1.blob, blob1) and torch.equal(e1.guard, guard1)
        assert len(_lib.packed_entries(_lib.PACK_CACHE, prob)) == 2
        new_scene = dict(scene, prob_p={k: v * 1.25 for k, v in scene["prob_p"].items()},
                         off_p={k: v * 1.25 for k, v in scene["off_p"].items()})
        mid = new2["max_pair_id"].long()
        r64 = _oracle_query_on(new_scene, cuda, torch.float64, mid)
        r32 = _oracle_query_on(new_scene, cuda, torch.float32, mid)
        for k in ("pred_offset", "pred_prob_end"):
            assert_f64_close(k + " logit", inv_out_act(new2[k]), inv_out_act(r64[k]), inv_out_act(r32[k]))
        for k in ("pair_pred_pos", "pred_pos", "pred_prob_end_softmax"):
            assert_f64_close(k, new2[k], r64[k], r32[k])
        check_selection(new_scene, new2, r64, r32)
        assert not torch.equal(new2["pred_prob_end"], old2["pred_prob_end"])
        # and s1, which made the update, follows it too — bit-equal to s2's answer
        with torch.cuda.stream(s1):
            new1 = so.tree_map(torch.clone, _query_call(scene, prob, off, live, cuda))
        s1.synchronize()
        ec.same(new1, new2, "s1 after its own update", ref="the run on s2")


def test_eviction_of_per_stream_weight_entries(cuda):
    """The same decoder pair through lidf_query on 17 different streams in turn, no device synchronisation between
    them: MAX_STREAM_ENTRIES = 16 entries at most, every answer bit-equal to the default-stream run, and the first
    stream — whose entry was the one evicted — gets a rebuilt entry and the right answer. (The packed-entry cache
    belongs to lidf_query, lidf_refine and the PointNet; decoders_forward at 300 rows packs into its workspace.)"""
    from implicit_depth_amd import _lib
    from util import make_module
    scene, ref = ec.query_scene()
    D = scene["D"]
    with tf32_off():
        prob, off = make_module("IMNET", scene["prob_p"], D, cuda), make_module("IEF", scene["off_p"], D, cuda)
        live = {k: scene[k].to(cuda) for k in ec._SCENE_KEYS[:-1]}
        torch.cuda.synchronize(cuda)
        base = so.tree_map(torch.clone, _query_call(scene, prob, off, live, cuda))
        torch.cuda.synchronize(cuda)
        for k in ("pred_offset", "pred_prob_end", "pair_pred_pos", "pred_pos"):
            assert (base[k].cpu() - ref[k]).abs().max().item() <= ec.TOL, k
        _lib.invalidate_packed(prob)
        streams = [torch.cuda.Stream(cuda) for _ in range(17)]
        assert len({s.cuda_stream for s in streams}) == 17
        outs = []
        for s in streams + streams[:1]:
            with torch.cuda.stream(s):
                outs.append(so.tree_map(torch.clone, _query_call(scene, prob, off, live, cuda)))
            assert len(_lib.packed_entries(_lib.PACK_CACHE, prob)) <= _lib.MAX_STREAM_ENTRIES
        per = _lib.PACK_CACHE[prob][1]
        assert len(per) == _lib.MAX_STREAM_ENTRIES == 16
        assert streams[1].cuda_stream not in per and streams[0].cuda_stream in per   # evicted: 0, then (for 0) 1
        torch.cuda.synchronize(cuda)
        for i, out in enumerate(outs):
            ec.same(out, base, "stream %d" % i, ref="the default-stream run")
