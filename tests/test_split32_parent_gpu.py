"""The split-f16 decoders on 32 x 32 tiles (precision="f16x3"; csrc/lidf_split32.h: one stream feed, one tail of the
pass and one packer under the fused per-point query and the decoder on materialised rows) against the outputs of the
two separate kernel files they were folded from: tests/golden/split32_parent.npz, written by
tests/golden/make_split32_parent.py with the build before the fold. The fold keeps the order of every accumulation and
the stream format, so the comparison is of bit patterns (float outputs through an int32 view: with offsets="selected"
the unwritten rows are NaN). The cases, what each of them reaches and the inputs (numpy PCG64, a fixed seed) are that
file's."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_split32_parent",
                                               os.path.join(HERE, "golden", "make_split32_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent():
    return np.load(gen.FIXTURE)


@pytest.fixture(scope="module")
def rows_inputs(cuda):
    return gen.rows_inputs(cuda)


@pytest.fixture(scope="module")
def query_inputs(cuda):
    return gen.query_inputs(cuda)


def _bits(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.float32 else a)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _rows_id(c):
    return "n%d-D%d-%s-%s%s" % (c[0], c[1], c[2], c[3], "-strided" if c[4] else "")


@pytest.mark.parametrize("i,case", list(enumerate(gen.rows_cases())), ids=[_rows_id(c) for c in gen.rows_cases()])
def test_rows_equal_the_parent(cuda, parent, rows_inputs, i, case):
    """decoders.decoders_forward at f16x3. 32,901 rows: SHA-256 of the output bytes, and the first and last 64 values
    of every net for a readable failure."""
    got = gen.run_rows_case(rows_inputs, case)
    if case[0] == gen.N_LARGE:
        assert got.shape[1] == gen.N_LARGE
        assert _same(got[:, :64], parent["rows_head_%d" % i]) and _same(got[:, -64:], parent["rows_tail_%d" % i]), case
        assert _same(gen.digest(got), parent["rows_sha_%d" % i]), case
    else:
        assert _same(got, parent["rows_%d" % i]), case


@pytest.mark.parametrize("i,case", list(enumerate(gen.query_cases())),
                         ids=["%s-rel%d-L%d-%s-%s" % (c[0], c[1], c[2], c[3], c[4]) for c in gen.query_cases()])
def test_query_equals_the_parent(cuda, parent, query_inputs, i, case):
    """query.lidf_query at f16x3: every output of the call."""
    for key, got in zip(gen.QUERY_KEYS, gen.run_query_case(query_inputs, case)):
        assert _same(got, parent["query_%d_%s" % (i, key)]), (case, key)


def test_stage2_equals_the_parent(cuda, parent):
    """query.lidf_refine at f16x3, 33 rays, two iterations: pred_pos and end_voxel_id."""
    pos, ev = gen.run_refine_case(cuda)
    assert _same(ev, parent["refine_ev"])
    assert _same(pos, parent["refine_pos"])


@pytest.mark.parametrize("i,case", list(enumerate(gen.stream_cases())),
                         ids=["L%d-%s" % c for c in gen.stream_cases()])
def test_packed_streams_equal_the_parent(cuda, parent, query_inputs, i, case):
    """The bytes both packers write: the fused query's blob and the rows stream with its aux."""
    fused, rows = gen.run_stream_case(query_inputs, case)
    assert _same(rows, parent["stream_rows_%d" % i]), case
    assert _same(fused, parent["stream_fused_%d" % i]), case
