"""The chained 16-row decoders (csrc/lidf_chain16.h: the f32 and split-f16 any-width chains and the stage-2 entry
over one tile body and one kernel body) against the outputs of the three separate kernel files they were folded from:
tests/golden/chain16_parent.npz, written by tests/golden/make_chain16_parent.py with the build before the fold. The
kernels have no atomics and the fold keeps the order of every accumulation, so the comparison is torch.equal. The
cases, what each of them reaches and the inputs (numpy PCG64, a fixed seed) are that file's."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_chain16_parent",
                                               os.path.join(HERE, "golden", "make_chain16_parent.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def parent():
    return np.load(gen.FIXTURE)


@pytest.fixture(scope="module")
def chain_inputs(cuda):
    return gen.chain_inputs(cuda)


def _same(got, want):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want)))


@pytest.mark.parametrize("precision", gen.PRECISIONS)
@pytest.mark.parametrize("kind", gen.KINDS)
@pytest.mark.parametrize("gf", gen.GFS)
def test_chain_small_rows_equal_the_parent(cuda, parent, chain_inputs, gf, kind, precision):
    """1, 17 and 33 rows at every k and table form: stored whole."""
    seen = 0
    rows = {n: 0 for n in gen.NS}
    for case in gen.chain_cases():
        n = case[-1]
        i, rows[n] = rows[n], rows[n] + 1
        if case[:3] != (gf, kind, precision) or n == gen.N_LARGE:
            continue
        got = gen.run_chain_case(chain_inputs, case)
        assert _same(got, parent["chain_%d" % n][i]), case
        seen += 1
    assert seen == len(gen.KS) * len(gen.TABLES) * 3


@pytest.mark.parametrize("precision", gen.PRECISIONS)
@pytest.mark.parametrize("kind", gen.KINDS)
@pytest.mark.parametrize("gf", gen.GFS)
def test_chain_81961_rows_equal_the_parent(cuda, parent, chain_inputs, gf, kind, precision):
    """81,961 rows (pairs and an odd sub-tile in every wavefront on 256 compute units): SHA-256 of the output bytes,
    and the first and last 64 values for a readable failure."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    if cus != gen.CUS:
        pytest.skip("the split of the sub-tiles over wavefronts the fixture was made for needs %d compute units; this "
                    "device has %d" % (gen.CUS, cus))
    seen = 0
    for i, case in enumerate(c for c in gen.chain_cases() if c[-1] == gen.N_LARGE):
        if case[:3] != (gf, kind, precision):
            continue
        got = gen.run_chain_case(chain_inputs, case)
        assert got.shape == (gen.N_LARGE,)
        assert _same(got[:64], parent["chain_head"][i]) and _same(got[-64:], parent["chain_tail"][i]), case
        assert _same(gen.digest(got), parent["chain_sha"][i]), case
        seen += 1
    assert seen == len(gen.KS) * len(gen.TABLES)


@pytest.mark.parametrize("i,case", list(enumerate(gen.refine_cases())),
                         ids=["%dx%d-L%d-%s" % (c[0][0], c[0][1], c[1], c[2]) for c in gen.refine_cases()])
def test_stage2_equals_the_parent(cuda, parent, i, case):
    """query.lidf_refine, two iterations: pred_pos and end_voxel_id."""
    pos, ev = gen.run_refine_case(cuda, case)
    assert _same(ev, parent["refine_ev_%d" % i]), case
    assert _same(pos, parent["refine_pos_%d" % i]), case
