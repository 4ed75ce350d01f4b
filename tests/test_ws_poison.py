"""tests/ws_poison.py on CPU tensors: each mode's bytes, sizes and dtypes, replay with size mismatches either
way, and that the patch of _lib.workspace is undone after the test."""
import pytest
import torch

from implicit_depth_amd import _lib
from ws_poison import MODES, Poisoner, poison_tensor

CPU = torch.device("cpu")
_ORIGINAL = _lib.workspace


@pytest.fixture
def poison(monkeypatch):
    return Poisoner("zeros", seed=1234).install(monkeypatch)


def test_modes_fill_the_stated_bytes(poison):
    assert _lib.workspace is not _ORIGINAL and _lib.workspace == poison.workspace
    z = _lib.workspace(4096, CPU)
    assert bool((z == 0).all())
    poison.begin("ones")
    o = _lib.workspace(4096, CPU)
    assert bool((o == 0xFF).all())
    assert bool(torch.isnan(o.view(torch.float32)).all())              # every float a NaN
    assert bool((o.view(torch.int32) == -1).all())                     # every int -1
    assert bool((o.view(torch.int64) == -1).all())                     # every 64-bit status word all bits set
    poison.begin("high")
    h = _lib.workspace(4096, CPU)
    assert bool((h == 0x7F).all())
    f = h.view(torch.float32)
    assert bool(torch.isfinite(f).all()) and bool((f > 3e38).all())    # every float finite and huge
    assert bool((h.view(torch.int32) == 0x7F7F7F7F).all())             # every int large and positive
    assert bool((h.view(torch.int64) >> 62 == 1).all())                # every status word: flag 1, an aggregate
    poison.begin("random")
    r = _lib.workspace(1 << 16, CPU)
    assert r.unique().numel() == 256                                   # every byte value occurs in 64 Ki draws
    again = Poisoner("random", seed=1234).workspace(1 << 16, CPU)
    assert torch.equal(r, again)                                       # seeded per Poisoner: reproducible
    other = Poisoner("random", seed=1235).workspace(1 << 16, CPU)
    assert not torch.equal(r, other)
    assert not torch.equal(r, _lib.workspace(1 << 16, CPU))            # the generator advances between requests


@pytest.mark.parametrize("mode", MODES)
def test_sizes_and_dtype(poison, mode):
    poison.begin(mode)
    for n in (0, 1, 7, 256, 4097):
        t = _lib.workspace(n, CPU)
        assert t.dtype == torch.uint8 and t.dim() == 1 and t.device == CPU
        assert t.numel() == max(n, 1)                                   # a zero-byte request still gets one byte
        assert t.is_contiguous()
    assert len(poison.handed) == 5
    a, b = poison.handed[2], poison.handed[3]
    assert a.data_ptr() != b.data_ptr()                                 # fresh tensors, never views of one pool


def test_replay_prefills_allocation_i_with_snapshot_i(poison):
    poison.begin("zeros")
    first, second, third = _lib.workspace(8, CPU), _lib.workspace(16, CPU), _lib.workspace(5, CPU)
    first.copy_(torch.arange(8, dtype=torch.uint8))                     # "what the kernels left there"
    second.copy_(torch.arange(100, 116, dtype=torch.uint8))
    third.copy_(torch.tensor([9, 8, 7, 6, 5], dtype=torch.uint8))
    snaps = poison.snapshot()
    assert len(snaps) == 3 and snaps[0].data_ptr() != first.data_ptr()
    first.zero_()                                                        # snapshots are clones
    assert torch.equal(snaps[0], torch.arange(8, dtype=torch.uint8))

    poison.begin("replay")
    same = _lib.workspace(8, CPU)
    assert torch.equal(same, torch.arange(8, dtype=torch.uint8))
    shorter = _lib.workspace(6, CPU)                                     # donor larger: truncated
    assert torch.equal(shorter, torch.arange(100, 106, dtype=torch.uint8))
    longer = _lib.workspace(12, CPU)                                     # donor smaller: tiled
    assert torch.equal(longer, torch.tensor([9, 8, 7, 6, 5, 9, 8, 7, 6, 5, 9, 8], dtype=torch.uint8))
    extra = _lib.workspace(3, CPU)                                       # more allocations than the donor made
    assert torch.equal(extra, torch.tensor([0, 1, 2], dtype=torch.uint8))
    assert len(poison.handed) == 4 and len(poison.snapshots) == 3       # begin() kept the snapshots

    empty = Poisoner("replay")                                           # no donor at all: zeros, not a crash
    assert bool((empty.workspace(4, CPU) == 0).all())


def test_poison_tensor_on_owned_buffers():
    gen = torch.Generator().manual_seed(7)
    f = torch.ones((3, 5), dtype=torch.float32)
    assert poison_tensor(f, "ones") is f and bool(torch.isnan(f).all())
    i = torch.ones((7,), dtype=torch.int64)
    poison_tensor(i, "ones")
    assert bool((i == -1).all())
    poison_tensor(i, "zeros")
    assert bool((i == 0).all())
    poison_tensor(i, "random", gen=gen)
    assert i.unique().numel() > 1
    d = torch.zeros((10,), dtype=torch.uint8)
    poison_tensor(d, "replay", donor=torch.tensor([1, 2, 3], dtype=torch.uint8))
    assert d.tolist() == [1, 2, 3, 1, 2, 3, 1, 2, 3, 1]
    poison_tensor(d, "replay", donor=torch.tensor([258], dtype=torch.int32).repeat(5))   # 20 donor bytes, truncated
    assert d.tolist() == [2, 1, 0, 0, 2, 1, 0, 0, 2, 1]
    assert poison_tensor(torch.empty((0,)), "ones").numel() == 0
    with pytest.raises(ValueError):
        poison_tensor(d, "random")
    with pytest.raises(ValueError):
        poison_tensor(d, "replay")
    with pytest.raises(ValueError):
        poison_tensor(d, "bogus")
    with pytest.raises(ValueError):
        poison_tensor(torch.zeros((4, 4)).t(), "ones")
    with pytest.raises(ValueError):
        Poisoner("bogus")


def test_patch_is_undone_after_the_test():
    """Runs after the tests above that used the fixture: monkeypatch restored the product's allocator."""
    assert _lib.workspace is _ORIGINAL
    t = _lib.workspace(0, CPU)
    assert t.numel() == 1 and t.dtype == torch.uint8
