"""Poisoned byte workspaces (tests only).

The C ABI takes all scratch memory from the caller and, except for lidf_depth_metrics_f32, promises the same
answer whatever bytes the workspace holds on entry (include/lidf_hip.h). `implicit_depth_amd._lib.workspace` is
the one place the Python layer allocates such scratch; `Poisoner.install(monkeypatch)` replaces it with an
allocator that hands out a fresh tensor of the requested size pre-filled by mode:

    zeros    all 0x00 — the clean run
    ones     all 0xFF — every float a NaN, every int -1, every 64-bit status word all bits set
    high     all 0x7F — every float a finite 3.4e38, every int and counter large and positive (what an integer
             maximum or an arg-max keeps, where -1 and NaN lose), every status word a finished "aggregate"
    random   bytes from a torch.Generator seeded per Poisoner
    replay   the i-th allocation is pre-filled with the i-th snapshot of an earlier run (tiled or truncated to
             size): tickets, status words and counters hold the finished values of another problem

`poison_tensor(t, mode)` does the same to a buffer the test owns (FrameRunner.ws / .buf, direct ctypes calls).
"""
import torch

MODES = ("zeros", "ones", "high", "random", "replay")


def _fit(src, nbytes):
    """`src` (uint8, 1-d, any device) tiled or truncated to nbytes."""
    src = src.reshape(-1)
    if src.numel() == 0:
        return torch.zeros((nbytes,), dtype=torch.uint8, device=src.device)
    if src.numel() >= nbytes:
        return src[:nbytes]
    reps = (nbytes + src.numel() - 1) // src.numel()
    return src.repeat(reps)[:nbytes]


def _random_bytes(nbytes, gen):
    """nbytes uniformly random bytes on the CPU from `gen`."""
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=gen)


def poison_tensor(t, mode, gen=None, donor=None):
    """Overwrite every byte of the contiguous tensor `t` in place: 'zeros' / 'ones' / 'high' / 'random' (needs `gen`, a
    CPU torch.Generator) / 'replay' (needs `donor`, any tensor: its bytes tiled or truncated). Returns t."""
    if not t.is_contiguous():
        raise ValueError("poison_tensor: contiguous tensors only")
    if t.numel() == 0:
        return t
    raw = t.view(-1).view(torch.uint8)
    if mode == "zeros":
        raw.zero_()
    elif mode == "ones":
        raw.fill_(0xFF)
    elif mode == "high":
        raw.fill_(0x7F)
    elif mode == "random":
        if gen is None:
            raise ValueError("poison_tensor: mode 'random' needs a generator")
        raw.copy_(_random_bytes(raw.numel(), gen))
    elif mode == "replay":
        if donor is None:
            raise ValueError("poison_tensor: mode 'replay' needs a donor")
        raw.copy_(_fit(donor.contiguous().view(-1).view(torch.uint8), raw.numel()))
    else:
        raise ValueError("poison_tensor: unknown mode %r" % (mode,))
    return t


class Poisoner:
    """Stand-in for _lib.workspace. One per test; `mode` may be switched between runs with begin()."""

    def __init__(self, mode="zeros", seed=0):
        self.gen = torch.Generator().manual_seed(int(seed))
        self.snapshots = []      # clones of a donor run's workspaces, in allocation order
        self.begin(mode)

    def begin(self, mode):
        """Start a run: forget the tensors handed out so far (snapshots are kept) and set the mode."""
        if mode not in MODES:
            raise ValueError("unknown mode %r" % (mode,))
        self.mode = mode
        self.handed = []
        return self

    def snapshot(self):
        """Clone every workspace handed out since begin() — what the kernels left there — as the donor of later
        'replay' runs. The stream is synchronised first."""
        if any(t.is_cuda for t in self.handed):
            torch.cuda.synchronize()
        self.snapshots = [t.clone() for t in self.handed]
        return self.snapshots

    def workspace(self, nbytes, device):
        """Same contract as _lib.workspace: a fresh uint8 tensor of max(nbytes, 1) bytes on `device`."""
        n = max(int(nbytes), 1)
        t = torch.empty((n,), dtype=torch.uint8, device=device)
        i = len(self.handed)
        if self.mode == "replay":
            if i < len(self.snapshots):
                t.copy_(_fit(self.snapshots[i], n))
            else:            # more allocations than the donor made: reuse them round-robin, zeros if none
                t.copy_(_fit(self.snapshots[i % len(self.snapshots)], n) if self.snapshots
                        else torch.zeros((n,), dtype=torch.uint8))
        else:
            poison_tensor(t, self.mode, gen=self.gen)
        self.handed.append(t)
        return t

    def install(self, monkeypatch):
        """Replace implicit_depth_amd._lib.workspace for the duration of the test."""
        from implicit_depth_amd import _lib
        monkeypatch.setattr(_lib, "workspace", self.workspace)
        return self
