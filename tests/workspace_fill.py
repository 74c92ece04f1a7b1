"""What a caller-owned workspace held must not reach the result (no test in here).

The handle-free entry points take their scratch memory from the caller, and the Python wrappers hand over `torch.empty`
memory: whatever the allocator gives back.  `same_bits_whatever_the_memory_held` runs one wrapper call three times with
`torch.empty` / `torch.empty_like` on the device served from ONE arena -- filled with 0x00 bytes, filled with 0xFF bytes (NaN
patterns), and as a call of another shape left it -- and asserts the same bits in all three runs."""
import math

import torch


class Arena:
    """Serves torch.empty / torch.empty_like on a HIP device from one buffer, in order, 256-byte aligned."""

    def __init__(self, dev, nbytes=64 << 20):
        self._empty, self._empty_like = torch.empty, torch.empty_like
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.off = self.handed = 0

    def empty(self, *size, dtype=None, device=None, **kw):
        if device is None or torch.device(device).type != "cuda":
            return self._empty(*size, dtype=dtype, device=device, **kw)
        assert not kw.get("requires_grad") and kw.get("out") is None, kw
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        dtype = dtype or torch.get_default_dtype()
        n = math.prod(shape) * dtype.itemsize
        off, self.off = self.off, (self.off + n + 255) // 256 * 256
        assert self.off <= self.buf.numel(), (shape, dtype)
        self.handed += 1
        return self.buf[off:off + n].view(dtype).view(shape)

    def empty_like(self, t, dtype=None, **kw):
        if not t.is_cuda:
            return self._empty_like(t, dtype=dtype, **kw)
        return self.empty(tuple(t.shape), dtype=dtype or t.dtype, device=t.device)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits_whatever_the_memory_held(monkeypatch, dev, run, other):
    """`run()` -> the output tensors of the call under test (None entries allowed); `other()`: a call of another shape."""
    arena = Arena(dev)
    monkeypatch.setattr(torch, "empty", arena.empty)
    monkeypatch.setattr(torch, "empty_like", arena.empty_like)
    results = []
    for fill in (0x00, 0xFF, "other"):
        if fill == "other":
            arena.off = 0
            other()
        else:
            arena.buf.fill_(fill)
        arena.off, before = 0, arena.handed
        out = run()
        assert arena.handed > before                      # the call's scratch memory did come from the arena
        results.append([None if t is None else t.clone() for t in out])
    torch.cuda.synchronize(dev)
    monkeypatch.undo()
    assert any(t is not None for t in results[0])
    for what, r in zip(("0xFF bytes", "another call's records"), results[1:]):
        for i, (a, b) in enumerate(zip(results[0], r)):
            assert (a is None) == (b is None)
            assert a is None or torch.equal(_bits(a), _bits(b)), (what, i)
