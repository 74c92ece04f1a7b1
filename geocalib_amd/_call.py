"""The one call path from the package to the C ABI (include/gclm.h): what every gclm_* call needs from torch -- pointers,
the stream, float32 device tensors, the HIP device the launch goes to -- and how a return code becomes an exception.
`_lib` stays the torch-free ctypes binding; every other module calls the library through `call` and prepares its
arguments with the helpers here."""
import torch

from . import _lib

MAX_CALL = 65535      # images per C call (grid.y of the kernels)


def slices(n: int):
    """(first, count) of the C calls a batch of `n` images takes."""
    for first in range(0, n, MAX_CALL):
        yield first, min(MAX_CALL, n - first)


def ptr(t):
    """The device pointer the C ABI takes; None (a tensor the caller does not have) is NULL."""
    return None if t is None else t.data_ptr()


def ptr_at(t, b0: int):
    """... of image `b0` onwards of a batch tensor: what a sliced call (slices) hands its entry."""
    return None if t is None else t[b0].data_ptr()


def raw_stream(device: torch.device) -> int:
    """The current HIP stream of `device` as the integer the C ABI takes (torch.cuda.current_stream(...).cuda_stream builds a
    Stream object first: 4.5 us per call on the single-image path)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    try:
        return torch._C._cuda_getCurrentRawStream(idx)
    except AttributeError:            # a torch without the private accessor
        return torch.cuda.current_stream(device).cuda_stream


def require_device(t: torch.Tensor, name: str) -> None:
    """THE device check of the package (a CPU test of the host side replaces this one function)."""
    if not t.is_cuda:
        raise RuntimeError(f"geocalib_amd: `{name}` must live on a HIP device (got {t.device}); "
                           "the MI355X path has no CPU fallback")


def dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    """`t` as the kernels read it: on a HIP device, float32, contiguous, detached."""
    require_device(t, name)
    if t.dtype is torch.float32 and t.is_contiguous() and not t.requires_grad:
        return t                                   # the common case: nothing to convert (saves three dispatcher trips)
    return t.detach().to(torch.float32).contiguous()


def dev_u8(t: torch.Tensor, name: str):
    """A (B, C, H, W) byte image as the kernels read it, and its layout flag: on a HIP device, uint8, detached; planar
    (contiguous, 0) or interleaved (channels_last with C <= 4, 1) as it lies in memory, without a copy.  Any other stride
    pattern, or channels_last with C > 4, is copied to planar."""
    require_device(t, name)
    if t.dtype is not torch.uint8 or t.dim() != 4:
        raise RuntimeError(f"geocalib_amd: `{name}` must be a (B, C, H, W) uint8 image, got {t.dtype} {tuple(t.shape)}")
    t = t.detach()
    if t.is_contiguous():
        return t, 0
    if t.shape[1] <= 4 and t.is_contiguous(memory_format=torch.channels_last):
        return t, 1
    return t.contiguous(), 0


def call(name: str, *args, handle=None, comm=None, device=None) -> None:
    """`name(*args)` of the library (looked up through _lib.load() at call time); a non-zero return raises GclmError.

    `args` are the C arguments in the order of include/gclm.h, the stream included: the caller passes it (raw_stream), since
    a solve keys its handle by the same integer and some entries take none.

    handle / comm: the gclm_handle / gclm_comm among `args`.  Such an entry switches to its own device inside the library, so
    no device context is entered here, and a failure carries the object's gclm_last_error / gclm_comm_last_error text.
    device: for an entry that takes neither, where the tensors live -- the launch goes to HIP's CURRENT device, so it is
    switched for the call only when that is another one (one process per GPU: never; the context manager costs 3-4 us of a
    10 us single-image call).  A failure of such an entry carries the code alone: without a handle gclm_last_error returns
    the thread's last failed gclm_create, which is that call's own message and nobody else's."""
    fn = getattr(_lib.load(), name)
    if handle is None and comm is None and device is not None and \
            (device.index if device.index is not None else torch.cuda.current_device()) != torch.cuda.current_device():
        with torch.cuda.device(device):
            rc = fn(*args)
    else:
        rc = fn(*args)
    if rc == 0:
        return
    if comm is not None or name == "gclm_comm_create":
        msg = _lib.load().gclm_comm_last_error(comm)
        raise _lib.GclmError(f"{name} failed ({rc}): {msg.decode() if msg else ''}")
    if handle is not None or name == "gclm_create":
        _lib.check(rc, handle, name)
    raise _lib.GclmError(f"{name} failed ({rc})")
