"""The step before the LM path: CNN-head epilogue fused into one HIP pass (gclm_pack_fields).

Replaces the tail of the reference's UpDecoder / LatitudeDecoder (geocalib/geocalib.py:57,73-75):

    up_field            = F.normalize(up_raw, dim=1)
    up_confidence       = sigmoid(up_log_confidence)
    latitude_field      = asin(clamp(tanh(lat_raw), -1 + 1e-5, 1 - 1e-5))
    latitude_confidence = sigmoid(lat_log_confidence)

and writes the five planes in the layout LMOptimizer reads (eager PyTorch: 8 kernels, ~18 plane passes) -- and, on request,
a sixth: sin(latitude_field), which the LM solve reads in place of the radians (gclm_pack_fields_ex).  `pack_fields_from_logits`
is the same step for classification heads (gclm_pack_fields_bins).  `pack_fields` reads float16 / bfloat16 raws as they are
(gclm_pack_fields_typed) and, for raws that require grad, carries a graph whose backward is one more HIP pass
(gclm_pack_fields_backward): with losses.perspective_field_loss and the differentiable LMOptimizer, everything after the
network's last convolution is this package's, forward and backward -- for classification heads too: `bin_loss` /
`bin_loss_grad` (gclm_bin_loss, gclm_bin_loss_grad) are the host wrappers behind losses.perspective_bin_loss."""
import ctypes
from typing import Dict, Optional

import torch
from torch.autograd.function import once_differentiable

from . import _call, _lib


_LOGIT_DTYPES = {torch.float32: _lib.LOGIT_DTYPE_IDS["float32"], torch.float16: _lib.LOGIT_DTYPE_IDS["float16"],
                 torch.bfloat16: _lib.LOGIT_DTYPE_IDS["bfloat16"]}
_HALF_DTYPES = (torch.float16, torch.bfloat16)


def _pack_call(up_raw, lat_raw, ulc, llc, inplace: bool, sin_latitude: bool):
    """The forward launch of pack_fields on raws as the kernels read them -- contiguous, detached, all float32 or all of one
    16-bit type: (up, lat, up_conf, lat_conf, sin_lat), None for a plane not asked for."""
    B, _, H, W = lat_raw.shape
    assert up_raw.shape == (B, 2, H, W), up_raw.shape
    for c in (ulc, llc):
        assert c is None or c.numel() == B * H * W, c.shape
    if lat_raw.dtype is torch.float32:
        out_like = (lambda t: t) if inplace else torch.empty_like
        entry, dtype = "gclm_pack_fields_ex", ()
    else:
        out_like = lambda t: torch.empty_like(t, dtype=torch.float32)      # noqa: E731
        entry, dtype = "gclm_pack_fields_typed", (_LOGIT_DTYPES[lat_raw.dtype],)
    up, lat = out_like(up_raw), out_like(lat_raw)
    upc = None if ulc is None else out_like(ulc).view(B, H, W)
    latc = None if llc is None else out_like(llc).view(B, H, W)
    slat = torch.empty_like(lat) if sin_latitude else None       # (never in place: a plane of its own)
    p = _call.ptr
    _call.call(entry, *dtype, p(up_raw), p(ulc), p(lat_raw), p(llc), B, H, W, p(up), p(upc), p(lat), p(latc), p(slat),
               _call.raw_stream(lat_raw.device), device=lat_raw.device)
    return up, lat, upc, latc, slat


class _PackFieldsFunction(torch.autograd.Function):
    """(up_raw, lat_raw, up_log_confidence, lat_log_confidence) -> (up, lat, up_conf, lat_conf, sin_lat) with a graph: the
    forward is _pack_call, the backward one pass of gclm_pack_fields_backward that reads the raws again -- nothing but the
    inputs is kept.  The raws come contiguous, all float32 or all of one 16-bit type; an absent confidence is None."""

    @staticmethod
    def forward(ctx, up_raw, lat_raw, ulc, llc, sin_latitude):
        out = _pack_call(up_raw, lat_raw, ulc, llc, False, sin_latitude)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*(t for t in (up_raw, lat_raw, ulc, llc) if t is not None))
        ctx.given = [t is not None for t in (up_raw, lat_raw, ulc, llc)]
        if out[4] is not None:
            ctx.mark_non_differentiable(out[4])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_up, g_lat, g_upc, g_latc, g_slat):
        saved = list(ctx.saved_tensors)
        up_raw, lat_raw, ulc, llc = (saved.pop(0) if g else None for g in ctx.given)
        B, _, H, W = lat_raw.shape
        # a raw gets a gradient where it asks for one and its output got one; every other group is left out of the pass
        raws, grads, out = [], [], []
        for i, (raw, g) in enumerate(((up_raw, g_up), (lat_raw, g_lat), (ulc, g_upc), (llc, g_latc))):
            want = raw is not None and g is not None and ctx.needs_input_grad[i]
            raws.append(raw if want else None)
            grads.append(g.to(torch.float32).contiguous() if want else None)
            out.append(torch.empty_like(raw) if want else None)
        if any(o is not None for o in out) and B > 0:
            p, dev = _call.ptr, lat_raw.device
            _call.call("gclm_pack_fields_backward", _LOGIT_DTYPES[lat_raw.dtype], p(raws[0]), p(raws[2]), p(raws[1]), p(raws[3]),
                       B, H, W, p(grads[0]), p(grads[2]), p(grads[1]), p(grads[3]), p(out[0]), p(out[2]), p(out[1]), p(out[3]),
                       _call.raw_stream(dev), device=dev)
        return (*out, None)


def pack_fields(up_raw: torch.Tensor, lat_raw: torch.Tensor, up_log_confidence: Optional[torch.Tensor] = None,
                lat_log_confidence: Optional[torch.Tensor] = None, inplace: bool = False,
                sin_latitude: bool = False) -> Dict[str, torch.Tensor]:
    """up_raw (B,2,H,W), lat_raw (B,1,H,W), log-confidences (B,H,W) or (B,1,H,W): raw head outputs on a HIP device.
    Returns the dict `LMOptimizer.forward` consumes, float32.

    `sin_latitude`: the dict also holds "sin_latitude" (B,1,H,W), sin of "latitude_field" written by the same launch with
    the solve's own polynomial.  LMOptimizer reads it in place of the radians where its sweeps can (include/gclm.h:
    gclm_solve_ex) -- same results bit for bit, no per-sweep sin and no library-owned scratch plane.  The key names no
    field / confidence / uncertainty, so GeoCalib._post_process neither resizes nor returns it.

    Raws that are all float16 or all bfloat16 (what the heads emit under autocast) and contiguous are read as they are
    (gclm_pack_fields_typed): no conversion pass, the bits of the call on `.float()` of them.  Mixed dtypes and strided raws
    are brought to contiguous float32 by torch first.

    In grad mode, with a raw that requires grad and `inplace` False, the outputs carry a graph: same values bit for bit, and
    backward is one HIP pass on torch's current stream (gclm_pack_fields_backward) that reads the raws again and keeps nothing
    else; gradients come back in each raw's dtype and shape, once (no double backward), none for "sin_latitude".
    `inplace=True` overwrites float32 raws as it always did and attaches NO graph, whatever requires grad."""
    names = ("up_raw", "lat_raw", "up_log_confidence", "lat_log_confidence")
    given = [t for t in (up_raw, lat_raw, up_log_confidence, lat_log_confidence) if t is not None]
    half = (not inplace and lat_raw.dtype in _HALF_DTYPES and all(t.dtype is lat_raw.dtype and t.is_contiguous() for t in given))
    graph = torch.is_grad_enabled() and not inplace and any(t.requires_grad for t in given)
    if graph or half:
        for t, name in zip((up_raw, lat_raw, up_log_confidence, lat_log_confidence), names):
            if t is not None:
                _call.require_device(t, name)
    if graph:
        if not half:      # differentiable torch ops, outside the Function: mixed or strided raws still get their gradients
            up_raw, lat_raw, up_log_confidence, lat_log_confidence = (
                None if t is None else t.float().contiguous() for t in (up_raw, lat_raw, up_log_confidence, lat_log_confidence))
        up, lat, upc, latc, slat = _PackFieldsFunction.apply(up_raw, lat_raw, up_log_confidence, lat_log_confidence, sin_latitude)
    elif half:
        up, lat, upc, latc, slat = _pack_call(*(None if t is None else t.detach() for t in
                                                 (up_raw, lat_raw, up_log_confidence, lat_log_confidence)), False, sin_latitude)
    else:
        up_raw, lat_raw = _call.dev_f32(up_raw, "up_raw"), _call.dev_f32(lat_raw, "lat_raw")
        ulc = None if up_log_confidence is None else _call.dev_f32(up_log_confidence, "up_log_confidence")
        llc = None if lat_log_confidence is None else _call.dev_f32(lat_log_confidence, "lat_log_confidence")
        up, lat, upc, latc, slat = _pack_call(up_raw, lat_raw, ulc, llc, inplace, sin_latitude)
    out = {"up_field": up, "latitude_field": lat}
    if upc is not None:
        out["up_confidence"] = upc
    if latc is not None:
        out["latitude_confidence"] = latc
    if slat is not None:
        out["sin_latitude"] = slat
    return out


def pack_fields_from_logits(up_logits: torch.Tensor, lat_logits: torch.Tensor, up_log_confidence: Optional[torch.Tensor] = None,
                            lat_log_confidence: Optional[torch.Tensor] = None, sin_latitude: bool = False) -> Dict[str, torch.Tensor]:
    """`pack_fields` for classification heads (the original PerspectiveFields weights; the reference's decoders with
    loss_type == "classification"): up_logits (B, Ku, h, w) and lat_logits (B, Kl, h, w) -- 73 and 180 bins there --, both
    float32, float16 or bfloat16 and contiguous; log-confidences (B, h, w) or (B, 1, h, w).  Returns the dict
    `LMOptimizer.forward` consumes, float32, with the keys of `pack_fields`:

        up_field       = decode_up_bin(up_logits.argmax(1), Ku)                     (B, 2, h, w)
        latitude_field = decode_bin_latitude(lat_logits.argmax(1), Kl)[:, None]     (B, 1, h, w)
        confidences    = sigmoid(log-confidences)                                    (B, h, w)

    with the decodes of `perspective_encoding` and torch.argmax's rule (the first index of the greatest value, a NaN greater
    than everything).  On a HIP device that is ONE launch on torch's current stream (gclm_pack_fields_bins), which gathers
    from the tables of `perspective_encoding`: fields equal to this composition's bit for bit.  On CPU tensors the composition
    itself runs -- the readable statement of the definition; there `sin_latitude` is torch.sin of the latitude, the device
    plane's definition up to the sweep's polynomial, not bit-equal to it.

    Raises ValueError for logits that are not two 4-D tensors of one (B, h, w), device and dtype, for another dtype, for more
    than 2048 bins, and for non-contiguous logits: 253 planes are not copied silently."""
    from . import perspective_encoding as pe
    if up_logits.dim() != 4 or lat_logits.dim() != 4:
        raise ValueError(f"logits are (B, bins, h, w), got {tuple(up_logits.shape)} and {tuple(lat_logits.shape)}")
    (B, Ku, H, W), Kl = up_logits.shape, lat_logits.shape[1]
    if lat_logits.shape != (B, Kl, H, W) or lat_logits.device != up_logits.device:
        raise ValueError(f"up logits {tuple(up_logits.shape)} on {up_logits.device} and latitude logits {tuple(lat_logits.shape)} "
                         f"on {lat_logits.device} must share B, h, w and the device")
    if up_logits.dtype != lat_logits.dtype:
        raise ValueError(f"the logits must share one dtype, got {up_logits.dtype} and {lat_logits.dtype}")
    if up_logits.dtype not in _LOGIT_DTYPES:
        raise ValueError(f"logits are float32, float16 or bfloat16, got {up_logits.dtype}")
    if not 2 <= Ku <= _lib.MAX_BINS or not 1 <= Kl <= _lib.MAX_BINS:
        raise ValueError(f"2..{_lib.MAX_BINS} up bins and 1..{_lib.MAX_BINS} latitude bins, got {Ku} and {Kl}")
    if not (up_logits.is_contiguous() and lat_logits.is_contiguous()):
        raise ValueError("the logits must be contiguous (B, bins, h, w): call .contiguous() if a copy of every plane is meant")
    confs = {"up_log_confidence": up_log_confidence, "lat_log_confidence": lat_log_confidence}
    for name, c in confs.items():
        if c is not None and (c.numel() != B * H * W or c.shape[-2:] != (H, W) or c.device != up_logits.device):
            raise ValueError(f"`{name}` {tuple(c.shape)} on {c.device} does not fit {B} images of {H} x {W} on {up_logits.device}")
    dev = up_logits.device
    up_table, lat_table = pe.up_bin_table(Ku, dev), pe.latitude_bin_table(Kl, dev)
    if not up_logits.is_cuda:
        up, lat = pe.fields_from_logits(up_logits.detach(), lat_logits.detach())
        upc, latc = (None if c is None else torch.sigmoid(c.detach().float()).reshape(B, H, W) for c in confs.values())
        slat = torch.sin(lat) if sin_latitude else None
    else:
        up_logits, lat_logits = up_logits.detach(), lat_logits.detach()
        ulc, llc = (None if c is None else _call.dev_f32(c, name) for name, c in confs.items())
        up, lat = up_table.new_empty((B, 2, H, W)), up_table.new_empty((B, 1, H, W))
        upc, latc = (None if c is None else torch.empty_like(c).view(B, H, W) for c in (ulc, llc))
        slat = torch.empty_like(lat) if sin_latitude else None
        p = _call.ptr
        _call.call("gclm_pack_fields_bins", p(up_logits), Ku, p(lat_logits), Kl, _LOGIT_DTYPES[up_logits.dtype], p(up_table),
                   p(lat_table), p(ulc), p(llc), B, H, W, p(up), p(upc), p(lat), p(latc), p(slat), _call.raw_stream(dev), device=dev)
    out = {"up_field": up, "latitude_field": lat}
    if upc is not None:
        out["up_confidence"] = upc
    if latc is not None:
        out["latitude_confidence"] = latc
    if slat is not None:
        out["sin_latitude"] = slat
    return out


def upsample_fields(t: torch.Tensor, size) -> torch.Tensor:
    """Bilinear resize of the trailing (h, w) planes of `t` to `size` = (H, W), matching
    `torch.nn.functional.interpolate(t, size, mode="bilinear", align_corners=False)` (extractor.py:60-63)."""
    H, W = int(size[0]), int(size[1])
    src = _call.dev_f32(t, "t")
    h, w = src.shape[-2:]
    dst = src.new_empty(src.shape[:-2] + (H, W))
    planes = src.numel() // (h * w)
    _call.call("gclm_upsample_fields", src.data_ptr(), planes, h, w, H, W, dst.data_ptr(), _call.raw_stream(src.device),
               device=src.device)
    return dst


def upsample_fields_multi(tensors, size):
    """`upsample_fields` for several tensors of equal (h, w) in ONE launch (gclm_upsample_fields_multi): the outputs are views
    of one allocation, each contiguous, with the leading shape of its source."""
    H, W = int(size[0]), int(size[1])
    srcs = [_call.dev_f32(t, "tensors") for t in tensors]
    h, w = srcs[0].shape[-2:]
    assert all(t.shape[-2:] == (h, w) and t.device == srcs[0].device for t in srcs) and 1 <= len(srcs) <= 8
    planes = [t.numel() // (h * w) for t in srcs]
    flat = srcs[0].new_empty((sum(planes), H, W))
    outs, lo = [], 0
    for t, n in zip(srcs, planes):
        outs.append(flat[lo:lo + n].view(t.shape[:-2] + (H, W)))
        lo += n
    C = _lib.C
    n = len(srcs)
    _call.call("gclm_upsample_fields_multi", (C.c_void_p * n)(*[t.data_ptr() for t in srcs]),
               (C.c_void_p * n)(*[o.data_ptr() for o in outs]), (C.c_int * n)(*planes), n, h, w, H, W,
               _call.raw_stream(srcs[0].device), device=srcs[0].device)
    return outs


def fastest_placement(allocate, solve, tries: int = 3, keep_first: bool = False):
    """Pick, out of `tries` allocations of the same field buffers, the one the sweep streams fastest.

    Where a batch of fields lands in PHYSICAL memory moves the memory-bound sweep by up to 8 % (928 ...
    1 005 us for the same 6.3 GB, exactly reproducible per allocation, a property of the combination of the planes'
    pages that neither the virtual layout nor the library controls) -- only another allocation changes it.  A serving
    loop allocates its field buffers ONCE (the CNN head writes into them every batch) and can afford to choose:

        allocate() -> dict of device tensors (a candidate; all candidates are alive at the same time, hence on
                      different pages);   solve(fields) -> anything (one calibration of the candidate, e.g. an LMOptimizer)

    Every candidate is solved three times (warm-up, then the better of two timed with HIP events on the current stream); returns
    (fields_of_the_fastest, [milliseconds of every candidate]).  The others are dropped.  `keep_first`: a third value,
    the FIRST candidate's fields (what a caller who allocates once gets) -- measurement rigs report both.

    Round 4 tried to control the placement instead of choosing it (HIP virtual-memory management: one physical handle per
    batch / per tensor / per 2 MiB .. 1 GiB chunk, 1 GiB-aligned tensors): same spread, same discrete levels
    (profiles/archive/r04_vmm_placement.log) -- choosing among allocations stays the only handle a caller has."""
    if tries <= 1:
        f = allocate()
        return (f, [], f) if keep_first else (f, [])
    cands, times = [], []
    for _ in range(tries):
        f = allocate()
        solve(f)
        best_ms = float("inf")
        for _ in range(2):            # the better of two timed solves: the candidates differ by 1-4 %, one solve's jitter is ~0.5 %
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            solve(f)
            e1.record()
            e1.synchronize()
            best_ms = min(best_ms, e0.elapsed_time(e1))
        cands.append(f)
        times.append(best_ms)
    best = min(range(tries), key=times.__getitem__)
    return (cands[best], times, cands[0]) if keep_first else (cands[best], times)


def _rows(t: torch.Tensor, k: int, device) -> torch.Tensor:
    """`t` as the render calls read their cameras (k = 8) and rotations (k = 9): (n, k) float32 rows on `device`, contiguous,
    detached."""
    return t.detach().to(device=device, dtype=torch.float32).reshape(-1, k).contiguous()


def _rows_at(t: Optional[torch.Tensor], b0: int, n: int):
    """(pointer, batch) of rows `t` for the images [b0, b0 + n) of a call: one row shared by them all, or their slice of one
    row per image; None is (NULL, 1)."""
    if t is None:
        return None, 1
    rows = t if t.shape[0] == 1 else t[b0:b0 + n]
    return rows.data_ptr(), rows.shape[0]         # (the rows behind the pointer: a batch of neither kind is the entry's to refuse)


def _warp_image(img: torch.Tensor, size, who: str):
    """What the two image warps share, and the one place that knows dtypes and memory formats: the image as the kernels read
    it, the arguments its entry takes before the destination (the byte calls' layout flag; none for float32), the empty
    output of `size` in the kernels' layout, and what turns that output into the input's memory format (a channels_last byte
    image of more than 4 channels runs planar)."""
    if img.dtype == torch.float32:
        src = _call.dev_f32(img, "img")
        return src, (), src.new_empty(tuple(src.shape[:2]) + size), lambda t: t
    if img.dtype != torch.uint8:
        raise RuntimeError(f"geocalib_amd.{who} needs a float32 or uint8 image")
    src, interleaved = _call.dev_u8(img, "img")
    dst = torch.empty(tuple(src.shape[:2]) + size, dtype=torch.uint8, device=src.device,
                      memory_format=torch.channels_last if interleaved else torch.contiguous_format)
    if not img.is_contiguous() and img.is_contiguous(memory_format=torch.channels_last):
        return src, (interleaved,), dst, lambda t: t.contiguous(memory_format=torch.channels_last)
    return src, (interleaved,), dst, lambda t: t


def undistort_image(camera_model: str, cam: torch.Tensor, img: torch.Tensor, size) -> torch.Tensor:
    """gclm_undistort_image / gclm_undistort_image_u8: `img` (B, C, Hin, Win) float32 or uint8 on a HIP device, resampled to
    `size` = (H, W) at the distorted position of every output pixel of `cam` ((1, 8) shared by the batch, or (B, 8)), in one
    launch per 65 535 images on torch's current stream.  A uint8 image is contiguous or channels_last (read as it lies for
    C <= 4), and its uint8 output has its memory format.  BaseCamera.undistort_image is the public entry; not differentiable."""
    H, W = int(size[0]), int(size[1])
    src, layout, dst, like_input = _warp_image(img, (H, W), "undistort_image")
    cam = _rows(cam, 8, src.device)
    B, C, Hin, Win = src.shape
    if dst.numel() == 0:
        return dst
    for b0, n in _call.slices(B):
        _call.call("gclm_undistort_image_u8" if src.dtype == torch.uint8 else "gclm_undistort_image",
                   _lib.CAMERA_MODEL_IDS[camera_model], *_rows_at(cam, b0, n), src[b0].data_ptr(), n, C, Hin, Win, H, W, *layout,
                   dst[b0].data_ptr(), _call.raw_stream(src.device), device=src.device)
    return like_input(dst)


def reproject_image(src_model: str, src_cam: torch.Tensor, dst_model: str, dst_cam: torch.Tensor, rot: Optional[torch.Tensor],
                    img: torch.Tensor, src_size, size, return_valid: bool = False):
    """gclm_reproject_image / gclm_reproject_image_u8: `img` (B, C, Hin, Win) float32 or uint8 on a HIP device, taken with
    `src_cam` of nominal `src_size` = (Hs, Ws), as `dst_cam` of `size` = (H, W) sees it after the rotation `rot` ((1 or B, 3,
    3), or None for the identity), in one launch per 65 535 images on torch's current stream.  The cameras are (1, 8) shared
    by the batch or (B, 8), both of one batch.  Returns (B, C, H, W), and with `return_valid` the (B, H, W) bool mask of the
    pixels that see the source.  A uint8 image is contiguous or channels_last (read as it lies for C <= 4), and its uint8
    output has its memory format.  BaseCamera.reproject_image is the public entry; not differentiable."""
    (Hs, Ws), (H, W) = (int(v) for v in src_size), (int(v) for v in size)
    src, layout, dst, like_input = _warp_image(img, (H, W), "reproject_image")
    dev, (B, C, Hin, Win) = src.device, src.shape
    src_cam, dst_cam, rot = _rows(src_cam, 8, dev), _rows(dst_cam, 8, dev), None if rot is None else _rows(rot, 9, dev)
    if src_cam.shape[0] != dst_cam.shape[0] or src_cam.shape[0] not in (1, B) or (rot is not None and rot.shape[0] not in (1, B)):
        raise ValueError(f"camera batches {src_cam.shape[0]} and {dst_cam.shape[0]} must be equal and, as the rotation batch "
                         f"{None if rot is None else rot.shape[0]}, 1 or {B}")
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=src.device) if return_valid else None
    if dst.numel() > 0:
        for b0, n in _call.slices(B):
            _call.call("gclm_reproject_image_u8" if src.dtype == torch.uint8 else "gclm_reproject_image",
                       _lib.CAMERA_MODEL_IDS[src_model], _rows_at(src_cam, b0, n)[0], _lib.CAMERA_MODEL_IDS[dst_model],
                       *_rows_at(dst_cam, b0, n), *_rows_at(rot, b0, n), src[b0].data_ptr(), n, C, Hin, Win, Hs, Ws, H, W, *layout,
                       dst[b0].data_ptr(), _call.ptr_at(valid, b0), _call.raw_stream(src.device), device=src.device)
    elif valid is not None:
        valid.zero_()
    dst = like_input(dst)
    return (dst, valid.bool()) if return_valid else dst


def render_from_pano(camera_model: str, cam: torch.Tensor, rot: torch.Tensor, panos, size) -> torch.Tensor:
    """gclm_render_from_pano: n images of `size` = (H, W) rendered from equirectangular panoramas, on torch's current stream.

    `cam` is (1, 8) shared by the batch or (n, 8); `rot` is (n, 3, 3), R_i = gravity.R[i] @ rad2rotmat(0, 0, yaw_i); `panos`
    is a sequence of n float32 (C, Hs, Ws) HIP device tensors, one per image (the same tensor may repeat).
    BaseCamera.get_img_from_pano is the public entry; not differentiable."""
    n = len(panos)
    if n == 0 or any(p.dtype != torch.float32 or p.dim() != 3 for p in panos):
        raise RuntimeError("geocalib_amd.render_from_pano needs float32 (C, H, W) panoramas")
    panos = [_call.dev_f32(p, "panos") for p in panos]
    dev, C = panos[0].device, panos[0].shape[0]
    if any(p.device != dev or p.shape[0] != C for p in panos):
        raise ValueError("every panorama must live on one device and carry the same number of channels")
    H, W = int(size[0]), int(size[1])
    cam, rot = _rows(cam, 8, dev), _rows(rot, 9, dev)
    if cam.shape[0] not in (1, n) or rot.shape[0] != n:
        raise ValueError(f"camera batch {cam.shape[0]} must be 1 or {n}, rotations {rot.shape[0]} must be {n}")
    dst = torch.empty((n, C, H, W), device=dev, dtype=torch.float32)
    if dst.numel() == 0:
        return dst
    for i0, m in _call.slices(n):
        srcs = (ctypes.c_void_p * m)(*(p.data_ptr() for p in panos[i0:i0 + m]))
        hw = (ctypes.c_int * (2 * m))(*(v for p in panos[i0:i0 + m] for v in p.shape[1:]))
        _call.call("gclm_render_from_pano", _lib.CAMERA_MODEL_IDS[camera_model], *_rows_at(cam, i0, m), rot[i0].data_ptr(),
                   srcs, hw, m, C, H, W, dst[i0].data_ptr(), _call.raw_stream(dev), device=dev)
    return dst


def perspective_fields(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, size, up: bool = True, latitude: bool = True,
                       normalize: bool = True):
    """gclm_perspective_fields: the up field (B, H, W, 2) and the latitude field (B, H, W, 1) of `size` = (H, W) for cameras
    `cam` (B, 8) and gravities `grav` (B, 3), float32 on one HIP device, in one launch per 65 535 images on torch's current
    stream.  A field not asked for is returned as None.  get_perspective_field and friends are the public entries; not
    differentiable here (their calibration_grad=True wraps this call and perspective_fields_backward in a Function).  simple_divisional's distort scale and its derivative take the forms that do not cancel in float32
    (include/gclm.h), where the torch composition keeps the reference's."""
    assert up or latitude, "at least one of up or latitude must be True"
    if not (cam.dtype == grav.dtype == torch.float32 and grav.device == cam.device):
        raise RuntimeError("geocalib_amd.perspective_fields needs float32 cameras and gravities on one device")
    cam, grav = _call.dev_f32(cam, "cam").reshape(-1, 8), _call.dev_f32(grav, "grav").reshape(-1, 3)
    if cam.shape[0] != grav.shape[0]:
        raise ValueError(f"camera batch {cam.shape[0]} and gravity batch {grav.shape[0]} must be equal")
    B, H, W = cam.shape[0], int(size[0]), int(size[1])
    u = cam.new_empty((B, H, W, 2)) if up else None
    lat = cam.new_empty((B, H, W, 1)) if latitude else None
    if B * H * W == 0:
        return u, lat
    for b0, n in _call.slices(B):
        _call.call("gclm_perspective_fields", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n, H, W,
                   int(normalize), None if u is None else u[b0].data_ptr(), None if lat is None else lat[b0].data_ptr(),
                   _call.raw_stream(cam.device), device=cam.device)
    return u, lat


def _field_planes(planes, B: int, dev):
    """The predicted planes of a scoring call as its kernel reads them (None stays None; kept in the order given, which is
    the order of the C arguments), and their (H, W): "up" holds two
    planes per image, every other one, and all lie on `dev` at the size of the latitude field (of the up field without it)."""
    planes = {k: None if t is None else _call.dev_f32(t, k) for k, t in planes.items()}
    H, W = (planes["up"] if planes["lat"] is None else planes["lat"]).shape[-2:]
    for k, t in planes.items():
        want = B * H * W * (2 if k == "up" else 1)
        if t is not None and (t.numel() != want or t.shape[-2:] != (H, W) or t.device != dev):
            raise ValueError(f"`{k}` {tuple(t.shape)} on {t.device} does not fit {B} images of {H} x {W} on {dev}")
    return planes, H, W


def field_errors(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, up: Optional[torch.Tensor] = None,
                 lat: Optional[torch.Tensor] = None, up_conf: Optional[torch.Tensor] = None,
                 lat_conf: Optional[torch.Tensor] = None, thresholds=(1.0, 3.0, 5.0, 10.0), return_errors: bool = False):
    """gclm_field_errors: predicted fields `up` (B, 2, H, W) / `lat` (B, 1, H, W) (one may be None) and their confidences
    (B, H, W) scored against the fields of cameras `cam` (B, 8) and gravities `grav` (B, 3), float32 on one HIP device, in one
    pass per 65 535 images on torch's current stream.  Returns (stats, up_error, latitude_error): stats (B, 2 (2 + n)) as
    include/gclm.h lays them out -- [mean, weighted, recall@t.. ] of up, then of latitude, NaN where a plane is absent -- and
    with `return_errors` the per-pixel errors in degrees (B, H, W) of the fields given, else None.
    metrics.perspective_field_metrics is the public entry; not differentiable."""
    if up is None and lat is None:
        raise ValueError("at least one of the up and latitude fields is needed")
    if (up is None and up_conf is not None) or (lat is None and lat_conf is not None):
        raise ValueError("a confidence needs its field")
    cam, grav = _call.dev_f32(cam, "cam").reshape(-1, 8), _call.dev_f32(grav, "grav").reshape(-1, 3)
    dev, B = cam.device, cam.shape[0]
    planes, H, W = _field_planes({"up": up, "lat": lat, "up_conf": up_conf, "lat_conf": lat_conf}, B, dev)
    if grav.shape[0] != B or grav.device != dev:
        raise ValueError(f"camera batch {B} and gravity batch {grav.shape[0]} must be equal and on one device")
    thr = [float(t) for t in thresholds]
    S = 2 * (2 + len(thr))
    stats = cam.new_empty((B, S))
    up_err = cam.new_empty((B, H, W)) if return_errors and up is not None else None
    lat_err = cam.new_empty((B, H, W)) if return_errors and lat is not None else None
    if B * H * W == 0:
        return stats.fill_(float("nan")), up_err, lat_err
    lib = _lib.load()
    ws_bytes = int(lib.gclm_field_errors_workspace(min(B, _call.MAX_CALL), H, W, len(thr)))
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=dev)
    c_thr = (_lib.C.c_float * len(thr))(*thr)
    for b0, n in _call.slices(B):
        _call.call("gclm_field_errors", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n, H, W,
                   *(_call.ptr_at(t, b0) for t in planes.values()), len(thr), c_thr, ws.data_ptr(), ws_bytes, stats[b0].data_ptr(),
                   _call.ptr_at(up_err, b0), _call.ptr_at(lat_err, b0), _call.raw_stream(dev), device=dev)
    return stats, up_err, lat_err


def _loss_call(who: str, cam, grav, up, lat, up_conf, lat_conf, up_loss: str, lat_loss: str):
    """What field_loss and field_loss_grad share: the checked inputs as their kernels read them -- (cam, grav, planes, B, H, W,
    loss ids)."""
    if up is None and lat is None:
        raise ValueError("at least one of the up and latitude fields is needed")
    if (up is None and up_conf is not None) or (lat is None and lat_conf is not None):
        raise ValueError("a confidence needs its field")
    if up_loss not in _lib.FIELD_LOSS_IDS or lat_loss not in _lib.FIELD_LOSS_IDS or lat_loss == "dot":
        raise ValueError(f"{who}: loss types are {sorted(_lib.FIELD_LOSS_IDS)} ('dot' for the up field only), got {up_loss!r} and "
                         f"{lat_loss!r}")
    cam, grav = _call.dev_f32(cam, "cam").reshape(-1, 8), _call.dev_f32(grav, "grav").reshape(-1, 3)
    dev, B = cam.device, cam.shape[0]
    planes, H, W = _field_planes({"up": up, "lat": lat, "up_conf": up_conf, "lat_conf": lat_conf}, B, dev)
    if grav.shape[0] != B or grav.device != dev:
        raise ValueError(f"camera batch {B} and gravity batch {grav.shape[0]} must be equal and on one device")
    return cam, grav, planes, B, H, W, (_lib.FIELD_LOSS_IDS[up_loss], _lib.FIELD_LOSS_IDS[lat_loss])


def field_loss(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, up: Optional[torch.Tensor] = None,
               lat: Optional[torch.Tensor] = None, up_conf: Optional[torch.Tensor] = None,
               lat_conf: Optional[torch.Tensor] = None, up_loss: str = "l1", lat_loss: str = "l1") -> torch.Tensor:
    """gclm_field_loss: the decoders' training losses of predicted fields `up` (B, 2, H, W) / `lat` (B, 1, H, W) (one may be
    None) against the fields of cameras `cam` (B, 8) and gravities `grav` (B, 3), float32 on one HIP device, in one pass per
    65 535 images on torch's current stream.  A confidence (B, H, W) weights its field's loss; None is the plain mean.
    Returns (B, 4) as include/gclm.h lays it out: [up loss, latitude loss, up denominator, latitude denominator], NaN for an
    absent field, no loss weight applied.  losses.perspective_field_loss is the public entry."""
    cam, grav, planes, B, H, W, ids = _loss_call("field_loss", cam, grav, up, lat, up_conf, lat_conf, up_loss, lat_loss)
    dev = cam.device
    out = cam.new_empty((B, 4))
    if B * H * W == 0:
        return out.fill_(float("nan"))
    ws_bytes = int(_lib.load().gclm_field_loss_workspace(min(B, _call.MAX_CALL), H, W))
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=dev)
    for b0, n in _call.slices(B):
        _call.call("gclm_field_loss", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n, H, W,
                   *(_call.ptr_at(t, b0) for t in planes.values()), *ids, ws.data_ptr(), ws_bytes, out[b0].data_ptr(),
                   _call.raw_stream(dev), device=dev)
    return out


def field_loss_grad(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, scale: torch.Tensor,
                    up: Optional[torch.Tensor] = None, lat: Optional[torch.Tensor] = None, up_conf: Optional[torch.Tensor] = None,
                    lat_conf: Optional[torch.Tensor] = None, up_loss: str = "l1", lat_loss: str = "l1"):
    """gclm_field_loss_grad: the gradients of field_loss's two losses with respect to the fields given, (grad_up (B, 2, H, W),
    grad_lat (B, 1, H, W)), None for an absent field: `scale` (B, 2) = [up, latitude] (grad_output x weight / denominator, on
    the device) times the per-pixel derivative, times the confidence where given.  The target is evaluated again in
    registers; one launch per 65 535 images on torch's current stream."""
    cam, grav, planes, B, H, W, ids = _loss_call("field_loss_grad", cam, grav, up, lat, up_conf, lat_conf, up_loss, lat_loss)
    dev = cam.device
    scale = _call.dev_f32(scale, "scale")
    if scale.shape != (B, 2) or scale.device != dev:
        raise ValueError(f"`scale` {tuple(scale.shape)} on {scale.device} must be ({B}, 2) on {dev}")
    g_up = None if planes["up"] is None else torch.empty_like(planes["up"])
    g_lat = None if planes["lat"] is None else torch.empty_like(planes["lat"])
    if B * H * W == 0:
        return g_up, g_lat
    for b0, n in _call.slices(B):
        _call.call("gclm_field_loss_grad", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n, H, W,
                   *(_call.ptr_at(t, b0) for t in planes.values()), *ids, scale[b0].data_ptr(), _call.ptr_at(g_up, b0),
                   _call.ptr_at(g_lat, b0), _call.raw_stream(dev), device=dev)
    return g_up, g_lat


def _bin_loss_call(who: str, up_logits, lat_logits, up_conf, lat_conf):
    """What bin_loss and bin_loss_grad share: the checked logits and confidences as their kernels read them -- (logits,
    confidences, B, H, W, device, gclm_logit_dtype).  The logits are taken as they lie (contiguous, one of the three dtypes, one
    device); a confidence is float32 (B, H, W)."""
    given = [t for t in (up_logits, lat_logits) if t is not None]
    if not given:
        raise ValueError(f"{who}: at least one of the up and latitude logits is needed")
    if (up_logits is None and up_conf is not None) or (lat_logits is None and lat_conf is not None):
        raise ValueError(f"{who}: a confidence needs its logits")
    first = given[0]
    for t in given:
        if t.dim() != 4 or t.dtype not in _LOGIT_DTYPES or t.dtype != first.dtype or t.device != first.device or \
                t.shape[0] != first.shape[0] or t.shape[-2:] != first.shape[-2:] or not t.is_contiguous():
            raise ValueError(f"{who}: logits are contiguous (B, bins, H, W) float32, float16 or bfloat16 tensors of one dtype, device, "
                             f"B, H and W, got {[(tuple(t.shape), t.dtype, str(t.device)) for t in given]}")
        _call.require_device(t, "logits")
    B, (H, W), dev = first.shape[0], first.shape[-2:], first.device
    if up_logits is not None and not 2 <= up_logits.shape[1] <= _lib.MAX_BINS or \
            lat_logits is not None and not 1 <= lat_logits.shape[1] <= _lib.MAX_BINS:
        raise ValueError(f"{who}: 2..{_lib.MAX_BINS} up bins and 1..{_lib.MAX_BINS} latitude bins, got "
                         f"{[t.shape[1] for t in given]}")
    confs = []
    for name, c in (("up_conf", up_conf), ("lat_conf", lat_conf)):
        if c is not None:
            c = _call.dev_f32(c, name)
            if c.numel() != B * H * W or c.shape[-2:] != (H, W) or c.device != dev:
                raise ValueError(f"{who}: `{name}` {tuple(c.shape)} on {c.device} does not fit {B} images of {H} x {W} on {dev}")
        confs.append(c)
    logits = [None if t is None else t.detach() for t in (up_logits, lat_logits)]
    return logits, confs, B, H, W, dev, _LOGIT_DTYPES[first.dtype]


def bin_loss(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, up_logits: Optional[torch.Tensor] = None,
             lat_logits: Optional[torch.Tensor] = None, up_conf: Optional[torch.Tensor] = None,
             lat_conf: Optional[torch.Tensor] = None):
    """gclm_bin_loss: the cross-entropy of classification-head logits `up_logits` (B, Ku, H, W) / `lat_logits` (B, Kl, H, W) (one
    may be None; float32, float16 or bfloat16, contiguous) against the bins of the fields of cameras `cam` (B, 8) and gravities
    `grav` (B, 3), float32, all on one HIP device, in one pass per 65 535 images on torch's current stream.  A confidence
    (B, H, W) weights its head's pixels; None is the plain mean.  Returns (out, lse, bins) as include/gclm.h lays them out: out
    (B, 6) = [numerator, denominator, hits] of up, then of latitude (NaN for an absent head), lse (B, 2, H, W) float32 and bins
    (B, 2, H, W) int16, which bin_loss_grad takes.  losses.perspective_bin_loss is the public entry."""
    logits, confs, B, H, W, dev, dtype = _bin_loss_call("bin_loss", up_logits, lat_logits, up_conf, lat_conf)
    cam, grav = _call.dev_f32(cam, "cam").reshape(-1, 8), _call.dev_f32(grav, "grav").reshape(-1, 3)
    if cam.shape[0] != B or grav.shape[0] != B or cam.device != dev or grav.device != dev:
        raise ValueError(f"camera batch {cam.shape[0]} on {cam.device} and gravity batch {grav.shape[0]} on {grav.device} must be {B} "
                         f"on {dev}")
    out = cam.new_empty((B, 6))
    lse = cam.new_empty((B, 2, H, W))
    bins = torch.empty((B, 2, H, W), dtype=torch.int16, device=dev)
    if B * H * W == 0:
        return out.fill_(float("nan")), lse, bins
    counts = [0 if t is None else t.shape[1] for t in logits]
    ws_bytes = int(_lib.load().gclm_bin_loss_workspace(min(B, _call.MAX_CALL), H, W))
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=dev)
    for b0, n in _call.slices(B):
        _call.call("gclm_bin_loss", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n, H, W,
                   _call.ptr_at(logits[0], b0), counts[0], _call.ptr_at(logits[1], b0), counts[1], dtype,
                   _call.ptr_at(confs[0], b0), _call.ptr_at(confs[1], b0), ws.data_ptr(), ws_bytes, out[b0].data_ptr(),
                   lse[b0].data_ptr(), bins[b0].data_ptr(), _call.raw_stream(dev), device=dev)
    return out, lse, bins


def bin_loss_grad(scale: torch.Tensor, lse: torch.Tensor, bins: torch.Tensor, up_logits: Optional[torch.Tensor] = None,
                  lat_logits: Optional[torch.Tensor] = None, up_conf: Optional[torch.Tensor] = None,
                  lat_conf: Optional[torch.Tensor] = None):
    """gclm_bin_loss_grad: the gradients of bin_loss's two losses with respect to the logits given, (grad_up (B, Ku, H, W),
    grad_lat (B, Kl, H, W)) in the logits' dtype, None for an absent head: `scale` (B, 2) = [up, latitude] (grad_output x weight
    / denominator, on the device) times softmax(z) - onehot(bin), times the confidence where given, with `lse` and `bins` as
    bin_loss returned them.  One launch per 65 535 images on torch's current stream."""
    logits, confs, B, H, W, dev, dtype = _bin_loss_call("bin_loss_grad", up_logits, lat_logits, up_conf, lat_conf)
    scale = _call.dev_f32(scale, "scale")
    if scale.shape != (B, 2) or scale.device != dev:
        raise ValueError(f"`scale` {tuple(scale.shape)} on {scale.device} must be ({B}, 2) on {dev}")
    if lse.shape != (B, 2, H, W) or lse.dtype != torch.float32 or bins.shape != (B, 2, H, W) or bins.dtype != torch.int16 or \
            lse.device != dev or bins.device != dev or not (lse.is_contiguous() and bins.is_contiguous()):
        raise ValueError(f"`lse` and `bins` are bin_loss's: contiguous ({B}, 2, {H}, {W}) float32 and int16 on {dev}")
    grads = [None if t is None else torch.empty_like(t) for t in logits]
    if B * H * W == 0:
        return tuple(grads)
    counts = [0 if t is None else t.shape[1] for t in logits]
    for b0, n in _call.slices(B):
        _call.call("gclm_bin_loss_grad", _call.ptr_at(logits[0], b0), counts[0], _call.ptr_at(logits[1], b0), counts[1], dtype,
                   _call.ptr_at(confs[0], b0), _call.ptr_at(confs[1], b0), n, H, W, lse[b0].data_ptr(), bins[b0].data_ptr(),
                   scale[b0].data_ptr(), _call.ptr_at(grads[0], b0), _call.ptr_at(grads[1], b0), _call.raw_stream(dev), device=dev)
    return tuple(grads)


def _param_grad_outputs(cam: torch.Tensor, B: int, want_cam: bool, want_grav: bool):
    if not (want_cam or want_grav):
        raise ValueError("at least one of the camera and gravity gradients must be asked for")
    return (cam.new_empty((B, 8)) if want_cam else None), (cam.new_empty((B, 3)) if want_grav else None)


def _param_grad_workspace(B: int, H: int, W: int, dev):
    ws_bytes = int(_lib.load().gclm_field_param_grad_workspace(min(B, _call.MAX_CALL), H, W))
    return torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=dev), ws_bytes


def field_loss_param_grad(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, scale: torch.Tensor,
                          up: Optional[torch.Tensor] = None, lat: Optional[torch.Tensor] = None,
                          up_conf: Optional[torch.Tensor] = None, lat_conf: Optional[torch.Tensor] = None, up_loss: str = "l1",
                          lat_loss: str = "l1", want_cam: bool = True, want_grav: bool = True):
    """gclm_field_loss_param_grad: the gradients of field_loss's two losses with respect to the calibration, (grad_cam (B, 8),
    grad_grav (B, 3)), None for the one not asked for: the inputs and `scale` (B, 2) of field_loss_grad, the target evaluated
    again in registers and its cotangent pulled back to the camera row (columns w, h zero) and the gravity as stored; two
    launches per 65 535 images on torch's current stream.  An image's gradients do not depend on which of the two is asked for."""
    cam, grav, planes, B, H, W, ids = _loss_call("field_loss_param_grad", cam, grav, up, lat, up_conf, lat_conf, up_loss, lat_loss)
    dev = cam.device
    scale = _call.dev_f32(scale, "scale")
    if scale.shape != (B, 2) or scale.device != dev:
        raise ValueError(f"`scale` {tuple(scale.shape)} on {scale.device} must be ({B}, 2) on {dev}")
    g_cam, g_grav = _param_grad_outputs(cam, B, want_cam, want_grav)
    if B * H * W == 0:
        return (None if g_cam is None else g_cam.zero_()), (None if g_grav is None else g_grav.zero_())
    ws, ws_bytes = _param_grad_workspace(B, H, W, dev)
    for b0, n in _call.slices(B):
        _call.call("gclm_field_loss_param_grad", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n, H, W,
                   *(_call.ptr_at(t, b0) for t in planes.values()), *ids, scale[b0].data_ptr(), ws.data_ptr(), ws_bytes,
                   _call.ptr_at(g_cam, b0), _call.ptr_at(g_grav, b0), _call.raw_stream(dev), device=dev)
    return g_cam, g_grav


def perspective_fields_backward(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, grad_up: Optional[torch.Tensor] = None,
                                grad_lat: Optional[torch.Tensor] = None, normalize: bool = True, want_cam: bool = True,
                                want_grav: bool = True):
    """gclm_perspective_fields_backward: the cotangents of perspective_fields' outputs, `grad_up` (B, H, W, 2) / `grad_lat`
    (B, H, W, 1) or (B, H, W) (one may be None), pulled back to the cameras `cam` (B, 8) and gravities `grav` (B, 3) they were
    rendered at: (grad_cam (B, 8), grad_grav (B, 3)), None for the one not asked for.  float32 on one HIP device; two launches
    per 65 535 images on torch's current stream."""
    if grad_up is None and grad_lat is None:
        raise ValueError("at least one of the up and latitude cotangents is needed")
    cam, grav = _call.dev_f32(cam, "cam").reshape(-1, 8), _call.dev_f32(grav, "grav").reshape(-1, 3)
    dev, B = cam.device, cam.shape[0]
    if grav.shape[0] != B or grav.device != dev:
        raise ValueError(f"camera batch {B} and gravity batch {grav.shape[0]} must be equal and on one device")
    grad_up = None if grad_up is None else _call.dev_f32(grad_up, "grad_up")
    grad_lat = None if grad_lat is None else _call.dev_f32(grad_lat, "grad_lat")
    if grad_up is not None and (grad_up.dim() != 4 or grad_up.shape[0] != B or grad_up.shape[3] != 2 or grad_up.device != dev):
        raise ValueError(f"`grad_up` {tuple(grad_up.shape)} on {grad_up.device} must be ({B}, H, W, 2) on {dev}")
    H, W = (grad_up.shape[1:3] if grad_up is not None else grad_lat.shape[1:3])
    if grad_lat is not None and (grad_lat.dim() not in (3, 4) or grad_lat.numel() != B * H * W or grad_lat.shape[:3] != (B, H, W)
                                 or grad_lat.device != dev):
        raise ValueError(f"`grad_lat` {tuple(grad_lat.shape)} on {grad_lat.device} must be ({B}, {H}, {W}[, 1]) on {dev}")
    g_cam, g_grav = _param_grad_outputs(cam, B, want_cam, want_grav)
    if B * H * W == 0:
        return (None if g_cam is None else g_cam.zero_()), (None if g_grav is None else g_grav.zero_())
    ws, ws_bytes = _param_grad_workspace(B, H, W, dev)
    for b0, n in _call.slices(B):
        _call.call("gclm_perspective_fields_backward", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n,
                   H, W, int(normalize), _call.ptr_at(grad_up, b0), _call.ptr_at(grad_lat, b0), ws.data_ptr(), ws_bytes,
                   _call.ptr_at(g_cam, b0), _call.ptr_at(g_grav, b0), _call.raw_stream(dev), device=dev)
    return g_cam, g_grav


HYPOTHESIS_CHUNK = _lib.HYPOTHESIS_CHUNK     # K: hypotheses scored per read of an image's planes (GCLM_HYPOTHESIS_CHUNK)


def hypothesis_scores(camera_model: str, cam: torch.Tensor, grav: torch.Tensor, up: Optional[torch.Tensor] = None,
                      lat: Optional[torch.Tensor] = None, up_conf: Optional[torch.Tensor] = None,
                      lat_conf: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, up_threshold: float = 1.0,
                      lat_threshold: float = 1.0, up_weight: float = 1.0, lat_weight: float = 1.0):
    """gclm_hypothesis_scores: N candidate calibrations per image, cameras `cam` (B, N, 8) and gravities `grav` (B, N, 3),
    scored against the image's predicted fields `up` (B, 2, H, W) / `lat` (B, 1, H, W) (one may be None), their confidences
    and an optional `mask` (B, H, W), float32 on one HIP device, in one pass per 65 535 images on torch's current stream.
    Returns (scores, best): scores (B, N, 3) = [up, lat, total] -- the confidence-weighted sums of the pixels whose error
    lies strictly below the field's threshold (degrees), and their weighted sum -- and best (B,) int32, the first index of
    each image's largest total.  metrics.rank_calibrations is the public entry; not differentiable."""
    if up is None and lat is None:
        raise ValueError("at least one of the up and latitude fields is needed")
    if (up is None and up_conf is not None) or (lat is None and lat_conf is not None):
        raise ValueError("a confidence needs its field")
    cam, grav = _call.dev_f32(cam, "cam"), _call.dev_f32(grav, "grav")
    if cam.dim() != 3 or grav.dim() != 3 or cam.shape[2] != 8 or grav.shape[2] != 3 or cam.shape[:2] != grav.shape[:2] \
            or grav.device != cam.device:
        raise ValueError(f"cameras {tuple(cam.shape)} and gravities {tuple(grav.shape)} must be (B, N, 8) and (B, N, 3) on one device")
    dev, (B, N) = cam.device, cam.shape[:2]
    planes, H, W = _field_planes({"up": up, "lat": lat, "up_conf": up_conf, "lat_conf": lat_conf, "mask": mask}, B, dev)
    scores = cam.new_empty((B, N, 3))
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    if B * N == 0 or H * W == 0:
        return scores.zero_(), best.zero_()
    if N > _call.MAX_CALL:
        raise ValueError(f"at most {_call.MAX_CALL} hypotheses per image and call (got {N})")
    lib = _lib.load()
    ws_bytes = int(lib.gclm_hypothesis_scores_workspace(min(B, _call.MAX_CALL), N, H, W))
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=dev)
    for b0, n in _call.slices(B):
        _call.call("gclm_hypothesis_scores", _lib.CAMERA_MODEL_IDS[camera_model], cam[b0].data_ptr(), grav[b0].data_ptr(), n, N, H, W,
                   *(_call.ptr_at(t, b0) for t in planes.values()), float(up_threshold), float(lat_threshold), float(up_weight),
                   float(lat_weight), ws.data_ptr(), ws_bytes, scores[b0].data_ptr(), best[b0].data_ptr(), _call.raw_stream(dev),
                   device=dev)
    return scores, best


def rpf_hypotheses(up: torch.Tensor, lat: Optional[torch.Tensor] = None, prior_focal: Optional[torch.Tensor] = None,
                   samples: Optional[torch.Tensor] = None, n: int = 1000, seed: int = 0, first_index: int = 0):
    """gclm_rpf_hypotheses: the three-pixel minimal solver on `up` (B, 2, H, W) and `lat` (B, 1, H, W) -- or `prior_focal`
    (B,) in its place --, float32 on one HIP device, one launch per 65 535 images on torch's current stream.  `samples`
    (B, N, 3, 2) int32 pixels (x, y) on the same device, or None: `n` per image are drawn in the kernel from (seed,
    first_index + b, sample, pixel).  Returns (cam (B, N Rn, 8), grav (B, N Rn, 3), samples (B, N, 3, 2) as used), Rn = 1 with
    a prior focal and 2 without; invalid rows are NaN.  ransac.solve_rpf is the public entry; not differentiable."""
    if lat is None and prior_focal is None:
        raise ValueError("the focal length needs the latitude field or a prior focal")
    up = _call.dev_f32(up, "up")
    dev, (B, _, H, W) = up.device, up.shape
    lat = None if lat is None or prior_focal is not None else _call.dev_f32(lat, "lat")
    prior = None if prior_focal is None else _call.dev_f32(prior_focal, "prior_focal").reshape(-1)
    if up.shape[1] != 2 or (lat is not None and (lat.numel() != B * H * W or lat.device != dev)) or \
            (prior is not None and (prior.numel() != B or prior.device != dev)):
        raise ValueError(f"`up` {tuple(up.shape)} must be (B, 2, H, W), with `lat` of B H W or `prior_focal` of B values on {dev}")
    if samples is not None:
        _call.require_device(samples, "samples")
        if samples.dtype != torch.int32 or samples.shape[0] != B or samples.shape[2:] != (3, 2) or samples.device != dev:
            raise ValueError(f"`samples` {tuple(samples.shape)} {samples.dtype} must be (B, N, 3, 2) int32 on {dev}")
        samples, n = samples.contiguous(), samples.shape[1]
    n, Rn = int(n), 1 if prior is not None else 2
    if not 1 <= n <= _lib.RPF_MAX_SAMPLES:
        raise ValueError(f"samples per image must lie in 1..{_lib.RPF_MAX_SAMPLES} (got {n})")
    cam, grav = up.new_empty((B, n * Rn, 8)), up.new_empty((B, n * Rn, 3))
    drawn = torch.empty((B, n, 3, 2), dtype=torch.int32, device=dev) if samples is None else None
    for b0, m in _call.slices(B):
        _call.call("gclm_rpf_hypotheses", up[b0].data_ptr(), _call.ptr_at(lat, b0), _call.ptr_at(prior, b0),
                   _call.ptr_at(samples, b0), int(seed) & (2 ** 64 - 1), int(first_index) + b0, m, n, H, W, cam[b0].data_ptr(),
                   grav[b0].data_ptr(), _call.ptr_at(drawn, b0), _call.raw_stream(dev), device=dev)
    return cam, grav, samples if samples is not None else drawn
