"""Gate of the uint8 image calls (gclm_undistort_image_u8, gclm_reproject_image_u8; Camera.undistort_image / reproject_image /
upright_image on torch.uint8), shared by the CPU self-check (test_u8_image_abi.py) and the GPU tests (test_u8_image.py).

No new yardstick: tests/undistort_gate.py and tests/reproject_gate.py take the source image as an argument and are fed the
byte image as float64 values 0..255, so their L (largest neighbour difference) and A (largest magnitude) scale by
themselves.  A byte output is the float call's sample rounded to nearest, which adds at most half a step of the quantiser:
    |out - ref| <= bound + 0.5,      bound = L * delta + 4 ulp(A) of the float gates, inf on their excluded pixels.
Where the float gate is 0 (no tap in the source, invisible, folded) this asks for |out| <= 0.5: the byte must be 0.

The byte images are the gates' own float images, (make_images(...) * 255).round(), clamped to 0..255: the "smooth" kind
spans -1..1, its negative half becomes flat 0 (and exercises nothing less: the positive half keeps its gradients)."""
import torch

import reproject_gate as rg
import undistort_gate as ug

HALF = 0.5                      # half a step of the quantiser


def to_bytes(img32):
    """A gate image (float32, nominally 0..1) as the uint8 image the byte calls are given."""
    return (img32 * 255).round().clamp(0, 255).to(torch.uint8)


def quantise(out32):
    """The definition's last step on a float32 sample: nearest, ties to even (torch.round), saturated."""
    return out32.round().clamp(0, 255).to(torch.uint8)


def worst_ratio(out, ref, bound):
    """max |out - ref| / (bound + 0.5) over the pixels whose bound is finite (the others are excluded by the float gate)."""
    keep = torch.isfinite(bound)
    if not keep.any():
        return 0.0
    return ((out.double() - ref).abs()[keep] / (bound[keep] + HALF)).max().item()


def reproject_parts(case):
    """rg.case_parts of one case of rg.CASES for its byte image: inputs, float64 yardstick, float32 restatement, delta, ref,
    bound and the mask parts, on the CPU; "img" is the uint8 image."""
    sm, tm, H, W = case[0], case[4], case[10], case[11]
    src, tgt, rot, img = rg.case_inputs(case)
    img = to_bytes(img)
    geo = (sm, src, tm, tgt, rot, H, W, rg.HS, rg.WS, rg.HIN, rg.WIN)
    c64, c32 = rg.coordinates(*geo), rg.coordinates(*geo, dtype=torch.float32)
    ex = rg.excluded(c64, sm)
    delta = rg.coordinate_bound(c64, c32, ex, rg.HIN, rg.WIN)
    ref, bound = rg.reference(img.double(), c64, ex, delta)
    return {"src": src, "tgt": tgt, "rot": rot, "img": img, "c64": c64, "c32": c32, "ex": ex, "delta": delta, "ref": ref,
            "bound": bound, "valid": rg.in_image(c64, rg.HIN, rg.WIN).expand(rg.B, -1, -1),
            "mask_free": (ex | rg.edge_band(c64, rg.HIN, rg.WIN, delta)).expand(rg.B, -1, -1)}


def undistort_parts(case, device="cpu"):
    """One case of ug.CASES for its byte image: cameras, the uint8 image (CPU), and on `device` the float64 yardstick `ref`
    and `bound` (delta is always derived on the CPU: it must not depend on the device under test)."""
    model, k1, k2, B, nb, C, H, W, Hin, Win, kind = case
    cams, img = ug.case_inputs(case)
    img = to_bytes(img)
    delta = ug.coordinate_bound(model, cams, H, W, Hin, Win)
    ix, iy = ug.coordinates(model, cams, H, W, Hin, Win, device=device)
    src64 = img.to(device=device, dtype=torch.float64)
    return {"cams": cams, "img": img, "delta": delta, "ref": ug.grid_sample64(src64, ix, iy), "bound": ug.gate(src64, ix, iy, delta)}


def undistort_id(case):
    return f"{case[0]}-{case[1]}-B{case[3]}-nb{case[4]}-C{case[5]}-{case[8]}x{case[9]}-{case[-1]}"
