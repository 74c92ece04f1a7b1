"""Perspective fields as classification bins: the other output format of the reference's up and latitude decoders
(siclib/models/decoders/up_decoder.py, latitude_decoder.py with loss_type == "classification"; the arithmetic is
siclib/models/utils/perspective_encoding.py).  It is the format of the original PerspectiveFields weights: the up head emits
one logit per 5-degree direction plus an "invalid" class (73 in all), the latitude head one per degree (180), and the fields
are the decodes of the per-pixel argmax.

A decode has one value per bin, so both decodes are TABLES: `up_bin_table` and `latitude_bin_table` evaluate the reference's
float32 expressions for every bin index on the CPU, once per (count, device), and `decode_*` gather from them.  The kernel
behind fields.pack_fields_from_logits (gclm_pack_fields_bins) gathers from the same tables, so what it writes is the
reference's output bit for bit and depends on no device cos or sin.

One deliberate deviation from the reference: its `encode_up_bin` returns deg2rad of the bin index, a float tensor; ours
returns the index itself (long), which is what `decode_up_bin` takes.  Everything else matches value for value."""
import math
from typing import Dict, Tuple

import torch

_tables: Dict[Tuple[str, int, torch.device], torch.Tensor] = {}


def _up_step(num_bin: int) -> float:
    if num_bin < 2:
        raise ValueError(f"the up field needs at least one direction and the invalid class (got {num_bin} bins)")
    return 360 / (num_bin - 1)


def _latitude_edges(num_classes: int) -> torch.Tensor:
    """The lower edge of every latitude class in degrees, float32: arange(-90, 90, 180 / num_classes).  Where the step is not
    exact the range can come out one element long or short; such a count has no table."""
    if num_classes < 1:
        raise ValueError(f"the latitude needs at least one class (got {num_classes})")
    edges = torch.arange(-90, 90, 180 / num_classes)
    if edges.numel() != num_classes:
        raise ValueError(f"arange(-90, 90, 180 / {num_classes}) has {edges.numel()} elements, not {num_classes}")
    return edges


def _cached(kind: str, count: int, device, make) -> torch.Tensor:
    key = (kind, int(count), torch.device(device))
    if key not in _tables:
        _tables[key] = make().to(key[2]).contiguous()
    return _tables[key]


def up_bin_table(num_bin: int, device="cpu") -> torch.Tensor:
    """(num_bin, 2) float32: (cos, sin) of the direction of every up bin, (0, 0) for the last, invalid one.  Bin k points at
    (k * 360 / (num_bin - 1) - 180) / 180 * pi, evaluated in float32 in that order, on the CPU."""
    def make():
        k = torch.arange(num_bin)
        angle = (k * _up_step(num_bin) - 180) / 180 * math.pi
        table = torch.stack((torch.cos(angle), torch.sin(angle)), dim=1)
        table[num_bin - 1] = 0
        return table
    return _cached("up", num_bin, device, make)


def latitude_bin_table(num_classes: int, device="cpu") -> torch.Tensor:
    """(num_classes,) float32: the centre of every latitude class in radians, (edge + half a class) / 180 * pi in float32."""
    def make():
        size = 180 / num_classes
        return (_latitude_edges(num_classes) + size / 2) / 180 * math.pi
    return _cached("lat", num_classes, device, make)


def decode_up_bin(bins: torch.Tensor, num_bin: int) -> torch.Tensor:
    """Up bins (B, h, w), integer -> the up field (B, 2, h, w) float32: channel 0 the cosine, channel 1 the sine of the bin's
    direction, both 0 where the bin is the invalid class num_bin - 1."""
    if bins.dim() != 3:
        raise ValueError(f"up bins are (B, h, w), got {tuple(bins.shape)}")
    return up_bin_table(num_bin, bins.device)[bins.long()].permute(0, 3, 1, 2).contiguous()


def decode_bin_latitude(bins: torch.Tensor, num_classes: int) -> torch.Tensor:
    """Latitude bins, integer, any shape -> the latitude in radians, float32, of the same shape: the centre of each bin."""
    return latitude_bin_table(num_classes, bins.device)[bins.long()]


def encode_up_bin(vector_field: torch.Tensor, num_bin: int) -> torch.Tensor:
    """An up field (2, h, w), channel 0 the cosine -> its bins (h, w), long: the direction in degrees, shifted to [0, 360),
    over the bin width, rounded half to even; a full turn wraps to bin 0, and a pixel whose two components are both exactly 0
    is the invalid class num_bin - 1.  (The reference returns deg2rad of these indices; see the module's docstring.)"""
    step = _up_step(num_bin)
    x, y = vector_field[0], vector_field[1]
    degrees = (torch.atan2(y, x) / math.pi * 180 + 180) % 360
    bins = torch.round(degrees / step).long()
    bins = torch.where(bins == num_bin - 1, torch.zeros_like(bins), bins)
    return torch.where((x == 0) & (y == 0), torch.full_like(bins, num_bin - 1), bins)


def encode_bin_latitude(latitude: torch.Tensor, num_classes: int) -> torch.Tensor:
    """A latitude in radians, any shape -> its bins, long: the class whose (lower, upper] range of degrees holds it, the
    first and the last class open-ended."""
    inner = _latitude_edges(num_classes)[1:].to(latitude.device)
    return torch.bucketize(latitude / math.pi * 180, inner, right=False).long()


def fields_from_logits(up_logits: torch.Tensor, lat_logits: torch.Tensor):
    """The definition of fields.pack_fields_from_logits as a torch composition: (up (B, 2, h, w), latitude (B, 1, h, w)) of
    logits (B, Ku, h, w) and (B, Kl, h, w).  torch.argmax's CPU rule decides: the first index of the greatest value, a NaN
    greater than everything (the first one wins), a pixel that is all -inf gives bin 0."""
    up = decode_up_bin(up_logits.argmax(1), up_logits.shape[1])
    lat = decode_bin_latitude(lat_logits.argmax(1), lat_logits.shape[1])
    return up, lat.unsqueeze(1)
