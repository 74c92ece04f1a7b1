"""What the tests of the classification-head epilogue share (tests/test_pack_bins_abi.py, tests/test_pack_bins.py) with the
generator of their fixture (tests/golden/make_golden_bins.py): the planted pixels -- logit vectors on which an argmax can go
wrong -- and where they are put in an image.  A plain module, like the other *_gate.py files.

Every planted vector holds only values that bfloat16 and float16 both represent (8 significant bits, magnitudes between
2^-7 and 8, the infinities, NaN), so planting it into logits that were rounded to a 16-bit type is planting it again after
the rounding, ties included."""
import torch

KINDS = ("tie of two", "tie of three", "winner in the first channel", "winner in the last channel", "NaN before the maximum",
         "NaN after the maximum, twice", "all -inf", "+inf twice")
TOP = 8.0          # above every background value (|background| <= 6)


def picks(K: int):
    """Up to three distinct channels of K, in order: off the first and the last where K allows, one in the first unrolled
    chunk of the kernel's channel loop, one in the middle, one in its remainder (K = 180: 1, 90, 178)."""
    return [1, max(K // 2, 2), K - 2] if K >= 5 else list(range(K))[-3:]


def planted(K: int, seed: int) -> torch.Tensor:
    """(len(KINDS), K) float32: one logit vector per kind, for K >= 1 bins (with fewer than three bins the kinds shrink to what
    K channels can hold)."""
    g = torch.Generator().manual_seed(seed)
    v = (2 * torch.randn(len(KINDS), K, generator=g)).clamp(-6, 6).bfloat16().float()
    v = torch.where(v.abs() < 2.0 ** -7, torch.full_like(v, 0.5), v)
    p = picks(K)
    a, b, c = p[0], p[len(p) // 2], p[-1]
    nan, inf = float("nan"), float("inf")
    v[0, [a, c]] = TOP
    v[1, p] = TOP
    v[2, 0] = TOP
    v[3, K - 1] = TOP
    v[4, c] = TOP
    v[4, a] = nan if a != c else TOP
    v[5, a] = TOP
    if K >= 3:
        v[5, [b, c]] = nan
    v[6] = -inf
    v[7, [a, c]] = inf
    return v


def plant(logits: torch.Tensor, vectors: torch.Tensor, slots: int = 8) -> list:
    """Writes the vectors into `logits` (B, K, h, w), in place, in rounds of `slots`: vector k of a round goes to a pixel whose
    index is k modulo `slots` -- the lane slots of a vector unit --, round after round to the next image and, once every image
    has one, to other pixels (never one twice).  Returns the (image, pixel) pairs."""
    B, K, h, w = logits.shape
    flat = logits.view(B, K, h * w)
    gens = h * w // slots
    where = []
    for j in range(vectors.shape[0]):
        r, k = divmod(j, slots)
        b, q = r % B, r // B
        assert q < gens, "more rounds than the images have room for"
        px = k + slots * ((k + q) % gens)
        flat[b, :, px] = vectors[j].to(logits.dtype)
        where.append((b, px))
    assert len(set(where)) == len(where)
    return where


def head_logits(B: int, Ku: int, Kl: int, h: int, w: int, seed: int, dtype=torch.float32, rounds: int = len(KINDS)):
    """Seeded float32 logits of both heads, rounded to `dtype`, then the planted pixels: `rounds` rounds of 8 vectors, round r
    holding the kinds rotated by r, so that after 8 rounds each kind has met each pixel index modulo 8.  Returns (up_logits,
    lat_logits, planted pixels)."""
    g = torch.Generator().manual_seed(seed)
    up = (2 * torch.randn(B, Ku, h, w, generator=g)).to(dtype).contiguous()
    lat = (2 * torch.randn(B, Kl, h, w, generator=g)).to(dtype).contiguous()
    rounds = min(rounds, B * (h * w // 8))
    order = torch.cat([torch.roll(torch.arange(len(KINDS)), r) for r in range(rounds)])
    where = plant(up, planted(Ku, seed + 1)[order])
    plant(lat, planted(Kl, seed + 2)[torch.roll(order, 3)])
    return up, lat, where
