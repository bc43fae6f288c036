"""Tile plans of the tiled autoencoder passes (include/gligen_amd_tiling.h): where the tiles sit along an axis, and the per-axis blend
weights. Pure host code, no torch: the engine uploads what these functions return.

Units: a plan is made on the LATENT grid for the decoder and the encoder alike (an encoder tile of T latent pixels is f T image pixels,
its origins multiples of f; f = 2 ** (n_mult - 1) is the autoencoder's factor). The weight tables are made on the OUTPUT grid of the
pass: image pixels for the decoder (scale = f), latent pixels for the encoder (scale = 1).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple, Union

import numpy as np

TILING_MODES = ("off", "on", "auto")
DEFAULT_TILE = 64          # latent pixels: a 512 x 512 image tile at f = 8
DEFAULT_OVERLAP = 16

IntOrPair = Union[int, Sequence[int]]


def tile_plan(L: int, T: int, overlap: int) -> List[int]:
    """Origins of the tiles along an axis of length L: one tile of extent L at 0 if L <= T, else n = ceil((L - overlap) / (T - overlap))
    tiles of extent exactly T, origins spread evenly from 0 to L - T and rounded (half up, in integers). Every stride is then at most
    T - overlap: neighbours overlap by at least `overlap`. Three tiles can cover one coordinate (L = 113, T = 64, overlap = 16:
    origins 0, 25, 49)."""
    L, T, overlap = int(L), int(T), int(overlap)
    if L < 1 or T < 1:
        raise ValueError(f"tile_plan: axis length {L} and tile {T} must be positive")
    if not 1 <= overlap <= T // 2:
        raise ValueError(f"tile_plan: overlap {overlap} must satisfy 1 <= overlap <= tile // 2 = {T // 2}")
    if L <= T:
        return [0]
    n = -(-(L - overlap) // (T - overlap))
    return [(2 * i * (L - T) + (n - 1)) // (2 * (n - 1)) for i in range(n)]


def _pair(v: IntOrPair, name: str) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{name}: an integer or a pair (per axis: y, x), got {v!r}")
        a, b = v
    else:
        a = b = v
    for x in (a, b):
        if isinstance(x, bool) or int(x) != x:
            raise ValueError(f"{name}: an integer or a pair of integers, got {v!r}")
    return int(a), int(b)


def check_tiling(tile: IntOrPair = DEFAULT_TILE, overlap: IntOrPair = DEFAULT_OVERLAP) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((th, tw), (oy, ox)) in latent pixels, or ValueError naming what is wrong: vae_tile must be a positive multiple of 8 per axis
    (the autoencoder's attention needs th * tw % 64 == 0), 1 <= vae_tile_overlap <= vae_tile // 2 per axis."""
    t, o = _pair(tile, "vae_tile"), _pair(overlap, "vae_tile_overlap")
    for T, ov, axis in zip(t, o, "yx"):
        if T < 8 or T % 8:
            raise ValueError(f"vae_tile: {T} along {axis} is not a positive multiple of 8 latent pixels (the VAE attention needs th * tw % 64 == 0)")
        if not 1 <= ov <= T // 2:
            raise ValueError(f"vae_tile_overlap: {ov} along {axis} must satisfy 1 <= overlap <= vae_tile // 2 = {T // 2}")
    return t, o


def check_mode(mode) -> str:
    m = "off" if mode is None else mode
    if m not in TILING_MODES:
        raise ValueError(f"vae_tiling: {mode!r} is not one of {', '.join(TILING_MODES)}")
    return m


def axis_weights64(L: int, T: int, overlap: int, origins: Sequence[int], scale: int = 1) -> np.ndarray:
    """float64 [n][T_out] weights of the tiles along one axis on the output grid (origin, extent, length and ramp times `scale`).
    m(x) = min(1, d_lo / R, d_hi / R) with d_lo = x - o + 0.5 where the tile does not start at the border, d_hi = o + T - x - 0.5 where
    it does not end at it (no ramp at an image border); the entry is m_t(x) / sum of m over the tiles covering x."""
    n = len(origins)
    Te = min(T, L) * scale                       # a single tile has the axis's extent
    Lo, R = L * scale, float(overlap * scale)
    m = np.zeros((n, Lo), dtype=np.float64)
    for t, o in enumerate(origins):
        o0 = o * scale
        x = np.arange(o0, o0 + Te, dtype=np.float64)
        v = np.ones(Te, dtype=np.float64)
        if o0 > 0:
            v = np.minimum(v, (x - o0 + 0.5) / R)
        if o0 + Te < Lo:
            v = np.minimum(v, (o0 + Te - x - 0.5) / R)
        m[t, o0:o0 + Te] = v
    total = m.sum(axis=0)
    assert (total > 0).all(), "tile plan leaves a coordinate uncovered"
    out = np.empty((n, Te), dtype=np.float64)
    for t, o in enumerate(origins):
        o0 = o * scale
        out[t] = m[t, o0:o0 + Te] / total[o0:o0 + Te]
    return out


def weight_tables(L: int, T: int, overlap: int, origins: Sequence[int], scale: int = 1) -> np.ndarray:
    """axis_weights64 stored as fp32: what the blend kernel reads."""
    return axis_weights64(L, T, overlap, origins, scale).astype(np.float32)


class Plan2D:
    """The plan of one (h, w) latent grid: origins and extents per axis (latent pixels)."""

    def __init__(self, h: int, w: int, tile: IntOrPair = DEFAULT_TILE, overlap: IntOrPair = DEFAULT_OVERLAP):
        (th, tw), (ovy, ovx) = check_tiling(tile, overlap)
        self.h, self.w, self.overlap = int(h), int(w), (ovy, ovx)
        self.oy, self.ox = tile_plan(h, th, ovy), tile_plan(w, tw, ovx)
        self.th, self.tw = min(th, self.h), min(tw, self.w)
        self.tile = (th, tw)

    @property
    def ny(self) -> int:
        return len(self.oy)

    @property
    def nx(self) -> int:
        return len(self.ox)

    @property
    def single(self) -> bool:
        return self.ny == 1 and self.nx == 1

    def tables(self, scale: int):
        """(wy, wx) fp32 on the output grid of a pass whose output is `scale` times the latent grid."""
        return (weight_tables(self.h, self.tile[0], self.overlap[0], self.oy, scale),
                weight_tables(self.w, self.tile[1], self.overlap[1], self.ox, scale))
