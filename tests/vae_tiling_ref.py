"""float64 reference of the tiled autoencoder passes (include/gligen_amd_tiling.h): the tile plan and weight tables restated
independently of gligen_amd/vae_tiling.py, the blend of a list of tiles, and the error bound the blend kernel is held to."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32


def plan(L, T, overlap):
    """Origins along one axis: one tile if L <= T, else n = ceil((L - overlap) / (T - overlap)) tiles of extent T spread evenly from 0 to
    L - T, rounded half up."""
    if L <= T:
        return [0]
    n = math.ceil((L - overlap) / (T - overlap))
    return [int(math.floor(i * (L - T) / (n - 1) + 0.5)) for i in range(n)]


def tables64(L, T, overlap, origins, scale=1):
    """float64 [n][min(T, L) * scale]: m_t(x) / sum of m over the covering tiles, m = min(1, d_lo / R, d_hi / R) with no ramp at an image
    border; origin, extent, length and ramp in output pixels (times `scale`)."""
    Te, Lo, R = min(T, L) * scale, L * scale, overlap * scale
    m = np.zeros((len(origins), Lo))
    for t, o in enumerate(origins):
        o *= scale
        for x in range(o, o + Te):
            v = 1.0
            if o > 0:
                v = min(v, (x - o + 0.5) / R)
            if o + Te < Lo:
                v = min(v, (o + Te - x - 0.5) / R)
            m[t, x] = v
    total = m.sum(0)
    return np.stack([m[t, o * scale:o * scale + Te] / total[o * scale:o * scale + Te] for t, o in enumerate(origins)])


def blend64(tiles, B, H, W, oy, ox, wy, wx):
    """tiles [B ny nx][C][TH][TW] (index (b ny + ty) nx + tx), origins oy / ox on the output grid, weight tables wy [ny][TH], wx [nx][TW]
    (the fp32 tables the kernel reads, taken to float64 exactly). Returns float64 (out [B][C][H][W], sum |wy wx v| [B][C][H][W],
    number of covering tiles [H][W])."""
    t = torch.as_tensor(tiles).double().cpu()
    wy, wx = torch.as_tensor(wy).double().cpu(), torch.as_tensor(wx).double().cpu()
    ny, nx = len(oy), len(ox)
    C, TH, TW = t.shape[1:]
    assert t.shape[0] == B * ny * nx and tuple(wy.shape) == (ny, TH) and tuple(wx.shape) == (nx, TW)
    out, mag, cnt = torch.zeros(B, C, H, W, dtype=torch.float64), torch.zeros(B, C, H, W, dtype=torch.float64), torch.zeros(H, W, dtype=torch.int64)
    for b in range(B):
        for ty, y0 in enumerate(oy):
            for tx, x0 in enumerate(ox):
                w = wy[ty][:, None] * wx[tx][None, :]
                v = t[(b * ny + ty) * nx + tx]
                out[b, :, y0:y0 + TH, x0:x0 + TW] += w * v
                mag[b, :, y0:y0 + TH, x0:x0 + TW] += (w * v).abs()
                if b == 0:
                    cnt[y0:y0 + TH, x0:x0 + TW] += 1
    assert int(cnt.min()) >= 1, "the plan leaves an element uncovered"
    return out, mag, cnt


def blend_bound(mag, cnt):
    """Per element (n + 2) 2^-24 sum |wy wx v|, n the number of covering tiles. Derivation from tile_blend_kernel's operation sequence
    (u = 2^-24): w = fl(wy wx) carries one rounding; the first covering tile's term fl(w v) one more; each of the other n - 1 tiles is
    one fma, acc = fl(w v + acc), i.e. one rounding of the running sum. A term therefore passes through at most 1 (its weight) + 1 (its
    own product or fma) + n - 1 (the later fmas) = n + 1 roundings, so |got - exact| <= ((1 + u)^(n + 1) - 1) sum |wy wx v|, and
    (1 + u)^(n + 1) - 1 <= (n + 2) u for every n + 1 < 2^11. The float64 reference works on the same fp32 tables and tiles, its own error
    (2^-53 relative) is far inside the spare unit. Nothing here was fitted to a measured error; underflow does not occur at these
    magnitudes (products of two weights >= 2^-20, values of order 1)."""
    return (cnt.double()[None, None] + 2.0) * U * mag


def posterior64(moments, quant_w, quant_b, noise, scale_factor):
    """AutoencoderKL.encode's tail in float64: quant_conv (1 x 1), logvar clamped to [-30, 20], mean + exp(0.5 logvar) * noise, times
    scale_factor."""
    m = moments.double().cpu()
    w = quant_w.double().cpu().reshape(quant_w.shape[0], quant_w.shape[1])
    q = torch.einsum("oc,bchw->bohw", w, m) + quant_b.double().cpu()[None, :, None, None]
    mean, logvar = q.chunk(2, dim=1)
    logvar = logvar.clamp(-30.0, 20.0)
    return (mean + torch.exp(0.5 * logvar) * noise.double().cpu()) * scale_factor
