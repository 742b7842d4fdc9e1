"""numpy restatement of the adaptive passes of gi.h ("adaptive passes"): the accumulator with one
sample count per pixel, the tile error in its stated summation order and the tile selection.
Builds on radiance_ref (pass statistics, luma weights, the noise tree's block size). The device
kernels (gi_radiance.hip accum_merge_kernel, tile_error_kernel, tile_select_kernel) are compared
with it bit for bit in tests/test_gpu_adaptive.py.
"""
import numpy as np

import radiance_ref as rr

LANES = 64
DEFAULTS = dict(tile_px=8, min_samples=8, max_samples=0, dilate=1, threshold=0.02)


def variance_of_mean(A, n):
    """A / (n - 1) / n per pixel in fp64 (A [..., 3], n [...] int64), 0 where n < 2."""
    n = np.asarray(n, dtype=np.int64)
    ok = n >= 2
    safe = np.where(ok, n, 2)
    v = np.asarray(A, dtype=np.float64) / (safe - 1).astype(np.float64)[..., None]
    v = v / safe.astype(np.float64)[..., None]
    return np.where(ok[..., None], v, 0.0)


def pixel_errors(mu, A, n):
    """e = sqrt(v) / (Y + 0.01) per pixel under its own count (0 where n < 2), shape of n."""
    n = np.asarray(n, dtype=np.int64)
    v3 = variance_of_mean(A, n)
    mu = np.asarray(mu, dtype=np.float64)
    L = rr.LUMA
    y = L[0] * mu[..., 0] + L[1] * mu[..., 1] + L[2] * mu[..., 2]
    v = (L[0] * L[0]) * v3[..., 0] + (L[1] * L[1]) * v3[..., 1] + (L[2] * L[2]) * v3[..., 2]
    return np.where(n >= 2, np.sqrt(v) / (y + 0.01), 0.0)


def noise(mu, A, n):
    """gi_accum_get's noise with per-pixel counts: accum_noise_kernel's order (radiance_ref.noise)."""
    e = pixel_errors(mu, A, n).reshape(-1)
    npix = len(e)
    B = rr.NOISE_BLOCK
    nb = (npix + B - 1) // B
    x = np.zeros(nb * B)
    x[:npix] = e
    x = x.reshape(nb, B)
    h = B // 2
    while h >= 1:
        x[:, :h] = x[:, :h] + x[:, h:2 * h]
        h //= 2
    total = 0.0
    for b in range(nb):
        total += float(x[b, 0])
    return total / float(npix)


class Accum:
    """The accumulator with one count per pixel: mu, A [H, W, 3], n [H, W] int64. add() is
    accum_merge_kernel (where = the pixels of a masked pass, None = all), get() is gi_accum_get."""

    def __init__(self, shape):
        self.mu = np.zeros(tuple(shape) + (3,))
        self.A = np.zeros(tuple(shape) + (3,))
        self.n = np.zeros(tuple(shape), dtype=np.int64)

    def add(self, m, m2, S, where=None):
        m = np.asarray(m, dtype=np.float64)
        m2 = np.asarray(m2, dtype=np.float64)
        sel = np.ones(self.n.shape, dtype=bool) if where is None else np.asarray(where, dtype=bool)
        first = (self.n == 0)[..., None]
        d = m - self.mu
        n1 = (self.n + S).astype(np.float64)[..., None]
        ns = (self.n.astype(np.float64) * float(S))[..., None]
        mu = self.mu + (d * float(S)) / n1
        A = (self.A + m2) + ((d * d) * ns) / n1
        mu = np.where(first, m, mu)    # a pixel without samples takes the pass as is
        A = np.where(first, m2, A)
        self.mu = np.where(sel[..., None], mu, self.mu)
        self.A = np.where(sel[..., None], A, self.A)
        self.n = np.where(sel, self.n + S, self.n)

    def add_samples(self, samples, bw, where=None):
        m, m2 = rr.pass_stats(samples, bw)
        self.add(m, m2, np.shape(samples)[-2], where)

    def get(self):
        """(mean float32, variance float32, smallest count, noise)"""
        return (self.mu.astype(np.float32), variance_of_mean(self.A, self.n).astype(np.float32),
                int(self.n.min()), noise(self.mu, self.A, self.n))


def tile_grid(w, h, T):
    return (w + T - 1) // T, (h + T - 1) // T


def tile_errors_of(e, n, T):
    """Per-pixel errors e and counts n [H, W] -> (tile_error [tiles] float64, n_min [tiles] int64,
    pixels inside [tiles]). Slot q = y * T + x of a tile (0 outside the frame); lane l sums the
    slots q = l, l + 64, ... in ascending q from 0; x[l] += x[l + h], h = 32 .. 1; / pixels."""
    h, w = e.shape
    tx, ty = tile_grid(w, h, T)
    err = np.zeros(tx * ty)
    nmin = np.zeros(tx * ty, dtype=np.int64)
    inside = np.zeros(tx * ty, dtype=np.int64)
    rows = (T * T + LANES - 1) // LANES
    for t in range(tx * ty):
        x0, y0 = (t % tx) * T, (t // tx) * T
        sub = e[y0:y0 + T, x0:x0 + T]
        slots = np.zeros((T, T))
        slots[:sub.shape[0], :sub.shape[1]] = sub
        q = np.zeros(rows * LANES)
        q[:T * T] = slots.reshape(-1)
        q = q.reshape(rows, LANES)
        x = np.zeros(LANES)
        for r in range(rows):
            x = x + q[r]
        hh = LANES // 2
        while hh >= 1:
            x[:hh] = x[:hh] + x[hh:2 * hh]
            hh //= 2
        inside[t] = sub.size
        err[t] = x[0] / float(sub.size)
        nmin[t] = n[y0:y0 + T, x0:x0 + T].min()
    return err, nmin, inside


def tile_errors(acc, T):
    """(tile_error, n_min, pixels inside) of an Accum."""
    return tile_errors_of(pixel_errors(acc.mu, acc.A, acc.n), acc.n, T)


def select(err, nmin, tx, ty, min_samples=8, max_samples=0, dilate=1, threshold=0.02, **_):
    """The selection: dict of bool [tiles] arrays by_error, core, dilated, active."""
    err = np.asarray(err).reshape(ty, tx)
    nmin = np.asarray(nmin).reshape(ty, tx)
    below_max = np.ones((ty, tx), dtype=bool) if max_samples == 0 else nmin < max_samples
    by_error = (err > threshold) & below_max
    core = (nmin < min_samples) | by_error
    near = np.zeros((ty, tx), dtype=bool)
    pad = np.zeros((ty + 2, tx + 2), dtype=bool)
    pad[1:-1, 1:-1] = by_error
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                near |= pad[1 + dy:1 + dy + ty, 1 + dx:1 + dx + tx]
    dilated = near & ~core & below_max if dilate else np.zeros((ty, tx), dtype=bool)
    out = dict(by_error=by_error, core=core, dilated=dilated, active=core | dilated)
    return {k: v.reshape(-1) for k, v in out.items()}


def pixel_mask(mask, w, h, T):
    """Tile mask [tiles] -> bool [H, W]: the pixels of the active tiles."""
    tx, ty = tile_grid(w, h, T)
    m = np.asarray(mask).reshape(ty, tx) != 0
    return np.repeat(np.repeat(m, T, axis=0), T, axis=1)[:h, :w]


def checkerboard(w, h, T, phase=0):
    """uint8 tile mask: tile (tx, ty) active when (tx + ty) % 2 == phase."""
    tx, ty = tile_grid(w, h, T)
    yy, xx = np.mgrid[0:ty, 0:tx]
    return (((xx + yy) % 2) == phase).astype(np.uint8).reshape(-1)
