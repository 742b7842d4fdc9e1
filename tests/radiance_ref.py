"""numpy restatement of the radiance-frame, accumulator, noise and tone-map definitions of gi.h
("radiance frames, accumulation over passes, tone map"): fp64, every sum left to right in the
stated order, one rounding to float32 at the end. The device kernels (gi_radiance.hip) are
compared with it bit for bit in tests/test_gpu_radiance.py. Also readers of the two float image
formats gi_write_image_float writes.
"""
import functools

import numpy as np

LUMA = (0.2126, 0.7152, 0.0722)
NOISE_BLOCK = 256


def box_weight(aa=None, spp=None):
    """reduce_kernel's own expressions: 1.0 / af / af for a camera frame, 1.0 / spp for rays."""
    if spp is not None:
        return 1.0 / spp
    af = 1 << aa
    return 1.0 / af / af


def pass_stats(samples, bw):
    """samples [..., S, 3] float64 -> (m, M2) float64 [..., 3]: m = bw * sum_j s_j,
    M2 = sum_j (s_j - m)^2, j in order."""
    s = np.asarray(samples, dtype=np.float64)
    acc = np.zeros(s.shape[:-2] + (3,))
    for j in range(s.shape[-2]):
        acc = acc + s[..., j, :]
    m = bw * acc
    m2 = np.zeros_like(m)
    for j in range(s.shape[-2]):
        d = s[..., j, :] - m
        m2 = m2 + d * d
    return m, m2


def variance_of_mean(m2, n):
    """M2 / (n - 1) / n in fp64, 0 when n < 2."""
    if n < 2:
        return np.zeros_like(m2)
    return m2 / float(n - 1) / float(n)


def mean_variance(samples, bw):
    """(mean, variance of the mean) float32 of a pass, as gi_render_radiance returns them."""
    m, m2 = pass_stats(samples, bw)
    return m.astype(np.float32), variance_of_mean(m2, np.shape(samples)[-2]).astype(np.float32)


def clamped_frame(samples, bw):
    """What reduce_kernel makes of the same samples: each clamped to [0, 1], summed in order,
    times bw; (rgbf float32, rgb8 = truncated 255 * the fp64 value)."""
    s = np.asarray(samples, dtype=np.float64)
    acc = np.zeros(s.shape[:-2] + (3,))
    for j in range(s.shape[-2]):
        c = s[..., j, :]
        acc = acc + np.where(c < 0, 0.0, np.where(c > 1.0, 1.0, c))
    v = bw * acc
    return v.astype(np.float32), (255 * v).astype(np.uint8)


class Accum:
    """The accumulator: mu, A per pixel and channel, one sample count N; add() is
    accum_merge_kernel, get() is gi_accum_get."""

    def __init__(self, shape):
        self.mu = np.zeros(tuple(shape) + (3,))
        self.A = np.zeros(tuple(shape) + (3,))
        self.N = 0

    def add(self, m, m2, S):
        if self.N == 0:  # the first pass is taken as is
            self.mu, self.A = np.array(m, dtype=np.float64), np.array(m2, dtype=np.float64)
        else:
            d = m - self.mu
            n1 = float(self.N + S)
            self.mu = self.mu + (d * float(S)) / n1
            self.A = (self.A + m2) + ((d * d) * (float(self.N) * float(S))) / n1
        self.N += S

    def add_samples(self, samples, bw):
        m, m2 = pass_stats(samples, bw)
        self.add(m, m2, np.shape(samples)[-2])

    def get(self):
        """(mean float32, variance float32, N, noise)"""
        return (self.mu.astype(np.float32), variance_of_mean(self.A, self.N).astype(np.float32),
                self.N, noise(self.mu, self.A, self.N))


def pixel_errors(mu, A, N):
    """e = sqrt(v) / (Y + 0.01) per pixel, flat in pixel order."""
    v3 = variance_of_mean(np.asarray(A, dtype=np.float64), N).reshape(-1, 3)
    mu = np.asarray(mu, dtype=np.float64).reshape(-1, 3)
    y = LUMA[0] * mu[:, 0] + LUMA[1] * mu[:, 1] + LUMA[2] * mu[:, 2]
    v = ((LUMA[0] * LUMA[0]) * v3[:, 0] + (LUMA[1] * LUMA[1]) * v3[:, 1]
         + (LUMA[2] * LUMA[2]) * v3[:, 2])
    return np.sqrt(v) / (y + 0.01)


def noise(mu, A, N):
    """Mean relative standard error of luminance in accum_noise_kernel's summation order: blocks
    of 256 consecutive pixels, zero-padded, each a tree x[i] += x[i + h] for h = 128 .. 1; the
    block sums added in order."""
    e = pixel_errors(mu, A, N)
    npix = len(e)
    nb = (npix + NOISE_BLOCK - 1) // NOISE_BLOCK
    x = np.zeros(nb * NOISE_BLOCK)
    x[:npix] = e
    x = x.reshape(nb, NOISE_BLOCK)
    h = NOISE_BLOCK // 2
    while h >= 1:
        x[:, :h] = x[:, :h] + x[:, h:2 * h]
        h //= 2
    total = 0.0
    for b in range(nb):
        total += float(x[b, 0])
    return total / float(npix)


def tonemap(c, exposure=1.0, white=0.0):
    """x = exposure * c; extended Reinhard x (1 + x / white^2) / (1 + x) when white > 0, else x;
    clamped to [0, 1]; float32."""
    x = exposure * np.asarray(c, dtype=np.float32).astype(np.float64)
    y = (x * (1.0 + x / (white * white))) / (1.0 + x) if white > 0 else x
    y = np.where(y < 0.0, 0.0, np.where(y > 1.0, 1.0, y))
    return y.astype(np.float32)


def quantize(rgbf):
    """gi_quantize: truncate 255 * c."""
    return (255 * np.asarray(rgbf, dtype=np.float32).astype(np.float64)).astype(np.uint8)


def read_pfm(path):
    """(array [H, W, 3] float32 with row 0 = bottom, the raw pixel bytes)"""
    with open(path, "rb") as f:
        data = f.read()
    head = data.split(b"\n", 3)
    assert head[0] == b"PF", head[0]
    w, h = (int(v) for v in head[1].split())
    assert float(head[2]) < 0  # little-endian
    assert head[2] == b"-1.0"
    raw = head[3]
    assert len(raw) == w * h * 12
    return np.frombuffer(raw, dtype="<f4").reshape(h, w, 3), raw


def read_hdr(path):
    """(header lines before the blank one, resolution line, rgbe bytes [H, W, 4] top row first)"""
    with open(path, "rb") as f:
        data = f.read()
    head, rest = data.split(b"\n\n", 1)
    res, raw = rest.split(b"\n", 1)
    t = res.split()
    assert t[0] == b"-Y" and t[2] == b"+X", res
    h, w = int(t[1]), int(t[3])
    assert len(raw) == w * h * 4
    return head.split(b"\n"), res, np.frombuffer(raw, dtype=np.uint8).reshape(h, w, 4)


# the ray batches (ray_cases: scene, sensor, spp) whose samples are compared with the oracle's
ORACLE_BATCHES = [("cornell_dim", "panorama", 3), ("stilllife", "lightfield", 5)]


@functools.lru_cache(maxsize=None)
def oracle_samples(name, sensor, spp):
    """The oracle's value of every ray of a ray_cases batch, [H, W, spp, 3] float32: the same
    rays and ids rendered as a (W * spp) x H frame at one ray per pixel (clamped to [0, 1]: the
    oracle keeps no unclamped value). Shared by the tests: do not modify."""
    import oracle_lib
    import ray_cases
    rays, ids = ray_cases.batch(name, sensor, spp)
    args = ray_cases.scene_args(name, ray_cases.W * spp, ray_cases.H)
    _rgb, f, _st = oracle_lib.render_rays(args, 1, rays, ids)
    f = f.reshape(ray_cases.H, ray_cases.W, spp, 3)
    f.setflags(write=False)
    return f
