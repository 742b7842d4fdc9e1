"""The radius schedule of the progressive photon-map passes (gi.h gi_progressive_radius), restated:
Knaus & Zwicker's r_{j+1}^2 = r_j^2 (j + alpha) / (j + 1), j counted from 1, in fp64 with one IEEE
operation per step. Python floats are IEEE doubles and math.sqrt is correctly rounded, so the
library's value is held to this one bit for bit."""
import math

MAX_PASS = 1 << 20


def radius(r0, alpha, npass):
    """The estimate radius of pass `npass` (0-based) from r0; NaN for a bad argument."""
    r0, alpha = float(r0), float(alpha)
    if not (r0 > 0.0 and math.isfinite(r0)) or not (0.0 < alpha < 1.0):
        return math.nan
    if npass < 0 or npass >= MAX_PASS:
        return math.nan
    r2 = r0 * r0
    for j in range(1, npass + 1):
        r2 = (r2 * (float(j) + alpha)) / (float(j) + 1.0)
    return math.sqrt(r2)


def pass_args(base_seed, npass, r0_global, r0_caustic, alpha):
    """The oracle flags that restate pass `npass`: its seed, estimate sizes no map reaches and the
    pass's two radii (repr round-trips a double exactly)."""
    return ["-seed", str(base_seed + npass), "-gs", "1000000000", "-cs", "1000000000",
            "-gd", repr(radius(r0_global, alpha, npass)),
            "-cd", repr(radius(r0_caustic, alpha, npass))]
