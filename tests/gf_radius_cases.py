"""Cases and bar of the guided filter's fused radii above 30 (tests/test_gpu_guided_filter_radius.py,
tests/test_guided_filter_radius_cases_cpu.py).  Plain numpy on the CPU; the judge (``restate`` / ``judge``) and the inputs are
tests/gf_cases.py's, and the device is never its own judge.

r = 60 and r = 90 run the two fused launches of radius 30 with a strip geometry of their own (csrc/guided_filter.hip: GfGeom).
GEOM mirrors that geometry as gf_cases.STRIP / SEG mirror radius 30's: the output columns per strip, the outputs per sliding
segment, and the rows per block of the FIRST launch in the default dispatch (where the error diffusion of the half planes
restarts).

The bar is gf_cases.judge with
    tau = tau_ref + ((runs + 1) / 2) * tau_half,        runs = (2r - 1) // VS1 + 2
tau_ref = gf_cases.min_tau(q64, oracle32) (where the float32 oracle still disagrees with rint(q64)), tau_half =
gf_cases.tau_half(A, Bp, r) (what two end residuals of the half storage can do to q).  A (2r + 1)-row window spans at most
``runs`` diffusion runs of VS1 rows and carries one residual per run plus the one before its first row: runs + 1 residuals,
tau_half counts two.  This is the counting that gives 2 tau_half at r = 30 with 32 rows (runs = 3); the factor is 3 at r = 60
(VS1 = 32, runs = 5) and 2.5 at r = 90 (VS1 = 64, runs = 4; it would be 4 with 32 rows).  Derived, not measured.  At most
gf_cases.EXEMPT_CAP of a case's values may lie within tau of a rounding boundary.

Extents sit on the geometry: r + 1 rows and columns (the minimum the entry point accepts), rows around the row blocks of both
launches, columns around one and two strips, 2048 columns, 600 x 530, and 1024^2 at r = 60.  No 1536^2 case: the float64
reference alone takes over ten seconds there.
"""
import functools

import numpy as np

import gf_cases as C

GEOM = {60: dict(strip=256, seg=16, vs1=32), 90: dict(strip=320, seg=16, vs1=64)}
RADII = tuple(sorted(GEOM))
EPS_LARGE = 1e-2 * 255 * 255


def strip_widths(r):
    S = GEOM[r]["strip"]
    return sorted({min(w, 2048) for w in (S - 1, S, S + 1, 2 * S - 1, 2 * S + 1)})


def extents(r):
    rows = {60: 70, 90: 100}[r]
    return ([(r + 2, r + 1), (r + 1, r + 1), ({60: 500, 90: 700}[r], r + 1)] +
            [(h, 200) for h in {60: (64, 65, 97), 90: (96, 97, 129)}[r]] +
            [(rows, w) for w in strip_widths(r)] + [(rows, 2048), (600, 530)])


def cases(r):
    """(kind, H, W, r, eps)"""
    S = GEOM[r]["strip"]
    out = [(k, h, w, r, C.EPS) for (h, w) in extents(r) for k in ("blocks", "flat")]
    if r == 60:
        out.append(("blocks", 1024, 1024, r, C.EPS))
    out += [(k, 130, S + 1, r, C.EPS) for k in ("saturating", "const_both", "aliased", "smooth")]
    out.append(("blocks", 130, S + 1, r, EPS_LARGE))
    return out


CASES = [c for r in RADII for c in cases(r)]
# the extent of the bit-equality tests (batch, stream, repeat, views), per radius
BITS_EXTENT = {r: (100, GEOM[r]["strip"] + 1) for r in RADII}


def runs(r):
    """the largest number of diffusion runs (VS1 rows each) that a (2r + 1)-row window can span"""
    return (2 * r - 1) // GEOM[r]["vs1"] + 2


class Ref:
    """everything the bar needs for one (guide, src, r, eps), r a fused radius above 30"""

    def __init__(self, guide, src, r, eps):
        import ppst_oracle as O
        self.r, self.eps = r, eps
        self.q64, A, Bp = C.restate(guide, src, r, eps)
        self.expect = C.round_u8(self.q64)
        self.oracle32 = O.guided_filter_color(guide, src, r, eps, dtype=np.float32)
        self.tau_ref = C.min_tau(self.q64, self.oracle32)
        self.tau_half = C.tau_half(A, Bp, r)
        self.tau = self.tau_ref + (runs(r) + 1) / 2 * self.tau_half
        d, _ = C.boundary_distance(self.q64)
        self.exempt = float((d <= self.tau).mean())
        self.saturating = float(((self.q64 < 0) | (self.q64 > 255)).mean())


@functools.lru_cache(maxsize=None)
def ref(kind, H, W, r, eps=C.EPS):
    g, s = C.inputs(kind, H, W)
    return Ref(g, s, r, eps)
