"""What the fixed-point accumulator (drt_amd/csrc/drt_fixed.h) must give, in Python's exact integers, and the edge cases both sides are
held to: tests/test_fixed_point.py runs them against the header compiled for the host, tests/test_gpu_fixed_device.py against the gfx950
compilation and the device atomics (tests/devsim/fx_device.hip).  One list, so that the two sides cannot drift."""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import numpy as np

FRAC = 80                      # kFxFrac: one unit = 2^-80
HUGE = 2.0 ** 46               # kFxHuge: |x| >= 2^46 is a flag, not a summand
NAN, POS, NEG = 1, 2, 4        # kFxNaN, kFxPosInf, kFxNegInf
M64, M128 = (1 << 64) - 1, (1 << 128) - 1
NAN_BITS = 0x7FF8000000000000


def q(x):
    """The truncated unit count of a finite double |x| < 2^46: int(Fraction(x) * 2**80), by frexp and a shift."""
    m, e = math.frexp(abs(x))
    mi, sh = int(m * 9007199254740992.0), e - 53 + FRAC          # |x| = mi * 2^(e - 53), mi < 2^53 exactly
    v = mi << sh if sh >= 0 else mi >> -sh
    return -v if x < 0 else v


def flags_of(x):
    """The sticky flags of a contribution that does not enter the sum (0: it does)."""
    if x != x:
        return NAN
    if x >= HUGE:
        return POS
    if x <= -HUGE:
        return NEG
    return 0


def signed64(u):
    return u - (1 << 64) if u >= 1 << 63 else u


def split(v):
    """An integer mod 2^128 as the (hi, lo) words of a cell, both as signed 64-bit numbers (what an int64 tensor holds)."""
    v &= M128
    return signed64(v >> 64), signed64(v & M64)


def signed128(v):
    v &= M128
    return v - (1 << 128) if v >= 1 << 127 else v


def bits_of(d):
    return NAN_BITS if d != d else struct.unpack("<q", struct.pack("<d", d))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def value_bits(v, flags=0):
    """The bit pattern (as int64) of fx_to_double: the exact sum v (any representative mod 2^128) rounded ONCE to nearest-even, or the
    inf / NaN the flags stand for (the NaN is the default quiet one)."""
    if flags:
        if flags & NAN or (flags & POS and flags & NEG):
            return signed64(NAN_BITS)
        return bits_of(math.inf if flags & POS else -math.inf)
    return bits_of(float(Fraction(signed128(v), 1 << FRAC)))             # (Fraction -> float rounds to nearest-even)


# ---- conversion: double -> units ---------------------------------------------------------------------------------------------------------
def _below(x):
    return math.copysign(math.nextafter(abs(x), 0.0), x)


CONVERSION_EDGES = []
for _s in (1.0, -1.0):
    CONVERSION_EDGES += [_s * HUGE, _below(_s * HUGE),                                  # the flag threshold and the largest summand
                         _s * 2.0 ** -80, _below(_s * 2.0 ** -80), _s * 1.5 * 2.0 ** -80,   # one unit, just below it (0), 1.5 units (1)
                         _s * 0.0, _s * math.inf]
CONVERSION_EDGES += [2.0 ** -28, _below(2.0 ** -28),                                    # the smallest exactly represented binade, and below it
                     2.0 ** -16 - 2.0 ** -69,                                           # low word all ones above bit 10
                     5e-324, 2.2250738585072014e-308,                                  # the smallest subnormal, DBL_MIN
                     from_bits(0x7FF8000000000000), from_bits(0xFFF8000000000ABC), from_bits(0x7FF0000000000123), from_bits(0xFFF4000000000001)]


def conversion_values(n_random=50000, seed=1):
    """The edges above and `n_random` values +-U(0,1) * 2^U(-120,50) (some of them beyond the flag threshold)."""
    rnd = random.Random(seed)
    return CONVERSION_EDGES + [rnd.choice([-1, 1]) * rnd.random() * 2.0 ** rnd.uniform(-120, 50) for _ in range(n_random)]


# ---- rounding: cell -> double ------------------------------------------------------------------------------------------------------------
def finalize_edges(seed=2):
    """[(v, flags)]: exact sums (signed integers of units) whose single rounding is easy to get wrong."""
    rnd = random.Random(seed)
    out = [(-(1 << 127), 0), ((1 << 127) - 1, 0), (-((1 << 127) - 1), 0), (1, 0), (-1, 0), (0, 0)]
    for p in range(53, 127):                                            # position of the leading one: p - 52 bits are dropped
        half = 1 << (p - 53)
        for keep in (rnd.getrandbits(51) << 1, (rnd.getrandbits(51) << 1) | 1):         # exact ties, even and odd kept bit
            v = (((1 << 52) | keep) << (p - 52)) | half
            out += [(v, 0), (-v, 0)]
        ones = ((1 << 53) - 1) << (p - 52)                              # an all-ones 53-bit field: a round-up carries into bit 53
        for v in (ones | half, ones | half | 1, ones | (half - 1), ones | half | (half - 1), ones):
            out += [(v, 0), (-v, 0)]
    for p in range(0, 53):                                              # p <= 52: exact
        v = (1 << p) | rnd.getrandbits(p)
        out += [(1 << p, 0), (v, 0), (-v, 0)]
    out += [((1 << 53) - 1, 0), (1 << 64, 0), ((1 << 64) - 1, 0), (-(1 << 64), 0), ((1 << 64) + 1, 0), ((1 << 117) + 1, 0), ((1 << 117) + (1 << 64), 0)]
    for f in range(1, 8):                                               # every flag combination, over sums of either sign and zero
        out += [(7, f), (-7, f), (0, f), (rnd.getrandbits(120), f)]
    return out


def finalize_values(n, seed=3):
    """`n` cells: the edges first, then random v of 1 to 126 bits of either sign."""
    rnd = random.Random(seed)
    out = finalize_edges()[:n]
    while len(out) < n:
        out.append((rnd.getrandbits(rnd.randint(1, 126)) * rnd.choice([-1, 1]), 0))
    return out


def cells_array(cases):
    """[(v, flags)] -> int64 [n, 3]: the words (hi, lo, flags) of each cell as the library lays them out."""
    out = np.empty((len(cases), 3), dtype=np.int64)
    for i, (v, f) in enumerate(cases):
        out[i, 0], out[i, 1] = split(v)
        out[i, 2] = f
    return out


# ---- the test-only device harness --------------------------------------------------------------------------------------------------------
def build_devsim(force=False):
    """hipcc tests/devsim/fx_device.hip for gfx950 (cross-compiles without a GPU) into tests/devsim/_build/; returns the library's path."""
    from drt_amd import build as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "devsim", "fx_device.hip")
    out_dir = os.path.join(root, "tests", "devsim", "_build")
    so = os.path.join(out_dir, "libfx_device.so")
    os.makedirs(out_dir, exist_ok=True)
    deps = [src] + [os.path.join(B.CSRC, f) for f in os.listdir(B.CSRC) if f.endswith(".h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc] + B.FLAGS + ["-shared", "-I", B.CSRC, "-I", os.path.join(root, "include"), "-o", so, src])
    return so
