"""The float32 cloud rule: a float32 cloud is the float64 cloud converted once, round to nearest
even, coordinate by coordinate.

The float32 fused instances compute in fp64 exactly as the float64 ones do and convert on the
store (csrc/triangulate.h ``tri_store``, phase D of ``main3_kernel``), and the float64 result is
pinned to the oracle bit for bit, so the float32 result is pinned too: ``oracle.astype(float32)``.
NumPy's ``astype`` is the C cast, round to nearest even.  The 1e-4 relative bound of
BASELINE.json stays the promise to users; the suite pins the stronger fact.
"""
import numpy as np

_F32_MIN_NORMAL = np.float32(2.0 ** -126)


def ulp_distance32(a, b):
    """Distance in float32 steps between two float32 arrays, for the failure report (-0.0 and
    +0.0 are 0 apart here; the bit comparison is what tells them apart)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def assert_xyz32_exact(got32, want64, what=""):
    """``got32`` (float32) equals ``want64`` (float64, from the reference) rounded once, bit for
    bit, the sign of a zero included."""
    got32, want64 = np.asarray(got32), np.asarray(want64)
    assert got32.dtype == np.float32, (what, got32.dtype)
    assert want64.dtype == np.float64, (what, want64.dtype)
    assert got32.shape == want64.shape, (what, got32.shape, want64.shape)
    with np.errstate(over="ignore"):
        want32 = want64.astype(np.float32)
    # a condition on the inputs, decided by the reference alone: the rule is stated for values
    # float32 holds as normal numbers (or zero)
    assert np.all(np.isfinite(want32)), (what, "the reference cloud overflows float32")
    assert not np.any((want32 != 0) & (np.abs(want32) < _F32_MIN_NORMAL)), \
        (what, "the reference cloud is subnormal in float32")
    g = np.ascontiguousarray(got32).view(np.uint32)
    w = np.ascontiguousarray(want32).view(np.uint32)
    bad = g != w
    if bad.any():
        flat = np.flatnonzero(bad.ravel())
        first = int(flat[0])
        with np.errstate(invalid="ignore"):
            ulps = ulp_distance32(got32.ravel()[flat], want32.ravel()[flat])
        raise AssertionError(
            f"{what}: {flat.size} of {bad.size} float32 coordinates differ from the float64 "
            f"reference rounded once; first at flat index {first} (got {got32.ravel()[first]!r} = "
            f"0x{int(g.ravel()[first]):08x}, want {want32.ravel()[first]!r} = 0x{int(w.ravel()[first]):08x}, "
            f"float64 {want64.ravel()[first]!r}); largest distance {int(ulps.max())} ulp")
