"""numpy restatement of the reference's 'Theory' and 's2vec_*' encoders (positional_encoding/theory.py,
sphere2vec/sphere2vec.py) for an arbitrary frequency table: what the GPU tests compare the kernel with
at shapes the fixture does not hold.  tests/test_posenc_cpu.py pins it to the fixture.

Coordinates are (lon, lat) in degrees, used as radians like the reference does.  x = lon, y = lat,
al = x * f[i], at = y * f[i] (one float64 multiply each).

``defect``: a planted mistake (None: none), for the tests that show the fixture catches it -
'swap' (two terms exchanged), 'nodup' (the sphere kinds' duplication dropped: narrower rows),
'fma' (Theory's angles as one fused multiply-add, emulated in long double).
"""
from __future__ import annotations

import numpy as np

KINDS = ("theory", "grid", "spherec", "spherecplus", "spherem", "spheremplus")
PER_FREQ = {"theory": 6, "grid": 4, "spherec": 6, "spherecplus": 12, "spherem": 10, "spheremplus": 16}
KIND_OF_MODEL = {"Theory": "theory", "s2vec_grid": "grid", "s2vec_spherec": "spherec",
                 "s2vec_spherecplus": "spherecplus", "s2vec_spherem": "spherem",
                 "s2vec_spheremplus": "spheremplus"}
S3H = np.sqrt(3.0) / 2.0


def _fma_angle(x, y, ux, uy):
    """x*ux + y*uy with ONE rounding of the second product and the sum (what a contracted FMA gives)."""
    ld = np.longdouble
    return (ld(x * ux) + ld(y) * ld(uy)).astype(np.float64)


def encode(kind: str, lonlat, freq, defect=None) -> np.ndarray:
    q = np.asarray(lonlat, dtype=np.float64)
    f = np.asarray(freq, dtype=np.float64)
    B, F = q.shape[0], f.shape[0]
    x, y = q[:, 0:1], q[:, 1:2]
    with np.errstate(invalid="ignore"):
        if kind == "theory":
            units = ((1.0, 0.0), (-0.5, S3H), (-0.5, -S3H))
            if defect == "fma":
                ang = [_fma_angle(x, y, ux, uy) for ux, uy in units]
            else:
                ang = [x * ux + y * uy for ux, uy in units]
            cols = []
            for a in ang:
                t = a * f[None, :]
                cols += [np.sin(t), np.cos(t)]
            if defect == "swap":
                cols[0], cols[1] = cols[1], cols[0]
            return np.stack(cols, axis=-1).reshape(B, 6 * F)            # out[6 i + j]
        al, at = x * f[None, :], y * f[None, :]
        sal, cal, sat, cat = np.sin(al), np.cos(al), np.sin(at), np.cos(at)
        if kind == "grid":
            lon = [sal, cal]
            if defect == "swap":
                lon = lon[::-1]
            return np.concatenate([np.stack(lon, axis=-1).reshape(B, 2 * F),
                                   np.stack([sat, cat], axis=-1).reshape(B, 2 * F)], axis=1)
        if kind == "spherec":
            terms = [sat, cat * cal, cat * sal]
        elif kind == "spherecplus":
            terms = [sat, cat, sal, cal, cat * cal, cat * sal]
        else:
            sx, cx, cy = np.sin(x), np.cos(x), np.cos(y)
            tail = [sat, cat * cx, cy * cal, cat * sx, cy * sal]
            if kind == "spherem":
                terms = tail
            elif kind == "spheremplus":
                terms = [sat, cat, sal, cal] + tail[1:]
            else:
                raise ValueError(kind)
        if defect == "swap":
            terms[1], terms[2] = terms[2], terms[1]
        t = np.stack(terms, axis=-1)                                     # (B, F, T)
        if defect == "nodup":
            return t.reshape(B, -1)
        return np.repeat(t, 2, axis=-1).reshape(B, -1)                   # out[i 2T + 2t + r]


def width(kind: str, F: int) -> int:
    return PER_FREQ[kind] * F


def max_argument(kind: str, freq) -> float:
    """Largest |argument| of a sine / cosine over |lon| <= 180, |lat| <= 90 (the own-table rule of the
    tests: one ulp of a frequency moves an output by 2^-52 times this)."""
    fmax = float(np.max(np.abs(freq)))
    if kind == "theory":
        return 180.0 * (0.5 + S3H) * fmax
    return 180.0 * max(fmax, 1.0)


# Bounds (derived, not tuned): a single sine / cosine 4e-16 (what the Wrap test grants a libm; numpy's and
# torch's differ by 1.1e-16 on these arguments); a product of two 2 * 4e-16 + 1.2e-16 -> 1e-15; float32
# results after rounding 6e-8 (one float32 ulp at 1).  They hold for a kernel given the SAME frequency
# table as the reference; `widen` is for a table that differs from it in the last bit (own_table_widen).
ATOL_SINGLE, ATOL_PRODUCT, ATOL_F32 = 4e-16, 1e-15, 6e-8


def product_mask(kind: str, F: int) -> np.ndarray:
    """Per output column: True where the entry is a product of two sines / cosines."""
    per = {"theory": [0] * 6, "grid": [0] * 4, "spherec": [0, 0, 1, 1, 1, 1],
           "spherecplus": [0] * 8 + [1] * 4, "spherem": [0, 0] + [1] * 8, "spheremplus": [0] * 8 + [1] * 8}[kind]
    if kind == "grid":
        return np.zeros(4 * F, dtype=bool)
    return np.tile(np.array(per, dtype=bool), F)


def assert_close(kind, got, ref, widen=0.0):
    """``got`` against ``ref`` at the bounds above (plus ``widen``), NaN positions equal."""
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    if ref.dtype == np.float32:
        atol = np.full(ref.shape[1], ATOL_F32)
    else:
        atol = np.where(product_mask(kind, ref.shape[1] // PER_FREQ[kind]), ATOL_PRODUCT, ATOL_SINGLE) + widen
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ok = np.isnan(ref) | (err <= atol[None, :])
    assert ok.all(), f"{kind}: max err {np.nanmax(err):.3e}"


def own_table_widen(kind: str, own, fixture) -> float:
    """The own-table rule: ``own`` must agree with the fixture's table within one ulp; bitwise equal keeps
    the tight bounds (0.0), else one ulp of a frequency moves an output by 2^-52 * max |argument|."""
    own, fixture = np.asarray(own), np.asarray(fixture)
    assert own.shape == fixture.shape and (np.abs(own - fixture) <= np.spacing(np.abs(fixture))).all()
    return 0.0 if np.array_equal(own, fixture) else 2.0 ** -52 * max_argument(kind, fixture)
