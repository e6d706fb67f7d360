"""Undistort::undistort<T> (reference src/frontend/Undistort.cc:357-457) restated in numpy float32, for tests/test_undistort_*.py: the photometric part
(PhotometricUndistorter::processFrame, :189-227), the bilinear remap (:390-443) with the DEVICE's bounds rule (a pixel whose four taps are not all inside the
source image is 0; the reference over-reads one row for the entry xxi == 0 && yyi == hOrg - 1), the loader of tests/golden/ref_undistort.npz
(scripts/golden/make_ref_undistort.py records it from the reference's own code) and a synthetic table generator for shapes without a fixture."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, RESPONSE, VIGNETTE = 0, 1, 2
CASES = ("A", "B", "C")
EXPOSURE = 1.5          # of every recorded calibrated run
SAMPLE_ROWS = 16        # the "_rows" outputs of the fixture hold every SAMPLE_ROWS-th row of the reference's image
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "ref_undistort.npz")) as z:
            _GOLDEN = {k: z[k] for k in z.files}
        # the 65536-entry response is stored as its first differences (exact: see the recording script)
        g = _GOLDEN
        g["G65536"] = np.concatenate([g["G65536_first"].astype(np.float64), g["G65536_first"][0] + np.cumsum(g["G65536_diff"].astype(np.float64))]).astype(np.float32)
    return _GOLDEN


def case(c):
    """(wOrg, hOrg, w, h, remapX or None, remapY or None) of a recorded case as the device takes it: passthrough = no tables"""
    g = golden()
    w_org, h_org, w, h, passthrough = (int(v) for v in g[c + "_dims"])
    if passthrough:
        return w_org, h_org, w, h, None, None
    return w_org, h_org, w, h, g[c + "_remapX"], g[c + "_remapY"]


def mode_of(G, exposure, photometric_calibration):
    """which path processFrame takes (:197-198)"""
    if G is None or not exposure > 0 or photometric_calibration == 0:
        return PLAIN
    return VIGNETTE if photometric_calibration == 2 else RESPONSE


def photometric(raw, G, vignette_inv, mode, factor=1.0):
    """processFrame: one float32 per source pixel"""
    r = np.asarray(raw).ravel()
    if mode == PLAIN:
        return np.float32(factor) * r.astype(np.float32)
    d = np.asarray(G, np.float32)[r.astype(np.int64)]
    if mode == VIGNETTE:
        with np.errstate(invalid="ignore", over="ignore"):
            d = d * np.asarray(vignette_inv, np.float32).ravel()
    return d


def taps_inside(remap_x, remap_y, w_org, h_org):
    """the device's rule: entries whose four taps all lie inside the image, with their integer parts"""
    xx, yy = np.asarray(remap_x, np.float32).ravel(), np.asarray(remap_y, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        ok = (xx >= 0) & (xx < np.float32(w_org)) & (yy > np.float32(-1)) & (yy < np.float32(h_org))
    xxi, yyi = np.where(ok, xx, 0).astype(np.int32), np.where(ok, yy, 0).astype(np.int32)          # truncation, as (int)
    ok &= (xxi + 1 <= w_org - 1) & (yyi >= 0) & (yyi + 1 <= h_org - 1)
    return ok, xxi, yyi


def undistort(raw, remap_x, remap_y, w_org, h_org, w, h, G=None, vignette_inv=None, mode=PLAIN, factor=1.0):
    """the irradiance image (h, w) float32; remap_x is None: passthrough"""
    src = photometric(raw, G, vignette_inv, mode, factor)
    if remap_x is None:
        return src.reshape(h, w).copy()
    ok, xxi, yyi = taps_inside(remap_x, remap_y, w_org, h_org)
    xx = np.where(ok, np.asarray(remap_x, np.float32).ravel(), 0).astype(np.float32) - xxi.astype(np.float32)
    yy = np.where(ok, np.asarray(remap_y, np.float32).ravel(), 0).astype(np.float32) - yyi.astype(np.float32)
    o = np.where(ok, xxi + yyi * w_org, 0)
    xxyy = xx * yy
    with np.errstate(invalid="ignore", over="ignore"):
        v = xxyy * src[o + 1 + w_org] + (yy - xxyy) * src[o + w_org] + (xx - xxyy) * src[o + 1] + (np.float32(1) - xx - yy + xxyy) * src[o]
    return np.where(ok, v, np.float32(0)).astype(np.float32).reshape(h, w)


def classify(remap_x, remap_y, w_org, h_org):
    """what the REFERENCE's loop (:416-441) does with a table: entries marked invalid (xx < 0), entries its range check zeroes, entries that pass the
    check and read past the end of the source image"""
    xx, yy = np.asarray(remap_x, np.float32).ravel(), np.asarray(remap_y, np.float32).ravel()
    invalid = xx < 0
    xxi, yyi = np.where(invalid, 0, xx).astype(np.int64), np.where(invalid, 0, yy).astype(np.int64)
    off = xxi + yyi * w_org
    zeroed = ~invalid & ((off < 0) | (off > (h_org - 1) * w_org))
    over = ~invalid & ~zeroed & (off + 1 + w_org > w_org * h_org - 1)
    return dict(invalid=int(invalid.sum()), zeroed=int(zeroed.sum()), overread=int(over.sum()))


def synthetic_tables(w_org, h_org, w, h, seed=0):
    """A smooth warp of the w x h output grid into the source image that overshoots it on every side, passed through the reference's validity rule
    (:853-864, with its `iy < wOrg - 1`): for w_org > h_org the tables keep rows at and beyond h_org - 1."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    u, v = x / np.float32(max(w - 1, 1)) - np.float32(0.5), y / np.float32(max(h - 1, 1)) - np.float32(0.5)
    r2 = u * u + v * v
    k = np.float32(1.12) + np.float32(0.25) * r2
    ix = (np.float32(0.5) + u * k) * np.float32(w_org - 1) + rng.uniform(-0.3, 0.3, (h, w)).astype(np.float32)
    iy = (np.float32(0.5) + v * k) * np.float32(h_org - 1) + rng.uniform(-0.3, 0.3, (h, w)).astype(np.float32)
    ok = (ix > 0) & (iy > 0) & (ix < w_org - 1) & (iy < w_org - 1)
    return np.where(ok, ix, np.float32(-1)).astype(np.float32), np.where(ok, iy, np.float32(-1)).astype(np.float32)


def adversarial_entries(w_org, h_org):
    """(xx, yy) entries no valid table holds; the device gives 0 for each: the reference's over-reading entry, column w_org - 1 (its right-hand taps wrap
    into the next row), the last row, huge and negative values"""
    e = [(0.5, h_org - 1), (0.0, h_org - 1 + 0.5), (w_org - 1, 3.25), (w_org - 1 + 0.5, 0.5), (w_org - 1, h_org - 1), (w_org - 0.5, h_org - 2.5),
         (2.5, h_org - 0.5), (2.5, h_org), (w_org, 2.5), (1e30, 1.0), (1.0, 1e30), (3e9, 3e9), (2147483648.0, 1.0), (1.0, 2147483648.0),
         (-5.0, 3.0), (3.0, -5.0), (3.0, -1.0), (3.0, -3e9), (-1.0, -1.0), (-1e30, 2.0), (65536.0 * 65536.0, 0.0)]
    a = np.array(e, np.float32)
    return a[:, 0].copy(), a[:, 1].copy()


def textured_frames(w_org, h_org, seed=3):
    """an 8-bit and a 16-bit raw frame with texture at every scale"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h_org, 0:w_org].astype(np.float64)
    base = 128 + 60 * np.sin(x / 7.0) * np.cos(y / 5.0) + 40 * np.sin((x + 2 * y) / 23.0)
    f8 = np.clip(np.rint(base + rng.normal(0, 12, base.shape)), 0, 255).astype(np.uint8)
    f16 = (f8.astype(np.uint16) << 8) | rng.integers(0, 256, base.shape).astype(np.uint16)
    f8[0, 0], f8[-1, -1], f16[0, 0], f16[-1, -1] = 0, 255, 0, 65535
    return f8, f16
