"""What scripts/golden/make_ref_pixel_select.py and tests/test_pixel_select_*.py share: the test images (8-bit valued, so that the fixture stores them as
bytes), the layout of tests/golden/ref_pixel_select.npz and the property every fixture case has to show.

The fixture holds, per case, a sequence of makeMaps calls on one PixelSelector (all but `carried` have one call).  Keys of call j of case `name`:
  {name}/{j}/image  name of the image ("img/<image>" holds it)      {name}/{j}/args   float32 [density, th_factor]
  {name}/{j}/iargs  int32 [potential set before the call or 0 = carried, recursions_left, response table 0/1]
  {name}/{j}/map    uint8 [h, w]       {name}/{j}/out  int32 [return value, n2, n3, n4, potential used, potential left]
  {name}/{j}/ths, /thsS  float32       {name}/{j}/uv  uint8 [k, 2], {name}/{j}/type  uint8 [k]: position and my_type of every ImmaturePoint, raster order
  {name}/{j}/imm    float32 [k, 23] = u, v, color[8], weights[8], gradH[4], energyTH of the same points (RECORD_CASES only)
  {name}/settings   float32 [minGradHistCut, minGradHistAdd, gradDownweightPerLevel, selectDirectionDistribution]
pattern/<w>x<h> is PixelSelector::randomPattern; plan_in [n2, n3, n4, potential, recursions_left] / plan_density / plan_out [recursed (-1: not visible), potential of the next pass or left, return value,
charTH at least, charTH at most]: the recorded decisions of makeMaps (test_pixel_select_cpu.py)."""
import functools
import os

import numpy as np

import feature_detect_common as fc

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pixel_select.npz")
DEFAULT_SETTINGS = (0.5, 7.0, 0.75, 1.0)          # Setting.cc:83-87
RECORD_CASES = ("natural", "response", "clipped7", "steps")
CASES = ("natural", "recurse_smaller", "recurse_larger", "thinning", "clipped5", "clipped7", "steps", "th_factor2", "response", "no_direction", "carried")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


def _bytes(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def image(name):
    """the test images, uint8 [h, w]"""
    if name in ("scene", "scene_flip", "scene_mirror"):
        a = fc.scene(160, 96)[0].copy()
        a[8:40, 100:150] = 120.0                                                     # a flat patch
        yy, xx = np.mgrid[0:40, 0:60]
        a[50:90, 10:70] = 90.0 + 3.0 * np.sin(0.55 * xx) * np.sin(0.45 * yy)         # weak texture: below the level-0 threshold, found on levels 1 and 2
        a = _bytes(a)
        return np.ascontiguousarray({"scene": a, "scene_flip": a[::-1], "scene_mirror": a[:, ::-1]}[name])
    if name == "small":
        return _bytes(fc.scene(96, 64)[0])
    if name == "steps":
        rng = np.random.default_rng(11)
        return np.ascontiguousarray(np.kron(rng.integers(40, 216, (8, 12)), np.ones((8, 8))).astype(np.uint8))          # 96 x 64, axis-aligned step edges
    if name == "flat":
        return np.full((96, 160), 100, np.uint8)
    raise KeyError(name)


def steps_image(w, h, seed=11):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.kron(rng.integers(40, 216, (h // 8, w // 8)), np.ones((8, 8))).astype(np.uint8))


def quotia(density, counts):
    return f32(density) / f32(int(np.sum(counts)))


def check_property(name, calls, numpy_passing=None):
    """the property the issue lists for case `name`; calls: list of dict(out=[ret, n2, n3, n4, used, left], pot0, density, rec)"""
    c = calls[0]
    ret, n2, n3, n4, used, left = (int(x) for x in c["out"])
    q = quotia(c["density"], (n2, n3, n4))
    if name in ("natural", "th_factor2", "response", "no_direction"):
        assert used == c["pot0"] == 3 and 0.95 <= q <= 1.25 and ret == n2 + n3 + n4, (name, q, used)
    if name == "natural":
        assert n2 > 0 and n3 > 0 and n4 > 0, (n2, n3, n4)
    if name == "recurse_smaller":
        assert used < c["pot0"], (used, c["pot0"])
    if name == "recurse_larger":
        assert used >= 12 and used > c["pot0"], (used, c["pot0"])
    if name == "thinning":
        assert used == c["pot0"] and 0.25 <= q < 0.95 and 0 < ret < n2 + n3 + n4, (q, ret, n2 + n3 + n4)
    if name in ("clipped5", "clipped7"):
        pot = 5 if name == "clipped5" else 7
        assert c["rec"] == 0 and used == pot and 96 % pot and 64 % pot and 96 % (4 * pot) and n2 > 0
    if name == "steps":
        assert c["rec"] == 0 and used == 1 and numpy_passing is not None and n2 < numpy_passing, (n2, numpy_passing)
    if name == "carried":
        assert len(calls) == 3 and all(calls[j]["pot0"] == int(calls[j - 1]["out"][5]) for j in (1, 2))          # each call starts from what the one before left
        assert int(calls[0]["out"][5]) != 3 and int(calls[1]["out"][5]) != int(calls[0]["out"][5])                     # ... and the potential moves


def passing_level0(img_u8, ths_smoothed, th_factor=1.0):
    """pixels inside select's border (PixelSelector2.cc:242) with absSquaredGrad[0] > thsSmoothed * thFactor, no response table: numpy, float32"""
    from ldso_amd import synth
    dI = synth.make_images(img_u8.astype(f32), 1)[0]
    ag = (dI[..., 1] * dI[..., 1] + dI[..., 2] * dI[..., 2]).astype(f32)
    h, w = ag.shape
    th = np.kron(np.asarray(ths_smoothed, f32).reshape(h // 32, w // 32), np.ones((32, 32), f32)).astype(f32)
    ok = ag > (th * f32(th_factor)).astype(f32)
    inside = np.zeros_like(ok)
    inside[4:h - 3, 4:w - 5] = True          # 4 <= x < w - 5, 4 <= y <= h - 4
    return int((ok & inside).sum())


def load_case(name):
    g = golden()
    calls, j = [], 0
    while f"{name}/{j}/map" in g:
        k = f"{name}/{j}/"
        ia, fa = g[k + "iargs"], g[k + "args"]
        calls.append(dict(image=str(g[k + "image"]), pot0=int(ia[0]), rec=int(ia[1]), response=bool(ia[2]), density=float(fa[0]), th_factor=float(fa[1]),
                          map=g[k + "map"], out=g[k + "out"], ths=g[k + "ths"], thsS=g[k + "thsS"], uv=g[k + "uv"], type=g[k + "type"],
                          imm=g[k + "imm"] if k + "imm" in g else None))
        j += 1
    return dict(settings=g[f"{name}/settings"], calls=calls)
