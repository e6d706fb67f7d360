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
charTH at least, charTH at most]: the recorded decisions of makeMaps (test_pixel_select_cpu.py).

tests/golden/ref_pixel_select_large.npz holds LARGE_CASES, all at 384 x 320 (122 880 bytes of pattern: more than the 64 KB k_pix_scan stages in LDS, 320 rows:
more than the 256 threads of the row scan), in the same layout with these differences: `uv` is uint16; "img/<image>" is absent and "crc/<image>" holds the
CRC32 of the image's bytes; `imm` is kept for LARGE_RECORD_CASES only, the other cases keep the records whose raster rank is a multiple of 101 as
`imm_every101`.  check_large_property says what each of these cases has to show."""
import functools
import os
import zlib

import numpy as np

import feature_detect_common as fc

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pixel_select.npz")
GOLDEN_LARGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pixel_select_large.npz")
DEFAULT_SETTINGS = (0.5, 7.0, 0.75, 1.0)          # Setting.cc:83-87
RECORD_CASES = ("natural", "response", "clipped7", "steps")
LARGE_W, LARGE_H = 384, 320
RP_LDS = 65536                                     # bytes of randomPattern k_pix_scan keeps in LDS (PIX_RP_LDS)
N2_PAST_LDS = RP_LDS + 4096                        # a level-1 count that has read the pattern well past them
LARGE_CASES = ("large_stripes_p1", "large_mixed_p1", "large_mixed_thinned", "large_natural", "large_recurse")
LARGE_RECORD_CASES = ("large_natural",)
LARGE_IMAGES = ("stripes", "stripes_noise", "large_scene")
CASES = ("natural", "recurse_smaller", "recurse_larger", "thinning", "clipped5", "clipped7", "steps", "th_factor2", "response", "no_direction", "carried")


@functools.lru_cache(maxsize=None)
def golden(path=GOLDEN):
    return np.load(path)


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
    if name in ("stripes", "stripes_noise"):
        # Vertical stripes 0, 0, 200, 200 (|dx| = 100 at every pixel) plus 0, 0, 50 down the rows: dy = -25, 25, 0 in rows y % 3 = 0, 1, 2.  A pixel of a row
        # y % 3 == 2 scores 0 under direction 0 = (0, 1) alone: its pot block's mask is 0xfffe, so a step of k_pix_scan that holds one is resolved block by
        # block.  The other rows select under every direction and move n2 on.  (Rows with dy = 0 ONLY would stop the reference's select for good at the first
        # pattern byte whose low nibble is 0: n2 stays, so the direction stays, so nothing scores again.)
        w, h = LARGE_W, LARGE_H
        a = np.tile(np.array([0, 0, 200, 200]), w // 4)[None, :] + np.tile(np.array([0, 0, 50]), h // 3 + 1)[:h, None]
        # a triangle wave of 50 per pixel: 50 * 50 lies under the level-0 threshold 55 * 55, 100 per pixel on level 1 over 0.75 * 55 * 55 -> the level-2 rule
        a[64:80, 64:84] = np.tile(np.array([0, 50, 100, 150, 200, 250, 200, 150, 100, 50]), 2)[None, :]
        if name == "stripes_noise":
            a[:, w // 2:] = np.random.default_rng(7).integers(0, 256, (h, w - w // 2))
        return np.ascontiguousarray(a.astype(np.uint8))
    if name == "large_scene":          # scene's two patches, scaled by 2.4 and 10 / 3
        a = fc.scene(LARGE_W, LARGE_H)[0].copy()
        a[27:133, 240:360] = 120.0
        yy, xx = np.mgrid[0:133, 0:144]
        a[167:300, 24:168] = 90.0 + 3.0 * np.sin(0.55 * xx) * np.sin(0.45 * yy)
        return np.ascontiguousarray(_bytes(a))
    raise KeyError(name)


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


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


def _passing(img_u8, ths_smoothed, th_factor):
    from ldso_amd import synth
    dI = synth.make_images(img_u8.astype(f32), 1)[0]
    ag = (dI[..., 1] * dI[..., 1] + dI[..., 2] * dI[..., 2]).astype(f32)
    h, w = ag.shape
    th = np.kron(np.asarray(ths_smoothed, f32).reshape(h // 32, w // 32), np.ones((32, 32), f32)).astype(f32)
    ok = ag > (th * f32(th_factor)).astype(f32)
    inside = np.zeros_like(ok)
    inside[4:h - 3, 4:w - 5] = True          # 4 <= x < w - 5, 4 <= y <= h - 4
    return ok & inside, dI


def passing_level0(img_u8, ths_smoothed, th_factor=1.0):
    """pixels inside select's border (PixelSelector2.cc:242) with absSquaredGrad[0] > thsSmoothed * thFactor, no response table: numpy, float32"""
    return int(_passing(img_u8, ths_smoothed, th_factor)[0].sum())


def chain_steps(img_u8, ths_smoothed):
    """Potential 1: (steps of k_pix_scan that hold a pot block whose mask is 0xfffe, steps whose blocks are all inside select's border).  A step is 64 pot
    blocks in the nested order = four 4 x 4 blocks = 16 columns by 4 rows here (the 96 4 x 4 blocks of a row are a multiple of four).  Mask 0xfffe: the pixel
    passes the threshold, dy == 0 and dx != 0, so that of the 16 directions only (0, 1) scores 0 - numpy on synth.make_images, as passing_level0."""
    ok, dI = _passing(img_u8, ths_smoothed, 1.0)
    h, w = ok.shape
    assert w % 64 == 0 and h % 4 == 0
    partial = (ok & (dI[..., 2] == 0) & (dI[..., 1] != 0)).reshape(h // 4, 4, w // 16, 16).any(axis=(1, 3))
    return partial, (slice(1, h // 4 - 1), slice(None))


def check_large_property(name, out, pot0, density, m, before=None, thsS=None):
    """the property of LARGE_CASES[name]; out = [ret, n2, n3, n4, used, left], m = the call's map [h, w] (any type), before = the map of large_mixed_p1 (the
    same select pass, nothing thinned) for large_mixed_thinned, thsS = the call's smoothed thresholds for large_stripes_p1"""
    ret, n2, n3, n4, used, left = (int(x) for x in out)
    q = quotia(density, (n2, n3, n4))
    m = np.asarray(m)
    assert m.shape == (LARGE_H, LARGE_W)
    if name in ("large_stripes_p1", "large_mixed_p1", "large_mixed_thinned"):
        assert used == pot0 == 1 and n2 >= N2_PAST_LDS, (name, used, n2)
    if name in ("large_stripes_p1", "large_mixed_p1"):
        assert ret == n2 + n3 + n4 == int((m != 0).sum())
        # n2 at the start of every step of k_pix_scan (chain_steps has the geometry): one step's selections use pattern bytes on both sides of the 64 KB in LDS
        per = (m == 1).reshape(LARGE_H // 4, 4, LARGE_W // 16, 16).sum(axis=(1, 3)).ravel()
        start = np.cumsum(per) - per
        assert int(per.sum()) == n2 and ((start < RP_LDS) & (start + per > RP_LDS)).any(), name
    if name == "large_stripes_p1":
        partial, inner = chain_steps(image("stripes"), thsS)
        assert n3 > 0 and partial[inner].all() and partial[inner].size >= 78 * 24, (n3, int(partial[inner].sum()))
    if name == "large_mixed_p1":          # both halves select: every step of the left one goes block by block, most of the right one's are ballots
        left_n, right_n = int((m[:, :LARGE_W // 2] == 1).sum()), int((m[:, LARGE_W // 2:] == 1).sum())
        assert left_n > 10000 and right_n > 10000, (left_n, right_n)
    if name == "large_mixed_thinned":
        b = np.asarray(before).ravel() != 0
        kept = m.ravel()[b] != 0          # in raster rank order
        assert 0 < ret < n2 + n3 + n4 == int(b.sum()) and ret == int((m != 0).sum()) == int(kept.sum()) and 0.25 <= q < 0.95, (ret, n2, n3, n4, q)
        assert not (m.ravel() != 0)[~b].any() and kept[RP_LDS:].any() and (~kept[RP_LDS:]).any()
    if name == "large_natural":
        assert used == pot0 == 3 and 0.95 <= q <= 1.25 and ret == n2 + n3 + n4 and n2 > 0 and n3 > 0 and n4 > 0, (used, q, n2, n3, n4)
        assert (m[256:] != 0).any() and (m[257::2] != 0).any()
    if name == "large_recurse":
        assert pot0 == 3 and used < 3, used


def load_case(name, path=GOLDEN):
    g = golden(path)
    calls, j = [], 0
    while f"{name}/{j}/map" in g:
        k = f"{name}/{j}/"
        ia, fa = g[k + "iargs"], g[k + "args"]
        calls.append(dict(image=str(g[k + "image"]), pot0=int(ia[0]), rec=int(ia[1]), response=bool(ia[2]), density=float(fa[0]), th_factor=float(fa[1]),
                          map=g[k + "map"], out=g[k + "out"], ths=g[k + "ths"], thsS=g[k + "thsS"], uv=g[k + "uv"], type=g[k + "type"],
                          imm=g[k + "imm"] if k + "imm" in g else None, imm_every101=g[k + "imm_every101"] if k + "imm_every101" in g else None))
        j += 1
    return dict(settings=g[f"{name}/settings"], calls=calls)
