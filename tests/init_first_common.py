"""What scripts/golden/make_ref_init_first.py and tests/test_init_first_*.py share: the inputs, the layout of tests/golden/ref_init_first.npz and the property
every recorded case has to show (asserted while recording and again by the tests).

Images are those of pixel_select_common (scene, scene_flip, small, steps, flat: 8-bit valued) plus `ramp`, a horizontal ramp of 2.5 per pixel whose gradient on
level 1 (5 per pixel) lies between the thresholds of THFac = 0.5 (3.75) and THFac = 1 (7.5): nothing is selected until makePixelStatus halves THFac.

Keys of the fixture:
  first/{frame}/meta       int32 [w, h, levels, sparsity before, sparsity after]; the frames of FRAMES are recorded in order in ONE process, so `scene_flip`
                           starts from the sparsityFactor `scene` left
  first/{frame}/n          int32 [levels] numPoints
  first/{frame}/const      float32 [idepth, iR, energy0, energy1, lastHessian, lastHessian_new, outlierTH, isGood]: the same for every record (asserted)
  first/{frame}/{l}/xy     uint8 [n, 2]: u = float32(x + 0.1), v likewise      first/{frame}/{l}/type  uint8 [n] my_type
  first/{frame}/{l}/nb     int16 [n, 10]   /par  int16 [n]   /nbd  float32 [n, 10] neighboursDist   /pard  float32 [n] parentDist
  first/{frame}/{l}/d10    float32 [n, 10] squared distances of the neighbours   /d1  float32 [n] of the parent (-1 on the coarsest level)
  status/{case}/args       float32 [desired density, THFac]     status/{case}/iargs  int32 [level, sparsity before, recsLeft]    status/{case}/image  name
  status/{case}/out        int32 [return value, passes, sparsity after]        status/{case}/map    packed bits of the bool map
  plan_in int32 [rows, 3] = n_good, sparsity, recs_left; plan_f float32 [rows, 2] = desired, THFac; plan_out int32 [rows, 2] = action (-1: not visible from
  outside makePixelStatus), sparsityFactor after the first pass
  nn/{set}/levels          int32 number of levels;  nn/{set}/{l}/xy  uint16 [n, 2];  /nb int16 [n, 10]; /par int16 [n]; /d10, /d1 as above

tests/golden/ref_init_first_large.npz holds the first/... keys of FRAMES_LARGE alone (recorded from sparsityFactor 5), xy as uint16: large_scene, 384 x 320 with 4 levels
(the coarsest is 48 x 40), whose level-0 tree is deeper than any of the other inputs' (LARGE_MIN_DEPTH)."""
import functools
import os

import numpy as np

import pixel_select_common as pc

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_init_first.npz")
GOLDEN_LARGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_init_first_large.npz")
FRAMES = (("scene", 4), ("scene_flip", 4), ("small", 3))          # (image, levels), recorded in this order
FRAMES_LARGE = (("large_scene", 4),)
LARGE_MIN_DEPTH = 10                                              # the deepest tree among FRAMES and NN_SETS is 9
DENSITIES = (f32(0.03), f32(0.05), f32(0.15), f32(0.5), f32(1))
K4 = {160: (150.0, 150.0, 79.5, 47.5), 96: (90.0, 90.0, 47.5, 31.5), 384: (360.0, 360.0, 191.5, 159.5)}
# (case, image, level, sparsity before, recsLeft, THFac, what sets the density)
STATUS_CASES = (
    ("pot1", "scene", 1, 1, 0, 1.0, 400.0), ("pot2", "scene", 1, 2, 0, 1.0, 400.0), ("pot3_clipped", "scene", 2, 3, 0, 1.0, 100.0),
    ("pot5_clipped", "small", 2, 5, 0, 1.0, 20.0), ("pot7", "scene", 1, 7, 0, 1.0, 100.0), ("pot12", "scene", 1, 12, 0, 1.0, 30.0),
    ("two_recursions", "scene", 1, 12, 5, 1.0, "search"), ("recs_exhausted", "scene", 1, 12, 1, 1.0, "as two_recursions"),
    ("th_half", "ramp", 1, 1, 5, 1.0, "search"), ("steps_ties", "steps", 1, 5, 0, 1.0, 100.0),
)
NN_SETS = ("n10", "n11", "n64", "n65", "row", "column", "grid", "clusters", "parent_outside")


@functools.lru_cache(maxsize=None)
def golden(path=GOLDEN):
    return np.load(path)


@functools.lru_cache(maxsize=None)
def image(name):
    """float32 [h, w]"""
    if name == "ramp":
        return np.ascontiguousarray(np.tile(f32(2.5) * np.arange(160, dtype=f32), (96, 1)))
    return pc.image(name).astype(f32)


def levels_of(name):
    return dict(FRAMES + FRAMES_LARGE).get(name, 3 if image(name).shape[1] == 96 else 4)


def pos(xy):
    """integer pixel positions -> (u, v) as setFirst forms them: the double sum x + 0.1 rounded to float"""
    return (np.asarray(xy, np.float64) + 0.1).astype(f32)


@functools.lru_cache(maxsize=None)
def nn_set(name):
    """integer positions per level, uint16 [n, 2]"""
    rng = np.random.default_rng(sum(map(ord, name)))

    def pick(n, w, h, x0=0, y0=0):
        i = rng.choice(w * h, n, replace=False)
        i.sort()          # raster order, as setFirst leaves the records
        return np.stack([x0 + i % w, y0 + i // w], 1).astype(np.uint16)
    if name in ("n10", "n11", "n64", "n65"):
        return [pick(int(name[1:]), 40, 24)]
    if name == "row":
        return [np.stack([np.arange(3, 53), np.full(50, 7)], 1).astype(np.uint16)]
    if name == "column":
        return [np.stack([np.full(50, 9), np.arange(3, 53)], 1).astype(np.uint16)]
    if name == "grid":
        yy, xx = np.mgrid[0:24, 0:40]
        y2, x2 = np.mgrid[0:12, 0:20]
        return [np.stack([xx.ravel(), yy.ravel()], 1).astype(np.uint16), np.stack([x2.ravel(), y2.ravel()], 1).astype(np.uint16)]
    if name == "clusters":
        return [np.concatenate([pick(30, 8, 8, 2, 2), pick(30, 8, 8, 500, 300)]).astype(np.uint16)]
    if name == "parent_outside":
        return [pick(120, 100, 60), pick(20, 6, 6, 30, 20)]
    raise KeyError(name)


def parent_query(uv):
    """pt * 0.5f - (0.25f, 0.25f), CoarseInitializer.cc:766"""
    return (np.asarray(uv, f32) * f32(0.5) - f32(0.25)).astype(f32)


def tie_share(d10, d11):
    """share of rows whose 10th and 11th squared distances are equal"""
    return float(np.mean(np.asarray(d10) == np.asarray(d11)))


def tidy_order(uv, k=10):
    """the k nearest by (squared distance in float32 as the reference forms it, index): what a tie rule by index would give"""
    uv = np.asarray(uv, f32)
    d0 = (uv[:, None, 0] - uv[None, :, 0]).astype(f32)
    d1 = (uv[:, None, 1] - uv[None, :, 1]).astype(f32)
    d = ((d0 * d0).astype(f32) + (d1 * d1).astype(f32)).astype(f32)
    idx = np.argsort(d, axis=1, kind="stable")
    return idx[:, :k + 1], np.take_along_axis(d, idx[:, :k + 1], 1)


def block_has_tie(dI, pot, th_fac=1.0):
    """True when some pot x pot block of gridMaxSelection on the level image dI [h, w, 3] holds its maximal |dx| (among the pixels over the threshold) twice"""
    h, w = dI.shape[:2]
    th = f32(th_fac) * f32(10) * f32(0.75)
    ok = (dI[..., 1] * dI[..., 1] + dI[..., 2] * dI[..., 2]).astype(f32) > th * th
    a = np.where(ok, np.abs(dI[..., 1]), f32(0))
    for y in range(1, h - pot, pot):
        for x in range(1, w - pot, pot):
            b = a[y:y + pot, x:x + pot]
            if b.max() > 0 and int((b == b.max()).sum()) > 1:
                return True
    return False


def check_status_property(case, w, h, pot0, out, rec, natural_passes):
    """out = [return value, passes, sparsity after]; natural_passes = the passes of the same call with recsLeft 5"""
    ret, passes, left = (int(x) for x in out)
    if case.startswith("pot") or case == "steps_ties":
        assert rec == 0 and passes == 1 and ret > 0, (case, out)
    if case.endswith("_clipped"):
        assert 1 + ((w - 2) // pot0) * pot0 < w - 1 and 1 + ((h - 2) // pot0) * pot0 < h - 1, (w, h, pot0)          # pixels inside the border that no block covers
    if case == "two_recursions":
        assert passes >= 3, out
    if case == "recs_exhausted":
        assert rec == 1 and passes == 2 and natural_passes > 2, (out, natural_passes)
    if case == "th_half":
        assert passes >= 2 and pot0 == 1 and left >= 1, out


def load_frame(name, path=GOLDEN):
    g = golden(path)
    k = f"first/{name}/"
    meta = [int(x) for x in g[k + "meta"]]
    lv = []
    for l in range(meta[2]):
        q = f"{k}{l}/"
        lv.append({s: g[q + s] for s in ("xy", "type", "nb", "par", "nbd", "pard", "d10", "d1")})
    return dict(w=meta[0], h=meta[1], levels=meta[2], sparsity_in=meta[3], sparsity_out=meta[4], n=g[k + "n"], const=g[k + "const"], lv=lv)


def load_nn(name):
    g = golden()
    out = []
    for l in range(int(g[f"nn/{name}/levels"])):
        q = f"nn/{name}/{l}/"
        out.append({s: g[q + s] for s in ("xy", "nb", "par", "d10", "d1")})
    return out


def nn_inputs():
    """every position set of the tree tests: name -> list of float32 [n, 2] per level (the recorded setFirst levels and the synthetic sets)"""
    sets = {}
    for name, _ in FRAMES:
        sets["first/" + name] = ([pos(lv["xy"]) for lv in load_frame(name)["lv"]], load_frame(name)["lv"])
    for name, _ in FRAMES_LARGE:
        lv = load_frame(name, GOLDEN_LARGE)["lv"]
        sets["first/" + name] = ([pos(a["xy"]) for a in lv], lv)
    for name in NN_SETS:
        sets["nn/" + name] = ([pos(a) for a in nn_set(name)], load_nn(name))
    return sets
