"""GPU tests of ldso_amd/csrc/init_first.hip: CoarseInitializer::setFirst from a resident pyramid - makePixelStatus, the records and makeNN on the device - against
the fixture recorded from the LDSO sources (tests/golden/ref_init_first.npz, scripts/golden/make_ref_init_first.py).  Maps, counts, positions, indices and squared
distances are integers or the result of the same IEEE operations in the same order: exact equality.  The three weight fields (neighboursDist, parentDist) go
through expf, which neither library rounds correctly (both document at most 1 ulp): two expf results can differ by 2 ulp, their sums by about as much, then one
division and one multiplication each round - about 6 ulp, so the limit is 1e-6 relative.  The largest deviation seen is printed.
Shapes: 160 x 96 with 4 levels (the coarsest is 20 x 12) and 96 x 64 with 3; one frame of 384 x 320 with 4 levels (tests/golden/ref_init_first_large.npz: the
selector's 64 KB pattern staging and 320 rows, 4000-6000 records a level, a level-0 tree deeper than 9)."""
import numpy as np
import pytest

import init_first_common as ic
import pixel_select_common as pc
from ldso_amd import binding, synth

pytestmark = pytest.mark.gpu
f32 = np.float32
WEIGHT_RTOL = 1e-6
DEVICE_FIELDS = [n for n in synth.INIT_POINT_DTYPE.names if n not in ("neighboursDist", "parentDist", "my_type", "pad_")]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def make_pyr(img, levels):
    h, w = img.shape
    return binding.Pyramid(w, h, max(levels, 3)).make_images(np.ascontiguousarray(img, f32))


def selector(w, h, path=pc.GOLDEN):
    return binding.PixelSelector(w, h, pc.golden(path)[f"pattern/{w}x{h}"])


@pytest.mark.parametrize("case", [c[0] for c in ic.STATUS_CASES])
def test_pixel_status_equals_the_reference(case):
    g = ic.golden()
    k = f"status/{case}/"
    name = str(g[k + "image"])
    (dens, thf), (lvl, sp, rec) = g[k + "args"], (int(x) for x in g[k + "iargs"])
    ret, passes, left = (int(x) for x in g[k + "out"])
    img = ic.image(name)
    h, w = img.shape
    levels = ic.levels_of(name)
    pyr, ini = make_pyr(img, levels), binding.Initializer(w, h, levels)
    ini.sparsity = sp
    n, ps = ini.pixel_status(pyr, lvl, float(dens), rec, float(thf))
    m = ini.status_map()
    ref = np.unpackbits(g[k + "map"])[:(h >> lvl) * (w >> lvl)].reshape(h >> lvl, w >> lvl)
    left_dev = ini.sparsity
    print(case, "device", (n, ps, left_dev), "reference", (ret, passes, left), "map differences", int((m != ref).sum()))
    natural = ps
    if case == "recs_exhausted":
        ini.sparsity = sp
        natural = ini.pixel_status(pyr, lvl, float(dens), 5, float(thf))[1]
    ic.check_status_property(case, w >> lvl, h >> lvl, sp, (n, ps, left_dev), rec, natural)
    if case == "steps_ties":
        assert ic.block_has_tie(pyr.get_level(lvl).reshape(h >> lvl, w >> lvl, 3), sp, float(thf))
    assert np.array_equal(m, ref)
    assert (n, ps, left_dev) == (ret, passes, left)
    assert n == int(ref.sum())
    ini.close(); pyr.close()


NN = None


def nn_inputs():
    global NN
    if NN is None:
        NN = ic.nn_inputs()
    return NN


@pytest.mark.parametrize("name", ["first/" + n for n, _ in ic.FRAMES + ic.FRAMES_LARGE] + ["nn/" + n for n in ic.NN_SETS])
def test_make_nn_equals_the_host_search(name):
    uv, ref = nn_inputs()[name]
    ini = binding.Initializer(160, 96, 4)
    dev = ini.make_nn(uv)
    trees = [binding.NNTree(a) for a in uv]
    for l, a in enumerate(uv):
        idx, d = trees[l].search(a, 10)
        assert np.array_equal(dev[l][0], idx) and np.array_equal(bits(dev[l][1]), bits(d)), (name, l)
        assert np.array_equal(idx, ref[l]["nb"].astype(np.int32))
        if l + 1 < len(uv):
            pidx, pd = trees[l + 1].search(ic.parent_query(a), 1)
            assert np.array_equal(dev[l][2], pidx[:, 0]) and np.array_equal(bits(dev[l][3]), bits(pd[:, 0])), (name, l)
            assert np.array_equal(pidx[:, 0], ref[l]["par"].astype(np.int32))
        else:
            assert np.all(dev[l][2] == -1) and np.all(dev[l][3] == -1)
    ini.close()


def test_make_nn_refuses_a_level_with_fewer_than_10_points():
    ini = binding.Initializer(160, 96, 4)
    with pytest.raises(binding.LdsoError) as e:
        ini.make_nn([ic.pos(ic.nn_set("n11")[0])[:9]])
    assert e.value.code == -4
    assert np.array_equal(ini.make_nn([ic.pos(ic.nn_set("n10")[0])])[0][0], ic.load_nn("n10")[0]["nb"])
    ini.close()


def check_frame(ini, n, name, path=ic.GOLDEN):
    """every record field of every level against the recorded setFirst; returns the largest relative deviation of the weight fields"""
    r = ic.load_frame(name, path)
    assert list(n) == [int(x) for x in r["n"]] and ini.sparsity == r["sparsity_out"], (n, r["n"], ini.sparsity, r["sparsity_out"])
    idepth, iR, e0, e1, lh, lhn, oth, good = (float(x) for x in r["const"])
    worst = 0.0
    for l, lv in enumerate(r["lv"]):
        p = ini.points(l)
        uv = ic.pos(lv["xy"])
        assert np.array_equal(bits(p["u"]), bits(uv[:, 0])) and np.array_equal(bits(p["v"]), bits(uv[:, 1]))
        assert np.all(p["idepth"] == idepth) and np.all(p["iR"] == iR) and np.all(p["isGood"] == int(good)) and np.all(p["energy"] == np.array([e0, e1], f32))
        assert np.all(p["lastHessian"] == lh) and np.all(p["lastHessian_new"] == lhn) and np.all(p["outlierTH"] == oth)
        assert np.array_equal(p["my_type"], lv["type"].astype(f32))
        assert np.array_equal(p["neighbours"], lv["nb"].astype(np.int32)) and np.array_equal(p["parent"], lv["par"].astype(np.int32))
        # the members the reference leaves uninitialised: the rule of LDSO_INIT_POINT_FILL_UNSET
        assert np.all(p["idepth_new"] == 1) and np.all(p["maxstep"] == 0) and np.all(p["iRSumNum"] == 0) and np.all(p["isGood_new"] == 0)
        assert np.all(p["energy_new"] == 0) and np.all(p["pad_"] == 0)
        dev = np.abs(p["neighboursDist"].astype(np.float64) - lv["nbd"]) / np.abs(lv["nbd"])
        worst = max(worst, float(dev.max()))
        if l + 1 < len(r["lv"]):
            worst = max(worst, float((np.abs(p["parentDist"].astype(np.float64) - lv["pard"]) / np.abs(lv["pard"])).max()))
        else:
            assert np.all(p["parentDist"] == -1)
    return worst


def test_set_first_frame_equals_the_reference_and_carries_the_sparsity():
    """scene, then scene_flip on the same handle (the reference recorded them in one process: the second starts from the sparsityFactor the first left), then small"""
    worst = 0.0
    ini, sel = binding.Initializer(160, 96, 4), selector(160, 96)
    assert ini.sparsity == 5
    for name in ("scene", "scene_flip"):
        assert ini.sparsity == ic.load_frame(name)["sparsity_in"]
        pyr = make_pyr(ic.image(name), 4)
        n = ini.set_first_frame(ic.K4[160], pyr, sel)
        worst = max(worst, check_frame(ini, n, name))
        pyr.close()
    ini.close(); sel.close()
    ini, sel = binding.Initializer(96, 64, 3), selector(96, 64)
    ini.sparsity = ic.load_frame("small")["sparsity_in"]
    pyr = make_pyr(ic.image("small"), 3)
    worst = max(worst, check_frame(ini, ini.set_first_frame(ic.K4[96], pyr, sel), "small"))
    print("largest relative deviation of neighboursDist / parentDist:", worst)
    assert worst <= WEIGHT_RTOL
    ini.close(); sel.close(); pyr.close()


def test_set_first_frame_large():
    """large_scene, 384 x 320 with 4 levels, from the sparsityFactor 5 of a new handle"""
    w, h = pc.LARGE_W, pc.LARGE_H
    r = ic.load_frame("large_scene", ic.GOLDEN_LARGE)
    assert (r["w"], r["h"], r["levels"], r["sparsity_in"]) == (w, h, 4, 5)
    tree = binding.NNTree(ic.pos(r["lv"][0]["xy"]))
    print("depth of the level-0 tree:", tree.depth, "records per level:", [int(x) for x in r["n"]])
    assert tree.depth >= ic.LARGE_MIN_DEPTH          # the search's stack goes deeper than with any other input of the suite
    tree.close()
    ini, sel = binding.Initializer(w, h, 4), selector(w, h, pc.GOLDEN_LARGE)
    assert ini.sparsity == 5
    pyr = make_pyr(ic.image("large_scene"), 4)
    n = ini.set_first_frame(ic.K4[w], pyr, sel)
    assert (sel.get_map()[256:] != 0).any()          # level 0 selects in the rows the row scan's threads reach second
    worst = check_frame(ini, n, "large_scene", ic.GOLDEN_LARGE)
    print("largest relative deviation of neighboursDist / parentDist:", worst)
    assert worst <= WEIGHT_RTOL
    ini.close(); sel.close(); pyr.close()


def test_two_calls_leave_identical_records_and_maps():
    ini, sel = binding.Initializer(160, 96, 4), selector(160, 96)
    pyr = make_pyr(ic.image("scene"), 4)
    got = []
    for _ in range(2):
        ini.sparsity = 5
        n = ini.set_first_frame(ic.K4[160], pyr, sel)
        got.append((n, [ini.points(l).tobytes() for l in range(4)], sel.get_map().tobytes(), ini.status_map().tobytes(), ini.sparsity))
    assert got[0] == got[1]
    ini.close(); sel.close(); pyr.close()


def test_tracking_equals_the_path_through_set_first():
    """The records of set_first_frame handed to a second handle through ldso_init_set_first with the same frame as a host image; three frames tracked on both.
    States and the records' device-resident fields are byte-identical after every frame; the three fields the device does not carry (the weights and my_type)
    keep, on the first handle, exactly what set_first_frame built."""
    w, h, L = 160, 96, 4
    seq = synth.make_init_sequence(w, h, n_frames=3, fx=400.0 * w / 640, levels=L)
    assert seq["levels"] == L
    a, b, sel = binding.Initializer(w, h, L), binding.Initializer(w, h, L), selector(w, h)
    pyr = make_pyr(seq["first"], L)
    a.set_first_frame(seq["K4"], pyr, sel)
    recs = [a.points(l) for l in range(L)]
    b.set_first(seq["K4"], seq["first"], recs)
    for k in range(3):
        sa, sb = a.track_frame(seq["frames"][k], 1.0), b.track_frame(seq["frames"][k], 1.0)
        assert sa.tobytes() == sb.tobytes(), k
        for l in range(L):
            pa, pb = a.points(l), b.points(l)
            for f in DEVICE_FIELDS:
                assert pa[f].tobytes() == pb[f].tobytes(), (k, l, f)
            for f in ("neighboursDist", "parentDist", "my_type"):
                assert pa[f].tobytes() == recs[l][f].tobytes(), (k, l, f)
    for x in (a, b, sel, pyr):
        x.close()


def test_error_cases_leave_the_handle_usable():
    # more than 5 levels: no such handle exists - ldso_init_create refuses it, which is where the entry's own check would otherwise be reached
    with pytest.raises(binding.LdsoError):
        binding.Initializer(192, 128, 6)
    ini, sel = binding.Initializer(160, 96, 4), selector(160, 96)
    good = make_pyr(ic.image("scene"), 4)

    def good_frame():
        ini.sparsity = 5
        assert check_frame(ini, ini.set_first_frame(ic.K4[160], good, sel), "scene") <= WEIGHT_RTOL
        assert ini.track_frame(ic.image("scene_flip"), 1.0)["frameID"] == 1          # the handle tracks from it

    # the flat image leaves fewer than 10 records per level
    flat = make_pyr(ic.image("flat"), 4)
    with pytest.raises(binding.LdsoError) as e:
        ini.set_first_frame(ic.K4[160], flat, sel)
    assert e.value.code == -4
    with pytest.raises(binding.LdsoError):
        ini.track_frame(ic.image("scene"), 1.0)          # no first frame after the refusal
    good_frame()
    # a NaN pixel
    img = ic.image("scene").copy()
    img[40, 70] = np.nan
    bad = make_pyr(img, 4)
    with pytest.raises(binding.LdsoError) as e:
        ini.set_first_frame(ic.K4[160], bad, sel)
    assert e.value.code == -3
    good_frame()
    # on the coarser levels the NaN never reaches a gradient: makeImages zeroes a non-finite dx / dy (FrameHessian.cc:86-87), so the stage entry selects around it
    ini.sparsity = 2
    ini.pixel_status(bad, 1, 400.0, 0, 1.0)
    lv1 = bad.get_level(1)
    assert np.isnan(lv1[..., 0]).any() and np.isfinite(lv1[..., 1:]).all() and ini.status_map().sum() > 0
    # a size that is no multiple of 32: no selector exists for it, the code is the selector's
    assert binding.PixelSelector.supported(176, 96) == -4
    with pytest.raises(binding.LdsoError) as e:
        binding.PixelSelector(176, 96, np.zeros(176 * 96, np.uint8))
    assert e.value.code == -4
    for x in (ini, sel, good, flat, bad):
        x.close()
