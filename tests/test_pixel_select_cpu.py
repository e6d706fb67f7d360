"""CPU tests of the pixel selector's host side (ldso_amd/csrc/pixel_select.hip): the symbols of the C-ABI, ldso_pixsel_plan against the decisions recorded
from the LDSO sources' own PixelSelector::makeMaps (tests/golden/ref_pixel_select.npz, scripts/golden/make_ref_pixel_select.py), the sizes it refuses, and
the property every fixture case must show for the GPU tests to mean something - those of the 384 x 320 cases (tests/golden/ref_pixel_select_large.npz) included."""
import os

import numpy as np
import pytest

import pixel_select_common as pc
from ldso_amd import binding, build as ldso_build

SYMBOLS = ("supported", "plan", "create", "destroy", "set_stream", "set_response", "set_settings", "set_potential", "get_potential", "make_maps", "get_map",
           "get_thresholds", "make_points", "get_points", "device", "profile")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(binding.lib_path()):
        ldso_build.build()
    return binding.lib()


def test_abi_symbols(lib):
    for s in SYMBOLS:
        assert hasattr(lib, "ldso_pixsel_" + s), s
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ldso_hip.h")).read()
    for s in SYMBOLS:
        assert f"int ldso_pixsel_{s}(" in header, s
    assert hasattr(binding, "PixelSelector")


def test_plan_equals_recorded_decisions(lib):
    g = pc.golden()
    pin, dens, pout = g["plan_in"], g["plan_density"], g["plan_out"]
    seen = dict(smaller=0, larger=0, empty=0, thinned=0, plain=0)
    for (n2, n3, n4, pot, rec), d, (action, newpot, ret, lo, hi) in zip(pin, dens, pout):
        have = int(n2) + int(n3) + int(n4)
        a, p, cth = binding.PixelSelector.plan((n2, n3, n4), float(d), int(pot), int(rec))
        if action == -1:          # an empty map whatever the potential: the recording shows only where the call ended (the counts are 0 at every potential)
            assert have == 0
            if a:
                a, p, cth = binding.PixelSelector.plan((0, 0, 0), float(d), p, int(rec) - 1)
            assert (a, p, cth) == (0, int(newpot), -1)
            seen["empty"] += 1
            continue
        assert (a, p) == (int(action), int(newpot)), (n2, n3, n4, pot, rec, d)
        if action:
            assert rec > 0
            seen["smaller" if newpot < pot else "larger"] += 1
            continue
        # charTH itself stays inside makeMaps; the recorded map pins it between the largest pattern value kept and the smallest removed
        if ret < have:
            assert lo <= cth <= hi, (cth, lo, hi)
            seen["thinned"] += 1
        else:
            assert cth == -1 or cth >= lo
            seen["plain"] += cth == -1
        seen["empty"] += have == 0
    assert all(v > 0 for v in seen.values()), seen


def test_plan_at_the_quotia_boundaries(lib):
    """quotia = density / numHave exactly 0.25, 0.95 (as a float) and 1.25, and one step to either side, in the recorded grid"""
    g = pc.golden()
    have = g["plan_in"][:, :3].sum(1)
    q = g["plan_density"][have > 0] / have[have > 0].astype(np.float32)
    for b in (0.25, 1.25):
        assert np.any(q == np.float32(b)) and np.any(q < np.float32(b)) and np.any((q > np.float32(b)) & (q < b + 1e-3))
    assert np.any((q < 0.95) & (q > 0.949)) and np.any((q >= 0.95) & (q < 0.951))
    # :133 `quotia > 1.25`, :141 `quotia < 0.25`: strict on both sides
    assert binding.PixelSelector.plan((400, 0, 0), 500.0, 3, 1)[0] == 0 and binding.PixelSelector.plan((400, 0, 0), 100.0, 3, 1)[0] == 0
    assert binding.PixelSelector.plan((400, 0, 0), 500.1, 3, 1)[:2] == (1, 2) and binding.PixelSelector.plan((400, 0, 0), 99.9, 3, 1)[:2] == (1, 7)
    assert binding.PixelSelector.plan((400, 0, 0), 500.1, 1, 1)[0] == 0          # potential 1 cannot shrink
    assert binding.PixelSelector.plan((0, 0, 0), 100.0, 3, 1)[:2] == (1, 1) and binding.PixelSelector.plan((0, 0, 0), 100.0, 3, 0) == (0, 1, -1)


def test_unsupported_sizes(lib):
    assert binding.PixelSelector.supported(640, 480) == 0 and binding.PixelSelector.supported(160, 96) == 0 and binding.PixelSelector.supported(32, 32) == 0
    for w, h in ((100, 64), (96, 70), (1232, 368)):
        assert binding.PixelSelector.supported(w, h) == binding.E_UNSUPPORTED
        assert "multiples of 32" in lib.ldso_last_error().decode()
    with pytest.raises(binding.LdsoError) as e:
        binding.PixelSelector.plan((1, 1, 1), 10.0, 0, 1)
    assert e.value.code == binding.E_INVALID and "ldso_pixsel_plan" in str(e.value)


@pytest.mark.parametrize("name", pc.CASES)
def test_fixture_properties(name):
    case = pc.load_case(name)
    calls = []
    for j, c in enumerate(case["calls"]):
        start = c["pot0"] if c["pot0"] else int(case["calls"][j - 1]["out"][5])
        calls.append(dict(out=c["out"], pot0=start, density=c["density"], rec=c["rec"]))
        assert c["map"].dtype == np.uint8 and set(np.unique(c["map"])) <= {0, 1, 2, 4}
        assert c["map"].shape == pc.image(c["image"]).shape and np.array_equal(pc.golden()["img/" + c["image"]], pc.image(c["image"]))
        assert int((c["map"] != 0).sum()) == int(c["out"][0])
        inner = c["map"][3:-4, 3:-4]          # FullSystem.cc:1290-1291
        ys, xs = np.nonzero(inner)
        assert np.array_equal(c["uv"], np.stack([xs + 3, ys + 3], 1)) and np.array_equal(c["type"], inner[ys, xs])
        if name in pc.RECORD_CASES:
            assert np.array_equal(c["imm"][:, :2], c["uv"].astype(np.float32)) and np.isfinite(c["imm"]).all()
    npass = pc.passing_level0(pc.image("steps"), case["calls"][0]["thsS"]) if name == "steps" else None
    pc.check_property(name, calls, npass)


def test_large_images_regenerate_to_the_stored_checksums():
    g = pc.golden(pc.GOLDEN_LARGE)
    assert {k[4:] for k in g.files if k.startswith("crc/")} == set(pc.LARGE_IMAGES)
    for name in pc.LARGE_IMAGES:
        a = pc.image(name)
        assert a.shape == (pc.LARGE_H, pc.LARGE_W) and a.dtype == np.uint8 and pc.crc(a) == g["crc/" + name], name
    assert g[f"pattern/{pc.LARGE_W}x{pc.LARGE_H}"].shape == (pc.LARGE_W * pc.LARGE_H,) and pc.LARGE_W * pc.LARGE_H > pc.RP_LDS
    assert np.array_equal(pc.image("stripes")[:, :pc.LARGE_W // 2], pc.image("stripes_noise")[:, :pc.LARGE_W // 2])


@pytest.mark.parametrize("name", pc.LARGE_CASES)
def test_large_fixture_properties(name):
    (c,) = pc.load_case(name, pc.GOLDEN_LARGE)["calls"]
    assert c["map"].dtype == np.uint8 and set(np.unique(c["map"])) <= {0, 1, 2, 4} and c["uv"].dtype == np.uint16 and c["th_factor"] == 1.0 and not c["response"]
    assert np.array_equal(pc.load_case(name, pc.GOLDEN_LARGE)["settings"], np.array(pc.DEFAULT_SETTINGS, np.float32))
    assert int((c["map"] != 0).sum()) == int(c["out"][0])
    inner = c["map"][3:-4, 3:-4]          # FullSystem.cc:1290-1291
    ys, xs = np.nonzero(inner)
    assert np.array_equal(c["uv"], np.stack([xs + 3, ys + 3], 1)) and np.array_equal(c["type"], inner[ys, xs])
    if name in pc.LARGE_RECORD_CASES:
        assert c["imm_every101"] is None and np.array_equal(c["imm"][:, :2], c["uv"].astype(np.float32)) and np.isfinite(c["imm"]).all()
    else:
        assert c["imm"] is None and np.array_equal(c["imm_every101"][:, :2], c["uv"][::101].astype(np.float32)) and np.isfinite(c["imm_every101"]).all()
    before = pc.load_case("large_mixed_p1", pc.GOLDEN_LARGE)["calls"][0]["map"] if name == "large_mixed_thinned" else None
    pc.check_large_property(name, c["out"], c["pot0"], c["density"], c["map"], before, c["thsS"])
    if name in ("large_stripes_p1", "large_mixed_p1"):
        assert 101 * (len(c["imm_every101"]) - 1) > pc.RP_LDS          # sampled records past rank 65 536


def test_plan_reproduces_the_large_calls(lib):
    """ldso_pixsel_plan on the counts of the five recorded 384 x 320 calls: the decision, the potential left, and for the thinned call a charTH between the largest
    pattern byte kept and the smallest removed (raster rank order over the unthinned map, ranks past 65 536 among them)"""
    g = pc.golden(pc.GOLDEN_LARGE)
    rp = g[f"pattern/{pc.LARGE_W}x{pc.LARGE_H}"].astype(np.int64)
    thinned = 0
    for name in pc.LARGE_CASES:
        (c,) = pc.load_case(name, pc.GOLDEN_LARGE)["calls"]
        ret, n2, n3, n4, used, left = (int(x) for x in c["out"])
        have = n2 + n3 + n4
        # the counts are those of the pass at `used`; a call that recursed got there with one recursion fewer for each step
        rec = c["rec"] if used == c["pot0"] else 0
        a, p, cth = binding.PixelSelector.plan((n2, n3, n4), c["density"], used, rec)
        assert (a, p) == (0, left), (name, a, p, left)
        if used != c["pot0"]:          # the first pass ran on large_natural's image at large_natural's potential: its counts are that case's
            first = pc.load_case("large_natural", pc.GOLDEN_LARGE)["calls"][0]
            assert name == "large_recurse" and c["rec"] == 2 and first["image"] == c["image"] and first["pot0"] == int(first["out"][4]) == c["pot0"]
            assert binding.PixelSelector.plan(tuple(int(x) for x in first["out"][1:4]), c["density"], c["pot0"], c["rec"])[:2] == (1, used)
        if name == "large_mixed_thinned":
            sel = np.flatnonzero(pc.load_case("large_mixed_p1", pc.GOLDEN_LARGE)["calls"][0]["map"].ravel() != 0)
            kept = c["map"].ravel()[sel] != 0
            v = rp[:len(sel)]
            lo, hi = int(v[kept].max()), int(v[~kept].min()) - 1
            assert len(sel) == have > pc.RP_LDS and lo <= cth <= hi and cth == int(np.float32(255) * pc.quotia(c["density"], (n2, n3, n4))), (cth, lo, hi)
            thinned += 1
        elif ret < have:
            assert name == "large_recurse" and cth == int(np.float32(255) * pc.quotia(c["density"], (n2, n3, n4)))
        else:
            assert cth == -1
    assert thinned == 1
