"""GPU tests of ldso_amd/csrc/pixel_select.hip: PixelSelector::makeMaps and the points of FullSystem::makeNewTraces (setting_pointSelection == 0) on the device
against the fixture recorded from the LDSO sources (tests/golden/ref_pixel_select.npz).  Everything compared is an integer or the result of the same IEEE
operations in the same order: exact equality, no tolerance.  Three-level pyramids of 160 x 96 and 96 x 64, and of 384 x 320 for pc.LARGE_CASES
(tests/golden/ref_pixel_select_large.npz): 122 880 bytes of random pattern, of which k_pix_scan stages the first 65 536 in LDS and reads the rest from global
memory, 320 rows for the row scan's 256 threads, raster ranks above 65 536 in the thinning, record buffers of about 100 000 entries.  Each of those cases has to
show its property (pc.check_large_property) on the device's own output too, so that a run that never crossed the 64 KB boundary fails."""
import numpy as np
import pytest

import pixel_select_common as pc
from ldso_amd import binding, synth

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Run:
    """one selector and the calls of a fixture case on it"""

    def __init__(self, name, path=pc.GOLDEN):
        self.case = pc.load_case(name, path)
        h, w = pc.image(self.case["calls"][0]["image"]).shape
        self.w, self.h = w, h
        self.sel = binding.PixelSelector(w, h, pc.golden(path)[f"pattern/{w}x{h}"])
        s = self.case["settings"]
        self.sel.set_settings(float(s[0]), float(s[1]), float(s[2]), bool(s[3]))
        self.pyrs = []

    def call(self, j, host=0, density=None):
        c = self.case["calls"][j]
        if density is not None:
            c = dict(c, density=density)
        pyr = binding.Pyramid(self.w, self.h, 3).make_images(pc.image(c["image"]).astype(np.float32))
        self.pyrs.append(pyr)
        self.sel.set_response(pc.golden()["B"] if c["response"] else None)
        if c["pot0"]:
            self.sel.potential = c["pot0"]
        n, counts, used = self.sel.make_maps(pyr, c["density"], c["rec"], c["th_factor"])
        m = self.sel.get_map()
        k = self.sel.make_points(pyr, host)
        q, t = self.sel.get_points()
        assert len(q) == k
        return dict(n=n, counts=counts, used=used, left=self.sel.potential, map=m, ths=self.sel.get_thresholds(), imm=q, type=t, pyr=pyr)

    def close(self):
        self.sel.close()
        for p in self.pyrs:
            p.close()


def check_call(r, c, host=0):
    ret, n2, n3, n4, used, left = (int(x) for x in c["out"])
    print("device", r["n"], r["counts"], r["used"], r["left"], "reference", c["out"], "map differences", int((r["map"] != c["map"]).sum()))
    assert np.array_equal(bits(r["ths"][0].ravel()), bits(c["ths"])) and np.array_equal(bits(r["ths"][1].ravel()), bits(c["thsS"]))
    assert r["counts"] == (n2, n3, n4) and r["used"] == used
    assert r["map"].dtype == np.float32 and np.array_equal(r["map"], c["map"].astype(np.float32))
    assert r["n"] == ret and r["left"] == left
    # the points: raster order inside the border of FullSystem.cc:1290-1291, my_type = the map value
    q = r["imm"]
    assert len(q) == len(c["uv"])
    assert np.array_equal(q["u"], c["uv"][:, 0].astype(np.float32)) and np.array_equal(q["v"], c["uv"][:, 1].astype(np.float32))
    assert np.array_equal(r["type"], c["type"].astype(np.float32)) and np.all(q["host"] == host)
    if c["imm"] is not None:
        g = c["imm"]
        assert np.array_equal(bits(q["color"]), bits(g[:, 2:10])) and np.array_equal(bits(q["weights"]), bits(g[:, 10:18]))
        assert np.array_equal(bits(q["gradH"]).reshape(-1, 4), bits(g[:, 18:22])) and np.array_equal(bits(q["energyTH"]), bits(g[:, 22]))
        assert np.all(q["idepth_min"] == 0) and np.isnan(q["idepth_max"]).all() and np.all(q["quality"] == 10000) and np.all(q["lastTraceStatus"] == 5)
        assert np.all(q["lastTraceUV"] == -1)
    if c["imm_every101"] is not None:          # every 101st record of a large case
        g, q = c["imm_every101"], q[::101]
        assert len(g) == len(q) and np.array_equal(q["u"], g[:, 0]) and np.array_equal(q["v"], g[:, 1])
        assert np.array_equal(bits(q["color"]), bits(g[:, 2:10])) and np.array_equal(bits(q["weights"]), bits(g[:, 10:18]))
        assert np.array_equal(bits(q["gradH"]).reshape(-1, 4), bits(g[:, 18:22])) and np.array_equal(bits(q["energyTH"]), bits(g[:, 22]))


@pytest.mark.parametrize("name", pc.CASES + pc.LARGE_CASES)
def test_against_reference_fixture(name):
    large = name in pc.LARGE_CASES
    R = Run(name, pc.GOLDEN_LARGE if large else pc.GOLDEN)
    try:
        for j, c in enumerate(R.case["calls"]):
            r = R.call(j, host=2)
            if large:          # the case's property on what the device gave, before anything is compared
                print(name, "device n2", r["counts"][0], "reference n2", int(c["out"][1]), "records", len(r["imm"]), "past the pattern in LDS:", r["counts"][0] - pc.RP_LDS)
                before = R.call(j, host=2, density=1e6)["map"] if name == "large_mixed_thinned" else None          # the same select pass, nothing thinned
                pc.check_large_property(name, (r["n"], *r["counts"], r["used"], r["left"]), c["pot0"], c["density"], r["map"], before, r["ths"][1].ravel())
            check_call(r, c, host=2)
    finally:
        R.close()


def test_two_calls_are_byte_identical():
    R = Run("thinning")
    try:
        a = R.call(0)
        b = R.call(0)
        assert a["map"].tobytes() == b["map"].tobytes() and a["imm"].tobytes() == b["imm"].tobytes() and a["type"].tobytes() == b["type"].tobytes()
        assert (a["n"], a["counts"], a["used"], a["left"]) == (b["n"], b["counts"], b["used"], b["left"]) and len(a["imm"]) > 100
        assert a["ths"][0].tobytes() == b["ths"][0].tobytes() and a["ths"][1].tobytes() == b["ths"][1].tobytes()
    finally:
        R.close()


def test_two_calls_are_byte_identical_large():
    """large_mixed_p1: the scan reads the pattern from LDS and from global memory, block by block and by ballot"""
    R = Run("large_mixed_p1", pc.GOLDEN_LARGE)
    try:
        a = R.call(0)
        b = R.call(0)
        assert a["map"].tobytes() == b["map"].tobytes() and a["imm"].tobytes() == b["imm"].tobytes() and a["type"].tobytes() == b["type"].tobytes()
        assert (a["n"], a["counts"], a["used"], a["left"]) == (b["n"], b["counts"], b["used"], b["left"]) and a["counts"][0] >= pc.N2_PAST_LDS
        assert a["ths"][0].tobytes() == b["ths"][0].tobytes() and a["ths"][1].tobytes() == b["ths"][1].tobytes()
    finally:
        R.close()


def test_raster_scan_two_rows_per_thread():
    """96 x 288: the row scan's 256 threads own two rows each (per = 2) and the threads from 144 on own none; the scanned columns 3..91 take two 64-column
    steps, the second one ragged.  The map's equality with the reference is the fixture cases' business; here the records are checked against the device's own
    map, and the thinning against its own count."""
    w, h, pot = 96, 288, 3
    sel = binding.PixelSelector(w, h, np.random.default_rng(5).integers(0, 256, w * h).astype(np.uint8))
    pyr = binding.Pyramid(w, h, 3).make_images(pc.steps_image(w, h).astype(np.float32))
    try:
        sel.potential = pot
        n, counts, used = sel.make_maps(pyr, 1e6, 0)          # quotia >= 0.95: nothing is thinned
        m = sel.get_map()
        assert used == pot and n == sum(counts) == (m != 0).sum()
        k = sel.make_points(pyr, 0)
        q, t = sel.get_points()
        vu = np.argwhere(m[3:h - 4, 3:w - 4] != 0) + 3          # raster order
        assert k == len(q) == len(vu)
        u, v = q["u"].astype(np.int64), q["v"].astype(np.int64)
        assert np.array_equal(q["u"], vu[:, 1].astype(np.float32)) and np.array_equal(q["v"], vu[:, 0].astype(np.float32)) and np.array_equal(t, m[vu[:, 0], vu[:, 1]])
        assert (v >= 256).any() and ((v >= 257) & (v % 2 == 1)).any() and (u < 67).any() and (u >= 67).any()
        sel.potential = pot
        n2, counts2, _ = sel.make_maps(pyr, 0.6 * sum(counts), 0)          # quotia = 0.6: thinned, no recursion
        assert counts2 == counts and 0 < n2 < sum(counts) and (sel.get_map() != 0).sum() == n2
    finally:
        sel.close(); pyr.close()


def test_append_points_device():
    R = Run("natural")
    try:
        r = R.call(0, host=1)
        win = synth.make_window(F=2, P=50, w=R.w, h=R.h, fx=R.w * 0.6, seed=71)
        a, _ = synth.make_immature_points(win, 5)
        n = len(r["imm"])
        tr = binding.Tracer(R.w, R.h, len(a) + n + 3)
        tr.set_points(a)
        imm_dev, type_dev, cnt = R.sel.device_ptrs()
        assert cnt == n > 500 and imm_dev and type_dev
        tr.append_points_device(cnt, imm_dev)
        got = tr.get_points()
        assert len(got) == len(a) + n and got.tobytes() == np.concatenate([a, r["imm"]]).tobytes()
        assert np.all(tr.get_point_types() == 1)
        tr.set_tail_types_device(cnt, type_dev)
        assert np.array_equal(tr.get_point_types(), np.concatenate([np.ones(len(a), np.float32), r["type"]])) and set(r["type"]) - {1.0}
        with pytest.raises(binding.LdsoError) as e:
            tr.set_tail_types_device(len(got) + 1, type_dev)
        assert e.value.code == binding.E_INVALID
        tr.close()
    finally:
        R.close()


def test_append_points_device_large():
    """the records of large_mixed_p1 (about 92 000: the selector's buffer grown far past its first 4096 entries, the tracer's sized to match) appended once"""
    R = Run("large_mixed_p1", pc.GOLDEN_LARGE)
    try:
        r = R.call(0, host=1)
        win = synth.make_window(F=2, P=50, w=R.w, h=R.h, fx=R.w * 0.6, seed=71)
        a, _ = synth.make_immature_points(win, 5)
        n = len(r["imm"])
        tr = binding.Tracer(R.w, R.h, len(a) + n)
        tr.set_points(a)
        imm_dev, type_dev, cnt = R.sel.device_ptrs()
        assert cnt == n == len(R.case["calls"][0]["uv"]) > pc.RP_LDS and imm_dev and type_dev
        tr.append_points_device(cnt, imm_dev)
        got = tr.get_points()
        assert len(got) == len(a) + n and got.tobytes() == np.concatenate([a, r["imm"]]).tobytes()
        tr.set_tail_types_device(cnt, type_dev)
        assert np.array_equal(tr.get_point_types(), np.concatenate([np.ones(len(a), np.float32), r["type"]])) and set(r["type"]) - {1.0}
        tr.close()
    finally:
        R.close()


def test_nonfinite_pixel():
    w, h = 160, 96
    bad = pc.image("scene").astype(np.float32)
    bad[40, 77] = np.nan
    sel = binding.PixelSelector(w, h, pc.golden()[f"pattern/{w}x{h}"])
    pyr = binding.Pyramid(w, h, 3).make_images(bad)
    with pytest.raises(binding.LdsoError) as e:
        sel.make_maps(pyr, 800.0, 1, 1.0)
    assert e.value.code == binding.E_NONFINITE and "ldso_pixsel_make_maps" in str(e.value)
    m = sel.get_map()
    assert set(np.unique(m)) <= {0.0, 1.0, 2.0, 4.0} and (m != 0).sum() > 100          # the rest of the image is still selected from
    sel.close(); pyr.close()


def test_refusals():
    with pytest.raises(binding.LdsoError) as e:
        binding.PixelSelector(100, 64, np.zeros(6400, np.uint8))
    assert e.value.code == binding.E_UNSUPPORTED
    w, h = 96, 64
    sel = binding.PixelSelector(w, h, pc.golden()[f"pattern/{w}x{h}"])
    pyr = binding.Pyramid(w, h, 2).make_images(pc.image("small").astype(np.float32))          # select reads three levels
    with pytest.raises(binding.LdsoError) as e:
        sel.make_maps(pyr, 100.0)
    assert e.value.code == binding.E_INVALID and "ldso_pixsel_make_maps" in str(e.value)
    sel.close(); pyr.close()
