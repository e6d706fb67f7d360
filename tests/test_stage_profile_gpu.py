"""The staged timing splits of ldso_feat_*, ldso_feat_group_*, ldso_pixsel_*, ldso_undist_* and ldso_undist_group_* (the *_profile entries; StageClock in
ldso_amd/csrc/hip_host.h), as a caller sees them, the same for every handle: zeros before the first profiled call, a finite non-negative value per stage after
one (positive for every stage that always launches), the results of a profiled call byte for byte those of an unprofiled one, and values that an unprofiled
call leaves alone.  The undistorters do not wait in the call: their read settles the pending measurement.  Nothing here depends on how long a stage takes.
Sizes are the smallest the solo tests of each stage use: 160 x 128 scenes for the detectors, the 96 x 64 / 160 x 96 fixture cases of the pixel selector,
the recorded 120 x 90 -> 104 x 72 tables of the undistorters with three-level pyramids."""
import numpy as np
import pytest

import feature_detect_common as fc
import pixel_select_common as pc
import undistort_common as uc
from ldso_amd import binding

pytestmark = pytest.mark.gpu


def stream():
    """a stream of its own for the members of one group"""
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    return ts.cuda_stream


class Feat:
    """one detector on a 160 x 128 scene; every stage launches (the grid has cells)"""
    N, ALWAYS = 4, (0, 1, 2, 3)

    def __init__(self, image=None):
        irr = fc.scene(160, 128)[0] if image is None else image
        self.det = binding.Features(160, 128, binding.Features.grid(160, 128, 700)["capacity"] + 1, fc.golden()["pattern"])
        self.pyr = binding.Pyramid(160, 128, 1).make_images(irr)
        self.profile = self.det.profile

    def run(self):
        n, nc = self.det.detect(self.pyr, 700, 2)
        return (n, nc) + tuple(a.tobytes() for a in self.det.get())

    def close(self):
        self.det.close(); self.pyr.close()


class FeatGroup:
    """two detectors on one stream; stage 4 is the append, which does not launch without tracers"""
    N, ALWAYS = 5, (0, 1, 2, 3)

    def __init__(self):
        irr = fc.scene(160, 128)[0]
        self.irr = [irr, np.ascontiguousarray(np.roll(irr, (3, 7), (0, 1)))]
        cap = binding.Features.grid(160, 128, 700)["capacity"] + 1
        self.det = [binding.Features(160, 128, cap, fc.golden()["pattern"]) for _ in self.irr]
        st = stream()
        for d in self.det:
            d.set_stream(st)
        self.pyr = [binding.Pyramid(160, 128, 1).make_images(i) for i in self.irr]
        self.grp = binding.FeaturesGroup(self.det)
        self.profile = self.grp.profile

    def run(self):
        cnt, cor, sta = self.grp.detect(self.pyr, 700, [1, 2])
        return (cnt.tobytes(), cor.tobytes(), sta.tobytes()) + tuple(a.tobytes() for fq in self.grp.get() for a in fq)

    def close(self):
        self.grp.close()
        for x in self.det + self.pyr:
            x.close()


class PixSel:
    """one selector on a fixture case whose makeMaps thins (stage 3 launches); stages 0..3 belong to make_maps, stage 4 to make_points"""
    N, ALWAYS = 5, (0, 1, 2, 3, 4)

    def __init__(self, name="thinning"):
        self.c = pc.load_case(name)["calls"][0]
        self.pot0 = self.c["pot0"] or 3                                                  # the potential every make_maps of this object starts from
        img = pc.image(self.c["image"]).astype(np.float32)
        h, w = img.shape
        self.sel = binding.PixelSelector(w, h, pc.golden()[f"pattern/{w}x{h}"])
        s = pc.load_case(name)["settings"]
        self.sel.set_settings(float(s[0]), float(s[1]), float(s[2]), bool(s[3]))
        self.sel.set_response(pc.golden()["B"] if self.c["response"] else None)
        self.pyr = binding.Pyramid(w, h, 3).make_images(img)
        self.profile = self.sel.profile

    def maps(self):
        self.sel.potential = self.pot0
        out = self.sel.make_maps(self.pyr, self.c["density"], self.c["rec"], self.c["th_factor"])
        return out + (self.sel.get_map().tobytes(),)

    def points(self):
        n = self.sel.make_points(self.pyr, 2)
        return (n,) + tuple(a.tobytes() for a in self.sel.get_points())

    def run(self):
        return self.maps() + self.points()

    def close(self):
        self.sel.close(); self.pyr.close()


class Undist:
    """one undistorter, recorded case B, into a three-level pyramid; the call does not wait"""
    N, ALWAYS = 3, (0, 1, 2)

    def __init__(self):
        g = uc.golden()
        w_org, h_org, w, h, rx, ry = uc.case("B")
        self.U = binding.Undistorter(w_org, h_org, w, h)
        self.U.set_remap(rx, ry)
        self.U.set_photometric(g["G256"], g["vignetteMapInv"], 1)
        self.pyr = binding.Pyramid(w, h, 3)
        self.raw = g["raw8"]
        self.profile = self.U.profile

    def enqueue(self):
        self.U.frame(self.raw, uc.EXPOSURE, 1.0, pyr=self.pyr)

    def results(self):
        return (self.U.get().tobytes(),) + tuple(self.pyr.get_level(l).tobytes() for l in range(3))

    def run(self):
        self.enqueue()
        return self.results()

    def close(self):
        self.U.close(); self.pyr.close()


class UndistGroup:
    """two undistorters (recorded cases A and B, an 8- and a 16-bit frame) on one stream, into a pyramid group; the call does not wait"""
    N, ALWAYS = 3, (0, 1, 2)

    def __init__(self):
        g = uc.golden()
        self.U, self.pyr, st = [], [], stream()
        for c, G in (("A", "G256"), ("B", "G65536")):
            w_org, h_org, w, h, rx, ry = uc.case(c)
            U = binding.Undistorter(w_org, h_org, w, h)
            U.set_stream(st)
            U.set_remap(rx, ry)
            U.set_photometric(g[G], g["vignetteMapInv"], 2)
            self.U.append(U)
            self.pyr.append(binding.Pyramid(w, h, 3))
        self.raws = [g["raw8"], g["raw16"]]
        self.grp = binding.UndistorterGroup(self.U)
        self.pg = binding.PyramidGroup(self.pyr)
        self.profile = self.grp.profile

    def enqueue(self):
        self.grp.frames(self.raws, [uc.EXPOSURE, uc.EXPOSURE], pyr_group=self.pg)

    def results(self):
        return tuple(U.get().tobytes() for U in self.U) + tuple(p.get_level(l).tobytes() for p in self.pyr for l in range(3))

    def run(self):
        self.enqueue()
        return self.results()

    def close(self):
        self.grp.close(); self.pg.close()
        for x in self.U + self.pyr:
            x.close()


def measured(us, n, positive):
    """a split after a profiled call: n finite values >= 0, the stages `positive` > 0"""
    print("profiled split (us):", list(us))
    assert us.shape == (n,) and np.isfinite(us).all() and (us >= 0).all(), us
    assert all(us[k] > 0 for k in positive), us


@pytest.mark.parametrize("make", [Feat, FeatGroup, PixSel, Undist, UndistGroup])
def test_switch_values_and_results(make):
    S = make()
    try:
        assert S.profile(False).tobytes() == np.zeros(S.N, np.float32).tobytes()          # (a) a fresh handle
        plain = S.run()                                                                  # an unprofiled call
        assert S.profile(True).tobytes() == np.zeros(S.N, np.float32).tobytes()          # ... measures nothing
        profiled = S.run()
        first = S.profile(True)
        measured(first, S.N, S.ALWAYS)                                                   # (b)
        assert profiled == plain                                                         # (c)
        again = S.profile(False)
        assert again.tobytes() == first.tobytes()                                        # a read changes nothing
        assert S.run() == plain                                                          # (d) one more call, unprofiled
        assert S.profile(False).tobytes() == first.tobytes()
    finally:
        S.close()


def test_pixel_selector_stage_4_belongs_to_make_points():
    S = PixSel()
    try:
        S.profile(True)
        S.maps()
        us = S.profile(True)
        measured(us, 5, (0, 1, 2, 3))
        assert us[4] == 0                                                                # make_points has not run yet
        S.points()
        both = S.profile(False)
        measured(both, 5, (0, 1, 2, 3, 4))
        assert both[:4].tobytes() == us[:4].tobytes()                                    # make_points leaves the stages of make_maps alone
    finally:
        S.close()


def test_pixel_selector_over_recursion_rounds():
    """recurse_smaller: a second select pass at another potential; stages 1 and 2 are summed over the rounds, the thinning may or may not follow"""
    S = PixSel("recurse_smaller")
    try:
        plain = S.run()
        assert plain[2] != S.pot0                                                   # the potential moved: more than one round
        S.profile(True)
        assert S.run() == plain
        measured(S.profile(False), 5, (0, 1, 2, 4))
    finally:
        S.close()


@pytest.mark.parametrize("make", [Undist, UndistGroup])
def test_undistorter_read_settles_the_pending_measurement(make):
    """(e) nothing waits between the call and the read"""
    S = make()
    try:
        S.profile(True)
        S.enqueue()
        us = S.profile(False)
        measured(us, 3, (0, 1, 2))
        want = S.results()
        S.enqueue()                                                                      # unprofiled, again without a wait before the read
        assert S.profile(False).tobytes() == us.tobytes()
        assert S.results() == want
    finally:
        S.close()


def test_detector_without_a_corner():
    """(f) a constant image: the grid has cells, no pixel passes the gradient threshold; the launches sized for the capacity still run"""
    S = Feat(np.full((128, 160), 100.0, np.float32))
    try:
        S.profile(True)
        assert S.run()[:2] == (0, 0)
        measured(S.profile(False), 4, ())
    finally:
        S.close()


def test_detector_on_a_grid_without_cells():
    """capacity 0 (40 x 40, four features wanted: the border of skipped cells leaves none): no kernel launches, every boundary is still recorded"""
    assert binding.Features.grid(40, 40, 4)["capacity"] == 0
    det = binding.Features(40, 40, 16, fc.golden()["pattern"])
    pyr = binding.Pyramid(40, 40, 1).make_images(fc.scene(160, 128)[0][:40, :40])
    try:
        det.profile(True)
        assert det.detect(pyr, 4, 0) == (0, 0)
        measured(det.profile(False), 4, ())
    finally:
        det.close(); pyr.close()
