"""ldso_feat_group_*: ldso_feat_detect (+ ldso_trace_append_points_device) of many detectors in five (six) launches (k_feat_*_group, ldso_amd/csrc/features.hip).
Every active member's counts, features, immature records and appended tracer records are those of a twin detector's (and twin tracer's) own solo calls on the same
pyramid, byte for byte: the grouped kernels run the device functions of the solo kernels on the same bytes, so no tolerance applies.  Scenes and the restatement come
from tests/feature_detect_common.py; one member is the case of tests/golden/ref_detect_corners.npz, compared to the fixture as the solo call is."""
import functools

import numpy as np
import pytest

import feature_detect_common as fc
from ldso_amd import binding, synth
from test_feature_detect_gpu import ANGLE_TOL, check_against
from test_trace_group_gpu import stream

pytestmark = pytest.mark.gpu


def sparse_image():
    """the scene of test_empty_and_sparse_cells: four gradient pixels, spread over three cells"""
    one = np.full((144, 192), 100.0, np.float32)
    one[60, 60] = 200.0
    return one


# (name) -> (irradiance, n wanted, response table or None, host index); shapes: gridsize 10 with two picks per cell; gridsize 15; gridsize 5, 228 cells;
# gridsize 6, 1218 cells, every one with a pick (five tiles of the suppression, workgroup ranges that start off the tile size); three cells with candidates
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "golden":
        g = fc.golden()
        return g["image"].astype(np.float32), int(g["n"]), g["B"], 0
    if name == "sparse":
        return sparse_image(), 300, None, 4
    if name == "nan":
        irr = fc.scene(192, 144)[0].copy()
        irr[65, 85] = np.nan          # inside a cell (gridsize 10: cells from x = 40, y = 40 on)
        return irr, 300, None, 0
    if name.startswith("small"):          # distinct scenes of (160, 128, 700)
        k = int(name[5:])
        return np.ascontiguousarray(np.roll(fc.scene(160, 128)[0], (3 * k, 7 * k), (0, 1))), 700, None, k % 7
    w, h, n, resp, host = {"g10": (192, 144, 300, False, 3), "g15": (192, 144, 120, True, 1), "g5": (160, 128, 700, False, 0), "g6": (320, 240, 2000, False, 2)}[name]
    return fc.scene(w, h)[0], n, fc.bent_response() if resp else None, host


MIXED = ("g10", "g15", "g5", "g6", "sparse")


def capacity(name):
    irr, n, _, _ = case(name)
    return binding.Features.grid(irr.shape[1], irr.shape[0], n)["capacity"]


def detector(name, st=None, max_features=None):
    irr, n, B, _ = case(name)
    det = binding.Features(irr.shape[1], irr.shape[0], max_features or capacity(name) + 1, fc.golden()["pattern"])
    if st is not None:
        det.set_stream(st)
    det.set_response(B)
    return det


def pyramid(name):
    irr = case(name)[0]
    return binding.Pyramid(irr.shape[1], irr.shape[0], 1).make_images(irr)


def solo_detect(det, pyr, name):
    """-> (n, n_corners, code) of the solo call"""
    try:
        nf, nc = det.detect(pyr, case(name)[1], case(name)[3])
        return nf, nc, 0
    except binding.LdsoError as e:
        assert e.code == binding.E_NONFINITE
        return det.n, det.n_corners, e.code


@functools.lru_cache(maxsize=None)
def solo(name):
    """the solo calls on a twin detector, once per case -> dict(n, nc, code, F, Q) (read-only)"""
    det, pyr = detector(name), pyramid(name)
    nf, nc, code = solo_detect(det, pyr, name)
    F, Q = det.get()
    det.close(); pyr.close()
    return dict(n=nf, nc=nc, code=code, F=F, Q=Q)


class Group:
    """detectors of the named cases on one stream, their pyramids, the group"""

    def __init__(self, names, st=None):
        self.st = st if st is not None else stream()
        self.names = list(names)
        self.det = [detector(nm, self.st) for nm in names]
        self.pyr = [pyramid(nm) for nm in names]
        self.grp = binding.FeaturesGroup(self.det)
        self.nf = [case(nm)[1] for nm in names]
        self.host = [case(nm)[3] for nm in names]

    def detect(self, tracers=None, active=None, pyr=None, nf=None):
        return self.grp.detect(pyr or self.pyr, nf or self.nf, self.host, tracers, active)

    def close(self):
        self.grp.close()
        for x in self.det + self.pyr:
            x.close()


def same_as_solo(name, F, Q, nf, nc):
    S = solo(name)
    assert (nf, nc) == (S["n"], S["nc"]), (name, nf, nc, S["n"], S["nc"])
    assert np.array_equal(F.view(np.uint8), S["F"].view(np.uint8)), name
    assert np.array_equal(Q.view(np.uint8), S["Q"].view(np.uint8)), name
    for k in ("score", "angle"):
        assert np.array_equal(F[k], S["F"][k], equal_nan=True), (name, k)


def det_state(d):
    return (d.n, d.n_corners) + tuple(a.tobytes() for a in d.get())


def trk_state(t):
    return t.n, t.get_points().tobytes(), t.get_point_types().tobytes()


@functools.lru_cache(maxsize=None)
def some_records(w, h, count):
    win = synth.make_window(F=2, P=50, w=w, h=h, fx=w * 0.6, seed=71)
    pts, _ = synth.make_immature_points(win, (count + 1) // 2)
    assert len(pts) >= count
    return pts[:count]


def loaded_tracer(w, h, held, room, st=None):
    """a tracer that holds `held` records with types other than 1 and has room for `room` more"""
    t = binding.Tracer(w, h, max(held + room, 1))
    if st is not None:
        t.set_stream(st)
    if held:
        t.set_points(some_records(w, h, held))
        t.set_point_types(2.0 + np.arange(held, dtype=np.float32) % 3)
    return t


def test_mixed_group_equals_the_solo_calls():
    G = Group(MIXED)
    cnt, cor, sta = G.detect()
    assert cnt[3] > 512 and list(sta) == [0] * 5 and 0 < cnt[4] < 8
    got = G.grp.get()
    tr = binding.Tracer(320, 240, 3000)
    for i, nm in enumerate(MIXED):
        same_as_solo(nm, got[i][0], got[i][1], int(cnt[i]), int(cor[i]))
        F, Q = G.det[i].get()          # the member's own ldso_feat_get ...
        same_as_solo(nm, F, Q, G.det[i].n, G.det[i].n_corners)
        _, imm_dev, n_dev = G.det[i].device_ptrs()          # ... and ldso_feat_device: the records as they lie on the device, through a tracer
        assert n_dev == cnt[i]
        tr.set_points(np.zeros(0, synth.IMMATURE_DTYPE))
        tr.append_points_device(n_dev, imm_dev)
        assert tr.get_points().tobytes() == solo(nm)["Q"].tobytes(), nm
    # a member stays usable on its own between group calls
    i = MIXED.index("g10")
    assert solo_detect(G.det[i], G.pyr[i], "g10") == (solo("g10")["n"], solo("g10")["nc"], 0)
    same_as_solo("g10", *G.det[i].get(), G.det[i].n, G.det[i].n_corners)
    us = G.grp.profile(True)
    G.detect()
    us = G.grp.profile(False)
    print("profiled split (us): cells+compaction, corners, angle+descriptor, records, append", list(us))
    assert us[:4].min() > 0 and us[4] >= 0
    tr.close(); G.close()


def test_a_member_equals_the_reference_fixture():
    names = ("g15", "golden", "g5")
    G = Group(names)
    cnt, cor, sta = G.detect()
    F, Q = G.grp.get()[1]
    nc = int(cor[1])
    g = fc.golden()
    img = g["image"].astype(np.float32)
    dI = synth.make_images(img, 1)[0]
    R = fc.detect(dI, int(g["n"]), g["B"], g["pattern"])
    check_against(F, Q, nc, R, dI)
    assert len(F) == len(g["u"]) and nc == int(g["n_corners"])
    assert np.array_equal(F["u"], g["u"]) and np.array_equal(F["v"], g["v"]) and np.array_equal(F["score"].view(np.uint32), g["score"].view(np.uint32))
    assert np.array_equal(F["is_corner"], g["is_corner"])
    d = np.abs(F["angle"].astype(np.float64) - g["angle"])
    assert np.minimum(d, 2 * np.pi - d).max() <= ANGLE_TOL
    diff = np.unpackbits(F["descriptor"] ^ g["descriptor"], axis=1, bitorder="little").astype(bool)
    assert not (diff & ~R["unsafe"]).any()
    for k in ("color", "weights", "gradH", "energyTH"):
        assert np.array_equal(Q[k].view(np.uint32), g[k].view(np.uint32)), k
    G.close()


def test_append_to_the_tracers():
    G = Group(MIXED)
    held = (10, 0, 37, 300, 5)
    trk, twin = [], []
    for nm, k in zip(MIXED, held):
        h, w = case(nm)[0].shape
        trk.append(loaded_tracer(w, h, k, capacity(nm), G.st))
        twin.append(loaded_tracer(w, h, k, capacity(nm)))
    NONE = 2          # this member appends nothing
    before = trk_state(trk[NONE])
    given = [t if i != NONE else None for i, t in enumerate(trk)]
    cnt, cor, sta = G.detect(tracers=given)
    for i, nm in enumerate(MIXED):
        same_as_solo(nm, *G.det[i].get(), int(cnt[i]), int(cor[i]))
        if i == NONE:
            assert trk_state(trk[i]) == before
            continue
        # the twin: ldso_feat_detect + ldso_trace_append_points_device
        det, pyr = detector(nm), G.pyr[i]
        nf, _, _ = solo_detect(det, pyr, nm)
        _, imm_dev, n_dev = det.device_ptrs()
        twin[i].append_points_device(n_dev, imm_dev)
        assert trk[i].n == held[i] + nf == twin[i].n, (nm, trk[i].n, held[i], nf)
        assert trk_state(trk[i]) == trk_state(twin[i]), nm
        assert np.all(trk[i].get_point_types()[held[i]:] == 1.0) and np.all(trk[i].get_point_types()[:held[i]] != 1.0)
        det.close()
    for t in trk + twin:
        t.close()
    G.close()


def test_active_list_single_member_and_repeated_calls():
    names = ("g10", "g5", "g15", "sparse")
    G = Group(names)
    INACTIVE = 1
    G.det[INACTIVE].detect(G.pyr[INACTIVE], 500, 6)          # a detection of its own, with other arguments than the group would use: the state it must keep
    before = det_state(G.det[INACTIVE])
    trk = [loaded_tracer(case(nm)[0].shape[1], case(nm)[0].shape[0], 9, capacity(nm), G.st) for nm in names]
    t_before = trk_state(trk[INACTIVE])
    active = [i != INACTIVE for i in range(len(names))]
    cnt, cor, sta = G.detect(tracers=trk, active=active)
    assert (cnt[INACTIVE], cor[INACTIVE], sta[INACTIVE]) == (-1, -1, -1)          # the rows of the outputs are left alone
    assert det_state(G.det[INACTIVE]) == before and trk_state(trk[INACTIVE]) == t_before
    got = G.grp.get(active)
    assert got[INACTIVE] is None
    for i, nm in enumerate(names):
        if i != INACTIVE:
            same_as_solo(nm, got[i][0], got[i][1], int(cnt[i]), int(cor[i]))
            assert trk[i].n == 9 + cnt[i]
    # a second identical call: byte-identical buffers
    first = [det_state(d) for d in G.det]
    G.detect(active=active)
    assert [det_state(d) for d in G.det] == first
    for t in trk:
        t.close()
    G.close()
    # n = 1
    G1 = Group(("g6",))
    cnt, cor, sta = G1.detect()
    same_as_solo("g6", *G1.grp.get()[0], int(cnt[0]), int(cor[0]))
    G1.close()


def test_nonfinite_member():
    names = ("g10", "nan", "g5", "g15")
    G = Group(names)
    clean_pyr = list(G.pyr)
    clean_pyr[1] = pyramid("g10")          # the same scene without the NaN
    cnt0, cor0, sta0 = G.detect(pyr=clean_pyr)
    assert list(sta0) == [0] * 4
    clean = [det_state(d) for d in G.det]
    h, w = case("nan")[0].shape
    trk = loaded_tracer(w, h, 3, capacity("nan"), G.st)
    with pytest.raises(binding.LdsoError) as e:
        G.detect(tracers=[None, trk, None, None])
    assert e.value.code == binding.E_NONFINITE and "ldso_feat_group_detect" in str(e.value) and "member 1" in str(e.value)
    cnt, cor, sta = G.grp.last
    assert list(sta) == [0, binding.E_NONFINITE, 0, 0]
    S = solo("nan")
    assert S["code"] == binding.E_NONFINITE
    same_as_solo("nan", *G.det[1].get(), int(cnt[1]), int(cor[1]))
    assert trk.n == 3 + cnt[1] and trk.get_points()[3:].tobytes() == S["Q"].tobytes()          # the append happens regardless
    for i in (0, 2, 3):
        assert det_state(G.det[i]) == clean[i], names[i]
        same_as_solo(names[i], *G.det[i].get(), int(cnt[i]), int(cor[i]))
    trk.close(); clean_pyr[1].close(); G.close()


def test_refusals_change_nothing():
    names = ("g10", "g5", "g15")
    G = Group(names)
    shapes = [case(nm)[0].shape for nm in names]
    trk = [loaded_tracer(s[1], s[0], 4 + i, capacity(nm), G.st) for i, (s, nm) in enumerate(zip(shapes, names))]
    G.detect()
    before = [det_state(d) for d in G.det] + [trk_state(t) for t in trk]

    def refused(call, code, *words):
        with pytest.raises(binding.LdsoError) as e:
            call()
        assert e.value.code == code and "ldso_feat_group_detect" in str(e.value), str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert [det_state(d) for d in G.det] + [trk_state(t) for t in trk] == before, words

    refused(lambda: G.detect(tracers=trk, nf=[300, 700, 600]), binding.E_INVALID, "member 2", "max_features")          # (192, 144, 600): capacity 396
    refused(lambda: G.detect(tracers=trk, nf=[6, 700, 120]), binding.E_UNSUPPORTED, "member 0", "gridsize")              # (192, 144, 6): gridsize 68
    refused(lambda: G.detect(tracers=trk, pyr=[G.pyr[0], G.pyr[0], G.pyr[2]]), binding.E_INVALID, "member 1", "pyramid")
    refused(lambda: G.detect(tracers=trk, nf=[300, 0, 120]), binding.E_INVALID, "member 1", "n_features")
    elsewhere = loaded_tracer(shapes[2][1], shapes[2][0], 2, capacity("g15"))          # on a stream of its own
    refused(lambda: G.detect(tracers=[trk[0], trk[1], elsewhere]), binding.E_INVALID, "member 2", "stream")
    assert trk_state(elsewhere)[0] == 2
    tight = loaded_tracer(shapes[1][1], shapes[1][0], 2, capacity("g5") - 1, G.st)      # room for all but one record of the capacity
    t_before = trk_state(tight)
    refused(lambda: G.detect(tracers=[trk[0], tight, trk[2]]), binding.E_INVALID, "member 1", "room")
    assert trk_state(tight) == t_before
    refused(lambda: G.detect(tracers=[trk[0], trk[1], trk[0]]), binding.E_INVALID, "member 2", "same tracer")
    # membership
    L = G.grp.L
    assert L.ldso_feat_destroy(G.det[1].h) == binding.E_INVALID and "ldso_feat_destroy" in L.ldso_last_error().decode()
    with pytest.raises(binding.LdsoError) as e:
        binding.FeaturesGroup([G.det[1]])
    assert e.value.code == binding.E_INVALID and "at most one group" in str(e.value)
    lone = detector("g5", G.st)
    with pytest.raises(binding.LdsoError) as e:
        binding.FeaturesGroup([lone, lone])
    assert e.value.code == binding.E_INVALID and "twice" in str(e.value)
    G.det[2].set_stream(None)
    refused(lambda: G.detect(tracers=trk), binding.E_INVALID, "stream")
    refused(lambda: G.detect(tracers=trk, active=[True, True, False]), binding.E_INVALID, "stream")          # ... also while that member sits out
    G.det[2].set_stream(G.st)
    cnt, cor, sta = G.detect(tracers=trk)          # and everything still works
    for i, nm in enumerate(names):
        same_as_solo(nm, *G.det[i].get(), int(cnt[i]), int(cor[i]))
        assert trk[i].n == 4 + i + cnt[i]
    for t in trk + [elsewhere, tight]:
        t.close()
    lone.close(); G.close()


def test_many_small_members():
    names = tuple("small%d" % k for k in range(17))
    G = Group(names)
    cnt, cor, sta = G.detect()
    got = G.grp.get()
    assert len({solo(nm)["F"].tobytes() for nm in names}) == 17          # distinct scenes
    for i, nm in enumerate(names):
        same_as_solo(nm, got[i][0], got[i][1], int(cnt[i]), int(cor[i]))
    G.close()
