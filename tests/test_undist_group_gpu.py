"""ldso_undist_group_* (ldso_amd/csrc/undistort.hip): the raw frames of a group of undistorters in one copy and one launch, optionally straight into a pyramid group.
Every member's irradiance has the bytes of a solo ldso_undist_frame on a twin handle, of the outputs recorded from the reference (tests/golden/ref_undistort.npz)
and of the numpy restatement (tests/undistort_common.py).  The members, in the order of the group - the smallest shapes at which the member lookup, a partial
last workgroup, the two pixel widths and the passthrough can go wrong:
  A     120 x 90 -> 104 x 72   recorded tables
  tiny  9 x 7 -> 5 x 3         synthetic_tables(seed=5): 15 pixels, a fraction of one workgroup, between larger members
  B     120 x 90 -> 104 x 72   recorded tables
  odd   67 x 53 -> 33 x 29     seed 33: 957 pixels, a partial fourth workgroup
  C     120 x 90 passthrough   recorded; no tables
  up    40 x 30 -> 96 x 64     seed 96: output larger than source
The synthetic tables have entries on both sides of the tap rule (12 of 15, 329 of 957, 1853 of 6144 outside).  A refusal for a pyramid group on another device
needs a second card and is not checked here."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import undistort_common as uc
from ldso_amd import binding
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
ENTRY = "ldso_undist_group_frames"
NAMES = ("A", "tiny", "B", "odd", "C", "up")
SYNTHETIC = {"tiny": ((9, 7), (5, 3)), "odd": ((67, 53), (33, 29)), "up": ((40, 30), (96, 64))}
# one frame of one member: pixel width in bits, setting_photometricCalibration, setting_useExposure, exposure, factor, frame variant (0: the recorded / base frame)
Spec = collections.namedtuple("Spec", "bits pc use_exposure exposure factor variant", defaults=(True, uc.EXPOSURE, 1.0, 0))
Member = collections.namedtuple("Member", "w_org h_org w h rx ry vig raw")


@functools.lru_cache(maxsize=None)
def stream():
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    return ts.cuda_stream


@functools.lru_cache(maxsize=None)
def member(name):
    """sizes, tables, vignette and the base frames {8: ..., 16: ...} of a member (read-only); the synthetic ones as test_shapes_against_the_restatement builds them"""
    g = uc.golden()
    if name in uc.CASES:
        w_org, h_org, w, h, rx, ry = uc.case(name)
        return Member(w_org, h_org, w, h, rx, ry, g["vignetteMapInv"], {8: g["raw8"], 16: g["raw16"]})
    (w_org, h_org), (w, h) = SYNTHETIC[name]
    rx, ry = uc.synthetic_tables(w_org, h_org, w, h, seed=w)
    f8, f16 = uc.textured_frames(w_org, h_org, seed=h)
    vig = (1.0 / np.random.default_rng(5).uniform(0.3, 1.0, (h_org, w_org))).astype(np.float32)
    return Member(w_org, h_org, w, h, rx, ry, vig, {8: f8, 16: f16})


def response(bits):
    return uc.golden()["G256" if bits == 8 else "G65536"]


def frame_of(name, spec):
    """the raw frame of a spec: the base frame, or (variant k) the same pixels shifted k * 13 columns"""
    raw = member(name).raw[spec.bits]
    return raw if spec.variant == 0 else np.roll(raw, 13 * spec.variant, axis=1).copy()


def make(name):
    m = member(name)
    U = binding.Undistorter(m.w_org, m.h_org, m.w, m.h)
    U.set_remap(m.rx, m.ry)
    return U


def configure(U, name, spec):
    U.set_photometric(response(spec.bits), member(name).vig, spec.pc, spec.use_exposure)


@functools.lru_cache(maxsize=None)
def twin(name):
    """the handle of the solo runs, one per member for the whole module"""
    return make(name)


@functools.lru_cache(maxsize=None)
def solo(name, spec):
    """(irradiance, exposure) of a solo ldso_undist_frame with the spec's inputs, computed once (read-only)"""
    U = twin(name)
    configure(U, name, spec)
    e = U.frame(frame_of(name, spec), spec.exposure, spec.factor)
    out = U.get()
    out.setflags(write=False)
    return out, e


@functools.lru_cache(maxsize=None)
def restated(name, spec):
    m = member(name)
    G = response(spec.bits)
    out = uc.undistort(frame_of(name, spec), m.rx, m.ry, m.w_org, m.h_org, m.w, m.h, G, m.vig, uc.mode_of(G, spec.exposure, spec.pc), spec.factor)
    out.setflags(write=False)
    return out


def same_bits(a, b):
    """device against device: the same bytes"""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_values(a, b):
    """device against the host's recording / restatement, as tests/test_undistort_gpu.py compares them: a NaN (0 * inf at an infinite vignette entry) equals a NaN"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class Group:
    """fresh undistorters for `names` on one stream, and their group"""

    def __init__(self, names=NAMES):
        self.names = tuple(names)
        self.U = [make(n) for n in self.names]
        for u in self.U:
            u.set_stream(stream())
        self.g = binding.UndistorterGroup(self.U)

    def frames(self, specs, pyr_group=None, active=None, raws=None):
        """one group call with a Spec per member (None: inactive) -> exposure_out"""
        if active is None and any(s is None for s in specs):
            active = [s is not None for s in specs]
        for u, n, s in zip(self.U, self.names, specs):
            if s is not None:
                configure(u, n, s)
        if raws is None:
            raws = [None if s is None else frame_of(n, s) for n, s in zip(self.names, specs)]
        filler = Spec(8, 0)
        return self.g.frames(raws, [(s or filler).exposure for s in specs], [(s or filler).factor for s in specs], pyr_group=pyr_group, active=active)

    def check(self, specs, exposure_out):
        """every active member has the solo bytes, the restatement's bytes and the solo exposure"""
        for i, (u, n, s) in enumerate(zip(self.U, self.names, specs)):
            if s is None:
                assert np.isnan(exposure_out[i]), n
                continue
            want, e = solo(n, s)
            got = u.get()
            assert same_bits(got, want), (n, s)
            assert same_values(got, restated(n, s)), (n, s)
            assert exposure_out[i] == np.float32(e), (n, s)

    def outputs(self):
        return [u.get().tobytes() for u in self.U]

    def close(self):
        self.g.close()
        for u in self.U:
            u.close()


def pyramids(shapes):
    pyr = [binding.Pyramid(w, h, lv) for w, h, lv in shapes]
    return pyr, binding.PyramidGroup(pyr)


def levels_of(p):
    return [p.get_level(l) for l in range(p.levels)]


@functools.lru_cache(maxsize=None)
def solo_levels(name, spec, levels):
    """the levels a solo ldso_undist_frame builds into a pyramid of its own on the twin handle, computed once"""
    U, m = twin(name), member(name)
    configure(U, name, spec)
    P = binding.Pyramid(m.w, m.h, levels)
    U.frame(frame_of(name, spec), spec.exposure, spec.factor, pyr=P)
    out = [lv.tobytes() for lv in levels_of(P)]
    P.close()
    return out


def test_synthetic_tables_have_both_branches():
    for name, outside in (("tiny", 12), ("odd", 329), ("up", 1853)):
        m = member(name)
        ok, _, _ = uc.taps_inside(m.rx, m.ry, m.w_org, m.h_org)
        assert 0 < (~ok).sum() < ok.size
        assert (~ok).sum() == outside and ok.size == m.w * m.h


# three calls on one group: mixed modes and widths; the widths swapped between the members; the remaining recorded outputs
CALLS = (
    ((Spec(8, 2), Spec(16, 1, True, 2.0), Spec(16, 2), Spec(8, 2, False, 2.0), Spec(8, 2, True, 0.0, 0.7), Spec(16, 0, True, 1.0, 1.3)),
     {"A": "A_u8_m2", "B": "B_u16_m2", "C": "C_u8_e0"}),
    ((Spec(16, 2), Spec(8, 1, True, 2.0), Spec(8, 1), Spec(16, 2, False, 2.0), Spec(16, 2), Spec(8, 0, True, 1.0, 1.3)),
     {"A": "A_u16_m2", "B": "B_u8_m1", "C": "C_u16_m2"}),
    ((Spec(8, 2, True, 0.0, 0.7), Spec(8, 2), Spec(8, 0), Spec(8, 1), Spec(8, 1), Spec(16, 2, True, 0.0, 0.25)),
     {"A": "A_u8_e0", "B": "B_u8_m0", "C": "C_u8_m1"}),
)


def test_bit_identity_mixed_modes_and_widths_in_one_call():
    g = uc.golden()
    G = Group()
    for specs, recorded in CALLS:
        e = G.frames(specs)
        G.check(specs, e)
        for name, key in recorded.items():
            assert same_values(G.U[NAMES.index(name)].get(), g[key]), key
    # setting_useExposure off: 1, whatever the caller passed (checked against the solo value above; here against the reference's)
    e = G.frames(CALLS[0][0])
    assert e[3] == 1.0 and e[0] == np.float32(uc.EXPOSURE) and e[4] == 0.0
    G.close()


def test_active_mask():
    G = Group()
    first = (Spec(8, 2), Spec(16, 1), None, Spec(8, 1), Spec(8, 0), None)
    e = G.frames(first)                               # the raw entries of the inactive members are None
    G.check(first, e)
    for i in (2, 5):                                  # never active: no frame yet
        with pytest.raises(binding.LdsoError) as err:
            G.U[i].get()
        assert err.value.code == -1
    before = [G.U[i].get().tobytes() for i in (0, 1)]
    second = (None, None, Spec(16, 2), Spec(16, 2, True, 1.0, 1.0, 1), None, Spec(8, 2))
    e = G.frames(second)
    G.check(second, e)
    assert [G.U[i].get().tobytes() for i in (0, 1)] == before                  # the inactive members keep the previous call's bytes
    assert same_bits(G.U[4].get(), solo("C", first[4])[0])
    G.close()


def test_into_a_pyramid_group():
    g = uc.golden()
    names, shapes = ("A", "B", "C"), ((104, 72, 3), (104, 72, 2), (120, 90, 1))
    G = Group(names)
    pyr, pg = pyramids(shapes)
    specs = (Spec(8, 2), Spec(8, 1), Spec(8, 0))
    e = G.frames(specs, pyr_group=pg)
    G.check(specs, e)
    first = [levels_of(p) for p in pyr]
    for n, s, (_, _, lv), got, key in zip(names, specs, shapes, first, ("A_u8_m2", "B_u8_m1", "C_u8_m0")):
        assert [x.tobytes() for x in got] == solo_levels(n, s, lv), n
        want = po.make_images(g[key], lv)
        for l in range(lv):
            assert same_values(got[l], want[l]), (n, l)
    for u, got in zip(G.U, first):
        assert same_bits(u.get(), np.ascontiguousarray(got[0][..., 0]))          # ldso_undist_get = channel 0 of level 0
        assert u.device_ptr() != 0
    # the active members of the two groups are the same set: pyramid 1 keeps its levels
    specs2 = (Spec(16, 2, True, uc.EXPOSURE, 1.0, 1), None, Spec(16, 1, True, uc.EXPOSURE, 1.0, 2))
    e = G.frames(specs2, pyr_group=pg)
    G.check(specs2, e)
    for i in (0, 2):
        assert [x.tobytes() for x in levels_of(pyr[i])] == solo_levels(names[i], specs2[i], shapes[i][2]), i
    assert [x.tobytes() for x in levels_of(pyr[1])] == [x.tobytes() for x in first[1]]
    assert same_bits(G.U[1].get(), solo("B", specs[1])[0])
    G.close()
    pg.close()
    for p in pyr:
        p.close()


def test_back_to_back_calls_without_a_host_wait():
    """the arena reuse rule: call 2 grows the arena while call 1 may be in flight, call 3 restages it while call 2 may be"""
    G = Group()
    # the tiny member has no legal pyramid (w, h > 16): its place in the pyramid group is a stand-in that no call writes, and it is inactive in call 3
    shapes = ((104, 72, 3), (17, 17, 1), (104, 72, 2), (33, 29, 1), (120, 90, 1), (96, 64, 2))
    pyr, pg = pyramids(shapes)
    call1 = (None, Spec(8, 2), None, None, None, None)
    call2 = (Spec(8, 2, True, uc.EXPOSURE, 1.0, 1), Spec(16, 1, True, 2.0, 1.0, 1), Spec(16, 2, True, uc.EXPOSURE, 1.0, 1), Spec(8, 1, True, 1.0, 1.0, 1),
             Spec(8, 0, True, 1.0, 1.3, 1), Spec(16, 2, True, 1.0, 1.0, 1))
    call3 = (Spec(16, 2, True, uc.EXPOSURE, 1.0, 2), None, Spec(8, 1, True, uc.EXPOSURE, 1.0, 2), Spec(16, 2, True, 1.0, 1.0, 2), Spec(16, 1, True, uc.EXPOSURE, 1.0, 2),
             Spec(8, 2, True, 1.0, 1.0, 2))
    for specs in (call1, call2, call3):               # the solo references first, so that nothing but the three calls runs between them
        for n, s in zip(NAMES, specs):
            if s is not None:
                solo(n, s), restated(n, s)
    for n, s, (_, _, lv) in zip(NAMES, call3, shapes):
        if s is not None:
            solo_levels(n, s, lv)
    G.frames(call1)
    G.frames(call2)
    e3 = G.frames(call3, pyr_group=pg)
    G.check(call3, e3)                                # get() synchronises
    for n, s, (_, _, lv), p in zip(NAMES, call3, shapes, pyr):
        if s is not None:
            assert [x.tobytes() for x in levels_of(p)] == solo_levels(n, s, lv), n
    assert same_bits(G.U[1].get(), solo("tiny", call2[1])[0])          # call 2's result of the member call 3 left out
    G.close()
    pg.close()
    for p in pyr:
        p.close()


@pytest.mark.parametrize("fetch_between", (True, False))
def test_arena_grows_while_in_use_and_the_next_call_moves_to_another_stream(fetch_between):
    """the reuse rule of both arenas (the undistorters' and the pyramids') on one pair of groups: three members, 8-bit frames, two pyramid levels.  Call 1 has one
    active member, call 2 all three (the arenas are replaced while in use), call 3 runs with every member moved to another stream (ordered behind call 2, whose
    kernels may still read what call 3 restages).  The members are configured once, so nothing but the calls touches their streams.  With the results fetched after
    every call each call's bytes are checked; without, the three calls are enqueued back to back and nothing waits on the host between them."""
    import torch
    names, shapes = ("odd", "up", "A"), ((33, 29, 2), (96, 64, 2), (104, 72, 2))
    calls = [tuple(Spec(8, 2, True, uc.EXPOSURE, 1.0, v) if on else None for on in mask) for v, mask in enumerate(((0, 1, 0), (1, 1, 1), (1, 1, 1)))]
    for specs in calls:                               # the solo references first
        for n, s, (_, _, lv) in zip(names, specs, shapes):
            if s is not None:
                solo(n, s), restated(n, s), solo_levels(n, s, lv)
    other = torch.cuda.Stream()
    G = Group(names)
    pyr, pg = pyramids(shapes)
    for u, n in zip(G.U, names):
        configure(u, n, calls[1][names.index(n)])

    def call(specs):
        raws = [None if s is None else frame_of(n, s) for n, s in zip(names, specs)]
        return G.g.frames(raws, [uc.EXPOSURE] * 3, pyr_group=pg, active=[s is not None for s in specs])

    def check(specs, e):
        G.check(specs, e)
        for n, s, (_, _, lv), p in zip(names, specs, shapes, pyr):
            if s is not None:
                assert [x.tobytes() for x in levels_of(p)] == solo_levels(n, s, lv), n

    for k, specs in enumerate(calls):
        if k == 2:
            for u in G.U:
                u.set_stream(other.cuda_stream)
        e = call(specs)
        if fetch_between or k == 2:
            check(specs, e)
    G.close()
    pg.close()
    for p in pyr:
        p.close()


def test_raw_frames_may_be_overwritten_when_the_call_returns():
    G = Group()
    specs = CALLS[0][0]
    for n, s in zip(NAMES, specs):
        solo(n, s)
    raws = [frame_of(n, s).copy() for n, s in zip(NAMES, specs)]
    e = G.frames(specs, raws=raws)
    for r in raws:
        r[...] = 0
    G.check(specs, e)
    G.close()


def test_a_member_on_its_own_between_group_calls():
    G = Group()
    e = G.frames(CALLS[0][0])
    G.check(CALLS[0][0], e)
    s = Spec(16, 1, True, uc.EXPOSURE, 1.0, 1)
    configure(G.U[2], "B", s)
    assert G.U[2].frame(frame_of("B", s), s.exposure, s.factor) == solo("B", s)[1]
    assert same_bits(G.U[2].get(), solo("B", s)[0])
    e = G.frames(CALLS[1][0])
    G.check(CALLS[1][0], e)
    G.close()


def c_call(G, raws, bpp, pg=None, active=None, exposures=None, null=()):
    """ldso_undist_group_frames through ctypes alone: arguments the binding would not pass (`null`: names of arrays handed over as NULL)"""
    n = len(G.U)
    ptrs = (C.c_void_p * n)(*[None if r is None else r.ctypes.data for r in raws])
    b = np.asarray(bpp, np.int32)
    e = np.full(n, uc.EXPOSURE, np.float32) if exposures is None else np.asarray(exposures, np.float32)
    f = np.ones(n, np.float32)
    act = None if active is None else np.asarray(active, np.uint8)
    args = dict(raw=ptrs, bpp=binding._p(b), exposure=binding._p(e), factor=binding._p(f))
    for k in null:
        args[k] = None
    L = binding.lib()
    rc = L.ldso_undist_group_frames(G.g.h, binding._p(act), args["raw"], args["bpp"], args["exposure"], args["factor"], pg.h if pg is not None else None, None)
    return rc, L.ldso_last_error().decode()


def test_refusals():
    g = uc.golden()
    L = binding.lib()
    names = ("A", "B", "C")
    G = Group(names)
    specs = (Spec(8, 2), Spec(8, 1), Spec(8, 2))
    e = G.frames(specs)
    G.check(specs, e)
    before = G.outputs()
    r8 = [g["raw8"]] * 3

    def refused(rc_msg, *words):
        rc, msg = rc_msg
        assert rc == -1 and ENTRY in msg, msg
        for w in words:
            assert w in msg, msg
        assert G.outputs() == before

    for k in ("raw", "bpp", "exposure", "factor"):
        refused(c_call(G, r8, [1, 1, 1], null=(k,)))
    refused(c_call(G, r8, [1, 1, 1], active=[0, 0, 0]), "no active member")
    refused(c_call(G, [g["raw8"], None, g["raw8"]], [1, 1, 1]), "member 1")
    refused(c_call(G, r8, [1, 3, 1]), "member 1")
    refused(c_call(G, r8, [1, 0, 1]), "member 1")
    refused(c_call(G, [g["raw8"], g["raw8"], g["raw16"]], [1, 1, 2]), "member 2")          # a 16-bit frame on the 256-entry response
    rc, _ = c_call(G, [g["raw8"], g["raw8"], g["raw16"]], [1, 1, 2], exposures=[uc.EXPOSURE, uc.EXPOSURE, 0.0])          # ... which the plain path never reads
    assert rc == 0
    assert same_values(G.U[2].get(), uc.undistort(g["raw16"], None, None, 120, 90, 120, 90))
    e = G.frames(specs)
    assert G.outputs() == before
    with pytest.raises(binding.LdsoError) as err:                                            # the same refusals through the binding
        G.g.frames([g["raw8"], g["raw8"], None], [1.0] * 3)
    assert err.value.code == -1 and ENTRY in str(err.value) and "member 2" in str(err.value)
    # pyramid groups of another length and of another size
    pyr2, pg2 = pyramids(((104, 72, 2), (104, 72, 2)))
    pyr3, pg3 = pyramids(((104, 72, 2), (120, 90, 2), (120, 90, 1)))
    refused(c_call(G, r8, [1, 1, 1], pg=pg2), "pyramid group")
    refused(c_call(G, r8, [1, 1, 1], pg=pg3), "member 1")
    for p in pyr2 + pyr3:
        with pytest.raises(binding.LdsoError):          # nothing was built
            p.get_level(0)
    # a member moved to another stream is refused at the next call, and accepted again once it is back
    G.U[1].set_stream(None)
    refused(c_call(G, r8, [1, 1, 1]), "stream")
    G.U[1].set_stream(stream())
    e = G.frames(specs)
    G.check(specs, e)
    # membership
    for members in ([G.U[0]], [twin("A"), G.U[2]]):                                          # a member of a live group
        with pytest.raises(binding.LdsoError) as err:
            binding.UndistorterGroup(members)
        assert err.value.code == -1 and "ldso_undist_group_create" in str(err.value)
    V, W = make("A"), make("B")
    with pytest.raises(binding.LdsoError) as err:                                            # the same member twice
        binding.UndistorterGroup([V, V])
    assert err.value.code == -1
    with pytest.raises(binding.LdsoError) as err:                                            # members on their own streams
        binding.UndistorterGroup([V, W])
    assert err.value.code == -1 and "stream" in str(err.value)
    assert L.ldso_undist_destroy(G.U[0].h) == -1 and "ldso_undist_destroy" in L.ldso_last_error().decode()
    e = G.frames(specs)                                                                      # the member still works
    G.check(specs, e)
    G.g.close()
    H = binding.UndistorterGroup([G.U[0], G.U[1]])                                           # free to join another group
    H.close()
    for u in G.U:
        assert L.ldso_undist_destroy(u.h) == 0
        u.h = None
    # a member whose tables were never set
    X = binding.Undistorter(120, 90, 104, 72)
    for u in (V, X):
        u.set_stream(stream())
    configure(V, "A", specs[0])
    K = binding.UndistorterGroup([V, X])
    K.frames([g["raw8"], None], [uc.EXPOSURE] * 2, active=[1, 0])
    kept = V.get().tobytes()
    with pytest.raises(binding.LdsoError) as err:
        K.frames([g["raw8"], g["raw8"]], [uc.EXPOSURE] * 2)
    assert err.value.code == -1 and ENTRY in str(err.value) and "member 1" in str(err.value) and "ldso_undist_set_remap" in str(err.value)
    assert V.get().tobytes() == kept == solo("A", specs[0])[0].tobytes()
    K.close()
    for x in (pg2, pg3, *pyr2, *pyr3, V, W, X):
        x.close()


def test_profile():
    names, shapes = ("A", "B", "C"), ((104, 72, 3), (104, 72, 2), (120, 90, 1))
    G = Group(names)
    pyr, pg = pyramids(shapes)
    specs = (Spec(8, 2), Spec(16, 2), Spec(8, 1))
    G.g.profile(True)
    e = G.frames(specs, pyr_group=pg)
    us = G.g.profile(False)
    assert us.shape == (3,) and (us > 0).all(), us
    G.check(specs, e)
    for n, s, (_, _, lv), p in zip(names, specs, shapes, pyr):
        assert [x.tobytes() for x in levels_of(p)] == solo_levels(n, s, lv), n
    G.close()
    pg.close()
    for p in pyr:
        p.close()
