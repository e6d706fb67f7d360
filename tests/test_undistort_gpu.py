"""ldso_undist_* (ldso_amd/csrc/undistort.hip) on the device: bit for bit the outputs recorded from the reference's own Undistort::undistort<T>
(tests/golden/ref_undistort.npz) and, for shapes without a recording, the numpy restatement of tests/undistort_common.py."""
import numpy as np
import pytest

import undistort_common as uc
from ldso_amd import binding
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def undistorter(c):
    w_org, h_org, w, h, rx, ry = uc.case(c)
    U = binding.Undistorter(w_org, h_org, w, h)
    U.set_remap(rx, ry)
    return U


@pytest.mark.parametrize("c", uc.CASES)
def test_recorded_cases_bit_for_bit(c):
    g = uc.golden()
    U = undistorter(c)
    vig = g["vignetteMapInv"]
    for pc in (2, 1, 0):          # setting_photometricCalibration
        U.set_photometric(g["G256"], vig, pc)
        assert U.frame(g["raw8"], uc.EXPOSURE, 1.0) == np.float32(uc.EXPOSURE)
        assert same_bits(U.get(), g[f"{c}_u8_m{pc}"]), pc
    # a factor on a calibrated path changes nothing; exposure <= 0 takes the plain path, where it shows
    U.set_photometric(g["G256"], vig, 2)
    U.frame(g["raw8"], uc.EXPOSURE, 0.7)
    assert same_bits(U.get(), g[c + "_u8_m2"])
    assert U.frame(g["raw8"], 0.0, 0.7) == g[c + "_exposure"][1] == 0.0
    assert same_bits(U.get(), g[c + "_u8_e0"])
    U.frame(g["raw8"], -1.0, 1.0)
    assert same_bits(U.get(), g[c + "_u8_m0"])
    # no valid calibration: plain as well
    U.set_photometric(None, None, 2)
    U.frame(g["raw8"], uc.EXPOSURE, 0.7)
    assert same_bits(U.get(), g[c + "_u8_e0"])
    # setting_useExposure off
    U.set_photometric(g["G256"], vig, 2, use_exposure=False)
    assert U.frame(g["raw8"], uc.EXPOSURE, 1.0) == g[c + "_exposure"][2] == 1.0
    assert same_bits(U.get(), g[c + "_u8_m2"])
    # the 16-bit frame with the 65536-entry response
    U.set_photometric(g["G65536"], vig, 2)
    U.frame(g["raw16"], uc.EXPOSURE, 1.0)
    assert same_bits(U.get(), g[c + "_u16_m2"])
    assert not np.isfinite(U.get()).all()          # the infinite vignette entry arrived
    # ... its other two paths, against the rows of the reference's output that the fixture holds
    U.set_photometric(g["G65536"], vig, 1)
    U.frame(g["raw16"], uc.EXPOSURE, 1.0)
    assert same_bits(U.get()[::uc.SAMPLE_ROWS], g[c + "_u16_m1_rows"])
    U.frame(g["raw16"], 0.0, 1.0 / 256)
    assert same_bits(U.get()[::uc.SAMPLE_ROWS], g[c + "_u16_e0_rows"])
    U.close()


def test_error_paths():
    g = uc.golden()
    U = undistorter("A")
    U.set_photometric(g["G256"], g["vignetteMapInv"], 2)
    with pytest.raises(binding.LdsoError) as e:          # 16-bit pixels would index past a 256-entry response
        U.frame(g["raw16"], uc.EXPOSURE, 1.0)
    assert e.value.code == -1
    U.frame(g["raw16"], 0.0, 1.0)                        # ... which the plain path never reads
    assert same_bits(U.get(), uc.undistort(g["raw16"], g["A_remapX"], g["A_remapY"], 120, 90, 104, 72))
    for bad in (np.nan, np.inf, -np.inf):
        rx = g["A_remapX"].copy()
        rx[5, 7] = bad
        for tabs in ((rx, g["A_remapY"]), (g["A_remapX"], rx)):
            with pytest.raises(binding.LdsoError) as e:
                U.set_remap(*tabs)
            assert e.value.code == -1
    with pytest.raises(binding.LdsoError) as e:          # passthrough needs equal sizes
        U.set_remap(None, None)
    assert e.value.code == -1
    with pytest.raises(binding.LdsoError) as e:          # mode 2 needs the vignette
        U.set_photometric(g["G256"], None, 2)
    assert e.value.code == -1
    # the tables of before the rejected calls are still in place
    U.frame(g["raw8"], uc.EXPOSURE, 1.0)
    assert same_bits(U.get(), g["A_u8_m2"])
    U.close()
    V = binding.Undistorter(120, 90, 104, 72)
    with pytest.raises(binding.LdsoError):               # no tables yet
        V.frame(g["raw8"], 1.0, 1.0)
    V.close()


def test_adversarial_entries_give_zero():
    g = uc.golden()
    ax, ay = uc.adversarial_entries(120, 90)
    n = len(ax)
    # a valid table with the adversarial entries written over its first pixels; everything else must stay what it was
    rx, ry = g["A_remapX"].copy(), g["A_remapY"].copy()
    rx.ravel()[:n], ry.ravel()[:n] = ax, ay
    U = binding.Undistorter(120, 90, 104, 72)
    U.set_remap(rx, ry)
    for raw, G in (("raw8", "G256"), ("raw16", "G65536")):
        for pc in (2, 1, 0):
            U.set_photometric(g[G], g["vignetteMapInv"], pc)
            U.frame(g[raw], uc.EXPOSURE, 1.0)
            out = U.get()
            assert not out.ravel()[:n].any()
            assert same_bits(out, uc.undistort(g[raw], rx, ry, 120, 90, 104, 72, g[G], g["vignetteMapInv"], pc))
    U.close()


@pytest.mark.parametrize("shape", [((67, 53), (33, 29)), ((40, 30), (96, 64)), ((120, 90), (104, 72))])
def test_shapes_against_the_restatement(shape):
    (w_org, h_org), (w, h) = shape
    rx, ry = uc.synthetic_tables(w_org, h_org, w, h, seed=w)
    ok, _, _ = uc.taps_inside(rx, ry, w_org, h_org)
    assert 0 < (~ok).sum() < ok.size          # both branches
    f8, f16 = uc.textured_frames(w_org, h_org, seed=h)
    rng = np.random.default_rng(5)
    vig = (1.0 / rng.uniform(0.3, 1.0, (h_org, w_org))).astype(np.float32)
    g = uc.golden()
    U = binding.Undistorter(w_org, h_org, w, h)
    U.set_remap(rx, ry)
    for raw, G in ((f8, g["G256"]), (f16, g["G65536"])):
        for pc, exposure, factor in ((2, 1.0, 1.0), (1, 2.0, 1.0), (0, 1.0, 1.3), (2, 0.0, 0.25)):
            U.set_photometric(G, vig, pc)
            U.frame(raw, exposure, factor)
            assert same_bits(U.get(), uc.undistort(raw, rx, ry, w_org, h_org, w, h, G, vig, uc.mode_of(G, exposure, pc), factor)), (pc, exposure)
    U.close()


def test_into_a_pyramid_every_level_and_repeatable():
    g = uc.golden()
    U = undistorter("B")
    U.set_photometric(g["G256"], g["vignetteMapInv"], 1)
    irr = g["B_u8_m1"]
    want = po.make_images(irr, 3)
    P, Q = binding.Pyramid(104, 72, 3), binding.Pyramid(104, 72, 3)
    U.frame(g["raw8"], uc.EXPOSURE, 1.0, pyr=P)
    first = [P.get_level(l) for l in range(3)]
    for l in range(3):
        assert same_bits(first[l], want[l]), l
    assert same_bits(U.get(), first[0][..., 0])          # ldso_undist_get = channel 0 of level 0
    assert U.device_ptr() != 0
    # another frame in between, then the same input again into another pyramid: identical buffers
    U.frame(g["raw16"], 0.0, 1.0, pyr=Q)
    U.frame(g["raw8"], uc.EXPOSURE, 1.0, pyr=Q)
    for l in range(3):
        assert Q.get_level(l).tobytes() == first[l].tobytes()
        assert P.get_level(l).tobytes() == first[l].tobytes()          # the first pyramid is untouched
    # the pyramid built from the same irradiance uploaded from the host (today's path)
    R = binding.Pyramid(104, 72, 3).make_images(irr)
    for l in range(3):
        assert R.get_level(l).tobytes() == first[l].tobytes()
    us = U.profile(True)
    U.frame(g["raw8"], uc.EXPOSURE, 1.0, pyr=Q)
    us = U.profile(False)
    assert (us > 0).all() and same_bits(U.get(), irr)
    with pytest.raises(binding.LdsoError):               # a pyramid of another size
        U.frame(g["raw8"], uc.EXPOSURE, 1.0, pyr=binding.Pyramid(120, 90, 3))
    for x in (P, Q, R, U):
        x.close()
