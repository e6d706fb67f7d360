"""CPU tests of the corner detector's yardsticks: the numpy restatement (tests/feature_detect_common.py) against the fixture recorded from the LDSO sources'
own FeatureDetector.cc (tests/golden/ref_detect_corners.npz, scripts/golden/make_ref_detect_corners.py), the host-side grid rule of the library against the
restatement, and the conditions the fixture must fulfil for the GPU tests to mean something."""
import ctypes as C

import numpy as np
import pytest

import feature_detect_common as fc
from ldso_amd import binding, synth, build as ldso_build


@pytest.fixture(scope="module")
def gold():
    g = fc.golden()
    dI = synth.make_images(g["image"].astype(np.float32), 1)[0]
    return g, dI, fc.detect(dI, int(g["n"]), g["B"], g["pattern"])


def test_restatement_equals_reference_fixture(gold):
    g, dI, R = gold
    F = R["features"]
    assert len(F) == len(g["u"]) and R["n_corners"] == int(g["n_corners"])
    assert np.array_equal(F["u"], g["u"]) and np.array_equal(F["v"], g["v"])
    assert np.array_equal(F["score"].view(np.uint32), g["score"].view(np.uint32))
    assert np.array_equal(F["is_corner"], g["is_corner"])
    assert np.array_equal(F["angle"].view(np.uint32), g["angle"].view(np.uint32))          # both sides are glibc's atan2f
    assert np.array_equal(F["descriptor"], g["descriptor"])
    q = fc.immature(dI, F)
    for k in ("color", "weights", "gradH", "energyTH"):
        assert np.array_equal(q[k].view(np.uint32), g[k].view(np.uint32)), k


GRID_SIZES = ((160, 128), (192, 144), (256, 192), (640, 480), (1232, 368))
GRID_EXACT = {(160, 128): (320,), (192, 144): (108, 432), (256, 192): (192, 768), (640, 480): (1200,), (1232, 368): (1771,)}          # nfeatInGrid == 1.0


def test_grid_rule_matches_restatement():
    if not __import__("os").path.exists(binding.lib_path()):
        ldso_build.build()
    exact = 0
    for (w, h) in GRID_SIZES:
        for n in sorted(set(range(50, 4001, 25)) | set(GRID_EXACT[(w, h)])):
            got, want = binding.Features.grid(w, h, n), fc.grid(w, h, n)
            assert got == {k: want[k] for k in got}, (w, h, n, got, want)
            if want["nfeatInGrid"] == int(want["nfeatInGrid"]):
                exact += 1
                assert want["per_cell"] == int(want["nfeatInGrid"]) + 1
    assert exact >= len(GRID_SIZES)
    # the table-driven shapes of the GPU tests
    assert [binding.Features.grid(*s)[k] for s in ((192, 144, 300), (192, 144, 120), (160, 128, 700)) for k in ("gridsize", "per_cell", "skip")] == [10, 2, 4, 15, 1, 3, 5, 1, 7]


def test_grid_rule_refuses_bad_arguments():
    for bad in ((0, 100, 10), (100, 100, 0), (100, 100, 100 * 100 + 1)):
        with pytest.raises(binding.LdsoError) as e:
            binding.Features.grid(*bad)
        assert e.value.code == -1 and "ldso_feat_grid" in str(e.value)


def test_fixture_conditions(gold):
    g, dI, R = gold
    F = R["features"]
    assert R["ties"] == 0                                              # no two equal scores among the top per_cell + 1 of any cell: std::sort's freedom is not used
    assert int((F["score"] <= R["score_th"]).sum()) >= 1               # the scoreTH rule decides something
    assert R["n_corners"] < R["n_candidates"]                          # and so does the suppression
    assert len(F) > 100 and R["n_corners"] > 30
    assert R["unsafe"][F["is_corner"] == 1].mean() < 0.02              # bits a one-ulp difference in cosf / sinf / atan2f could move: the cap of the GPU tests
    assert g["image"].dtype == np.uint8 and g["image"].shape == (144, 192) and int(g["n"]) == 300 and g["pattern"].size == 1024


@pytest.mark.parametrize("shape", ((192, 144, 300, 168, 59), (192, 144, 120, 28, 23), (160, 128, 700, 228, 88)))
def test_table_shapes(shape):
    """what the table-driven GPU shapes exercise: feature / corner counts, no ties, the unsafe-bit cap; 160 x 128 holds a feature under scoreTH"""
    w, h, n, nf, nc = shape
    R = fc.restated(w, h, n)
    F = R["features"]
    assert (len(F), R["n_corners"], R["ties"]) == (nf, nc, 0)
    assert R["unsafe"][F["is_corner"] == 1].mean() < 0.02
    if (w, h) == (160, 128):
        assert int((F["score"] <= R["score_th"]).sum()) >= 1


def test_feature_dtype_matches_header():
    assert synth.FEATURE_DTYPE.itemsize == 64 and synth.FEATURE_DTYPE.fields["descriptor"][1] == 24
