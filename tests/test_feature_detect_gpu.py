"""GPU tests of ldso_amd/csrc/features.hip: FeatureDetector::DetectCorners and the ImmaturePoint constructors on the device against the numpy restatement
(tests/feature_detect_common.py) and the fixture recorded from the LDSO sources (tests/golden/ref_detect_corners.npz).  One-level pyramids, small shapes."""
import numpy as np
import pytest

import feature_detect_common as fc
from ldso_amd import binding, synth

pytestmark = pytest.mark.gpu
ANGLE_TOL = 2e-6          # rad: eight float32 ulps at pi, several times the documented errors of both atan2f implementations
UNSAFE_CAP = 0.02


def run(irradiance, n, B=None, pattern=True, host=0, max_features=None, allow_nonfinite=False):
    h, w = irradiance.shape
    pyr = binding.Pyramid(w, h, 1).make_images(irradiance)
    det = binding.Features(w, h, max_features or binding.Features.grid(w, h, n)["capacity"] + 1, fc.golden()["pattern"] if pattern else None)
    det.set_response(B)
    code = 0
    try:
        nf, nc = det.detect(pyr, n, host)
    except binding.LdsoError as e:
        if not (allow_nonfinite and e.code == binding.E_NONFINITE):
            raise
        code, nf, nc = e.code, det.n, det.n_corners
    F, Q = det.get()
    assert len(F) == nf
    det.close(); pyr.close()
    return F, Q, nc, code


def check_against(F, Q, nc, R, dI, host=0):
    """everything the restatement fixes: exact but for the angle (tolerance) and the descriptor bits whose taps sit on an integer boundary"""
    W = R["features"]
    assert len(F) == len(W) and nc == R["n_corners"]
    assert np.array_equal(F["u"], W["u"]) and np.array_equal(F["v"], W["v"])
    assert np.array_equal(F["score"].view(np.uint32), W["score"].view(np.uint32))
    assert np.array_equal(F["is_corner"], W["is_corner"]) and np.array_equal(F["cell"], W["cell"])
    d = np.abs(F["angle"].astype(np.float64) - W["angle"])
    d = np.minimum(d, 2 * np.pi - d)
    print("max angle difference", d.max() if len(d) else 0.0)
    assert len(d) == 0 or d.max() <= ANGLE_TOL
    assert np.all(F["angle"][W["is_corner"] == 0] == 0)
    c = W["is_corner"] == 1
    if c.any():
        assert R["unsafe"][c].mean() <= UNSAFE_CAP
        diff = np.unpackbits(F["descriptor"] ^ W["descriptor"], axis=1, bitorder="little").astype(bool)
        print("descriptor bits differing (all / outside the mask)", int(diff.sum()), int((diff & ~R["unsafe"]).sum()))
        assert not (diff & ~R["unsafe"]).any()
    assert not F["descriptor"][~c].any()
    assert Q.tobytes() == fc.immature(dI, W, host).tobytes()


@pytest.mark.parametrize("shape", ((192, 144, 300), (192, 144, 120), (160, 128, 700)))
def test_shapes_against_restatement(shape):
    w, h, n = shape
    irr, dI = fc.scene(w, h)
    F, Q, nc, _ = run(irr, n, host=3)
    check_against(F, Q, nc, fc.restated(w, h, n), dI, host=3)


def test_against_reference_fixture():
    g = fc.golden()
    img = g["image"].astype(np.float32)
    F, Q, nc, _ = run(img, int(g["n"]), g["B"])
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


def test_response_table():
    w, h, n = 192, 144, 300
    irr, dI = fc.scene(w, h)
    F0, Q0, nc0, _ = run(irr, n)
    Fi, Qi, nci, _ = run(irr, n, np.arange(256, dtype=np.float32))
    assert F0.tobytes() == Fi.tobytes() and Q0.tobytes() == Qi.tobytes() and nc0 == nci          # NULL = the identity table
    Fb, Qb, ncb, _ = run(irr, n, fc.bent_response())
    R = fc.restated(w, h, n, response=True)
    assert not (len(Fb) == len(F0) and np.array_equal(Fb["u"], F0["u"]) and np.array_equal(Fb["v"], F0["v"]))          # the table changes the selection
    check_against(Fb, Qb, ncb, R, dI)


def periodic_image(w=192, h=144, seed=5):
    """period 4 in x: pixels four apart have bit-equal gradients, boxes and scores"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, 4)).astype(np.float32)
    return np.ascontiguousarray(np.tile(base, (1, w // 4)))


def test_tie_rule():
    irr = periodic_image()
    n = 300
    dI = synth.make_images(irr, 1)[0]
    R = fc.detect(dI, n, None, fc.golden()["pattern"])
    W = R["features"]
    g = R["grid"]["gridsize"]
    assert R["ties"] > 0 and len(W) > 50
    F, Q, nc, _ = run(irr, n)
    assert np.array_equal(F["u"], W["u"]) and np.array_equal(F["v"], W["v"]) and np.array_equal(F["score"].view(np.uint32), W["score"].view(np.uint32))
    assert np.array_equal(F["is_corner"], W["is_corner"]) and nc == R["n_corners"]
    # inside a cell: the first pick has no equal candidate four pixels to its left, so it sits in the cell's first four columns; the second pick is an
    # equal candidate of the same row further right (the gradients are multiples of 0.5, the sums exact: every box of a row holds the same two periods)
    first = np.r_[True, F["cell"][1:] != F["cell"][:-1]]
    assert np.all(F["u"][first].astype(int) % g < 4)
    twin = np.nonzero(~first)[0]
    assert len(twin) and np.all(F["score"][twin] == F["score"][twin - 1]) and np.all(F["u"][twin] > F["u"][twin - 1]) and np.all(F["v"][twin] == F["v"][twin - 1])
    assert np.all(F["u"][twin] - F["u"][twin - 1] < 5)
    # suppression (FeatureDetector.cc:111-114): of two equal candidates within five pixels the one later in the output stays
    both = twin[(F["score"][twin] > R["score_th"])]
    assert len(both) and not F["is_corner"][both - 1].any()


def test_empty_and_sparse_cells():
    flat = np.full((144, 192), 100.0, np.float32)
    F, Q, nc, code = run(flat, 300)
    assert len(F) == 0 and len(Q) == 0 and nc == 0 and code == 0
    one = flat.copy()
    one[60, 60] = 200.0          # four gradient pixels around it, spread over three cells: two of the cells hold fewer candidates than per_cell = 2
    dI = synth.make_images(one, 1)[0]
    R = fc.detect(dI, 300, None, fc.golden()["pattern"])
    assert len(R["features"]) == 4 and len(set(R["features"]["cell"])) == 3
    F, Q, nc, code = run(one, 300)
    assert code == 0
    check_against(F, Q, nc, R, dI)


def test_nonfinite_pixel():
    w, h, n = 192, 144, 300
    irr, dI = fc.scene(w, h)
    bad = irr.copy()
    nx, ny = 85, 65
    bad[ny, nx] = np.nan
    with pytest.raises(binding.LdsoError) as e:
        run(bad, n)
    assert e.value.code == binding.E_NONFINITE and "ldso_feat_detect" in str(e.value)
    F, Q, nc, code = run(bad, n, allow_nonfinite=True)
    assert code == binding.E_NONFINITE
    W = fc.restated(w, h, n)["features"]
    G = fc.restated(w, h, n)["grid"]
    g = G["gridsize"]

    def untouched(A):
        # cells whose staged patch [x0 - 4, x0 + g + 4) x [y0 - 4, y0 + g + 4) holds none of the pixels whose gradients the NaN changes
        x0, y0 = (A["cell"] // G["gridY"]) * g, (A["cell"] % G["gridY"]) * g
        return (nx + 1 < x0 - 4) | (nx - 1 >= x0 + g + 4) | (ny + 1 < y0 - 4) | (ny - 1 >= y0 + g + 4)
    a, b = F[untouched(F)], W[untouched(W)]
    assert len(b) > 100 and len(b) < len(W)
    assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["v"], b["v"]) and np.array_equal(a["score"].view(np.uint32), b["score"].view(np.uint32))


def test_two_calls_are_byte_identical():
    w, h, n = 160, 128, 700
    irr, _ = fc.scene(w, h)
    pyr = binding.Pyramid(w, h, 1).make_images(irr)
    det = binding.Features(w, h, 400, fc.golden()["pattern"])
    det.detect(pyr, n)
    F1, Q1 = det.get()
    det.detect(pyr, n)
    F2, Q2 = det.get()
    assert len(F1) == 228 and F1.tobytes() == F2.tobytes() and Q1.tobytes() == Q2.tobytes()
    det.close(); pyr.close()


def test_capacity_is_checked():
    w, h, n = 192, 144, 300
    irr, _ = fc.scene(w, h)
    pyr = binding.Pyramid(w, h, 1).make_images(irr)
    det = binding.Features(w, h, binding.Features.grid(w, h, n)["capacity"] - 1)
    with pytest.raises(binding.LdsoError) as e:
        det.detect(pyr, n)
    assert e.value.code == -1 and "ldso_feat_detect" in str(e.value)
    det.close(); pyr.close()


def test_without_pattern_angles_only():
    w, h, n = 192, 144, 120
    irr, dI = fc.scene(w, h)
    F, Q, nc, _ = run(irr, n, pattern=False)
    R = fc.restated(w, h, n)
    assert not F["descriptor"].any() and nc == R["n_corners"]
    assert np.abs(F["angle"].astype(np.float64) - R["features"]["angle"]).max() <= ANGLE_TOL and np.abs(F["angle"]).max() > 1e-2


def test_append_points_device():
    w, h, n = 192, 144, 120
    irr, _ = fc.scene(w, h)
    pyr = binding.Pyramid(w, h, 1).make_images(irr)
    det = binding.Features(w, h, 64, fc.golden()["pattern"])
    nf, _ = det.detect(pyr, n, 2)
    _, Q = det.get()
    win = synth.make_window(F=2, P=50, w=w, h=h, fx=w * 0.6, seed=71)
    a, _ = synth.make_immature_points(win, 5)
    tr = binding.Tracer(w, h, len(a) + nf + 3)
    tr.set_points(a)
    _, imm_dev, cnt = det.device_ptrs()
    assert cnt == nf == 28
    tr.append_points_device(cnt, imm_dev)
    got = tr.get_points()
    assert len(got) == len(a) + nf and got.tobytes() == np.concatenate([a, Q]).tobytes()
    with pytest.raises(binding.LdsoError) as e:
        tr.append_points_device(cnt, imm_dev)          # 10 + 28 + 28 > 41
    assert e.value.code == -1 and "ldso_trace_append_points_device" in str(e.value)
    assert len(tr.get_points()) == len(a) + nf
    tr.close(); det.close(); pyr.close()
