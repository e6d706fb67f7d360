"""A scene that drives ImmaturePoint::traceOn (reference src/internal/ImmaturePoint.cc:47-310) through the paths the synthetic windows never reach, for
tests/test_trace_branches_*.py and the fixture tests/golden/ref_trace_branches.npz (scripts/golden/make_ref_trace_branches.py): more than 64 search steps
(the second pass of k_trace_on), the clamp to 99, tied best energies, y-dominant epipolar lines, non-finite taps, non-finite intervals, the scale-change
exit, every tracer setting away from its default.

One 640 x 480 target image; the points' colours are sampled FROM it at a chosen inverse depth (Kt has length 100, so inverse depth 0.01 is one pixel of
disparity), which makes the true match known.  Everything is generated from SEED; nothing here reads a file.

The searches stay inside the image by construction (points in a centre box, interval ends at least 12 px from the border); the oracle's diagnostics column
TD_MARGIN says so per point, and tests/test_trace_branches_cpu.py asserts it before any device runs the scene."""
import numpy as np

from ldso_amd import synth

SEED = 20261018
W, H = 640, 480
CX, CY = 319.5, 239.5
T = 100.0                              # |Kt|: pixels of disparity per unit of inverse depth
BOX = (125, 515, 125, 355)             # u0, u1, v0, v1 of the points
PERIODIC_ROWS = (228, 268)             # I = tab[x % 16]: steps 16 apart have exactly equal energies
ZERO_ROWS = (298, 318)
NAN_PATCH = (200, 170)                 # x, y of the 4 x 4 patches
INF_PATCH = (440, 300)
GRADNAN_BLOCK = (150, 190, 380, 420)   # x0, x1, y0, y1: NaN in the GRADIENT channels, only in the image of the call "gradnan"
N_HOSTS = 8
ZOOM_HOST, ROT_HOST, AFF_HOST = 7, 5, 6

_SCENE = None


def _upsample(rng, gh, gw):
    c = rng.random((gh + 1, gw + 1))
    ys = np.linspace(0, gh, H); xs = np.linspace(0, gw, W)
    rows = np.stack([np.interp(xs, np.arange(gw + 1), c[j]) for j in range(gh + 1)])            # [gh+1, W]
    return np.stack([np.interp(ys, np.arange(gh + 1), rows[:, i]) for i in range(W)], axis=1)     # [H, W]


def make_image(rng):
    """irradiance float32 [H, W]: smooth random texture, a band of period 16 along x, a band of zeros, a NaN and a +Inf patch"""
    I = (20 + 110 * _upsample(rng, 12, 16) + 70 * _upsample(rng, 48, 64) + 45 * _upsample(rng, 120, 160)).astype(np.float32)
    tab = (128 + 90 * np.sin(2 * np.pi * np.arange(16) / 16) + 20 * rng.random(16)).astype(np.float32)
    I[PERIODIC_ROWS[0]:PERIODIC_ROWS[1], :] = tab[np.arange(W) % 16][None, :]
    I[ZERO_ROWS[0]:ZERO_ROWS[1], :] = 0
    I[NAN_PATCH[1]:NAN_PATCH[1] + 4, NAN_PATCH[0]:NAN_PATCH[0] + 4] = np.nan
    I[INF_PATCH[1]:INF_PATCH[1] + 4, INF_PATCH[0]:INF_PATCH[0] + 4] = np.inf
    return I


def make_hosts():
    """KRKi [8, 9], Kt [8, 3], aff [8, 2]: +x, -x, +y, -y, two diagonals (the second rotated in plane about the image centre), (0.6, 0.8) with an affine
    pair other than (1, 0), and a forward motion (Kt[2] = 0.8: a zoom about the image centre plus (0.6, -0.8))"""
    KRKi = np.tile(np.eye(3, dtype=np.float32).ravel(), (N_HOSTS, 1))
    c, s = np.cos(0.2), np.sin(0.2)
    KRKi[ROT_HOST] = np.array([[c, -s, CX - c * CX + s * CY], [s, c, CY - s * CX - c * CY], [0, 0, 1]], np.float32).ravel()
    Kt = np.array([[T, 0, 0], [-T, 0, 0], [0, T, 0], [0, -T, 0], [71, 71, 0], [71, -71, 0], [60, 80, 0], [CX * 0.8 + 60, CY * 0.8 - 80, 0.8]], np.float32)
    aff = np.tile(np.array([1, 0], np.float32), (N_HOSTS, 1))
    aff[AFF_HOST] = (1.1, -3.0)
    return KRKi, Kt, aff


def project(KRKi, Kt, host, u, v, idepth):
    M = KRKi[host].reshape(3, 3).astype(np.float64)
    p = M @ np.array([u, v, 1.0]) + Kt[host].astype(np.float64) * idepth
    return p[0] / p[2], p[1] / p[2]


def _sample(dI, KRKi, aff, host, x, y):
    """colour (in the host's brightness), weights and gradH of the 8-pattern around (x, y) of the target image, as synth.make_immature_points computes them"""
    M = KRKi[host].reshape(3, 3)
    rx = np.array([M[0, 0] * px + M[0, 1] * py for px, py in synth.PATTERN], np.float32)
    ry = np.array([M[1, 0] * px + M[1, 1] * py for px, py in synth.PATTERN], np.float32)
    with np.errstate(invalid="ignore"):
        c, gx, gy = synth.interp_bilin33(dI, np.float32(x) + rx, np.float32(y) + ry)
    wgt = np.sqrt(np.float32(2500.0) / (np.float32(2500.0) + (gx * gx + gy * gy))).astype(np.float32)
    gh = np.array([(gx * gx).sum(), (gx * gy).sum(), (gx * gy).sum(), (gy * gy).sum()], np.float32)
    color = ((c - aff[host, 1]) / aff[host, 0]).astype(np.float32)
    return color, wgt, gh


def _inside(x, y, m):
    return m <= x <= W - 1 - m and m <= y <= H - 1 - m


def make_points(n, rng, dI, hosts, finite):
    """n fresh immature points (idepth interval [0, NaN)), or with finite=True with hand-made intervals around the true inverse depth -> records, true idepth"""
    KRKi, Kt, aff = hosts
    out = np.zeros(n, synth.IMMATURE_DTYPE)
    true_id = np.zeros(n, np.float32)
    out["energyTH"] = 8 * 12 * 12; out["quality"] = 10000.0; out["lastTraceStatus"] = 5; out["lastTraceUV"] = -1.0
    out["idepth_min"] = 0.0; out["idepth_max"] = np.nan
    for i in range(n):
        kind = i % 20
        for _ in range(1000):
            host = int(rng.integers(0, N_HOSTS))
            u = float(rng.integers(BOX[0], BOX[1])); v = float(rng.integers(BOX[2], BOX[3]))
            frac = i % 3
            if frac == 1:
                u += 0.25 * rng.integers(0, 4); v += 0.25 * rng.integers(0, 4)
            elif frac == 2:
                u = float(np.float32(u + rng.random())); v = float(np.float32(v + rng.random()))
            disp = rng.uniform(0, 112)
            if kind in (0, 1, 2):                                    # in the periodic band, along x: tied energies 16 steps apart
                host = int(rng.integers(0, 2)); v = float(rng.integers(PERIODIC_ROWS[0] + 4, PERIODIC_ROWS[1] - 5)); u = float(int(u)) + 0.25 * rng.integers(0, 4)
                disp = float(rng.integers(0, 100)) + 0.5 * rng.integers(0, 2)
            elif kind == 3:                                          # in the zero band: every energy equal, zero gradient
                host = int(rng.integers(0, 2)); v = float(rng.integers(ZERO_ROWS[0] + 4, ZERO_ROWS[1] - 5))
            elif kind == 4:
                disp = float(rng.choice([64, 64.25, 65, 65.5, 66]))   # best step right behind the end of the first pass
            elif kind == 5:
                disp = rng.uniform(96, 97.6)                         # ... and at the end of the second
            elif kind == 6:
                disp = rng.uniform(99, 118)                          # beyond every search: the match is not on the line
            elif kind == 7 and i % 40 == 7:
                disp = 0.0
            elif kind == 7:
                disp = -rng.uniform(1.5, 3.0)                        # behind the start of the line: the new interval ends below zero
            elif kind == 12:                                         # a non-finite patch on the search line, 10 to 100 steps from its start
                host = int(rng.choice([0, 1, 2, 3, 4, 6]))
                px, py = NAN_PATCH if i % 40 == 12 else INF_PATCH
                k = rng.uniform(10, 100) / T
                u = float(np.float32(px + 2 * rng.random() - Kt[host, 0] * k)); v = float(np.float32(py + 2 * rng.random() - Kt[host, 1] * k))
                if not (BOX[0] <= u <= BOX[1] and BOX[2] <= v <= BOX[3]):
                    continue
            idt = disp / T
            x, y = project(KRKi, Kt, host, u, v, idt)
            if not _inside(x, y, 9):
                continue
            lo = hi = None
            if finite:
                width = 1.0 + 99.0 * ((i * 0.6180339887) % 1.0)
                a = min(width * rng.random(), disp + 3.0)
                lo, hi = (disp - a) / T, (disp - a + width) / T
                if kind == 8:
                    hi = lo                                          # zero width
                elif kind == 9:
                    lo, hi = hi, lo                                  # handed over in the wrong order
                ends = [project(KRKi, Kt, host, u, v, d) for d in (lo, hi)]
                if not all(_inside(ex, ey, 13) for ex, ey in ends):
                    continue
            color, wgt, gh = _sample(dI, KRKi, aff, host, x, y)
            if not (np.isfinite(color).all() and np.isfinite(wgt).all() and np.isfinite(gh).all()):
                continue                                             # the point's own pattern touches a non-finite pixel
            break
        else:
            raise RuntimeError("trace_branch_common: no admissible point")
        p = out[i]
        p["u"] = u; p["v"] = v; p["host"] = host; p["color"] = color; p["weights"] = wgt; p["gradH"] = gh
        true_id[i] = idt
        if finite:
            p["idepth_min"] = lo; p["idepth_max"] = hi
        if kind == 10 and i % 40 == 10:
            p["gradH"] = 0                                           # errorInPixel = 0.2 + 0.2 * (0 / 0)
        if kind == 11 and i % 80 == 11:
            p["host"] = (-1, N_HOSTS, N_HOSTS + 3)[(i // 80) % 3]     # no such host: the record stays as it is
    return out, true_id


def _aim_at(pts, true_id, idx, rng, dI, hosts, target_xy, disp, half_width, color_offset):
    """rewrite points idx: hosts 0 / 2 (+x / +y), placed so that inverse depth disp / T lands on target_xy, interval disp -+ half_width pixels, colours sampled
    color_offset pixels further along the line"""
    KRKi, Kt, aff = hosts
    for j, i in enumerate(idx):
        host = (0, 2)[j % 2]
        d = np.array([1.0, 0.0]) if host == 0 else np.array([0.0, 1.0])
        off = np.array([(j % 3) - 1.0, ((j // 3) % 3) - 1.0]) * 0.75
        u, v = np.float32(target_xy[0] + off[0] - d[0] * disp), np.float32(target_xy[1] + off[1] - d[1] * disp)
        x, y = project(KRKi, Kt, host, u, v, (disp + color_offset) / T)
        color, wgt, gh = _sample(dI, KRKi, aff, host, x, y)
        assert np.isfinite(color).all() and np.isfinite(wgt).all() and np.isfinite(gh).all()
        p = pts[i]
        p["u"] = u; p["v"] = v; p["host"] = host; p["color"] = color; p["weights"] = wgt; p["gradH"] = gh
        p["idepth_min"] = (disp - half_width) / T; p["idepth_max"] = (disp + half_width) / T
        true_id[i] = (disp + color_offset) / T


def settings(**kw):
    s = synth.default_trace_settings()
    for k, val in kw.items():
        s[k] = val
    return s


def scene():
    """dict: color [H, W] (irradiance), dI = level 0 of synth.make_images(color), dI_gradnan, hosts (KRKi, Kt, aff), calls.
    A call is a dict: name, pts (the records it starts from: copy them), settings, image ("dI" or "dI_gradnan"), second (trace a second time from the records of the
    first), raw (the device test passes the irradiance through set_frame_raw), golden (recorded in the fixture)."""
    global _SCENE
    if _SCENE is not None:
        return _SCENE
    rng = np.random.default_rng(SEED)
    color = make_image(rng)
    with np.errstate(invalid="ignore"):                # the NaN and Inf patches pass through the gradient stencil
        dI = synth.make_images(color, 1)[0]
    hosts = make_hosts()
    fresh, fresh_id = make_points(401, rng, dI, hosts, finite=False)
    fin, fin_id = make_points(403, rng, dI, hosts, finite=True)
    # six points whose short interval lies ON the NaN patch while their colours come from 20 px further: every step has a non-finite tap, so has the refinement
    _aim_at(fin, fin_id, [392, 393, 394, 395, 396, 397], rng, dI, hosts, (NAN_PATCH[0] + 2.0, NAN_PATCH[1] + 2.0), 30.0, 1.5, 20.0)
    # the image of the call "gradnan": a block of NaN in the gradient channels only.  makeImages never writes one (it zeroes them, FrameHessian.cc:86-87), and
    # with finite colours, weights and affine values nothing else makes the Gauss-Newton step non-finite; ldso_trace_set_frame takes any (I, dx, dy).
    dI_g = dI.copy()
    gx0, gx1, gy0, gy1 = GRADNAN_BLOCK
    dI_g[gy0:gy1, gx0:gx1, 1:] = np.nan
    grad, grad_id = make_points(41, rng, dI, hosts, finite=True)
    _aim_at(grad, grad_id, list(range(41)), rng, dI, hosts, (0.5 * (gx0 + gx1), 0.5 * (gy0 + gy1)), 40.0, 6.0, 0.0)
    calls = []
    for mp, steps in ((62.5, 64), (63.5, 65), (84.0, 85), (112.0, 99)):
        calls.append(dict(name=f"inf{steps}", pts=fresh, settings=settings(maxPixSearch=mp / (W + H)), second=True, golden=steps in (85, 99), raw=steps == 85))
    wide = dict(maxPixSearch=112.0 / (W + H))
    calls.append(dict(name="finite", pts=fin, settings=settings(**wide), second=True, golden=True))
    for name, kw in (("gn0", dict(trace_GNIterations=0)), ("radius0", dict(minTraceTestRadius=0)), ("radius120", dict(minTraceTestRadius=120)),
                     ("step05", dict(trace_stepsize=0.5)), ("step2", dict(trace_stepsize=2.0)), ("slack0", dict(trace_slackInterval=0.0))):
        calls.append(dict(name=name, pts=fin, settings=settings(**wide, **kw), second=False))
    calls.append(dict(name="default_fresh", pts=fresh, settings=settings(), second=True))
    calls.append(dict(name="default_finite", pts=fin, settings=settings(), second=False))
    calls.append(dict(name="single", pts=fresh[37:38].copy(), settings=settings(maxPixSearch=84.0 / (W + H)), second=False))
    calls.append(dict(name="gradnan", pts=grad, settings=settings(**wide), image="dI_gradnan", second=False))
    # a NaN handed in through gradH: errorInPixel and the new interval carry ITS bits (sign and payload, quieted), not those of a NaN made by 0 / 0
    gh = fresh[40:52].copy()
    gh["host"] = np.where((gh["host"] < 0) | (gh["host"] >= N_HOSTS), 0, gh["host"])
    for j, (k, bits) in enumerate(((0, 0x7FC00000), (3, 0x7FC00000), (1, 0xFFC12345), (2, 0x7F812345), (0, 0xFFFFFFFF), (3, 0x7FC00001))):
        gh["gradH"][2 * j:2 * j + 2, k] = np.array([bits], np.uint32).view(np.float32)[0]
    calls.append(dict(name="gradh_nan", pts=gh, settings=settings(maxPixSearch=84.0 / (W + H)), second=False))
    for c in calls:
        c.setdefault("image", "dI"); c.setdefault("raw", False); c.setdefault("golden", False)
    _SCENE = dict(color=color, dI=dI, dI_gradnan=dI_g, hosts=hosts, calls=calls, w=W, h=H)
    return _SCENE


def call_names():
    return [c["name"] for c in scene()["calls"]]


def get_call(name):
    return next(c for c in scene()["calls"] if c["name"] == name)


def run(call, trace_fn):
    """the call through trace_fn (pyoracle.trace_on, pyref.trace_on: same signature) -> [(counts, records)] for its one or two traces"""
    sc = scene()
    KRKi, Kt, aff = sc["hosts"]
    pts = call["pts"].copy()
    out = []
    for _ in range(2 if call["second"] else 1):
        counts = trace_fn(pts, sc[call["image"]], KRKi, Kt, aff, call["settings"])
        out.append((np.asarray(counts).copy(), pts.copy()))
    return out


_ORACLE = {}


def oracle(name):
    """run(call, pyoracle.trace_on), computed once per call and shared (treat as read-only)"""
    if name not in _ORACLE:
        from oracle import pyoracle as po
        _ORACLE[name] = run(get_call(name), po.trace_on)
    return _ORACLE[name]
