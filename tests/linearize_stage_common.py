"""What tests/test_linearize_stage_cpu.py and tests/test_linearize_stage_gpu.py share: a float64 reference of ONE linearisation pass of the windowed bundle
adjustment (PointFrameResidual::linearize + applyRes / takeData, AccumulatedTopHessianSSE::addPoint<0 | 1>, AccumulatedSCHessianSSE::addPoint and the two stitches,
the HFinal | bFinal of EnergyFunctional::solveSystemF - what linearize_body, k_reduce and k_gather restate), its error scale, the cases and the assertion both files make.

The reference computes everything in float64 FROM THE FLOAT32 INPUTS THE IMPLEMENTATION ITSELF USES: the per-pair records of get_precalc() (KRKi, Kt, R0, t0, aff, b0),
the float32 point records, the level-0 image triples, the settings, the frames' frameEnergyTH, the calibration as float32(fx), float32(1 / fx) ..., and the adjoints (the
float64 of EnergyFunctional::setAdjointsF from the frames' evalPT, with the affine factor rounded through float as both implementations do).  oracle/spec_np.py, which
recomputes the pair geometry from the poses, stays the independent model; test_linearize_stage_cpu.py holds the two together.

ERROR SCALE.  Every quantity is a V: its value v and S, the sum of the absolute values of its addends, composed through the arithmetic to first order:
    input (a float32 the implementation reads)   S = |v|                       a + b   S = S_a + S_b
    a * b   S = S_a |b| + |a| S_b - |a b|        a / b   S = S_a / |b| + |a| S_b / b^2 - |a / b|          sqrt(a)   S = (sqrt(a) + S_a / sqrt(a)) / 2
    bilinear tap   S = sum of weight x |corner| + (S_x + S_y) x (largest - smallest corner)   (the tap-composition scale of init_stage_common._taps)
so that S / |v| - 1 is the sum of the relative excesses of the factors: a product of inputs has S = |v|, a sum that cancels keeps the size of what cancelled.  An
implementation is measured per entry in UNITS of eps32 * S (eps32 = 2^-24), so a small entry is held to its own size and not to that of the largest one.

DECISIONS.  In the image (centre and the 8 pattern pixels), drescale > 0, the Huber branch per pixel, outlier against max(frameEnergyTH) and wJI2_sum < 2 are taken by
the reference itself, each with its margin.  Where a margin is under the guard (GUARD_PX pixels at a border and for the depth, GUARD_REL relative at a threshold) the
reference ADOPTS the implementation's decision: the residual state it reports (OOB / OUTLIER / IN), and for a pattern pixel at the Huber threshold the combination of
branches whose energy is nearest to everything it reports for that residual (energy, JpJdF, the dumped Jacobians).  Everywhere else state_NewState is compared bit for bit.  The residuals whose decision was
under a guard are counted (adoptions); a case may have at most ADOPT_CAP of them.

Modelled on purpose (each a place where a float64 reference would otherwise round differently from BOTH implementations):
  * il = 1 / (1 + lambda) of the Schur part of HFinal is the double both implementations form (`1.0f / (1 + lambda)` divides in double);
  * the priors enter HL / HFinal exactly (they are doubles added in double): their share of S is prior * 2^-29, the float64 rounding in units of eps32;
  * dp = adHTdeltaF (the delta of a pair for the linearised residuals) is formed from the float32 adjoints, as setDeltaF does."""
import copy
import functools
import types

import numpy as np

from ldso_amd import synth
from ldso_amd.synth import SCALE_A, SCALE_B, SCALE_C, SCALE_F, SCALE_XI_ROT, SCALE_XI_TRANS
from init_stage_common import FLOOR_UNITS, ORACLE_FACTOR, GUARD_PX, GUARD_REL, _units

ADOPT_CAP = 0.02
IN, OOB, OUTLIER = 0, 1, 2
PAT = synth.PATTERN.astype(np.float64)
F32 = lambda x: np.asarray(x, np.float32).astype(np.float64)

PER_RES = ("state_NewEnergy", "JpJdF", "centerProjectedTo")
DUMP = ("resF", "JIdx", "JabF", "Jpdxi", "Jpdc", "Jpdd", "JIdx2", "JabJIdx", "Jab2")
PER_POINT_ACC = ("Hdd_accAF", "bd_accAF", "Hcd_accAF")
PER_POINT_SOLVE = ("HdiF", "bdSumF", "idepth_hessian")
PER_POINT_L = ("Hdd_accLF", "bd_accLF", "Hcd_accLF")
SYSTEM = ("HA", "bA", "Hsc", "bsc")
SYSTEM_L = ("HL", "bL")
FINAL = ("HFinal", "bFinal")
QUANTITIES = PER_RES + DUMP + PER_POINT_ACC + PER_POINT_SOLVE + PER_POINT_L + SYSTEM + SYSTEM_L + FINAL
FAULTS = ("drop_pixel7", "drop_residual", "swap_adjoint", "no_sqrt_huber", "b0_current", "geo_current_idepth", "hcd_neighbour")

# The yardstick: the worst the oracle (oracle/backend.cc, the float32 restatement of the reference project) shows on any case of CASES, per quantity, in units of
# eps32 * S, rounded up.  test_linearize_stage_cpu.py asserts that the oracle stays within it; the kernel's bound is max(FLOOR_UNITS, ORACLE_FACTOR x yardstick).
# (DESIGN.md section 9 carries the same table.)
YARDSTICK = {
    "state_NewEnergy": 1.4, "JpJdF": 1.5, "centerProjectedTo": 3.2,
    "resF": 3.8, "JIdx": 3.0, "JabF": 2.7, "Jpdxi": 4.6, "Jpdc": 5.0, "Jpdd": 3.8, "JIdx2": 1.5, "JabJIdx": 1.3, "Jab2": 1.7,
    "Hdd_accAF": 0.65, "bd_accAF": 0.75, "Hcd_accAF": 1.0, "HdiF": 0.65, "bdSumF": 0.75, "idepth_hessian": 0.65,
    "Hdd_accLF": 2.2, "bd_accLF": 0.2, "Hcd_accLF": 2.1,
    "HA": 0.9, "bA": 0.12, "Hsc": 0.1, "bsc": 0.08, "HL": 2.4, "bL": 0.03, "HFinal": 0.17, "bFinal": 0.06,
}


def bounds():
    return {q: max(FLOOR_UNITS, ORACLE_FACTOR * YARDSTICK[q]) for q in QUANTITIES}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# values with their error scale
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
class V:
    __slots__ = ("v", "s")
    __array_ufunc__ = None

    def __init__(self, v, s=None):
        self.v = np.asarray(v, np.float64)
        self.s = np.abs(self.v) if s is None else np.asarray(s, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.s + o.s)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.s + o.s)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.s)

    def __mul__(self, o):
        o = V.of(o)
        a, b = np.abs(self.v), np.abs(o.v)
        return V(self.v * o.v, self.s * b + a * o.s - a * b)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            return V(v, self.s / np.abs(o.v) + np.abs(self.v) * o.s / (o.v * o.v) - np.abs(v))

    def __rtruediv__(self, o):
        return V.of(o) / self

    def sqrt(self):
        with np.errstate(all="ignore"):
            r = np.sqrt(self.v)
            return V(r, np.where(r > 0, 0.5 * (r + self.s / np.where(r > 0, r, 1.0)), 0.0))

    def sum(self, axis):
        return V(self.v.sum(axis=axis), self.s.sum(axis=axis))

    def __getitem__(self, i):
        return V(self.v[i], self.s[i])

    def where(self, m, other=0.0):
        o = V.of(other)
        return V(np.where(m, self.v, o.v), np.where(m, self.s, o.s))

    @property
    def shape(self):
        return self.v.shape


def vstack(xs, axis=-1):
    xs = [V.of(x) for x in xs]
    shp = np.broadcast_shapes(*[x.shape for x in xs])
    return V(np.stack([np.broadcast_to(x.v, shp) for x in xs], axis), np.stack([np.broadcast_to(x.s, shp) for x in xs], axis))


def vcat(xs, axis):
    return V(np.concatenate([x.v for x in xs], axis), np.concatenate([x.s for x in xs], axis))


def veinsum(spec, a, b):
    """einsum of two V with the product rule on S"""
    a, b = V.of(a), V.of(b)
    aa, ab = np.abs(a.v), np.abs(b.v)
    return V(np.einsum(spec, a.v, b.v), np.einsum(spec, a.s, ab) + np.einsum(spec, aa, b.s) - np.einsum(spec, aa, ab))


def seg_sum(x, idx, n, mask=None):
    """sum of the rows of x (leading axis) into n bins"""
    if mask is not None:
        x, idx = x[mask], idx[mask]
    out = V(np.zeros((n,) + x.shape[1:]), np.zeros((n,) + x.shape[1:]))
    np.add.at(out.v, idx, x.v)
    np.add.at(out.s, idx, x.s)
    return out


def taps(imgs, t, x, y, ok):
    """bilinear (I, dx, dy) of image t [R] at the V positions (x, y) [R, 8] where ok (GlobalFuncs.h:89-103) -> V [R, 8, 3]"""
    xv, yv = np.where(ok, x.v, 1.0), np.where(ok, y.v, 1.0)
    ix, iy = xv.astype(np.int64), yv.astype(np.int64)
    dx, dy = (xv - ix)[..., None], (yv - iy)[..., None]
    tt = t[:, None]
    c = [imgs[tt, iy + 1, ix + 1], imgs[tt, iy + 1, ix], imgs[tt, iy, ix + 1], imgs[tt, iy, ix]]
    wt = [dx * dy, dy - dx * dy, dx - dx * dy, 1 - dx - dy + dx * dy]
    val = wt[0] * c[0] + wt[1] * c[1] + wt[2] * c[2] + wt[3] * c[3]
    pos = np.where(ok, x.s + y.s, 0.0)[..., None]
    sc = sum(wq * np.abs(cq) for wq, cq in zip(wt, c)) + pos * (np.maximum.reduce(c) - np.minimum.reduce(c))
    return V(val, sc)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def adjoints(frames):
    """EnergyFunctional::setAdjointsF (:431-489) in float64 -> adHost, adTarget [F, F (host, target), 8, 8]; the affine factor is rounded through float there"""
    F = len(frames)
    T = []
    for f in frames:
        M = np.eye(4); M[:3, :4] = np.asarray(f["worldToCam_evalPT"]).reshape(3, 4); T.append(M)
    rs = np.array([SCALE_XI_TRANS] * 3 + [SCALE_XI_ROT] * 3 + [SCALE_A, SCALE_B])
    adH, adT = np.zeros((F, F, 8, 8)), np.zeros((F, F, 8, 8))
    for h in range(F):
        for t in range(F):
            M = T[t] @ synth.se3_inv(T[h])
            Rm, tt = M[:3, :3], M[:3, 3]
            Adj = np.zeros((6, 6)); Adj[:3, :3] = Rm; Adj[3:, 3:] = Rm; Adj[:3, 3:] = synth.hat(tt) @ Rm
            AH, AT = np.eye(8), np.eye(8)
            AH[:6, :6] = -Adj.T
            al = float(np.float32(np.exp(SCALE_A * frames[t]["state_zero"][6] - SCALE_A * frames[h]["state_zero"][6]) * float(frames[t]["ab_exposure"]) / float(frames[h]["ab_exposure"])))
            AT[6, 6] = -al; AH[6, 6] = al; AT[7, 7] = -1; AH[7, 7] = al
            adH[h, t], adT[h, t] = rs[:, None] * AH, rs[:, None] * AT
    return adH, adT


def make_inputs(win, precalc, frames=None, calib_value=None, idepth=None, idepth_zero=None, state=None, active=None, lam=1e-1):
    """the inputs of one pass on window `win` as an implementation holds them: its precalc; frames / calibration / inverse depths / residual states where they have
    moved on from the window's (the fused step).  state: state_state of every residual when the pass starts (default: the active set after collectActiveResiduals,
    all IN); active: isActive of the linearised residuals and of residuals the pass does not touch"""
    fr = np.asarray(win.frames if frames is None else frames)
    res = win.residuals
    lin = res["is_linearized"] != 0
    return types.SimpleNamespace(
        F=win.F, P=win.P, R=win.R, w=win.w, h=win.h, precalc=np.asarray(precalc, np.float32), frames=fr, res=res, pts=win.points, lin=lin,
        imgs=np.stack([np.asarray(win.images[f][0], np.float32) for f in range(win.F)]).astype(np.float64), settings=win.settings,
        cv=np.asarray(win.calib["value"] if calib_value is None else calib_value, np.float64), cv0=np.asarray(win.calib["value_zero"], np.float64),
        idp=F32(win.points["idepth"] if idepth is None else idepth), idz=F32(win.points["idepth_zero"] if idepth_zero is None else idepth_zero),
        state=np.where(lin, res["state_state"], 0) if state is None else np.asarray(state), active=res["is_active"] != 0 if active is None else np.asarray(active) != 0,
        lin_J=win.lin_J, lin_rtz=win.lin_res_toZeroF, HM=np.asarray(win.HM, np.float64), bM=np.asarray(win.bM, np.float64), lam=lam)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def reference(inp, impl=None, fault=None, want_system=True):
    with np.errstate(all="ignore"):
        return _reference(inp, impl, fault, want_system)


def _one_residual(inp, r):
    """the inputs of residual r alone (the per-residual part of the reference reads nothing else)"""
    sub = copy.copy(inp)
    sub.R, sub.res, sub.lin, sub.state, sub.active = 1, inp.res[r:r + 1], inp.lin[r:r + 1], inp.state[r:r + 1], inp.active[r:r + 1]
    return sub


def _residual_units(per_res, impl, r):
    """how far the implementation's record of residual r is from a one-residual reference, over everything the implementation reports for it"""
    out = impl["out"][r]
    u_ = _units(out["state_NewEnergyWithOutlier"], per_res["energyWO"].v[0], per_res["energyWO"].s[0])
    if out["state_NewState"] == IN:
        u_ = max(u_, _units(out["JpJdF"], per_res["JpJdF"].v[0], per_res["JpJdF"].s[0]))
    if impl.get("J") is not None:
        for k in DUMP:
            u_ = max(u_, _units(impl["J"][k][r].reshape(per_res[k].shape[1:]), per_res[k].v[0], per_res[k].s[0]))
    return u_


def _reference(inp, impl, fault, want_system, _flips=None):
    """float64 of one linearisation pass and of the system it gives.  impl: dict(out=RES_OUT records [R], J=RAWJAC records of a debug-dump pass or None) of the
    implementation that is held to this reference - its decisions are adopted where a margin is under the guard; None: the reference's own decisions throughout.
    fault: one of FAULTS (sensitivity tests)."""
    F, P, R, s = inp.F, inp.P, inp.R, inp.settings
    res, pts = inp.res, inp.pts
    h, t, p = res["host"].astype(np.int64), res["target"].astype(np.int64), res["point"].astype(np.int64)
    assert float(s["affineOptModeA"]) >= 0 and float(s["affineOptModeB"]) >= 0
    huberTH, othc = float(s["huberTH"]), float(s["outlierTHSumComponent"])
    pc = inp.precalc[h, t].astype(np.float64)
    KRKi, Kt, R0, t0, aff = V(pc[:, 0:9].reshape(R, 3, 3)), V(pc[:, 9:12]), V(pc[:, 12:21].reshape(R, 3, 3)), V(pc[:, 21:24]), V(pc[:, 24:26])
    b0 = pc[:, 26]
    if fault == "b0_current":
        b0 = F32(SCALE_B * inp.frames["state"][:, 7])[h]
    fx, fy, cx, cy = (float(np.float32(x)) for x in (SCALE_F * inp.cv[0], SCALE_F * inp.cv[1], SCALE_C * inp.cv[2], SCALE_C * inp.cv[3]))
    fxi, fyi = float(np.float32(1.0) / np.float32(fx)), float(np.float32(1.0) / np.float32(fy))
    lo, wM3, hM3 = float(np.float32(1.1)), float(inp.w - 3), float(inp.h - 3)
    thF = F32(inp.frames["frameEnergyTH"])
    thMax = np.maximum(thF[h], thF[t])
    u, v = F32(pts["u"])[p], F32(pts["v"])[p]
    idp, idz = inp.idp[p], inp.idz[p]
    if fault == "geo_current_idepth":
        idz = idp
    want = ~inp.lin & (inp.state != OOB)                                  # the residuals this pass linearises

    with np.errstate(all="ignore"):
        # ---- centre at the linearisation point (ResidualProjections.h:57-84) and the geometric Jacobians (Residuals.cc:67-104)
        K0, K1 = (V(u) - cx) * fxi, (V(v) - cy) * fyi
        ptp = [R0[:, i, 0] * K0 + R0[:, i, 1] * K1 + R0[:, i, 2] + t0[:, i] * idz for i in range(3)]
        dres = 1.0 / ptp[2]
        nid, uu, vv = V(idz) * dres, ptp[0] * dres, ptp[1] * dres
        cKu, cKv = uu * fx + cx, vv * fy + cy
        c_margin = np.minimum.reduce([np.abs(cKu.v - lo), np.abs(cKv.v - lo), np.abs(cKu.v - wM3), np.abs(cKv.v - hM3), np.abs(ptp[2].v)])
        c_ok = (dres.v > 0) & (cKu.v > lo) & (cKv.v > lo) & (cKu.v < wM3) & (cKv.v < hM3)
        Jpdd = [dres * (t0[:, 0] - t0[:, 2] * uu) * fx, dres * (t0[:, 1] - t0[:, 2] * vv) * fy]
        dCx2, dCx3 = dres * (R0[:, 2, 0] * uu - R0[:, 0, 0]), dres * (R0[:, 2, 1] * uu - R0[:, 0, 1]) * fx * fyi
        dCy2, dCy3 = dres * (R0[:, 2, 0] * vv - R0[:, 1, 0]) * fy * fxi, dres * (R0[:, 2, 1] * vv - R0[:, 1, 1])
        x10 = vstack([(K0 * dCx2 + uu) * SCALE_F, K1 * dCx3 * SCALE_F, (dCx2 + 1.0) * SCALE_C, dCx3 * SCALE_C,
                      nid * fx, V(np.zeros(R)), -(nid * uu) * fx, -(uu * vv) * fx, (1.0 + uu * uu) * fx, -vv * fx])
        y10 = vstack([K0 * dCy2 * SCALE_F, (K1 * dCy3 + vv) * SCALE_F, dCy2 * SCALE_C, (dCy3 + 1.0) * SCALE_C,
                      V(np.zeros(R)), nid * fy, -(nid * vv) * fy, -(1.0 + vv * vv) * fy, uu * vv * fy, uu * fy])
        # ---- pattern pixels at the current state (ResidualProjections.h:24-33)
        px, py = V(u[:, None] + PAT[None, :, 0]), V(v[:, None] + PAT[None, :, 1])
        q = [KRKi[:, i, 0][:, None] * px + KRKi[:, i, 1][:, None] * py + KRKi[:, i, 2][:, None] + Kt[:, i][:, None] * idp[:, None] for i in range(3)]
        Ku, Kv = q[0] / q[2], q[1] / q[2]
        p_margin = np.nan_to_num(np.minimum.reduce([np.abs(Ku.v - lo), np.abs(Kv.v - lo), np.abs(Ku.v - wM3), np.abs(Kv.v - hM3)]), nan=0.0)
        p_ok = (Ku.v > lo) & (Kv.v > lo) & (Ku.v < wM3) & (Kv.v < hM3)
        c_margin = np.nan_to_num(c_margin, nan=0.0)
        geo_ok = c_ok & p_ok.all(axis=1)
        geo_guard = want & ((c_margin < GUARD_PX) | (p_margin < GUARD_PX).any(axis=1))
        near = (c_ok | (c_margin < GUARD_PX)) & (p_ok | (p_margin < GUARD_PX)).all(axis=1)          # in the image up to the guard: the taps are readable
        oob = want & ~geo_ok
        if impl is not None:
            oob = np.where(geo_guard & near, want & (impl["out"]["state_NewState"] == OOB), oob)
        comp = want & ~oob & near                                                                  # the residuals with photometric terms
        cm = comp[:, None]
        hit = taps(inp.imgs, t, Ku, Kv, cm & np.ones((1, 8), bool))
        assert np.isfinite(hit.v[comp]).all()
        color, wgt = V(F32(pts["color"])[p]), V(F32(pts["weights"])[p])
        r_ = hit[..., 0] - (aff[:, 0][:, None] * color + aff[:, 1][:, None])
        drdA = color - V(b0)[:, None]
        g2 = hit[..., 1] * hit[..., 1] + hit[..., 2] * hit[..., 2]
        w_ = 0.5 * ((othc / (othc + g2)).sqrt() + wgt)
        ar = np.abs(r_.v)
        h_margin = np.where(cm, np.abs(ar / huberTH - 1.0), np.inf)
        inside = ar < huberTH
        if _flips is not None:
            inside = inside ^ _flips
        hw = V(np.ones((R, 8))).where(inside, huberTH / V(ar, r_.s))
        e_k = w_ * w_ * hw * r_ * r_ * (2.0 - hw)
        shw = hw if fault == "no_sqrt_huber" else hw.sqrt().where(hw.v < 1, hw)
        hp = shw * w_
        use = cm & np.ones((1, 8), bool)
        if fault == "drop_pixel7":
            use = use & (np.arange(8) < 7)[None, :]
        z = lambda a: a.where(use)
        gx, gy, rF, ja0, ja1, e_k = z(hit[..., 1] * hp), z(hit[..., 2] * hp), z(r_ * hp), z(drdA * hp), z(hp), z(e_k)
        energy = e_k.sum(1)
        wJI2 = (hp * hp * (gx * gx + gy * gy)).where(use).sum(1)
        JI2 = [(gx * gx).sum(1), (gx * gy).sum(1), (gy * gy).sum(1)]                         # 00, 10, 11
        JabJI = [(ja0 * gx).sum(1), (ja0 * gy).sum(1), (ja1 * gx).sum(1), (ja1 * gy).sum(1)]
        Jab2 = [(ja0 * ja0).sum(1), (ja0 * ja1).sum(1), (ja1 * ja1).sum(1)]
        JIr = [(rF * gx).sum(1), (rF * gy).sum(1)]
        Jabr = [(rF * ja0).sum(1), (rF * ja1).sum(1)]
        rr = (rF * rF).sum(1)
        # ---- the Huber branch of pixels at the threshold: the combination of branches nearest to what the implementation reports for the residual
        h_guard = comp & (h_margin < GUARD_REL).any(axis=1)
        if impl is not None and _flips is None and h_guard.any():
            flips = np.zeros((R, 8), bool)
            for r in np.nonzero(h_guard)[0]:
                ks = np.nonzero(h_margin[r] < GUARD_REL)[0][:6]
                sub = _one_residual(inp, r)
                best, best_u = 0, np.inf
                for m in range(1 << len(ks)):
                    fl = np.zeros((1, 8), bool)
                    fl[0, ks] = [(m >> j) & 1 for j in range(len(ks))]
                    u_ = _residual_units(_reference(sub, None, fault, False, _flips=fl).per_res, impl, r)
                    if u_ < best_u:
                        best, best_u = m, u_
                flips[r, ks] = [(best >> j) & 1 for j in range(len(ks))]
            if flips.any():
                return _reference(inp, impl, fault, want_system, _flips=flips)
        # ---- outlier (Residuals.cc:191-199)
        out_margin = np.where(comp, np.minimum(np.abs(energy.v / thMax - 1.0), np.abs(wJI2.v / 2.0 - 1.0)), np.inf)
        outlier = comp & ((energy.v > thMax) | (wJI2.v < 2))
        o_guard = comp & (out_margin < GUARD_REL)
        if impl is not None:
            outlier = np.where(o_guard, impl["out"]["state_NewState"] == OUTLIER, outlier)
    state = np.where(want, np.where(oob | ~comp, OOB, np.where(outlier, OUTLIER, IN)), inp.state)
    adopted = want & (geo_guard | (comp & (h_guard | o_guard)))
    newE = energy.where(~outlier, V(thMax))
    # takeData (Residuals.h:123-128)
    v0, v1 = JI2[0] * Jpdd[0] + JI2[1] * Jpdd[1], JI2[1] * Jpdd[0] + JI2[2] * Jpdd[1]
    JpJd = vstack([x10[:, 4 + i] * v0 + y10[:, 4 + i] * v1 for i in range(6)] + [JabJI[0] * Jpdd[0] + JabJI[1] * Jpdd[1], JabJI[2] * Jpdd[0] + JabJI[3] * Jpdd[1]])
    per_res = dict(state_NewEnergy=newE, energyWO=energy, JpJdF=JpJd, centerProjectedTo=vstack([cKu, cKv, nid]),
                   resF=rF, JIdx=vstack([gx, gy], 1), JabF=vstack([ja0, ja1], 1), Jpdxi=vstack([x10[:, 4:], y10[:, 4:]], 1), Jpdc=vstack([x10[:, :4], y10[:, :4]], 1),
                   Jpdd=vstack(Jpdd), JIdx2=vstack([JI2[0], JI2[1], JI2[1], JI2[2]]), JabJIdx=vstack(JabJI), Jab2=vstack([Jab2[0], Jab2[1], Jab2[1], Jab2[2]]))
    actA = want & (state == IN)
    actL = inp.lin & inp.active
    ref = types.SimpleNamespace(R=R, P=P, F=F, want=want, state=state, computed=want & (state != OOB), actA=actA, actL=actL, adopted=adopted, n_adopted=int(adopted.sum()),
                                per_res=per_res, margins=dict(geo=np.where(want, np.minimum(c_margin, p_margin.min(axis=1)), np.inf), huber=h_margin, outlier=out_margin),
                                huber_inside=inside & use, huber_used=use)
    if not want_system:
        return ref

    # ---- accumulate (AccumulatedTopHessian.cc:8-118): the active set in mode 0, the linearised residuals in mode 1
    accA = actA.copy()
    if fault == "drop_residual":
        cnt = np.bincount(p[actA], minlength=P)
        cand = np.nonzero(cnt >= min(2, cnt.max()))[0]
        accA[np.nonzero(actA & (p == cand[len(cand) // 2]))[0][0]] = False
    adH, adT = adjoints(inp.frames)
    if fault == "swap_adjoint":
        hh, tt_ = (1, 0) if F > 2 else (0, 1)
        adH, adT = adH.copy(), adT.copy()
        adH[hh, tt_], adT[hh, tt_] = adT[hh, tt_].copy(), adH[hh, tt_].copy()
    n = 8 * F + 4

    def blocks(x, y, ji2, jabji, jab2, jir, jabr, rr_):
        """the 13 x 13 of AccumulatorApprox::update / updateTopRight / updateBotRight per residual -> V [R, 13, 13]"""
        a, b, c = ji2
        xx, yy, xy = veinsum("ri,rj->rij", x, x), veinsum("ri,rj->rij", y, y), veinsum("ri,rj->rij", x, y)
        xy = xy + V(np.swapaxes(xy.v, 1, 2), np.swapaxes(xy.s, 1, 2))
        e3 = lambda q_: q_[:, None, None]
        H10 = e3(a) * xx + e3(c) * yy + e3(b) * xy
        e2 = lambda q_: q_[:, None]
        TR = vstack([x * e2(jabji[0]) + y * e2(jabji[1]), x * e2(jabji[2]) + y * e2(jabji[3]), x * e2(jir[0]) + y * e2(jir[1])], 2)
        BR = vstack([vstack([jab2[0], jab2[1], jabr[0]]), vstack([jab2[1], jab2[2], jabr[1]]), vstack([jabr[0], jabr[1], rr_])], 1)
        top = V(np.concatenate([H10.v, TR.v], 2), np.concatenate([H10.s, TR.s], 2))
        bot = V(np.concatenate([np.swapaxes(TR.v, 1, 2), BR.v], 2), np.concatenate([np.swapaxes(TR.s, 1, 2), BR.s], 2))
        return V(np.concatenate([top.v, bot.v], 1), np.concatenate([top.s, bot.s], 1))

    def lift(adh, adt):
        """[F, F, n + 1, 13]: rows of [calib | frames | b] from the columns of a pair's 13 x 13"""
        L = np.zeros((F, F, n + 1, 13))
        for a in range(F):
            for b in range(F):
                L[a, b, 0:4, 0:4] = np.eye(4)
                L[a, b, 4 + 8 * a:12 + 8 * a, 4:12] += adh[a, b]
                L[a, b, 4 + 8 * b:12 + 8 * b, 4:12] += adt[a, b]
                L[a, b, n, 12] = 1.0
        return L.reshape(F * F, n + 1, 13)

    Lm = lift(adH, adT)
    pair = h * F + t

    def stitch(B, mask):
        acc = seg_sum(B, pair, F * F, mask)
        aL = np.abs(Lm)
        return V(np.einsum("qia,qab,qjb->ij", Lm, acc.v, Lm, optimize=True), np.einsum("qia,qab,qjb->ij", aL, acc.s, aL, optimize=True))

    def point_sums(ji2, jir, jpdd, x4, y4, mask):
        a0, a1 = ji2[0] * jpdd[0] + ji2[1] * jpdd[1], ji2[1] * jpdd[0] + ji2[2] * jpdd[1]
        bd, Hdd = jir[0] * jpdd[0] + jir[1] * jpdd[1], a0 * jpdd[0] + a1 * jpdd[1]
        Hcd = x4 * a0[:, None] + y4[:, :] * a1[:, None]
        return seg_sum(Hdd, p, P, mask), seg_sum(bd, p, P, mask), seg_sum(Hcd, p, P, mask)

    HddA, bdA, HcdA = point_sums(JI2, JIr, Jpdd, x10[:, :4], y10[:, :4], accA)
    topA = stitch(blocks(x10, y10, JI2, JabJI, Jab2, JIr, Jabr, rr), accA)
    sysd = dict(HA=topA[:n, :n], bA=topA[:n, n])
    zP = V(np.zeros(P))
    HddL, bdL, HcdL = zP, zP, V(np.zeros((P, 4)))
    jp_all = JpJd.where(actA[:, None])
    cDelta = F32(inp.cv - inp.cv0)
    dstate = np.asarray(inp.frames["state"], np.float64)[:, :8] - np.asarray(inp.frames["state_zero"], np.float64)[:, :8]
    topL = V(np.zeros((n + 1, n + 1)))
    if actL.any():
        J = inp.lin_J
        g = lambda k: V(F32(J[k]))
        lx, ly = vcat([g("Jpdc")[:, 0], g("Jpdxi")[:, 0]], 1), vcat([g("Jpdc")[:, 1], g("Jpdxi")[:, 1]], 1)
        dp = veinsum("rk,rkc->rc", V(F32(dstate)[h]), V(F32(adH[h, t]))) + veinsum("rk,rkc->rc", V(F32(dstate)[t]), V(F32(adT[h, t])))          # setDeltaF (:403-429)
        dd = V(inp.idp[p]) - V(inp.idz[p])
        jpd = [g("Jpdd")[:, 0], g("Jpdd")[:, 1]]
        Jpx = (lx[:, 4:] * dp[:, :6]).sum(1) + (lx[:, :4] * V(cDelta)[None, :]).sum(1) + jpd[0] * dd
        Jpy = (ly[:, 4:] * dp[:, :6]).sum(1) + (ly[:, :4] * V(cDelta)[None, :]).sum(1) + jpd[1] * dd
        lgx, lgy, la0, la1 = g("JIdx")[:, 0], g("JIdx")[:, 1], g("JabF")[:, 0], g("JabF")[:, 1]
        ra = V(F32(inp.lin_rtz)) + lgx * Jpx[:, None] + lgy * Jpy[:, None] + la0 * dp[:, 6][:, None] + la1 * dp[:, 7][:, None]          # resApprox (AccumulatedTopHessian.cc:44-63)
        lji2 = [g("JIdx2")[:, 0], g("JIdx2")[:, 1], g("JIdx2")[:, 3]]
        ljabji = [g("JabJIdx")[:, i] for i in range(4)]
        ljab2 = [g("Jab2")[:, 0], g("Jab2")[:, 1], g("Jab2")[:, 3]]
        ljir, ljabr, lrr = [(ra * lgx).sum(1), (ra * lgy).sum(1)], [(ra * la0).sum(1), (ra * la1).sum(1)], (ra * ra).sum(1)
        HddL, bdL, HcdL = point_sums(lji2, ljir, jpd, lx[:, :4], ly[:, :4], actL)
        topL = stitch(blocks(lx, ly, lji2, ljabji, ljab2, ljir, ljabr, lrr), actL)
        lv0, lv1 = lji2[0] * jpd[0] + lji2[1] * jpd[1], lji2[1] * jpd[0] + lji2[2] * jpd[1]
        ljp = vstack([lx[:, 4 + i] * lv0 + ly[:, 4 + i] * lv1 for i in range(6)] + [ljabji[0] * jpd[0] + ljabji[1] * jpd[1], ljabji[2] * jpd[0] + ljabji[3] * jpd[1]])
        jp_all = jp_all.where(~actL[:, None], ljp)
    # priors (top_add_prior): exact doubles; their float64 rounding in units of eps32 is their share of S
    prior = np.concatenate([np.full(4, float(s["initialCalibHessian"])), np.asarray(inp.frames["prior"], np.float64).reshape(-1)])
    dprior = np.concatenate([cDelta, np.asarray(inp.frames["state"], np.float64)[:, :8].reshape(-1)])
    HLv, HLs = topL.v[:n, :n].copy(), topL.s[:n, :n].copy()
    HLv[np.arange(n), np.arange(n)] += prior; HLs[np.arange(n), np.arange(n)] += prior * 2.0 ** -29
    sysd["HL"], sysd["bL"] = V(HLv, HLs), V(topL.v[:n, n] + prior * dprior, topL.s[:n, n] + np.abs(prior * dprior) * 2.0 ** -29)
    # ---- per point and Schur complement (AccumulatedSCHessian.cc:9-51 and the stitch)
    if fault == "hcd_neighbour":
        withres = np.nonzero(np.bincount(p[actA], minlength=P)[:-1] > 0)[0]
        i = int(withres[len(withres) // 3])
        HcdA = V(HcdA.v.copy(), HcdA.s.copy()); HcdA.v[i + 1], HcdA.s[i + 1] = HcdA.v[i], HcdA.s[i]
    act_all = accA | actL
    ngood = np.bincount(p[act_all], minlength=P)
    has = ngood > 0
    priorF = V(F32(pts["priorF"]))
    Hs = HddA + HddL + priorF
    Hs = Hs.where(Hs.v >= 1e-10, V(np.full(P, 1e-10)))
    with np.errstate(all="ignore"):
        Hdi = (1.0 / Hs).where(has)
    bdS = (bdA + bdL + priorF * (V(inp.idp) - V(inp.idz))).where(has)
    Hcd = HcdA + HcdL
    G = V(np.zeros((P, n)), np.zeros((P, n)))
    G.v[:, :4], G.s[:, :4] = Hcd.v, Hcd.s
    cols = np.arange(8)[None, :]
    ra_ = np.nonzero(act_all)[0]
    for ad, fr_ in ((adH, h), (adT, t)):
        c_ = veinsum("rij,rj->ri", V(ad[h, t][ra_]), jp_all[ra_])
        np.add.at(G.v, (p[ra_][:, None], 4 + 8 * fr_[ra_][:, None] + cols), c_.v)
        np.add.at(G.s, (p[ra_][:, None], 4 + 8 * fr_[ra_][:, None] + cols), c_.s)
    G = G.where(has[:, None])
    Wg = G * Hdi[:, None]
    sysd["Hsc"], sysd["bsc"] = veinsum("pi,pj->ij", Wg, G), veinsum("pi,p->i", Wg, bdS)
    pp = dict(Hdd_accAF=HddA, bd_accAF=bdA, Hcd_accAF=HcdA, Hdd_accLF=HddL, bd_accLF=bdL, Hcd_accLF=HcdL, HdiF=Hdi, bdSumF=bdS, idepth_hessian=Hs.where(has))
    # ---- HFinal | bFinal (EnergyFunctional.cc:240-291, the branch without LDSO_SOLVER_ORTHOGONALIZE_SYSTEM)
    sm = int(s["solverMode"])
    assert not sm & 2
    lam = 0.0 if sm & 64 else inp.lam
    lam = 1e-5 if sm & 128 else lam
    l1, il = 1.0 + lam, 1.0 / (1.0 + lam)
    delta = np.concatenate([np.asarray(cDelta, np.float64), dstate.reshape(-1)])
    dscale = np.where(np.eye(n, dtype=bool), l1, 1.0)
    Ht = sysd["HA"] + sysd["HL"] + V(inp.HM, np.abs(inp.HM) * 2.0 ** -29)
    bM = inp.bM + inp.HM @ delta
    sysd["HFinal"] = V(Ht.v * dscale - sysd["Hsc"].v * il, Ht.s * dscale + sysd["Hsc"].s * il)
    sysd["bFinal"] = sysd["bA"] + sysd["bL"] + V(bM, np.abs(bM) * 2.0 ** -29) - sysd["bsc"]
    ref.per_point, ref.system, ref.has_L, ref.ngood = pp, sysd, bool(actL.any()), ngood
    return ref


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# measuring an implementation
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def measure(got, ref, point_solve=True):
    """-> the error of `got` per quantity in units of eps32 * S, after asserting what is exact: state_NewState of the whole active set.
    got: dict with out (RES_OUT records), and optionally J (RAWJAC records of a debug-dump pass), pts (POINT_OUT records; point_solve: HdiF / bdSumF / idepth_hessian
    are those of a solve on this linearisation), sys (HA, bA, Hsc, bsc, HL, bL as get_system returns them), final ((H [n, n] of which the lower triangle counts, b [n]))"""
    out = got["out"]
    w = ref.want
    bad = np.nonzero(w & (out["state_NewState"] != ref.state))[0]
    assert len(bad) == 0, ("state_NewState differs from the reference outside the guards at residuals", bad[:8], out["state_NewState"][bad[:8]], ref.state[bad[:8]],
                           {k: m[bad[:8]] for k, m in ref.margins.items() if m.ndim == 1})
    un = {}
    c, a = ref.computed, ref.actA
    U = lambda g, q, m=slice(None): _units(np.asarray(g)[m], q.v[m], q.s[m])
    un["state_NewEnergy"] = max(U(out["state_NewEnergy"], ref.per_res["state_NewEnergy"], c), U(out["state_NewEnergyWithOutlier"], ref.per_res["energyWO"], c))
    un["centerProjectedTo"] = U(out["centerProjectedTo"], ref.per_res["centerProjectedTo"], c)
    un["JpJdF"] = U(out["JpJdF"], ref.per_res["JpJdF"], a)
    if got.get("J") is not None:
        for k in DUMP:
            un[k] = U(got["J"][k].reshape(ref.per_res[k].shape), ref.per_res[k], c)
    if got.get("pts") is not None:
        names = PER_POINT_ACC + (PER_POINT_SOLVE if point_solve else ()) + (PER_POINT_L if ref.has_L else ())
        for k in names:
            un[k] = U(got["pts"][k], ref.per_point[k])
    if got.get("sys") is not None:
        for k in SYSTEM + (SYSTEM_L if ref.has_L else ()):
            assert np.isfinite(got["sys"][k]).all(), k
            un[k] = U(got["sys"][k], ref.system[k])
    if got.get("final") is not None:
        Hf, bf = got["final"]
        n = len(bf)
        lo = np.tril(np.ones((n, n), bool))
        assert np.isfinite(Hf[lo]).all() and np.isfinite(bf).all()
        un["HFinal"] = _units(np.asarray(Hf)[lo], ref.system["HFinal"].v[lo], ref.system["HFinal"].s[lo])
        un["bFinal"] = U(bf, ref.system["bFinal"])
    return un


def check(got, ref, label="", point_solve=True):
    """THE assertion of the linearisation stage tests: every entry within max(FLOOR_UNITS, ORACLE_FACTOR x yardstick) x eps32 x S of the float64 value, every decision
    outside the guards equal, at most ADOPT_CAP of the residuals under a guard.  -> the measured units"""
    un = measure(got, ref, point_solve)
    bd = bounds()
    print(label, "units", {q: round(un[q], 2) for q in un}, "adopted", ref.n_adopted, "of", int(ref.want.sum()))
    assert ref.n_adopted <= ADOPT_CAP * max(int(ref.want.sum()), 1), (label, "adoptions", ref.n_adopted, int(ref.want.sum()))
    over = {q: (un[q], bd[q]) for q in un if not un[q] <= bd[q]}
    assert not over, (label, over)
    return un


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _rebuild(win, keep_point, keep_res):
    """the window with the points keep_point [P] and, of their residuals, keep_res [R]"""
    w2 = copy.copy(win)
    new_idx = np.cumsum(keep_point) - 1
    kr = keep_res & keep_point[win.residuals["point"]]
    res = win.residuals[kr].copy()
    res["point"] = new_idx[res["point"]]
    pts = win.points[keep_point].copy()
    cnt = np.bincount(res["point"], minlength=len(pts))
    pts["res_count"] = cnt
    pts["res_begin"] = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    w2.points, w2.residuals = pts, res
    return w2


# name -> F, P, seed, chunk points (0: the handle's default), what the chunk sizes must show, variant
CASES = {
    "F5_default": (5, 63, 11, 0, lambda z: z.max() == 4 and z.min() < 4, None),
    "F5_chunk12": (5, 67, 12, 12, lambda z: ((z >= 9) & (z <= 16)).any() and (z == 1).any(), None),                 # hosts of 14 | 13 points: chunks 12 + 2, 12 + 1
    "F5_chunk20": (5, 107, 13, 20, lambda z: ((z >= 17) & (z <= 24)).any() and (z == 1).any(), None),               # hosts of 22 | 21 points: 20 + 2, 20 + 1
    "F5_chunk36": (5, 187, 14, 36, lambda z: (z > 32).any() and (z == 1).any(), None),                              # hosts of 38 | 37 points: 36 + 2, 36 + 1
    "F2": (2, 37, 15, 0, lambda z: z.max() <= 4, None),
    "F3": (3, 41, 24, 0, lambda z: z.max() <= 4, None),
    "F8": (8, 85, 16, 0, lambda z: z.max() <= 4, None),
    "F9_pair": (9, 85, 17, 0, lambda z: (z % 2 == 1).any() and (z == 1).any(), None),                                 # hosts of 10 | 9 points: 4 + 4 + 2, 4 + 4 + 1
    "F12_pair": (12, 127, 18, 0, lambda z: (z == 3).any() and (z == 1).any(), "odd_hosts"),
    "F13": (13, 101, 19, 0, lambda z: z.max() <= 4, None),
    "F16": (16, 97, 20, 0, lambda z: z.max() <= 4, None),
    "F6_empty_host": (6, 71, 21, 0, lambda z: z.max() <= 4, "empty_host"),
    "F5_residual_counts": (5, 61, 22, 0, lambda z: z.max() <= 4, "residual_counts"),
    "F5_mixed": (5, 83, 23, 0, lambda z: z.max() <= 4, "mixed"),
}


@functools.lru_cache(maxsize=None)
def case_window(name):
    F, P, seed, _, _, variant = CASES[name]
    win = synth.make_window(F=F, P=P, w=256, h=192, fx=160.0, seed=seed)
    rng = np.random.default_rng(seed)
    keep_p, keep_r = np.ones(win.P, bool), np.ones(win.R, bool)
    if variant == "empty_host":                                           # a host frame without points in the middle of the window
        keep_p = win.points["host"] != 3
    if variant == "odd_hosts":                                            # 11 | 10 points per host -> 11 | 7: chunks of 4 + 4 + 3 and 4 + 3 ... and one host of 9: 4 + 4 + 1
        host = win.points["host"]
        for hh in range(F):
            idx = np.nonzero(host == hh)[0]
            keep_p[idx[(11 if hh % 2 == 0 else 7) if hh != 5 else 9:]] = False
    if variant == "residual_counts":                                      # a point without residuals, points observed in one frame, the rest in every other frame
        first = win.points["res_begin"]
        for i in range(0, win.P, 5):
            keep_r[first[i]:first[i] + win.points["res_count"][i]] = False
            if i % 10 == 0:
                keep_r[first[i] + int(rng.integers(0, F - 1))] = True
    if not (keep_p.all() and keep_r.all()):
        win = _rebuild(win, keep_p, keep_r)
    else:
        win = copy.copy(win)
        win.points = win.points.copy()
    if variant == "mixed":
        from oracle import pyoracle as po
        win = po.make_mixed_window(win)
    else:                                                                  # idepth != idepth_zero: the geometric Jacobians stay at the linearisation point
        win.points["idepth"] = (win.points["idepth"] * (1 + rng.normal(0, 2e-3, win.P))).astype(np.float32)
    return win


def chunk_sizes(cuts):
    return np.diff(np.concatenate([[0], np.asarray(cuts)]))


def got_of(out, J=None, pts=None, sys=None, final=None):
    return dict(out=out, J=J, pts=pts, sys=sys, final=final)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the oracle's plain pass and solveSystemF(0) on the case -> its inputs and what it computed"""
    from oracle import pyoracle as po
    win = case_window(name)
    o = po.OracleWindow(win)
    inp = make_inputs(win, o.get_precalc())
    o.collect_active()
    o.linearize_all(False)
    r = o.get_residuals()
    o.apply_res()
    r["out"]["JpJdF"] = o.get_residuals(False)["out"]["JpJdF"]          # takeData happens in applyRes
    o.backup_state(); o.solve_system(0)
    sysd = o.get_system()
    pts, _ = o.get_points()
    o.close()
    got = got_of(r["out"], r["J"], pts, sysd, (sysd["HFinal"], sysd["bFinal"]))
    return inp, got


@functools.lru_cache(maxsize=None)
def oracle_reference(name, fault=None):
    inp, got = oracle_run(name)
    return reference(inp, got, fault)
