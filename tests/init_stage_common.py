"""What tests/test_init_stage_cpu.py and tests/test_init_stage_gpu.py share: a float64 reference of one evaluation of the monocular initialiser (calcResAndGS
:181-405, calcEC :412-428, doStep :645-671, applyStep :673-687 and the per-point part of resetPoints :625-626 of CoarseInitializer.cc, as k_ini_eval and the
INI_STAGE part of k_ini_ctl restate them), its own error scale, the cases, and the assertion both files make.

The reference takes the float32 inputs and computes everything from them in float64, vectorised over points x 8 pattern pixels.  For every sum it returns the
value and S = the sum of the absolute values of the addends; a float32 implementation is measured in UNITS of eps32 * S (eps32 = 2^-24) per entry, so a small
entry is held to its own size and not to that of the largest one.  Decisions (in the image, new_idepth > 0, outlier, alpha branch) are kept away from their
thresholds by the case builder: a point whose margin is under the guard is given isGood = 0, so two correct float32 implementations cannot disagree on one."""
import functools
import types

import numpy as np

from ldso_amd import synth

EPS32 = 2.0 ** -24
PATTERN = np.array([[0, -2], [-1, -1], [1, -1], [-2, 0], [0, 0], [2, 0], [-1, 1], [0, 2]], np.float64)          # Setting.cc:221
ALPHA_K, ALPHA_W = 2.5 * 2.5, 150.0 * 150.0
GUARD_PX, GUARD_REL = 1e-2, 1e-3
W0, H0, LEVELS, FX = 192, 144, 2, 120.0
HUBER = 9.0
FLOOR_UNITS, ORACLE_FACTOR = 16.0, 4.0
SUMS = ("H", "b", "Hsc", "bsc", "E", "ec0", "ec1")
PER_POINT = ("energy_new", "lastHessian_new", "maxstep", "Jb")
QUANTITIES = SUMS + PER_POINT


def level_calib(K4, lvl):
    """-> (fx, fy, cx, cy) as the float32 the kernels multiply with, K^-1 in double (makeK :689-715)"""
    fx, fy, cx, cy = (float(np.float32(x)) for x in K4)
    if lvl > 0:
        fx, fy, cx, cy = fx * 0.5 ** lvl, fy * 0.5 ** lvl, (cx + 0.5) / (1 << lvl) - 0.5, (cy + 0.5) / (1 << lvl) - 0.5
    Ki = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1.0]])
    return tuple(float(np.float32(x)) for x in (fx, fy, cx, cy)), Ki


def _taps(img, x, y, ok):
    """bilinear taps of img [h, w, c] (float32) in float64 at (x, y) where ok; elsewhere the value of pixel (1, 1) (not used).  -> the taps and their error
    scale: the weighted sum of the four |values|, plus what a relative error of the position moves the tap by, (|x| + |y|) * (largest - smallest of the four)"""
    x, y = np.where(ok, x, 1.0), np.where(ok, y, 1.0)
    ix, iy = x.astype(np.int64), y.astype(np.int64)
    dx, dy = (x - ix)[..., None], (y - iy)[..., None]
    I = img.astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = [I[iy + 1, ix + 1], I[iy + 1, ix], I[iy, ix + 1], I[iy, ix]]
        wt = [dx * dy, dy - dx * dy, dx - dx * dy, 1 - dx - dy + dx * dy]
        val = wt[0] * c[0] + wt[1] * c[1] + wt[2] * c[2] + wt[3] * c[3]
        scale = sum(wq * np.abs(cq) for wq, cq in zip(wt, c)) + (np.abs(x) + np.abs(y))[..., None] * (np.maximum.reduce(c) - np.minimum.reduce(c))
        return val, scale


def alpha_branch(T, n):
    """-> alphaOpt, alphaEnergy (res[1]) as float32 arithmetic decides them (:353-361), and the relative distance of |t|^2 from alphaK / alphaW"""
    tsq = float(T[:3, 3] @ T[:3, 3])
    alphaEnergy = np.float32(ALPHA_W * (0.0 + tsq * n))
    cap = np.float32(ALPHA_K) * np.float32(n)
    margin = abs(tsq * ALPHA_W / ALPHA_K - 1.0)
    return (0.0, float(cap), margin) if alphaEnergy > cap else (ALPHA_W, float(alphaEnergy), margin)


def stage_ref(K4, lvl, first, cur, pts, T, a, b, snapped, huberTH=HUBER, fault=None):
    """float64 calcResAndGS + calcEC of the points `pts` (records; idepth_new, idepth, iR, isGood, energy, outlierTH are read) of level lvl at pose T [3 or 4, 4]
    and affine (a, b).  first / cur: the level's images [h, w, 3] (I, dx, dy) of the first and of the new frame.
    fault: a deliberately wrong variant (sensitivity tests): ("drop_points", indices), "drop_pixel7", "swap_alpha", "no_sqrt_huber", "sc_diag"."""
    T = np.asarray(T, np.float64)
    (fx, fy, cx, cy), Ki = level_calib(K4, lvl)
    h, w = cur.shape[:2]
    n = len(pts)
    RKi = (T[:3, :3] @ Ki).astype(np.float32).astype(np.float64)
    t = T[:3, 3].astype(np.float32).astype(np.float64)
    affA, affB = np.exp(float(np.float32(a))), float(np.float32(b))
    u, v, idn = (pts[f].astype(np.float64) for f in ("u", "v", "idepth_new"))
    idp, iR, oTH = (pts[f].astype(np.float64) for f in ("idepth", "iR", "outlierTH"))
    good = pts["isGood"] != 0
    e_old = pts["energy"].astype(np.float64)
    px, py = u[:, None] + PATTERN[:, 0], v[:, None] + PATTERN[:, 1]
    with np.errstate(all="ignore"):
        pt = [RKi[r, 0] * px + RKi[r, 1] * py + RKi[r, 2] + t[r] * idn[:, None] for r in range(3)]
        uu, vv = pt[0] / pt[2], pt[1] / pt[2]
        Ku, Kv = fx * uu + cx, fy * vv + cy
        new_id = idn[:, None] / pt[2]
        inb = (Ku > 1) & (Kv > 1) & (Ku < w - 2) & (Kv < h - 2) & (new_id > 0)
        hit, hit_a = _taps(cur, Ku, Kv, inb)
        rlR, rlR_a = (x[..., 0] for x in _taps(first, px, py, np.ones_like(inb)))
        okpix = inb & np.isfinite(rlR) & np.isfinite(hit[..., 0])
        first_bad = np.where(okpix.all(axis=1), 8, np.argmin(okpix, axis=1))
        hit = np.where(okpix[..., None], hit, 0.0); rlR = np.where(okpix, rlR, 0.0)
        hit_a = np.where(okpix[..., None], hit_a, 0.0); rlR_a = np.where(okpix, rlR_a, 0.0)
        uu, vv, new_id, pz = (np.where(okpix, x, 1.0) for x in (uu, vv, new_id, pt[2]))
        res = hit[..., 0] - affA * rlR - affB
        hw = np.where(np.abs(res) < huberTH, 1.0, huberTH / np.maximum(np.abs(res), 1e-300))
        e = hw * res * res * (2 - hw)
        dxdd, dydd = (t[0] - t[2] * uu) / pz, (t[1] - t[2] * vv) / pz
        dxdd_a, dydd_a = (abs(t[0]) + np.abs(t[2] * uu)) / np.abs(pz), (abs(t[1]) + np.abs(t[2] * vv)) / np.abs(pz)
        hwj = hw if fault == "no_sqrt_huber" else np.sqrt(hw)
        dxI, dyI = hwj * hit[..., 1] * fx, hwj * hit[..., 2] * fy
        J = np.stack([new_id * dxI, new_id * dyI, -new_id * (uu * dxI + vv * dyI), -uu * vv * dxI - (1 + vv * vv) * dyI,
                      (1 + uu * uu) * dxI + uu * vv * dyI, -vv * dxI + uu * dyI, -hwj * affA * rlR, -hwj * np.ones_like(rlR), hwj * res], axis=-1)      # [n, 8, 9]
        auu, avv = np.abs(uu), np.abs(vv)

        def scales(adx, ady, R_a, arl):
            """|addends| of the Jacobian rows, of dd and of the energy, from the sizes of the image terms"""
            J_a = np.stack([new_id * adx, new_id * ady, new_id * (auu * adx + avv * ady), auu * avv * adx + (1 + vv * vv) * ady,
                            (1 + uu * uu) * adx + auu * avv * ady, avv * adx + auu * ady, hwj * affA * arl, hwj * np.ones_like(arl), hwj * R_a], axis=-1)
            return J_a, adx * dxdd_a + ady * dydd_a, e + 2 * hw * np.abs(res) * R_a

        # for the sums: the sizes of the values themselves (the addends of a sum over many points; their own rounding errors average out)
        J_a, dd_a, e_a = scales(np.abs(dxI), np.abs(dyI), np.abs(hit[..., 0]) + np.abs(affA * rlR) + abs(affB), np.abs(rlR))
        # for the quantities of ONE point: the sizes of what the taps are made of, where a gradient tap near zero has the error of its four addends
        J_t, dd_t, e_t = scales(hwj * hit_a[..., 1] * fx, hwj * hit_a[..., 2] * fy, hit_a[..., 0] + affA * rlR_a + abs(affB), rlR_a)
        dd = dxI * dxdd + dyI * dydd
        n2, n2_a = (dxdd * fx) ** 2 + (dydd * fy) ** 2, (dxdd_a * fx) ** 2 + (dydd_a * fy) ** 2
        ms = 1.0 / np.sqrt(n2)                                                  # +inf at t = 0
        ms_scale = np.where(n2 > 0, ms * n2_a / np.where(n2 > 0, n2, 1.0), 0.0)  # first-order error scale of 1 / sqrt(nx^2 + ny^2) under cancellation in nx, ny
    kk = np.arange(8)[None, :]
    use = kk < first_bad[:, None]                                               # the pixels the reference has visited when it breaks (:245-259)
    if fault == "drop_pixel7":
        use = use & (kk < 7)
    ms_m = np.where(use & good[:, None], ms, 1e10)
    maxstep = ms_m.min(axis=1)
    maxstep_scale = np.take_along_axis(np.where(use & good[:, None], ms_scale, 0.0), ms_m.argmin(axis=1)[:, None], 1)[:, 0]
    J, J_a, J_t = (np.where(use[..., None], x, 0.0) for x in (J, J_a, J_t))
    dd, dd_a, dd_t, e, e_a, e_t = (np.where(use, x, 0.0) for x in (dd, dd_a, dd_t, e, e_a, e_t))
    energy, energy_a, energy_t = e.sum(axis=1), e_a.sum(axis=1), e_t.sum(axis=1)
    full = good & (first_bad == 8)
    outlier = full & (energy > oTH * 20)
    gn = full & ~outlier
    if isinstance(fault, tuple) and fault[0] == "drop_points":
        drop = np.zeros(n, bool); drop[list(fault[1])] = True
    else:
        drop = np.zeros(n, bool)
    acc = gn & ~drop                                                            # the points whose addends reach the sums
    alphaOpt, alphaEnergy, alpha_margin = alpha_branch(T, n)
    if fault == "swap_alpha":
        alphaOpt = ALPHA_W - alphaOpt
    Jb = np.einsum("nkq,nk->nq", J, dd)
    Jb_a = np.einsum("nkq,nk->nq", J_a, dd_a)
    Jb_t = np.einsum("nkq,nk->nq", J_t, dd_t)
    lastH, lastH_t = (dd * dd).sum(axis=1), (dd_t * dd_t).sum(axis=1)
    j8 = alphaOpt * (idn - 1) + ((idn - iR) if alphaOpt == 0 else 0.0)
    j8_a = np.abs(alphaOpt * (idn - 1)) + (np.abs(idn - iR) if alphaOpt == 0 else 0.0)
    Jb[:, 8] += j8; Jb_a[:, 8] += j8_a; Jb_t[:, 8] += j8_a
    wgt = 1.0 / (1.0 + lastH + alphaOpt + (1.0 if alphaOpt == 0 else 0.0))
    Jb10 = np.concatenate([Jb, wgt[:, None]], axis=1)
    Jb10_t = np.concatenate([Jb_t, (wgt * (1 + wgt * lastH_t))[:, None]], axis=1)          # d(1 / (1 + x)) = w^2 dx
    A = acc[:, None, None]
    H9 = np.where(A, np.einsum("nkr,nkc->nrc", J, J), 0.0).sum(axis=0)
    H9_a = np.where(A, np.einsum("nkr,nkc->nrc", J_a, J_a), 0.0).sum(axis=0)
    S9 = np.where(A, Jb[:, :, None] * Jb[:, None, :] * wgt[:, None, None], 0.0).sum(axis=0)
    S9_a = np.where(A, Jb_a[:, :, None] * Jb_a[:, None, :] * wgt[:, None, None], 0.0).sum(axis=0)
    if fault == "sc_diag":
        S9[np.arange(9), np.arange(9)] = np.where(acc[:, None], Jb * wgt[:, None], 0.0).sum(axis=0)
    Hm, Hm_a, bm, bm_a = H9[:8, :8].copy(), H9_a[:8, :8].copy(), H9[:8, 8].copy(), H9_a[:8, 8].copy()
    alpha_H = alphaOpt * n
    alpha_b = synth.se3_log(np.vstack([T[:3], [0, 0, 0, 1.0]]))[:3].astype(np.float32).astype(np.float64) * alphaOpt * n
    for q in range(3):
        Hm[q, q] += alpha_H; Hm_a[q, q] += abs(alpha_H); bm[q] += alpha_b[q]; bm_a[q] += abs(alpha_b[q])
    e_terms = np.where(acc, energy, np.where(drop, 0.0, e_old[:, 0]))
    ro2, rn2 = np.where(acc, (idp - iR) ** 2, 0.0), np.where(acc, (idn - iR) ** 2, 0.0)
    sums = {"H": (Hm, Hm_a), "b": (bm, bm_a), "Hsc": (S9[:8, :8], S9_a[:8, :8]), "bsc": (S9[:8, 8], S9_a[:8, 8]), "E": (e_terms.sum(), np.where(acc, energy_a, np.abs(e_terms)).sum()),
            "ec0": (ro2.sum() if snapped else 0.0, ro2.sum() if snapped else 0.0), "ec1": (rn2.sum() if snapped else 0.0, rn2.sum() if snapped else 0.0)}
    energy_new = np.where(gn[:, None], np.stack([energy, (idn - 1) ** 2], axis=1), e_old)
    with np.errstate(all="ignore"):
        m_px = np.minimum.reduce([np.abs(Ku - 1), np.abs(Kv - 1), np.abs(Ku - (w - 2)), np.abs(Kv - (h - 2))])
        margins = types.SimpleNamespace(px=np.nan_to_num(m_px, nan=0.0).min(axis=1), depth=np.nan_to_num(np.abs(pt[2]), nan=0.0).min(axis=1),
                                        energy=np.where(full, np.abs(energy / (20 * oTH) - 1), np.inf), alpha=alpha_margin,
                                        frac=np.minimum.reduce([Ku - np.floor(Ku), np.ceil(Ku) - Ku, Kv - np.floor(Kv), np.ceil(Kv) - Kv]), Ku=Ku, Kv=Kv)
    return types.SimpleNamespace(
        n=n, sums=sums, res1=alphaEnergy, res2=float(2 * n), ec2=float(acc.sum()) if snapped else float(n), isGood_new=gn, outlier=outlier, first_bad=first_bad,
        energy_new=energy_new, energy_scale=np.stack([energy_t, (idn - 1) ** 2], axis=1), lastHessian_new=lastH, lastHessian_scale=lastH_t, maxstep=maxstep, maxstep_scale=maxstep_scale,
        Jb=Jb10, Jb_scale=Jb10_t, alphaOpt=alphaOpt, alpha_H=alpha_H, alpha_b=alpha_b, margins=margins, residual=np.where(use & gn[:, None], res, np.nan),
        new_idepth_nonpositive=good & (np.where(np.isnan(pt[2]), 1.0, pt[2]) <= 0).any(axis=1), t_is_zero=not t.any())


def as_got(ref, drop_maxstep_inf=False):
    """a reference (or a wrong variant of it) in the form an implementation returns: float32 sums, records, Jb"""
    pts = np.zeros(ref.n, synth.INIT_POINT_DTYPE)
    pts["isGood_new"] = ref.isGood_new
    pts["energy_new"] = ref.energy_new
    pts["lastHessian_new"] = ref.lastHessian_new
    with np.errstate(over="ignore"):
        pts["maxstep"] = ref.maxstep
    f = np.float32
    return dict(H=ref.sums["H"][0].astype(f), b=ref.sums["b"][0].astype(f), Hsc=ref.sums["Hsc"][0].astype(f), bsc=ref.sums["bsc"][0].astype(f),
                res=np.array([ref.sums["E"][0], ref.res1, ref.res2], f), ec=np.array([ref.sums["ec0"][0], ref.sums["ec1"][0], ref.ec2], f), pts=pts, jb=ref.Jb.astype(f))


def _units(got, val, scale):
    got, val, scale = np.asarray(got, np.float64), np.asarray(val, np.float64), np.asarray(scale, np.float64)
    d = np.abs(got - val)
    with np.errstate(all="ignore"):
        r = np.where(d == 0, 0.0, d / (EPS32 * scale))
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


def measure(got, ref, cap_maxstep=False):
    """-> the error of `got` (dict: H, b, Hsc, bsc, res, ec, pts, jb) per quantity in units of eps32 * S, after asserting everything that is exact: isGood_new, the
    carried energies and the 1e10 of points that are not good after the evaluation, res[1], res[2], ec[2], +inf / 0 at t = 0.
    cap_maxstep: `got` takes the minimum into a maxstep that starts at 1e10, as the reference implementation does (so +inf never enters); the kernel's minimum
    runs over the visited pixels alone."""
    p = got["pts"]
    gn = ref.isGood_new
    assert np.array_equal(p["isGood_new"] != 0, gn), ("isGood_new differs at", np.nonzero((p["isGood_new"] != 0) != gn)[0][:8])
    assert np.array_equal(p["energy_new"][~gn], ref.energy_new[~gn].astype(np.float32)), "carried energy of a point that is not good-new"
    ms_ref = np.minimum(ref.maxstep, 1e10) if cap_maxstep else ref.maxstep
    ms_exact = ~np.isfinite(ms_ref) | (ms_ref == 1e10)                      # nothing visited (1e10) or t = 0 (+inf): prescribed exactly
    with np.errstate(over="ignore"):
        assert np.array_equal(p["maxstep"][ms_exact], ms_ref[ms_exact].astype(np.float32)), "maxstep where it is prescribed exactly (1e10 / +inf)"
    assert np.isfinite(p["maxstep"][~ms_exact]).all()
    assert float(got["res"][1]) == float(np.float32(ref.res1)) and float(got["res"][2]) == ref.res2 and float(got["ec"][2]) == ref.ec2, (got["res"], got["ec"], ref.res1, ref.ec2)
    for nm in ("H", "b", "Hsc", "bsc", "res", "ec"):
        assert np.isfinite(got[nm]).all(), nm
    if ref.t_is_zero:
        assert np.array_equal(p["lastHessian_new"][gn], np.zeros(gn.sum(), np.float32))
    un = {nm: _units(got[nm], *ref.sums[nm]) for nm in ("H", "b", "Hsc", "bsc")}
    un["E"] = _units(got["res"][0], *ref.sums["E"])
    un["ec0"], un["ec1"] = _units(got["ec"][0], *ref.sums["ec0"]), _units(got["ec"][1], *ref.sums["ec1"])
    un["energy_new"] = _units(p["energy_new"][gn], ref.energy_new[gn], ref.energy_scale[gn])
    un["lastHessian_new"] = _units(p["lastHessian_new"][gn], ref.lastHessian_new[gn], ref.lastHessian_scale[gn])
    un["maxstep"] = _units(p["maxstep"][~ms_exact], ms_ref[~ms_exact], ref.maxstep_scale[~ms_exact])
    un["Jb"] = _units(got["jb"][gn], ref.Jb[gn], ref.Jb_scale[gn])
    return un


def bounds(u_oracle):
    return {q: max(ORACLE_FACTOR * u_oracle[q], FLOOR_UNITS) for q in QUANTITIES}


def check_stage(got, ref, u_oracle, label="", cap_maxstep=False):
    """THE assertion of the stage tests: every entry within max(4 * u_oracle, 16) * eps32 * S of the float64 value.  -> the measured units"""
    un = measure(got, ref, cap_maxstep)
    bd = bounds(u_oracle)
    print(label, "units", {q: round(un[q], 2) for q in QUANTITIES}, "bound", {q: round(bd[q], 1) for q in QUANTITIES})
    over = {q: (un[q], bd[q]) for q in QUANTITIES if not un[q] <= bd[q]}
    assert not over, (label, over)
    return un


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# doStep / applyStep / resetPoints' per-point part
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def step_ref(pts, jb, mode, apply_pending, inc, lam, fault=None):
    """float64 of what k_ini_eval does to the records before it evaluates: applyStep of a pending step, then resetPoints' per-point part (mode 0) or doStep
    (mode 1) on JbBuffer `jb` [n, 10].  -> the records an exact implementation leaves (idepth_new in float64 in .idn), the scale of the step's terms, and where
    the clamp to [1e-3, 50] acts with a margin.  fault: "no_maxstep_clamp", "no_lastHessian" (sensitivity tests)."""
    out = pts.copy()
    good = pts["isGood"] != 0
    idn = pts["idepth_new"].astype(np.float64)
    if apply_pending:
        out["idepth"] = np.where(good, pts["idepth_new"], pts["iR"])
        idn = np.where(good, idn, pts["iR"].astype(np.float64))
        out["energy"] = np.where(good[:, None], pts["energy_new"], pts["energy"])
        out["isGood"] = np.where(good, pts["isGood_new"], pts["isGood"])
        if fault != "no_lastHessian":
            out["lastHessian"] = np.where(good, pts["lastHessian_new"], pts["lastHessian"])
    idp = out["idepth"].astype(np.float64)
    g2 = out["isGood"] != 0
    scale = np.abs(idn)
    clamp_lo, clamp_hi = np.zeros(len(pts), bool), np.zeros(len(pts), bool)
    if mode == 0:
        out["energy"] = 0
        idn = idp.copy()
        exact = np.ones(len(pts), bool)
    else:
        J = jb.astype(np.float64)
        incd = np.asarray(inc, np.float32).astype(np.float64)
        lamd = float(np.float32(lam))
        bb = J[:, 8] + J[:, :8] @ incd
        bb_a = np.abs(J[:, 8]) + np.abs(J[:, :8]) @ np.abs(incd)
        step = -bb * J[:, 9] / (1 + lamd)
        with np.errstate(over="ignore"):
            mx = np.minimum(0.25 * pts["maxstep"].astype(np.float64), 1e10)
        if fault != "no_maxstep_clamp":
            step = np.clip(step, -mx, mx)
        raw = idp + step
        new = np.clip(raw, float(np.float32(1e-3)), 50.0)
        clamp_lo, clamp_hi = g2 & (raw < 1e-3 * (1 - GUARD_REL)), g2 & (raw > 50.0 * (1 + GUARD_REL))
        idn = np.where(g2, new, idn)
        scale = np.where(g2, np.abs(idp) + bb_a * np.abs(J[:, 9]) / (1 + lamd), np.abs(idn))
        exact = ~g2
    return types.SimpleNamespace(pts=out, idn=idn, scale=scale, exact=exact, clamp_lo=clamp_lo, clamp_hi=clamp_hi, good=g2)


STEP_UNITS = 8.0


def check_step(got_pts, sr, label=""):
    """THE assertion of the step tests on the records: applyStep's copies and resetPoints' writes byte-equal, idepth_new exactly at the clamp where the clamp acts
    with a margin, elsewhere within 8 * eps32 * (|idepth| + sum |terms of the step|).  -> the measured units"""
    for f in ("energy", "isGood", "idepth", "lastHessian"):
        assert np.array_equal(got_pts[f], sr.pts[f]), (label, f, "not byte-equal")
    idn = got_pts["idepth_new"]
    assert np.array_equal(idn[sr.exact], sr.idn[sr.exact].astype(np.float32)), (label, "idepth_new where no step is taken")
    assert (idn[sr.clamp_lo] == np.float32(1e-3)).all() and (idn[sr.clamp_hi] == np.float32(50.0)).all(), (label, "clamp to [1e-3, 50]")
    assert (idn[sr.good] >= np.float32(1e-3)).all() and (idn[sr.good] <= np.float32(50.0)).all(), (label, "outside [1e-3, 50]")
    un = _units(idn[~sr.exact], sr.idn[~sr.exact], sr.scale[~sr.exact])
    print(label, "idepth_new units", round(un, 3), "bound", STEP_UNITS)
    assert un <= STEP_UNITS, (label, un)
    return un


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 8, 31, 32, 33, 8191, 8192, 8193, 8225, 16385)
ONE_HOT = tuple(range(32)) + (32, 8191, 8192, 8224)
# poses: |t|^2 against alphaK / alphaW = 2.78e-4.  t_z < 0 moves the pattern outwards at all four borders; rotations of a quarter to half a degree
POSES = {"large_t": ((0.03, -0.01, -0.03), (0.002, -0.004, 0.003)), "small_t": ((0.008, -0.003, -0.009), (0.002, -0.004, 0.003)), "zero_t": ((0.0, 0.0, 0.0), (0.004, 0.009, -0.005))}
AFF = (0.02, 1.5)


def pose(kind):
    t, w = POSES[kind]
    T = np.eye(4)
    T[:3, :3] = synth.so3_exp(np.array(w))
    T[:3, 3] = t
    return T


@functools.lru_cache(maxsize=None)
def sequence():
    seq = synth.make_init_sequence(W0, H0, n_frames=2, fx=FX, seed=20261020, levels=LEVELS)
    return seq, synth.make_images(seq["first"], LEVELS), synth.make_images(seq["frames"][1], LEVELS)


@functools.lru_cache(maxsize=None)
def nonfinite_frames():
    """-> first frame, new frame (irradiance) with one NaN in the first and one NaN and one +Inf in the new one, their pyramids, the pixels"""
    seq, _, _ = sequence()
    first, new = seq["first"].copy(), seq["frames"][1].copy()
    px = {"first_nan": (60, 40), "new_nan": (120, 90), "new_inf": (41, 101)}             # (x, y)
    first[px["first_nan"][1], px["first_nan"][0]] = np.nan
    new[px["new_nan"][1], px["new_nan"][0]] = np.nan
    new[px["new_inf"][1], px["new_inf"][0]] = np.inf
    return first, new, synth.make_images(first, LEVELS), synth.make_images(new, LEVELS), px


@functools.lru_cache(maxsize=None)
def base_points(n):
    """records of a two-level handle with exactly n points on level 0 (a fixed random choice among the 185 x 137 interior pixels, in random order) and a regular
    grid of 23 x 17 on level 1; the points at the indices of ONE_HOT lie at least 12 pixels inside"""
    xs, ys = np.meshgrid(np.arange(3, W0 - 4), np.arange(3, H0 - 4))
    assert xs.size == 185 * 137
    order = np.random.default_rng(7).permutation(xs.size)
    inner = lambda i: 12 <= xs.ravel()[order[i]] < W0 - 12 and 12 <= ys.ravel()[order[i]] < H0 - 12
    spare = (i for i in range(max(ONE_HOT) + 1, xs.size) if inner(i))          # beyond every count: the choice is the same for every n
    for i in ONE_HOT:                                                           # the points of the one-good-point cases stay in the image under every pose
        if not inner(i):
            j = next(spare)
            order[i], order[j] = order[j], order[i]
    order = order[:n]
    x1, y1 = np.meshgrid(np.arange(3, W0 // 2 - 4, 4), np.arange(3, H0 // 2 - 4, 4))
    return synth.init_point_records([(xs.ravel()[order], ys.ravel()[order]), (x1.ravel(), y1.ravel())])


def randomise(p, seed, t_z):
    """the state of the points of a case: random idepth, idepth_new and iR, 5 % not good, carried energies, 10 % with a low outlier threshold, a few idepth_new
    near 40 (new_idepth <= 0 under t_z < -1 / 40)"""
    rng = np.random.default_rng(seed)
    n = len(p)
    p = p.copy()
    p["idepth"] = (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    p["idepth_new"] = (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    p["iR"] = (1.0 + 0.05 * rng.standard_normal(n)).astype(np.float32)
    p["isGood"] = (rng.uniform(size=n) > 0.05).astype(np.int32)
    p["energy"] = rng.uniform(0, 50, (n, 2)).astype(np.float32)
    p["lastHessian"] = rng.uniform(0, 5, n).astype(np.float32)
    low = rng.uniform(size=n) < 0.10
    p["outlierTH"] = np.where(low, rng.uniform(2.0, 30.0, n), p["outlierTH"]).astype(np.float32)
    far = rng.uniform(size=n) < 1.0 / 64
    p["idepth_new"] = np.where(far, rng.uniform(38.0, 45.0, n), p["idepth_new"]).astype(np.float32)
    p["isGood"][0] = 1; p["idepth_new"][0] = 1.05; p["outlierTH"][0] = 1152.0              # so that n = 1 evaluates its point
    return p


def guard(K4, lvl, first, cur, p, T, a, b, snapped, nonfinite=False):
    """isGood = 0 on every point with a decision margin under the guard -> records, reference of the guarded records, share of points removed"""
    ref = stage_ref(K4, lvl, first, cur, p, T, a, b, snapped)
    m = ref.margins
    bad = (p["isGood"] != 0) & ((m.px < GUARD_PX) | (m.depth < GUARD_PX) | (m.energy < GUARD_REL))
    if nonfinite:                                               # which 2 x 2 cell a tap next to a non-finite pixel reads must not depend on rounding either
        nf = ~np.isfinite(cur[..., 0])
        near = np.zeros_like(nf)
        for yy, xx in zip(*np.nonzero(nf)):
            near[max(yy - 2, 0):yy + 3, max(xx - 2, 0):xx + 3] = True
        with np.errstate(invalid="ignore"):
            ix, iy = np.clip(np.nan_to_num(m.Ku), 0, cur.shape[1] - 1).astype(int), np.clip(np.nan_to_num(m.Kv), 0, cur.shape[0] - 1).astype(int)
            bad |= (p["isGood"] != 0) & (near[iy, ix] & (np.nan_to_num(m.frac) < GUARD_PX)).any(axis=1)
    assert m.alpha > GUARD_REL or not np.asarray(T)[:3, 3].any()
    p = p.copy()
    p["isGood"][bad] = 0
    return p, stage_ref(K4, lvl, first, cur, p, T, a, b, snapped), float(bad.mean())


# a case: name -> (n on level 0, level, pose, snapped, kind); kind "random", ("one_hot", index) or "nonfinite"
def _cases():
    c = {}
    for n in COUNTS:
        for kind in POSES:
            for snapped in (0, 1):
                c[f"n{n}_{kind}_s{snapped}"] = (n, 0, kind, snapped, "random")
    c["n16385_level1_large_t_s1"] = (16385, 1, "large_t", 1, "random")
    c["n16385_level1_small_t_s0"] = (16385, 1, "small_t", 0, "random")
    for i in ONE_HOT:
        c[f"n8225_one_hot_{i}"] = (8225, 0, "large_t", 1, ("one_hot", i))
    for kind in POSES:
        c[f"n8225_nonfinite_{kind}"] = (8225, 0, kind, 1, "nonfinite")
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace: n0, lvl, T, a, b, snapped, pts (guarded records of the level), ref (their float64 reference), removed (share of guarded points), frames"""
    n0, lvl, kind, snapped, what = CASES[name]
    seq, pyr_first, pyr_new = sequence()
    if what == "nonfinite":
        _, _, pyr_first, pyr_new, _ = nonfinite_frames()
    T = pose(kind)
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    a, b = AFF
    for attempt in range(64):          # at most 1 % of a case may be guarded: where one point is more than that, the first seed that guards none
        c = _build(name, n0, lvl, T, a, b, snapped, what, seed + 1000 * attempt, seq, pyr_first, pyr_new)
        if c.removed <= 0.01:
            return c
    return c


def _build(name, n0, lvl, T, a, b, snapped, what, seed, seq, pyr_first, pyr_new):
    p = randomise(base_points(n0)[lvl], seed, T[2, 3])
    if isinstance(what, tuple):
        keep = what[1]
        # the one good point: one that stays in the image, with a moderate depth
        p["idepth_new"][keep] = 1.05; p["outlierTH"][keep] = 1152.0
        g = np.zeros(len(p), np.int32); g[keep] = 1
        p["isGood"] = g
    p, ref, removed = guard(seq["K4"], lvl, pyr_first[lvl], pyr_new[lvl], p, T, a, b, snapped, nonfinite=what == "nonfinite")
    return types.SimpleNamespace(name=name, n0=n0, lvl=lvl, T=T, a=a, b=b, snapped=snapped, pts=p, ref=ref, removed=removed, what=what, K4=seq["K4"],
                                 first=pyr_first[lvl], cur=pyr_new[lvl])


def run_impl(impl, c):
    """one stage evaluation of case c on an implementation with the interface of binding.Initializer / pyoracle.OracleInitializer -> `got`"""
    st = impl.state(); st["snapped"] = c.snapped; impl.set_state(st)
    impl.set_points(c.lvl, c.pts)
    H, b, Hsc, bsc, res, ec = impl.calc_res_and_gs(c.lvl, c.T, c.a, c.b)
    return dict(H=H, b=b, Hsc=Hsc, bsc=bsc, res=res, ec=ec, pts=impl.points(c.lvl), jb=impl.jb(c.lvl))


@functools.lru_cache(maxsize=None)
def oracle_handle(n0, nonfinite=False):
    from oracle import pyoracle
    seq, pyr_first, pyr_new = sequence()
    if nonfinite:
        _, _, pyr_first, pyr_new, _ = nonfinite_frames()
    o = pyoracle.OracleInitializer(W0, H0, LEVELS)
    o.set_first(seq["K4"], pyr_first, 1.0, base_points(n0))
    o.set_new_frame(pyr_new, 1.0)
    return o


@functools.lru_cache(maxsize=None)
def oracle_units(name):
    """the oracle's own error on the case, per quantity, in units of eps32 * S (its maxstep starts at 1e10: cap_maxstep)"""
    c = case(name)
    got = run_impl(oracle_handle(c.n0, c.what == "nonfinite"), c)
    return measure(got, c.ref, cap_maxstep=True), got
