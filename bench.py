#!/usr/bin/env python
"""bench.py — Gauss-Newton iterations/s (and Mresiduals/s) of the windowed photometric BA hot path on MI355X.

Workload (BASELINE.json configs[2], "C3"): 7 keyframes x 2000 points x 8-pixel pattern, 640x480, R = 12000
residuals, synthetic window (seed 20260925), forced iterations (canbreak ignored).  One *step* = one GN iteration
= solveSystem (accumulate A/L/SC, stitch, solve, back-substitute) + doStepFromBackup + linearizeAll + applyRes
(reference FullSystem.cc:777-831), with the window resident in HBM: two launches on one GPU (k_reduce_solve = k_reduce + the control
step in one launch -> k_linearize with the point step fused in).  N > 1: points are sharded across the ranks,
one RCCL all-reduce of the stitched system per iteration, replicated solve (strong scaling).

Prints ONE JSON line (rank 0).  A plain run sets the window up, runs --warmup iterations, times ONE block of exactly --steps
iterations between two fences (`ms_per_step` = that block / --steps), writes the outputs if --dump-outputs is given and prints
the line.  --dump-outputs DIR: the state the timed iterations left behind (frame states and poses, calibration, inverse depths
and their Hessians, residual energies and states) as DIR/<name>.npy, float32 / float64, taken right after the first timed block
so that a plain and a --full run of the same arguments write the same arrays.

--full adds everything else, as before: the timed block repeated until --min-timed-s (default 2 s) has been measured (median
block reported), the parity checks against the oracle, the kernel timings, `roofline`, `cpu_baseline` and the other windows
and components (C4 / C5, batched windows, adapter, tracker, tracer, initialiser).  `roofline` is for the dominant kernel
(k_linearize): algorithmic bytes per launch (436 B per residual + 112 B per point) / average launch duration
measured with HIP events on the launch stream in a separate profiled pass of the same process.  `cpu_baseline` times the oracle
(CPU restatement of the reference, "port") on this box's host cores with the reference's 6-worker IndexThreadReduce schedule.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def committed_profile(config, what):
    """Committed rocprofv3 figures of the same command (profiles/rNN_*): never part of `achieved`, printed next to the live numbers."""
    import csv, glob
    try:
        if what == "kernel_us":
            cand = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_bench_{config}_kernel_stats*.csv")))
            if cand:
                for row in csv.DictReader(open(cand[-1])):
                    if "k_linearize" in row["Name"]:
                        return round(float(row["AverageNs"]) / 1e3, 3), os.path.relpath(cand[-1], ROOT)
        else:
            cand = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic*.json")), key=lambda f: os.path.basename(f)[:3])
            for fn in reversed(cand):                               # latest round first
                pj = json.load(open(fn))
                if pj.get("config", "C3") == config:
                    # the GN-iteration kernel = the k_linearize* entry with the most launches (k_linearize_batch<1> with one window from
                    # round 2 on, k_linearize<...> before and for windows with linearised residuals)
                    cands = [(kv.get("launches_FETCH_SIZE", 0), kv["hbm_bytes_per_launch_corrected"]) for kname, kv in pj["kernels"].items()
                             if kname.startswith("k_linearize") and "hbm_bytes_per_launch_corrected" in kv]
                    if cands:
                        return max(cands)[1], os.path.relpath(fn, ROOT)
    except Exception:
        pass
    return None, None


def committed_per_kernel(config):
    """{short kernel name: {"rocprofv3_us", "hbm_bytes_pmc"}} of the GN iteration's kernels from the latest committed profiles of this config."""
    import csv, glob
    out = {}
    try:
        cand = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_bench_{config}_kernel_stats*.csv")))
        if cand:
            for row in csv.DictReader(open(cand[-1])):
                nm = row["Name"].replace("void ", "").split("(")[0]
                if nm.startswith(("k_linearize_one", "k_reduce_solve", "k_gn_solve", "k_reduce")) and int(row["Calls"]) > 100:
                    out.setdefault(nm, {})["rocprofv3_us"] = round(float(row["AverageNs"]) / 1e3, 3)
                    out[nm]["rocprofv3_profile"] = os.path.relpath(cand[-1], ROOT)
        cand = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic*.json")), key=lambda f: os.path.basename(f)[:3])
        for fn in reversed(cand):
            pj = json.load(open(fn))
            if pj.get("config", "C3") == config:
                for kname, kv in pj["kernels"].items():
                    if kname in out and "hbm_bytes_per_launch_corrected" in kv:
                        out[kname]["hbm_bytes_pmc"] = kv["hbm_bytes_per_launch_corrected"]; out[kname]["pmc_profile"] = os.path.relpath(fn, ROOT)
                break
    except Exception:
        pass
    return out


def transplant(win, frames, points, residuals):
    """The window with the evaluation state a GPU handle holds (frames, calibration, inverse depths, residual states)."""
    import copy
    w2 = copy.deepcopy(win)
    w2.frames = frames["frames"].copy()
    w2.calib = w2.calib.copy(); w2.calib["value"] = frames["calib_value"]
    w2.points = w2.points.copy()
    w2.points["idepth"] = points["idepth"]; w2.points["idepth_zero"] = points["idepth"]
    w2.residuals = w2.residuals.copy()
    w2.residuals["state_state"] = residuals["state_state"]; w2.residuals["is_active"] = residuals["is_active"]
    w2.residuals["state_energy"] = residuals["out"]["state_NewEnergy"]
    return w2


def parity_check(win, ba, stream):
    """OUTSIDE the timed region (oracle = checker only): (i) the oracle re-evaluates the state the timed run left behind - the
    energy the GPU reports for it must be the oracle's; (ii) a fresh 10-iteration run of the same fast path against the oracle's
    FullSystem::optimize loop, energy per iteration.  Tolerance 1e-4 relative (north_star).  Raises on violation."""
    from ldso_amd import binding
    from oracle import pyoracle as po
    n = 8 * win.F + 4
    buf = torch.zeros(ba.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    ba.gn_reduce_local(buf.data_ptr(), 1e-1); ba.sync(); torch.cuda.synchronize()
    e_gpu = float(buf[n * n + n].item())
    w2 = transplant(win, ba.get_frames(), ba.get_points(), ba.get_residuals())
    o = po.OracleWindow(w2); o.collect_active(reset_oob=False)
    e_orc = o.linearize_all(False); o.close()
    o2 = po.OracleWindow(win); o2.set_force_all_iterations(True); o2.optimize(10)
    g2 = binding.BA.from_window(win, stream=stream); g2.optimize(10, force_all=True)
    eo, eg = o2.energy_log(), g2.get_energy_log()
    o2.close(); g2.close()
    r1 = abs(e_gpu - e_orc) / abs(e_orc)
    r2 = float(np.max(np.abs(eg - eo) / np.abs(eo)))
    res = {"energy_after_timed_run_gpu": e_gpu, "energy_oracle_at_that_state": e_orc, "rel": r1,
           "energy_log_10_iterations_max_rel": r2, "tolerance": 1e-4, "ok": bool(r1 <= 1e-4 and r2 <= 1e-4 and len(eo) == len(eg))}
    if not res["ok"]:
        raise SystemExit(f"bench.py: parity check against the oracle failed: {res}")
    return res


def parity_check_dist(win, ba, rank, world, dist, pb, pe, stream, device):
    """The N > 1 (or --force-dist-path) counterpart of parity_check, OUTSIDE the timed region: (i) every rank's frame states must be
    bit-identical (replicated solve on the all-reduced system); the shards' points / residual states are gathered on rank 0, the oracle
    re-evaluates that state and its energy must be the sum of the ranks' energies; (ii) a fresh sharded 10-iteration run (reduce_local ->
    all-reduce -> solve_reduced) against the oracle's FullSystem::optimize loop, total energy before every iteration and after the last.
    Tolerance 1e-4 relative (north_star).  Rank 0 raises on violation (the other ranks return None)."""
    from ldso_amd import binding
    from oracle import pyoracle as po
    n = 8 * win.F + 4

    def allsum(t):
        if world > 1:
            dist.all_reduce(t)
        return t

    def gathered(x):
        if world == 1:
            return [x]
        out = [None] * world
        dist.all_gather_object(out, x)
        return out

    buf = torch.zeros(ba.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    ba.gn_reduce_local(buf.data_ptr(), 1e-1); ba.sync(); torch.cuda.synchronize()
    e_gpu = float(allsum(buf[n * n + n:n * n + n + 1].clone()).item())
    fr, pts, res = ba.get_frames(), ba.get_points(), ba.get_residuals()
    mine = (win.residuals["point"] >= pb) & (win.residuals["point"] < pe)
    parts = gathered({"pb": pb, "pe": pe, "state": fr["frames"]["state"].copy(), "calib": np.asarray(fr["calib_value"]).copy(), "idepth": pts["idepth"][pb:pe].copy(),
                      "rows": np.nonzero(mine)[0], "state_state": res["state_state"][mine].copy(), "is_active": res["is_active"][mine].copy(),
                      "energy": res["out"]["state_NewEnergy"][mine].copy()})
    # (ii) fresh sharded run, energies of the all-reduced scalar block
    g2 = binding.BA.from_window(win, device=device, stream=stream)
    if world > 1:
        g2.set_shard(pb, pe)
    g2.collect_active(); g2.linearize_all(False); g2.apply_res()
    b2 = torch.zeros(g2.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    es = []
    for i in range(11):
        g2.gn_reduce_local(b2.data_ptr(), 1e-1)
        allsum(b2)
        torch.cuda.synchronize()
        es.append(float(b2[n * n + n].item()))
        if i < 10:
            g2.gn_solve_reduced(b2.data_ptr(), i, 1e-1)
    g2.sync(); g2.close()
    if rank != 0:
        return None
    ranks_diff = max(float(np.max(np.abs(q["state"] - parts[0]["state"]))) for q in parts)
    ranks_diff = max(ranks_diff, max(float(np.max(np.abs(q["calib"] - parts[0]["calib"]))) for q in parts))
    idepth = pts["idepth"].copy(); ss = res["state_state"].copy(); act = res["is_active"].copy(); en = res["out"]["state_NewEnergy"].copy()
    for q in parts:
        idepth[q["pb"]:q["pe"]] = q["idepth"]; ss[q["rows"]] = q["state_state"]; act[q["rows"]] = q["is_active"]; en[q["rows"]] = q["energy"]
    covered = int(sum(len(q["rows"]) for q in parts))
    w2 = transplant(win, fr, {"idepth": idepth}, {"state_state": ss, "is_active": act, "out": {"state_NewEnergy": en}})
    o = po.OracleWindow(w2); o.collect_active(reset_oob=False)
    e_orc = o.linearize_all(False); o.close()
    o2 = po.OracleWindow(win); o2.set_force_all_iterations(True); o2.optimize(10)
    eo = np.asarray(o2.energy_log())[:11]; o2.close()
    eg = np.asarray(es)
    r1 = abs(e_gpu - e_orc) / abs(e_orc)
    r2 = float(np.max(np.abs(eg - eo) / np.abs(eo))) if len(eo) == len(eg) else float("inf")
    out = {"ranks": world, "energy_after_timed_run_sum_over_ranks": e_gpu, "energy_oracle_at_that_state": e_orc, "rel": r1,
           "energy_log_10_iterations_max_rel": r2, "frame_states_max_abs_diff_between_ranks": ranks_diff, "residuals_covered_by_shards": covered,
           "tolerance": 1e-4, "ok": bool(r1 <= 1e-4 and r2 <= 1e-4 and ranks_diff == 0.0 and covered == win.R)}
    if not out["ok"]:
        raise SystemExit(f"bench.py: sharded parity check against the oracle failed: {out}")
    return out


GRAPH_CHUNK = 1000          # iterations per enqueue of the timed path at most (see measure: run_steps)


def collect_outputs(win, ba, world, dist, pb, pe):
    """What a caller of the timed path receives after it: frame states and poses, calibration, inverse depths, residual energies and
    states (float32 / float64).  N > 1: the frame states are replicated, the points and residuals of the other ranks' shards are
    gathered (all ranks call this).  -> {name: array} on rank 0, None elsewhere."""
    fr, pts, res = ba.get_frames(), ba.get_points(), ba.get_residuals()
    idepth, hess = pts["idepth"].copy(), pts["idepth_hessian"].copy()
    energy, state = res["out"]["state_NewEnergy"].copy(), res["state_state"].copy()
    if world > 1:
        mine = (win.residuals["point"] >= pb) & (win.residuals["point"] < pe)
        parts = [None] * world
        dist.all_gather_object(parts, {"pb": pb, "pe": pe, "idepth": idepth[pb:pe], "hess": hess[pb:pe], "rows": np.nonzero(mine)[0],
                                       "energy": energy[mine], "state": state[mine]})
        if dist.get_rank() != 0:
            return None
        for q in parts:
            idepth[q["pb"]:q["pe"]] = q["idepth"]; hess[q["pb"]:q["pe"]] = q["hess"]
            energy[q["rows"]] = q["energy"]; state[q["rows"]] = q["state"]
    return {"frames_state": np.asarray(fr["frames"]["state"], np.float64),
            "frames_world_to_cam": np.asarray(fr["pre_worldToCam"], np.float64),
            "calib_value": np.asarray(fr["calib_value"], np.float64),
            "points_idepth": idepth.astype(np.float32),
            "points_idepth_hessian": hess.astype(np.float32),
            "residuals_energy": energy.astype(np.float32),
            "residuals_state": state.astype(np.float32)}


def write_outputs(outputs, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    assert sum(a.nbytes for a in outputs.values()) <= 64 << 20
    for name, a in outputs.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def measure(args, config, rank, local_rank, world, dist, steps, warmup, min_timed_s=2.0, with_parity=True, full=True, dump_dir=None):
    """One BASELINE window: time of blocks of EXACTLY `steps` forced GN iterations (one block when min_timed_s is 0, else the median
    block) and, with `full`, the parity checks and the live roofline of k_linearize.  dump_dir: write the outputs of the first block."""
    from ldso_amd import synth, binding, dist as ldist
    win = synth.make_config(config)
    if not args.no_prior:
        synth.add_synthetic_prior(win)          # steady-state windows always carry H_M / b_M (EnergyFunctional::marginalizeFrame)
    F, P, R = win.F, win.P, win.R
    # everything (our kernels, torch ops, the RCCL all-reduce) is ordered on ONE non-default torch stream
    tstream = torch.cuda.Stream()
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    ba = binding.BA.from_window(win, device=local_rank, stream=stream)
    pb, pe = ldist.shard_range(P, rank, world)
    if world > 1:
        ba.set_shard(pb, pe)
    ba.collect_active()
    ba.linearize_all(False)
    ba.apply_res()
    dist_path = world > 1 or args.force_dist_path
    rbuf = torch.zeros(ba.gn_reduce_doubles(), dtype=torch.float64, device="cuda") if dist_path else None
    windows = None
    if dist_path and args.allreduce == "p2p":
        # every rank's receive window, exchanged as hipIpcMemHandle_t through the process group (control plane only: the data path is peer stores)
        own, hnd = ba.p2p_window_alloc(world, with_ipc_handle=True)
        if world > 1:
            allh = [None] * world
            dist.all_gather_object(allh, hnd)
            windows = [own if q == rank else ba.p2p_window_open(allh[q]) for q in range(world)]
        else:
            windows = [own]

    def run(k, it0):
        if not dist_path:
            ba.enqueue_gn(it0, k)
        elif windows is not None:
            ba.enqueue_gn_p2p(rank, world, windows, it0, k)     # reduce_local -> peer-write exchange -> replicated solve, all enqueued by the library
        elif world == 1:
            for i in range(k):                      # the multi-GPU step without the collective (one rank owns everything)
                ba.gn_reduce_local(rbuf.data_ptr(), 1e-1)
                ba.gn_solve_reduced(rbuf.data_ptr(), it0 + i, 1e-1)
        else:
            # the all-reduce buffer is the HFinal / bFinal accumulator of the 3-launch iteration (+ scalars, energy candidates)
            for i in range(k):
                ba.gn_reduce_local(rbuf.data_ptr(), 1e-1)
                dist.all_reduce(rbuf)
                ba.gn_solve_reduced(rbuf.data_ptr(), it0 + i, 1e-1)

    def run_steps(n, it0):
        # enqueue_gn captures one HIP graph per (first iteration, count, parity of the handle's buffer sets) and replays it afterwards: n iterations go as
        # chunks of at most GRAPH_CHUNK (even, so every full chunk replays the same graph); the kernels only distinguish iteration < 2, so later chunks start at 2
        while n > 0:
            k = min(n, GRAPH_CHUNK)
            run(k, it0)
            n, it0 = n - k, max(it0, 2)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    run_steps(warmup, 0)
    # capture the graphs of the timed block before the clock starts: its chunk shapes once each, then one more iteration if that left the parity flipped
    shapes = [min(steps, GRAPH_CHUNK)] + ([steps % GRAPH_CHUNK] if steps > GRAPH_CHUNK and steps % GRAPH_CHUNK else [])
    for k in shapes:
        run(k, 2)
    if sum(shapes) % 2:
        run(1, 2)
    fence()
    # The contract times EXACTLY `steps` iterations between two fences.  A plain run (min_timed_s 0) times one such block.  With
    # min_timed_s > 0 (--full: 2 s for the headline window, long enough for GPU-busy sampling to see it) the block is repeated until
    # that much has been timed and the MEDIAN block is reported (every block bracketed by the fences, maximum over ranks per block).
    blocks, total, outputs = [], 0.0, None
    while not blocks or ((total < min_timed_s or len(blocks) < 3) and min_timed_s > 0 and len(blocks) < 200000):
        fence()
        t0 = time.perf_counter()
        run_steps(steps, 2)
        fence()
        d = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([d], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            d = float(t.item())
        blocks.append(d); total += d
        if len(blocks) == 1 and dump_dir is not None:
            # the state after warmup + the first block of `steps` iterations: the same in a plain and a --full run
            ba.sync(); fence()
            outputs = collect_outputs(win, ba, world, dist, pb, pe)
    dt = float(np.median(blocks))
    if windows is not None:
        ba.p2p_check()
    ok = bool(np.all(np.isfinite(ba.get_frames()["frames"]["state"])))
    if outputs is not None:
        write_outputs(outputs, dump_dir)
    headline = {
        "win": win,
        "value": round(steps / dt, 2),                       # median of the timed blocks of exactly `steps` iterations
        "mresiduals_per_s": round(steps * R / dt / 1e6, 3),
        "ms_per_step": round(dt / steps * 1e3, 5),
        "workload": f"{config}: {F} KF x {P} pt x 8 px, {win.w}x{win.h}, R={R}, forced GN iterations, "
                    + ("no prior" if args.no_prior else "synthetic rank-6 marginalisation prior H_M/b_M"),
        "timed_blocks": len(blocks), "timed_total_ms": round(total * 1e3, 2),
        "ms_per_step_min_max": [round(min(blocks) / steps * 1e3, 5), round(max(blocks) / steps * 1e3, 5)],
        "state_finite": ok,
    }
    if not full:
        ba.close()
        return headline
    parity = parity_check(win, ba, stream) if (with_parity and world == 1 and not dist_path) else None

    # ---- roofline of the dominant kernel: separate profiled pass (HIP events around every launch) -------------
    ba.profile(True)
    run(min(50, steps), 2)
    fence()
    names = ["k_linearize", "k_reduce", "k_gn_solve", "k_point_step"]
    ktimes = {}
    for i, nm in enumerate(names):
        ms, n = ba.kernel_time_ms(i)
        ktimes[nm] = {"avg_us": round(ms * 1e3, 3), "launches": n}
    if ktimes["k_reduce"]["launches"] == 0 and ktimes["k_gn_solve"]["launches"] > 0:      # single-GPU fast path: the two are one launch
        ktimes["k_reduce_solve"] = ktimes.pop("k_gn_solve")
        ktimes.pop("k_reduce")
    ev_ms, _ = ba.kernel_time_ms(4)          # empty event pair = overhead of the measurement itself
    ba.profile(False)
    Rloc = int(((win.residuals["point"] >= pb) & (win.residuals["point"] < pe)).sum())
    alg_bytes = 436 * Rloc + 112 * (pe - pb)
    # dominant kernel, measured LIVE in this process: (i) back-to-back launches between one event pair (event overhead amortised,
    # the dependent-launch boundary included), (ii) per-launch event pairs inside the GN pipeline minus an empty pair.  The larger
    # (conservative) of the two is `avg_launch_us` and the only figure `achieved` is computed from; the committed rocprofv3 average
    # of the same command is printed next to it (profiles/ is regenerated in the commit that changes a kernel).
    lin_b2b = ba.time_linearize(100)
    lin_insitu = max(ktimes["k_linearize"]["avg_us"] - ev_ms * 1e3, 0.0)
    lin_live_us = max(lin_b2b, lin_insitu)
    single = world == 1 and not args.no_prior and not dist_path
    rocprof_us, rocprof_src = committed_profile(config, "kernel_us") if single else (None, None)
    # `achieved` / `frac` follow from the LONGER of (live HIP-event duration in this process, committed rocprofv3 --kernel-trace average of
    # the same command under profiles/): a reader who recomputes frac from profiles/ gets this number or a better one, never a worse one.
    lin_us = max(lin_live_us, rocprof_us or 0.0)
    achieved = alg_bytes / (lin_us * 1e-6) / 1e9 if lin_us > 0 else 0.0
    achieved_live = alg_bytes / (lin_live_us * 1e-6) / 1e9 if lin_live_us > 0 else 0.0
    # HBM traffic per launch: rocprofv3 PMC counters cannot be read from inside this process; the value is the committed
    # measurement of the same command (profiles/rNN_pmc_traffic.json: 2 x FETCH_SIZE + WRITE_SIZE, the guide's gfx950 correction)
    traffic, traffic_src = committed_profile(config, "traffic") if single else (None, None)
    if with_parity and dist_path:
        if windows is not None:
            ba.sync(); fence()
        parity = parity_check_dist(win, ba, rank, world, dist, pb, pe, stream, local_rank)
    ba.close()
    # the WHOLE step against the roofline (436 R + 112 P + 8 n^2 algorithmic bytes per GN iteration over the driver-timed ms_per_step), and every
    # kernel of the iteration with its own bytes and time: k_linearize is the HBM-side kernel `frac` grades, the control kernel is where the time goes
    n_sys = 8 * F + 4
    step_bytes = alg_bytes + 8 * n_sys * n_sys
    step_GBps = step_bytes / (dt / steps) / 1e9
    comm = committed_per_kernel(config) if single else {}
    per_kernel = []
    for nm, kt in ktimes.items():
        if kt["launches"] == 0:
            continue
        live = max(kt["avg_us"] - ev_ms * 1e3, 0.0)
        kb = alg_bytes if nm == "k_linearize" else (8 * n_sys * n_sys if nm in ("k_reduce_solve", "k_gn_solve") else 0)
        cm = next((v for k_, v in comm.items() if (k_.startswith("k_linearize_one") if nm == "k_linearize" else k_ == nm)), {})
        per_kernel.append({"name": nm, "live_us_in_pipeline": round(live, 3), "rocprofv3_us_committed": cm.get("rocprofv3_us"),
                           "algorithmic_bytes": kb, "hbm_bytes_pmc_committed": cm.get("hbm_bytes_pmc"),
                           "share_of_step": round(live / (dt / steps * 1e6), 3),
                           "frac_of_8TBps": round(kb / (max(live, cm.get("rocprofv3_us") or 0.0) * 1e-6) / 8e12, 5) if live > 0 else None})
    return {
        **headline,
        "roofline": {"bound": "hbm", "kernel": "k_linearize", "achieved": round(achieved, 2), "peak": 8000.0, "unit": "GB/s",
                     "frac": round(achieved / 8000.0, 5), "traffic": traffic, "traffic_source": traffic_src,
                     "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_us": round(lin_us, 3),
                     "avg_launch_us_source": "committed rocprofv3 average" if (rocprof_us or 0.0) >= lin_live_us else "live HIP events",
                     "achieved_live": round(achieved_live, 2), "frac_live": round(achieved_live / 8000.0, 5), "avg_launch_us_live": round(lin_live_us, 3),
                     "avg_launch_us_back_to_back_100": round(lin_b2b, 3), "avg_launch_us_in_pipeline_events_minus_empty_pair": round(lin_insitu, 3),
                     "rocprofv3_avg_us_committed_profile": rocprof_us, "rocprofv3_profile": rocprof_src,
                     "step_algorithmic_bytes": step_bytes, "step_achieved_GBps": round(step_GBps, 2), "step_frac": round(step_GBps / 8000.0, 5),
                     "per_kernel": per_kernel},
        "kernels": ktimes, "parity_vs_oracle": parity,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--full", action="store_true", help="also the parity checks, kernel timings, roofline, CPU baseline and the other windows / components (off: the headline line only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the state the timed iterations left behind as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the informational C4 / C5 / tracker / tracer / initialiser lines")
    ap.add_argument("--no-prior", action="store_true", help="window without the (synthetic) marginalisation prior H_M / b_M")
    ap.add_argument("--min-timed-s", type=float, default=None, help="repeat the timed block of exactly --steps iterations until this much time has been measured and report the median block "
                                                                   "(default: 2 with --full, profiling runs pass a small value; 0 without it: one block)")
    ap.add_argument("--allreduce", choices=["rccl", "p2p"], default="rccl", help="N > 1 (or --force-dist-path): RCCL all-reduce through torch.distributed, or the library's one-shot peer-write exchange (ldso_ba_enqueue_gn_p2p, windows shared as IPC handles)")
    ap.add_argument("--force-dist-path", action="store_true", help="1 GPU only: run the multi-GPU step (reduce_local / solve_reduced) with a no-op all-reduce")
    args = ap.parse_args()
    if args.min_timed_s is None:
        args.min_timed_s = 2.0 if args.full else 0.0

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE={world})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False (no CPU fallback)")
    # debugging aid (never set by the driver): LDSO_BENCH_ONE_GPU=1 runs all ranks on GPU 0 over gloo, to exercise the N > 1 code
    # path on a one-GPU box (RCCL refuses two ranks on one device)
    one_gpu_debug = os.environ.get("LDSO_BENCH_ONE_GPU") == "1"
    if one_gpu_debug:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_gpu_debug:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            # device_id binds the communicator to this rank's GPU up front (barrier() then never has to guess a device)
            try:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            except TypeError:          # older torch without device_id
                dist.init_process_group("nccl", rank=rank, world_size=world)

    m = measure(args, args.config, rank, local_rank, world, dist, args.steps, args.warmup, min_timed_s=args.min_timed_s, full=args.full, dump_dir=args.dump_outputs)
    win = m.pop("win")
    if rank == 0:
        out = {
            "metric": "GN iters/sec + Mresiduals/sec, 7-KF/2000-pt window",
            "value": m["value"],
            "unit": "GN iters/s",
            "mresiduals_per_s": m["mresiduals_per_s"],
            "n_gpus": world,
            "rccl_ranks": (world if (dist is not None and dist.get_backend() == "nccl") else 0),      # ranks of the RCCL communicator this line ran on (0: single process, or the gloo debug mode)
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": m["ms_per_step"],
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",      # residuals, Jacobians and accumulators as the reference; the stitch and the solve are f64 (see config.arithmetic)
            "data": "synthetic",
            "config": {"workload": m["workload"],
                       "arithmetic": "f32 residuals / Jacobians / accumulators as the reference, f64 stitch and solve",
                       "parallelism": "1 GPU" if world == 1 else f"points sharded over {world} GPUs, " + ("RCCL all-reduce" if args.allreduce == "rccl" else "one-shot peer-write all-reduce (ldso_ba_enqueue_gn_p2p)") + " of the stitched system per iteration"},
            **({"roofline": m["roofline"]} if args.full else {}),
            "timed_blocks": m["timed_blocks"], "timed_total_ms": m["timed_total_ms"], "ms_per_step_min_max": m["ms_per_step_min_max"],
            **({"kernels": m["kernels"]} if args.full else {}),
            "state_finite": m["state_finite"],
            **({"parity_vs_oracle": m["parity_vs_oracle"]} if args.full else {}),
        }
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(win)
        if args.full and not args.no_extras and world == 1 and not args.force_dist_path:
            # the other BASELINE windows (configs[3], configs[4]) on one GPU, each with its own live roofline and parity check
            for key, cfg in (("c4", "C4"), ("c5", "C5")):
                if cfg == args.config:
                    continue
                try:
                    e = measure(args, cfg, rank, local_rank, world, dist, min(args.steps, 100), min(args.warmup, 10), min_timed_s=0.2)
                    e.pop("win")
                    out[key] = e
                except SystemExit:
                    raise
                except Exception as ex:
                    out[key] = {"error": repr(ex)}
            try:
                out["batched"] = batched_line(args, local_rank)
            except Exception as ex:
                out["batched"] = {"error": repr(ex)}
            for key, fn in (("adapter", adapter_line), ("tracker", tracker_line), ("tracer", tracer_line), ("initializer", initializer_line)):
                try:
                    out[key] = fn()          # informational lines; never fail the BA metric on them
                except Exception as ex:
                    out[key] = {"error": repr(ex)}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def _batch_profile_figures(B):
    """Committed rocprofv3 evidence of the whole-batch k_linearize_batch launch (profiles/r*_bench_B<B>_linearize_by_grid.json: the largest grid) and its
    PMC traffic (profiles/r*_pmc_traffic_B<B>.json, whole-batch launches when the summary splits them by grid)."""
    import glob
    out = {}
    try:
        cand = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_bench_B{B}_linearize_by_grid.json")))
        if cand:
            by = json.load(open(cand[-1]))["by_workgroups"]
            k = max(by, key=lambda s: int(s))
            out["rocprofv3_us"] = by[k]["avg_us"]; out["rocprofv3_profile"] = os.path.relpath(cand[-1], ROOT); out["workgroups"] = int(k)
        cand = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_traffic_B{B}.json")))
        if cand:
            pj = json.load(open(cand[-1]))
            for kname, kv in pj["kernels"].items():
                if kname.startswith("k_linearize_batch"):
                    v = kv.get("hbm_bytes_per_launch_corrected_whole_batch", kv.get("hbm_bytes_per_launch_corrected"))
                    if v:
                        out["hbm_bytes_pmc"] = v; out["pmc_profile"] = os.path.relpath(cand[-1], ROOT)
                        out["pmc_scope"] = "whole-batch launches" if "hbm_bytes_per_launch_corrected_whole_batch" in kv else "mean over whole- and half-batch launches"
    except Exception:
        pass
    return out


def batch_parity_check(win, ba):
    """OUTSIDE the timed region (oracle = checker only), the batched counterpart of parity_check (i): the state the timed batch left in one of its
    windows is transplanted into the oracle, which re-evaluates it - the energy the GPU holds for that state must be the oracle's (1e-4 relative,
    north_star).  Raises on violation: a diverged window must not stand behind a throughput figure."""
    from oracle import pyoracle as po
    n = 8 * win.F + 4
    buf = torch.zeros(ba.gn_reduce_doubles(), dtype=torch.float64, device="cuda")
    ba.gn_reduce_local(buf.data_ptr(), 1e-1); ba.sync(); torch.cuda.synchronize()
    e_gpu = float(buf[n * n + n].item())
    res = ba.get_residuals()
    w2 = transplant(win, ba.get_frames(), ba.get_points(), res)
    o = po.OracleWindow(w2); o.collect_active(reset_oob=False)
    e_orc = o.linearize_all(False)
    ro = o.get_residuals(False)
    o.close()
    mism = int(np.sum(ro["out"]["state_NewState"] != res["state_state"]))
    rel = abs(e_gpu - e_orc) / abs(e_orc)
    # (states: informational - the oracle decides them with the thresholds of the transplanted frames, the GPU decided them one iteration earlier)
    return {"energy_gpu": e_gpu, "energy_oracle_at_that_state": e_orc, "rel": rel, "residual_states_differing": mism, "ok": bool(np.isfinite(e_gpu) and rel <= 1e-4)}


def batch_trajectory_check(win, ba):
    """OUTSIDE the timed region (oracle = checker only): the window was taken through exactly 10 forced GN iterations BY THE BATCHED LAUNCHES from its initial state;
    the oracle runs its own FullSystem::optimize loop for 10 forced iterations from the same initial state, and re-evaluates the state the batch reached - the two
    energies must agree (1e-4 relative, north_star).  batch_parity_check alone accepts ANY finite state (it asks whether the GPU's energy for a state is the oracle's
    energy for that state): a batched kernel that skipped every residual passed it in round 6 until the test suite caught it."""
    from oracle import pyoracle as po
    res = ba.get_residuals()
    w2 = transplant(win, ba.get_frames(), ba.get_points(), res)
    o = po.OracleWindow(w2); o.collect_active(reset_oob=False)
    e_state = o.linearize_all(False); o.close()
    o2 = po.OracleWindow(win); o2.set_force_all_iterations(True); o2.optimize(10)
    eo = o2.energy_log(); o2.close()
    rel = abs(e_state - eo[-1]) / abs(eo[-1])
    return {"energy_of_the_batch_state_after_10_iterations_by_the_oracle": e_state, "energy_after_the_oracle_s_own_10_iterations": float(eo[-1]), "energy_before": float(eo[0]),
            "rel": rel, "ok": bool(np.isfinite(e_state) and rel <= 1e-4)}


def batched_line(args, local_rank, Bs=(8, 32), min_timed_s=0.2):
    """Batched windows: B independent C3 windows per launch (ldso_ba_batch_*), three launches per iteration for the
    whole batch.  Aggregate GN iterations/s over the batch, the roofline of the batched k_linearize (B x the algorithmic bytes of
    one window / its launch time) and, after the clock has stopped, the oracle's verdict on the state two of the B windows were left in."""
    from ldso_amd import synth, binding
    win = synth.make_config("C3")
    synth.add_synthetic_prior(win)
    tstream = torch.cuda.Stream()
    torch.cuda.set_stream(tstream)
    out = {"workload": f"B independent, DIFFERENT C3 windows (seeds 20260925 + i: own scene, images, poses, points; {win.F} KF x {win.P} pt, R = {win.R}) per launch, forced GN iterations"}
    handles, wins, iterated = [], [], set()
    for B in Bs:
        while len(handles) < B:
            wi = win if not handles else synth.add_synthetic_prior(synth.make_config("C3", seed=20260925 + len(handles)))
            g = binding.BA.from_window(wi, device=local_rank, stream=tstream.cuda_stream)
            g.collect_active(); g.linearize_all(False); g.apply_res()
            handles.append(g); wins.append(wi)
        bt = binding.BABatch(handles[:B])
        bt.enqueue_gn(0, 10); torch.cuda.synchronize()
        # the trajectory of the batched launches against the oracle's own 10 iterations, on the windows of this batch that start from their initial state (the first and
        # the last of them); the batch is taken apart for it (handles back on their own chunking and residual sets) and formed again
        fresh = [i for i in range(B) if i not in iterated]
        traj = {}
        if fresh:
            bt.close()
            traj = {f"window_{i}": batch_trajectory_check(wins[i], handles[i]) for i in sorted({fresh[0], fresh[-1]})}
            bt = binding.BABatch(handles[:B])
        iterated.update(range(B))
        blocks, total, steps = [], 0.0, 50
        while total < min_timed_s or len(blocks) < 3:
            t0 = time.perf_counter()
            bt.enqueue_gn(2, steps)
            torch.cuda.synchronize()
            d = time.perf_counter() - t0
            blocks.append(d); total += d
        dt = float(np.median(blocks))
        lin_us = bt.time_linearize(50)
        chunk_pts = bt.chunk_points() if hasattr(bt, "chunk_points") else None
        alg = B * (436 * win.R + 112 * win.P)
        ok = bool(all(np.all(np.isfinite(h.get_frames()["frames"]["state"])) for h in handles[:B]))
        bt.close()
        # the oracle on what the timed batch left behind: the first and the last window of the batch (handles back on their own chunking)
        par = {f"window_{i}": batch_parity_check(wins[i], handles[i]) for i in sorted({0, B - 1})}
        par["tolerance"] = 1e-4
        par["first_10_iterations"] = traj
        par["ok"] = bool(all(v["ok"] for k, v in par.items() if k.startswith("window_")) and all(v["ok"] for v in traj.values()))
        prof = _batch_profile_figures(B)
        us = max(lin_us, prof.get("rocprofv3_us", 0.0))          # as for the headline: the longer of the live and the committed duration
        roof = {"bound": "hbm", "kernel": "k_linearize_batch (all B windows in one launch)", "achieved": round(alg / (us * 1e-6) / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                "frac": round(alg / (us * 1e-6) / 1e9 / 8000.0, 5), "traffic": prof.get("hbm_bytes_pmc"), "algorithmic_bytes_per_launch": alg,
                "avg_launch_us_live": round(lin_us, 3), "frac_live": round(alg / (lin_us * 1e-6) / 1e9 / 8000.0, 5), "committed": prof}
        out[f"B{B}"] = {"gn_iters_per_s_aggregate": round(B * steps / dt, 1), "ms_per_batch_iteration": round(dt / steps * 1e3, 5),
                        "mresiduals_per_s": round(B * steps * win.R / dt / 1e6, 1),
                        "k_linearize": {"avg_launch_us": round(lin_us, 3), "algorithmic_bytes_per_launch": alg, "achieved_GBps": round(alg / (lin_us * 1e-6) / 1e9, 1),
                                        "frac_of_8TBps": round(alg / (lin_us * 1e-6) / 1e9 / 8000.0, 5), "points_per_workgroup": chunk_pts},
                        "roofline": roof,
                        "state_finite": ok,
                        "parity_vs_oracle": par}
        if not par["ok"]:
            raise SystemExit(f"bench.py: batched windows (B = {B}): parity check against the oracle failed: {par}")
    for g in handles:
        g.close()
    return out


def adapter_line(name="C3"):
    """What a maintainer sees after the switch (informational): wall time of ldso::GpuBackend::optimize(6) - the compiled drop-in of
    adapter/ldso_gpu_adapter.cc - against the reference's own FullSystem::optimize(6) ON THE SAME REFERENCE OBJECT GRAPH (Frame / FrameHessian /
    PointHessian / PointFrameResidual objects built by oracle/ref_driver.cc from the reference's translation units: they are the boundary's
    types here, and the reference leg is a cpu_baseline), with the adapter's time split into flatten + upload | device | fetch | write-back.
    None where the prebuilt libraries are absent."""
    from ldso_amd import synth
    try:
        from oracle import pyref as pr
        if not (pr.available() and pr.adapter_available()):
            return None
    except Exception:
        return None
    win = synth.add_synthetic_prior(synth.make_config(name))
    out = {"workload": f"{name}: {win.F} KF x {win.P} pt, R = {win.R}; one optimize(6) call on the reference's object graph (canbreak decides the iterations executed)"}
    with _QuietCStdout():
        keep = pr.RefWindow(win)          # the reference's globals (image size, calibration: internal/GlobalCalib.h) are set by the first object graph
        A = pr.GpuAdapter(max_frames=win.F + 1, max_points=win.P + 16)
        for wb in (False, True):
            A.set_write_back_jacobians(wb)
            ts, splits, ups, its = [], [], [], 0
            for rep in range(6):
                r = pr.RefWindow(win); r.fs_attach()          # (the FullSystem object of the graph exists before the clock starts, as for the reference leg)
                t0 = time.perf_counter(); rv, its, lost = A.optimize(r, 6); ts.append(time.perf_counter() - t0); splits.append(A.last_optimize_times().copy()); ups.append(A.last_upload_times().copy())
                r.close()
            sp = np.median(np.array(splits[1:]), axis=0)
            up = np.median(np.array(ups[1:]), axis=0)
            if not wb:
                out["first_call_flatten_upload_split_ms"] = dict(zip(("settings_images", "host_walk", "set_window", "set_point_stats", "set_frames", "set_prior"), [round(float(v) * 1e3, 3) for v in up]))
            # the FIRST optimize() of a window (every rep is a new object graph: nothing of it is resident, the whole window is flattened and uploaded)
            out["first_call_full_upload_ms" if not wb else "first_call_full_upload_ms_with_jacobian_write_back"] = round(float(np.median(ts[1:])) * 1e3, 3)
            out["first_call_split_ms" if not wb else "first_call_split_ms_with_jacobian_write_back"] = {"flatten_upload": round(sp[0] * 1e3, 3), "device": round(sp[1] * 1e3, 3), "fetch": round(sp[2] * 1e3, 3),
                                                                                                        "write_back": round(sp[3] * 1e3, 3)}
            out["iterations_executed"] = its
        # the window RESIDENT between two optimize() calls (GpuBackend::residentWindow, ldso_ba_update_window): (a) a second optimize(6) on the same graph - every
        # point survives, nothing fresh: the floor of the delta path; (b) key frames in FullSystem::makeKeyFrame's order (tests/adapter_sequence_common.py: the oldest
        # frame leaves, a new one arrives with one residual per surviving point, ~10 % of the points are freshly activated) - optimize()'s wall time per key frame
        A.set_write_back_jacobians(False)
        ts2, sp2, up2 = [], [], []
        for rep in range(5):
            r = pr.RefWindow(win); r.fs_attach()
            A.optimize(r, 6)
            t0 = time.perf_counter(); A.optimize(r, 6); ts2.append(time.perf_counter() - t0); sp2.append(A.last_optimize_times().copy()); up2.append(A.last_upload_times().copy())
            r.close()
        sp = np.median(np.array(sp2[1:]), axis=0); up = np.median(np.array(up2[1:]), axis=0)
        # the adapter's figure: what optimize(6) costs from a window's second call on (the window is resident, GpuBackend::residentWindow - LDSO calls optimize() once per
        # key frame for the lifetime of the system; the full upload above happens once)
        out["gpu_backend_optimize_resident_floor_ms"] = round(float(np.median(ts2[1:])) * 1e3, 3)
        out["gpu_backend_optimize_resident_floor_ms_is"] = "a second optimize(6) on the same object graph: window resident, every point survives, nothing fresh - the floor of the delta path, never met in a key-frame sequence"
        out["gpu_backend_optimize_ms"] = out["gpu_backend_optimize_resident_floor_ms"]          # (rounds 5 and 6 report the floor under this key; resident_window.keyframe_sequence_resident.optimize_ms_median is the per-key-frame figure)
        out["gpu_backend_optimize_ms_is"] = "= gpu_backend_optimize_resident_floor_ms; first_call_full_upload_ms = flatten + upload of a whole window (the meaning of this key until round 4); resident_window.keyframe_sequence_resident.optimize_ms_median = per key frame of a makeKeyFrame sequence"
        out["split_ms"] = {"flatten_upload": round(sp[0] * 1e3, 3), "device": round(sp[1] * 1e3, 3), "fetch": round(sp[2] * 1e3, 3), "write_back": round(sp[3] * 1e3, 3)}
        out["flatten_upload_split_ms"] = dict(zip(("settings_images", "host_walk", "update_window", "set_point_stats", "set_frames", "set_prior"), [round(float(v) * 1e3, 3) for v in up]))
        out["resident_window"] = {}
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from adapter_sequence_common import run_sequence
            Kseq = 4
            wseq = synth.make_config(name, extra_frames=Kseq)
            for resident in (True, False):
                A2 = pr.GpuAdapter(max_frames=win.F + 2, max_points=2 * win.P)
                A2.set_resident_window(resident)
                times, ups = [], []
                run_sequence(wseq, Kseq, adapter=A2, max_frames=win.F, per_frame=max(120, win.P // 20), on_keyframe=lambda rec: (times.append(A2.last_optimize_times().copy()), ups.append(A2.last_upload_times().copy())))
                d_, f_ = A2.upload_counts()
                A2.close()
                tt = np.array(times[1:]); uu = np.array(ups[1:])          # the first key frame holds the handle's first (full) upload
                out["resident_window"]["keyframe_sequence_resident" if resident else "keyframe_sequence_full_upload"] = {
                    "key_frames_timed": int(len(tt)), "optimize_ms_median": round(float(np.median(tt.sum(axis=1))) * 1e3, 3),
                    "split_ms_median": dict(zip(("flatten_upload", "device", "fetch", "write_back"), [round(float(v) * 1e3, 3) for v in np.median(tt, axis=0)])),
                    "host_walk_ms_median": round(float(np.median(uu[:, 1])) * 1e3, 3), "uploads_delta_full": [d_, f_]}
        except Exception as e:          # informational leg
            out["resident_window"]["keyframe_sequence_error"] = repr(e)[:200]
        tr = []
        for rep in range(3):
            r = pr.RefWindow(win); r.fs_attach()
            t0 = time.perf_counter(); r.fs_optimize(6); tr.append(time.perf_counter() - t0)
            r.close()
        A.close(); keep.close()
    # ONE baseline for this line, the same build and threading as the headline's cpu_baseline: the reference's translation units at the reference's own
    # optimisation level (-O3, x86-64-v3) with its own 6-worker IndexThreadReduce; the -O2 single-thread pin build (what the adapter links here) beside it
    out["reference_FullSystem_optimize_pin_build_1_thread_ms"] = round(float(np.median(tr)) * 1e3, 3)
    try:
        if pr.lib_fast() is not None:
            with _QuietCStdout():
                tf = []
                for rep in range(4):
                    r = pr.RefWindow(win, fast=True); r.fs_attach(True)
                    t0 = time.perf_counter(); r.fs_optimize(6); tf.append(time.perf_counter() - t0)
                    r.close()
            out["reference_FullSystem_optimize_ms"] = round(float(np.median(tf[1:])) * 1e3, 3)
            out["reference_build"] = "reference translation units, g++ -O3 -march=x86-64-v3, the reference's own IndexThreadReduce (6 workers), Eigen = oracle/ref_shim: the build and threading of cpu_baseline"
        else:
            out["reference_FullSystem_optimize_ms"] = out["reference_FullSystem_optimize_pin_build_1_thread_ms"]
            out["reference_build"] = "reference translation units, g++ -O2, single thread (the -O3 build is not available on this host)"
    except Exception as ex:
        out["reference_FullSystem_optimize_ms"] = out["reference_FullSystem_optimize_pin_build_1_thread_ms"]
        out["reference_build"] = "pin build, single thread (" + repr(ex)[:120] + ")"
    return out


def tracker_line():
    """BASELINE configs[1] (informational): CoarseTracker::trackNewestCoarse on a 640x480 pair, 5 pyramid levels — one
    ldso_tr_track call (images resident, host round trip included) and a 20-hypothesis batch, next to the oracle on one core."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tracker_common import tracker_scenario
    from ldso_amd import synth, binding
    from oracle import pyoracle as po
    sc = tracker_scenario("C3", levels=5)
    win = sc["win"]
    a, b = sc["new_aff"]
    g = binding.Tracker(win.w, win.h, sc["levels"], win.settings, win.calib)
    o = po.OracleTracker(win.w, win.h, sc["levels"], win.settings, win.calib, fast=True)
    for t in (g, o):
        t.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"])
        t.set_new_frame(sc["new_pyr"], 1.0)

    def timeit(t, n):
        r = None
        t0 = time.perf_counter()
        for _ in range(n):
            r = t.track(np.eye(4), a, b, sc["levels"] - 1)
        return (time.perf_counter() - t0) / n, r

    timeit(g, 3)
    tg, rg = timeit(g, 50)
    ev, pcn = g.last_track_evals()
    track_bytes = int(sum(int(e) * int(n) * 64 for e, n in zip(ev, pcn)))        # pc_n * (16 B point + 48 B taps) per calcRes
    to, ro = timeit(o, 5)
    guesses = [synth.se3_exp([0.002 * i, 0, 0, 0, 0.0005 * i, 0]) for i in range(20)]
    g.track_batch(guesses, [(a, b)] * 20, sc["levels"] - 1)
    t0 = time.perf_counter()
    for _ in range(10):
        g.track_batch(guesses, [(a, b)] * 20, sc["levels"] - 1)
    tb = (time.perf_counter() - t0) / 10
    # the reference's OWN CoarseTracker::trackNewestCoarse (src/frontend/CoarseTracker.cc compiled unmodified at the reference's optimisation level,
    # oracle/_ref/libldso_ref_fast.so) on the same pair, one core: the cpu_baseline of this line (the oracle's figure stays beside it)
    ref_base = None
    try:
        from oracle import pyref as pr
        if pr.lib_fast() is not None:
            with _QuietCStdout():
                rt = pr.RefTracker(win.w, win.h, sc["levels"], win.settings, win.calib, fast=True)
                rt.set_ref(sc["ref_pyr"], sc["ref_aff"][0], sc["ref_aff"][1], 1.0, sc["pts"]); rt.set_new_frame(sc["new_pyr"], 1.0)
                timeit(rt, 1)
                tr, rr = timeit(rt, 5)
                rt.close()
            ref_base = {"value": round(tr * 1e3, 4), "unit": "ms per track", "cores": 1, "kind": "reference",
                        "sample": "5 x CoarseTracker::trackNewestCoarse of the reference's own translation units (-O3, x86-64-v3), same pair, identity initial guess",
                        "pose_vs_gpu_max_abs": float(np.abs(np.asarray(rr["T"])[:3] - np.asarray(rg["T"])[:3]).max())}
    except Exception as ex:
        ref_base = {"error": repr(ex)}
    return {"workload": f"C2: {win.w}x{win.h} pair, {sc['levels']} levels, {len(sc['pts'])} reference points",
            "cpu_baseline": ref_base,
            "gpu_track_ms": round(tg * 1e3, 4), "gpu_tracks_per_s": round(1.0 / tg, 1), "gpu_hypotheses_per_s_batch20": round(20.0 / tb, 1),
            "lm_iterations": int(rg["iterations"]), "gpu_track_batch20_ms": round(tb * 1e3, 4),
            "evaluations_per_level": [int(e) for e in ev[:sc["levels"]]], "points_per_level": [int(n) for n in pcn[:sc["levels"]]],
            "algorithmic_bytes_per_track": track_bytes, "algorithmic_GBps": round(track_bytes / tg / 1e9, 3),
            "cpu_oracle_track_ms": round(to * 1e3, 4), "cpu_cores": 1}


def tracer_line():
    """Informational: FullSystem::traceNewCoarse on 7000 fresh immature points, 640x480 - one ldso_trace_on call
    (points resident, pose upload + launch + count read-back) next to the oracle on one core."""
    from ldso_amd import synth, binding
    from oracle import pyoracle as po
    win = synth.make_config("C3", extra_frames=1)
    pts, _ = synth.make_immature_points(win, 1000)
    KRKi, Kt, aff = synth.trace_poses(win, win.F)
    img = win.images[win.F][0]
    g = binding.Tracer(win.w, win.h, len(pts))
    g.set_frame(img)
    tg = []
    for _ in range(10):
        g.set_points(pts)
        t0 = time.perf_counter(); c = g.trace_on(KRKi, Kt, aff); tg.append(time.perf_counter() - t0)
    ref = pts.copy()
    t0 = time.perf_counter(); po.trace_on(ref, img, KRKi, Kt, aff); to = time.perf_counter() - t0
    return {"workload": f"{len(pts)} fresh immature points on {win.F} key frames, {win.w}x{win.h}", "gpu_trace_on_ms": round(float(np.median(tg[2:])) * 1e3, 4),
            "cpu_oracle_ms": round(to * 1e3, 3), "cpu_cores": 1, "status_counts_good_oob_outlier": [int(c[0]), int(c[1]), int(c[2])]}


def initializer_line():
    """Informational: CoarseInitializer::trackFrame on a 640x480 sequence - one ldso_init_track_frame call per
    frame (new image upload + makeImages + the whole LM loop on the device + state read-back) next to the oracle on one core."""
    from ldso_amd import synth, binding
    from oracle import pyoracle as po
    seq = synth.make_init_sequence(640, 480, n_frames=4)
    L = seq["levels"]
    pyr0 = synth.make_images(seq["first"], L)
    pts = synth.select_init_points(pyr0)
    o = po.OracleInitializer(640, 480, L); o.set_first(seq["K4"], pyr0, 1.0, pts)
    g = binding.Initializer(640, 480, L); g.set_first(seq["K4"], seq["first"], pts)
    tg, tc, ev = [], [], []
    for k, img in enumerate(seq["frames"]):
        o.set_new_frame(synth.make_images(img, L), 1.0)
        t0 = time.perf_counter(); so = o.track_frame(); tc.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); sg = g.track_frame(img, 1.0); tg.append(time.perf_counter() - t0)
        ev.append((int(so["evals"]), int(sg["evals"])))
    dT = float(np.abs(so["thisToNext"] - sg["thisToNext"]).max())
    return {"workload": f"640x480, {L} levels, points per level {[len(p) for p in pts]}, 4 frames (snapped from the 2nd)",
            "gpu_track_frame_ms": [round(t * 1e3, 3) for t in tg], "cpu_oracle_track_frame_ms": [round(t * 1e3, 2) for t in tc], "cpu_cores": 1,
            "evaluations_cpu_gpu": ev, "max_abs_pose_diff_last_frame": dT}


def _host_cpu():
    """model name and frequency governor of the host the CPU baseline ran on (the baseline drifts 200 -> 250 it/s between boxes)"""
    model, gov = None, None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip(); break
    except OSError:
        pass
    try:
        gov = open("/sys/devices/system/cpu/cpu0/cpufreq/scaling_governor").read().strip()
    except OSError:
        pass
    return {"model": model, "governor": gov}


def cpu_baseline(win):
    """Oracle (CPU restatement of the reference) timed on the host cores: GN iterations/s on the same window.
    Per-iteration time by differencing optimize(12) - optimize(2) (removes window set-up and the final fix pass)."""
    from oracle import pyoracle as po
    fast = True
    try:
        po.build(fast=True)
    except Exception:
        fast = False

    def t_opt(n, mt):
        o = po.OracleWindow(win, multithreading=mt, fast=fast)
        o.set_force_all_iterations(True)
        t = o.time_optimize(n)
        o.close()
        return t

    res = {}
    for mt, key in ((True, "mt6"), (False, "st1")):
        d = []
        t_end = time.perf_counter() + 8.0
        while time.perf_counter() < t_end or len(d) < 3:
            d.append((t_opt(12, mt) - t_opt(2, mt)) / 10.0)
        res[key] = float(np.median(d))
    ncpu = os.cpu_count()
    port = {"value": round(1.0 / res["mt6"], 2), "unit": "GN iters/s", "cores": 6, "kind": "port",
            "sample": f"median per-iteration time of optimize(12)-optimize(2) over ~8 s, same {win.F} KF x {win.P} pt window, 6 worker threads "
                      f"(reference NUM_THREADS) on a {ncpu}-vCPU host; -O3 -march=native" if fast else "portable build",
            "single_thread_value": round(1.0 / res["st1"], 2), "host_vcpus": ncpu, "host_cpu": _host_cpu(),
            "upper_bound_of_reference": True,      # the restatement has no shared_ptr / weak_ptr.lock() graph: it is faster than the code it restates
            "window_recreated_per_sample": True}
    ref = reference_compiled_baseline(win)
    if ref is None:
        return port
    # the reference's own translation units are the baseline; the restatement's figure rides along
    ref["port"] = port
    return ref


class _QuietCStdout:
    """The reference's translation units printf() to stdout ("using pyramid levels ...", "destroyed ThreadReduce"): bench.py prints ONE JSON
    line, so file descriptor 1 points at /dev/null while they run (and C stdio is flushed on both sides of the switch)."""
    def __enter__(self):
        import ctypes
        self.libc = ctypes.CDLL(None)
        sys.stdout.flush(); self.libc.fflush(None)
        self.saved = os.dup(1)
        self.null = os.open(os.devnull, os.O_WRONLY)
        os.dup2(self.null, 1)
        return self

    def __exit__(self, *a):
        sys.stdout.flush(); self.libc.fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved); os.close(self.null)
        return False


def reference_compiled_baseline(win):
    """oracle/_ref/libldso_ref_fast.so: the reference's OWN FullSystem::optimize / EnergyFunctional / PointFrameResidual::linearize /
    IndexThreadReduce (translation units compiled unmodified, -O3 x86-64-v3) on the same window, 6 worker threads (multiThreading = true,
    NUM_THREADS = 6: the reference's default) and 1 thread.  Eigen / Sophus are the header shim of oracle/ref_shim (eager evaluation,
    no expression templates): stated in the JSON.  None where the prebuilt library is absent."""
    import copy
    try:
        from oracle import pyref as pr
        if pr.lib_fast() is None:
            return None
    except Exception:
        return None
    w = copy.deepcopy(win)
    w.settings = w.settings.copy(); w.settings["minOptIterations"] = 1000          # forced iterations: canbreak never ends the loop (FullSystem.cc:829)

    def t_opt(n, mt):
        r = pr.RefWindow(w, fast=True)
        r.fs_attach(multithreading=mt)
        t = r.fs_time_optimize(n)
        r.close()
        return t

    res = {}
    with _QuietCStdout():
        for mt, key in ((True, "mt6"), (False, "st1")):
            d = []
            t_end = time.perf_counter() + 8.0
            while time.perf_counter() < t_end or len(d) < 3:
                d.append((t_opt(12, mt) - t_opt(2, mt)) / 10.0)
            res[key] = float(np.median(d))
    return {"value": round(1.0 / res["mt6"], 2), "unit": "GN iters/s", "cores": 6, "kind": "reference",
            "sample": f"the reference's FullSystem::optimize on the same {win.F} KF x {win.P} pt window: median per-iteration time of optimize(12)-optimize(2) "
                      f"over ~8 s per mode, multiThreading = true (IndexThreadReduce, NUM_THREADS = 6) on a {os.cpu_count()}-vCPU host",
            "single_thread_value": round(1.0 / res["st1"], 2), "host_vcpus": os.cpu_count(), "host_cpu": _host_cpu(),
            "build": "reference translation units compiled unmodified, g++ -O3 -march=x86-64-v3", "eigen": "shim (oracle/ref_shim: eager evaluation, no expression templates)",
            "window_recreated_per_sample": True}


if __name__ == "__main__":
    main()
