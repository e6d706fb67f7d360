"""What it costs to turn every window of a batch into the next one between two key frames, timed on an MI355X at B = 8 and B = 32 different C3 windows (7 key frames x
2000 points, 640 x 480: the windows of bench.py's batched line, seeds 20260925 + i, each with the synthetic prior) in the steady-state edit: the oldest frame leaves
with its points, a new one arrives in its image slot, every surviving point gets a residual towards it, and as many fresh points as left arrive, hosted by the
second-newest frame.  With seven frames that replaces a seventh of the window per round (286 of 2000 points; two sevenths every seventh round, when the frame that
took the first round's fresh points leaves) - a window that keeps its size cannot replace fewer while whole frames leave; the JSON line reports the mean.
  sequential   ldso_ba_batch_destroy, then per handle ldso_ba_update_window + ldso_ba_set_frames + ldso_ba_set_prior, then ldso_ba_batch_create: the only route
               there was before the batched entries (a balanced batch refuses members that were re-chunked behind its back)
  batched      ONE ldso_ba_batch_update_windows + ONE ldso_ba_batch_set_frames on the live batch
The legs alternate round by round on two sets of handles that hold the same windows and receive the same deltas (built before the clock starts, passed through the C
entries), every leg ends in a stream synchronisation, and the median of `--reps` rounds after `--warmup` is reported with the 10th / 90th percentile, one JSON line
per batch size.  No optimize() runs between the rounds, so no window holds an applied linearisation: the re-linearisation launch that ldso_ba_batch_destroy and
ldso_ba_batch_create each add per window in a real key-frame loop is NOT in the sequential leg (it reads lower here than it would there).  The first round checks
that the two sets end as the same bytes.  Nothing is asserted about time.  Each batch size runs as a child process of its own under `timeout`; the second does not
start when the first failed.  For the per-kernel split run one batch size under `rocprofv3 --kernel-trace --stats` (k_win_rebuild_batch, k_win_scatter_batch,
k_point_stats_batch, k_solve_batch); what remains of the batched leg is its host side (validation, staging, chunk policy, upload, launches, waits).
    python scripts/time_batch_update_window.py [--reps 50] [--warmup 5] [--batch 8|32]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_TIMEOUT_S = 560
SEED0 = 20260925


def stats(t):
    t = np.asarray(t) * 1e6
    return dict(median_us=round(float(np.median(t)), 1), p10_us=round(float(np.percentile(t, 10)), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def make_c3(seed):
    from ldso_amd import synth
    return synth.add_synthetic_prior(synth.make_config("C3", seed=seed))


class Book:
    """host-side picture of one window across the rounds: host frame and residual mask of every point, the image slot of every frame"""

    def __init__(self, win, seed):
        self.win, self.F, self.rng = win, win.F, np.random.default_rng(seed)
        self.host = win.points["host"].astype(np.int32).copy()
        self.mask = np.zeros(win.P, np.uint32)
        np.bitwise_or.at(self.mask, win.residuals["point"], (1 << win.residuals["target"]).astype(np.uint32))
        self.slots = np.arange(self.F, dtype=np.int32)

    def next_delta(self):
        """the steady-state edit as the arguments of ldso_ba_update_window; the book moves on to the new window"""
        from ldso_amd import synth
        F, P = self.F, len(self.host)
        stay = np.nonzero(self.host != 0)[0]
        n_fresh = P - len(stay)
        new_host = F - 2                                                   # the frame that was the newest: where DSO activates most of its points
        frame_from = np.concatenate([np.arange(1, F), [-1]]).astype(np.int32)
        slots = np.concatenate([self.slots[1:], self.slots[:1]]).astype(np.int32)
        mask_stay = ((self.mask[stay] >> 1) | np.uint32(1 << (F - 1))).astype(np.uint32)          # the oldest frame's bit drops out, insertResidual towards the new frame
        mask_fresh = np.uint32(((1 << F) - 1) & ~(1 << new_host))
        point_from = np.concatenate([stay, -1 - np.arange(n_fresh)]).astype(np.int32)          # fresh points behind every survivor: frame F - 1 hosts nothing yet
        res_mask = np.concatenate([mask_stay, np.full(n_fresh, mask_fresh, np.uint32)])
        fresh = self.win.points[self.rng.integers(0, self.win.P, n_fresh)].copy()
        fresh["host"] = new_host
        targets = np.array([t for t in range(F) if t != new_host], np.int32)
        fresh_res = np.zeros(n_fresh * len(targets), synth.RESIDUAL_DTYPE)
        fresh_res["point"] = np.repeat(np.arange(n_fresh), len(targets)); fresh_res["host"] = new_host; fresh_res["target"] = np.tile(targets, n_fresh); fresh_res["is_new"] = 1
        self.host = np.concatenate([self.host[stay] - 1, np.full(n_fresh, new_host, np.int32)]).astype(np.int32)
        self.mask, self.slots = res_mask, slots
        assert (np.diff(self.host) >= 0).all()
        return dict(slots=slots, frame_from=frame_from, point_from=point_from, res_mask=res_mask, fresh=fresh, fresh_res=fresh_res,
                    mrb=np.zeros(n_fresh, np.float32), ngr=np.zeros(n_fresh, np.int32))


def run(a):
    B = a.batch
    # the windows first, on a few cores, before anything opens the device
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=min(8, B)) as ex:
        wins = list(ex.map(make_c3, [SEED0 + i for i in range(B)]))
    import torch
    from ldso_amd import binding
    from ldso_amd.binding import _p
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    sets = [[binding.BA.from_window(w, stream=ts.cuda_stream) for w in wins] for _ in range(2)]          # [0]: the sequential leg's handles, [1]: the batched leg's
    L = binding.lib()
    books = [Book(w, SEED0 + 100 + i) for i, w in enumerate(wins)]
    arr = [(C.c_void_p * B)(*[g.h for g in hs]) for hs in sets]
    bt = [C.c_void_p(), C.c_void_p()]
    for k in range(2):
        assert L.ldso_ba_batch_create(arr[k], C.c_int(B), C.byref(bt[k])) == 0, L.ldso_last_error()
    frames = [np.ascontiguousarray(w.frames) for w in wins]
    calibs = [np.ascontiguousarray(w.calib) for w in wins]
    HMs, bMs = [np.ascontiguousarray(w.HM, np.float64) for w in wins], [np.ascontiguousarray(w.bM, np.float64) for w in wins]
    FJ = (binding.FramesJob * B)()
    for i in range(B):
        FJ[i].frames, FJ[i].calib, FJ[i].HM, FJ[i].bM = frames[i].ctypes.data, calibs[i].ctypes.data, HMs[i].ctypes.data, bMs[i].ctypes.data

    def sequential(deltas):
        rc = L.ldso_ba_batch_destroy(bt[0])
        for i, (g, d) in enumerate(zip(sets[0], deltas)):
            rc = rc or L.ldso_ba_update_window(g.h, C.c_int(len(d["slots"])), _p(d["slots"]), _p(d["frame_from"]), C.c_int(len(d["point_from"])), _p(d["point_from"]), _p(d["res_mask"]),
                                               C.c_int(len(d["fresh"])), _p(d["fresh"]), C.c_int(len(d["fresh_res"])), _p(d["fresh_res"]), _p(d["mrb"]), _p(d["ngr"]))
            rc = rc or L.ldso_ba_set_frames(g.h, _p(frames[i]), _p(calibs[i]))
            rc = rc or L.ldso_ba_set_prior(g.h, _p(HMs[i]), _p(bMs[i]))
        rc = rc or L.ldso_ba_batch_create(arr[0], C.c_int(B), C.byref(bt[0]))
        return rc or L.ldso_ba_sync(sets[0][0].h)

    t_seq, t_bat, t_upd, replaced = [], [], [], []
    for it in range(a.warmup + a.reps):
        deltas = [b.next_delta() for b in books]
        replaced.append(np.mean([len(d["fresh"]) for d in deltas]))
        WJ = (binding.WinJob * B)()
        for i, d in enumerate(deltas):
            j = WJ[i]
            j.F, j.image_slot, j.frame_from, j.P, j.point_from, j.res_mask = len(d["slots"]), d["slots"].ctypes.data, d["frame_from"].ctypes.data, len(d["point_from"]), d["point_from"].ctypes.data, d["res_mask"].ctypes.data
            j.n_fresh, j.fresh, j.n_fresh_res, j.fresh_res, j.fresh_mrb, j.fresh_ngr = len(d["fresh"]), d["fresh"].ctypes.data, len(d["fresh_res"]), d["fresh_res"].ctypes.data, d["mrb"].ctypes.data, d["ngr"].ctypes.data
        t0 = time.perf_counter()
        rc = sequential(deltas)
        t1 = time.perf_counter()
        assert rc == 0, (rc, L.ldso_last_error())
        t2 = time.perf_counter()
        rc = L.ldso_ba_batch_update_windows(bt[1], WJ)
        t3 = time.perf_counter()
        rc = rc or L.ldso_ba_batch_set_frames(bt[1], FJ)
        t4 = time.perf_counter()
        assert rc == 0, (rc, L.ldso_last_error())
        t_seq.append(t1 - t0); t_bat.append(t4 - t2); t_upd.append(t3 - t2)
        if it == 0:
            for gs, gb in zip(sets[0], sets[1]):
                gs._sync_dims(); gb._sync_dims()
                ps, pb = gs.get_points(), gb.get_points()
                assert (gs.F, gs.P, gs.R) == (gb.F, gb.P, gb.R) and ps.tobytes() == pb.tobytes() and gs.get_residuals()["state_state"].tobytes() == gb.get_residuals()["state_state"].tobytes() \
                    and gs.get_chunk_cuts().tobytes() == gb.get_chunk_cuts().tobytes(), "the legs disagree: nothing to time"
    w = a.warmup
    bal = C.c_int()
    L.ldso_ba_batch_balanced(bt[1], C.byref(bal))
    print(json.dumps(dict(step="batch_update_window", B=B, window="C3 %d KF x %d pt" % (wins[0].F, wins[0].P), replaced_per_window=round(float(np.mean(replaced[w:])), 1), reps=a.reps,
                          balanced=int(bal.value), sequential_with_batch_recreation=stats(t_seq[w:]), batched=stats(t_bat[w:]),
                          batched_update_windows_alone=stats(t_upd[w:]), ratio_of_medians=round(float(np.median(t_seq[w:]) / np.median(t_bat[w:])), 2))), flush=True)
    for k in range(2):
        L.ldso_ba_batch_destroy(bt[k])
    for hs in sets:
        for g in hs:
            g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, choices=(8, 32))
    a = ap.parse_args()
    if a.batch:
        run(a)
        return 0
    for B in (8, 32):
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--batch", str(B), "--reps", str(a.reps), "--warmup", str(a.warmup)]).returncode
        if rc != 0:
            print(f"B = {B} ended with status {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
