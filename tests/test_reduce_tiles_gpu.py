"""The Schur tile workgroups of the reduction in atomic mode (reduce_body, "Part B, atomic mode"): every wavefront loads its matrix-core operands straight
from the lifted rows G, a batch of 256 rows at a time, instead of going through an LDS slab.  The fp32 partial tiles must stay what the staging kernel
formed - same k-steps on the same accumulator in the same order - so only the arrival order of the fp64 atomics separates the two.

Every case: a 320 x 240 window with the synthetic prior, collect_active -> linearize_all -> apply_res, then ONE ldso_ba_gn_reduce_local (the stand-alone
k_reduce) into a zeroed buffer: lower triangle of HFinal | bFinal.  Two yardsticks, neither of them the code under test:
  (a) tests/golden/reduce_tiles_parent.npz, recorded on an MI355X with the library of the commit before this kernel (scripts/golden/make_reduce_tiles_parent.py):
      the system of the staging kernel and `spread`, the largest entrywise difference among 20 repetitions of it (the order of its atomics).  The partial
      tiles being bit-identical, the kernel under test may differ from the record by 4 x spread: two runs' worth of atomic order, doubled for the small sample.
  (b) the oracle's HFinal / bFinal of the same state.  The file also holds the staging kernel's own largest deviation from it - H in units of
      sqrt(H_ii H_jj), b in units of sqrt(H_ii) times the largest |b_k| / sqrt(H_kk) - and the kernel under test gets 1.5 x that: the figure is fp32
      accumulation error, the margin covers the run-to-run order of the atomics on it.
The sharded case (points 101..399: pBegin no multiple of 4) is compared with the record as the shard's own contribution, and with the oracle as the sum of
the two shards 0..100 and 101..399.

Cases (rows = points per K-split, rounded up to a multiple of 4):
  F5 P400 ks8    52 rows: three full k-steps per wavefront pair and a tail of 4        F5 P400 ks16   28 rows
  F5 P400 ks1    400 rows: a second batch of 256                                      F5 P600 ks1    three batches, across the former 512-row slab
  F5 P20 ks8     4 rows per split, splits 5..7 empty                                  F5 P6 ks8      a split of 2 rows: masked rows
  F2 P64 ks8     slots behind F                                                       F8 P64 ks8     all eight slots live
  F9 P64 ks8     FS = 16: 45 tiles                                                    F5 P400 ks8 shard 101..400
"""
import functools
import os

import numpy as np
import pytest

from ldso_amd import binding, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reduce_tiles_parent.npz")
LAMBDA = 1e-1
# name, F, P, K-splits per tile, shard (None: the whole window)
CASES = [
    ("F5_P400_ks8", 5, 400, 8, None),
    ("F5_P400_ks16", 5, 400, 16, None),
    ("F5_P400_ks1", 5, 400, 1, None),
    ("F5_P600_ks1", 5, 600, 1, None),
    ("F5_P20_ks8", 5, 20, 8, None),
    ("F5_P6_ks8", 5, 6, 8, None),
    ("F2_P64_ks8", 2, 64, 8, None),
    ("F8_P64_ks8", 8, 64, 8, None),
    ("F9_P64_ks8", 9, 64, 8, None),
    ("F5_P400_ks8_shard101", 5, 400, 8, (101, 400)),
]


@functools.lru_cache(maxsize=None)
def make_win(F, P):
    return synth.add_synthetic_prior(synth.make_config("small", F=F, P=P))


def reduce_runs(win, splits, shard, reps):
    """`reps` times one ldso_ba_gn_reduce_local of the applied state -> [(lower triangle of HFinal, bFinal)].  The handle initialises a buffer when it is
    lent another one than before, so the repetitions alternate between two."""
    import torch
    g = binding.BA.from_window(win)
    g.set_reduce_splits(splits)
    if shard is not None:
        g.set_shard(*shard)
    g.collect_active(); g.linearize_all(False); g.apply_res()
    n = 8 * win.F + 4
    bufs = [torch.zeros(g.gn_reduce_doubles(), dtype=torch.float64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    out = []
    for k in range(reps):
        b = bufs[k & 1]
        b.zero_(); torch.cuda.synchronize()
        g.gn_reduce_local(b.data_ptr(), LAMBDA); g.sync(); torch.cuda.synchronize()
        host = b.cpu().numpy()
        out.append((np.tril(host[:n * n].reshape(n, n)).copy(), host[n * n:n * n + n].copy()))
    g.close()
    return out


def oracle_system(win):
    from oracle import pyoracle as po
    o = po.OracleWindow(win)
    o.collect_active(); o.linearize_all(False); o.apply_res(); o.backup_state(); o.solve_system(0, LAMBDA)
    s = o.get_system()
    o.close()
    return np.tril(s["HFinal"]), s["bFinal"].copy()


def oracle_deviation(H, b, Ho, bo):
    """largest deviation of (H, b) from the oracle's (Ho, bo): H in units of sqrt(H_ii H_jj), b in units of sqrt(H_ii) max_k |b_k| / sqrt(H_kk)"""
    d = np.sqrt(np.diag(Ho))
    assert np.isfinite(d).all() and (d > 0).all()
    dev_h = float((np.abs(H - Ho) / np.outer(d, d)).max())
    dev_b = float((np.abs(b - bo) / d).max() / (np.abs(bo) / d).max())
    return dev_h, dev_b


def run_case(F, P, splits, shard, reps=1):
    """-> the runs of the case, and per run the system that stands against the oracle's (a shard: with the complementary shard's contribution)"""
    win = make_win(F, P)
    runs = reduce_runs(win, splits, shard, reps)
    if shard is None:
        return win, runs, runs
    assert shard[1] == win.P
    rest = reduce_runs(win, splits, (0, shard[0]), 1)[0]
    return win, runs, [(h + rest[0], b + rest[1]) for h, b in runs]


@pytest.mark.parametrize("name,F,P,splits,shard", CASES, ids=[c[0] for c in CASES])
def test_reduce_tiles_against_the_staging_kernel_and_the_oracle(name, F, P, splits, shard):
    gold = np.load(GOLDEN)
    win, runs, whole = run_case(F, P, splits, shard)
    (H, b), (Hw, bw) = runs[0], whole[0]
    assert np.isfinite(H).all() and np.isfinite(b).all()
    # (a) the staging kernel's record
    spread = float(gold[name + "__spread"])
    diff = max(float(np.abs(H - gold[name + "__H"]).max()), float(np.abs(b - gold[name + "__b"]).max()))
    print(f"{name}: against the record {diff:.3e}, spread of the record {spread:.3e} (allowed {4 * spread:.3e})")
    # (b) the oracle
    dev_h, dev_b = oracle_deviation(Hw, bw, *oracle_system(win))
    ph, pb = float(gold[name + "__oracle_dev_H"]), float(gold[name + "__oracle_dev_b"])
    print(f"{name}: against the oracle H {dev_h:.3e} (record {ph:.3e}, allowed {1.5 * ph:.3e}), b {dev_b:.3e} (record {pb:.3e}, allowed {1.5 * pb:.3e})")
    assert diff <= 4 * spread
    assert dev_h <= 1.5 * ph and dev_b <= 1.5 * pb
