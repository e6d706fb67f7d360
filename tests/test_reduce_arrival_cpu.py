"""Host logic of the hand-over inside the fused reduce + control-step launch (no device): the reduce workgroups of k_reduce_solve arrive on a fixed number of
words, workgroup q on word ldso_ba_arrival_shard(q), and the control workgroup waits on word s for ldso_ba_arrival_targets(total)[s] arrivals.  Both exports
are the functions the kernel compiles (ba_dev.h: arrive_shard, arrive_target); nothing here restates the rule, the targets are checked against a count of the
shards the library itself names.  A target that is too large would leave the control workgroup waiting (until its bounded poll gives up), one that is too small
would let it read the system before the last sums are in."""
import numpy as np

from ldso_amd import binding

TOTALS = range(0, 301)


def test_targets_sum_to_the_arrivers():
    for total in TOTALS:
        t = binding.arrival_targets(total)
        assert 1 <= len(t) <= 64
        assert (t >= 0).all(), (total, t)
        assert int(t.sum()) == total, (total, t)


def test_targets_are_the_count_of_the_workgroups_on_each_word():
    shards = len(binding.arrival_targets(0))
    shard = np.array([binding.arrival_shard(q) for q in range(max(TOTALS))])
    assert ((shard >= 0) & (shard < shards)).all()
    for total in TOTALS:
        count = np.bincount(shard[:total], minlength=shards)
        assert (binding.arrival_targets(total) == count).all(), total


def test_fewer_arrivers_than_words():
    shards = len(binding.arrival_targets(0))
    assert (binding.arrival_targets(0) == 0).all()
    for total in range(1, shards):
        t = binding.arrival_targets(total)
        assert (t >= 0).all() and (t <= 1).all() and int((t == 0).sum()) == shards - total, (total, t)


def test_bad_arguments_are_refused():
    for call in (lambda: binding.arrival_targets(-1), lambda: binding.arrival_shard(-1)):
        try:
            call()
        except binding.LdsoError:
            continue
        raise AssertionError("a negative count was accepted")
