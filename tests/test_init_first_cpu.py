"""Host-only parts of the initialiser's first frame (no device): the recursion of makePixelStatus (ldso_init_pixel_status_plan) against its recorded decisions, and
the k-d tree of makeNN - built by ldso_init_nn_build, searched by ldso_init_nn_search_host - against the LDSO sources' own makeNN on the recorded setFirst
levels and on synthetic position sets (tests/golden/ref_init_first.npz, scripts/golden/make_ref_init_first.py).  Indices and squared distances are compared
exactly: the same index in the same place, rows with equally distant candidates included."""
import numpy as np
import pytest

import init_first_common as ic
from ldso_amd import binding

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_plan_grid_matches_the_recorded_decisions():
    g = ic.golden()
    pi, pf, po = g["plan_in"], g["plan_f"], g["plan_out"]
    seen = 0
    for (n_good, sp, rec), (desired, thf), (act, sp_after) in zip(pi, pf, po):
        a, s, t = binding.init_pixel_status_plan(int(n_good), float(desired), int(sp), int(rec), float(thf))
        assert s == sp_after, (n_good, sp, rec, desired, thf, s, sp_after)
        if act >= 0:
            assert a == act, (n_good, sp, rec, desired, thf, a, act)
            seen += 1
        assert t == (0.5 if (s == 1 and sp == 1) else thf)
    assert seen > 400


def test_plan_grid_covers_what_it_must():
    g = ic.golden()
    pi, pf, po = g["plan_in"], g["plan_f"], g["plan_out"]
    assert set(np.unique(pi[:, 1])) == {1, 2, 5, 12} and set(np.unique(pi[:, 2])) == {0, 1, 5} and set(np.unique(pf[:, 1])) == {f32(0.5), f32(1.0)}
    assert (pi[:, 0] == 0).any()
    assert ((po[:, 0] == 1) & (pi[:, 1] == 1) & (po[:, 1] == 1)).any()          # recursion with both sparsities 1: only the THFac = 0.5 branch gets there
    # one float step either side of quotia = 0.8 and 1 / quotia = 0.8: neighbouring densities with different, visible decisions
    q = pi[:, 0].astype(f32) / pf[:, 0]
    flips = 0
    rows = {}
    for i in range(len(pi)):
        if pi[i, 2] > 0:
            rows.setdefault((*pi[i].tolist(), float(pf[i, 1])), []).append((pf[i, 0], int(po[i, 0])))
    for r in rows.values():
        r.sort()
        flips += sum(b[0] == np.nextafter(a[0], f32(1e9)) and a[1] >= 0 and b[1] >= 0 and a[1] != b[1] for a, b in zip(r, r[1:]))
    assert flips >= 2, flips
    assert np.isfinite(q[pi[:, 0] > 0]).all()


NN = None


def nn_inputs():
    global NN
    if NN is None:
        NN = ic.nn_inputs()
    return NN


def test_the_large_frame_is_deeper_than_every_other_input():
    depth = {name: max(binding.NNTree(a).depth for a in uv) for name, (uv, _) in nn_inputs().items()}
    large = depth.pop("first/large_scene")
    assert max(depth.values()) == ic.LARGE_MIN_DEPTH - 1 and large >= ic.LARGE_MIN_DEPTH, (large, depth)
    r = ic.load_frame("large_scene", ic.GOLDEN_LARGE)
    assert (r["w"], r["h"], r["levels"], r["sparsity_in"]) == (384, 320, 4, 5) and r["lv"][0]["xy"].dtype == np.uint16
    assert all(int((lv["xy"][:, 0] >= 256).sum()) > 0 for lv in r["lv"][:1]) and int(r["lv"][0]["xy"][:, 1].max()) >= 256


@pytest.mark.parametrize("name", ["first/" + n for n, _ in ic.FRAMES + ic.FRAMES_LARGE] + ["nn/" + n for n in ic.NN_SETS])
def test_tree_and_host_search_equal_the_reference(name):
    uv, ref = nn_inputs()[name]
    trees = [binding.NNTree(a) for a in uv]
    for l, a in enumerate(uv):
        idx, d = trees[l].search(a, 10)
        assert np.array_equal(idx, ref[l]["nb"].astype(np.int32)), (name, l, int((idx != ref[l]["nb"]).any(1).sum()))
        assert np.array_equal(bits(d), bits(ref[l]["d10"]))
        if l + 1 < len(uv):
            pidx, pd = trees[l + 1].search(ic.parent_query(a), 1)
            assert np.array_equal(pidx[:, 0], ref[l]["par"].astype(np.int32)) and np.array_equal(bits(pd[:, 0]), bits(ref[l]["d1"]))
        else:
            assert np.all(ref[l]["par"] == -1)
    for t in trees:
        t.close()


def test_tree_arrays_are_a_tree_over_a_permutation():
    uv = ic.pos(ic.nn_set("grid")[0])
    t = binding.NNTree(uv)
    nodes, vind = t.arrays()
    assert sorted(vind.tolist()) == list(range(len(uv)))
    leaves = nodes[nodes["child1"] < 0]
    assert np.all(leaves["right"] - leaves["left_or_feat"] <= 5) and int((leaves["right"] - leaves["left_or_feat"]).sum()) == len(uv)
    inner = nodes[nodes["child1"] >= 0]
    assert len(inner) == len(leaves) - 1 and np.all(inner["divlow"] <= inner["divhigh"]) and 0 < t.depth <= 64
    assert np.array_equal(t.root_box, np.array([uv[:, 0].min(), uv[:, 0].max(), uv[:, 1].min(), uv[:, 1].max()], f32))


def test_fixture_tells_the_reference_order_from_the_tidy_one():
    uv, ref = nn_inputs()["nn/grid"]
    ti, td = ic.tidy_order(uv[0])
    assert ic.tie_share(td[:, 9], td[:, 10]) >= 0.5
    differ = 0
    for name in ic.NN_SETS:
        u, r = nn_inputs()["nn/" + name]
        for l, a in enumerate(u):
            if len(a) > 10:
                differ += int((ic.tidy_order(a)[0][:, :10] != r[l]["nb"]).any(1).sum())
    assert differ > 0


def test_one_span_zero_and_query_outside_the_root_box():
    row = ic.pos(ic.nn_set("row")[0])
    assert np.all(row[:, 1] == row[0, 1])
    lo, up = (ic.pos(a) for a in ic.nn_set("parent_outside"))
    q = ic.parent_query(lo)
    outside = (q[:, 0] < up[:, 0].min()) | (q[:, 0] > up[:, 0].max()) | (q[:, 1] < up[:, 1].min()) | (q[:, 1] > up[:, 1].max())
    assert outside.mean() > 0.5


def test_search_refuses_other_result_sizes_and_bad_positions():
    t = binding.NNTree(ic.pos(ic.nn_set("n11")[0]))
    with pytest.raises(binding.LdsoError) as e:
        t.search(np.zeros((1, 2), f32), 3)
    assert e.value.code == -4
    with pytest.raises(binding.LdsoError):
        binding.NNTree(np.array([[0.0, np.nan]], f32))
