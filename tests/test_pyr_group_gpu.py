"""ldso_pyr_group_make_images: FrameHessian::makeImages of several pyramids in at most 2 x Lmax launches.  Every level of every member holds the bytes of its own
ldso_pyr_make_images, and equals synth.make_images.  The members:
  36 x 20, 3 levels     the smallest legal shape; level 2 is 9 x 5
  100 x 52, 5 levels    widths 100, 50, 25, 12, 6: odd widths drop a column in the 2 x 2 mean; the last level (6 x 3) has one gradient row
  70 x 44, 2 levels     level 1 is 35 x 22
  320 x 240, 1 level    one level among deeper members: from level 1 on it contributes no workgroups
The images are random irradiance with a NaN patch, an Inf patch and a step of 1000 (central difference above 372 > 255: the gradient is zeroed, FrameHessian.cc:86-87)."""
import ctypes as C
import functools

import numpy as np
import pytest

from ldso_amd import binding, synth

pytestmark = pytest.mark.gpu
LDSO_OK, LDSO_E_INVALID = 0, -1
SHAPES = ((36, 20, 3), (100, 52, 5), (70, 44, 2), (320, 240, 1))


def stream():
    import torch
    ts = torch.cuda.Stream(); torch.cuda.set_stream(ts)
    return ts.cuda_stream


@functools.lru_cache(maxsize=None)
def images(seed):
    """one irradiance image per member (read-only)"""
    rng = np.random.default_rng(seed)
    out = []
    for w, h, _ in SHAPES:
        I = (255 * rng.random((h, w))).astype(np.float32)
        I[:, 3 * w // 4:] += 1000.0                                  # a step larger than 510: |dx| > 255 across it
        I[h // 4:h // 4 + 2, w // 4:w // 4 + 2] = np.nan
        I[h // 2:h // 2 + 2, w // 2 + 1:w // 2 + 3] = np.inf
        out.append(I)
    return out


def fetch(p):
    return [p.get_level(l) for l in range(p.levels)]


@functools.lru_cache(maxsize=None)
def solo_levels(seed):
    """every member's levels from its own ldso_pyr_make_images, computed once (read-only)"""
    out = []
    for (w, h, lv), I in zip(SHAPES, images(seed)):
        p = binding.Pyramid(w, h, lv).make_images(I)
        out.append(fetch(p))
        p.close()
    return out


def make_group():
    pyr = [binding.Pyramid(w, h, lv) for w, h, lv in SHAPES]
    return pyr, binding.PyramidGroup(pyr)


def close_all(grp, pyr):
    grp.close()
    for p in pyr:
        p.close()


def assert_levels(tag, p, want):
    got = fetch(p)
    assert len(got) == len(want)
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, l)


def test_every_level_equals_the_solo_build_and_the_host_restatement():
    st = stream()
    pyr, grp = make_group()
    grp.make_images(images(1), stream=st)
    for i, (p, I) in enumerate(zip(pyr, images(1))):
        assert_levels(i, p, solo_levels(1)[i])
        with np.errstate(invalid="ignore"):
            want = synth.make_images(I, p.levels)
        for l, a in enumerate(fetch(p)):
            assert np.array_equal(a, want[l], equal_nan=True), (i, l)
            assert np.isnan(a[..., 0]).any() or l > 0
            assert not np.isnan(a[..., 1:]).any() and np.abs(a[..., 1:]).max() <= 255.0, (i, l)
    # the last level of the deepest member: 6 x 3, one row of gradients
    last = pyr[1].get_level(4)
    assert last.shape == (3, 6, 3) and (last[0, :, 1:] == 0).all() and (last[2, :, 1:] == 0).all()
    close_all(grp, pyr)


def test_active_mask_overwrite_and_the_device_pointer_entry():
    import torch
    st = stream()
    pyr, grp = make_group()
    active = [True, False, True, False]
    grp.make_images([I if a else None for I, a in zip(images(1), active)], stream=st, active=active)
    for i, p in enumerate(pyr):
        if active[i]:
            assert_levels((i, "first"), p, solo_levels(1)[i])
        else:
            with pytest.raises(binding.LdsoError):          # never built: it holds no image
                p.get_level(0)
    grp.make_images(images(1), stream=st)
    # other images for two members: they are overwritten cleanly, the others keep theirs
    active = [False, True, False, True]
    grp.make_images([I if a else None for I, a in zip(images(2), active)], stream=st, active=active)
    for i, p in enumerate(pyr):
        assert_levels((i, "second"), p, solo_levels(2 if active[i] else 1)[i])
    # the same images from device memory
    dev = [torch.from_numpy(I).cuda() for I in images(2)]
    torch.cuda.current_stream().synchronize()
    grp.make_images_device([d.data_ptr() for d in dev], stream=st)
    for i, p in enumerate(pyr):
        assert_levels((i, "device"), p, solo_levels(2)[i])
    # a member on its own between group calls
    pyr[2].make_images(images(1)[2], stream=st)
    assert_levels("solo between", pyr[2], solo_levels(1)[2])
    with pytest.raises(binding.LdsoError) as e:
        grp.make_images([None] * 4, stream=st, active=[False] * 4)
    assert e.value.code == LDSO_E_INVALID and "ldso_pyr_group_make_images" in str(e.value)
    close_all(grp, pyr)


@pytest.mark.parametrize("fetch_between", (True, False))
def test_arena_grows_while_in_use_and_the_next_call_moves_to_another_stream(fetch_between):
    """the arena's reuse rule on one group of three members with two levels: call 1 has one active member, call 2 all three (128 -> 320 bytes of tables: the arena
    is replaced while it is in use), call 3 runs on another stream (ordered behind call 2, whose kernels may still read what call 3 restages).  With the levels
    fetched after every call each call's bytes are checked; without, the three calls are enqueued back to back and nothing waits on the host between them."""
    import torch
    st = stream()
    other = torch.cuda.Stream()
    want = {seed: [solo_levels(seed)[i][:2] for i in range(3)] for seed in (1, 2)}          # levels 0 and 1 do not depend on how many lie above them
    pyr = [binding.Pyramid(w, h, 2) for w, h, _ in SHAPES[:3]]
    grp = binding.PyramidGroup(pyr)
    grp.make_images([None, images(2)[1], None], stream=st, active=[False, True, False])
    if fetch_between:
        assert_levels("first call", pyr[1], want[2][1])
    grp.make_images(images(1)[:3], stream=st)
    for i, p in enumerate(pyr if fetch_between else []):
        assert_levels((i, "second call"), p, want[1][i])
    grp.make_images(images(2)[:3], stream=other.cuda_stream)
    for i, p in enumerate(pyr):
        assert_levels((i, "third call"), p, want[2][i])
    close_all(grp, pyr)


def test_refusals():
    L = binding.lib()
    pyr, grp = make_group()
    with pytest.raises(binding.LdsoError) as e:              # a pyramid in a second group
        binding.PyramidGroup([pyr[1]])
    assert e.value.code == LDSO_E_INVALID and "ldso_pyr_group_create" in str(e.value)
    with pytest.raises(binding.LdsoError):                   # the same pyramid twice
        loose = binding.Pyramid(36, 20, 1)
        binding.PyramidGroup([loose, loose])
    assert L.ldso_pyr_destroy(pyr[0].h) == LDSO_E_INVALID and "ldso_pyr_destroy" in L.ldso_last_error().decode()
    grp.make_images(images(1), stream=stream())              # the refused destroy left the member whole
    assert_levels("after refused destroy", pyr[0], solo_levels(1)[0])
    grp.close()
    assert L.ldso_pyr_destroy(pyr[0].h) == LDSO_OK           # free once the group is gone
    pyr[0].h = None
    binding.PyramidGroup([pyr[1]]).close()                   # ... and free to join another
    for p in pyr[1:] + [loose]:
        p.close()
