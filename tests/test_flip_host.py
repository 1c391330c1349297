"""Host side of the flip test: the numpy restatement (tests/flip_ref.py) against a literal transcription of HRNet's
flip_back + shift + average, ``ops.flip_permutation``, and the argument checks of the three new C entry points.
No GPU needed."""
import ctypes

import numpy as np
import pytest

from otpose_amd import augment, hip, ops
from tests import flip_ref as R


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("shape", [(1, 17, 6, 5), (3, 17, 9, 12), (2, 5, 4, 7)])
def test_restatement_matches_hrnet_flip_back_shift_average(shape, shift):
    b, j, h, w = shape
    rng = np.random.RandomState(b * 100 + w + shift)
    hm = rng.standard_normal((2 * b, j, h, w)).astype(np.float32)
    pairs = augment.FLIP_PAIRS if j == 17 else [[0, 3], [1, 4]]
    perm = ops.flip_permutation(pairs, j)
    got = R.flip_merge(hm, perm, shift)
    want = R.hrnet_flip_merge(hm[:b], hm[b:], pairs, shift)
    assert got.dtype == np.float32 and got.shape == (b, j, h, w)
    assert np.array_equal(got, want)
    if shift:
        assert not np.array_equal(got, R.flip_merge(hm, perm, False))


def test_flip_permutation_of_the_posetrack_pairs():
    perm = ops.flip_permutation(augment.FLIP_PAIRS, 17)
    assert perm.dtype == np.int32 and perm.shape == (17,)
    assert list(perm[:3]) == [0, 1, 2]                       # nose, head bottom, head top: unpaired
    assert perm[3] == 4 and perm[4] == 3 and perm[15] == 16 and perm[16] == 15
    assert np.array_equal(perm[perm], np.arange(17))
    assert np.array_equal(ops.flip_permutation([], 4), np.arange(4))


@pytest.mark.parametrize("pairs, j", [([[1, 17]], 17), ([[-1, 2]], 17), ([[1, 2], [2, 3]], 17), ([[5, 5]], 17),
                                      ([[1, 2, 3]], 17), ([[0, 1]], 0)])
def test_flip_permutation_rejects_non_involutions_and_out_of_range_joints(pairs, j):
    with pytest.raises(ValueError):
        ops.flip_permutation(pairs, j)


def _perm(values):
    return (ctypes.c_int * len(values))(*values)


def test_new_entry_points_return_error_codes_without_a_gpu():
    L = hip.lib()
    fake = ctypes.c_void_p(0x1000)                 # never dereferenced: every call below fails its host-side checks
    ok = _perm(list(ops.flip_permutation(augment.FLIP_PAIRS, 17)))
    # null pointers
    assert L.otp_crop_clips_pair_u8(None, 1, 8, 8, None, None, None, 1, 5, 8, 8, 0., 0., 0., 1., 1., 1., None) == -1
    assert L.otp_crop_clips_pair_u8(fake, 1, 8, 8, fake, fake, None, 1, 5, 8, 8, 0., 0., 0., 1., 1., 1., None) == -1
    assert L.otp_clip_mirror_pair(None, fake, 1, 3, 4, 4, None) == -1
    assert L.otp_clip_mirror_pair(fake, None, 1, 3, 4, 4, None) == -1
    assert L.otp_heatmap_flip_decode(None, ok, fake, fake, fake, None, None, 1, 17, 4, 4, 0, None) == -1
    assert L.otp_heatmap_flip_decode(fake, None, fake, fake, fake, None, None, 1, 17, 4, 4, 0, None) == -1
    assert L.otp_heatmap_flip_decode(fake, ok, None, fake, fake, None, None, 1, 17, 4, 4, 0, None) == -1
    # bad shapes / arguments
    assert L.otp_crop_clips_pair_u8(fake, 1, 8, 8, fake, fake, fake, 0, 5, 8, 8, 0., 0., 0., 1., 1., 1., None) == -1
    assert L.otp_crop_clips_pair_u8(fake, 1, 8, 8, fake, fake, fake, 1, 5, 8, 8, 0., 0., 0., 0., 1., 1., None) == -2
    assert L.otp_crop_clips_pair_u8(fake, 1, 8, 8, fake, fake, fake, 70000, 5, 8, 8, 0., 0., 0., 1., 1., 1., None) == -2
    assert L.otp_clip_mirror_pair(fake, fake, 1, 3, 0, 4, None) == -1
    assert L.otp_clip_mirror_pair(fake, fake, 1 << 14, 15, 384, 288, None) == -2         # 2 B C H W >= 2^31
    assert L.otp_heatmap_flip_decode(fake, ok, fake, fake, fake, None, None, 0, 17, 4, 4, 0, None) == -1
    assert L.otp_heatmap_flip_decode(fake, ok, fake, fake, fake, fake, None, 1, 17, 4, 4, 0, None) == -1
    assert L.otp_heatmap_flip_decode(fake, _perm(range(300)), fake, fake, fake, None, None, 1, 300, 4, 4, 0, None) == -2
    # perm: not an involution / a joint out of range
    bad = list(range(17))
    bad[3], bad[4], bad[5] = 4, 5, 3
    assert L.otp_heatmap_flip_decode(fake, _perm(bad), fake, fake, fake, None, None, 1, 17, 4, 4, 0, None) == -1
    out = list(range(17))
    out[16] = 17
    assert L.otp_heatmap_flip_decode(fake, _perm(out), fake, fake, fake, None, None, 1, 17, 4, 4, 0, None) == -1
    neg = list(range(17))
    neg[0] = -1
    assert L.otp_heatmap_flip_decode(fake, _perm(neg), fake, fake, fake, None, None, 1, 17, 4, 4, 1, None) == -1
