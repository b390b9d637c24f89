"""ydorb_triangulate_matches on the GPU equals the CPU restatement tests/triangulate_ref bit for bit: the bit patterns of x3d and the
status bytes, for rejected matches too."""
import numpy as np
import pytest

import triangulate_support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    views, problems = S.scene()
    return views, problems, S.ref_triangulate(views, problems)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g["status"], w["status"])
        assert np.array_equal(g["x3d"].view(np.uint32), w["x3d"].view(np.uint32))
        assert g["n_accepted"] == w["n_accepted"] == int(((w["status"] & 15) == 0).sum())


def test_batch_of_four_problems_over_three_views(scene):
    """Four problems over three shared keyframes with an empty one in the middle, about 200 matches each.  First, on the restatement:
    every exit 0-8 and every source occurs in this batch."""
    from ydorbslam_amd.triangulate import triangulate_matches
    views, problems, want = scene
    assert [len(p["idx1"]) for p in problems] == [203, 0, 198, 211]
    st = np.concatenate([w["status"] for w in want])
    assert set((st & 15).tolist()) >= set(range(9))
    assert set(((st >> 4) & 3).tolist()) == {0, 1, 2, 3}
    got = triangulate_matches(views, problems)
    _same(got, want)
    _same(triangulate_matches(views, problems), got)            # a second call gives the same output


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_match_counts_around_wave_and_block_sizes(scene, m):
    """One problem of m matches: below, at and above a wave, and 257 = one past a 256-thread block."""
    from ydorbslam_amd.triangulate import triangulate_matches
    views, problems, want = scene
    i1 = np.concatenate([problems[0]["idx1"], problems[0]["idx1"][::-1]])[:m]
    i2 = np.concatenate([problems[0]["idx2"], problems[0]["idx2"][::-1]])[:m]
    prob = [dict(first=0, second=1, idx1=i1, idx2=i2)]
    ref = S.ref_triangulate(views, prob)
    if 0 < m <= 203:
        assert np.array_equal(ref[0]["status"], want[0]["status"][:m])
    _same(triangulate_matches(views, prob), ref)


def test_explicit_rows_and_release():
    """The hand-built cases as one batch of 13 problems over 26 views: exit 9, the accepted NaN point (bit 7) and every other exit; then
    ydorb_triangulate_release followed by another call."""
    from ydorbslam_amd.triangulate import release, triangulate_matches
    views, problems, want = S.explicit_rows()
    ref = S.ref_triangulate(views, problems)
    assert [int(r["status"][0]) for r in ref] == want
    assert 0x29 in want and 0xA0 in want
    _same(triangulate_matches(views, problems), ref)
    release()
    _same(triangulate_matches(views, problems), ref)
