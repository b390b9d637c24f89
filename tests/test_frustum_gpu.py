"""ydorb_frustum_cull on the GPU equals the CPU restatement tests/frustum_ref bit for bit: the status bytes and the bit patterns of
every YdTrackView field.  The restatement predicts the level with the log formula, the kernel with the threshold table."""
import numpy as np
import pytest

import frustum_support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    views, logs, table, lists, skips = S.scene()
    return views, logs, table, lists, skips, S.ref_cull(views, logs, table, lists, skips)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        S.same_rows(g, w)
        assert g["n_in_view"] == w["n_in_view"] == int((w["status"] == 0).sum())
        assert not g["rows"][g["status"] != 0].tobytes().strip(b"\0")        # rows of entries not in view are all zero


def test_batch_of_three_views_over_one_table(scene):
    """Three views over one table of 300 points, an empty list in the middle, overlapping index lists.  First, on the restatement:
    every exit 0-6 and every level 0-7 occurs in this batch."""
    from ydorbslam_amd.frustum import frustum_cull
    views, logs, table, lists, skips, want = scene
    assert [len(a) for a in lists] == [300, 0, 150] and len(set(lists[2].tolist()) & set(lists[0].tolist())) > 100
    st = np.concatenate([w["status"] for w in want])
    lv = np.concatenate([w["rows"]["level"][w["status"] == 0] for w in want])
    assert set(st.tolist()) == set(range(7))
    assert set(lv.tolist()) == set(range(8))
    got = frustum_cull(views, table, lists, skips)
    _same(got, want)
    _same(frustum_cull(views, table, lists, skips), got)            # a second call gives the same output


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_list_lengths_around_wave_and_block_sizes(scene, m):
    """One view with a list of m entries: below, at and above a wave, and 257 = one past a 256-thread block."""
    from ydorbslam_amd.frustum import frustum_cull
    views, logs, table, lists, skips, want = scene
    ref = S.ref_cull(views[:1], logs[:1], table, [lists[0][:m]], [skips[0][:m]])
    assert np.array_equal(ref[0]["status"], want[0]["status"][:m])
    _same(frustum_cull(views[:1], table, [lists[0][:m]], [skips[0][:m]]), ref)


def test_hand_built_rows_and_release():
    """The hand-built rows as one batch of 14 one-entry views (PcZ == 0, the NaN position and dist == 0 among them); then
    ydorb_frustum_release followed by another call."""
    from ydorbslam_amd.frustum import frustum_cull, release
    views, logs, table, lists, skips, names = S.hand_batch()
    ref = S.ref_cull(views, logs, table, lists, skips)
    assert [int(r["status"][0]) for r in ref] == [S.hand_rows()[n]["status"] for n in names]
    assert np.isnan(ref[names.index("nan_position")]["rows"]["u"][0]) and ref[names.index("dist_zero")]["rows"]["level"][0] == 7
    _same(frustum_cull(views, table, lists, skips), ref)
    release()
    _same(frustum_cull(views, table, lists, skips), ref)


def test_four_level_pyramid_with_scale_factor_two(scene):
    """Another table: scale factor 2, 4 levels (three thresholds); every level 0-3 occurs."""
    from ydorbslam_amd.frustum import frustum_cull
    _, _, table, lists, skips, _ = scene
    v, lg = S.view(*S.pose(), scale_factor=2.0, n_levels=4)
    ref = S.ref_cull([v], [lg], table, lists[:1], skips[:1])
    assert set(ref[0]["rows"]["level"][ref[0]["status"] == 0].tolist()) == {0, 1, 2, 3}
    _same(frustum_cull([v], table, lists[:1], skips[:1]), ref)
