"""ydorb_search_local_points (frustum test, query build on the device and projection search in one call) equals its definition, the
composition ydorb_frustum_cull -> host query build -> ydorb_search_by_projection(mode 0), and the composition equals the CPU
restatement followed by the matcher oracle."""
import numpy as np
import pytest

import frustum_support as S

pytestmark = pytest.mark.gpu
TH, RATIO = 3.0, 0.8


@pytest.fixture(scope="module")
def scenario():
    s = S.local_map()
    return s, S.ref_search_local_points(s, TH, RATIO)


@pytest.fixture(scope="module")
def matcher():
    import ydorbslam_amd as y
    m = y.OrbMatcher(RATIO, check_orientation=False)
    yield m
    m.close()


def _frame(s):
    import ydorbslam_amd as y
    return y.FrameView(s["kps"], s["desc"], S.BOUNDS, s["right_x"])


def _same(got, want):
    assert got["n_to_match"] == want["n_to_match"] and got["n_matches"] == want["n_matches"]
    assert np.array_equal(got["assigned"], want["assigned"]) and np.array_equal(got["taken"], want["taken"])
    S.same_rows(got, want)


def test_reference_side_preconditions(scenario):
    """On the restatement + oracle only: enough matches, an in-view point left unmatched, a skip-flagged point that would be in view,
    and a keypoint wanted by two queries."""
    from oracle.orb_oracle import FrameOracle
    s, want = scenario
    assert len(s["kps"]) == 500 and s["table"].n == 300
    assert want["n_matches"] >= 50 and want["n_to_match"] > want["n_matches"]
    matched = set(want["assigned"][want["assigned"] >= 0].tolist())
    in_view = set(np.nonzero(want["status"] == 0)[0].tolist())
    assert matched <= in_view and in_view - matched
    unflagged = S.ref_search_local_points(s, TH, RATIO, skip=np.zeros_like(s["skip"]))
    assert np.any((s["skip"] != 0) & (unflagged["status"] == 0)) and np.all(want["status"][s["skip"] != 0] == 1)
    fo = FrameOracle(s["kps"], s["desc"], S.BOUNDS, s["right_x"])
    wanted = {}
    for i in sorted(in_view):                                   # each query alone: the keypoint it would take without competition
        q = np.zeros_like(want["queries"])
        q[i] = want["queries"][i]
        _, a, _ = fo.search_by_projection(0, q, s["table"].desc, RATIO, False, s["taken"], None)
        for kp in np.nonzero(a >= 0)[0]:
            wanted.setdefault(int(kp), []).append(i)
    assert any(len(v) >= 2 for v in wanted.values())


def test_fused_equals_composition_equals_reference(scenario, matcher):
    from ydorbslam_amd.frustum import search_local_points
    s, want = scenario
    f = _frame(s)
    composed = S.search_local_points_composed(matcher, f, s["view"], s["table"], s["skip"], s["has_obs"], TH, s["taken"])
    _same(composed, want)
    fused = search_local_points(matcher, f, s["view"], s["table"], s["skip"], s["has_obs"], TH, s["taken"])
    _same(fused, composed)


def test_no_point_in_view_leaves_assigned_untouched(scenario, matcher):
    from ydorbslam_amd.frustum import search_local_points
    s, _ = scenario
    skip = np.ones_like(s["skip"])
    before = np.arange(len(s["kps"]), dtype=np.int32) - 7
    got = search_local_points(matcher, _frame(s), s["view"], s["table"], skip, s["has_obs"], TH, s["taken"], before)
    assert got["n_to_match"] == 0 and got["n_matches"] == 0
    assert np.array_equal(got["assigned"], before) and np.array_equal(got["taken"], s["taken"])
    assert np.all(got["status"] == 1) and not got["rows"].tobytes().strip(b"\0")


def test_two_calls_of_different_sizes_on_one_handle(scenario, matcher):
    """A smaller local map after a larger one, then the larger one again: rows left in the handle's query buffer must not be read."""
    from ydorbslam_amd.frustum import PointTable, search_local_points
    s, want = scenario
    t, k = s["table"], 97
    small = dict(s, table=PointTable(t.pos_min[:k, :3], t.normal_max[:k, :3], t.pos_min[:k, 3], t.normal_max[:k, 3], t.max_distance[:k], t.desc[:k]),
                 skip=s["skip"][:k], has_obs=s["has_obs"][:k])
    want_small = S.ref_search_local_points(small, TH, RATIO)
    f = _frame(s)
    _same(search_local_points(matcher, f, s["view"], s["table"], s["skip"], s["has_obs"], TH, s["taken"]), want)
    _same(search_local_points(matcher, f, small["view"], small["table"], small["skip"], small["has_obs"], TH, s["taken"]), want_small)
    _same(search_local_points(matcher, f, s["view"], s["table"], s["skip"], s["has_obs"], TH, s["taken"]), want)
