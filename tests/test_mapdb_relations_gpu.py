"""All parts of the resident map table moving in the same sync on one handle (ydorbslam_amd/csrc/map_resident.hip): the point table,
the attribute table and the four span relations (keyframe rows, point views, descriptor blocks, keyframe features) are staged together
in every round and applied by one export, on a handle created so small that every one of them grows and repacks on the way.  After
every round all six exports are compared byte for byte with a plain Python model of what was staged; at the end the stats must show
that every span relation went through a kept and a grown repack and the row headers through a growth.

The rounds, in elements of the row / block / feature pools (the view pool holds two int32 per view and follows the same pattern):
  1  6 points with attributes (both tables 4 -> 8), keyframes 0-2 with spans of 5, points 0-2 with 3 views each
  2  keyframe 1's spans replaced by 20 elements, point 1's views by 12
  3, 4  the same slots again, fresh content of the same length
  5  keyframes 3 and 4 with spans of 5
  6  clear(), then round 1 again
Under span_pool.h's rule (repack when used + incoming > cap; keep the capacity when survivors + incoming <= cap / 2, else grow to twice
that sum) a pool of capacity 8 goes: 15 > 8, grown to 30; 15 + 20 > 30 and 10 + 20 > 15, grown to 60 with two survivors moved; 30 + 20
<= 60, no repack; 50 + 20 > 60 and 10 + 20 <= 30, kept; 30 + 10 <= 60.  The feature pool starts at 1 and does the same from round 1
on.  Round 5 names a fifth keyframe slot: the headers grow with three live spans to copy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
I32, U8, F32 = np.int32, np.uint8, np.float32


class Model:
    """What was staged, per slot; the last value wins."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.points, self.centres, self.rows, self.blocks, self.feats, self.views, self.attrs = {}, {}, {}, {}, {}, {}, {}

    @property
    def n_points(self):
        return 1 + max(self.points) if self.points else 0

    @property
    def n_keyframes(self):
        named = list(self.centres) + list(self.rows) + list(self.blocks) + list(self.feats) + [k for p in self.points.values() for k in p["observers"]]
        return 1 + max(named) if named else 0


def _stage(db, model, rng, kps_dtype, points=(), keyframes=(), span=0, view_points=(), n_views=0):
    """Stages fresh content for the named point slots (table and attributes), keyframe slots (centre, row, block, features of `span`
    elements) and the views of view_points, on the handle and in the model alike."""
    points, keyframes, view_points = list(points), list(keyframes), list(view_points)
    if keyframes:
        centre = rng.uniform(-4, 4, (len(keyframes), 3)).astype(F32)
        db.set_centres(keyframes, centre)
        model.centres.update(zip(keyframes, centre))
    n_kf = max(model.n_keyframes, 1)
    if points:
        rec = [dict(observers=rng.choice(n_kf, min(2, n_kf), replace=False).astype(I32), levels=rng.integers(0, 8, min(2, n_kf)).astype(U8), bad=0,
                    ref_kf=int(rng.integers(0, n_kf)), ref_level=int(rng.integers(0, 8)), pos=rng.uniform(-6, 6, 3).astype(F32)) for _ in points]
        db.set_points(points, [r["observers"] for r in rec], [r["levels"] for r in rec], [r["bad"] for r in rec], [r["ref_kf"] for r in rec],
                      [r["ref_level"] for r in rec], np.stack([r["pos"] for r in rec]))
        model.points.update(zip(points, rec))
        att = [dict(normal=rng.uniform(-1, 1, 3).astype(F32), min_distance=F32(rng.uniform(0.1, 1)), max_distance=F32(rng.uniform(5, 50)),
                    desc=rng.integers(0, 256, 32).astype(U8), flags=3) for _ in points]
        db.set_point_attributes(points, np.stack([a["normal"] for a in att]), [a["min_distance"] for a in att], [a["max_distance"] for a in att],
                                np.stack([a["desc"] for a in att]))
        model.attrs.update(zip(points, att))
    if keyframes:
        rows = [rng.integers(-1, model.n_points, span).astype(I32) for _ in keyframes]
        blocks = [rng.integers(0, 256, (span, 32)).astype(U8) for _ in keyframes]
        feats = []
        for _ in keyframes:
            kps = np.zeros(span, kps_dtype)
            for name in ("x", "y", "size", "angle", "response"):
                kps[name] = rng.uniform(0, 640, span).astype(F32)
            kps["octave"], kps["class_id"] = rng.integers(0, 8, span), rng.integers(-1, 100, span)
            feats.append((kps, rng.uniform(-1, 640, span).astype(F32)))
        db.set_keyframe_rows(keyframes, rows)
        db.set_keyframe_descriptors(keyframes, blocks)
        db.set_keyframe_features(keyframes, [f[0] for f in feats], [f[1] for f in feats])
        model.rows.update(zip(keyframes, rows)); model.blocks.update(zip(keyframes, blocks)); model.feats.update(zip(keyframes, feats))
    if view_points:
        views = [np.stack([rng.integers(0, model.n_keyframes, n_views), rng.integers(0, 1000, n_views)], axis=1).astype(I32) for _ in view_points]
        db.set_point_views(view_points, views)
        model.views.update(zip(view_points, views))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_exports_equal_model(db, model, kps_dtype, tag):
    n, k = model.n_points, model.n_keyframes
    got = db.export()                                                           # the one export that triggers the sync of everything staged
    assert got["table"].n_points == n and got["table"].n_keyframes == k, tag
    point = [model.points.get(p) for p in range(n)]                             # every slot below n was staged in these rounds
    obs_start = np.concatenate([[0], np.cumsum([len(p["observers"]) for p in point])]).astype(I32)
    assert _same(got["table"].obs_start, obs_start), tag
    assert _same(got["table"].obs_kf, np.concatenate([p["observers"] for p in point])), tag
    assert _same(got["table"].obs_level, np.concatenate([p["levels"] for p in point])), tag
    assert _same(got["table"].bad, np.array([p["bad"] for p in point], U8)), tag
    assert _same(got["ref_kf"], np.array([p["ref_kf"] for p in point], I32)) and _same(got["ref_level"], np.array([p["ref_level"] for p in point], U8)), tag
    assert _same(got["pos"], np.stack([p["pos"] for p in point])), tag
    assert _same(got["centre"], np.stack([model.centres.get(s, np.zeros(3, F32)) for s in range(k)])), tag
    rows, blocks, feats, views, attrs = db.export_rows(), db.export_descriptors(), db.export_features(), db.export_views(), db.export_attributes()
    assert len(rows) == len(blocks) == len(feats) == k and len(views) == n, tag
    for s in range(k):
        assert _same(rows[s], model.rows.get(s, np.zeros(0, I32))), (tag, "row", s)
        assert _same(blocks[s], model.blocks.get(s, np.zeros((0, 32), U8))), (tag, "block", s)
        kps, rx = model.feats.get(s, (np.zeros(0, kps_dtype), np.zeros(0, F32)))
        assert _same(feats[s][0], kps) and _same(feats[s][1], rx), (tag, "features", s)
    for p in range(n):
        assert _same(views[p], model.views.get(p, np.zeros((0, 2), I32))), (tag, "views", p)
    att = [model.attrs[p] for p in range(n)]
    assert _same(attrs["normal"], np.stack([a["normal"] for a in att])) and _same(attrs["desc"], np.stack([a["desc"] for a in att])), tag
    assert _same(attrs["min_distance"], np.array([a["min_distance"] for a in att], F32)), tag
    assert _same(attrs["max_distance"], np.array([a["max_distance"] for a in att], F32)), tag
    assert _same(attrs["flags"], np.array([a["flags"] for a in att], U8)), tag


def test_every_relation_grows_and_repacks_in_the_same_syncs():
    from ydorbslam_amd import MapDb
    from ydorbslam_amd.extractor import KP_DTYPE
    db = MapDb(0, 4, 2, 8)
    db.reserve_descriptors(4, 8)
    db.enable_attributes()
    db.enable_features()
    model, rng = Model(), np.random.default_rng(7)
    rounds = [dict(points=range(6), keyframes=[0, 1, 2], span=5, view_points=[0, 1, 2], n_views=3),
              dict(points=[1], keyframes=[1], span=20, view_points=[1], n_views=12),
              dict(points=[1], keyframes=[1], span=20, view_points=[1], n_views=12),
              dict(points=[1], keyframes=[1], span=20, view_points=[1], n_views=12),
              dict(points=[1], keyframes=[3, 4], span=5, view_points=[], n_views=0)]
    for r, what in enumerate(rounds, 1):
        _stage(db, model, rng, KP_DTYPE, **what)
        _assert_exports_equal_model(db, model, KP_DTYPE, "round %d" % r)
    assert db.stats()["point_capacity"] == 8 and db.attr_stats()["capacity"] == 8   # both SoA tables grew 4 -> 8 in round 1
    db.clear()
    model.clear()
    _stage(db, model, rng, KP_DTYPE, **rounds[0])
    _assert_exports_equal_model(db, model, KP_DTYPE, "round 6")
    rows, desc, feat = db.row_stats(), db.desc_stats(), db.feat_stats()
    for name, kept, grown in (("rows", rows["repacks_kept"], rows["repacks_grown"]), ("views", desc["view_repacks_kept"], desc["view_repacks_grown"]),
                              ("blocks", desc["desc_repacks_kept"], desc["desc_repacks_grown"]), ("features", feat["repacks_kept"], feat["repacks_grown"])):
        assert kept >= 1 and grown >= 1, (name, kept, grown)
    assert rows["header_growths"] >= 1
    db.close()
