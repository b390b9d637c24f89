"""optimizeEssentialGraphImpl (include/ydorb/optimizer.hpp) EXECUTED on the GPU (tests/cpp_host/essgraph_run.cpp on stand-ins of KeyFrame /
MapPoint / Map that carry data): vertex compaction over a bad keyframe, the three edge groups in the reference's order with the
inserted-pair rule, Tiw = [R | t / s] and the corrected points, against a replay of the rules here and the ctypes path on the same graph."""
import os
import subprocess

import numpy as np
import pytest

import essgraph_support as S
from essgraph_support import ROOT

pytestmark = pytest.mark.gpu
SRC = os.path.join(ROOT, "tests", "cpp_host", "essgraph_run.cpp")
IDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
BAD = {4}
LOOP_KF, CUR_KF = 0, 9
PARENT = {1: 0, 2: 1, 3: 2, 4: 3, 5: 3, 6: 5, 7: 6, 8: 7, 9: 8}
# (a, b, weight) by falling weight.  (9, 0) is below minFeat and enters only as the current / loop pair; (9, 1) and (8, 0) are below it and
# do not; (8, 1) enters as a loop connection, so the covisibility pass must not insert it again; (6, 2) is an earlier loop edge and is not
# repeated as a covisible; (5, 0) is too weak; (7, 5) and (8, 2) are plain covisibility edges; (5, 4) leads to the bad keyframe.
COVIS = [(1, 0, 200), (2, 1, 190), (3, 2, 180), (5, 3, 170), (6, 5, 160), (7, 6, 150), (8, 7, 140), (9, 8, 135), (8, 2, 130), (7, 5, 120),
         (5, 4, 115), (8, 1, 110), (6, 2, 105), (5, 0, 50), (9, 1, 30), (8, 0, 20), (9, 0, 10)]
LOOP_EDGES = [(6, 2)]
CONNECTIONS = {8: [1, 0], 9: [0, 1]}


def _build(tmp):
    exe = os.path.join(tmp, "essgraph_run")
    lib_dir = os.path.join(ROOT, "ydorbslam_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpu_harness", "mockrt"),
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + lib_dir, "-l:libydorb.so", "-Wl,-rpath," + lib_dir])
    return exe


def _rotation(q):
    """Eigen's Quaternion::toRotationMatrix in its operation order"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _scenario():
    rng = np.random.default_rng(5)
    g = S.make_graph(len(IDS), [(0, 1)], 77, True, drift=0.01)
    poses = {}
    for k, i in enumerate(IDS):   # the keyframes' float poses: the drifted estimates
        poses[i] = (_rotation(g["sim3"][k][:4]).astype(np.float32), g["sim3"][k][4:7].astype(np.float32))
    as_sim3 = lambda k: np.concatenate([g["sim3"][k][:7], [1.0]])
    non_corrected = {8: as_sim3(8), 9: as_sim3(9)}
    corrected = {8: np.concatenate([g["truth"][8][:7], [1.0]]), 9: np.concatenate([g["truth"][9][:7], [1.0]])}
    n_mp = 40
    mp = dict(pos=rng.uniform(-6, 6, (n_mp, 3)).astype(np.float32), bad=(rng.uniform(size=n_mp) < 0.1).astype(np.int32),
              ref=rng.choice(IDS, n_mp).astype(np.int32), by=np.full(n_mp, -1, np.int32), cref=np.full(n_mp, -1, np.int32))
    mp["ref"][:3] = [0, 4, 9]          # the fixed keyframe, the bad one (no vertex: the point stays), the current one
    mp["bad"][:3] = 0
    mp["by"][3:6], mp["cref"][3:6], mp["bad"][3:6] = CUR_KF, [8, 9, 2], 0   # corrected in correctLoop: mnCorrectedReference decides
    return dict(poses=poses, non_corrected=non_corrected, corrected=corrected, mp=mp)


def _blob(sc):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    b = [i32(len(IDS))]
    for i in IDS:
        R, t = sc["poses"][i]
        b += [i32(i, int(i in BAD), PARENT.get(i, -1)), R.tobytes(), t.tobytes()]
    b.append(i32(len(COVIS)))
    b += [i32(*c) for c in COVIS]
    b.append(i32(len(LOOP_EDGES)))
    b += [i32(*e) for e in LOOP_EDGES]
    for m in (sc["corrected"], sc["non_corrected"]):
        b.append(i32(len(m)))
        for i in sorted(m):
            b += [i32(i), np.asarray(m[i], np.float64).tobytes()]
    b.append(i32(len(CONNECTIONS)))
    for i in CONNECTIONS:
        b += [i32(i, len(CONNECTIONS[i])), i32(*CONNECTIONS[i])]
    mp = sc["mp"]
    b.append(i32(len(mp["pos"])))
    for k in range(len(mp["pos"])):
        b += [mp["pos"][k].tobytes(), i32(mp["bad"][k], mp["ref"][k], mp["by"][k], mp["cref"][k])]
    b.append(i32(LOOP_KF, CUR_KF, 1))
    return b"".join(b)


def _expected_edges():
    """The reference's three groups over keyframe ids: (vertex(0) id, vertex(1) id, group)."""
    weight = {}
    for a, b, w in COVIS:
        weight[(a, b)] = weight[(b, a)] = w
    good = [i for i in IDS if i not in BAD]
    edges, inserted = [], set()
    for i in sorted(CONNECTIONS):   # the stand-ins are allocated in id order, so the map's pointer order is the id order
        for j in sorted(CONNECTIONS[i]):
            if (i != CUR_KF or j != LOOP_KF) and weight.get((i, j), 0) < 100:
                continue
            edges.append((i, j, "loop"))
            inserted.add((min(i, j), max(i, j)))
    children = {i: {c for c, p in PARENT.items() if p == i} for i in IDS}
    loop_of = {i: {b if a == i else a for a, b in LOOP_EDGES if i in (a, b)} for i in IDS}
    for i in good:
        p = PARENT.get(i)
        if p is not None and p not in BAD:
            edges.append((i, p, "tree"))
        for l in sorted(loop_of[i]):
            if l < i:
                edges.append((i, l, "earlier"))
        for a, b, w in COVIS:   # by falling weight, as getCovisiblesByWeight returns them
            if w < 100 or i not in (a, b):
                continue
            n = b if a == i else a
            if n == p or n in children[i] or n in loop_of[i] or n in BAD or n >= i or (min(i, n), max(i, n)) in inserted:
                continue
            edges.append((i, n, "covisible"))
    return edges


def test_adapter_builds_the_reference_graph_and_writes_back(tmp_path):
    from ydorbslam_amd.essential_graph import optimize_essential_graph
    sc = _scenario()
    exe = _build(str(tmp_path))
    scen, out = str(tmp_path / "scenario.bin"), str(tmp_path / "out.bin")
    open(scen, "wb").write(_blob(sc))
    subprocess.check_call([exe, scen, out], timeout=120)
    raw = open(out, "rb").read()
    off = [0]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, off[0]).copy()
        off[0] += a.nbytes
        return a

    V = int(take(np.int32, 1)[0])
    vert_ids = take(np.int32, V).tolist()
    sim3, fixed = take(np.float64, 8 * V).reshape(V, 8), take(np.uint8, V)
    E = int(take(np.int32, 1)[0])
    v0, v1, meas = take(np.int32, E), take(np.int32, E), take(np.float64, 8 * E).reshape(E, 8)
    # vertices: the good keyframes in the map's order, mnId compacted over the gap, the loop keyframe fixed
    assert vert_ids == [i for i in IDS if i not in BAD] and V == 9
    assert fixed.tolist() == [1 if i == LOOP_KF else 0 for i in vert_ids]
    for v, i in enumerate(vert_ids):
        if i in sc["corrected"]:
            assert np.array_equal(sim3[v], sc["corrected"][i])
        else:   # (Rcw, tcw, 1): the float pose in double
            R, t = sc["poses"][i]
            assert sim3[v][7] == 1.0 and np.array_equal(sim3[v][4:7], t.astype(np.float64))
            assert np.abs(_rotation(sim3[v][:4]) - R).max() < 1e-6
    # edges: the three groups in order, the weak loop connections and the pair inserted as a loop connection left out
    want = _expected_edges()
    vertex = {i: v for v, i in enumerate(vert_ids)}
    assert [(int(a), int(b)) for a, b in zip(v0, v1)] == [(vertex[i], vertex[j]) for i, j, _ in want]
    groups = [g for _, _, g in want]
    assert groups.count("loop") == 2 and groups.count("earlier") == 1 and groups.count("covisible") == 2 and groups.count("tree") == 8
    assert (9, 0, "loop") in want and (8, 1, "loop") in want and (8, 1, "covisible") not in want and (6, 2, "covisible") not in want
    for e, (i, j, group) in enumerate(want):   # Sji = Sjw * Swi, Swi from the non-corrected pose outside the loop group
        Siw = sim3[vertex[i]] if group == "loop" else sc["non_corrected"].get(i, sim3[vertex[i]])
        Sjw = sim3[vertex[j]] if group == "loop" else sc["non_corrected"].get(j, sim3[vertex[j]])
        assert np.array_equal(meas[e], S.compose(Sjw, S.inverse(Siw))), (e, i, j, group)
    # the call, replayed through ctypes on the dumped graph and the points the adapter must gather
    mp = sc["mp"]
    ref_id = np.where(mp["by"] == CUR_KF, mp["cref"], mp["ref"])
    gathered = [k for k in range(len(ref_id)) if not mp["bad"][k] and int(ref_id[k]) in vertex]
    got = optimize_essential_graph(sim3, fixed, np.stack([v0, v1], axis=1), meas, mp["pos"][gathered], [vertex[int(ref_id[k])] for k in gathered],
                                   fix_scale=True)
    for k, i in enumerate(IDS):
        written = int(take(np.int32, 1)[0])
        T = take(np.float32, 16).reshape(4, 4)
        assert written == (0 if i in BAD else 1)
        if i in BAD:
            continue
        s = got["sim3"][vertex[i]]
        want_T = np.eye(4, dtype=np.float32)
        want_T[:3, :3] = _rotation(s[:4]).astype(np.float32)
        want_T[:3, 3] = (s[4:7] * (1.0 / s[7])).astype(np.float32)
        assert np.array_equal(T, want_T), i
    moved = 0
    for k in range(len(ref_id)):
        n_set, n_upd = take(np.int32, 2)
        pos = take(np.float32, 3)
        if k in gathered:
            assert n_set == 1 and n_upd == 1 and np.array_equal(pos, got["points"][gathered.index(k)])
            moved += int(np.abs(pos - mp["pos"][k]).max() > 1e-4)
        else:
            assert n_set == 0 and n_upd == 0 and np.array_equal(pos, mp["pos"][k])
    assert 1 not in gathered and 0 in gathered and moved > 10   # the bad keyframe's point stays; drifted keyframes' points move
    assert np.array_equal(got["points"][gathered.index(0)], mp["pos"][0])   # the fixed keyframe's point comes back as it went
    assert off[0] == len(raw)
