"""Synthetic matching scenes shared by the oracle (CPU) tests and the GPU parity tests."""
import numpy as np

from ydorbslam_amd.synth import synth_frame

QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("r", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                        ("ur", "<f4"), ("rs", "<f4"), ("angle", "<f4"), ("level", "<i4"), ("flags", "<i4")])


def shifted_pair(w, h, idx, dx, dy):
    """Two views of one synthetic scene: B is A moved by (dx, dy) px plus fresh sensor noise."""
    big = synth_frame(w + 32, h + 32, idx)
    rng = np.random.default_rng(7000 + idx)
    a = big[16:16 + h, 16:16 + w]
    b = big[16 - dy:16 - dy + h, 16 - dx:16 - dx + w].astype(np.int16) + rng.integers(-2, 3, (h, w))
    return np.ascontiguousarray(a), np.clip(b, 0, 255).astype(np.uint8)


def projection_queries(kps_a, scale_factors, dx, dy, th, mode, seed, stereo=False):
    """Queries as the adapter would build them from frame A's keypoints (orbMatcher.cpp:30-31, 94-101, 182-183)."""
    rng = np.random.default_rng(seed)
    n = len(kps_a)
    q = np.zeros(n, QUERY_DTYPE)
    q["u"] = (kps_a["x"] + np.float32(dx) + rng.normal(0, 1.5, n)).astype(np.float32)
    q["v"] = (kps_a["y"] + np.float32(dy) + rng.normal(0, 1.5, n)).astype(np.float32)
    oct_ = kps_a["octave"]
    sf = scale_factors[oct_]
    if mode == 0:  # radius = th * (2.5 | 4.0), window radius*sf[level], levels (level-1, level)
        fac = np.where(rng.random(n) > 0.5, np.float32(2.5), np.float32(4.0))
        rad = (np.float32(th) * fac).astype(np.float32)
        q["r"] = (rad * sf).astype(np.float32)
        q["min_level"] = oct_ - 1
        q["max_level"] = oct_
    else:
        q["r"] = (np.float32(th) * sf).astype(np.float32)
        sel = rng.integers(0, 3, n) if mode == 1 else np.full(n, 2)
        q["min_level"] = np.where(sel == 0, oct_, np.where(sel == 1, 0, oct_ - 1))
        q["max_level"] = np.where(sel == 0, -1, np.where(sel == 1, oct_, oct_ + 1))
    q["rs"] = q["r"]
    q["ur"] = q["u"] - np.float32(20.0) if stereo else 0
    q["angle"] = kps_a["angle"]
    q["level"] = oct_
    valid = rng.random(n) > 0.1
    obs = rng.random(n) > 0.2
    q["flags"] = valid.astype(np.int32) | (obs.astype(np.int32) << 1)
    return q


def bow_nodes(desc, bits=5):
    """Stand-in for DBoW3's vocabulary (the blob is absent): node id from the leading descriptor bits."""
    return (desc[:, 0].astype(np.uint32) >> (8 - bits)) * 7 + 3  # non-contiguous ascending ids


def feature_vector(nodes):
    ids = np.unique(nodes)
    order = np.argsort(nodes, kind="stable").astype(np.int32)
    counts = np.array([(nodes == i).sum() for i in ids], np.int64)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return ids.astype(np.uint32), start, order


# ---------------------------------------------------------------------------------------------------------------------------------
# Planted contention for the resolve step of the projection searches.  The product decides the queries 64 at a time (one per lane, in
# windows of 512 queries of which those with candidates are "live") and must notice every case in which a query's outcome depends on a
# query before it.  These builders put such cases into a natural query set on purpose and say, from the serial oracle's output alone,
# how often each really happened.  Used by tests/test_oracle_matcher.py (CPU: the seeds meet the counts) and tests/test_matcher_gpu.py.
# ---------------------------------------------------------------------------------------------------------------------------------
RESOLVE_WINDOW, RESOLVE_GROUP = 512, 64          # queries staged at a time / live queries decided per step (match_kernels.hip.h)
PLANTED_PER_KIND = 36
KINDS = {0: ("observed", "unobserved", "distant", "second", "pretaken"), 1: ("observed", "unobserved", "distant", "pretaken"),
         2: ("observed", "distant", "pretaken"), 7: ("observed", "distant", "pretaken"), 6: ("observed", "distant")}


def natural_queries(s, mode, seed, th=None):
    """The query sets the existing parity tests use for `mode` on scene entry s (6 and 7: explicit level window, no level rule in the
    window search), plus keypoint-derived queries (mode "kp": what the device-resident pair search builds from frame A's keypoints)."""
    ka, sf = s["ka"], s["sf"].astype(np.float32)
    if mode == "kp":
        q = np.zeros(len(ka), QUERY_DTYPE)
        q["u"], q["v"] = ka["x"], ka["y"]
        q["r"] = (np.float32(15.0) * sf[ka["octave"]]).astype(np.float32)
        q["min_level"], q["max_level"] = ka["octave"] - 1, ka["octave"] + 1
        q["angle"], q["level"] = ka["angle"], ka["octave"]
        q["flags"] = np.where((q["u"] >= 0) & (q["u"] < s["w"]) & (q["v"] >= 0) & (q["v"] < s["h"]), 3, 0)
        return q
    if mode in (6, 7):
        rng = np.random.default_rng(seed + 1)
        q = projection_queries(ka, s["sf"], s["dx"], s["dy"], 4.0 if th is None else th, 1, seed=seed)
        q["min_level"], q["max_level"] = -1, -1
        q["level"] = np.clip(ka["octave"] + rng.integers(-1, 2, len(q)), 0, 7)
        q["r"] = (np.float32(4.0 if th is None else th) * sf[q["level"]]).astype(np.float32)
        return q
    return projection_queries(ka, s["sf"], s["dx"], s["dy"], 15 if th is None else th, mode, seed=seed)


def _popcount_rows(a, b):
    return int(np.unpackbits(a ^ b).sum())


def plant_contention(fo, s, mode, q0, d0, seed, ratio=0.9, kinds=None, with_taken=True):
    """Insert planted queries into the natural set (q0, d0) for a search of `mode` in frame s["kb"] (fo: its FrameOracle).

    A planted query takes the window of a natural query and the descriptor of one keypoint X among that window's candidates, so X is
    its best keypoint at distance 0.  Kinds:
      observed    the query and a copy right behind it, observed flag set: the copy must lose X
      unobserved  the same with the flag clear (modes 0, 1): nothing is taken and the copy must own assigned[X]
      distant     the copy 2..9 natural queries later
      second      (mode 0) a query between X and Y - best X, second Y, rejected by the ratio test - behind a query with Y's
                  descriptor: with Y gone its second-best moves away and the ratio test passes
      pretaken    X is taken before the call
    Planted pairs are placed inside a 64-lane group of live queries, and a few on purpose across a group edge, using the candidate
    lists of the oracle's window search as the estimate of which queries are live.
    Returns dict(q, d, taken0, assigned0, planted=[dict(kind, first, second, X, Y, same_group, observed)])."""
    rng = np.random.default_rng(seed)
    kb, db = s["kb"], s["db"]
    level_family = mode in (6, 7)
    kinds = KINDS[mode] if kinds is None else kinds
    taken0 = (rng.random(len(kb)) < 0.1).astype(np.uint8) if with_taken else np.zeros(len(kb), np.uint8)

    def candidates(row):
        if not (row["flags"] & 1):
            return np.zeros(0, np.int32)
        idx = fo.keypoints_in_area(np.float32(row["u"]), np.float32(row["v"]), np.float32(row["r"]), int(row["min_level"]), int(row["max_level"]))
        if level_family:
            idx = idx[(kb["octave"][idx] >= row["level"] - 1) & (kb["octave"][idx] <= row["level"])]
        return idx

    cand = [candidates(q0[i]) for i in range(len(q0))]
    used = set()
    free = lambda i: [int(x) for x in cand[i] if not taken0[x] and int(x) not in used]
    bases = [int(i) for i in rng.permutation(len(q0))]
    jobs = []
    for kind in kinds:
        made = 0
        while made < PLANTED_PER_KIND and bases:
            b = bases.pop()
            f = free(b)
            if len(f) < (3 if kind == "second" else 1 if kind == "pretaken" or level_family else 2):   # (the level family's windows are small)
                continue
            job = dict(kind=kind, base=b, Y=-1, gap=0, observed=True)
            if kind == "second":
                pick = None
                for X in f:
                    for Y in f:
                        D = _popcount_rows(db[X], db[Y])
                        k = int(np.floor(ratio * D / (1.0 + ratio))) + 1
                        if X != Y and kb["octave"][X] == kb["octave"][Y] and D >= 40 and k < D - k and k <= 90 and np.float32(k) > np.float32(ratio) * np.float32(D - k):
                            pick = (X, Y, k)
                            break
                    if pick:
                        break
                if not pick:
                    continue
                X, Y, k = pick
                bits_x, bits_y = np.unpackbits(db[X]), np.unpackbits(db[Y])
                differ = np.flatnonzero(bits_x != bits_y)
                bits = bits_x.copy()
                bits[differ[:k]] = bits_y[differ[:k]]                      # k of the differing bits taken from Y: distance k to X, D - k to Y
                job.update(X=X, Y=Y, desc=np.packbits(bits), first_desc=db[Y].copy(), gap=int(rng.integers(0, 4)), observed=bool(made % 3 != 2))
                used.update((X, Y))
            else:
                X = f[int(rng.integers(0, len(f)))]
                job.update(X=X, desc=db[X].copy(), first_desc=db[X].copy(), observed=kind != "unobserved")
                if kind == "distant":
                    job["gap"] = int(rng.integers(2, 10))
                if kind == "pretaken":
                    taken0[X] = 1
                used.add(X)
            jobs.append(job)
            made += 1
        assert made == PLANTED_PER_KIND, (mode, kind, made)
    assigned0 = np.where(taken0 > 0, 100000 + np.arange(len(taken0)), -1).astype(np.int32)
    order = [jobs[i] for i in rng.permutation(len(jobs))]
    straddlers = [j for k in kinds if k != "pretaken" for j in [x for x in order if x["kind"] == k][:4]]   # four of each kind go across a group edge
    straddlers = [straddlers[i] for i in rng.permutation(len(straddlers))]
    inside = [j for j in order if not any(j is x for x in straddlers)]

    out_q, out_d, where, planted = [], [], [], []
    state = dict(live=0)

    def emit(row, desc, is_live):
        if len(out_q) % RESOLVE_WINDOW == 0:
            state["live"] = 0
        out_q.append(row)
        out_d.append(desc)
        where.append((len(out_q) // RESOLVE_WINDOW, state["live"] // RESOLVE_GROUP))
        state["live"] += int(is_live)
        return len(out_q) - 1

    def planted_row(job, observed):
        row = q0[job["base"]].copy()
        row["flags"] = 3 if observed else 1
        return row

    pending = None                                   # (natural queries still to pass, job, index of its first query)
    for i in range(len(q0)):
        if pending is None:
            lane, room = state["live"] % RESOLVE_GROUP, RESOLVE_WINDOW - len(out_q) % RESOLVE_WINDOW
            job = None
            if straddlers and room > 16 and ((straddlers[0]["gap"] == 0 and lane == RESOLVE_GROUP - 1) or
                                             (straddlers[0]["gap"] > 0 and lane >= RESOLVE_GROUP - 2)):
                job = straddlers.pop(0)
            elif inside and room > 16 and 2 <= lane <= RESOLVE_GROUP - 16 and rng.random() < min(1.0, 6.0 * len(inside) / max(len(q0) - i, 1)):
                job = inside.pop(0)
            if job is not None:
                if job["kind"] == "pretaken":
                    a = emit(planted_row(job, True), job["desc"], True)
                    planted.append(dict(kind="pretaken", first=a, second=a, X=job["X"], Y=-1, same_group=True, observed=True))
                else:
                    a = emit(planted_row(job, job["observed"]), job["first_desc"], True)
                    pending = [job["gap"], job, a]
        emit(q0[i].copy(), d0[i].copy(), len(cand[i]) > 0)
        if pending is not None:
            if pending[0] == 0:
                job, a = pending[1], pending[2]
                if job["gap"] == 0:                  # the copy goes right behind the original: before this natural query
                    nat_q, nat_d, nat_w = out_q.pop(), out_d.pop(), where.pop()
                    state["live"] -= int(len(cand[i]) > 0)
                    c = emit(planted_row(job, True if job["kind"] == "second" else job["observed"]), job["desc"], True)
                    emit(nat_q, nat_d, len(cand[i]) > 0)
                else:
                    c = emit(planted_row(job, True if job["kind"] == "second" else job["observed"]), job["desc"], True)
                planted.append(dict(kind=job["kind"], first=a, second=c, X=job["X"], Y=job["Y"], same_group=where[a] == where[c], observed=job["observed"]))
                pending = None
            else:
                pending[0] -= 1
    assert not inside and pending is None, (mode, len(inside), len(straddlers))
    return dict(q=np.array(out_q, QUERY_DTYPE), d=np.ascontiguousarray(np.stack(out_d), np.uint8), taken0=taken0, assigned0=assigned0, planted=planted)


def match_of_query(assigned, nq):
    """Per query the keypoint that names it in `assigned` (the query that owns the keypoint when the search ends), or -1."""
    out = np.full(nq, -1, np.int64)
    idx = np.flatnonzero((assigned >= 0) & (assigned < nq))
    out[assigned[idx]] = idx
    return out


def contention_occurrence(fo, mode, case, ratio, a_ref, t_ref):
    """What the planted cases did in the serial oracle's run (a_ref / t_ref: its assigned / taken, orientation check off).  Counts per
    kind of the pairs in which the dependence really happened, and the placement counts (same group / across an edge)."""
    nq = len(case["q"])
    mo = match_of_query(a_ref, nq)
    n = dict(observed=0, unobserved=0, distant=0, second=0, pretaken=0)
    place = {}
    for p in case["planted"]:
        k, a, c, X = p["kind"], p["first"], p["second"], p["X"]
        place.setdefault(k, [0, 0])[0 if p["same_group"] else 1] += 1
        if k in ("observed", "distant"):
            n[k] += int(mo[a] == X and mo[c] != X and t_ref[X] == 1)         # the copies ended differently: the later one lost X
        elif k == "unobserved":
            n[k] += int(a_ref[X] == c and t_ref[X] == 0 and mo[a] == -1)       # nothing taken, the later copy owns the assignment
        elif k == "pretaken":
            n[k] += int(a_ref[X] == 100000 + X and mo[a] != X)
        elif k == "second" and p["observed"]:
            alone = case["q"].copy()
            alone["flags"] = 0
            alone["flags"][c] = case["q"]["flags"][c]
            _, a1, _ = fo.search_by_projection(mode, alone, case["d"], ratio, False, case["taken0"], case["assigned0"], orb_dist=64)
            n[k] += int(match_of_query(a1, nq)[c] != mo[c])                   # with the earlier queries before it the outcome differs
    return n, place


def contention_case(oracle_lib, s, mode, seed, ratio=0.9):
    """Planted set for `mode` (0, 1, 2, 7 through search_by_projection; 6 through the fuse search) on scene entry s, the oracle's answers
    and the occurrence counts, asserted here: at least 8 observed / unobserved / distant pairs and at least 4 mode-0 second-best cases
    in which the order of the queries decided the outcome, and planted pairs both inside a group and across a group edge."""
    fo = oracle_lib.FrameOracle(s["kb"], s["db"], s["bounds"], None)
    q0 = natural_queries(s, mode, seed)
    case = plant_contention(fo, s, mode, q0, s["da"], seed, ratio, with_taken=mode != 6)
    case["fo"] = fo
    if mode == 6:
        zero = np.zeros(8, np.float32)
        case["ref"] = fo.fuse_search(case["q"], case["d"], zero)
        both = sum(int(case["ref"][1][p["first"]] == p["X"] == case["ref"][1][p["second"]]) for p in case["planted"])
        assert both >= 32, both                                               # two lanes of a group accept one keypoint
        return case
    case["ref"] = {chk: fo.search_by_projection(mode, case["q"], case["d"], ratio, chk, case["taken0"], case["assigned0"], orb_dist=64)
                   for chk in ((False, True) if mode in (1, 2) else (False,))}
    _, a_ref, t_ref = case["ref"][False]
    n, place = contention_occurrence(fo, mode, case, ratio, a_ref, t_ref)
    case["occurred"], case["placement"] = n, place
    for k in KINDS[mode]:
        assert sum(1 for p in case["planted"] if p["kind"] == k) >= 32, (mode, k)
        assert n[k] >= (4 if k == "second" else 8), (mode, k, n)
        if k != "pretaken":
            assert place[k][0] >= 8 and place[k][1] >= 1, (mode, k, place)   # inside a group / across a group edge
    return case
