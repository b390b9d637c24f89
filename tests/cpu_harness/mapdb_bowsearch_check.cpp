// Stand-alone check of ydorbslam_amd/csrc/mapdb_bowsearch_host.h (no HIP, no GPU): the host half of the batched BoW searches over the
// resident map table.  tests/test_mapdb_bowsearch_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.
// Part 1 prints one line per case, the case names are the rules: every refusal of the frame validation, the flattening of the frame's
// feature vector, the query prefix sums and "has a good map point".
// Part 2 drives a seeded sequence in which keyframe rows, features, descriptor blocks and BoW spans are staged through their host
// halves (mapdb_rows_host.h, mapdb_feat_host.h, mapdb_desc_host.h, mapdb_bow_host.h), with every packed delta executed on host arrays
// and keyframes coming and going until the pools repack.  After every sync bowSearchOnHost runs over the host copies of the pools,
// where the spans lie after the delta, and must equal a second statement of the two searches that never sees a pool: the model's own
// vectors, DBoW3-style std::map<node, vector<feature>> feature vectors walked with iterators and lower_bound as the reference's loop
// does (orbMatcher.cpp:317-361), validity from a per-feature list computed up front.
// The exit status is the number of failed cases.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_bowsearch_host.h"
#include "../../ydorbslam_amd/csrc/mapdb_desc_host.h"
#include "../../ydorbslam_amd/csrc/mapdb_feat_host.h"

constexpr int kNameWidth = 92;
#include "check_common.h"

using namespace ydorb::mapdb;

// --------------------------------------------------------------------------------------------------------------------- part 1
struct FrameIn {   // a YdBowSide over vectors
  std::vector<YdKeyPoint> kps;
  std::vector<uint8_t> desc, valid;
  std::vector<uint32_t> ids;
  std::vector<int32_t> start{0}, feat;
  bool useValid = false;
  YdBowSide side() const {
    YdBowSide s{};
    s.kps = kps.data(); s.desc = desc.data(); s.valid = useValid ? valid.data() : nullptr; s.n = (int32_t)kps.size();
    s.fv.node_ids = ids.data(); s.fv.node_start = start.data(); s.fv.feat = feat.data(); s.fv.n_nodes = (int32_t)ids.size();
    return s;
  }
};

static FrameIn smallFrame() {
  FrameIn f;
  f.kps.resize(4); f.desc.resize(4 * 32, 0x5a); f.valid.assign(4, 1);
  f.ids = {3, 7, 9}; f.start = {0, 2, 3, 4}; f.feat = {2, 0, 3, 1};
  return f;
}

static void cases() {
  std::string e;
  const FrameIn ok = smallFrame();
  { YdBowSide s = ok.side(); e.clear(); expect("a well-formed frame", checkBowFrame(&s, e), e, nullptr); }
  e.clear(); expect("null frame", checkBowFrame(nullptr, e), e, "null frame");
  { YdBowSide s = ok.side(); s.n = -1; e.clear(); expect("n of -1", checkBowFrame(&s, e), e, "frame: n -1 outside 0..65535"); }
  { YdBowSide s = ok.side(); s.n = 65536; e.clear(); expect("n of 65536", checkBowFrame(&s, e), e, "frame: n 65536 outside 0..65535"); }
  { YdBowSide s = ok.side(); s.kps = nullptr; e.clear(); expect("null kps", checkBowFrame(&s, e), e, "frame: null kps or desc"); }
  { YdBowSide s = ok.side(); s.desc = nullptr; e.clear(); expect("null desc", checkBowFrame(&s, e), e, "frame: null kps or desc"); }
  { YdBowSide s = ok.side(); s.fv.n_nodes = -2; e.clear(); expect("negative n_nodes", checkBowFrame(&s, e), e, "frame: negative number of nodes: -2"); }
  { YdBowSide s = ok.side(); s.fv.node_start = nullptr; e.clear(); expect("null node_start", checkBowFrame(&s, e), e, "frame: null node_start"); }
  { FrameIn f = ok; f.start[0] = 1; YdBowSide s = f.side(); e.clear(); expect("node_start[0] != 0", checkBowFrame(&s, e), e, "frame: node_start[0] is 1, not 0"); }
  { FrameIn f = ok; f.start[2] = 1; YdBowSide s = f.side(); e.clear(); expect("node_start decreases", checkBowFrame(&s, e), e, "frame: node_start decreases at 2"); }
  { YdBowSide s = ok.side(); s.fv.node_ids = nullptr; e.clear(); expect("null node_ids", checkBowFrame(&s, e), e, "frame: null node_ids"); }
  { FrameIn f = ok; f.ids[2] = 7; YdBowSide s = f.side(); e.clear(); expect("node ids that repeat", checkBowFrame(&s, e), e, "frame: node id 7 after 7"); }
  { FrameIn f = ok; f.ids[2] = 5; YdBowSide s = f.side(); e.clear(); expect("node ids that decrease", checkBowFrame(&s, e), e, "frame: node id 5 after 7"); }
  { YdBowSide s = ok.side(); s.fv.feat = nullptr; e.clear(); expect("null feat", checkBowFrame(&s, e), e, "frame: null feat"); }
  { FrameIn f = ok; f.feat[3] = 4; YdBowSide s = f.side(); e.clear(); expect("a feature index of n", checkBowFrame(&s, e), e, "frame: entry 3: feature index 4 outside 0..3"); }
  { FrameIn f = ok; f.feat[1] = -1; YdBowSide s = f.side(); e.clear(); expect("a feature index of -1", checkBowFrame(&s, e), e, "frame: entry 1: feature index -1 outside 0..3"); }
  {
    FrameIn f;
    f.kps.resize(65535); f.desc.resize((size_t)65535 * 32); f.ids = {1}; f.start = {0, 1}; f.feat = {65534};
    YdBowSide s = f.side(); e.clear(); expect("a frame of 65535 features", checkBowFrame(&s, e), e, nullptr);
  }
  {
    const int32_t zero = 0;
    YdBowSide s{}; s.fv.node_start = &zero;
    e.clear(); expect("an empty frame", checkBowFrame(&s, e), e, nullptr);
    YdBowSide t = ok.side(); t.fv.n_nodes = 0; t.fv.node_ids = nullptr; t.fv.feat = nullptr; t.fv.node_start = &zero;
    e.clear(); expect("a frame without nodes", checkBowFrame(&t, e), e, nullptr);
  }
  { FrameIn f = ok; f.useValid = false; YdBowSide s = f.side(); e.clear(); expect("null valid is every feature", checkBowFrame(&s, e) && s.valid == nullptr, e, nullptr); }
  {
    FrameIn f = ok; f.ids[2] = 0xFFFFFFFFu;
    YdBowSide s = f.side();
    std::vector<BowRec> flat;
    e.clear();
    const bool pass = checkBowFrame(&s, e);
    flattenFrameBow(s.fv, flat);
    expect("a node id of 2^32 - 1", pass && flat.size() == 4 && (uint32_t)flat[3].node == 0xFFFFFFFFu, e, nullptr);
  }
  {
    YdBowSide s = ok.side();
    std::vector<BowRec> flat;
    flattenFrameBow(s.fv, flat);
    const int32_t want[4][2] = {{3, 2}, {3, 0}, {7, 3}, {9, 1}};
    bool same = flat.size() == 4;
    for (size_t i = 0; same && i < 4; i++) same = flat[i].node == want[i][0] && flat[i].feat == want[i][1];
    expect("flatten: map order", same, "", nullptr);
  }
  {
    const int32_t len[4] = {5, 7, 0, 3};
    const uint8_t status[4] = {0, 4, 0, 0};
    std::vector<int32_t> start;
    const bool pass = bowQueryStarts(len, status, 4, start);
    expect("query starts skip the unusable", pass && start == std::vector<int32_t>({0, 5, 5, 5, 8}), "", nullptr);
    const int32_t big[3] = {INT32_MAX, 1, 1};
    const uint8_t none[3] = {0, 0, 0};
    expect("query starts past INT32_MAX", !bowQueryStarts(big, none, 3, start), "", nullptr);
  }
  {
    const uint8_t bad[4] = {0, 1, 0, 1};
    expect("good map point: the three clauses",
           goodMapPoint(0, bad, 4) && goodMapPoint(2, bad, 4) && !goodMapPoint(1, bad, 4) && !goodMapPoint(-1, bad, 4) && !goodMapPoint(4, bad, 4) && !goodMapPoint(2, bad, 2) &&
               !goodMapPoint(INT32_MAX, bad, 4),
           "", nullptr);
  }
}

// --------------------------------------------------------------------------------------------------------------------- part 2
constexpr int32_t kPoints = 240, kPointCap = 256, kKeyframes = 12, kBase = 200;

struct KfModel {   // one keyframe as the caller holds it
  std::vector<int32_t> row;
  std::vector<YdKeyPoint> kps;
  std::vector<uint8_t> desc, valid;   // valid: the frame only
  std::vector<BowRec> bow;            // map order
};

struct Db {   // the handle's four keyframe relations without a device
  RowsHost rows;
  DescHost desc;
  FeatHost feat;
  BowHost bow;
  RowTables R;
  BlockTables B;
  FeatTables F;
  BowTables W;
  std::vector<uint8_t> delta;
  RowPlan lastR, lastB, lastF, lastW;
  Db() : rows(kKeyframes, 512), desc(kPointCap, kKeyframes), feat(kKeyframes), bow(kKeyframes) { feat.enable(); bow.enable(); }
  void sync() {
    syncOnHost(rows, lastR, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, R); });
    syncOnHost(desc.blocks, lastB, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, B); });
    syncOnHost(feat.feats, lastF, delta, [this](const RowPlan& P, const uint8_t* d) { executeFeatures(P, d, F); });
    syncOnHost(bow.spans, lastW, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, W); });
  }
  bool set(int32_t k, const KfModel& m, std::string& e) {
    const int32_t n = (int32_t)m.row.size(), start[2] = {0, n}, bstart[2] = {0, (int32_t)m.bow.size()}, none = 0;
    const YdKeyPoint nokp{};
    std::vector<uint32_t> node;
    std::vector<int32_t> feats;
    for (const BowRec& r : m.bow) { node.push_back((uint32_t)r.node); feats.push_back(r.feat); }
    const uint32_t nonode = 0;
    return rows.setRows(&k, 1, start, n ? m.row.data() : &none, kPoints, e) && desc.setBlocks(&k, 1, start, n ? m.desc.data() : (const uint8_t*)"", e) &&
           feat.set(&k, 1, start, n ? m.kps.data() : &nokp, nullptr, e) && bow.set(&k, 1, bstart, node.empty() ? &nonode : node.data(), feats.empty() ? &none : feats.data(), e);
  }
  // the side of bowSearchOnHost for keyframe k: pointers into the pools, where the spans lie after the last sync
  BowSearchSide side(int32_t k) const {
    BowSearchSide s{};
    s.bow = W.pool.data() + W.rowStart[(size_t)k]; s.bowLen = W.rowLen[(size_t)k];
    s.kps = F.kps.data() + F.start[(size_t)k]; s.n = F.len[(size_t)k];
    s.desc = reinterpret_cast<const uint8_t*>(B.pool.data() + B.rowStart[(size_t)k]);
    s.row = R.pool.data() + R.rowStart[(size_t)k];
    return s;
  }
};

static std::vector<uint8_t> g_base;   // [kBase][32]

static KfModel makeKf(std::mt19937& g, int n, const std::vector<int32_t>& neverSet, bool frame) {
  KfModel m;
  std::vector<int32_t> base((size_t)kBase);
  for (int i = 0; i < kBase; i++) base[(size_t)i] = i;
  std::shuffle(base.begin(), base.end(), g);
  m.row.resize((size_t)n); m.kps.resize((size_t)n); m.desc.resize((size_t)n * 32); m.valid.resize((size_t)n);
  std::vector<std::pair<int32_t, int32_t>> filed;   // (node, feature)
  for (int i = 0; i < n; i++) {
    const int32_t b = base[(size_t)i % kBase];
    memcpy(&m.desc[(size_t)i * 32], &g_base[(size_t)b * 32], 32);
    for (int f = 0; f < 3; f++) { const unsigned bit = g() % 256; m.desc[(size_t)i * 32 + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
    YdKeyPoint& kp = m.kps[(size_t)i];
    kp = YdKeyPoint{};
    kp.x = (float)(g() % 64000) / 100.0f; kp.y = (float)(g() % 48000) / 100.0f; kp.size = 31.0f; kp.octave = (int32_t)(g() % 8); kp.class_id = -1;
    kp.angle = (float)((b * 37 + (g() % 6 == 0 ? g() % 360 : 20)) % 360);
    m.row[(size_t)i] = g() % 10 < 7 ? b : -1;
    if (g() % 40 == 0) m.row[(size_t)i] = neverSet[g() % neverSet.size()];
    m.valid[(size_t)i] = g() % 10 != 0;
    filed.push_back({(b % 9) * 3 + 1, i});
  }
  std::shuffle(filed.begin(), filed.end(), g);   // within a node the features keep the vector's order, which need not ascend
  std::stable_sort(filed.begin(), filed.end(), [](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) { return a.first < b.first; });
  for (const auto& f : filed) m.bow.push_back(BowRec{f.first, f.second});
  if (frame) m.row.assign((size_t)n, -1);
  return m;
}

// The second statement: the reference's loop over DBoW3-style feature vectors.  mode 4: out / point [A.n]; mode 3: [B.n].
struct Decided { int bad = 0, never = 0, invalid = 0; };
static int secondStatement(int mode, const KfModel& A, const KfModel& B, const std::vector<uint8_t>& bad, const std::vector<int32_t>& neverSet, bool useValid, float ratio,
                           int checkOri, std::vector<int32_t>& out, std::vector<int32_t>& point, Decided& why) {
  using FeatureVector = std::map<uint32_t, std::vector<int32_t>>;
  FeatureVector fa, fb;
  for (const BowRec& r : A.bow) fa[(uint32_t)r.node].push_back(r.feat);
  for (const BowRec& r : B.bow) fb[(uint32_t)r.node].push_back(r.feat);
  auto isNever = [&](int32_t p) { return std::find(neverSet.begin(), neverSet.end(), p) != neverSet.end(); };
  auto validOf = [&](const KfModel& K, bool isFrame) {
    std::vector<uint8_t> v(K.row.size());
    for (size_t i = 0; i < v.size(); i++) {
      if (isFrame) { v[i] = !useValid || K.valid[i]; why.invalid += !v[i]; continue; }
      const int32_t p = K.row[i];
      v[i] = p >= 0 && p < kPointCap && !bad[(size_t)p];
      if (p >= 0 && !v[i]) (isNever(p) ? why.never : why.bad)++;
    }
    return v;
  };
  const std::vector<uint8_t> va = validOf(A, false), vb = validOf(B, mode == 3);
  const size_t nOut = mode == 3 ? B.row.size() : A.row.size();
  out.assign(nOut, -1); point.assign(nOut, -1);
  std::vector<uint8_t> matchedB(B.row.size(), 0);
  std::vector<std::vector<int32_t>> rotHist(30);
  int matchNum = 0;
  auto ia = fa.begin(), ib = fb.begin();
  while (ia != fa.end() && ib != fb.end()) {
    if (ia->first == ib->first) {
      for (const int32_t idxA : ia->second) {
        if (!va[(size_t)idxA]) continue;
        int bestDist = 256, secondDist = 256;
        int32_t bestIdx = -1;
        for (const int32_t idxB : ib->second) {
          if (matchedB[(size_t)idxB] || !vb[(size_t)idxB]) continue;
          int dist = 0;
          for (int w = 0; w < 32; w++) dist += __builtin_popcount((unsigned)(A.desc[(size_t)idxA * 32 + (size_t)w] ^ B.desc[(size_t)idxB * 32 + (size_t)w]));
          if (dist < bestDist) { secondDist = bestDist; bestDist = dist; bestIdx = idxB; }
          else if (dist < secondDist) secondDist = dist;
        }
        if (bestDist <= 50 && static_cast<float>(bestDist) < ratio * static_cast<float>(secondDist)) {
          matchedB[(size_t)bestIdx] = 1;
          const int32_t o = mode == 3 ? bestIdx : idxA;
          out[(size_t)o] = mode == 3 ? idxA : bestIdx;
          point[(size_t)o] = mode == 3 ? A.row[(size_t)idxA] : B.row[(size_t)bestIdx];
          if (checkOri) {
            float rot = A.kps[(size_t)idxA].angle - B.kps[(size_t)bestIdx].angle;
            if (rot < 0.0) rot += 360.0;
            int bin = (int)round(rot * (float)(1.0 / 30));
            if (bin == 30) bin = 0;
            rotHist[(size_t)bin].push_back(o);
          }
          matchNum++;
        }
      }
      ++ia; ++ib;
    } else if (ia->first < ib->first) {
      ia = fa.lower_bound(ib->first);
    } else {
      ib = fb.lower_bound(ia->first);
    }
  }
  if (checkOri) {
    int i1 = -1, i2 = -1, i3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < 30; i++) {
      const int s = (int)rotHist[(size_t)i].size();
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
      else if (s > max3) { max3 = s; i3 = i; }
    }
    if (max2 < max1 / 10) { i3 = -1; i2 = -1; }
    else if (max3 < max1 / 10) { i3 = -1; }
    for (int i = 0; i < 30; i++)
      if (i != i1 && i != i2 && i != i3)
        for (const int32_t o : rotHist[(size_t)i]) { out[(size_t)o] = -1; point[(size_t)o] = -1; matchNum--; }
  }
  return matchNum;
}

static void sequence() {
  std::mt19937 g(20240611);
  g_base.resize((size_t)kBase * 32);
  for (uint8_t& b : g_base) b = (uint8_t)(g() % 256);
  const std::vector<int32_t> neverSet = {17, 88, 150, 201};
  std::vector<uint8_t> bad((size_t)kPointCap, 1);   // a slot never set reads as bad
  for (int32_t p = 0; p < kPoints; p++)
    if (std::find(neverSet.begin(), neverSet.end(), p) == neverSet.end()) bad[(size_t)p] = g() % 10 == 0;
  Db d;
  std::map<int32_t, KfModel> model;
  std::string e;
  bool same = true;
  int searches = 0, matches[2] = {0, 0}, culled = 0;
  Decided why;
  for (int round = 0; round < 40 && same; round++) {
    // keyframes come, are replaced by longer or shorter ones and go: garbage accumulates in every pool until it repacks
    for (int c = 0; c < 3; c++) {
      const int32_t k = (int32_t)(g() % kKeyframes);
      const bool erase = g() % 5 == 0 && model.size() > 4;
      KfModel m = erase ? KfModel() : makeKf(g, 60 + (int)(g() % 120), neverSet, false);
      if (!d.set(k, m, e)) { printf("sequence: a set was refused: %s FAILED\n", e.c_str()); g_failed++; return; }
      if (erase) model.erase(k); else model[k] = m;
    }
    if (!model.empty() && round % 3 == 1) {   // a single row entry and a bad flag change
      auto it = model.begin();
      std::advance(it, (long)(g() % model.size()));
      const int32_t k = it->first, i = (int32_t)(g() % it->second.row.size()), v = (int32_t)(g() % kPoints);
      if (!d.rows.setEntries(&k, &i, &v, 1, kPoints, e)) { printf("sequence: set_row_entries refused: %s FAILED\n", e.c_str()); g_failed++; return; }
      it->second.row[(size_t)i] = v;
      const int32_t p = (int32_t)(g() % kPoints);
      if (std::find(neverSet.begin(), neverSet.end(), p) == neverSet.end()) bad[(size_t)p] ^= 1;
    }
    d.sync();
    if (model.size() < 2) continue;
    const KfModel frame = makeKf(g, 150 + (int)(g() % 60), neverSet, true);
    for (int pair = 0; pair < 3 && same; pair++) {
      auto ia = model.begin(), ib = model.begin();
      std::advance(ia, (long)(g() % model.size()));
      std::advance(ib, (long)(g() % model.size()));   // may be the same keyframe
      const float ratio = pair == 0 ? 0.6f : pair == 1 ? 0.75f : 0.9f;
      for (int mode = 3; mode <= 4 && same; mode++)
        for (int ori = 0; ori <= 1 && same; ori++) {
          const bool useValid = (round + pair) % 2 == 0;
          const KfModel& MB = mode == 4 ? ib->second : frame;
          BowSearchSide A = d.side(ia->first), B{};
          if (mode == 4) B = d.side(ib->first);
          else { B.bow = frame.bow.data(); B.bowLen = (int32_t)frame.bow.size(); B.kps = frame.kps.data(); B.desc = frame.desc.data(); B.n = (int32_t)frame.row.size(); B.valid = useValid ? frame.valid.data() : nullptr; }
          const size_t nOut = mode == 3 ? frame.row.size() : ia->second.row.size();
          std::vector<int32_t> got(nOut, -9), gotPoint(nOut, -9), want, wantPoint;
          const int nGot = bowSearchOnHost(mode, A, B, bad.data(), kPointCap, ratio, ori, got.data(), gotPoint.data());
          const int nWant = secondStatement(mode, ia->second, MB, bad, neverSet, useValid, ratio, ori, want, wantPoint, why);
          same = nGot == nWant && got == want && gotPoint == wantPoint;
          if (!same) printf("sequence: round %d pair %d mode %d ori %d: %d matches, the second statement has %d MISMATCH\n", round, pair, mode, ori, nGot, nWant);
          searches++;
          if (!ori) matches[mode - 3] += nGot;
          else {
            std::vector<int32_t> w2, p2;
            Decided unused;
            culled += secondStatement(mode, ia->second, MB, bad, neverSet, useValid, ratio, 0, w2, p2, unused) - nWant;
          }
        }
    }
  }
  YdMapDbRowStats rs, ws;
  d.rows.stats(rs); d.bow.spans.stats(ws);
  char text[160];
  snprintf(text, sizeof text, "%d searches", searches);
  expect("sequence: every search equals the second statement", same && searches >= 400, text, nullptr);
  snprintf(text, sizeof text, "rows %d kept %d grown, BoW %d kept %d grown", rs.repacks_kept, rs.repacks_grown, ws.repacks_kept, ws.repacks_grown);
  expect("sequence: the row and BoW pools repacked", rs.repacks_kept + rs.repacks_grown >= 1 && ws.repacks_kept + ws.repacks_grown >= 1, text, nullptr);
  snprintf(text, sizeof text, "%d frame form, %d keyframe form", matches[0], matches[1]);
  expect("sequence: matches in both modes", matches[0] >= 1000 && matches[1] >= 1000, text, nullptr);
  snprintf(text, sizeof text, "%d bad, %d never set, %d invalid", why.bad, why.never, why.invalid);
  expect("sequence: a bad point, a never-set slot and an invalid frame feature each decided a query", why.bad >= 1 && why.never >= 1 && why.invalid >= 1, text, nullptr);
  snprintf(text, sizeof text, "%d culled", culled);
  expect("sequence: the rotation histogram culled a match", culled >= 1, text, nullptr);
}

int main() {
  cases();
  sequence();
  printf("%d failed\n", g_failed);
  return g_failed;
}
