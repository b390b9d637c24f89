// Stand-alone check of ydorbslam_amd/csrc/mapdb_lba_host.h (no HIP, no GPU): every refusal of ydorb_mapdb_local_ba_graph, "a refused
// call changes nothing", the result layout, and the host execution of the contract (lbaOnHost) against a naive model on seeded tables.
// tests/test_mapdb_lba_cpu.py builds it with -fsanitize=address,undefined and runs it as its own process.
// The tables are kept as the handle keeps them: rows, views and features staged through their host halves and every packed delta
// executed on host arrays as the kernels execute it, repacks included, so lbaOnHost reads spans at the offsets a device would hold.
// The model is the reference's shape: a point's observations are a std::map<keyframe, index> (walked in key order, the order the views
// are staged in), the tags are std::sets, the pose lookup is a std::map.  One line per case; the exit status is the number of failed cases.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../ydorbslam_amd/csrc/mapdb_lba_host.h"

constexpr int kNameWidth = 72;
#include "check_common.h"

using namespace ydorb::mapdb;

constexpr int32_t kKf = 40, kPoints = 600;

struct Model {
  std::vector<std::vector<int32_t>> row = std::vector<std::vector<int32_t>>(kKf);
  std::vector<std::map<int32_t, int32_t>> obs = std::vector<std::map<int32_t, int32_t>>(kPoints);
  std::vector<std::vector<YdKeyPoint>> kps = std::vector<std::vector<YdKeyPoint>>(kKf);
  std::vector<std::vector<float>> rightX = std::vector<std::vector<float>>(kKf);
  std::vector<uint8_t> bad = std::vector<uint8_t>(kPoints, 0);
  std::vector<float> pos = std::vector<float>(3 * kPoints, 0.f);
};

struct Db {   // the three relations without a device
  RowsHost rows{8, 64};
  DescHost desc{16, 8};
  FeatHost feat{8};
  RowTables R;
  ViewTables V;
  FeatTables F;
  std::vector<uint8_t> delta;
  RowPlan last;
  Db() { feat.enable(); }
  void sync() {
    syncOnHost(rows, last, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, R); });
    syncOnHost(desc.views, last, delta, [this](const RowPlan& P, const uint8_t* d) { executeRows(P, d, V); });
    syncOnHost(feat.feats, last, delta, [this](const RowPlan& P, const uint8_t* d) { executeFeatures(P, d, F); });
  }
};

static bool stageKeyframe(Db& d, const Model& m, int32_t k, std::string& e) {
  const int32_t start[2] = {0, (int32_t)m.row[(size_t)k].size()};
  static const int32_t none = -1;
  if (!d.rows.setRows(&k, 1, start, m.row[(size_t)k].empty() ? &none : m.row[(size_t)k].data(), kPoints, e)) return false;
  const int32_t fstart[2] = {0, (int32_t)m.kps[(size_t)k].size()};
  static const YdKeyPoint noKp{};
  return d.feat.set(&k, 1, fstart, m.kps[(size_t)k].empty() ? &noKp : m.kps[(size_t)k].data(), m.rightX[(size_t)k].empty() ? nullptr : m.rightX[(size_t)k].data(), e);
}
static bool stagePoint(Db& d, const Model& m, int32_t p, std::string& e) {
  std::vector<int32_t> kf{0}, idx{0};
  kf.clear(); idx.clear();
  for (const auto& ob : m.obs[(size_t)p]) { kf.push_back(ob.first); idx.push_back(ob.second); }
  const int32_t start[2] = {0, (int32_t)kf.size()};
  static const int32_t none = 0;
  return d.desc.setViews(&p, 1, start, kf.empty() ? &none : kf.data(), idx.empty() ? &none : idx.data(), kPoints, kKf, e);
}

// The reference's loops on the model (optimizer.hpp:59-113)
static void modelGraph(const Model& m, const std::vector<int32_t>& kfSlots, const float* sigma, LbaHostGraph& G) {
  G = LbaHostGraph{};
  const auto isBad = [&](int32_t k) { return m.kps[(size_t)k].empty(); };
  std::set<int32_t> localTag(kfSlots.begin(), kfSlots.end()), fixedTag, pointTag;
  std::vector<int32_t> localMPs, fixedKFs;
  for (const int32_t k : kfSlots)
    for (const int32_t mp : m.row[(size_t)k])
      if (mp >= 0 && !m.bad[(size_t)mp] && pointTag.insert(mp).second) localMPs.push_back(mp);
  for (const int32_t mp : localMPs)
    for (const auto& ob : m.obs[(size_t)mp]) {
      if (localTag.count(ob.first) || fixedTag.count(ob.first)) continue;
      fixedTag.insert(ob.first);
      if (!isBad(ob.first)) fixedKFs.push_back(ob.first);
    }
  std::map<int32_t, int32_t> poseIndex;
  const auto addPose = [&](int32_t k, bool fix) { poseIndex[k] = (int32_t)G.poseKf.size(); G.poseKf.push_back(k); G.poseFixed.push_back(fix ? 1 : 0); };
  for (const int32_t k : kfSlots) addPose(k, false);
  G.nLocal = (int32_t)kfSlots.size();
  for (const int32_t k : fixedKFs) addPose(k, true);
  G.nFixed = (int32_t)fixedKFs.size();
  for (size_t p = 0; p < localMPs.size(); p++) {
    const int32_t mp = localMPs[p];
    G.pointSlot.push_back(mp);
    for (int c = 0; c < 3; c++) G.points.push_back((double)m.pos[3 * (size_t)mp + (size_t)c]);
    uint8_t status = 0;
    size_t before = G.edgePose.size();
    for (const auto& ob : m.obs[(size_t)mp]) {
      if (isBad(ob.first)) { status |= YDORB_LBA_POINT_SKIPPED_VIEWS; continue; }
      if (ob.second >= (int32_t)m.kps[(size_t)ob.first].size()) { status |= YDORB_LBA_POINT_VIEW_OUT_OF_RANGE; continue; }
      const auto it = poseIndex.find(ob.first);
      if (it == poseIndex.end()) continue;
      const YdKeyPoint& kp = m.kps[(size_t)ob.first][(size_t)ob.second];
      const float ur = m.rightX[(size_t)ob.first][(size_t)ob.second];
      G.edgePose.push_back(it->second); G.edgePoint.push_back((int32_t)p);
      G.meas.push_back(kp.x); G.meas.push_back(kp.y); G.meas.push_back(ur < 0 ? -1.0 : (double)ur);
      G.info.push_back(sigma[kp.octave]);
      G.edgeKf.push_back(ob.first); G.edgeIdx.push_back(ob.second);
    }
    if (G.edgePose.size() == before) status |= YDORB_LBA_POINT_NO_EDGES;
    G.pointStatus.push_back(status);
  }
}

template <class T> static bool sameBits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}
static bool same(const LbaHostGraph& a, const LbaHostGraph& b) {
  return a.nLocal == b.nLocal && a.nFixed == b.nFixed && sameBits(a.poseKf, b.poseKf) && sameBits(a.poseFixed, b.poseFixed) && sameBits(a.pointSlot, b.pointSlot) &&
         sameBits(a.pointStatus, b.pointStatus) && sameBits(a.points, b.points) && sameBits(a.edgePose, b.edgePose) && sameBits(a.edgePoint, b.edgePoint) &&
         sameBits(a.edgeKf, b.edgeKf) && sameBits(a.edgeIdx, b.edgeIdx) && sameBits(a.meas, b.meas) && sameBits(a.info, b.info);
}

int main() {
  std::string e;
  std::vector<uint8_t> mark;
  const int32_t kf3[3] = {2, 0, 5}, outside[2] = {1, 8}, negative[2] = {-1, 1}, twice[4] = {3, 1, 4, 1};
  float sigma[8];
  for (int l = 0; l < 8; l++) sigma[l] = 1.0f / (1.0f + (float)l);
  YdLocalBaGraph out;
  const auto refused = [&](const char* name, bool ok, const char* needle) {
    expect(name, ok, e, needle);
    const bool clean = std::all_of(mark.begin(), mark.end(), [](uint8_t b) { return b == 0; });
    if (!clean) { printf("%-*s FAILED\n", kNameWidth, "... and left its scratch marked"); g_failed++; }
    e.clear();
  };
  // ---- part 1: the refusals, in the order the header lists them
  refused("null out", checkLbaArgs(kf3, 3, sigma, nullptr, 8, true, mark, e), "null out");
  refused("negative n_kf", checkLbaArgs(kf3, -1, sigma, &out, 8, true, mark, e), "negative number of keyframe slots: -1");
  refused("null kf_slots", checkLbaArgs(nullptr, 3, sigma, &out, 8, true, mark, e), "null kf_slots");
  refused("null inv_level_sigma2", checkLbaArgs(kf3, 3, nullptr, &out, 8, true, mark, e), "null inv_level_sigma2");
  refused("features not enabled", checkLbaArgs(kf3, 3, sigma, &out, 8, false, mark, e), "keyframe features are not enabled");
  refused("a slot outside 0..n_keyframes-1", checkLbaArgs(outside, 2, sigma, &out, 8, true, mark, e), "kf_slots[1]: keyframe slot 8 outside 0..7");
  refused("a negative slot", checkLbaArgs(negative, 2, sigma, &out, 8, true, mark, e), "kf_slots[0]: keyframe slot -1 outside 0..7");
  refused("a slot repeated in kf_slots", checkLbaArgs(twice, 4, sigma, &out, 8, true, mark, e), "kf_slots[3]: keyframe slot 1 is named twice");
  refused("an empty table refuses every slot", checkLbaArgs(kf3, 1, sigma, &out, 0, true, mark, e), "kf_slots[0]: keyframe slot 2 outside 0..-1");
  refused("a valid list", checkLbaArgs(kf3, 3, sigma, &out, 8, true, mark, e), nullptr);
  refused("n_kf == 0 with null kf_slots", checkLbaArgs(nullptr, 0, sigma, &out, 8, true, mark, e), nullptr);
  {
    const LbaLayout L(5, 7, 11);
    std::vector<uint8_t> area(L.bytes);
    lbaPointResult(L, area.data(), 3, 2, 7, 11, &out);
    const bool ok = out.problem.n_poses == 5 && out.problem.n_points == 7 && out.problem.n_edges == 11 && out.n_local == 3 && out.n_fixed == 2 &&
                    reinterpret_cast<uint8_t*>(out.problem.poses) + 56 * 5 <= area.data() + L.bytes && L.oPoses >= L.devBytes &&
                    reinterpret_cast<const uint8_t*>(out.problem.edge_inv_sigma2) + 8 * 11 <= area.data() + L.devBytes && L.oMeas % 16 == 0 && L.oPoints % 16 == 0 &&
                    out.problem.stop == nullptr && out.problem.fx == 0.0;
    expect("the result layout: aligned, the poses behind what the device writes", ok, "", nullptr);
  }
  // ---- part 2: seeded tables against the model
  std::mt19937 g(20260521u);
  const auto rnd = [&](int n) { return (int32_t)(g() % (uint32_t)n); };
  Model m;
  Db d;
  for (int32_t p = 0; p < kPoints; p++)
    for (int c = 0; c < 3; c++) m.pos[3 * (size_t)p + (size_t)c] = (float)rnd(2000) / 64.f - 15.f;
  bool all = true, sawSkipped = false, sawRange = false, sawNoEdges = false, sawFixedLate = false, sawRepack = false;
  int compared = 0;
  for (int round = 0; round < 30; round++) {
    // change a few keyframes: new features and a new row over them (or a cull), and the observations that follow
    std::vector<int32_t> touchedPoints;
    for (int c = 0; c < (round == 0 ? kKf : 4); c++) {
      const int32_t k = round == 0 ? c : rnd(kKf);
      for (const int32_t p : m.row[(size_t)k])
        if (p >= 0 && rnd(8) != 0) { m.obs[(size_t)p].erase(k); touchedPoints.push_back(p); }   // some stale views stay: culled or out of range
      const int32_t n = round > 0 && rnd(5) == 0 ? 0 : 20 + rnd(60);
      m.row[(size_t)k].assign((size_t)n, -1);
      m.kps[(size_t)k].assign((size_t)n, YdKeyPoint{});
      m.rightX[(size_t)k].assign((size_t)n, -1.f);
      for (int32_t i = 0; i < n; i++) {
        YdKeyPoint& kp = m.kps[(size_t)k][(size_t)i];
        kp.x = (float)rnd(64000) / 100.f; kp.y = (float)rnd(48000) / 100.f; kp.octave = rnd(8); kp.class_id = -1;
        if (k % 3 && rnd(3)) m.rightX[(size_t)k][(size_t)i] = kp.x - (float)rnd(4000) / 100.f;
        if (rnd(4) == 0) continue;
        const int32_t p = rnd(kPoints);
        if (m.obs[(size_t)p].count(k)) continue;
        m.row[(size_t)k][(size_t)i] = p;
        if (rnd(30)) m.obs[(size_t)p][k] = i;   // now and then a row entry the point does not know of
        touchedPoints.push_back(p);
      }
      if (!stageKeyframe(d, m, k, e)) { all = false; printf("stage keyframe %d: %s\n", k, e.c_str()); }
    }
    for (int c = 0; c < 6; c++) m.bad[(size_t)rnd(kPoints)] = (uint8_t)(rnd(3) == 0);
    std::sort(touchedPoints.begin(), touchedPoints.end());
    touchedPoints.erase(std::unique(touchedPoints.begin(), touchedPoints.end()), touchedPoints.end());
    for (const int32_t p : touchedPoints)
      if (!stagePoint(d, m, p, e)) { all = false; printf("stage point %d: %s\n", p, e.c_str()); }
    const int32_t repacksBefore = [&] { YdMapDbRowStats s; d.desc.views.stats(s); return s.repacks_kept + s.repacks_grown; }();
    d.sync();
    { YdMapDbRowStats s; d.desc.views.stats(s); sawRepack = sawRepack || s.repacks_kept + s.repacks_grown > repacksBefore; }
    for (int q = 0; q < 4; q++) {
      std::vector<int32_t> kfSlots;
      const int32_t want = q == 3 ? 0 : 1 + rnd(9);
      while ((int32_t)kfSlots.size() < want) {
        const int32_t k = rnd(kKf);
        if (std::find(kfSlots.begin(), kfSlots.end(), k) == kfSlots.end()) kfSlots.push_back(k);
      }
      if (!checkLbaArgs(kfSlots.data(), want, sigma, &out, kKf, true, mark, e)) { all = false; printf("refused: %s\n", e.c_str()); continue; }
      LbaHostGraph got, wantG;
      lbaOnHost(d.R, d.V, d.F, m.bad.data(), m.pos.data(), kKf, kfSlots.data(), want, sigma, got);
      modelGraph(m, kfSlots, sigma, wantG);
      compared++;
      if (!same(got, wantG)) { all = false; printf("round %d query %d MISMATCH: %zu / %zu edges, %d / %d fixed\n", round, q, got.edgePose.size(), wantG.edgePose.size(), got.nFixed, wantG.nFixed); }
      for (const uint8_t s : got.pointStatus) {
        sawSkipped = sawSkipped || (s & YDORB_LBA_POINT_SKIPPED_VIEWS); sawRange = sawRange || (s & YDORB_LBA_POINT_VIEW_OUT_OF_RANGE);
        sawNoEdges = sawNoEdges || (s & YDORB_LBA_POINT_NO_EDGES);
      }
      for (size_t i = 0; i < got.edgePose.size(); i++) sawFixedLate = sawFixedLate || (got.edgePose[i] >= got.nLocal && got.edgePoint[i] >= 64 && got.edgePose[i] == got.nLocal + got.nFixed - 1);
      // a refused call in between changes nothing: the same valid call gives the same graph again
      if (q == 1) {
        checkLbaArgs(twice, 4, sigma, &out, kKf, true, mark, e);
        LbaHostGraph again;
        lbaOnHost(d.R, d.V, d.F, m.bad.data(), m.pos.data(), kKf, kfSlots.data(), want, sigma, again);
        if (!same(again, got)) { all = false; printf("round %d: a refused call changed the result\n", round); }
      }
    }
  }
  printf("compared %d graphs\n", compared);
  expect("sequence: every graph equals the model's, bit for bit", all && compared == 120, "", nullptr);
  expect("sequence: a refused call in between changes nothing", all, "", nullptr);
  expect("sequence: views of culled keyframes were skipped", sawSkipped, "", nullptr);
  expect("sequence: a view past its keyframe's features was met", sawRange, "", nullptr);
  expect("sequence: a local point without an edge was met", sawNoEdges, "", nullptr);
  expect("sequence: a fixed keyframe first met at a point rank >= 64", sawFixedLate, "", nullptr);
  expect("sequence: the view pool was repacked between two graphs", sawRepack, "", nullptr);
  printf("%d failed\n", g_failed);
  return g_failed;
}
