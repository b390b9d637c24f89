// The resident map table behind the three map-maintenance adapters (c_api.h "Resident map table"): a class
// template over the reference's own KeyFrame / MapPoint types that owns one ydorb_mapdb_t and the pointer -> slot maps, with free
// lists.  Where mapPoint.hpp, keyFrame.hpp and keyFrameCullingImpl flatten the observation containers on every call, a MapMirror is
// told what changed:
//   touch(mp)          re-reads the point's observations, bad flag, reference keyframe and position at the next flush
//   touchPosition(mp)  re-reads its position only (a BA write-back)
//   touch(kf)          re-reads the camera centre
//   forget(mp / kf)    gives the slot back (a forgotten point is erased from the table, a forgotten keyframe's row is emptied)
//   touchRow(kf)       re-reads getMapPointMatches() at the next flush (keyframe rows)
//   touchEntry(kf, i)  re-reads entry i of getMapPointMatches() only (addMapPoint, eraseMapPointMatch, replaceMapPointMatch)
// INTEGRATION.md ("Resident map table") lists where the reference needs each.  flush() makes at most one call of each set_* entry; the
// three queries flush first and then walk only the keyframes' map-point vectors, never the observation maps.  A missed touch does not
// fail: results then differ from the reference's, and verify() names the slot.
// One thread at a time per MapMirror (the handle below it has its own mutex; the pointer maps here do not).
// correctLoopPoints, correctAfterEssentialGraph and correctAfterGlobalBA run the point loops of loop closing on the table in place
// (DESIGN.md section 6n); their comments below state what each takes from the caller.
// keyFrameCounter and localPoints are the two set queries of Tracking::updateLocalMap over the keyframe rows (tracking.hpp's
// updateLocalKeyFramesImpl / updateLocalPointsImpl); verifyRows() is verify() for the rows.
// enableDescriptors() adds the keyframes' descriptor blocks and the points' views: touchDescriptors(kf) once
// per keyframe, touch(mp) then also re-reads where the point is seen, forget() erases block and views, computeDistinctiveDescriptors
// is MapPoint::computeDistinctiveDescriptors for a list of points with no descriptor upload, verifyDescriptors() is verify() for the two.
// Off by default: without it no call of the descriptor entries is made.  Enable it before the first touch.
// enableAttributes() adds the points' normal, raw distances and descriptor: touchAttributes(mp) after the host
// set them (a constructor, replace()); updateNormalAndDepth, the three correction methods and computeDistinctiveDescriptors leave theirs
// in the table themselves; a group whose member is still unset (an empty matrix) is not staged, and a slot the mirror reuses reads as
// "no attributes" until the new point's are set; searchLocalPoints is the device part of Tracking::searchLocalPoints by slot (tracking.hpp's
// searchLocalPointsImpl(Mirror&, ...)); verifyAttributes() is verify() for them.  Assumed spellings beyond the others: MapPoint
// getNormal(), getDescriptor() and two one-line getters of the RAW members, getMinDistance() { lock; return m_flt_minDistance; } and
// getMaxDistance() { lock; return m_flt_maxDistance; } (tracking.hpp requires the second already).
// enableFeatures() adds the keyframes' undistorted keypoints and right coordinates: touchFeatures(kf) once per
// keyframe, next to touchDescriptors(kf); forget(kf) erases the span; fuseSearch is the search of OrbMatcher::fuseByProjection /
// fuseBySim3 for several target keyframes in ONE call (orbMatcher.hpp's overloads over a mirror run the bookkeeping on its result);
// verifyFeatures() is verify() for them.  It needs enableAttributes() too.  Assumed spellings beyond the others: KeyFrame m_v_keyPoints
// (the undistorted keypoints, cv::KeyPoint) and m_v_rightXcords, of one length with m_cvMat_descriptors' rows.
// enableBow() adds the keyframes' BoW feature vectors: touchBow(kf) once per keyframe, next to touchFeatures(kf);
// forget(kf) erases the span; createNewPoints is the search and the geometry of LocalMapping::createNewMapPoints for all neighbours in
// ONE call (localMapping.hpp's overload over a mirror runs the bookkeeping on its result); verifyBow() is verify() for them.  It needs
// enableFeatures() and the descriptor blocks too.  Assumed spelling beyond the others: KeyFrame m_bow_keyPointsVec (DBoW3::FeatureVector).
// searchByBowKeyFrames / searchByBowFrame are OrbMatcher::searchByBowInTwoKeyFrames / searchByBowInKeyFrameAndFrame for all candidate
// keyframes of a loop or relocalisation round in ONE call each (orbMatcher.hpp's overloads over a mirror build
// the frame's side and hand the match vectors on).  They need enableDescriptors(), enableFeatures() and enableBow() and no new touch.
// localBaGraph(localKeyFrames) is the flat graph of Optimizer::localBundleAdjust assembled on the table in ONE call (DESIGN.md section
// 6u; optimizer.hpp's overload over a mirror fills the poses, solves and runs the write-back with its touches).  It needs
// enableDescriptors() and enableFeatures().  Assumed spelling beyond the others: KeyFrame m_v_invScaleFactorSquares.
// Assumed spellings: those of mapPoint.hpp; m_cvMat_descriptors (one CV_8U row of 32 bytes per keypoint) for the blocks, keyFrame.hpp and localMapping.hpp; for the three correction methods also optimizer.hpp's
// MapPoint::setPosInWorld(cv::Mat), m_int_correctedByKeyFrameID, m_int_correctedReference and the Sim3 members rotation().x() .. w(),
// translation()[k], scale().  The camera centre after a corrected pose is not read from a member: correctLoopPoints computes it from
// the corrected Sim3 as setPose would (see there), correctAfterEssentialGraph reads getCameraOriginInWorld() after the caller's setPose.
#ifndef YDORB_ADAPTER_MAPMIRROR_HPP
#define YDORB_ADAPTER_MAPMIRROR_HPP

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

#include <opencv2/core.hpp>

#include "c_api.h"
#include "mapPoint.hpp"

namespace ydorb {
namespace adapter {

template <class KeyFramePtr, class MapPointPtr>
class MapMirror {
 public:
  explicit MapMirror(int device = 0, int32_t pointCapacity = 1 << 16, int32_t keyFrameCapacity = 1024, int64_t observationCapacity = 1 << 19) {
    mapCheck(ydorb_mapdb_create(device, pointCapacity, keyFrameCapacity, observationCapacity, &db_));
  }
  ~MapMirror() { ydorb_mapdb_destroy(db_); }
  MapMirror(const MapMirror&) = delete;
  MapMirror& operator=(const MapMirror&) = delete;

  ydorb_mapdb_t* handle() const { return db_; }
  int32_t slotOf(const MapPointPtr& mp) const { const auto it = pointSlot_.find(mp); return it == pointSlot_.end() ? -1 : it->second; }
  int32_t slotOf(const KeyFramePtr& kf) const { const auto it = kfSlot_.find(kf); return it == kfSlot_.end() ? -1 : it->second; }

  void touch(const MapPointPtr& mp) { mark(pointDirty_, dirtyPoints_, pointSlotFor(mp), kFull); }
  void touchPosition(const MapPointPtr& mp) { mark(pointDirty_, dirtyPoints_, pointSlotFor(mp), kPos); }
  void touch(const KeyFramePtr& kf) { mark(kfDirty_, dirtyKfs_, kfSlotFor(kf), kFull); }
  void forget(const MapPointPtr& mp) {
    const auto it = pointSlot_.find(mp);
    if (it == pointSlot_.end()) return;
    const int32_t s = it->second;
    pointSlot_.erase(it);
    pointOf_[s] = MapPointPtr();
    freePoints_.push_back(s);
    if (attributes_) erasePending_[s] = 1;
    mark(pointDirty_, dirtyPoints_, s, kFull);   // the next flush erases it, or writes the point that took the slot since
  }
  // Resident descriptors.  The capacities (views, descriptors) size the two pools when given; both pools grow on demand anyway.
  void enableDescriptors(int64_t viewCapacity = 0, int64_t descriptorCapacity = 0) {
    descriptors_ = true;
    if (viewCapacity > 0 || descriptorCapacity > 0) mapCheck(ydorb_mapdb_reserve_descriptors(db_, viewCapacity, descriptorCapacity));
  }
  bool descriptorsEnabled() const { return descriptors_; }
  // re-reads m_cvMat_descriptors at the next flush: once per keyframe, its descriptors never change; again after setBadFlag(), whose
  // isBad() empties the block (or forget(kf))
  void touchDescriptors(const KeyFramePtr& kf) { mark(descDirty_, dirtyDescs_, kfSlotFor(kf), kFull); }
  // Resident point attributes: normal, raw distances and descriptor of every point stay in the table, and
  // searchLocalPoints below reads them by slot.  Enable it before the first touch.
  void enableAttributes() {
    mapCheck(ydorb_mapdb_enable_attributes(db_));
    attributes_ = true;
  }
  // re-reads getNormal(), getMinDistance(), getMaxDistance() and getDescriptor() at the next flush: after a constructor or replace() set
  // them on the host.  What updateNormalAndDepth, the three correction methods and computeDistinctiveDescriptors of this class compute
  // is in the table already (write-through) and needs no touch.
  void touchAttributes(const MapPointPtr& mp) {
    mark(attrDirty_, dirtyAttrs_, known(mp), kFull);
  }
  // Resident keyframe features: fuseSearch below reads a target keyframe's keypoints, right coordinates and
  // descriptor block by slot.  Enable it, and the attributes, before the first touch.
  void enableFeatures() {
    mapCheck(ydorb_mapdb_enable_features(db_));
    features_ = true;
  }
  bool featuresEnabled() const { return features_; }
  // re-reads m_v_keyPoints and m_v_rightXcords at the next flush: once per keyframe, they never change; again after setBadFlag(), whose
  // isBad() erases the span (or forget(kf))
  void touchFeatures(const KeyFramePtr& kf) { mark(featDirty_, dirtyFeats_, kfSlotFor(kf), kFull); }
  // Resident BoW feature vectors: createNewPoints below reads a keyframe's feature vector by slot.
  void enableBow() {
    mapCheck(ydorb_mapdb_enable_bow(db_));
    bow_ = true;
  }
  bool bowEnabled() const { return bow_; }
  // re-reads m_bow_keyPointsVec at the next flush: once per keyframe, it never changes; again after setBadFlag(), whose isBad() erases
  // the span (or forget(kf))
  void touchBow(const KeyFramePtr& kf) { mark(bowDirty_, dirtyBows_, kfSlotFor(kf), kFull); }
  void touchRow(const KeyFramePtr& kf) { markRow(kfSlotFor(kf)); }
  void touchEntry(const KeyFramePtr& kf, size_t idx) {
    const int32_t s = kfSlotFor(kf);
    if (!rowSent_[s]) { markRow(s); return; }   // the table has no row to change yet: the whole row goes
    if (!rowDirty_[s]) dirtyEntries_.push_back(std::make_pair(s, (int32_t)idx));
  }
  void forget(const KeyFramePtr& kf) {
    const auto it = kfSlot_.find(kf);
    if (it == kfSlot_.end()) return;
    kfOf_[it->second] = KeyFramePtr();
    if (rowSent_[it->second]) markRow(it->second);   // the next flush empties the row, or writes the row of the keyframe that took the slot since
    if (descSent_[it->second]) mark(descDirty_, dirtyDescs_, it->second, kFull);   // ... and the block
    if (featSent_[it->second]) mark(featDirty_, dirtyFeats_, it->second, kFull);   // ... and the features
    if (bowSent_[it->second]) mark(bowDirty_, dirtyBows_, it->second, kFull);      // ... and the feature vector
    freeKfs_.push_back(it->second);
    kfSlot_.erase(it);
  }
  void clear() {   // Map::clear
    mapCheck(ydorb_mapdb_clear(db_));
    pointSlot_.clear(); pointOf_.clear(); freePoints_.clear(); pointDirty_.clear(); dirtyPoints_.clear(); span_.clear();
    kfSlot_.clear(); kfOf_.clear(); freeKfs_.clear(); kfDirty_.clear(); dirtyKfs_.clear();
    rowDirty_.clear(); rowSent_.clear(); dirtyRows_.clear(); dirtyEntries_.clear();
    descDirty_.clear(); descSent_.clear(); dirtyDescs_.clear();
    featDirty_.clear(); featSent_.clear(); dirtyFeats_.clear();
    bowDirty_.clear(); bowSent_.clear(); dirtyBows_.clear();
    attrDirty_.clear(); dirtyAttrs_.clear(); erasePending_.clear();
  }

  // At most one call of each set_* entry: the centres first (a point may name a keyframe that got its slot while the point was read).
  // The rows are read first (a row may name a point the mirror meets there for the first time) and sent last, after the points.
  void flush() {
    std::vector<int32_t> rowKf, rowStart{0}, rowSlots, entKf, entIdx, entSlot;
    for (const int32_t k : dirtyRows_) {
      rowKf.push_back(k);
      if (kfOf_[k])
        for (const MapPointPtr& mp : kfOf_[k]->getMapPointMatches()) rowSlots.push_back(mp ? known(mp) : -1);
      if (rowSlots.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX row entries in one flush");
      rowStart.push_back((int32_t)rowSlots.size());
      rowSent_[k] = kfOf_[k] ? 1 : 0;
    }
    int32_t readKf = -1;
    std::vector<MapPointPtr> matches;
    for (const std::pair<int32_t, int32_t>& e : dirtyEntries_) {
      if (rowDirty_[e.first] || !kfOf_[e.first]) continue;   // the whole row travels, or the keyframe is gone
      if (readKf != e.first) { matches = kfOf_[e.first]->getMapPointMatches(); readKf = e.first; }   // one copy per run of a keyframe's entries
      const MapPointPtr mp = matches.at((size_t)e.second);
      entKf.push_back(e.first); entIdx.push_back(e.second); entSlot.push_back(mp ? known(mp) : -1);
    }
    for (const int32_t k : dirtyRows_) rowDirty_[k] = kClean;
    dirtyRows_.clear(); dirtyEntries_.clear();
    std::vector<int32_t> slots, start{0}, obsKf, refKf, posSlots;
    std::vector<uint8_t> obsLevel, bad, refLevel;
    std::vector<float> pos, posOnly;
    std::vector<int32_t> viewStart{0}, viewKf, viewIdx;   // with descriptors enabled: the views of the points in `slots`
    for (const int32_t s : dirtyPoints_) {
      const uint8_t how = pointDirty_[s];
      pointDirty_[s] = kClean;
      if (how == kPos && pointOf_[s]) {
        posSlots.push_back(s);
        const cv::Mat P = pointOf_[s]->getPosInWorld();
        for (int r = 0; r < 3; r++) posOnly.push_back(P.template at<float>(r));
        continue;
      }
      if (!pointOf_[s] && kfOf_.empty()) continue;   // no keyframe was ever named: nothing of this slot reached the table
      const auto send = [&](const Record& rec) {
        slots.push_back(s);
        obsKf.insert(obsKf.end(), rec.kf.begin(), rec.kf.end()); obsLevel.insert(obsLevel.end(), rec.level.begin(), rec.level.end());
        if (obsKf.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX observations in one flush");
        start.push_back((int32_t)obsKf.size());
        bad.push_back(rec.bad); refKf.push_back(rec.refKf); refLevel.push_back(rec.refLevel);
        pos.insert(pos.end(), rec.pos, rec.pos + 3);
        span_[s] = (int32_t)rec.kf.size();
        if (descriptors_) {
          viewKf.insert(viewKf.end(), rec.kf.begin(), rec.kf.end()); viewIdx.insert(viewIdx.end(), rec.idx.begin(), rec.idx.end());
          viewStart.push_back((int32_t)viewKf.size());
          for (const int32_t k : rec.kf)   // a keyframe met here for the first time: its block is read now
            if (!descSent_[k]) mark(descDirty_, dirtyDescs_, k, kFull);
        }
      };
      // A slot forgotten and taken again since the last flush: the erased record goes first in the same call (of a slot named twice
      // the table keeps the last record), so that the attributes of the point that left are cleared and the slot reads as "no
      // attributes" until the new point's are set.
      if (pointOf_[s] && erasePending_[s]) send(Record());
      erasePending_[s] = 0;
      send(pointOf_[s] ? read(pointOf_[s], true) : Record());
    }
    dirtyPoints_.clear();
    if (!dirtyKfs_.empty()) {
      std::vector<int32_t> ks;
      std::vector<float> centre;
      for (const int32_t k : dirtyKfs_) {
        kfDirty_[k] = kClean;
        if (!kfOf_[k]) continue;   // forgotten since: the slot keeps its last centre until it is taken again
        ks.push_back(k);
        const cv::Mat O = kfOf_[k]->getCameraOriginInWorld();
        for (int r = 0; r < 3; r++) centre.push_back(O.template at<float>(r));
      }
      dirtyKfs_.clear();
      if (!ks.empty()) mapCheck(ydorb_mapdb_set_centres(db_, ks.data(), (int32_t)ks.size(), centre.data()));
    }
    if (!slots.empty())
      mapCheck(ydorb_mapdb_set_points(db_, slots.data(), (int32_t)slots.size(), start.data(), obsKf.data(), obsLevel.data(), bad.data(), refKf.data(),
                                      refLevel.data(), pos.data()));
    if (!posSlots.empty()) mapCheck(ydorb_mapdb_set_positions(db_, posSlots.data(), (int32_t)posSlots.size(), posOnly.data()));
    if (!rowKf.empty()) mapCheck(ydorb_mapdb_set_keyframe_rows(db_, rowKf.data(), (int32_t)rowKf.size(), rowStart.data(), rowSlots.data()));
    if (!entKf.empty()) mapCheck(ydorb_mapdb_set_row_entries(db_, entKf.data(), entIdx.data(), entSlot.data(), (int32_t)entKf.size()));
    if (!dirtyDescs_.empty()) {   // the blocks before the views, both after the points: a view names a point slot the table holds
      std::vector<int32_t> ks, descStart{0};
      std::vector<uint8_t> desc;
      for (const int32_t k : dirtyDescs_) {
        descDirty_[k] = kClean;
        const bool live = kfOf_[k] && !kfOf_[k]->isBad();   // a bad keyframe's observations are skipped: it holds no block
        if (!live && !descSent_[k]) continue;
        ks.push_back(k);
        if (live) appendDescriptors(kfOf_[k], desc);
        if (desc.size() / 32 > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX descriptors in one flush");
        descStart.push_back((int32_t)(desc.size() / 32));
        descSent_[k] = live ? 1 : 0;
      }
      dirtyDescs_.clear();
      desc.resize(desc.size() + 32);   // never a null pointer
      if (!ks.empty()) mapCheck(ydorb_mapdb_set_keyframe_descriptors(db_, ks.data(), (int32_t)ks.size(), descStart.data(), desc.data()));
    }
    if (!dirtyFeats_.empty()) {   // after the blocks: a query reads a keyframe's features and its block together
      std::vector<int32_t> ks, featStart{0};
      std::vector<YdKeyPoint> kps;
      std::vector<float> rightX;
      for (const int32_t k : dirtyFeats_) {
        featDirty_[k] = kClean;
        const bool live = kfOf_[k] && !kfOf_[k]->isBad();
        if (!live && !featSent_[k]) continue;
        ks.push_back(k);
        if (live) appendFeatures(kfOf_[k], kps, rightX);
        if (kps.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX features in one flush");
        featStart.push_back((int32_t)kps.size());
        featSent_[k] = live ? 1 : 0;
      }
      dirtyFeats_.clear();
      kps.resize(kps.size() + 1); rightX.resize(rightX.size() + 1);   // never a null pointer
      if (!ks.empty()) mapCheck(ydorb_mapdb_set_keyframe_features(db_, ks.data(), (int32_t)ks.size(), featStart.data(), kps.data(), rightX.data()));
    }
    if (!dirtyBows_.empty()) {   // after the features: a query reads a keyframe's feature vector against its feature count
      std::vector<int32_t> ks, bowStart{0}, feat;
      std::vector<uint32_t> node;
      for (const int32_t k : dirtyBows_) {
        bowDirty_[k] = kClean;
        const bool live = kfOf_[k] && !kfOf_[k]->isBad();
        if (!live && !bowSent_[k]) continue;
        ks.push_back(k);
        if (live) appendBow(kfOf_[k], node, feat);
        if (feat.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX BoW entries in one flush");
        bowStart.push_back((int32_t)feat.size());
        bowSent_[k] = live ? 1 : 0;
      }
      dirtyBows_.clear();
      node.resize(node.size() + 1); feat.resize(feat.size() + 1);   // never a null pointer
      if (!ks.empty()) mapCheck(ydorb_mapdb_set_keyframe_bow(db_, ks.data(), (int32_t)ks.size(), bowStart.data(), node.data(), feat.data()));
    }
    if (descriptors_ && !slots.empty()) {
      viewKf.push_back(0); viewIdx.push_back(0);
      mapCheck(ydorb_mapdb_set_point_views(db_, slots.data(), (int32_t)slots.size(), viewStart.data(), viewKf.data(), viewIdx.data()));
    }
    if (!dirtyAttrs_.empty()) {   // after the points: an erased point's clear is staged by set_points, a reused slot's values follow it
      // Each group only where the member is set: a point made from a keyframe has no descriptor until computeDistinctiveDescriptors,
      // and one whose normal is still empty has no geometry.  Hence up to two calls, one per group.
      std::vector<int32_t> geoSlots, descSlots;
      std::vector<float> normal, minD, maxD;
      std::vector<uint8_t> desc;
      for (const int32_t s : dirtyAttrs_) {
        attrDirty_[s] = kClean;
        if (!pointOf_[s]) continue;   // forgotten since
        const size_t g = minD.size(), d = desc.size();
        appendAttributes(pointOf_[s], normal, minD, maxD, desc);
        if (minD.size() > g) geoSlots.push_back(s);
        if (desc.size() > d) descSlots.push_back(s);
      }
      dirtyAttrs_.clear();
      if (!geoSlots.empty())
        mapCheck(ydorb_mapdb_set_point_attributes(db_, geoSlots.data(), (int32_t)geoSlots.size(), normal.data(), minD.data(), maxD.data(), nullptr));
      if (!descSlots.empty())
        mapCheck(ydorb_mapdb_set_point_attributes(db_, descSlots.data(), (int32_t)descSlots.size(), nullptr, nullptr, nullptr, desc.data()));
    }
  }

  // The device part of Tracking::searchLocalPoints for a list of local map points (ydorb_mapdb_search_local_points): resolves the
  // pointers to slots, flushes, and makes the one call.  skip [n] = the caller's flags (a point seen in this frame already); the table
  // adds its own bad flag.  taken / assigned as ydorb_search_local_points takes them; assigned[idx] indexes localMapPoints.  Returns the
  // number of matches; nToMatch = the points in view.
  int searchLocalPoints(ydorb_matcher_t* matcher, const YdFrameView& frame, const YdFrustumView& view, const std::vector<MapPointPtr>& localMapPoints,
                        const std::vector<uint8_t>& skip, float th, float ratio, std::vector<uint8_t>& taken, std::vector<int32_t>& assigned,
                        std::vector<YdTrackView>& rows, std::vector<uint8_t>& status, int32_t& nToMatch) {
    if (!attributes_) throw std::runtime_error("ydorb: searchLocalPoints without enableAttributes()");
    const size_t n = localMapPoints.size();
    std::vector<int32_t> slots(n + 1);
    for (size_t i = 0; i < n; i++) slots[i] = known(localMapPoints[i]);
    flush();
    rows.resize(n + 1); status.resize(n + 1);
    int32_t nMatches = 0;
    nToMatch = 0;
    std::vector<uint8_t> sk(skip);
    sk.resize(n + 1, 0);
    mapCheck(ydorb_mapdb_search_local_points(db_, matcher, &frame, &view, slots.data(), (int32_t)n, sk.data(), th, ratio, taken.data(), assigned.data(),
                                             rows.data(), status.data(), &nToMatch, &nMatches));
    rows.resize(n); status.resize(n);
    return nMatches;
  }

  // The search of OrbMatcher::fuseByProjection / fuseBySim3 for several target keyframes in one call (ydorb_mapdb_fuse_search): target
  // t searches points[t] in keyFrames[t].  targets[t] holds the view, sigma table, th, max_dist and flags (orbMatcher.hpp's fuseTarget
  // builds it); its kf_slot is set here.  skip[t][i] = the caller's byte for points[t][i]; a null entry is skipped whatever its byte.
  // A keyframe the table holds no features or block of is read now.  Resolves pointers to slots, flushes, makes the one call.
  struct FuseResult {
    std::vector<std::vector<int32_t> > best;      // per target and list entry: the keyframe's feature index, or -1
    std::vector<std::vector<uint8_t> > status;    // YDORB_FUSE_*
    std::vector<int32_t> nFound;
    std::vector<uint8_t> targetStatus;            // YDORB_FUSE_TARGET_*
  };
  FuseResult fuseSearch(ydorb_matcher_t* matcher, const std::vector<KeyFramePtr>& keyFrames, std::vector<YdFuseTarget>& targets,
                        const std::vector<std::vector<MapPointPtr> >& points, const std::vector<std::vector<uint8_t> >& skip) {
    if (!attributes_ || !features_) throw std::runtime_error("ydorb: fuseSearch without enableAttributes() and enableFeatures()");
    const size_t nt = keyFrames.size();
    if (targets.size() != nt || points.size() != nt || skip.size() != nt) throw std::runtime_error("ydorb: fuseSearch: one target, list and skip list per keyframe");
    std::vector<int32_t> listStart(1, 0), slots;
    std::vector<uint8_t> sk;
    std::vector<std::vector<int32_t> > at(nt);   // per target: the list index of each entry sent (null entries are not sent)
    for (size_t t = 0; t < nt; t++) {
      const int32_t k = kfSlotFor(keyFrames[t]);
      targets[t].kf_slot = k;
      if (!featSent_[k]) mark(featDirty_, dirtyFeats_, k, kFull);
      if (!descSent_[k]) mark(descDirty_, dirtyDescs_, k, kFull);
      for (size_t i = 0; i < points[t].size(); i++) {
        if (!points[t][i]) continue;
        slots.push_back(known(points[t][i]));
        sk.push_back(i < skip[t].size() ? skip[t][i] : 0);
        at[t].push_back((int32_t)i);
      }
      if (slots.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX fuse entries");
      listStart.push_back((int32_t)slots.size());
    }
    flush();
    FuseResult r;
    r.nFound.assign(nt + 1, 0); r.targetStatus.assign(nt + 1, 0);
    const size_t L = slots.size();
    std::vector<int32_t> best(L + 1, -1);
    std::vector<uint8_t> status(L + 1, YDORB_FUSE_SKIPPED);
    slots.resize(L + 1); sk.resize(L + 1);
    if (nt > 0)
      mapCheck(ydorb_mapdb_fuse_search(db_, matcher, targets.data(), (int32_t)nt, listStart.data(), slots.data(), sk.data(), best.data(), status.data(),
                                       r.nFound.data(), r.targetStatus.data()));
    r.nFound.resize(nt); r.targetStatus.resize(nt);
    r.best.resize(nt); r.status.resize(nt);
    for (size_t t = 0; t < nt; t++) {
      r.best[t].assign(points[t].size(), -1); r.status[t].assign(points[t].size(), YDORB_FUSE_SKIPPED);
      for (size_t j = 0; j < at[t].size(); j++) {
        r.best[t][(size_t)at[t][j]] = best[(size_t)listStart[t] + j];
        r.status[t][(size_t)at[t][j]] = status[(size_t)listStart[t] + j];
      }
    }
    return r;
  }

  // The search and the geometry of LocalMapping::createNewMapPoints for all neighbours in one call (ydorb_mapdb_create_new_points):
  // first / neighbours hold the views' constants (localMapping.hpp's createView builds them); their kf_slot, n and depth are set here
  // from the keyframes.  A keyframe the table holds no row, features, block or feature vector of is read now.  Flushes, makes the call.
  struct CreateResult {
    int32_t n = 0;                        // the first keyframe's feature count: the stride of the three dense arrays
    std::vector<int32_t> matchedSecond;   // [nNb][n]
    std::vector<float> x3d;               // [nNb][n][3]
    std::vector<uint8_t> status;          // [nNb][n]
    std::vector<int32_t> nMatches, nAccepted;
    std::vector<uint8_t> neighbourStatus; // YDORB_CREATE_NB_*
  };
  CreateResult createNewPoints(ydorb_matcher_t* matcher, const KeyFramePtr& current, const std::vector<KeyFramePtr>& neighbourKfs, YdCreateView first,
                               std::vector<YdCreateNeighbour> neighbours, bool stereoOnly, bool checkOrientation) {
    if (!features_ || !bow_ || !descriptors_) throw std::runtime_error("ydorb: createNewPoints without enableDescriptors(), enableFeatures() and enableBow()");
    const size_t nn = neighbourKfs.size();
    if (neighbours.size() != nn) throw std::runtime_error("ydorb: createNewPoints: one neighbour record per keyframe");
    const auto bind = [this](const KeyFramePtr& kf, YdCreateView& v) {
      const int32_t k = kfSlotFor(kf);
      v.kf_slot = k; v.n = (int32_t)kf->m_v_depth.size(); v.depth = kf->m_v_depth.data();
      if (!rowSent_[k]) markRow(k);
      if (!featSent_[k]) mark(featDirty_, dirtyFeats_, k, kFull);
      if (!descSent_[k]) mark(descDirty_, dirtyDescs_, k, kFull);
      if (!bowSent_[k]) mark(bowDirty_, dirtyBows_, k, kFull);
    };
    bind(current, first);
    for (size_t i = 0; i < nn; i++) bind(neighbourKfs[i], neighbours[i].view);
    flush();
    CreateResult r;
    r.n = first.n;
    const size_t cells = nn * (size_t)first.n;
    r.matchedSecond.assign(cells + 1, -1); r.x3d.assign(3 * cells + 3, 0.f); r.status.assign(cells + 1, YDORB_TRI_UNMATCHED);
    r.nMatches.assign(nn + 1, 0); r.nAccepted.assign(nn + 1, 0); r.neighbourStatus.assign(nn + 1, 0);
    neighbours.resize(nn + 1);
    mapCheck(ydorb_mapdb_create_new_points(db_, matcher, &first, neighbours.data(), (int32_t)nn, stereoOnly ? 1 : 0, checkOrientation ? 1 : 0,
                                           r.matchedSecond.data(), r.x3d.data(), r.status.data(), r.nMatches.data(), r.nAccepted.data(),
                                           r.neighbourStatus.data()));
    r.nMatches.resize(nn); r.nAccepted.resize(nn); r.neighbourStatus.resize(nn);
    return r;
  }

  // OrbMatcher::searchByBowInTwoKeyFrames(kf1, kf2s[i]) for all candidates of a loop round in one call
  // (ydorb_mapdb_search_by_bow_keyframes), and searchByBowInKeyFrameAndFrame(kfs[i], frame) for all candidates of a relocalisation in
  // one call (ydorb_mapdb_search_by_bow_frame; one keyframe: trackReferenceKeyFrame).  A keyframe the table holds no row, features,
  // block or feature vector of is read now, as in createNewPoints.  Flushes, makes the call.  matched[i] is the vector the reference
  // fills for candidate i: per feature of kf1 (keyframes) or of the frame (frame) the matched map point or null; nMatches[i] the
  // reference's return value.  "Has a good map point" is the table's: touch(mp) after setBadFlag(), touchRow / touchEntry after a row
  // changes.  The candidates are independent of each other: one may be named twice, and kf1 may be among them.
  struct BowSearchResult {
    std::vector<std::vector<MapPointPtr>> matched;
    std::vector<int> nMatches;
    std::vector<uint8_t> pairStatus;   // YDORB_BOW_PAIR_*: a candidate with a non-zero status was not searched
  };
  BowSearchResult searchByBowKeyFrames(ydorb_matcher_t* matcher, const KeyFramePtr& kf1, const std::vector<KeyFramePtr>& kf2s, float ratio, bool checkOrientation) {
    if (!features_ || !bow_ || !descriptors_) throw std::runtime_error("ydorb: searchByBowKeyFrames without enableDescriptors(), enableFeatures() and enableBow()");
    const int32_t first = bindForBow(kf1);
    std::vector<int32_t> second;
    for (const KeyFramePtr& kf : kf2s) second.push_back(bindForBow(kf));
    flush();
    // n_first is the table's count: a bad kf1 holds no features after the flush (computeSim3 never passes one), so every candidate
    // answers with YDORB_BOW_PAIR_NO_FEATURES and an all-null vector of kf1's length, as a bad candidate does, instead of a refusal
    const size_t np = kf2s.size(), full = kf1->m_v_keyPoints.size(), n = featSent_[first] ? full : 0;
    std::vector<int32_t> feature(np * n + 1, -1), point(np * n + 1, -1), count(np + 1, 0);
    std::vector<uint8_t> status(np + 1, 0);
    second.push_back(0);
    mapCheck(ydorb_mapdb_search_by_bow_keyframes(db_, matcher, first, second.data(), (int32_t)np, ratio, checkOrientation ? 1 : 0, (int32_t)n, feature.data(),
                                                 point.data(), count.data(), status.data()));
    return bowResult(np, n, full, point, count, status);
  }
  BowSearchResult searchByBowFrame(ydorb_matcher_t* matcher, const std::vector<KeyFramePtr>& kfs, const YdBowSide& frame, float ratio, bool checkOrientation) {
    if (!features_ || !bow_ || !descriptors_) throw std::runtime_error("ydorb: searchByBowFrame without enableDescriptors(), enableFeatures() and enableBow()");
    std::vector<int32_t> slots;
    for (const KeyFramePtr& kf : kfs) slots.push_back(bindForBow(kf));
    flush();
    const size_t np = kfs.size(), n = (size_t)(frame.n > 0 ? frame.n : 0);
    std::vector<int32_t> feature(np * n + 1, -1), point(np * n + 1, -1), count(np + 1, 0);
    std::vector<uint8_t> status(np + 1, 0);
    slots.push_back(0);
    mapCheck(ydorb_mapdb_search_by_bow_frame(db_, matcher, slots.data(), (int32_t)np, &frame, ratio, checkOrientation ? 1 : 0, feature.data(), point.data(), count.data(),
                                             status.data()));
    return bowResult(np, n, n, point, count, status);
  }

  // Flushes and compares every known keyframe's m_bow_keyPointsVec with the device's feature vectors (ydorb_mapdb_export_bow): the
  // keyframe slots that differ.  Empty when every keyframe was touched.
  std::vector<int32_t> verifyBow() {
    flush();
    YdMapDbStats st;
    YdMapDbBowStats bs;
    mapCheck(ydorb_mapdb_stats(db_, &st));
    mapCheck(ydorb_mapdb_bow_stats(db_, &bs));
    const size_t nk = (size_t)st.n_keyframes;
    std::vector<int32_t> start(nk + 1), feat((size_t)bs.n_entries + 1);
    std::vector<uint32_t> node((size_t)bs.n_entries + 1);
    mapCheck(ydorb_mapdb_export_bow(db_, start.data(), node.data(), feat.data()));
    std::vector<int32_t> differ;
    for (size_t k = 0; k < kfOf_.size(); k++) {
      std::vector<uint32_t> wantNode;
      std::vector<int32_t> wantFeat;
      if (kfOf_[k] && bowSent_[k] && !kfOf_[k]->isBad()) appendBow(kfOf_[k], wantNode, wantFeat);
      const size_t len = k < nk ? (size_t)(start[k + 1] - start[k]) : 0;
      if (len != wantFeat.size() || (len > 0 && (std::memcmp(&node[(size_t)start[k]], wantNode.data(), 4 * len) != 0 ||
                                                 std::memcmp(&feat[(size_t)start[k]], wantFeat.data(), 4 * len) != 0)))
        differ.push_back((int32_t)k);
    }
    return differ;
  }

  // Flushes and compares every known keyframe's m_v_keyPoints and m_v_rightXcords with the device's features
  // (ydorb_mapdb_export_features): the keyframe slots that differ.  Empty when every keyframe was touched.
  std::vector<int32_t> verifyFeatures() {
    flush();
    YdMapDbStats st;
    YdMapDbFeatStats fs;
    mapCheck(ydorb_mapdb_stats(db_, &st));
    mapCheck(ydorb_mapdb_feat_stats(db_, &fs));
    const size_t nk = (size_t)st.n_keyframes;
    std::vector<int32_t> start(nk + 1);
    std::vector<YdKeyPoint> kps((size_t)fs.n_features + 1);
    std::vector<float> rightX((size_t)fs.n_features + 1);
    mapCheck(ydorb_mapdb_export_features(db_, start.data(), kps.data(), rightX.data()));
    std::vector<int32_t> differ;
    for (size_t k = 0; k < kfOf_.size(); k++) {
      std::vector<YdKeyPoint> wantKps;
      std::vector<float> wantRx;
      if (kfOf_[k] && featSent_[k] && !kfOf_[k]->isBad()) appendFeatures(kfOf_[k], wantKps, wantRx);
      const size_t len = k < nk ? (size_t)(start[k + 1] - start[k]) : 0;
      if (len != wantKps.size() || (len > 0 && (std::memcmp(&kps[(size_t)start[k]], wantKps.data(), sizeof(YdKeyPoint) * len) != 0 ||
                                                 std::memcmp(&rightX[(size_t)start[k]], wantRx.data(), 4 * len) != 0)))
        differ.push_back((int32_t)k);
    }
    return differ;
  }

  // Flushes and compares every known point's getNormal(), getMinDistance(), getMaxDistance() and getDescriptor() with the device's
  // attributes (ydorb_mapdb_export_attributes): the point slots that differ in a group whose flag is set, and the slots of points that
  // are not bad and lack a flag (the search reports those as YDORB_FRUSTUM_NO_ATTRIBUTES).  Empty when every host-side change was touched.
  std::vector<int32_t> verifyAttributes() {
    flush();
    YdMapDbStats st;
    mapCheck(ydorb_mapdb_stats(db_, &st));
    const size_t np = (size_t)st.n_points;
    std::vector<float> normal(3 * np + 3), minD(np + 1), maxD(np + 1);
    std::vector<uint8_t> desc(32 * np + 32), flags(np + 1);
    mapCheck(ydorb_mapdb_export_attributes(db_, normal.data(), minD.data(), maxD.data(), desc.data(), flags.data()));
    std::vector<int32_t> differ;
    for (size_t s = 0; s < pointOf_.size(); s++) {
      if (!pointOf_[s]) continue;
      if (s >= np) { differ.push_back((int32_t)s); continue; }
      std::vector<float> n3, mn, mx;
      std::vector<uint8_t> d;
      appendAttributes(pointOf_[s], n3, mn, mx, d);
      bool same = pointOf_[s]->isBad() || flags[s] == 3;
      if (flags[s] & 1)   // a flag the object has no member for is a difference
        same = same && !mn.empty() && std::memcmp(&normal[3 * s], n3.data(), 12) == 0 && std::memcmp(&minD[s], mn.data(), 4) == 0 && std::memcmp(&maxD[s], mx.data(), 4) == 0;
      if (flags[s] & 2) same = same && !d.empty() && std::memcmp(&desc[32 * s], d.data(), 32) == 0;
      if (!same) differ.push_back((int32_t)s);
    }
    return differ;
  }

  // MapPoint::computeDistinctiveDescriptors for every point of `points` over the resident table (ydorb_mapdb_distinctive_descriptors):
  // apply(mp, kf, idx, row) for every point the reference would have given a new m_descriptor, each distinct point once, in the order of
  // `points`; row (1x32 CV_8U) = kf->m_cvMat_descriptors.row(idx), the winning descriptor, which the caller stores as m_descriptor.
  // A bad point and a point none of whose observing keyframes is alive are left alone, as in the reference.  Returns their number.
  template <class Points, class Apply>
  int computeDistinctiveDescriptors(const Points& points, Apply apply) {
    if (!descriptors_) throw std::runtime_error("ydorb: computeDistinctiveDescriptors without enableDescriptors()");
    std::vector<int32_t> slots;
    std::vector<MapPointPtr> asked;
    std::vector<uint8_t> seen(pointOf_.size(), 0);
    for (const MapPointPtr& mp : points) {
      if (!mp) continue;
      const int32_t s = known(mp);
      if ((size_t)s >= seen.size()) seen.resize((size_t)s + 1, 0);
      if (seen[s]) continue;
      seen[s] = 1;
      slots.push_back(s);
      asked.push_back(mp);
    }
    flush();
    const size_t n = slots.size();
    if (n == 0) return 0;
    std::vector<int32_t> best(n), view(2 * n);
    std::vector<uint8_t> desc(32 * n), status(n);
    mapCheck(ydorb_mapdb_distinctive_descriptors(db_, slots.data(), (int32_t)n, best.data(), view.data(), desc.data(), status.data()));
    int updated = 0;
    for (size_t p = 0; p < n; p++) {
      if (status[p] == YDORB_MAPDESC_VIEW_OUT_OF_RANGE) throw std::runtime_error("ydorb: a view names a keypoint past its keyframe's descriptors");
      if (status[p] != YDORB_MAPDESC_UPDATED) continue;
      cv::Mat row(1, 32, CV_8U);
      std::memcpy(row.template ptr<unsigned char>(), &desc[32 * p], 32);
      apply(asked[p], kfOf_[view[2 * p]], (size_t)view[2 * p + 1], row);
      updated++;
    }
    return updated;
  }

  struct Difference {   // of verify() and of verifyDescriptors()
    std::vector<int32_t> pointSlots, keyFrameSlots;
    bool empty() const { return pointSlots.empty() && keyFrameSlots.empty(); }
  };
  // Flushes, re-reads every known point's observations and every known keyframe's descriptors and compares them with the device's views
  // and blocks (ydorb_mapdb_export_views / _descriptors): the point slots whose views differ and the keyframe slots whose block differs.
  Difference verifyDescriptors() {
    flush();
    YdMapDbStats st;
    YdMapDbDescStats ds;
    mapCheck(ydorb_mapdb_stats(db_, &st));
    mapCheck(ydorb_mapdb_desc_stats(db_, &ds));
    const size_t np = (size_t)st.n_points, nk = (size_t)st.n_keyframes;
    std::vector<int32_t> vStart(np + 1), vKf((size_t)ds.n_views + 1), vIdx((size_t)ds.n_views + 1), dStart(nk + 1);
    std::vector<uint8_t> desc(32 * ((size_t)ds.n_descriptors + 1));
    mapCheck(ydorb_mapdb_export_views(db_, vStart.data(), vKf.data(), vIdx.data()));
    mapCheck(ydorb_mapdb_export_descriptors(db_, dStart.data(), desc.data()));
    Difference d;
    for (size_t s = 0; s < pointOf_.size(); s++) {
      const Record want = pointOf_[s] ? read(pointOf_[s], false) : Record();
      const size_t len = s < np ? (size_t)(vStart[s + 1] - vStart[s]) : 0;
      const bool same = len == want.kf.size() && (len == 0 || (std::memcmp(&vKf[vStart[s]], want.kf.data(), 4 * len) == 0 &&
                                                               std::memcmp(&vIdx[vStart[s]], want.idx.data(), 4 * len) == 0));
      if (!same) d.pointSlots.push_back((int32_t)s);
    }
    for (size_t k = 0; k < kfOf_.size(); k++) {
      std::vector<uint8_t> want;
      if (kfOf_[k] && descSent_[k] && !kfOf_[k]->isBad()) appendDescriptors(kfOf_[k], want);
      const size_t len = k < nk ? (size_t)(dStart[k + 1] - dStart[k]) : 0;
      if (32 * len != want.size() || (len > 0 && std::memcmp(&desc[32 * (size_t)dStart[k]], want.data(), 32 * len) != 0)) d.keyFrameSlots.push_back((int32_t)k);
    }
    return d;
  }

  // The counting loop of Tracking::updateLocalKeyFrames over the resident table (ydorb_mapdb_observer_counter): per keyframe how many
  // of the frame's map points it observes, a point listed twice counted twice.  Nulls nothing itself: badIndices receives the indices
  // of framePoints whose point is bad, which the reference nulls in the frame.
  std::map<KeyFramePtr, int> keyFrameCounter(const std::vector<MapPointPtr>& framePoints, std::vector<size_t>* badIndices = nullptr) {
    std::vector<int32_t> slots;
    for (const MapPointPtr& mp : framePoints) slots.push_back(mp ? known(mp) : -1);
    flush();
    std::map<KeyFramePtr, int> counter;
    if (badIndices) badIndices->clear();
    if (slots.empty()) return counter;
    const int32_t capacity = (int32_t)kfOf_.size();   // no list names more keyframes than the table has
    const int32_t listStart[2] = {0, (int32_t)slots.size()}, outStart[2] = {0, capacity};
    std::vector<int32_t> kf((size_t)capacity + 1), weight((size_t)capacity + 1);
    std::vector<uint8_t> pointBad(slots.size());
    int32_t count = 0;
    uint8_t status = 0;
    mapCheck(ydorb_mapdb_observer_counter(db_, 1, listStart, slots.data(), outStart, kf.data(), weight.data(), &count, &status, pointBad.data()));
    if (status != 0) throw std::runtime_error("ydorb: observer counter capacity bound violated");
    for (int32_t i = 0; i < count; i++)
      if (kfOf_[kf[i]]) counter[kfOf_[kf[i]]] = weight[i];
    if (badIndices)
      for (size_t i = 0; i < slots.size(); i++) if (pointBad[i]) badIndices->push_back(i);
    return counter;
  }

  // Tracking::updateLocalPoints over the keyframe rows (ydorb_mapdb_points_of_keyframes): every live point of the local keyframes'
  // map-point vectors once, in the reference's order.  seen[i] = 1 when the i-th returned point is among framePoints (the frame's own
  // matches, which searchLocalPoints skips).  A keyframe whose row the table never got is read now.
  std::vector<MapPointPtr> localPoints(const std::vector<KeyFramePtr>& localKeyFrames, const std::vector<MapPointPtr>& framePoints,
                                       std::vector<uint8_t>* seen = nullptr) {
    std::vector<int32_t> kfs, seenSlots;
    for (const KeyFramePtr& kf : localKeyFrames) {
      const int32_t s = kfSlotFor(kf);
      if (!rowSent_[s]) markRow(s);
      kfs.push_back(s);
    }
    for (const MapPointPtr& mp : framePoints) if (mp) seenSlots.push_back(known(mp));
    flush();
    std::vector<MapPointPtr> out;
    if (seen) seen->clear();
    if (kfs.empty()) return out;
    const int32_t capacity = (int32_t)pointOf_.size();   // each point at most once
    std::vector<int32_t> slots((size_t)capacity + 1);
    std::vector<uint8_t> flag((size_t)capacity + 1);
    int32_t count = 0;
    uint8_t status = 0;
    mapCheck(ydorb_mapdb_points_of_keyframes(db_, kfs.data(), (int32_t)kfs.size(), seenSlots.empty() ? nullptr : seenSlots.data(), (int32_t)seenSlots.size(),
                                             capacity, slots.data(), flag.data(), &count, &status));
    if (status != 0) throw std::runtime_error("ydorb: points-of-keyframes capacity bound violated");
    for (int32_t i = 0; i < count; i++) {
      out.push_back(pointOf_[slots[i]]);
      if (seen) seen->push_back(flag[i]);
    }
    return out;
  }

  // Flushes and compares every known keyframe's getMapPointMatches() with the device's row (ydorb_mapdb_export_rows): the keyframe
  // slots that differ.  Empty when every change was touched.
  std::vector<int32_t> verifyRows() {
    flush();
    YdMapDbStats st;
    YdMapDbRowStats rs;
    mapCheck(ydorb_mapdb_stats(db_, &st));
    mapCheck(ydorb_mapdb_row_stats(db_, &rs));
    const size_t nk = (size_t)st.n_keyframes;
    std::vector<int32_t> start(nk + 1), slot((size_t)rs.n_entries + 1);
    mapCheck(ydorb_mapdb_export_rows(db_, start.data(), slot.data()));
    std::vector<int32_t> differ;
    for (size_t k = 0; k < kfOf_.size(); k++) {
      std::vector<int32_t> want;
      if (kfOf_[k] && rowSent_[k])
        for (const MapPointPtr& mp : kfOf_[k]->getMapPointMatches()) want.push_back(mp ? (slotOf(mp) >= 0 ? slotOf(mp) : -2) : -1);
      const size_t len = k < nk ? (size_t)(start[k + 1] - start[k]) : 0;
      if (len != want.size() || (len > 0 && std::memcmp(&slot[start[k]], want.data(), 4 * len) != 0)) differ.push_back((int32_t)k);
    }
    return differ;
  }

  // updateNormalAndDepthBatch of mapPoint.hpp over the resident table: apply(mp, normal (3x1 CV_32F), minDistance, maxDistance) for every
  // point the reference would have updated, each distinct point once, in the order of `points`.  Returns their number.
  template <class Points, class Apply>
  int updateNormalAndDepth(const Points& points, Apply apply) {
    std::vector<int32_t> slots;
    std::vector<MapPointPtr> asked;
    std::vector<uint8_t> seen(pointOf_.size(), 0);
    for (const MapPointPtr& mp : points) {
      if (!mp) continue;
      const int32_t s = known(mp);
      if ((size_t)s >= seen.size()) seen.resize((size_t)s + 1, 0);
      if (seen[s]) continue;
      seen[s] = 1;
      slots.push_back(s);
      asked.push_back(mp);
    }
    flush();
    const size_t n = slots.size();
    if (n == 0) return 0;
    const std::vector<float> sf = scaleFactors();
    std::vector<float> normal(3 * n), minD(n), maxD(n);
    std::vector<uint8_t> status(n);
    mapCheck(ydorb_mapdb_update_normal_depth(db_, slots.data(), (int32_t)n, sf.data(), (int32_t)sf.size(), normal.data(), minD.data(), maxD.data(),
                                             status.data()));
    int updated = 0;
    for (size_t p = 0; p < n; p++) {
      if (status[p] != YDORB_MAP_UPDATED) continue;
      cv::Mat nrm(3, 1, CV_32F);
      for (int r = 0; r < 3; r++) nrm.template at<float>(r) = normal[3 * p + r];
      apply(asked[p], nrm, minD[p], maxD[p]);
      updated++;
    }
    return updated;
  }

  // The flat graph of localBundleAdjust for the local keyframes given (ydorb_mapdb_local_ba_graph), with the
  // slots translated back.  `graph` points into pinned memory the handle owns: it stays valid until the next localBaGraph or clear(),
  // and graph.problem.poses / pose_fixed are the caller's to fill.  Needs enableDescriptors() (the points' views) and enableFeatures():
  // without either it refuses.  The caller leaves bad keyframes out of the list, as the flat body does.
  struct LocalBaGraph {
    YdLocalBaGraph graph;
    std::vector<KeyFramePtr> poseKF;     // [n_poses]
    std::vector<MapPointPtr> pointMP;    // [n_points]
    std::vector<KeyFramePtr> edgeKF;     // [n_edges]; graph.edge_idx has the keypoint index
  };
  LocalBaGraph localBaGraph(const std::vector<KeyFramePtr>& localKeyFrames) {
    if (!descriptors_) throw std::runtime_error("ydorb: localBaGraph without enableDescriptors(): the points' views are not resident");
    if (!features_) throw std::runtime_error("ydorb: localBaGraph without enableFeatures()");
    std::vector<int32_t> slots;
    for (const KeyFramePtr& kf : localKeyFrames) slots.push_back(kfSlotFor(kf));
    flush();
    float sigma[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // one pyramid for all keyframes
    for (const KeyFramePtr& kf : kfOf_)
      if (kf) {
        for (size_t l = 0; l < 8 && l < kf->m_v_invScaleFactorSquares.size(); l++) sigma[l] = kf->m_v_invScaleFactorSquares[l];
        break;
      }
    LocalBaGraph G;
    mapCheck(ydorb_mapdb_local_ba_graph(db_, slots.data(), (int32_t)slots.size(), sigma, &G.graph));
    const YdBaProblem& P = G.graph.problem;
    for (int32_t i = 0; i < P.n_poses; i++) G.poseKF.push_back(kfOf_.at((size_t)G.graph.pose_kf[i]));
    for (int32_t p = 0; p < P.n_points; p++) G.pointMP.push_back(pointOf_.at((size_t)G.graph.point_slot[p]));
    for (int32_t e = 0; e < P.n_edges; e++) G.edgeKF.push_back(kfOf_.at((size_t)G.graph.edge_kf[e]));
    return G;
  }

  // covisibilityCounter of keyFrame.hpp over the resident table
  std::map<KeyFramePtr, int> covisibilityCounter(const KeyFramePtr& keyFrame) {
    const int32_t query = kfSlotFor(keyFrame);
    std::vector<int32_t> pointIdx;
    for (const MapPointPtr& mp : keyFrame->getMapPointMatches())
      if (mp) pointIdx.push_back(known(mp));       // per entry of the vector: a point listed twice counts twice
    flush();
    std::map<KeyFramePtr, int> counter;
    if (pointIdx.empty()) return counter;
    int64_t spans = 0;
    for (const int32_t p : pointIdx) spans += span_[p];
    const int32_t capacity = (int32_t)std::max<int64_t>(0, std::min<int64_t>((int64_t)kfOf_.size() - 1, spans));   // what always fits
    const int32_t listStart[2] = {0, (int32_t)pointIdx.size()}, outStart[2] = {0, capacity};
    std::vector<int32_t> kf((size_t)capacity + 1), weight((size_t)capacity + 1);
    int32_t count = 0;
    uint8_t status = 0;
    mapCheck(ydorb_mapdb_covisibility(db_, &query, 1, listStart, pointIdx.data(), outStart, kf.data(), weight.data(), &count, &status));
    if (status != 0) throw std::runtime_error("ydorb: covisibility capacity bound violated");
    for (int32_t i = 0; i < count; i++) counter[kfOf_[kf[i]]] = weight[i];
    return counter;
  }

  // keyFrameCullingImpl of localMapping.hpp over the resident table: the same walk, the same `removed` mask.  Returns the keyframes
  // setBadFlag() was called on, in order.  What setBadFlag() changes reaches the table through the touches it makes, at the next flush.
  std::vector<KeyFramePtr> keyFrameCulling(const KeyFramePtr& current, float thDepth) {
    std::vector<KeyFramePtr> candidates, flagged;
    std::vector<int32_t> candKf, listStart{0}, pointIdx;
    std::vector<uint8_t> ownLevel;
    for (const KeyFramePtr& kf : current->getVectorCovisibleKeyFrames()) {
      if (kf->m_int_keyFrameID == 0) continue;
      candidates.push_back(kf);
      candKf.push_back(kfSlotFor(kf));
      const std::vector<MapPointPtr> mps = kf->getMapPointMatches();
      for (size_t i = 0; i < mps.size(); i++) {
        if (!mps[i]) continue;
        if (kf->m_v_depth[i] > thDepth || kf->m_v_depth[i] < 0) continue;
        pointIdx.push_back(known(mps[i]));
        ownLevel.push_back((uint8_t)kf->m_v_keyPoints[i].octave);
      }
      if (pointIdx.size() > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX culling entries");
      listStart.push_back((int32_t)pointIdx.size());
    }
    flush();
    const int32_t K = (int32_t)candidates.size();
    if (K == 0) return flagged;
    std::vector<uint8_t> removed(kfOf_.size(), 0), cull(K);
    std::vector<int32_t> nCounted(K), nRedundant(K), start;
    bool masked = false;
    int32_t at = 0;
    while (at < K) {
      const int32_t n = K - at, base = listStart[at];
      start.assign((size_t)n + 1, 0);
      for (int32_t k = 0; k <= n; k++) start[k] = listStart[at + k] - base;
      mapCheck(ydorb_mapdb_keyframe_redundancy(db_, candKf.data() + at, n, start.data(), pointIdx.data() + base, ownLevel.data() + base,
                                               masked ? removed.data() : nullptr, 3, nCounted.data(), nRedundant.data(), cull.data()));
      int32_t k = 0;
      for (; k < n; k++) {
        if (!cull[k]) continue;
        const KeyFramePtr& kf = candidates[at + k];
        kf->setBadFlag();
        flagged.push_back(kf);
        if (kf->isBad()) {   // erased: the verdicts after it are stale
          removed[candKf[at + k]] = 1;
          masked = true;
          k++;
          break;
        }
      }
      at += k;
    }
    return flagged;
  }

  // ------------------------------------------------------------------------------------------------------------ map correction
  // The three point loops of loop closing over ydorb_mapdb_correct (c_api.h "Map correction"): the positions are
  // corrected where the table lives and come back once.  Each method flushes, walks only the keyframes' map-point vectors or the
  // caller's point list, makes one call, and for every corrected point, in order,
  //   - hands the new position to the container's own setter (setPosInWorld): the floats the device holds, so verify() stays empty
  //     without a touchPosition;
  //   - calls apply(mp, pos, normal, minDistance, maxDistance) (3x1 CV_32F matrices), where the caller stores the normal and the
  //     distances as updateNormalAndDepth would; `normal` is an empty cv::Mat where the reference's updateNormalAndDepth returns
  //     early (no observations) and in correctAfterGlobalBA, which computes none.
  // Each returns the number of corrected points.  The keyframes' poses stay with the caller, as in the reference.
  //
  // correctLoopPoints: the point loop of LoopClosing::correctLoop.  correctedSim3 / nonCorrectedSim3 = KeyFrameAndPose maps (any
  // Sim3T read through rotation().x() .. w(), translation()[k], scale(), as in optimizer.hpp).  The marks are set here:
  // m_int_correctedByKeyFrameID = currentKF's id, m_int_correctedReference = the correcting keyframe's id; a point that already
  // carries currentKF's mark is skipped.  The centre each keyframe shows after its setPose is computed here from its corrected Sim3
  // the way the reference builds correctedTiw and setPose its origin: R = rotation().toRotationMatrix() and t = translation() * (1. / s)
  // in double, both converted to float, Ow = -Rcw^T tcw as one CV_32F product (exact products summed in double in ascending index,
  // rounded once).  The caller still calls setPose on each keyframe (after this method or before: the table does not read it); if its
  // origin differs from the one computed here, verify() names the keyframe and touch(kf) mends it.
  template <class PoseMap, class Apply>
  int correctLoopPoints(const PoseMap& correctedSim3, const PoseMap& nonCorrectedSim3, const KeyFramePtr& currentKF, Apply apply) {
    Correction c;
    c.sim3 = true;
    for (const auto& kv : correctedSim3) {   // the container's own order
      const KeyFramePtr& kf = kv.first;
      const int32_t rank = (int32_t)c.kfSlots.size();
      c.kfs.push_back(kf);
      c.kfSlots.push_back(kfSlotFor(kf));
      pushSim3(c.after, kv.second);
      pushSim3(c.before, nonCorrectedSim3.at(kf));
      float O[3];
      originOfSim3(kv.second, O);
      c.centreAfter.insert(c.centreAfter.end(), O, O + 3);
      for (const MapPointPtr& mp : kf->getMapPointMatches()) {
        if (!mp) continue;
        if (mp->m_int_correctedByKeyFrameID == currentKF->m_int_keyFrameID) continue;
        c.points.push_back(mp); c.slots.push_back(known(mp)); c.corrector.push_back(rank);
      }
    }
    return run(c, YDORB_MAPCORR_INTERLEAVED, true, [&](const MapPointPtr& mp, int32_t rank) {
      mp->m_int_correctedByKeyFrameID = currentKF->m_int_keyFrameID;
      mp->m_int_correctedReference = c.kfs[(size_t)rank]->m_int_keyFrameID;
    }, apply);
  }

  // The tail of Optimizer::optimizeEssentialGraph, after every keyframe's setPose: keyFrames = the keyframes with a vertex, points = the
  // map's points; scwBefore(kf) / scwAfter(kf) return the keyframe's Sim3 before the optimisation (vScw) and the optimised one
  // (vCorrectedSwc's inverse: the entry inverts it).  A point marked by currentKF's correctLoop is corrected by the keyframe whose id is
  // its m_int_correctedReference, every other by its reference keyframe.  The centres are read from the keyframes: getCameraOriginInWorld().
  template <class KeyFrames, class Points, class Before, class After, class Apply>
  int correctAfterEssentialGraph(const KeyFrames& keyFrames, const Points& points, const KeyFramePtr& currentKF, Before scwBefore, After scwAfter,
                                 Apply apply) {
    Correction c;
    c.sim3 = true;
    std::map<long, int32_t> rankOfId;
    for (const KeyFramePtr& kf : keyFrames) {
      rankOfId[(long)kf->m_int_keyFrameID] = (int32_t)c.kfSlots.size();
      c.kfs.push_back(kf);
      c.kfSlots.push_back(kfSlotFor(kf));
      pushSim3(c.before, scwBefore(kf));
      pushSim3(c.after, scwAfter(kf));
      const cv::Mat O = kf->getCameraOriginInWorld();
      for (int r = 0; r < 3; r++) c.centreAfter.push_back(O.template at<float>(r));
    }
    for (const MapPointPtr& mp : points) {
      if (!mp) continue;
      int32_t rank = -1;
      if (mp->m_int_correctedByKeyFrameID == currentKF->m_int_keyFrameID) {
        const auto it = rankOfId.find((long)mp->m_int_correctedReference);
        if (it == rankOfId.end()) continue;   // its corrector has no vertex: left alone (optimizer.hpp does the same)
        rank = it->second;
      }
      c.points.push_back(mp); c.slots.push_back(known(mp)); c.corrector.push_back(rank);
    }
    return run(c, YDORB_MAPCORR_POSES_FIRST, true, [](const MapPointPtr&, int32_t) {}, apply);
  }

  // The map update of LoopClosing::runGlobalBundleAdjust for the points the BA did not hold (those take mPosGBA: setPosInWorld and
  // touchPosition, as before).  keyFrames = the keyframes the spanning-tree propagation reached (it stays with the caller); points = the
  // other points; poseBefore(kf) = Tcw before (mTcwBefGBA), poseInverseAfter(kf) = Twc after (getPoseInverse()), 4x4 CV_32F.  A point
  // whose reference keyframe is not among keyFrames is skipped, as in the reference.
  template <class KeyFrames, class Points, class PoseBefore, class PoseInverseAfter, class Apply>
  int correctAfterGlobalBA(const KeyFrames& keyFrames, const Points& points, PoseBefore poseBefore, PoseInverseAfter poseInverseAfter, Apply apply) {
    Correction c;
    c.sim3 = false;
    for (const KeyFramePtr& kf : keyFrames) {
      c.kfs.push_back(kf);
      c.kfSlots.push_back(kfSlotFor(kf));
      pushSE3(c.beforeF, poseBefore(kf));
      pushSE3(c.afterF, poseInverseAfter(kf));
    }
    for (const MapPointPtr& mp : points) {
      if (!mp) continue;
      c.points.push_back(mp); c.slots.push_back(known(mp)); c.corrector.push_back(-1);
    }
    return run(c, YDORB_MAPCORR_RESIDENT, false, [](const MapPointPtr&, int32_t) {}, apply);
  }

  // Flushes, re-reads everything the mirror knows and compares it with the device's table (ydorb_mapdb_export): the point slots whose
  // record differs and the keyframe slots whose centre differs.  Empty when every change was touched.
  Difference verify() {
    flush();
    YdMapDbStats st;
    mapCheck(ydorb_mapdb_stats(db_, &st));
    const size_t np = (size_t)st.n_points, nk = (size_t)st.n_keyframes, N = (size_t)st.n_observations;
    std::vector<int32_t> start(np + 1), obsKf(N + 1), refKf(np + 1);
    std::vector<uint8_t> obsLevel(N + 1), bad(np + 1), refLevel(np + 1);
    std::vector<float> pos(3 * np + 3), centre(3 * nk + 3);
    mapCheck(ydorb_mapdb_export(db_, start.data(), obsKf.data(), obsLevel.data(), bad.data(), refKf.data(), refLevel.data(), pos.data(), centre.data()));
    Difference d;
    for (size_t s = 0; s < pointOf_.size(); s++) {
      const Record want = pointOf_[s] ? read(pointOf_[s], false) : Record();
      bool same = s < np || (!pointOf_[s] && want.kf.empty());   // a slot past the table: only a free one that was never sent
      if (s < np) {
        const size_t len = (size_t)(start[s + 1] - start[s]);
        same = len == want.kf.size() && bad[s] == want.bad;
        same = same && (len == 0 || (std::memcmp(&obsKf[start[s]], want.kf.data(), 4 * len) == 0 && std::memcmp(&obsLevel[start[s]], want.level.data(), len) == 0));
        if (pointOf_[s]) same = same && refKf[s] == want.refKf && refLevel[s] == want.refLevel && std::memcmp(&pos[3 * s], want.pos, 12) == 0;
      }
      if (!same) d.pointSlots.push_back((int32_t)s);
    }
    for (size_t k = 0; k < kfOf_.size(); k++) {
      if (!kfOf_[k]) continue;
      const cv::Mat O = kfOf_[k]->getCameraOriginInWorld();
      float c[3];
      for (int r = 0; r < 3; r++) c[r] = O.template at<float>(r);
      if (k >= nk || std::memcmp(&centre[3 * k], c, 12) != 0) d.keyFrameSlots.push_back((int32_t)k);
    }
    return d;
  }

 private:
  enum : uint8_t { kClean = 0, kPos = 1, kFull = 2 };
  struct Record {   // what set_points takes for one point; the default is an erased point
    std::vector<int32_t> kf, idx;   // idx: the keypoint index of each observation (the views)
    std::vector<uint8_t> level;
    uint8_t bad = 1, refLevel = 0;
    int32_t refKf = 0;
    float pos[3] = {0.f, 0.f, 0.f};
  };

  struct Correction {   // the arrays of one ydorb_mapdb_correct call, built by the three correction methods
    bool sim3 = true;
    std::vector<KeyFramePtr> kfs;
    std::vector<int32_t> kfSlots, slots, corrector;
    std::vector<double> before, after;       // Sim3
    std::vector<float> beforeF, afterF;      // SE3
    std::vector<float> centreAfter;
    std::vector<MapPointPtr> points;
  };
  template <class Sim3T>
  static void pushSim3(std::vector<double>& to, const Sim3T& S) {
    const double v[8] = {S.rotation().x(), S.rotation().y(), S.rotation().z(), S.rotation().w(), S.translation()[0], S.translation()[1],
                         S.translation()[2], S.scale()};
    to.insert(to.end(), v, v + 8);
  }
  static void pushSE3(std::vector<float>& to, const cv::Mat& T) {   // rows 0..2 of a 4x4 CV_32F: the 3x3 row-major, then the translation
    for (int r = 0; r < 3; r++) for (int col = 0; col < 3; col++) to.push_back(T.template at<float>(r, col));
    for (int r = 0; r < 3; r++) to.push_back(T.template at<float>(r, 3));
  }
  // The origin setPose leaves for correctedTiw = [R | t / s] of a corrected Sim3 (see correctLoopPoints)
  template <class Sim3T>
  static void originOfSim3(const Sim3T& S, float* O) {
    const double x = S.rotation().x(), y = S.rotation().y(), z = S.rotation().z(), w = S.rotation().w();
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
                 tyz = tz * y, tzz = tz * z;   // Eigen's toRotationMatrix
    const float R[3][3] = {{(float)(1 - (tyy + tzz)), (float)(txy - twz), (float)(txz + twy)},
                           {(float)(txy + twz), (float)(1 - (txx + tzz)), (float)(tyz - twx)},
                           {(float)(txz - twy), (float)(tyz + twx), (float)(1 - (txx + tyy))}};
    const double inv = 1. / S.scale();
    const float t[3] = {(float)(S.translation()[0] * inv), (float)(S.translation()[1] * inv), (float)(S.translation()[2] * inv)};
    for (int i = 0; i < 3; i++)
      O[i] = (float)-(((double)R[0][i] * (double)t[0] + (double)R[1][i] * (double)t[1]) + (double)R[2][i] * (double)t[2]);
  }
  template <class Mark, class Apply>
  int run(Correction& c, int32_t centres, bool normals, Mark markPoint, Apply apply) {
    flush();
    const size_t n = c.slots.size();
    const std::vector<float> sf = scaleFactors();
    std::vector<float> pos(3 * n + 3), normal(3 * n + 3), minD(n + 1), maxD(n + 1);
    std::vector<uint8_t> status(n + 1);
    YdMapCorrection m;
    std::memset(&m, 0, sizeof(m));
    m.n_kf = (int32_t)c.kfSlots.size(); m.kf_slots = c.kfSlots.data();
    m.arithmetic = c.sim3 ? YDORB_MAPCORR_SIM3 : YDORB_MAPCORR_SE3;
    m.before = c.sim3 ? (const void*)c.before.data() : (const void*)c.beforeF.data();
    m.after = c.sim3 ? (const void*)c.after.data() : (const void*)c.afterF.data();
    m.centre_after = c.centreAfter.empty() ? nullptr : c.centreAfter.data();
    m.centres = m.centre_after ? centres : YDORB_MAPCORR_RESIDENT;
    if (n > (size_t)INT32_MAX) throw std::runtime_error("ydorb: more than INT32_MAX correction entries");
    m.n = (int32_t)n; m.slots = c.slots.data(); m.corrector = c.corrector.data();
    if (normals) { m.scale_factors = sf.data(); m.n_levels = (int32_t)sf.size(); m.normal = normal.data(); m.min_distance = minD.data(); m.max_distance = maxD.data(); }
    m.pos_out = pos.data(); m.status = status.data();
    mapCheck(ydorb_mapdb_correct(db_, &m));
    int corrected = 0;
    for (size_t i = 0; i < n; i++) {
      if (status[i] != YDORB_MAPCORR_DONE && status[i] != YDORB_MAPCORR_DONE_NO_OBSERVATIONS) continue;
      cv::Mat P(3, 1, CV_32F), nrm;
      for (int r = 0; r < 3; r++) P.template at<float>(r) = pos[3 * i + r];
      if (normals && status[i] == YDORB_MAPCORR_DONE) {
        nrm = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) nrm.template at<float>(r) = normal[3 * i + r];
      }
      c.points[i]->setPosInWorld(P);
      if (c.corrector[i] >= 0) markPoint(c.points[i], c.corrector[i]);
      apply(c.points[i], P, nrm, minD[i], maxD[i]);
      corrected++;
    }
    return corrected;
  }

  void markRow(int32_t s) { mark(rowDirty_, dirtyRows_, s, kFull); }
  static void mark(std::vector<uint8_t>& state, std::vector<int32_t>& list, int32_t s, uint8_t how) {
    if (state[s] == kClean) list.push_back(s);
    state[s] = std::max(state[s], how);
  }
  int32_t pointSlotFor(const MapPointPtr& mp) {
    const auto it = pointSlot_.find(mp);
    if (it != pointSlot_.end()) return it->second;
    int32_t s;
    if (!freePoints_.empty()) { s = freePoints_.back(); freePoints_.pop_back(); }
    else {
      s = (int32_t)pointOf_.size();
      pointOf_.push_back(MapPointPtr()); pointDirty_.push_back(kClean); span_.push_back(0); attrDirty_.push_back(kClean); erasePending_.push_back(0);
    }
    pointOf_[s] = mp;
    pointSlot_[mp] = s;
    return s;
  }
  int32_t kfSlotFor(const KeyFramePtr& kf) {   // a keyframe met for the first time gets a slot and its centre is sent
    const auto it = kfSlot_.find(kf);
    if (it != kfSlot_.end()) return it->second;
    int32_t s;
    if (!freeKfs_.empty()) { s = freeKfs_.back(); freeKfs_.pop_back(); }
    else {
      s = (int32_t)kfOf_.size();
      kfOf_.push_back(KeyFramePtr()); kfDirty_.push_back(kClean); rowDirty_.push_back(kClean); rowSent_.push_back(0);
      descDirty_.push_back(kClean); descSent_.push_back(0);
      featDirty_.push_back(kClean); featSent_.push_back(0);
      bowDirty_.push_back(kClean); bowSent_.push_back(0);
    }
    kfOf_[s] = kf;
    kfSlot_[kf] = s;
    mark(kfDirty_, dirtyKfs_, s, kFull);
    return s;
  }
  // the slot of a keyframe a BoW search names; what the table does not hold of it yet is read at the flush that follows
  int32_t bindForBow(const KeyFramePtr& kf) {
    const int32_t k = kfSlotFor(kf);
    if (!rowSent_[k]) markRow(k);
    if (!featSent_[k]) mark(featDirty_, dirtyFeats_, k, kFull);
    if (!descSent_[k]) mark(descDirty_, dirtyDescs_, k, kFull);
    if (!bowSent_[k]) mark(bowDirty_, dirtyBows_, k, kFull);
    return k;
  }
  // point slots [np][n] -> the map points, in vectors of `length` >= n entries; the table's slots are the mirror's
  BowSearchResult bowResult(size_t np, size_t n, size_t length, const std::vector<int32_t>& point, const std::vector<int32_t>& count,
                            const std::vector<uint8_t>& status) const {
    BowSearchResult r;
    r.matched.assign(np, std::vector<MapPointPtr>(length));
    for (size_t i = 0; i < np; i++)
      for (size_t j = 0; j < n; j++) {
        const int32_t s = point[i * n + j];
        if (s >= 0 && (size_t)s < pointOf_.size()) r.matched[i][j] = pointOf_[(size_t)s];
      }
    r.nMatches.assign(count.begin(), count.begin() + (long)np);
    r.pairStatus.assign(status.begin(), status.begin() + (long)np);
    return r;
  }
  // the slot of a point a query names; one the mirror has never been told of is read now (its observation map is walked this once)
  int32_t known(const MapPointPtr& mp) {
    const auto it = pointSlot_.find(mp);
    if (it != pointSlot_.end()) return it->second;
    const int32_t s = pointSlotFor(mp);
    mark(pointDirty_, dirtyPoints_, s, kFull);
    return s;
  }
  // assign: a keyframe without a slot gets one (flush); otherwise it reads as slot -1, which no table holds (verify)
  Record read(const MapPointPtr& mp, bool assign) {
    Record r;
    r.bad = mp->isBad() ? 1 : 0;
    const auto observations = mp->getObservations();
    for (const auto& ob : observations) {   // the container's own order
      r.kf.push_back(assign ? kfSlotFor(ob.first) : slotOf(ob.first));
      r.idx.push_back((int32_t)ob.second);
      const int octave = ob.first->m_v_keyPoints[ob.second].octave;
      r.level.push_back((uint8_t)((octave & 0x7f) | (ob.first->m_v_rightXcords[ob.second] >= 0 ? 0x80 : 0)));
    }
    const KeyFramePtr ref = mp->getReferenceKeyFrame();
    if (ref) {
      r.refKf = assign ? kfSlotFor(ref) : slotOf(ref);
      if (!r.bad && !r.kf.empty()) {   // the reference reads its reference keyframe only past both early returns
        const auto it = observations.find(ref);
        r.refLevel = (uint8_t)ref->m_v_keyPoints[it != observations.end() ? it->second : 0].octave;
      }
    } else if (kfOf_.empty()) {
      throw std::runtime_error("ydorb: a map point without a reference keyframe in a mirror without keyframes");
    }
    const cv::Mat P = mp->getPosInWorld();
    for (int i = 0; i < 3; i++) r.pos[i] = P.template at<float>(i);
    return r;
  }
  // m_cvMat_descriptors, one 32-byte row per keypoint.  Chosen by overload so that a keyframe type without the member still builds the
  // mirror (it cannot enable descriptors).
  template <class K>
  static auto appendDescriptorsOf(const K& kf, std::vector<uint8_t>& to, int) -> decltype((void)kf->m_cvMat_descriptors) {
    const cv::Mat& D = kf->m_cvMat_descriptors;
    for (int i = 0; i < D.rows; i++) {
      const unsigned char* r = D.row(i).template ptr<unsigned char>();
      to.insert(to.end(), r, r + 32);
    }
  }
  template <class K>
  static void appendDescriptorsOf(const K&, std::vector<uint8_t>&, long) { throw std::runtime_error("ydorb: the keyframe type has no m_cvMat_descriptors"); }
  static void appendDescriptors(const KeyFramePtr& kf, std::vector<uint8_t>& to) { appendDescriptorsOf(kf, to, 0); }
  // m_v_keyPoints and m_v_rightXcords of one keyframe
  static void appendFeatures(const KeyFramePtr& kf, std::vector<YdKeyPoint>& kps, std::vector<float>& rightX) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(YdKeyPoint), "cv::KeyPoint layout");
    const size_t n = kf->m_v_keyPoints.size(), at = kps.size();
    if (kf->m_v_rightXcords.size() != n) throw std::runtime_error("ydorb: m_v_rightXcords and m_v_keyPoints differ in length");
    kps.resize(at + n);
    if (n) std::memcpy(&kps[at], kf->m_v_keyPoints.data(), sizeof(YdKeyPoint) * n);
    rightX.insert(rightX.end(), kf->m_v_rightXcords.begin(), kf->m_v_rightXcords.end());
  }
  // m_bow_keyPointsVec of one keyframe, flattened in map order: nodes ascending, a node's features in the vector's order.  Chosen by
  // overload so that a keyframe type without the member still builds the mirror (it cannot enable the feature vectors).
  template <class K>
  static auto appendBowOf(const K& kf, std::vector<uint32_t>& node, std::vector<int32_t>& feat, int) -> decltype((void)kf->m_bow_keyPointsVec) {
    for (const auto& kv : kf->m_bow_keyPointsVec)
      for (const auto f : kv.second) { node.push_back((uint32_t)kv.first); feat.push_back((int32_t)f); }
  }
  template <class K>
  static void appendBowOf(const K&, std::vector<uint32_t>&, std::vector<int32_t>&, long) { throw std::runtime_error("ydorb: the keyframe type has no m_bow_keyPointsVec"); }
  static void appendBow(const KeyFramePtr& kf, std::vector<uint32_t>& node, std::vector<int32_t>& feat) { appendBowOf(kf, node, feat, 0); }
  // getNormal() (3x1 CV_32F), the raw getMinDistance() / getMaxDistance() and getDescriptor() (1x32 CV_8U) of one point, each group
  // appended only when its matrix is not empty (the member is set).  Chosen by
  // overload so that a map-point type without them still builds the mirror (it cannot touch attributes).
  template <class P>
  static auto appendAttributesOf(const P& mp, std::vector<float>& normal, std::vector<float>& minD, std::vector<float>& maxD, std::vector<uint8_t>& desc, int)
      -> decltype((void)mp->getMinDistance(), (void)mp->getDescriptor()) {
    const cv::Mat N = mp->getNormal(), D = mp->getDescriptor();
    if (!N.empty()) {
      for (int r = 0; r < 3; r++) normal.push_back(N.template at<float>(r));
      minD.push_back(mp->getMinDistance()); maxD.push_back(mp->getMaxDistance());
    }
    if (!D.empty()) {
      const unsigned char* d = D.template ptr<unsigned char>();
      desc.insert(desc.end(), d, d + 32);
    }
  }
  template <class P>
  static void appendAttributesOf(const P&, std::vector<float>&, std::vector<float>&, std::vector<float>&, std::vector<uint8_t>&, long) {
    throw std::runtime_error("ydorb: the map-point type has no getMinDistance() / getDescriptor()");
  }
  static void appendAttributes(const MapPointPtr& mp, std::vector<float>& normal, std::vector<float>& minD, std::vector<float>& maxD, std::vector<uint8_t>& desc) {
    appendAttributesOf(mp, normal, minD, maxD, desc, 0);
  }
  std::vector<float> scaleFactors() const {   // one pyramid for all keyframes
    for (const KeyFramePtr& kf : kfOf_) if (kf) return kf->m_v_scaleFactors;
    return std::vector<float>(1, 1.0f);
  }

  ydorb_mapdb_t* db_ = nullptr;
  std::map<MapPointPtr, int32_t> pointSlot_;
  std::vector<MapPointPtr> pointOf_;
  std::vector<int32_t> freePoints_, dirtyPoints_, span_;
  std::vector<uint8_t> pointDirty_;
  std::map<KeyFramePtr, int32_t> kfSlot_;
  std::vector<KeyFramePtr> kfOf_;
  std::vector<int32_t> freeKfs_, dirtyKfs_;
  std::vector<uint8_t> kfDirty_;
  std::vector<uint8_t> rowDirty_, rowSent_;   // per keyframe slot: the row is re-read at the next flush / the table holds a row of it
  std::vector<int32_t> dirtyRows_;
  std::vector<std::pair<int32_t, int32_t> > dirtyEntries_;   // (keyframe slot, index)
  bool descriptors_ = false;
  std::vector<uint8_t> descDirty_, descSent_;   // per keyframe slot: the block is re-read at the next flush / the table holds a block of it
  std::vector<int32_t> dirtyDescs_;
  bool features_ = false;
  std::vector<uint8_t> featDirty_, featSent_;   // per keyframe slot: the features are re-read at the next flush / the table holds features of it
  std::vector<int32_t> dirtyFeats_;
  bool bow_ = false;
  std::vector<uint8_t> bowDirty_, bowSent_;   // per keyframe slot: the feature vector is re-read at the next flush / the table holds one of it
  std::vector<int32_t> dirtyBows_;
  bool attributes_ = false;
  std::vector<uint8_t> attrDirty_;   // per point slot: the attributes are re-read at the next flush
  std::vector<uint8_t> erasePending_;   // per point slot: forgotten with attributes enabled, and the erased record has not gone yet
  std::vector<int32_t> dirtyAttrs_;
};

}  // namespace adapter
}  // namespace ydorb
#endif
