// Drop-in adapter for YDORBSLAM::Optimizer::localBundleAdjust (reference src/optimizer.hpp:34, src/optimizer.cpp:138-352)
// on top of the ydorb C ABI.  Template over the reference's KeyFrame / MapPoint / Map types: the body of
//   void Optimizer::localBundleAdjust(std::shared_ptr<KeyFrame> kf, std::shared_ptr<Map> map, bool& stop)
// becomes  ydorb::adapter::localBundleAdjust(kf, map, &stop == nullptr ? nullptr : &stop);
// The host keeps the covisibility walk (:140-173), the float->double conversions of Converter (converter.cpp:12-19) and the
// write-back under Map::m_mutex_updateMap (:336-351); residuals, Jacobians, Huber, Schur, Cholesky, LM run on the GPU.
#ifndef YDORB_ADAPTER_OPTIMIZER_HPP
#define YDORB_ADAPTER_OPTIMIZER_HPP

#include <algorithm>
#include <cmath>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <Eigen/Core>
#include <Eigen/Geometry>
#include <opencv2/core.hpp>

#include "c_api.h"

namespace ydorb {
namespace adapter {

// Converter::transform_cvMat_SE3Quat (converter.cpp:12-19): float 4x4 -> (t, unit quaternion) in double
inline void poseToSE3Quat(const cv::Mat& T, double* p7) {
  Eigen::Matrix3d R;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R(i, j) = T.at<float>(i, j);
  Eigen::Quaterniond q(R);
  if (q.w() < 0) q.coeffs() *= -1;
  q.normalize();
  p7[0] = T.at<float>(0, 3); p7[1] = T.at<float>(1, 3); p7[2] = T.at<float>(2, 3);
  p7[3] = q.x(); p7[4] = q.y(); p7[5] = q.z(); p7[6] = q.w();
}
// Converter::transform_SE3_cvMat (converter.cpp:20-38): back to a float 4x4
inline cv::Mat se3QuatToPose(const double* p7) {
  const Eigen::Matrix3d R = Eigen::Quaterniond(p7[6], p7[3], p7[4], p7[5]).toRotationMatrix();
  cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T.at<float>(i, j) = (float)R(i, j);
    T.at<float>(i, 3) = (float)p7[i];
  }
  return T;
}

template <class KeyFramePtr, class MapPtr, class FrameT>
void localBundleAdjustImpl(KeyFramePtr kf0, MapPtr map, const volatile bool* stop, int solver = YDORB_BA_SOLVER_AUTO) {
  typedef decltype(kf0->getMatchedMapPointsVec()) MapPointVec;
  typedef typename MapPointVec::value_type MapPointPtr;
  const long int tag = kf0->m_int_keyFrameID;
  // local keyframes = current + its covisible ones; local points = what they see; fixed keyframes = other observers (:140-173)
  std::list<KeyFramePtr> localKFs{kf0};
  kf0->m_int_localBAForKeyFrameID = tag;
  for (const KeyFramePtr& c : kf0->getOrderedConnectedKeyFrames()) {
    c->m_int_localBAForKeyFrameID = tag;
    if (!c->isBad()) localKFs.push_back(c);
  }
  std::list<MapPointPtr> localMPs;
  for (const KeyFramePtr& k : localKFs)
    for (const MapPointPtr& mp : k->getMatchedMapPointsVec())
      if (mp && !mp->isBad() && mp->m_int_localBAForKeyFrameID != tag) { localMPs.push_back(mp); mp->m_int_localBAForKeyFrameID = tag; }
  std::list<KeyFramePtr> fixedKFs;
  for (const MapPointPtr& mp : localMPs)
    for (const auto& ob : mp->getObservations())
      if (ob.first->m_int_localBAForKeyFrameID != tag && ob.first->m_int_fixedBAForKeyFrameID != tag) {
        ob.first->m_int_fixedBAForKeyFrameID = tag;
        if (!ob.first->isBad()) fixedKFs.push_back(ob.first);
      }
  // flat graph (:185-283)
  std::vector<KeyFramePtr> poseKF;
  std::map<long int, int> poseIndex;
  std::vector<double> poses;
  std::vector<uint8_t> fixed;
  long int maxKFid = 0;
  auto addPose = [&](const KeyFramePtr& k, bool fix) {
    poseIndex[k->m_int_keyFrameID] = (int)poseKF.size();
    poseKF.push_back(k);
    poses.resize(poses.size() + 7);
    poseToSE3Quat(k->getCameraPoseByTransform_c2w(), &poses[poses.size() - 7]);
    fixed.push_back(fix ? 1 : 0);
    if (k->m_int_keyFrameID > maxKFid) maxKFid = k->m_int_keyFrameID;
  };
  for (const KeyFramePtr& k : localKFs) if (!k->isBad()) addPose(k, k->m_int_keyFrameID == 0);
  const size_t nLocal = poseKF.size();
  for (const KeyFramePtr& k : fixedKFs) addPose(k, true);
  std::vector<MapPointPtr> pointMP(localMPs.begin(), localMPs.end());
  std::vector<double> points(3 * pointMP.size());
  std::vector<int32_t> ePose, ePoint;
  std::vector<double> eMeas, eInfo;
  std::vector<KeyFramePtr> edgeKF;
  for (size_t p = 0; p < pointMP.size(); p++) {
    const cv::Mat X = pointMP[p]->getPosInWorld();
    for (int d = 0; d < 3; d++) points[3 * p + d] = X.at<float>(d);
    for (const auto& ob : pointMP[p]->getObservations()) {
      if (ob.first->isBad() || ob.first->m_int_keyFrameID > maxKFid) continue;
      const auto it = poseIndex.find(ob.first->m_int_keyFrameID);
      if (it == poseIndex.end()) continue;
      const cv::KeyPoint& kp = ob.first->m_v_keyPoints[ob.second];
      const float ur = ob.first->m_v_rightXcords[ob.second];
      ePose.push_back(it->second); ePoint.push_back((int32_t)p);
      eMeas.push_back(kp.pt.x); eMeas.push_back(kp.pt.y); eMeas.push_back(ur < 0 ? -1.0 : (double)ur);
      eInfo.push_back(ob.first->m_v_invScaleFactorSquares[kp.octave]);
      edgeKF.push_back(ob.first);
    }
  }
  if (stop && *stop) return;  // :284-286
  YdBaProblem P{};
  P.n_poses = (int32_t)poseKF.size(); P.n_points = (int32_t)pointMP.size(); P.n_edges = (int32_t)ePose.size();
  P.poses = poses.data(); P.pose_fixed = fixed.data(); P.points = points.data();
  P.edge_pose = ePose.data(); P.edge_point = ePoint.data(); P.edge_meas = eMeas.data(); P.edge_inv_sigma2 = eInfo.data();
  P.fx = FrameT::m_flt_fx; P.fy = FrameT::m_flt_fy; P.cx = FrameT::m_flt_cx; P.cy = FrameT::m_flt_cy; P.bf = FrameT::m_flt_baseLineTimesFx;
  P.stop = reinterpret_cast<const volatile uint8_t*>(stop);
  std::vector<uint8_t> outlier(ePose.size() + 1, 0);
  YdBaResult res{};
  res.edge_outlier = outlier.data();
  const YdBaSolverOptions SO = {solver, YDORB_ESS_ORDER_SMALLER, 0};   // AUTO: the dense solve up to its 3 200 free keyframes, block-skyline above
  if (ydorb_ba_solve_with(&P, nullptr, &SO, &res, nullptr) != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  // write-back (:336-351)
  std::unique_lock<std::mutex> lock(map->m_mutex_updateMap);
  for (size_t e = 0; e < ePose.size(); e++)
    if (outlier[e] && !pointMP[ePoint[e]]->isBad()) {
      edgeKF[e]->eraseMatchedMapPoint(pointMP[ePoint[e]]);
      pointMP[ePoint[e]]->eraseObservation(edgeKF[e]);
    }
  for (size_t k = 0; k < nLocal; k++) poseKF[k]->setCameraPoseByTransform_c2w(se3QuatToPose(&poses[7 * k]));
  for (size_t p = 0; p < pointMP.size(); p++) {
    cv::Mat X(3, 1, CV_32F);
    for (int d = 0; d < 3; d++) X.at<float>(d) = (float)points[3 * p + d];
    pointMP[p]->setPosInWorld(X);
    pointMP[p]->updateNormalAndDepth();
  }
}

// localBundleAdjust over a MapMirror (mapMirror.hpp) with enableDescriptors() and enableFeatures(): the body of the reference becomes
//   ydorb::adapter::localBundleAdjustImpl<Frame>(mirror, kf, map, &stop == nullptr ? nullptr : &stop, apply);
// The covisibility list (kf0 + getOrderedConnectedKeyFrames() minus bad) stays on the host; the local points, the fixed keyframes and
// every edge come from ONE mirror.localBaGraph call on the resident table (ydorb_mapdb_local_ba_graph), in the
// flat body's order, so the solve is the flat body's bit for bit.  Only the poses are read from the keyframes.  The write-back follows
// the flat body and tells the mirror what it changed: an erased observation touches the point and the keyframe's row entry (the
// keypoint index is the graph's edge_idx), a moved keyframe its centre, a moved point its position; then ONE
// mirror.updateNormalAndDepth over all points in place of a call per point, apply(mp, normal, minDistance, maxDistance) storing what
// MapPoint::updateNormalAndDepth would.  Of the reference's BA tags only the local keyframes' m_int_localBAForKeyFrameID is written:
// the point and fixed-keyframe tags exist to build the lists, which the table does here.
template <class FrameT, class MirrorT, class KeyFramePtr, class MapPtr, class Apply>
void localBundleAdjustImpl(MirrorT& mirror, KeyFramePtr kf0, MapPtr map, const volatile bool* stop, Apply apply, int solver = YDORB_BA_SOLVER_AUTO) {
  const long int tag = kf0->m_int_keyFrameID;
  std::vector<KeyFramePtr> localKFs{kf0};
  kf0->m_int_localBAForKeyFrameID = tag;
  for (const KeyFramePtr& c : kf0->getOrderedConnectedKeyFrames()) {
    c->m_int_localBAForKeyFrameID = tag;
    if (!c->isBad()) localKFs.push_back(c);
  }
  auto G = mirror.localBaGraph(localKFs);
  YdBaProblem P = G.graph.problem;
  const size_t nLocal = (size_t)G.graph.n_local, nPoints = (size_t)P.n_points, nEdges = (size_t)P.n_edges;
  uint8_t* fixed = const_cast<uint8_t*>(P.pose_fixed);   // writable in the handle's result (c_api.h)
  for (size_t k = 0; k < G.poseKF.size(); k++) {
    poseToSE3Quat(G.poseKF[k]->getCameraPoseByTransform_c2w(), P.poses + 7 * k);
    if (k < nLocal && G.poseKF[k]->m_int_keyFrameID == 0) fixed[k] = 1;
  }
  if (stop && *stop) return;  // :284-286
  P.fx = FrameT::m_flt_fx; P.fy = FrameT::m_flt_fy; P.cx = FrameT::m_flt_cx; P.cy = FrameT::m_flt_cy; P.bf = FrameT::m_flt_baseLineTimesFx;
  P.stop = reinterpret_cast<const volatile uint8_t*>(stop);
  std::vector<uint8_t> outlier(nEdges + 1, 0);
  YdBaResult res{};
  res.edge_outlier = outlier.data();
  const YdBaSolverOptions SO = {solver, YDORB_ESS_ORDER_SMALLER, 0};
  if (ydorb_ba_solve_with(&P, nullptr, &SO, &res, nullptr) != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  // write-back (:336-351)
  std::unique_lock<std::mutex> lock(map->m_mutex_updateMap);
  for (size_t e = 0; e < nEdges; e++) {
    const auto& mp = G.pointMP[(size_t)P.edge_point[e]];
    if (!outlier[e] || mp->isBad()) continue;
    G.edgeKF[e]->eraseMatchedMapPoint(mp);
    mp->eraseObservation(G.edgeKF[e]);
    mirror.touch(mp);
    mirror.touchEntry(G.edgeKF[e], (size_t)G.graph.edge_idx[e]);
  }
  for (size_t k = 0; k < nLocal; k++) {
    G.poseKF[k]->setCameraPoseByTransform_c2w(se3QuatToPose(P.poses + 7 * k));
    mirror.touch(G.poseKF[k]);
  }
  for (size_t p = 0; p < nPoints; p++) {
    cv::Mat X(3, 1, CV_32F);
    for (int d = 0; d < 3; d++) X.at<float>(d) = (float)P.points[3 * p + d];
    G.pointMP[p]->setPosInWorld(X);
    mirror.touchPosition(G.pointMP[p]);
  }
  mirror.updateNormalAndDepth(G.pointMP, apply);
}

// Optimizer::bundleAdjust (optimizer.cpp:7-137): every given keyframe (id 0 fixed) and map point, ONE optimize(iterNum) call, Huber
// optional; results go to the vertices' GBA fields when loopKeyFrameID != 0 (:113-136).  Same C ABI call with
// YDORB_BA_SINGLE_STAGE; the body of
//   void Optimizer::bundleAdjust(kfs, mps, iterNum, stop, loopKFid, robust)
// becomes  ydorb::adapter::bundleAdjustImpl<Frame>(kfs, mps, iterNum, &stop == nullptr ? nullptr : &stop, loopKFid, robust);
template <class FrameT, class KeyFramePtr, class MapPointPtr>
void bundleAdjustImpl(const std::vector<KeyFramePtr>& kfs, const std::vector<MapPointPtr>& mps, int iterNum, const volatile bool* stop,
                      long int loopKeyFrameID, bool robust, int solver = YDORB_BA_SOLVER_AUTO) {
  std::vector<KeyFramePtr> poseKF;
  std::map<long int, int> poseIndex;
  std::vector<double> poses;
  std::vector<uint8_t> fixed;
  long int maxKFid = 0;
  for (const KeyFramePtr& k : kfs) {
    if (k->isBad()) continue;
    poseIndex[k->m_int_keyFrameID] = (int)poseKF.size();
    poseKF.push_back(k);
    poses.resize(poses.size() + 7);
    poseToSE3Quat(k->getCameraPoseByTransform_c2w(), &poses[poses.size() - 7]);
    fixed.push_back(k->m_int_keyFrameID == 0 ? 1 : 0);
    if (k->m_int_keyFrameID > maxKFid) maxKFid = k->m_int_keyFrameID;
  }
  std::vector<double> points(3 * mps.size(), 0.0);
  std::vector<uint8_t> excluded(mps.size(), 1);   // bad points and points without a usable observation stay untouched (:103-110)
  std::vector<int32_t> ePose, ePoint;
  std::vector<double> eMeas, eInfo;
  for (size_t p = 0; p < mps.size(); p++) {
    if (!mps[p] || mps[p]->isBad()) continue;
    const cv::Mat X = mps[p]->getPosInWorld();
    for (int d = 0; d < 3; d++) points[3 * p + d] = X.at<float>(d);
    for (const auto& ob : mps[p]->getObservations()) {
      if (ob.first->isBad() || ob.first->m_int_keyFrameID > maxKFid) continue;
      const auto it = poseIndex.find(ob.first->m_int_keyFrameID);
      if (it == poseIndex.end()) continue;   // g2o: optimizer.vertex(id) == nullptr -> the edge cannot be added
      const cv::KeyPoint& kp = ob.first->m_v_keyPoints[ob.second];
      const float ur = ob.first->m_v_rightXcords[ob.second];
      ePose.push_back(it->second); ePoint.push_back((int32_t)p);
      eMeas.push_back(kp.pt.x); eMeas.push_back(kp.pt.y); eMeas.push_back(ur < 0 ? -1.0 : (double)ur);
      eInfo.push_back(ob.first->m_v_invScaleFactorSquares[kp.octave]);
      excluded[p] = 0;
    }
  }
  YdBaProblem P{};
  P.n_poses = (int32_t)poseKF.size(); P.n_points = (int32_t)mps.size(); P.n_edges = (int32_t)ePose.size();
  P.poses = poses.data(); P.pose_fixed = fixed.data(); P.points = points.data();
  P.edge_pose = ePose.data(); P.edge_point = ePoint.data(); P.edge_meas = eMeas.data(); P.edge_inv_sigma2 = eInfo.data();
  P.fx = FrameT::m_flt_fx; P.fy = FrameT::m_flt_fy; P.cx = FrameT::m_flt_cx; P.cy = FrameT::m_flt_cy; P.bf = FrameT::m_flt_baseLineTimesFx;
  P.stop = reinterpret_cast<const volatile uint8_t*>(stop);
  YdBaOptions O;
  ydorb_ba_default_options(&O);
  O.iters1 = iterNum; O.iters2 = 0;
  O.delta_mono = (double)(float)std::sqrt(5.99);   // `const float monoDelta = sqrt(5.99)`, :37
  O.flags = YDORB_BA_SINGLE_STAGE | (robust ? 0 : YDORB_BA_NO_ROBUST);
  YdBaResult res{};
  const YdBaSolverOptions SO = {solver, YDORB_ESS_ORDER_SMALLER, 0};   // AUTO: the dense solve up to its 3 200 free keyframes, block-skyline above
  if (ydorb_ba_solve_with(&P, &O, &SO, &res, nullptr) != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  for (size_t k = 0; k < poseKF.size(); k++) {   // :113-124
    const cv::Mat T = se3QuatToPose(&poses[7 * k]);
    if (loopKeyFrameID == 0) {
      poseKF[k]->setCameraPoseByTransform_c2w(T);
    } else {
      poseKF[k]->m_cvMat_T_c2w_GlobalBA.create(4, 4, CV_32F);
      T.copyTo(poseKF[k]->m_cvMat_T_c2w_GlobalBA);
      poseKF[k]->m_int_globalBAForKeyFrameID = loopKeyFrameID;
    }
  }
  for (size_t p = 0; p < mps.size(); p++) {     // :126-136
    if (!mps[p] || mps[p]->isBad() || excluded[p]) continue;
    cv::Mat X(3, 1, CV_32F);
    for (int d = 0; d < 3; d++) X.at<float>(d) = (float)points[3 * p + d];
    if (loopKeyFrameID == 0) {
      mps[p]->setPosInWorld(X);
      mps[p]->updateNormalAndDepth();
    } else {
      mps[p]->m_cvMat_posGlobalBA.create(3, 1, CV_32F);
      X.copyTo(mps[p]->m_cvMat_posGlobalBA);
      mps[p]->m_int_globalBAforKeyFrameID = loopKeyFrameID;
    }
  }
}

// Optimizer::optimizePose (optimizer.cpp:358-501): pose-only refinement of one frame against its matched map points; returns the
// number of inliers and updates Frame::m_v_isOutliers and the frame pose exactly where the reference does.  The body of
//   int Optimizer::optimizePose(Frame& frame)   becomes   return ydorb::adapter::optimizePoseImpl(frame);
// (A tracker that refines several frames at once — replay, multi-camera rigs — can hand them to ydorb_pose_optimize as one batch:
// one workgroup per frame, 64 frames cost about as much as one.)
template <class FrameT>
int optimizePoseImpl(FrameT& frame) {
  std::vector<int> idx;
  std::vector<double> X, z, w;
  for (int i = 0; i < frame.m_int_keyPointsNum; i++) {
    if (!frame.m_v_sptrMapPoints[i]) continue;
    frame.m_v_isOutliers[i] = false;                       // :392
    const cv::KeyPoint& kp = frame.m_v_keyPoints[i];
    const cv::Mat Xw = frame.m_v_sptrMapPoints[i]->getPosInWorld();
    for (int d = 0; d < 3; d++) X.push_back(Xw.at<float>(d));
    const float ur = frame.m_v_rightXcords[i];
    z.push_back(kp.pt.x); z.push_back(kp.pt.y); z.push_back(ur < 0 ? -1.0 : (double)ur);
    w.push_back(frame.m_v_invScaleFactorSquares[kp.octave]);
    idx.push_back(i);
  }
  if (idx.size() < 3) return 0;                            // :443-445
  double pose[7];
  poseToSE3Quat(frame.getCameraPoseByTransform_c2w(), pose);
  const int32_t start[2] = {0, (int32_t)idx.size()};
  YdPoseBatch B{};
  B.n_frames = 1; B.device = 0; B.edge_start = start; B.poses = pose; B.points = X.data(); B.meas = z.data(); B.inv_sigma2 = w.data();
  B.fx = FrameT::m_flt_fx; B.fy = FrameT::m_flt_fy; B.cx = FrameT::m_flt_cx; B.cy = FrameT::m_flt_cy; B.bf = FrameT::m_flt_baseLineTimesFx;
  std::vector<uint8_t> outlier(idx.size());
  int32_t inliers = 0;
  if (ydorb_pose_optimize(&B, outlier.data(), &inliers, nullptr, nullptr) != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  for (size_t k = 0; k < idx.size(); k++) frame.m_v_isOutliers[idx[k]] = outlier[k] != 0;
  frame.setCameraPoseByTransform_c2w(se3QuatToPose(pose));  // :498-499
  return inliers;
}

// Optimizer::optimizeSim3 (ORB-SLAM2 Optimizer::OptimizeSim3, src/Optimizer.cc): the pairs of matches1 whose two
// map points are set, not bad and indexed in KF2 go to ydorb_sim3_optimize; the matches it drops are set to null as the reference does.
// S12 is g2o::Sim3 as 8 doubles (qx, qy, qz, qw, tx, ty, tz, s), in/out; INTEGRATION.md shows the conversion in the forwarding body.
// Camera-frame points: each product exact in double, summed in double, rounded to float, plus t in float (the float cv::Mat transform
// the reference does before Converter::toVector3d).
template <class FrameT, class KeyFramePtr, class MapPointPtr>
int optimizeSim3Impl(KeyFramePtr kf1, KeyFramePtr kf2, std::vector<MapPointPtr>& matches1, double* S12, const float th2, const bool fixScale,
                     int device = 0) {
  const cv::Mat R1 = kf1->getRotation_c2w(), t1 = kf1->getTranslation_c2w(), R2 = kf2->getRotation_c2w(), t2 = kf2->getTranslation_c2w();
  const std::vector<MapPointPtr> mps1 = kf1->getMatchedMapPointsVec();
  std::vector<int> idx;
  std::vector<double> X1, X2, o1, o2, w1, w2;
  auto cam = [](const cv::Mat& R, const cv::Mat& t, const cv::Mat& Xw, std::vector<double>& out) {
    for (int r = 0; r < 3; r++) {
      const double s = ((double)R.at<float>(r, 0) * (double)Xw.at<float>(0) + (double)R.at<float>(r, 1) * (double)Xw.at<float>(1)) +
                       (double)R.at<float>(r, 2) * (double)Xw.at<float>(2);
      out.push_back((double)((float)s + t.at<float>(r)));
    }
  };
  for (int i = 0; i < (int)matches1.size(); i++) {
    if (!matches1[i]) continue;
    const MapPointPtr mp1 = mps1[i], mp2 = matches1[i];
    if (!mp1) continue;
    const int i2 = mp2->getIdxInKeyFrame(kf2);
    if (mp1->isBad() || mp2->isBad() || i2 < 0) continue;
    cam(R1, t1, mp1->getPosInWorld(), X1);
    cam(R2, t2, mp2->getPosInWorld(), X2);
    const cv::KeyPoint& k1 = kf1->m_v_keyPoints[i];
    const cv::KeyPoint& k2 = kf2->m_v_keyPoints[i2];
    o1.push_back(k1.pt.x); o1.push_back(k1.pt.y);
    o2.push_back(k2.pt.x); o2.push_back(k2.pt.y);
    w1.push_back(kf1->m_v_invScaleFactorSquares[k1.octave]);
    w2.push_back(kf2->m_v_invScaleFactorSquares[k2.octave]);
    idx.push_back(i);
  }
  const int32_t start[2] = {0, (int32_t)idx.size()};
  const double K[4] = {FrameT::m_flt_fx, FrameT::m_flt_fy, FrameT::m_flt_cx, FrameT::m_flt_cy};
  const uint8_t fix = fixScale ? 1 : 0;
  YdSim3Batch B{};
  B.n_problems = 1; B.device = device; B.corr_start = start; B.S12 = S12; B.K1 = K; B.K2 = K; B.fix_scale = &fix;
  B.X1c = X1.data(); B.X2c = X2.data(); B.obs1 = o1.data(); B.obs2 = o2.data(); B.inv_sigma2_1 = w1.data(); B.inv_sigma2_2 = w2.data();
  B.th2 = th2;
  std::vector<uint8_t> outlier(std::max<size_t>(idx.size(), 1));
  int32_t nIn = 0;
  if (ydorb_sim3_optimize(&B, outlier.data(), &nIn, nullptr, nullptr) != YDORB_OK) throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  for (size_t k = 0; k < idx.size(); k++)
    if (outlier[k]) matches1[idx[k]] = MapPointPtr();
  return nIn;
}

// Optimizer::optimizeEssentialGraph (ORB-SLAM2 Optimizer::OptimizeEssentialGraph, src/Optimizer.cc).  The body of
//   void Optimizer::optimizeEssentialGraph(map, loopKF, curKF, nonCorrectedSim3, correctedSim3, loopConnections, fixScale)
// becomes  ydorb::adapter::optimizeEssentialGraphImpl<Frame>(map, loopKF, curKF, nonCorrectedSim3, correctedSim3, loopConnections, fixScale);
// Member spellings assumed beyond the ones used above (the reference is not at hand; ORB-SLAM2's names in the project's lowerCamelCase):
//   KeyFrame  getParent(), hasChild(kf), getLoopEdges() -> std::set<KeyFramePtr>, getCovisiblesByWeight(int) -> std::vector<KeyFramePtr>,
//             getWeight(kf), getRotation_c2w(), getTranslation_c2w(), setCameraPoseByTransform_c2w(cv::Mat), m_int_keyFrameID
//   MapPoint  m_int_correctedByKeyFrameID, m_int_correctedReference (mnCorrectedByKF, mnCorrectedReference), getReferenceKeyFrame()
//   Map       getAllKeyFrames(), getAllMapPoints(), m_mutex_updateMap
//   the maps  KeyFrameAndPose = std::map<KeyFramePtr, Sim3T>; Sim3T is read through rotation().x() .. w(), translation()[k], scale() only,
//             so the host keeps g2o::Sim3 or replaces it by any type with those three members
// Differences from the reference's text, all where it would dereference a null vertex: a bad keyframe gets no vertex (as there), and here
// it also gets no edges, no pose write-back, and a map point whose reference keyframe has no vertex is left alone.  One more difference:
// the map points' world positions are read before the call and outside Map::m_mutex_updateMap (the GPU corrects them in the same call),
// where the reference reads each one under the lock after the optimisation; a position written by another thread during the call is
// overwritten.  correctLoop runs with LocalMapping stopped, so nothing writes them then.
struct Sim3d {   // g2o::Sim3 as the C ABI stores it
  double q[4], t[3], s;   // q = x y z w
  static void rot(const double* q, const double* v, double* o) {   // Eigen quaternion * vector
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int k = 0; k < 3; k++) o[k] = (v[k] + uv[k] * q[3]) + c[k];
  }
  Sim3d operator*(const Sim3d& b) const {   // r = r * b.r, t = s * (r * b.t) + t, s = s * b.s
    Sim3d o;
    o.q[0] = q[3] * b.q[0] + q[0] * b.q[3] + q[1] * b.q[2] - q[2] * b.q[1];
    o.q[1] = q[3] * b.q[1] + q[1] * b.q[3] + q[2] * b.q[0] - q[0] * b.q[2];
    o.q[2] = q[3] * b.q[2] + q[2] * b.q[3] + q[0] * b.q[1] - q[1] * b.q[0];
    o.q[3] = q[3] * b.q[3] - q[0] * b.q[0] - q[1] * b.q[1] - q[2] * b.q[2];
    double r[3];
    rot(q, b.t, r);
    for (int k = 0; k < 3; k++) o.t[k] = r[k] * s + t[k];
    o.s = s * b.s;
    return o;
  }
  Sim3d inverse() const {   // (r^-1, r^-1 * ((-1 / s) * t), 1 / s)
    Sim3d o;
    o.q[0] = -q[0]; o.q[1] = -q[1]; o.q[2] = -q[2]; o.q[3] = q[3];
    const double f = -1. / s, v[3] = {t[0] * f, t[1] * f, t[2] * f};
    rot(o.q, v, o.t);
    o.s = 1. / s;
    return o;
  }
  template <class Sim3T> static Sim3d from(const Sim3T& S) {
    Sim3d o;
    o.q[0] = S.rotation().x(); o.q[1] = S.rotation().y(); o.q[2] = S.rotation().z(); o.q[3] = S.rotation().w();
    for (int k = 0; k < 3; k++) o.t[k] = S.translation()[k];
    o.s = S.scale();
    return o;
  }
};

// The graph of one optimizeEssentialGraph call: vertices in the order of the map's keyframes (bad ones skipped, mnId compacted to dense
// indices), edges in the reference's order.
template <class KeyFramePtr>
struct EssentialGraphData {
  std::vector<KeyFramePtr> vertexKF;
  std::map<long int, int> vertexOf;   // mnId -> vertex
  std::vector<double> sim3;           // [V][8], vScw
  std::vector<uint8_t> fixed;
  std::vector<int32_t> v0, v1;
  std::vector<double> meas;           // [E][8]
};

template <class KeyFramePtr, class MapPtr, class PoseMap, class ConnMap>
EssentialGraphData<KeyFramePtr> buildEssentialGraph(MapPtr map, KeyFramePtr loopKF, KeyFramePtr curKF, const PoseMap& nonCorrectedSim3,
                                                    const PoseMap& correctedSim3, const ConnMap& loopConnections) {
  EssentialGraphData<KeyFramePtr> G;
  const std::vector<KeyFramePtr> kfs = map->getAllKeyFrames();
  const int minFeat = 100;
  std::vector<Sim3d> vScw;
  for (const KeyFramePtr& kf : kfs) {   // Set KeyFrame vertices
    if (kf->isBad()) continue;
    Sim3d S;
    const auto it = correctedSim3.find(kf);
    if (it != correctedSim3.end()) {
      S = Sim3d::from(it->second);
    } else {   // g2o::Sim3(Rcw, tcw, 1.0): the float pose in double, the quaternion Eigen makes of the matrix
      const cv::Mat Rcw = kf->getRotation_c2w(), tcw = kf->getTranslation_c2w();
      Eigen::Matrix3d R;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R(i, j) = Rcw.at<float>(i, j);
      const Eigen::Quaterniond q(R);
      S.q[0] = q.x(); S.q[1] = q.y(); S.q[2] = q.z(); S.q[3] = q.w();
      for (int k = 0; k < 3; k++) S.t[k] = tcw.at<float>(k);
      S.s = 1.0;
    }
    G.vertexOf[kf->m_int_keyFrameID] = (int)G.vertexKF.size();
    G.vertexKF.push_back(kf);
    vScw.push_back(S);
    G.fixed.push_back(kf == loopKF ? 1 : 0);
  }
  auto vertex = [&](const KeyFramePtr& kf) -> int {
    const auto it = G.vertexOf.find(kf->m_int_keyFrameID);
    return it == G.vertexOf.end() ? -1 : it->second;
  };
  auto addEdge = [&](int i, int j, const Sim3d& Sji) {   // vertex(0) = i, vertex(1) = j
    G.v0.push_back(i); G.v1.push_back(j);
    for (int k = 0; k < 4; k++) G.meas.push_back(Sji.q[k]);
    for (int k = 0; k < 3; k++) G.meas.push_back(Sji.t[k]);
    G.meas.push_back(Sji.s);
  };
  auto nonCorrected = [&](const KeyFramePtr& kf, int v) -> Sim3d {   // the pose before the loop correction, where the keyframe had one
    const auto it = nonCorrectedSim3.find(kf);
    return it != nonCorrectedSim3.end() ? Sim3d::from(it->second) : vScw[v];
  };
  std::set<std::pair<long int, long int>> inserted;
  for (const auto& conn : loopConnections) {   // Set Loop edges
    const KeyFramePtr& kf = conn.first;
    const int vi = vertex(kf);
    if (vi < 0) continue;
    const long int idi = kf->m_int_keyFrameID;
    const Sim3d Swi = vScw[vi].inverse();
    for (const KeyFramePtr& other : conn.second) {
      const long int idj = other->m_int_keyFrameID;
      if ((idi != curKF->m_int_keyFrameID || idj != loopKF->m_int_keyFrameID) && kf->getWeight(other) < minFeat) continue;
      const int vj = vertex(other);
      if (vj < 0) continue;
      addEdge(vi, vj, vScw[vj] * Swi);
      inserted.insert(std::make_pair(std::min(idi, idj), std::max(idi, idj)));
    }
  }
  for (const KeyFramePtr& kf : kfs) {   // Set normal edges
    const int vi = vertex(kf);
    if (vi < 0) continue;
    const long int idi = kf->m_int_keyFrameID;
    const Sim3d Swi = nonCorrected(kf, vi).inverse();
    const KeyFramePtr parent = kf->getParent();
    if (parent) {   // Spanning tree edge
      const int vj = vertex(parent);
      if (vj >= 0) addEdge(vi, vj, nonCorrected(parent, vj) * Swi);
    }
    const auto loopEdges = kf->getLoopEdges();   // Loop edges
    for (const KeyFramePtr& l : loopEdges) {
      if (l->m_int_keyFrameID >= idi) continue;
      const int vl = vertex(l);
      if (vl >= 0) addEdge(vi, vl, nonCorrected(l, vl) * Swi);
    }
    for (const KeyFramePtr& n : kf->getCovisiblesByWeight(minFeat)) {   // Covisibility graph edges
      if (!n || n == parent || kf->hasChild(n) || loopEdges.count(n)) continue;
      if (n->isBad() || n->m_int_keyFrameID >= idi) continue;
      if (inserted.count(std::make_pair(std::min(idi, (long int)n->m_int_keyFrameID), std::max(idi, (long int)n->m_int_keyFrameID)))) continue;
      const int vn = vertex(n);
      if (vn >= 0) addEdge(vi, vn, nonCorrected(n, vn) * Swi);
    }
  }
  G.sim3.resize(8 * vScw.size());
  for (size_t v = 0; v < vScw.size(); v++) {
    for (int k = 0; k < 4; k++) G.sim3[8 * v + k] = vScw[v].q[k];
    for (int k = 0; k < 3; k++) G.sim3[8 * v + 4 + k] = vScw[v].t[k];
    G.sim3[8 * v + 7] = vScw[v].s;
  }
  return G;
}

template <class FrameT, class KeyFramePtr, class MapPtr, class PoseMap, class ConnMap>
void optimizeEssentialGraphImpl(MapPtr map, KeyFramePtr loopKF, KeyFramePtr curKF, const PoseMap& nonCorrectedSim3, const PoseMap& correctedSim3,
                                const ConnMap& loopConnections, const bool& fixScale, int device = 0, int solver = YDORB_ESS_SOLVER_AUTO) {
  EssentialGraphData<KeyFramePtr> G = buildEssentialGraph(map, loopKF, curKF, nonCorrectedSim3, correctedSim3, loopConnections);
  // every good map point with the vertex of its reference keyframe, or of the keyframe that corrected it in correctLoop
  const auto mps = map->getAllMapPoints();
  typedef typename std::decay<decltype(mps[0])>::type MapPointPtr;
  std::vector<MapPointPtr> pointMP;
  std::vector<float> points;
  std::vector<int32_t> pointRef;
  for (const MapPointPtr& mp : mps) {
    if (!mp || mp->isBad()) continue;
    const long int idr = mp->m_int_correctedByKeyFrameID == curKF->m_int_keyFrameID ? (long int)mp->m_int_correctedReference
                                                                                    : (long int)mp->getReferenceKeyFrame()->m_int_keyFrameID;
    const auto it = G.vertexOf.find(idr);
    if (it == G.vertexOf.end()) continue;
    const cv::Mat X = mp->getPosInWorld();
    for (int d = 0; d < 3; d++) points.push_back(X.at<float>(d));
    pointRef.push_back(it->second);
    pointMP.push_back(mp);
  }
  YdEssentialGraph P{};
  P.device = device; P.n_vertices = (int32_t)G.vertexKF.size(); P.n_edges = (int32_t)G.v0.size(); P.n_points = (int32_t)pointMP.size();
  P.sim3 = G.sim3.data(); P.fixed = G.fixed.data(); P.edge_v0 = G.v0.data(); P.edge_v1 = G.v1.data(); P.edge_meas = G.meas.data();
  P.points = points.data(); P.point_ref = pointRef.data();
  P.fix_scale = fixScale ? 1 : 0; P.iterations = 20; P.max_trials = 10; P.lambda_init = 1e-16;
  std::vector<float> corrected(points.size() + 3);
  YdBaResult res{};
  // AUTO: the dense solver while the map fits it (2 742 free keyframes), the block-skyline one above
  YdEssentialSolverOptions opt{};
  opt.solver = solver;
  if (ydorb_essential_graph_optimize_with(&P, &opt, corrected.data(), &res, nullptr) != YDORB_OK)
    throw std::runtime_error(std::string("ydorb: ") + ydorb_last_error());
  std::unique_lock<std::mutex> lock(map->m_mutex_updateMap);
  for (size_t v = 0; v < G.vertexKF.size(); v++) {   // SE3 pose recovering: Sim3 [sR t; 0 1] -> SE3 [R t/s; 0 1]
    const double* S = &G.sim3[8 * v];
    const Eigen::Matrix3d R = Eigen::Quaterniond(S[3], S[0], S[1], S[2]).toRotationMatrix();
    const double inv = 1. / S[7];
    cv::Mat Tiw = cv::Mat::eye(4, 4, CV_32F);
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Tiw.at<float>(i, j) = (float)R(i, j);
      Tiw.at<float>(i, 3) = (float)(S[4 + i] * inv);
    }
    G.vertexKF[v]->setCameraPoseByTransform_c2w(Tiw);
  }
  for (size_t p = 0; p < pointMP.size(); p++) {   // correct points
    cv::Mat X(3, 1, CV_32F);
    for (int d = 0; d < 3; d++) X.at<float>(d) = corrected[3 * p + d];
    pointMP[p]->setPosInWorld(X);
    pointMP[p]->updateNormalAndDepth();
  }
}

// Optimizer::globalBundleAdjust (optimizer.cpp:353-357)
template <class FrameT, class MapPtr>
void globalBundleAdjustImpl(MapPtr map, int iterNum, const volatile bool* stop, long int loopKeyFrameID, bool robust, int solver = YDORB_BA_SOLVER_AUTO) {
  bundleAdjustImpl<FrameT>(map->getAllKeyFrames(), map->getAllMapPoints(), iterNum, stop, loopKeyFrameID, robust, solver);
}

}  // namespace adapter
}  // namespace ydorb
#endif
