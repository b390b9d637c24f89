// Host driver of the Frame constructor's tail + its C ABI (include/ydorb/c_api.h, "Frame construction"): ydorb_undistort_points,
// ydorb_image_bounds, ydorb_frame_tail, ydorb_extract_rgbd, ydorb_frame_release.  The host forms copy their inputs into one pinned
// staging area, upload it in one copy, run the kernels and read every output back in one copy behind one synchronise; the
// device-pointer form of ydorb_frame_tail only enqueues.  ydorb_extract_rgbd puts the extractor's device entry in front of the
// same launches on the same stream, so a frame leaves the GPU once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>

#include "../../include/ydorb/c_api.h"
#include "frame_kernels.hip.h"
#include "host_buffers.h"
#include "ydorb_host.h"

using namespace ydorb;
using namespace ydorb::frame;

namespace {

StagedCtx g_ctx[16];   // this driver's own: nothing is shared with the other staged solvers

static_assert(sizeof(YdKeyPoint) == sizeof(KeyPointDev), "YdKeyPoint is the kernels' keypoint");
static_assert((int)kDepthNone == YDORB_DEPTH_NONE && (int)kDepthU16 == YDORB_DEPTH_U16 && (int)kDepthF32 == YDORB_DEPTH_F32 &&
              (int)kDepthSamples == YDORB_DEPTH_SAMPLES && (int)kStatusDepthIndex == YDORB_FRAME_STATUS_DEPTH_INDEX &&
              (int)kStatusIcdist == YDORB_FRAME_STATUS_ICDIST && (int)kFlagDepthAtUndistorted == YDORB_FRAME_DEPTH_AT_UNDISTORTED,
              "the kernels' constants are the header's");

int invalid(const char* what) { set_error("frame: %s", what); return YDORB_ERR_INVALID_ARG; }

CamDev camDev(const YdCamera& c) { return CamDev{c.fx, c.fy, c.cx, c.cy, c.dist[0], c.dist[1], c.dist[2], c.dist[3], c.dist[4], c.n_iter}; }

size_t depthElem(int type) { return type == YDORB_DEPTH_U16 ? 2 : 4; }

// The launches of one tail on `s`.  T.kpsUn may be null when neither the caller nor the grid wants the keypoints; maxN bounds the
// counts where the host knows them (cap otherwise).
int enqueueTail(const TailArgs& T, int maxN, const float* bounds, int* cellStart, int* cellIdx, hipStream_t s) {
  if (T.status) HIPCHK(hipMemsetAsync(T.status, 0, sizeof(int) * (size_t)T.nFrames, s));
  if (maxN > 0 && (T.kpsUn || T.rightX || T.depthOut || T.status))
    hipLaunchKernelGGL(k_frame_tail, dim3((maxN + kThreads - 1) / kThreads, T.nFrames), dim3(kThreads), 0, s, T);
  if (cellStart) {
    GridArgs G;
    G.kpsUn = T.kpsUn; G.n = T.n; G.cap = T.cap; G.minX = bounds[0];
    G.gridWInv = static_cast<float>(kGridCols) / (bounds[1] - bounds[0]);   // frame.cpp:99-100, as the matcher computes them
    G.gridHInv = static_cast<float>(kGridRows) / (bounds[3] - bounds[2]);
    G.cellStart = cellStart; G.cellIdx = cellIdx;
    const size_t dyn = sizeof(int16_t) * (size_t)T.cap;
    if (dyn > 48 * 1024)
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_frame_grid), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    hipLaunchKernelGGL(k_frame_grid, dim3(T.nFrames), dim3(256), dyn, s, G);
  }
  HIPCHK(hipGetLastError());
  return YDORB_OK;
}

int checkCamera(const YdCamera* cam) {
  if (!cam) return invalid("null camera");
  if (cam->n_iter < 1) return invalid("camera n_iter must be at least 1");
  return YDORB_OK;
}

int checkGrid(const int32_t* cellStart, const int32_t* cellIdx, const float* bounds, int cap) {
  if (!cellStart && !cellIdx) return YDORB_OK;
  if (!cellStart || !cellIdx) return invalid("cell_start and cell_idx go together");
  if (!bounds || !(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2])) return invalid("the grid needs bounds with max > min");
  if (cap > 65535) return invalid("the grid takes at most 65535 keypoints per frame");
  return YDORB_OK;
}

// xy [n][2] -> out [n][2] through k_undistort_points; the caller holds c.mu and has validated.
int undistortStaged(StagedCtx& c, const YdCamera& cam, const float* xy, int n, float* out) {
  int rc;
  const size_t bytes = sizeof(float2) * (size_t)n;
  if ((rc = c.ensure(bytes, bytes))) return rc;
  std::memcpy(c.hUp.p, xy, bytes);
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, bytes, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_undistort_points, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, camDev(cam), c.up.as<float2>(), n, c.down.as<float2>(),
                     static_cast<int*>(nullptr));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(out, c.hDown.p, bytes);
  return YDORB_OK;
}

// Offsets of the outputs inside the read-back area (device copy and pinned copy alike); npos = not asked for.
constexpr size_t npos = ~(size_t)0;
struct DownLayout {
  Layout D;
  size_t kpsUn = npos, rightX = npos, depth = npos, cellStart = npos, cellIdx = npos, status = npos;
  DownLayout(size_t nFrames, size_t cap, bool wantUn, bool wantRx, bool wantDepth, bool wantGrid, bool wantStatus) {
    const size_t total = nFrames * cap;
    if (wantUn || wantGrid) kpsUn = D.add(sizeof(YdKeyPoint) * total);
    if (wantRx) rightX = D.add(4 * total);
    if (wantDepth) depth = D.add(4 * total);
    if (wantGrid) { cellStart = D.add(4 * nFrames * (kGridCells + 1)); cellIdx = D.add(4 * total); }
    if (wantStatus) status = D.add(4 * nFrames);
  }
  template <class T> T* ptr(Mem& m, size_t off) const { return off == npos ? nullptr : m.at<T>(off); }
};

int frameTailDevice(const YdFrameTail* B, YdKeyPoint* kpsUn, float* rightX, float* depth, int32_t* cellStart, int32_t* cellIdx, int32_t* status,
                    void* stream) {
  StagedCtx& c = g_ctx[B->device];
  std::lock_guard<std::mutex> lock(c.mu);
  int rc = c.init(B->device);
  if (rc) return rc;
  if (cellStart && !kpsUn) {   // the grid reads the undistorted keypoints: keep them in scratch
    if ((rc = c.scratch.ensure(sizeof(YdKeyPoint) * (size_t)B->n_frames * B->cap))) return rc;
    kpsUn = c.scratch.as<YdKeyPoint>();
  }
  TailArgs T{};
  T.kps = reinterpret_cast<const KeyPointDev*>(B->kps); T.n = B->n; T.nFrames = B->n_frames; T.cap = B->cap;
  T.depth = B->depth; T.depthType = B->depth ? B->depth_type : (int)YDORB_DEPTH_NONE; T.w = B->depth_w; T.h = B->depth_h;
  T.rowStride = B->depth_row_stride; T.frameStride = B->depth_frame_stride; T.factor = B->depth_factor;
  T.cam = camDev(B->cam); T.bf = B->bf; T.flags = B->flags;
  T.kpsUn = reinterpret_cast<KeyPointDev*>(kpsUn); T.rightX = rightX; T.depthOut = depth; T.status = status;
  return enqueueTail(T, B->cap, B->bounds, cellStart, cellIdx, stream ? (hipStream_t)stream : c.stream);
}

}  // namespace

extern "C" int ydorb_undistort_points(const YdCamera* cam, const float* xy, int32_t n, float* xy_out, int32_t device) {
  int rc = checkCamera(cam);
  if (rc) return rc;
  if (n < 0 || device < 0 || device >= 16) return invalid("negative count or invalid device");
  if (n > 0 && (!xy || !xy_out)) return invalid("null point arrays");
  if ((rc = require_device(device))) return rc;
  if (n == 0) return YDORB_OK;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  return undistortStaged(c, *cam, xy, n, xy_out);
}

extern "C" int ydorb_image_bounds(const YdCamera* cam, int32_t w, int32_t hgt, float* bounds, int32_t device) {
  int rc = checkCamera(cam);
  if (rc) return rc;
  if (w <= 0 || hgt <= 0 || !bounds || device < 0 || device >= 16) return invalid("image bounds need a size, an output and a device");
  if ((rc = require_device(device))) return rc;
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  const float corners[8] = {0.f, 0.f, (float)w, 0.f, 0.f, (float)hgt, (float)w, (float)hgt};
  float un[8];
  if ((rc = undistortStaged(c, *cam, corners, 4, un))) return rc;
  bounds[0] = std::min(un[0], un[4]); bounds[1] = std::max(un[2], un[6]);
  bounds[2] = std::min(un[1], un[3]); bounds[3] = std::max(un[5], un[7]);
  return YDORB_OK;
}

extern "C" int ydorb_frame_tail(const YdFrameTail* B, YdKeyPoint* kpsUn, float* rightX, float* depth, int32_t* cellStart, int32_t* cellIdx,
                                int32_t* status, void* stream) {
  if (!B || B->n_frames < 0 || B->cap < 0 || B->device < 0 || B->device >= 16) return invalid("invalid batch");
  int rc = checkCamera(&B->cam);
  if (rc) return rc;
  const int nF = B->n_frames, cap = B->cap;
  if (nF > 0 && !B->n) return invalid("null counts");
  if (nF > 0 && cap > 0 && !B->kps) return invalid("null keypoints");
  const int type = B->depth_type;
  if (type < YDORB_DEPTH_NONE || type > YDORB_DEPTH_SAMPLES) return invalid("unknown depth type");
  const bool image = type == YDORB_DEPTH_U16 || type == YDORB_DEPTH_F32;
  if (type != YDORB_DEPTH_NONE && nF > 0 && cap > 0 && !B->depth) return invalid("null depth with a depth source");
  if (image) {
    if (B->depth_w <= 0 || B->depth_h <= 0) return invalid("depth image without a size");
    if (B->depth_row_stride < (int64_t)(depthElem(type) * (size_t)B->depth_w)) return invalid("depth row stride smaller than a row");
    if (nF > 1 && B->depth_frame_stride < 0) return invalid("negative depth frame stride");
  }
  if ((rc = checkGrid(cellStart, cellIdx, B->bounds, cap))) return rc;
  const bool devPtrs = (B->flags & YDORB_FRAME_DEVICE_POINTERS) != 0;
  int maxN = 0;
  if (!devPtrs)
    for (int f = 0; f < nF; f++) {
      if (B->n[f] < 0 || B->n[f] > cap) {
        set_error("frame: frame %d: count %d outside 0..cap %d", f, B->n[f], cap);
        return YDORB_ERR_INVALID_ARG;
      }
      maxN = std::max(maxN, B->n[f]);
    }
  if ((rc = require_device(B->device))) return rc;
  if (nF == 0) return YDORB_OK;
  if (devPtrs) return frameTailDevice(B, kpsUn, rightX, depth, cellStart, cellIdx, status, stream);

  StagedCtx& c = g_ctx[B->device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(B->device))) return rc;
  const size_t total = (size_t)nF * cap, rowBytes = image ? depthElem(type) * (size_t)B->depth_w : 0, imgBytes = rowBytes * (image ? B->depth_h : 0);
  Layout U;
  const size_t oN = U.add(4 * (size_t)nF), oKps = U.add(sizeof(YdKeyPoint) * total),
               oDepth = U.add(image ? imgBytes * nF : type == YDORB_DEPTH_SAMPLES ? 4 * total : 0);
  const DownLayout L(nF, cap, kpsUn, rightX, depth, cellStart, status);
  if ((rc = c.ensure(U.bytes, L.D.bytes))) return rc;
  std::memcpy(at<void>(c.hUp, oN), B->n, 4 * (size_t)nF);
  for (int f = 0; f < nF; f++) {
    const size_t n = B->n[f];
    std::memcpy(at<YdKeyPoint>(c.hUp, oKps) + (size_t)f * cap, B->kps + (size_t)f * cap, sizeof(YdKeyPoint) * n);
    if (type == YDORB_DEPTH_SAMPLES)
      std::memcpy(at<float>(c.hUp, oDepth) + (size_t)f * cap, static_cast<const float*>(B->depth) + (size_t)f * cap, 4 * n);
    if (image)   // rows packed tightly in the staging area
      for (int r = 0; r < B->depth_h; r++)
        std::memcpy(at<uint8_t>(c.hUp, oDepth) + (size_t)f * imgBytes + (size_t)r * rowBytes,
                    static_cast<const uint8_t*>(B->depth) + (size_t)f * B->depth_frame_stride + (size_t)r * B->depth_row_stride, rowBytes);
  }
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  TailArgs T{};
  T.kps = at<KeyPointDev>(c.up, oKps); T.n = at<int>(c.up, oN); T.nFrames = nF; T.cap = cap;
  T.depth = type == YDORB_DEPTH_NONE ? nullptr : at<void>(c.up, oDepth); T.depthType = type; T.w = B->depth_w; T.h = B->depth_h;
  T.rowStride = (long long)rowBytes; T.frameStride = (long long)imgBytes; T.factor = B->depth_factor;
  T.cam = camDev(B->cam); T.bf = B->bf; T.flags = B->flags;
  T.kpsUn = L.ptr<KeyPointDev>(c.down, L.kpsUn); T.rightX = L.ptr<float>(c.down, L.rightX); T.depthOut = L.ptr<float>(c.down, L.depth);
  T.status = L.ptr<int>(c.down, L.status);
  if ((rc = enqueueTail(T, maxN, B->bounds, L.ptr<int>(c.down, L.cellStart), L.ptr<int>(c.down, L.cellIdx), s))) return rc;
  if (L.D.bytes) HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, L.D.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int f = 0; f < nF; f++) {
    const size_t n = B->n[f], o = (size_t)f * cap;
    if (kpsUn) std::memcpy(kpsUn + o, L.ptr<YdKeyPoint>(c.hDown, L.kpsUn) + o, sizeof(YdKeyPoint) * n);
    if (rightX) std::memcpy(rightX + o, L.ptr<float>(c.hDown, L.rightX) + o, 4 * n);
    if (depth) std::memcpy(depth + o, L.ptr<float>(c.hDown, L.depth) + o, 4 * n);
    if (cellIdx) std::memcpy(cellIdx + o, L.ptr<int>(c.hDown, L.cellIdx) + o, 4 * n);
  }
  if (cellStart) std::memcpy(cellStart, L.ptr<int>(c.hDown, L.cellStart), 4 * (size_t)nF * (kGridCells + 1));
  if (status) std::memcpy(status, L.ptr<int>(c.hDown, L.status), 4 * (size_t)nF);
  return YDORB_OK;
}

extern "C" int ydorb_extract_rgbd(ydorb_extractor_t* h, const uint8_t* gray, int32_t w, int32_t hgt, int32_t stride, const void* depthImg,
                                  int32_t depthType, int32_t depthStride, float depthFactor, const YdCamera* cam, float bf, const float* bounds,
                                  int32_t flags, YdKeyPoint* kpsRaw, YdKeyPoint* kpsUn, uint8_t* desc, float* rightX, float* depthOut,
                                  int32_t* cellStart, int32_t* cellIdx, int32_t cap, int32_t* nOut, int32_t* status) {
  if (!h || !nOut) return invalid("null extractor or n_out");
  int rc = checkCamera(cam);
  if (rc) return rc;
  if (flags & YDORB_FRAME_DEVICE_POINTERS) return invalid("ydorb_extract_rgbd takes host pointers");
  if (!depthImg) depthType = YDORB_DEPTH_NONE;
  if (depthType != YDORB_DEPTH_NONE && depthType != YDORB_DEPTH_U16 && depthType != YDORB_DEPTH_F32) return invalid("depth must be an image or absent");
  if ((rc = checkGrid(cellStart, cellIdx, bounds, ydorb_extractor_max_keypoints(h)))) return rc;
  if (!gray || w <= 0 || hgt <= 0) {   // empty image: silent return, orbExtractor.cpp:357-359
    *nOut = 0;
    if (status) *status = 0;
    return YDORB_OK;
  }
  if (!kpsRaw || !desc || cap < 0 || stride < w) return invalid("null keypoint or descriptor buffer, or stride below the width");
  const size_t rowBytes = depthType == YDORB_DEPTH_NONE ? 0 : depthElem(depthType) * (size_t)w, depthBytes = rowBytes * hgt, grayBytes = (size_t)w * hgt;
  if (depthType != YDORB_DEPTH_NONE && (size_t)std::max(depthStride, 0) < rowBytes) return invalid("depth row stride smaller than a row");
  // the handle's device: its pyramid view names it once the handle has run; before that its synchronise makes it current
  int device = -1;
  PyramidView pv;
  if (extractor_pyramid_view(h, &pv) == YDORB_OK) device = pv.device;
  else if ((rc = ydorb_extractor_synchronize(h))) return rc;
  else HIPCHK(hipGetDevice(&device));
  if (device < 0 || device >= 16) return invalid("extractor on an unsupported device ordinal");
  StagedCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lock(c.mu);
  if ((rc = c.init(device))) return rc;
  const int Q = ydorb_extractor_max_keypoints(h);
  Layout U;
  const size_t oGray = U.add(grayBytes), oDepth = U.add(depthBytes);
  Layout X;   // what the extractor writes, in front of the tail's outputs in the one read-back area
  const size_t oN = X.add(4), oRaw = X.add(sizeof(YdKeyPoint) * (size_t)Q), oDesc = X.add((size_t)32 * Q);
  const DownLayout L(1, Q, kpsUn, rightX, depthOut, cellStart, status);
  const size_t downBytes = X.bytes + L.D.bytes;
  if ((rc = c.ensure(U.bytes, downBytes))) return rc;
  for (int r = 0; r < hgt; r++) {
    std::memcpy(at<uint8_t>(c.hUp, oGray) + (size_t)r * w, gray + (size_t)r * stride, w);
    if (rowBytes) std::memcpy(at<uint8_t>(c.hUp, oDepth) + (size_t)r * rowBytes, static_cast<const uint8_t*>(depthImg) + (size_t)r * depthStride, rowBytes);
  }
  hipStream_t s = c.stream;
  HIPCHK(hipMemcpyAsync(c.up.p, c.hUp.p, U.bytes, hipMemcpyHostToDevice, s));
  if ((rc = ydorb_extract_batch_device(h, at<uint8_t>(c.up, oGray), w, hgt, w, 0, 1, at<YdKeyPoint>(c.down, oRaw), at<uint8_t>(c.down, oDesc), Q,
                                       at<int32_t>(c.down, oN), s)))
    return rc;
  auto out = [&](size_t off) { return off == npos ? npos : X.bytes + off; };
  TailArgs T{};
  T.kps = at<KeyPointDev>(c.down, oRaw); T.n = at<int>(c.down, oN); T.nFrames = 1; T.cap = Q;
  T.depth = rowBytes ? at<void>(c.up, oDepth) : nullptr; T.depthType = depthType; T.w = w; T.h = hgt;
  T.rowStride = (long long)rowBytes; T.frameStride = 0; T.factor = depthFactor;
  T.cam = camDev(*cam); T.bf = bf; T.flags = flags;
  T.kpsUn = L.ptr<KeyPointDev>(c.down, out(L.kpsUn)); T.rightX = L.ptr<float>(c.down, out(L.rightX)); T.depthOut = L.ptr<float>(c.down, out(L.depth));
  T.status = L.ptr<int>(c.down, out(L.status));
  if ((rc = enqueueTail(T, Q, bounds, L.ptr<int>(c.down, out(L.cellStart)), L.ptr<int>(c.down, out(L.cellIdx)), s))) return rc;
  HIPCHK(hipMemcpyAsync(c.hDown.p, c.down.p, downBytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // the device entry of the extractor reports its capacity errors here; its streams are idle by now
  if ((rc = ydorb_extractor_synchronize(h))) return rc;
  const int n = *at<int32_t>(c.hDown, oN);
  if (n > cap) { set_error("frame has %d keypoints, caller capacity %d", n, cap); return YDORB_ERR_CAPACITY; }
  *nOut = n;
  std::memcpy(kpsRaw, at<void>(c.hDown, oRaw), sizeof(YdKeyPoint) * (size_t)n);
  std::memcpy(desc, at<void>(c.hDown, oDesc), (size_t)32 * n);
  if (kpsUn) std::memcpy(kpsUn, L.ptr<void>(c.hDown, out(L.kpsUn)), sizeof(YdKeyPoint) * (size_t)n);
  if (rightX) std::memcpy(rightX, L.ptr<void>(c.hDown, out(L.rightX)), 4 * (size_t)n);
  if (depthOut) std::memcpy(depthOut, L.ptr<void>(c.hDown, out(L.depth)), 4 * (size_t)n);
  if (cellStart) std::memcpy(cellStart, L.ptr<void>(c.hDown, out(L.cellStart)), 4 * (size_t)(kGridCells + 1));
  if (cellIdx) std::memcpy(cellIdx, L.ptr<void>(c.hDown, out(L.cellIdx)), 4 * (size_t)n);
  if (status) *status = *L.ptr<int>(c.hDown, out(L.status));
  return YDORB_OK;
}

extern "C" int ydorb_frame_release(int32_t device) { return release_staged(g_ctx, device); }
