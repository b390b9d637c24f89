"""ydorbslam_amd — MI355X-native (gfx950) ORB front-end, descriptor matcher and local-BA back-end.

The package is a thin ctypes mirror of the C ABI in include/ydorb/c_api.h (the drop-in boundary of the
reference's OrbExtractor / OrbMatcher / Optimizer hot path).  All computation happens in
ydorbslam_amd/libydorb.so (host C++ + hand-written HIP kernels).  There is no CPU fallback: importing
succeeds without the library, but every operator raises YdorbError until it is built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C ydorbslam_amd/csrc`).
"""
from ._lib import YdorbError, lib, library_path, build_library  # noqa: F401
from .extractor import OrbExtractor, KP_DTYPE  # noqa: F401
from .matcher import OrbMatcher, FrameView, FeatureVector, QUERY_DTYPE  # noqa: F401
from .optimizer import Optimizer  # noqa: F401
from .vocabulary import Vocabulary  # noqa: F401
from .sim3 import Sim3Solver, optimize_sim3  # noqa: F401
from .pnp import PnPsolver  # noqa: F401
from .kfdb import KeyFrameDatabase  # noqa: F401
from .triangulate import triangulate_matches  # noqa: F401
from .frustum import frustum_cull, search_local_points  # noqa: F401
from .frame import extract_rgbd, frame_tail, image_bounds, undistort_points  # noqa: F401
from .essential_graph import optimize_essential_graph  # noqa: F401
from .map_maintenance import COVIS_WINDOW, ObservationTable, covisibility, keyframe_redundancy, update_normal_depth  # noqa: F401
from .map_resident import MapDb  # noqa: F401

__all__ = ["YdorbError", "lib", "library_path", "build_library", "OrbExtractor", "KP_DTYPE", "OrbMatcher", "FrameView",
           "FeatureVector", "QUERY_DTYPE", "Optimizer", "Vocabulary", "Sim3Solver", "optimize_sim3", "PnPsolver", "KeyFrameDatabase",
           "triangulate_matches", "frustum_cull", "search_local_points", "extract_rgbd", "frame_tail", "image_bounds", "undistort_points",
           "optimize_essential_graph", "ObservationTable", "update_normal_depth", "covisibility", "keyframe_redundancy", "COVIS_WINDOW", "MapDb"]
