"""The C++ adapters (include/ydorb/*.hpp, reference signatures over the C ABI) type-check against declarations of the
reference types they touch.  OpenCV is absent here, so a declaration-only mock stands in for <opencv2/core.hpp>, and the Eigen
stand-in of tests/cpu_harness/mockrt for <Eigen/Core> / <Eigen/Geometry> (test-only).  This is the type check alone: the bodies are
EXECUTED by the *_adapter_gpu.py modules, tests/test_adapter_exec.py and, for the projection, Sim3, fuse, triangulation and stereo
bodies of orbMatcher.hpp / frame.hpp, tests/test_matcher_adapters_gpu.py; DESIGN.md section 6w lists every body with its test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "tests", "cpu_harness")


def _syntax(src, *extra):
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(H, "mock"), *extra, os.path.join(H, src)])


def test_extractor_adapter_typechecks():
    _syntax("adapter_syntax_check_extractor.cpp")


def test_matcher_adapter_typechecks():
    _syntax("adapter_syntax_check.cpp")


def test_optimizer_adapter_typechecks():
    # Eigen: the test-only stand-in of tests/cpu_harness/mockrt (the two types optimizer.hpp uses), so the check needs nothing outside the repository
    eigen = os.path.join(H, "mockrt")
    assert os.path.isfile(os.path.join(eigen, "Eigen", "Core")) and os.path.isfile(os.path.join(eigen, "Eigen", "Geometry"))
    _syntax("adapter_syntax_check.cpp", "-DYDORB_CHECK_OPTIMIZER", "-I" + eigen)
