"""The host LM schedule of the BA driver (ydorbslam_amd/csrc/lm_schedule.h) against a nested-loop transcription of g2o's, on the CPU.

The single solve and the lock-step batch of ba_solver.hip step the same LmSchedule.  Its branches on non-finite values (rho = NaN:
rejected without a retry, chi2 recomputed at the next iteration; lambda = +-inf: break after counting the trial) cannot be reached by a
GPU test whose decisions are stable under rounding, so they are driven here by a scripted stream of the scalars the device would
return.  tests/cpu_harness/lm_schedule_check.cpp is a program of its own, built with the address and undefined-behaviour sanitizers;
nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_harness", "lm_schedule_check.cpp")
HEADER = os.path.join(ROOT, "ydorbslam_amd", "csrc", "lm_schedule.h")

BRANCHES = ["rejected trial, then a retry", "iteration ended by max_trials", "iteration ended by rho == 0", "iteration ended by a non-finite lambda",
            "trial with rho = NaN", "chi2 recomputed after a rejected last trial", "failed solve", "second stage left at noEdgesLeft",
            "stage with 0 iterations", "stop seen before an iteration", "stop seen after a trial", "stop seen at the hand-over",
            "stop seen at the start of a stage", "single-stage run", "more than 32 iterations"]


def test_schedule_equals_the_nested_loops_on_scripted_streams(tmp_path):
    """20 000 seeded streams: log rows (NaN equal to NaN), n_trials, n_iterations, the accept sequence, the number of culls, stopped and
    the order in which the scalars are asked for are those of the reference loops, for the schedule stepped as the single solve steps
    it and as a batch member does.  Every branch listed above must have occurred on the reference side."""
    exe = str(tmp_path / "lm_schedule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    r = subprocess.run([exe, "20000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[0].startswith("20000 streams") and lines[0].endswith(" 0 mismatches")
    counts = {l[2:48].strip(): int(l[48:]) for l in lines[1:] if l.startswith("  ")}
    assert sorted(counts) == sorted(BRANCHES)
    assert all(n > 0 for n in counts.values()), counts


def test_schedule_header_has_no_hip():
    """It is the part of the driver that a plain host compiler builds: no HIP header, qualifier or runtime call."""
    text = open(HEADER).read()
    assert "#include <hip" not in text and "hipStream" not in text and "__global__" not in text
