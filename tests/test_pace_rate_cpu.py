"""The store pacer's rate rules (csrc/flat_pace.h: PaceRate, pace_rate_for, pace_judge, pace_rate_reset), deterministically.

On the GPU the rules are only met through the memory system's real behaviour (test_store_pacer_* in test_flat_gpu.py).
Here tests/pace_rate_main.cpp -- plain C++17 that includes nothing of the library but that header -- is compiled with
the host compiler, fed scripted launches and asked for the state.  A launch is `slow` (1.2 x the time its target
explains; a strike is > 1.06 x) or `clean` (exactly that time), recorded at the current target unless `stale`.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-accelerated-point-cloud-registration-using-hierarchical-gmm_amd", "csrc")
START, FLOOR, NEVER = 6600.0, 5800.0, 1e30
REL = 1e-12


@pytest.fixture(scope="module")
def pacer(tmp_path_factory):
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", rocm_clang) if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("pace") / "pace_rate")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "pace_rate_main.cpp"),
                    "-o", exe], check=True)

    def run(script):
        """the states at the script's `dump`s, one dict each"""
        out = subprocess.run([exe] + script.split(), check=True, capture_output=True, text=True).stdout
        return [{k: float(v) for k, v in (kv.split("=") for kv in line.split())} for line in out.splitlines()]
    return run


def test_header_needs_no_hip():
    with open(os.path.join(CSRC, "flat_pace.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<algorithm>"]


def test_three_strikes_lower_the_rate(pacer):                                    # (a)
    s, = pacer("start 800 6600 slow 3 dump")
    assert s["target"] == pytest.approx(START * 0.98, rel=REL)
    assert s["steps_down"] == 1 and s["ceiling"] == START and s["strikes"] == 0


def test_a_clean_launch_clears_the_strikes(pacer):                               # (b)
    s, = pacer("start 800 6600 slow 2 clean 1 slow 2 dump")
    assert s["target"] == START and s["steps_down"] == 0 and s["steps_up"] == 0 and s["ceiling"] == NEVER
    assert s["strikes"] == 2 and s["probe_base"] == 0


def test_the_floor_holds(pacer):                                                 # (c)
    states = pacer("start 800 6600 " + "slow 3 dump " * 100)
    targets = [s["target"] for s in states]
    assert all(a >= b >= FLOOR for a, b in zip(targets, targets[1:]))
    assert targets[-1] == FLOOR and targets[5] > FLOOR
    assert states[-1]["steps_down"] == 100


def test_a_probe_that_holds(pacer):                                              # (d)
    before, probing, kept = pacer("start 800 6600 clean 23 dump clean 1 dump clean 3 dump")
    assert before["target"] == START and before["probe_base"] == 0
    assert probing["target"] == pytest.approx(START * 1.02, rel=REL) and probing["probe_base"] == START
    assert probing["steps_up"] == 0
    assert kept["target"] == probing["target"] and kept["probe_base"] == 0 and kept["steps_up"] == 1


def test_a_probe_that_fails_leaves_a_ceiling(pacer):                             # (e)
    failed, later = pacer("start 800 6600 clean 24 slow 1 dump clean 48 dump")
    assert failed["target"] == START and failed["probe_base"] == 0
    assert failed["ceiling"] == pytest.approx(START * 1.02, rel=REL)
    assert failed["probe_after"] == 48 and failed["steps_down"] == 0 and failed["steps_up"] == 0
    # 48 clean launches are the wait, but 6732 is not below 0.995 x the ceiling: no probe
    assert later["target"] == START and later["probe_base"] == 0 and later["clean"] == 48
    assert later["ceiling"] == failed["ceiling"] and later["ceilings_forgotten"] == 0


def test_a_ceiling_is_forgotten(pacer):                                          # (f)
    before, at = pacer("forget 40 start 800 6600 clean 24 slow 1 clean 39 dump clean 1 dump")
    assert before["ceilings_forgotten"] == 0 and before["probe_after"] == 48 and before["target"] == START
    assert at["ceilings_forgotten"] == 1 and at["ceiling"] == NEVER and at["probe_after"] == 24
    # ... and the probe starts on that same launch: 40 clean ones are more than the first waiting time
    assert at["probe_base"] == START and at["target"] == pytest.approx(START * 1.02, rel=REL)


def test_no_probe_above_the_ceiling_rate(pacer):                                 # (g)
    s, = pacer("start 800 7500 clean 24 dump")
    assert s["target"] == 7500.0 and s["probe_base"] == 0 and s["clean"] == 24


@pytest.mark.parametrize("lead", ["slow 2", "clean 24", "clean 24 slow 1 clean 5"])
def test_a_launch_recorded_under_another_target_says_nothing(pacer, lead):       # (h)
    before, after = pacer("start 800 6600 %s dump stale 5 dump" % lead)
    assert before == after


def test_another_row_length_starts_over(pacer):                                  # (i)
    lowered, same_j, other_j = pacer("start 800 6600 slow 4 dump start 800 6600 dump start 100 6600 dump")
    assert lowered["target"] == pytest.approx(START * 0.98, rel=REL) and lowered["strikes"] == 1
    assert same_j == lowered
    assert other_j["target"] == START and other_j["J"] == 100 and other_j["ceiling"] == NEVER
    assert other_j["strikes"] == 0 and other_j["clean"] == 0 and other_j["probe_after"] == 24
    assert other_j["steps_down"] == 1                       # (the counters are hgmm_pace_info's: only a reset clears them)


def test_reset(pacer):
    cleared, fresh = pacer("start 800 6600 slow 3 clean 30 reset dump start 800 6600 dump")
    assert cleared["target"] == 0 and cleared["steps_down"] == 0 and cleared["steps_up"] == 0
    assert cleared["ceilings_forgotten"] == 0
    assert fresh["target"] == START and fresh["ceiling"] == NEVER and fresh["probe_base"] == 0 and fresh["clean"] == 0
