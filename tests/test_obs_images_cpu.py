"""The rules round 13 added to the retained observation render, without a GPU: the slot images carried forward from the cells that
changed (obsc_update_cell, marl-ctf-development_amd/csrc/ctf_obs_chunk.h), the dirty lines marked per (changed cell, viewer) pair
(obsd_pair_changed, ctf_obs_delta.h) and the mask compacted 64 lines per pass (obsd_rank) are compiled for the host into a
stand-alone program together with the C oracle, under AddressSanitizer + UBSan, and run over the golden cases' configurations and
random 2..16-agent ones, each under all four FLIP_AXIS values and five reverse masks: 50 steps of random actions with resets, and
after every step the carried images must be the images of the new grid dword for dword, every chunk from them the oracle's render,
and the pairs' marks the cell rule's (tests/obs_images/obs_images_main.cpp).

A unit test of rules the device code shares, not a CPU path of the product."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import _agent_counts
from _cases import Case, case_names

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "obs_images", "obs_images_main.cpp")
RANDOM_CONFIGS = [(2, 0), (3, 1), (5, 0), (7, 1), (8, 0), (11, 1), (13, 0), (16, 0), (16, 1)]  # (agents, lopsided teams)


def _compilers():
    llvm = "/opt/rocm/lib/llvm/bin"
    cc, cxx = os.path.join(llvm, "clang"), os.path.join(llvm, "clang++")
    if os.path.exists(cc) and os.path.exists(cxx):
        return cc, cxx
    cc, cxx = shutil.which("cc"), shutil.which("c++")
    if not (cc and cxx):
        pytest.fail("no C / C++ compiler on this machine")
    return cc, cxx


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("obs_images")
    cc, cxx = _compilers()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    obj = str(out / "ctf_oracle.o")
    subprocess.check_call([cc, "-std=c11", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", *san, "-c",
                           os.path.join(ROOT, "oracle", "ctf_oracle.c"), "-o", obj])
    exe = str(out / "obs_images_main")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", *san, SRC, obj, "-lm", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def configs(tmp_path_factory):
    """the ctf_config structs the program reads: every golden case's, then the random ones'"""
    path = tmp_path_factory.mktemp("obs_images_cfg") / "configs.bin"
    names = [n for n in case_names() if not n.startswith("fuzz")]  # the 19 distinct configurations (the fuzz cases replay arena / split ones)
    with open(path, "wb") as f:
        for name in names:
            f.write(bytes(Case(name).config()[0]))
        for n, lop in RANDOM_CONFIGS:
            f.write(bytes(_agent_counts.build(n, lop)))
    assert os.path.getsize(path) == (len(names) + len(RANDOM_CONFIGS)) * C.sizeof(_agent_counts.abi.CtfConfig)
    return str(path), len(names)


def test_carried_images_pair_marks_and_compaction(program, configs):
    path, n_golden = configs
    assert n_golden == 19
    out = subprocess.run([program, path, "50"], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)  # per config: changed cells, image bits moved, lines marked
    assert out.returncode == 0, out.stdout[-3000:] + "\n" + out.stderr[-3000:]
    assert "ok compaction" in out.stdout
    assert out.stdout.count("ok config") == n_golden + len(RANDOM_CONFIGS)
    assert "all obs-images cases passed" in out.stdout
