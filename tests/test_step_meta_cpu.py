"""The metadata rows k_step writes (marl-ctf-development_amd/csrc/ctf_meta.h), without a GPU.

``test_rows_are_the_oracles``: the header is compiled for the host into a stand-alone program with the C oracle, under
AddressSanitizer + UBSan (tests/hostsim/meta_main.cpp), and run over every ``meta_cases`` row of tests/_obs_cases.py and over random
play on the 29 agent-count configurations of tests/_agent_counts.py: the rows made the step kernels' way (the flat passes of
step_block at W = 1, 64 envs per wave, ragged blocks, guard bands) and the renders' way must be the oracle's bit for bit; f64_to_f16
is run over every binary16 value, every tie and the doubles beside it, the exact integer path over 0 .. 255 and the uint8 wrap.

The other tests are the gate of tests/test_gpu_step_meta.py, on the oracle alone: the states that test plants are stepped before
anything is compared, and AFTER the step (tests/_step_meta_cases.py) they must still reach every class of the conversion through the
step fraction and through the capture ratio, zero through the integer elements, and every hp and flag pattern.

A unit test of rules the device code shares, not a CPU path of the product."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

import _agent_counts
import _obs_cases as oc
import _step_meta_cases as smc
from _cases import abi
from _rule_cases import to_view
from test_obs_cases_cpu import metadata_order

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostsim", "meta_main.cpp")
ONE = 0x3C00


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
    out = tmp_path_factory.mktemp("step_meta")
    cc, cxx = _compilers()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    obj = str(out / "ctf_oracle.o")
    subprocess.check_call([cc, "-std=c11", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-source-uses-openmp", *san, "-c",
                           os.path.join(ROOT, "oracle", "ctf_oracle.c"), "-o", obj])
    exe = str(out / "meta_main")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-fno-strict-aliasing", *san, SRC, obj, "-lm", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    """per config: the ctf_config, a count, that many ctf_state_view structs (none: the program plays the config itself)"""
    path = tmp_path_factory.mktemp("step_meta_cases") / "cases.bin"
    with open(path, "wb") as f:
        for name in oc.MAP_NAMES:
            cases = oc.meta_cases(name)
            f.write(bytes(oc.config(name)))
            f.write(np.int32(len(cases)).tobytes())
            for c in cases:
                f.write(bytes(to_view(c.state)))
        for n, lop in _agent_counts.CONFIGS:
            f.write(bytes(_agent_counts.build(n, lop)))
            f.write(np.int32(0).tobytes())
    assert C.sizeof(abi.CtfStateView) > 0 and len(_agent_counts.CONFIGS) == 29
    return str(path)


def test_rows_are_the_oracles(program, cases_file):
    out = subprocess.run([program, cases_file], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + "\n" + out.stderr[-3000:]
    assert "ok conversions" in out.stdout
    assert out.stdout.count("ok config") == len(oc.MAP_NAMES) + 29 and out.stdout.count("(played)") == 29
    assert "all step-meta cases passed" in out.stdout


# ---- the gate of the GPU test: the table AFTER the step, on the oracle alone ----------------------------------------------------------------
def test_after_the_step_every_conversion_class_is_still_reached():
    seen = {0: set(), 1: set()}
    zero_by_integer = False
    for name in oc.MAP_NAMES:
        after, meta = smc.stepped(name)
        tm = oc.teams(name)
        assert len(after) == len(oc.meta_cases(name)) == meta.shape[0]
        for k, s in enumerate(after):
            a, b = s["team_captures"]
            for element, team, q in ((0, None, F(s["step_count"], oc.game_steps(name))), (1, 0, F(a + 1, b + 1)), (1, 1, F(b + 1, a + 1))):
                bits, cls = oc.half_of(q)
                seen[element].add(cls)
                for i in range(len(tm)):
                    if team in (None, tm[i]):
                        assert int(meta[k, i, element]) == bits, (name, k, element, i, cls)
        zero_by_integer |= bool((meta[:, :, 6:] == 0).any())
    # a step count is at least 1 after a step and a ratio of two positive counts is not zero: the general conversion meets zero only
    # as an underflow there; the hp and flag elements, which take the integer path, show it
    assert seen[0] == set(oc.CLASSES) - {"zero"}, set(oc.CLASSES) - seen[0]
    assert seen[1] == set(oc.CLASSES) - {"zero"}, set(oc.CLASSES) - seen[1]
    assert zero_by_integer


@pytest.mark.parametrize("name", oc.MAP_NAMES)
def test_after_the_step_every_flag_element_shows_one_agent(name):
    _, meta = smc.stepped(name)
    n, nb = oc.shape(name)[0], oc.flag_case_count(name)
    rows = [meta[[c.name for c in oc.meta_cases(name)].index(f"flag-{k}")] for k in range(nb)]
    for viewer in range(n):
        for slot, agent in enumerate(metadata_order(name, viewer)):
            seq = [int(rows[k][viewer, 7 + 2 * slot]) for k in range(nb)]
            assert set(seq) <= {0, ONE} and seq[-1] == ONE
            assert sum((seq[k] == ONE) << k for k in range(nb - 1)) == agent, (viewer, slot)


@pytest.mark.parametrize("name", oc.MAP_NAMES)
def test_after_the_step_every_hp_element_shows_one_agent_and_its_divisor(name):
    after, meta = smc.stepped(name)
    n = oc.shape(name)[0]
    ty, full = oc.types(name), oc.type_hp(name)
    at = [[c.name for c in oc.meta_cases(name)].index(f"hp-{r}") for r in range(4)]
    rows = [meta[k] for k in at]
    hp = [after[k]["hp"] for k in at]  # after the step: where the map heals, the quotients below 1 have moved
    divisors = sorted({full[t] for t in ty})
    shown = lambda v, d: [oc.half_of(math.floor(F(float(hp[r][v])) / F(d)) % 256)[0] for r in range(4)]
    candidates = {(v, d): shown(v, d) for v in range(4) for d in divisors}
    assert len({tuple(s) for s in candidates.values()}) == len(candidates)  # no two (source agent, divisor) look alike
    for viewer in range(n):
        for slot, agent in enumerate(metadata_order(name, viewer)):
            seq = [int(rows[r][viewer, 6 + 2 * slot]) for r in range(4)]
            assert [k for k, s in candidates.items() if s == seq] == [(ty[agent], full[ty[agent]])], (viewer, slot, seq)
    values = {int(x) for r in rows for x in r[:, 6::2].reshape(-1)}
    assert oc.half_of(255)[0] in values
    if name == "term16":  # all four types at one full hp each agent's own: the elements show the planted quotients themselves
        assert {oc.half_of(v)[0] for v in (0, 1, 2, 37, 200, 255)} <= values
