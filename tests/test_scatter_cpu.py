"""The scattered reset without a GPU: the boundary (header, binding and library agree on ctf_reset_scattered), the properties of the
plain restatement tests/_scatter_ref.py, the rule as csrc/ctf_scatter.h states it — compiled for the host into a stand-alone program
under AddressSanitizer + UBSan (tests/scatter/scatter_main.cpp; nothing is loaded into Python) and held to the restatement cell for
cell on every config and argument combination of tests/_scatter_cases.py — and ScatteredStarts / collect(starts=...) on a stub vec."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import _scatter_cases as scs  # noqa: E402
import _scatter_ref as sr  # noqa: E402
from _cases import abi, pkg  # noqa: E402


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    raw_text = open(os.path.join(ROOT, "include", "ctf_env.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw_text, flags=re.S)
    assert re.search(r"int\s+ctf_reset_scattered\s*\(\s*ctf_env\s*\*[^,]*,\s*const\s+uint8_t\s*\*[^,]*,\s*uint32_t[^,]*,\s*int32_t[^,]*,\s*uint32_t[^,]*,"
                     r"\s*uint64_t[^,]*,\s*uint32_t[^,]*,\s*uint32_t\s*\*[^,]*,\s*uint32_t[^,]*,\s*void\s*\*", text)
    assert int(re.search(r"#define\s+CTF_SCATTER_OWN_SIDE\s+(\d+)u", text).group(1)) == 1 == abi.SCATTER_OWN_SIDE == sr.OWN_SIDE
    header = open(os.path.join(ROOT, "marl-ctf-development_amd", "csrc", "ctf_scatter.h")).read()
    assert int(re.search(r"#define\s+CTF_SCATTER_TAG\s+0x([0-9A-Fa-f]+)u", header).group(1), 16) == 0x53435431 == abi.SCATTER_TAG == sr.SCATTER_TAG
    assert bytes.fromhex("53435431") == b"SCT1"
    assert header.count("philox4x32_10(") == 1 and "ctf_mt.h" in header  # the existing generator is called, not copied
    restype, argtypes = abi.SYMBOLS["ctf_reset_scattered"]
    assert restype is ctypes.c_int and [ctypes.sizeof(t) for t in argtypes] == [8, 8, 4, 4, 4, 8, 4, 8, 4, 8]
    capturable = raw_text[:raw_text.index("#ifndef CTF_ENV_H")]  # the list of capturable calls
    assert "ctf_reset_scattered" in capturable
    assert abi.ABI_VERSION == 2 and int(re.search(r"#define\s+CTF_ABI_VERSION\s+(\d+)", text).group(1)) == 2  # added symbols, no more
    assert "the reference has no such reset" in " ".join(raw_text.split())  # what the call is not, in so many words
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = abi.load_library()
    assert hasattr(ctypes.CDLL(abi.LIB_PATH), "ctf_reset_scattered")
    assert lib.ctf_reset_scattered(None, None, 0, 0, 0, 0, 0, None, 0, None) == -1  # a null handle is refused before anything is launched
    assert pkg.ScatteredStarts is pkg.starts.ScatteredStarts


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
ENVS = np.arange(67, dtype=np.uint64) + scs.ENV_OFFSET  # the GPU test's largest batch, at its env offset: global indices that wrap


def test_arena_candidate_counts():
    rules = sr.cfg_rules(scs.configs()["arena"][1])
    assert (rules["n"], rules["g"]) == (8, 15) and int((rules["init"] == 0).sum()) == 178
    for radius, counts in scs.ARENA_COUNTS.items():
        assert [len(sr.candidates(rules, i, radius, False)) for i in range(8)] == counts
    for radius in (14, 15, 1 << 30):  # any radius >= G - 1 is the whole grid
        assert {len(sr.candidates(rules, i, radius, False)) for i in range(8)} == {scs.ARENA_WHOLE}
        assert {len(sr.candidates(rules, i, radius, True)) for i in range(8)} == {scs.ARENA_WHOLE_OWN_SIDE}
    assert all(sr.candidates(rules, i, 0, own) == [rules["starts"][i][0] * 15 + rules["starts"][i][1]] for i in range(8) for own in (False, True))


@pytest.mark.parametrize("name", scs.config_names())
def test_restatement_properties(name):
    cfg = scs.configs()[name][1]
    rules = sr.cfg_rules(cfg)
    n, g = rules["n"], rules["g"]
    starts = [r * g + c for r, c in rules["starts"]]
    assert all(rules["init"][s] != 0 for s in rules["starts"]) and len(set(starts)) == n  # a start cell holds its agent's tile: never OPEN
    for k, (radius, own_side, mask, seed, rnd, ep) in enumerate(scs.combos(cfg)):
        cells = sr.place(rules, mask, radius, own_side, seed, ENVS, rnd + ep)
        assert cells.shape == (67, n)
        for e in (0, 1, 2, 66) if k % 4 == 0 else (k % 67,):  # the batch form is the plain rule
            assert cells[e].tolist() == sr.place_one(rules, mask, radius, own_side, seed, int(ENVS[e]) & sr.U32, (rnd + ep) & sr.U32), (k, e)
        assert all(len(set(row)) == n for row in cells.tolist())  # agents never share a cell
        for i in range(n):
            col = cells[:, i]
            rr, cc = col // g, col % g
            at_start = col == starts[i]
            if not (mask >> i) & 1 or radius == 0:
                assert at_start.all()
                continue
            assert (at_start | (rules["init"][rr, cc] == 0)).all()
            sr_, sc_ = rules["starts"][i]
            assert (np.maximum(abs(rr - sr_), abs(cc - sc_)) <= radius).all()
            if own_side:
                (hr, hc), (or_, oc) = rules["flags"][rules["teams"][i]], rules["flags"][1 - rules["teams"][i]]
                own = np.maximum(abs(rr - hr), abs(cc - hc)) <= np.maximum(abs(rr - or_), abs(cc - oc))
                assert (at_start | own).all()
        if radius == 0 or mask == 0:
            grid, pos = sr.state(rules, cells[0])
            assert np.array_equal(grid, rules["init"]) and pos.tolist() == [list(s) for s in rules["starts"]]


def test_uniformity_on_the_arena():
    """4 096 envs at radius G: agent 0 reaches all 179 of its candidates.  A cell is missed with probability (178 / 179)^4096 = 1.1e-10
    and one of 179 with less than 2e-8 < 1e-7: a condition, not a statistic"""
    rules = sr.cfg_rules(scs.configs()["arena"][1])
    cells = sr.place(rules, 0xFF, 15, False, 0xC0FFEE, np.arange(4096), 0)
    assert sorted(set(cells[:, 0].tolist())) == sr.candidates(rules, 0, 15, False) and len(set(cells[:, 0].tolist())) == 179
    assert 179 * (178 / 179) ** 4096 < 1e-7
    counts = np.bincount(cells[:, 0], minlength=225)
    assert counts.max() < 60  # mean 22.9, sigma 4.8: nothing piles up
    # the episode counter redraws: the same env, the next round, elsewhere — for all but the few that draw the same cell twice
    again = sr.place(rules, 0xFF, 15, False, 0xC0FFEE, np.arange(4096), 1)
    assert (again[:, 0] != cells[:, 0]).mean() > 0.98


# ---- the host program ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """-> run(cases): cases are (cfg, log_metrics, agent_mask, radius, flags, seed, env, r) -> per case a dict of what the env holds"""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = "clang++"
    build = tmp_path_factory.mktemp("scatter")
    exe = str(build / "scatter_main")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "marl-ctf-development_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "scatter", "scatter_main.cpp")])
    count = [0]

    def run(cases):
        lines = [str(len(cases))]
        for cfg, log_metrics, mask, radius, flags, seed, env, r in cases:
            n, g = cfg.n_agents, cfg.grid_size
            team_mask = sum(int(cfg.agent_team[i]) << i for i in range(n))
            type_pack = sum(int(cfg.agent_type[i]) << (2 * i) for i in range(n))
            flag_pack = sum((int(cfg.flag_pos[t][0]) | int(cfg.flag_pos[t][1]) << 8) << (16 * t) for t in range(2))
            lines.append(f"{n} {g} {team_mask} {type_pack} {flag_pack} {int(log_metrics)} {mask} {radius} {flags} {seed} {env} {r}")
            lines.append(" ".join(float(cfg.type_hp[t]).hex() for t in range(4)))
            lines.append(" ".join(f"{int(cfg.start_pos[i][0])} {int(cfg.start_pos[i][1])}" for i in range(n)))
            lines.append(" ".join(str(int(v)) for v in cfg.init_grid[:g * g]))
        path = build / f"cases_{count[0]}.txt"
        count[0] += 1
        path.write_text("\n".join(lines) + "\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + "\n" + out.stderr[-3000:]
        rows = out.stdout.strip().split("\n")
        assert rows[-1] == f"done {len(cases)}"
        got = []
        for (cfg, *_), row in zip(cases, rows[:-1]):
            v, n, gg = [int(x) for x in row.split()], cfg.n_agents, cfg.grid_size ** 2
            assert len(v) == 9 * n + gg + 5
            cut = np.cumsum([n, gg, 2 * n, n, n, n, n, 4, 1])
            parts = [v[a:b] for a, b in zip([0] + cut.tolist(), cut.tolist() + [len(v)])]
            got.append(dict(zip(("cells", "grid", "pos", "has_flag", "inv", "perm", "hp", "misc", "metrics", "vis"), parts)))
        return got

    return run


@pytest.mark.parametrize("group", ["named", "counts"])
def test_program_against_the_restatement(program, group):
    names = [n for n in scs.config_names() if n.startswith("count-") == (group == "counts")]
    cases, want = [], []
    for name in names:
        cfg = scs.configs()[name][1]
        rules = sr.cfg_rules(cfg)
        for k, (radius, own_side, mask, seed, rnd, ep) in enumerate(scs.combos(cfg)):
            r = (rnd + ep) & sr.U32
            cells = sr.place(rules, mask, radius, own_side, seed, ENVS, r)
            for e in (0, 1, 2, 66):
                cases.append((cfg, k % 5 != 4, mask, radius, sr.OWN_SIDE if own_side else 0, seed, int(ENVS[e]) & sr.U32, r))
                want.append((name, rules, cells[e]))
            if radius == cfg.grid_size:  # any radius >= G - 1 is the whole grid, up to the largest int32
                for big in (cfg.grid_size - 1, 0x7FFFFFFF):
                    cases.append((cfg, True, mask, big, sr.OWN_SIDE if own_side else 0, seed, int(ENVS[0]) & sr.U32, r))
                    want.append((name, rules, cells[0]))
    got = program(cases)
    moved_any = 0
    for case, out, (name, rules, cells) in zip(cases, got, want):
        cfg, log_metrics = case[0], case[1]
        n, g = rules["n"], rules["g"]
        what = (name,) + case[1:]
        grid, pos = sr.state(rules, cells)
        assert out["cells"] == cells.tolist(), what
        assert out["grid"] == grid.reshape(-1).tolist() and out["pos"] == pos.reshape(-1).tolist(), what
        assert out["has_flag"] == [0] * n and out["inv"] == [0] * n and out["perm"] == [0xAB] * n, what  # perm is kept
        assert out["hp"] == [struct.unpack("<Q", struct.pack("<d", float(cfg.type_hp[cfg.agent_type[i]])))[0] for i in range(n)], what
        moved = cells.tolist() != [r * g + c for r, c in rules["starts"]]
        moved_any += moved
        assert out["misc"] == [0, 0, 0, 0 if moved else 2], what  # CTF_F_BASE_ZERO unless somebody moved
        gs = (g * g + 15) // 16 * 16
        assert out["metrics"] == [0 if log_metrics else 5 * abi.N_METRICS * n], what
        if log_metrics and moved:  # the maps written out: a single 1 per agent, at its cell
            assert out["vis"] == [x for c in cells.tolist() for x in (1, c)], what
        else:
            assert out["vis"] == [7 * gs, 0] * n, what
    assert moved_any > len(cases) // 2


# ---- ScatteredStarts and collect(starts=...) on a stub vec ------------------------------------------------------------------------------
class _Vec:
    """two agents on a 3 x 3 grid, on the CPU: what BatchedRolloutCollector touches of a VecGridworldCtf, with the calls recorded"""

    def __init__(self, n_envs=4):
        import torch

        self.torch, self.n_envs, self.device = torch, n_envs, torch.device("cpu")
        self.N_AGENTS, self.GRID_SIZE, self.N_CHANNELS, self.META_LEN = 2, 3, 2, 10
        self.AGENT_TEAMS, self.AGENT_TYPES, self.derived = [0, 1], [0, 0], dict(flip_axis=None)
        self.calls, self.t = [], 0

    def reset(self, mask=None):
        self.calls.append(("reset", mask))

    def reset_scattered(self, **kw):
        self.calls.append(("reset_scattered", kw))
        ep = kw["episodes"]  # what the kernel does for the masked envs (here: all); torch adds no uint32 on the CPU
        ep.copy_((ep.to(self.torch.int64) + 1).to(self.torch.uint32))

    def step(self, actions):
        self.t += 1
        return self.torch.full((self.n_envs, 2), float(self.t)), self.torch.zeros(self.n_envs, dtype=self.torch.uint8)

    def observe(self):
        torch = self.torch
        obs = torch.zeros((self.n_envs, 2, 2, 3, 3), dtype=torch.uint8)
        obs[:, :, 0, self.t % 3, 0] = 1
        return obs, torch.zeros((self.n_envs, 2, 10), dtype=torch.float16)


def test_scattered_starts_and_the_collector_on_a_stub_vec():
    torch = pytest.importorskip("torch")
    from _stub_policy import StubPolicy

    vec = _Vec()
    starts = pkg.ScatteredStarts(2, own_side=True, team=1, seed=7)
    col = pkg.BatchedRolloutCollector(vec, 3, 0)
    for k in range(3):
        col.collect(StubPolicy(1), StubPolicy(2), starts=starts)
    assert [c[0] for c in vec.calls] == ["reset_scattered"] * 3  # once per collect, and no plain reset beside it
    kws = [c[1] for c in vec.calls]
    assert all(kw["episodes"] is kws[0]["episodes"] for kw in kws)  # one counter tensor per vec, reused
    ep = kws[0]["episodes"]
    assert ep.dtype == torch.uint32 and ep.shape == (4,) and ep.tolist() == [3] * 4 and starts.episodes(vec) is ep
    assert {k: v for k, v in kws[0].items() if k != "episodes"} == dict(mask=None, radius=2, agent_mask=None, team=1, own_side=True, seed=7, round=0,
                                                                        env_offset=0)
    other = _Vec(5)
    starts.reset(other, mask="m")
    assert other.calls[0][1]["mask"] == "m" and other.calls[0][1]["episodes"].shape == (5,) and starts.episodes(vec) is ep
    # starts=None: vec.reset() as before
    plain = _Vec()
    pkg.BatchedRolloutCollector(plain, 3, 0).collect(StubPolicy(1), StubPolicy(2))
    assert plain.calls == [("reset", None)]
    with pytest.raises(ValueError):
        col.collect(StubPolicy(1), StubPolicy(2), reset=False, starts=starts)
    with pytest.raises(ValueError):
        pkg.ScatteredStarts(-1)
    with pytest.raises(ValueError):
        pkg.ScatteredStarts(1, agent_mask=1, team=0)
