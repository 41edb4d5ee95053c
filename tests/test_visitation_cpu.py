"""The visitation harvest without a GPU: the boundary (header, binding and library agree on ctf_visitation_words /
ctf_harvest_visitation / ctf_export_visitation) and the host side of ``harvest.EpisodeHarvest(..., visitation=True)`` over a host
stand-in for ``vec``: the table it owns, the two launches ``update()`` issues, ``visitation(g, table)`` of a hand-written table,
``zero()`` — and that the default, ``visitation=False``, makes no such call and adds no key."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

from _cases import abi  # noqa: E402

harvest_mod = importlib.import_module("marl-ctf-development_amd.harvest")
NEW = ("ctf_visitation_words", "ctf_harvest_visitation", "ctf_export_visitation")


def test_header_binding_and_library_agree_on_the_visitation_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctf_env.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ctf_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    raw = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert name in declared, f"include/ctf_env.h does not declare {name}"
        assert name in abi.SYMBOLS, f"_abi.SYMBOLS lacks {name}"
        assert hasattr(raw, name), f"libctf_hip.so does not export {name}"
    assert re.search(r"int32_t\s+ctf_visitation_words\s*\(\s*const\s+ctf_env\s*\*", text)
    assert abi.SYMBOLS["ctf_harvest_visitation"] == abi.SYMBOLS["ctf_harvest_episodes"]  # (the same arguments: the same envs)
    assert len(abi.SYMBOLS["ctf_export_visitation"][1]) == 5
    assert abi.ABI_VERSION == 2 and int(re.search(r"#define\s+CTF_ABI_VERSION\s+(\d+)", text).group(1)) == 2  # (no struct changed)
    assert abi.load_library().ctf_visitation_words(None) == 0  # (a null handle has no maps)


class _Vec:
    """what EpisodeHarvest needs of a VecGridworldCtf, on the host"""

    def __init__(self, n_agents=4, grid=5, n_envs=4):
        self.N_AGENTS, self.GRID_SIZE = n_agents, grid
        self.AGENT_TEAMS, self.AGENT_TYPES = {i: i % 2 for i in range(n_agents)}, {i: 0 for i in range(n_agents)}
        self.n_envs, self.device = n_envs, "cpu"
        self.harvest_words = 8 + abi.N_METRICS * n_agents
        self.visitation_words = n_agents * grid * grid
        self.calls = []

    def harvest(self, acc, groups=None, mask=None, all_envs=False):
        self.calls.append(("harvest", acc, groups, mask, all_envs))

    def harvest_visitation(self, acc, groups=None, mask=None, all_envs=False):
        self.calls.append(("harvest_visitation", acc, groups, mask, all_envs))


def test_a_visitation_harvest_owns_a_table_and_issues_both_launches_with_the_same_arguments():
    torch = pytest.importorskip("torch")
    vec = _Vec()
    h = harvest_mod.EpisodeHarvest(vec, n_groups=3, groups=np.array([0, 2, 1, 0]), visitation=True)
    assert tuple(h.vis_acc.shape) == (3, 4, 5, 5) and h.vis_acc.dtype == torch.int64 and h.vis_acc.is_contiguous()
    assert not bool(h.vis_acc.any())
    mask = torch.ones(4, dtype=torch.uint8)
    h.update(mask=mask, all_envs=True)
    h.update()
    assert [c[0] for c in vec.calls] == ["harvest", "harvest_visitation"] * 2
    assert vec.calls[0][1] is h.acc and vec.calls[1][1] is h.vis_acc
    for a, b in ((vec.calls[0], vec.calls[1]), (vec.calls[2], vec.calls[3])):
        assert a[2] is b[2] is h.groups and a[3] is b[3] and a[4] is b[4]
    assert vec.calls[1][3] is mask and vec.calls[1][4] is True and vec.calls[3][3] is None and vec.calls[3][4] is False

    table = np.zeros((3, 4, 5, 5), np.int64)
    table[1, 0, 2, 3] = 700      # (past a u8: nothing wraps)
    table[1, 3, 4, 4] = 5
    table[2, 1] = np.arange(25).reshape(5, 5)
    got = h.visitation(1, table)
    assert sorted(got) == [0, 1, 2, 3] and all(v.shape == (5, 5) and v.dtype == np.int64 for v in got.values())
    assert got[0][2, 3] == 700 and got[3][4, 4] == 5 and sum(int(v.sum()) for v in got.values()) == 705
    assert np.array_equal(h.visitation(2, table)[1], np.arange(25).reshape(5, 5)) and not any(v.any() for v in h.visitation(0, table).values())
    m = h.metrics(1, np.zeros((3, h.H), np.int64))
    m["agent_visitation_maps"] = h.visitation(1, table)  # (the docstring's use)
    assert m["agent_visitation_maps"][0][2, 3] == 700

    h.acc.fill_(3)
    h.vis_acc.copy_(torch.from_numpy(table))
    assert np.array_equal(h.visitation_table(), table) and h.visitation(1)[0][2, 3] == 700
    h.zero()
    assert not h.table().any() and not h.visitation_table().any()


def test_without_the_flag_nothing_changes():
    pytest.importorskip("torch")
    vec = _Vec()
    h = harvest_mod.EpisodeHarvest(vec, n_groups=2, groups=np.array([0, 1, 1, 0]))
    assert h.vis_acc is None
    h.update(all_envs=True)
    h.update()
    h.zero()
    assert [c[0] for c in vec.calls] == ["harvest", "harvest"]
    assert "agent_visitation_maps" not in h.metrics(0, np.zeros((2, h.H), np.int64))
    with pytest.raises(ValueError):
        h.visitation(0)
