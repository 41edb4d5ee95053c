"""CPU-side checks of the boundary: the HIP library loads without a GPU, exports every symbol that
include/*.h declare, and the ctypes mirror matches the compiled struct layouts.  No compute calls."""
import ctypes
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
abi = importlib.import_module("marl-ctf-development_amd._abi")


def declared_symbols():
    names = set()
    for header in ("ctf_env.h", "ctf_policy.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names |= set(re.findall(r"\b(ctf_[a-z0-9_]+)\s*\(", text))
    return sorted(names)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return abi.load_library()


def test_header_and_binding_name_the_same_entry_points():
    assert declared_symbols() == sorted(abi.SYMBOLS)


def test_library_exports_every_declared_symbol(lib):
    raw = ctypes.CDLL(abi.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(raw, name), f"libctf_hip.so does not export {name}"


def test_struct_mirrors_match_compiled_layout(lib):
    assert lib.ctf_abi_version() == abi.ABI_VERSION
    assert lib.ctf_sizeof_config() == ctypes.sizeof(abi.CtfConfig)
    assert lib.ctf_sizeof_state_view() == ctypes.sizeof(abi.CtfStateView)


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(abi.CtfLibraryError):
        abi.load_library(str(tmp_path / "nope.so"))


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "marl-ctf-development_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), f
                assert "ctf_oracle" not in src, f


def test_only_tests_smoke_and_the_cpu_baseline_leg_touch_the_oracle():
    """oracle/ is test infrastructure: outside tests/ only __graft_entry__.smoke() and bench.py's cpu_baseline may use it."""
    allowed = {os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")}
    for dirpath, dirnames, files in os.walk(ROOT):
        dirnames[:] = [d for d in dirnames if d not in (".git", "gpurun_out", "tests", "oracle", "__pycache__", ".pytest_cache")]
        for f in files:
            path = os.path.join(dirpath, f)
            if f.endswith((".py", ".sh", ".hip", ".h", ".cpp", ".c")) and path not in allowed:
                src = open(path, errors="replace").read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M) and "ctf_oracle" not in src, path


# -- the package's one call layer (_abi.call / ptr): a stand-in library object, no device -------------------------------------------
class _StandInLib:
    def __init__(self, rc, policy_error=b"why", env_error=b"why"):
        self.rc, self.seen = rc, []
        self.ctf_policy_last_error = lambda: policy_error
        self.ctf_last_error = lambda: env_error

    def _entry(self, *args):
        self.seen.append(args)
        return self.rc

    ctf_policy_x = ctf_rollout_x = ctf_x = _entry


def test_call_raises_the_policy_headers_error_text_for_policy_and_rollout_names():
    for name in ("ctf_policy_x", "ctf_rollout_x"):  # include/ctf_policy.h declares both families; one error getter
        with pytest.raises(abi.CtfLibraryError) as e:
            abi.call(_StandInLib(3, env_error=b"not this one"), name, 1)
        assert str(e.value) == name + ": why"
    with pytest.raises(abi.CtfLibraryError) as e:
        abi.call(_StandInLib(3, policy_error=None), "ctf_policy_x")
    assert str(e.value) == "ctf_policy_x: "


def test_call_raises_check_s_text_for_an_env_name():
    with pytest.raises(abi.CtfLibraryError) as e:
        abi.call(_StandInLib(3, policy_error=b"not this one"), "ctf_x", 1)
    assert str(e.value) == "ctf call failed (3): why"
    with pytest.raises(abi.CtfLibraryError) as e:
        abi.call(_StandInLib(-1, env_error=None), "ctf_x")
    assert str(e.value) == "ctf call failed (-1): "


def test_call_passes_the_arguments_through_unchanged_and_in_order():
    lib, marker = _StandInLib(0), object()
    assert abi.call(lib, "ctf_policy_x", 1, None, marker, 2.5) is None
    assert abi.call(lib, "ctf_x", marker) is None
    assert lib.seen == [(1, None, marker, 2.5), (marker,)] and lib.seen[0][2] is marker
    with pytest.raises(AttributeError):  # a name the library does not have is the caller's bug, not a library error
        abi.call(lib, "ctf_policy_nope")


def test_ptr_is_the_tensors_address_and_none_stays_null():
    import torch

    t = torch.zeros(4)
    assert abi.ptr(None) is None
    assert ctypes.c_void_p(abi.ptr(t)).value == t.data_ptr()
    assert ctypes.c_void_p(abi.ptr(t[1:])).value == t.data_ptr() + 4
    # ... in a form a void* argument takes (what bind() gives every pointer argument of SYMBOLS)
    echo = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)(lambda p: p)
    assert echo(abi.ptr(t)) == t.data_ptr() and echo(abi.ptr(None)) is None
