"""docs/SWITCHES.md is generated from the switch table of the native library (csrc/fg_switches.h) and the os.environ sites of the
Python source (profiles/gen_switch_table.py); this test fails when a switch was added or removed without regenerating it, holds the
table's defaults and parse rules to what fg_create / fg_mb_create read before the table existed (fg_switch_values needs no device),
and checks that the library reports the switches of a handle (fg_mb_config_dump works on a host-only handle; fg_config_dump needs a
GPU: tests/test_gpu_switch_per_handle.py)."""
import ctypes
import glob
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_table_is_current():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "gen_switch_table.py"), "--check"], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, "docs/SWITCHES.md is stale: run python profiles/gen_switch_table.py\n" + out.stdout + out.stderr


def test_multi_block_handle_reports_its_switches(monkeypatch):
    from fluidgym_amd import _lib as L

    monkeypatch.setenv("FG_MB_COMPACT", "0")
    lib = L.load()
    h = ctypes.c_void_p()
    assert lib.fg_mb_create(2, 1, -1, ctypes.byref(h)) == 0
    try:
        small = ctypes.create_string_buffer(8)
        need = lib.fg_mb_config_dump(h, small, 8)
        assert need > 8                                  # too small: the length needed comes back
        buf = ctypes.create_string_buffer(need)
        assert lib.fg_mb_config_dump(h, buf, need) == 0
        cfg = json.loads(buf.value.decode())
        assert cfg["FG_MB_COMPACT"] == 0 and cfg["FG_MB_BICG_FUSE"] == 2 and cfg["FG_MB_ONCHIP"] == 1
    finally:
        lib.fg_mb_destroy(h)


# what fg_create / fg_mb_create gave with no FG_* variable set, before the table existed (written out from that code, not from the table)
DEFAULTS = [
    {"FG_POLL_SPIN": 1, "FG_POLL_WORDS": 1, "FG_ADV_JACOBI": 0, "FG_CG_FUSED": 1, "FG_BICG_PFUSED": 1, "FG_BICG_FUSED": 1, "FG_BICG_SUB": -1,
     "FG_BICG3": -1, "FG_BICG3_BXL": 0, "FG_BICG3_MIX": 3, "FG_REDUCE_WGS": 0, "FG_HELM_ROWFORM": 1, "FG_ADV_LINESWEEP": 0, "FG_FD_FACFUSE": 1,
     "FG_FD_ROWMEAN": 1, "FG_FCG_FIRST": 1, "FG_FCG_SPEC": 1, "FG_JAC_SPEC": 1, "FG_JAC_PREFACTOR": 1, "FG_JAC_WARM": -1, "FG_JAC_XCD": 1,
     "FG_JAC_SHAPE": 0, "FG_JAC_SWEEPS": 0, "FG_FORCE_ZMARCH": 0, "FG_ZMARCH_SB": -1, "FG_DEV_DT": 1, "FG_PROF_PERIOD": 64, "FG_HTRACE": 0, "FG_ROCTX": 0},
    {"FG_POLL_SPIN": 1, "FG_POLL_WORDS": 1, "FG_ADV_JACOBI": 0, "FG_MB_BICG_VEC4": 31, "FG_MB_BICG_FUSE": 2, "FG_MB_ML_FUSE": 1, "FG_MB_ML_TRY_CAP": 200,
     "FG_MB_TRACE": 0, "FG_MB_TRACE_FAIL": 0, "FG_MB_COMPACT": 1, "FG_MB_OC_RTG_NT": 1024, "FG_MB_ONCHIP": 1, "FG_MB_OC_AGG": 1, "FG_MB_OC_VARIANT": 0,
     "FG_MB_CLUSTER": 1, "FG_MB_CL_JACOBI": 1, "FG_MB_CL_HALF": 1, "FG_MB_CL_MAXCL": 0, "FG_MB_CL_NEAR": 1, "FG_MB_RUNG_ILU": 1, "FG_MB_PCG_KERNEL": 0,
     "FG_HTRACE": 0, "FG_ROCTX": 0},
]
STALE = ("FG_CG_WGS_PER_SLOT", "FG_TRIDIAG_CB", "FG_HELM_CB", "FG_MB_SCALAR_CG", "FG_MB_PRED", "FG_MB_ML_SB", "FG_MB_ML_WARMUP", "FG_MB_GRAPH")


def _no_switches(monkeypatch):
    for name in list(os.environ):
        if name.startswith("FG_"):
            monkeypatch.delenv(name)


def _values(family):
    from fluidgym_amd import _lib as L

    return L.read_json(L.load().fg_switch_values, family)


@pytest.mark.parametrize("family", [0, 1])
def test_defaults_are_those_of_the_create_calls(family, monkeypatch):
    _no_switches(monkeypatch)
    assert _values(family) == DEFAULTS[family]


# (family, variable, members for "0", "1", "7", "-1") by the rule the variable was read with before the table: plain atoi |
# atoi(e) == 0 turns off | e[0] == '0' turns off | e[0] == '1' turns on | present | and the special cases
@pytest.mark.parametrize("family,name,want", [
    (0, "FG_FD_FACFUSE", (0, 1, 7, -1)), (0, "FG_DEV_DT", (0, 1, 7, -1)), (0, "FG_BICG3", (0, 1, 7, -1)), (0, "FG_BICG_SUB", (0, 1, 7, -1)),
    (0, "FG_ZMARCH_SB", (0, 1, 7, -1)), (0, "FG_FORCE_ZMARCH", (0, 1, 7, -1)), (0, "FG_JAC_SWEEPS", (0, 1, 7, -1)), (1, "FG_MB_CLUSTER", (0, 1, 7, -1)),
    (0, "FG_FCG_FIRST", (0, 1, 1, 1)), (0, "FG_JAC_SPEC", (0, 1, 1, 1)), (0, "FG_POLL_SPIN", (0, 1, 1, 1)), (1, "FG_POLL_WORDS", (0, 1, 1, 1)),
    (0, "FG_HELM_ROWFORM", (0, 1, 1, 1)), (1, "FG_MB_ONCHIP", (0, 1, 1, 1)), (1, "FG_MB_CL_HALF", (0, 1, 1, 1)), (1, "FG_MB_RUNG_ILU", (0, 1, 1, 1)),
    (1, "FG_MB_PCG_KERNEL", (0, 1, 0, 0)), (1, "FG_MB_TRACE", (1, 1, 1, 1)), (1, "FG_MB_TRACE_FAIL", (1, 1, 1, 1)),
    (0, "FG_JAC_WARM", (0, 1, 1, 1)), (1, "FG_MB_BICG_VEC4", (0, 31, 7, -1)), (1, "FG_MB_ML_TRY_CAP", (200, 1, 7, 200)), (0, "FG_PROF_PERIOD", (64, 1, 7, 64)),
    (0, "FG_ADV_JACOBI", (0, 1, 7, -1)), (1, "FG_ADV_JACOBI", (0, 1, 7, -1))])
def test_parse_rules_give_the_members_of_the_three_old_rules(family, name, want, monkeypatch):
    _no_switches(monkeypatch)
    for text, member in zip(("0", "1", "7", "-1"), want):
        monkeypatch.setenv(name, text)
        got = _values(family)
        assert got[name] == member, (name, text)
        others = {k: v for k, v in got.items() if k != name and not (name == "FG_POLL_SPIN" and k == "FG_POLL_WORDS")}      # (no spinning, no result words)
        assert others == {k: v for k, v in DEFAULTS[family].items() if k in others}


def test_process_scope_tracers_follow_the_off_unless_non_zero_rule():
    """FG_HTRACE / FG_ROCTX are read when the library is loaded: a child process that loads nothing but the library"""
    from fluidgym_amd import _lib as L

    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); buf = ctypes.create_string_buffer(4096); "
            "assert lib.fg_switch_values(0, buf, 4096) == 0; print(buf.value.decode())")
    env = dict(os.environ, FG_HTRACE="7", FG_ROCTX="0")
    out = subprocess.run([sys.executable, "-c", code, L.load()._name], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout)
    assert got["FG_HTRACE"] == 1 and got["FG_ROCTX"] == 0


def test_multi_block_dump_holds_every_switch_of_its_family(monkeypatch):
    from fluidgym_amd import _lib as L

    _no_switches(monkeypatch)
    monkeypatch.setenv("FG_MB_CL_HALF", "0")
    monkeypatch.setenv("FG_ADV_JACOBI", "1")
    lib = L.load()
    h = ctypes.c_void_p()
    assert lib.fg_mb_create(2, 1, -1, ctypes.byref(h)) == 0
    try:
        cfg = L.read_json(lib.fg_mb_config_dump, h)
        assert set(cfg) >= set(_values(1))
        assert not set(cfg) & set(STALE)
        assert cfg["FG_MB_CL_HALF"] == 0 and cfg["FG_ADV_JACOBI"] == 1
        assert {k: cfg[k] for k in DEFAULTS[1]} == dict(DEFAULTS[1], FG_MB_CL_HALF=0, FG_ADV_JACOBI=1)
        assert lib.fg_mb_set_advection_jacobi(h, 0) == 0      # the variable was set: it wins over the call
        assert L.read_json(lib.fg_mb_config_dump, h)["FG_ADV_JACOBI"] == 1
    finally:
        lib.fg_mb_destroy(h)


def test_document_table_and_library_name_the_same_native_switches(monkeypatch):
    _no_switches(monkeypatch)
    doc = open(os.path.join(ROOT, "docs", "SWITCHES.md")).read()
    native = {m.group(1) for m in re.finditer(r"^\| `(FG_\w+)` \|[^|]*\| `fluidgym_amd/csrc/", doc, flags=re.M)}
    assert native == set(_values(0)) | set(_values(1))
    # the environment is read in the table's reader and by the two process-scope tracers, nowhere else
    sites = []
    for path in sorted(glob.glob(os.path.join(ROOT, "fluidgym_amd", "csrc", "*.hip"))):
        sites += [(os.path.basename(path), line.strip()) for line in open(path, errors="replace") if "getenv(" in line]
    assert len(sites) == 3 and sorted(f for f, _ in sites) == ["fg_poll.hip", "fg_poll.hip", "fg_switches.hip"], sites
    assert all(("FG_HTRACE" in line) or ("FG_ROCTX" in line) for f, line in sites if f == "fg_poll.hip")
