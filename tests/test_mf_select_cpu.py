"""The launch choice of the multifrontal path (csrc/mf_select.cpp) without a GPU and without the library:
tests/select_smoke.cpp is compiled once per session together with mf_select.cpp under the address and undefined-behaviour
sanitizers and run as a child process per switch set.  Every line it prints -- the census names, the front kernel over the
whole domain (tiles 1 .. 15, small, narrow, big_lds), the solve-side kernels, the switches as read from the environment --
is compared with the independent mirror tests/mf_select_ref.py; and mf_same_selection is held to mf_select_front: two
launches it calls equal get the same kernel and image under every switch set, which is what the deferral pass of
mf_build_plan relies on."""
from __future__ import annotations

import itertools
import os
import subprocess

import pytest

import mf_select_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the variants of tests/test_gpu_mf_structures.py (ENV_VARIANTS) and of tests/test_gpu_front_packed.py (HALF_WAVES)
ENV_VARIANTS = [{}, {"SQPHIP_MF_STATIC_MIN": "1"}, {"SQPHIP_MF_STATIC": "0"},
                {"SQPHIP_MF_TOP2": "0", "SQPHIP_MF_LEVEL2": "0", "SQPHIP_MF_BIG_LDSIMG": "0"},
                {"SQPHIP_MF_NW4": "0", "SQPHIP_MF_NW8": "0"}, {"SQPHIP_MF_SPINE": "1"}]
HALF_WAVES = {"SQPHIP_MF_NW4": "0", "SQPHIP_MF_NW8": "0"}
SWITCH_SETS = ENV_VARIANTS + [HALF_WAVES] + [{"SQPHIP_MF_STATIC_MIN": v} for v in "123"] + \
    [{"SQPHIP_MF_STATIC_MAX": "8"}, {"SQPHIP_MF_V1": "1"}, {"SQPHIP_MF_F2_PACKED": "0"}, {"SQPHIP_MF_FRONT_PACKED": "0"}] + \
    [{"SQPHIP_MF_NW4": v} for v in "0123"]
SOLVE_SETS = [{}, {"SQPHIP_MF_LEVEL2": "0"}, {"SQPHIP_MF_GENERIC": "1"}, {"SQPHIP_MF_LEVEL2": "0", "SQPHIP_MF_GENERIC": "1"},
              {"SQPHIP_MF_INERTIA_KERNEL": "1"}]
# field -> environment name: every switch of MfSwitches and MfPlanSwitches
SWITCH_ENV = {"values_serial": "SQPHIP_MF_VALUES_SERIAL", "v1": "SQPHIP_MF_V1", "stat": "SQPHIP_MF_STATIC", "f2_packed": "SQPHIP_MF_F2_PACKED",
              "front_packed": "SQPHIP_MF_FRONT_PACKED", "static_min": "SQPHIP_MF_STATIC_MIN", "static_max": "SQPHIP_MF_STATIC_MAX",
              "nw4": "SQPHIP_MF_NW4", "nw8": "SQPHIP_MF_NW8", "big_ldsimg": "SQPHIP_MF_BIG_LDSIMG", "generic": "SQPHIP_MF_GENERIC",
              "level2": "SQPHIP_MF_LEVEL2", "inertia_kernel": "SQPHIP_MF_INERTIA_KERNEL", "inertia_serial": "SQPHIP_INERTIA_SERIAL"}
PLAN_ENV = {"big_solve": "SQPHIP_MF_BIG_SOLVE", "top": "SQPHIP_MF_TOP", "top_narrow": "SQPHIP_MF_TOP_NARROW", "merge_t": "SQPHIP_MF_MERGE_T",
            "no_level_merge": "SQPHIP_MF_NO_LEVEL_MERGE", "top2": "SQPHIP_MF_TOP2", "spine": "SQPHIP_MF_SPINE", "defer": "SQPHIP_MF_DEFER",
            "sym_dump": "SQPHIP_SYM_DUMP"}
DESCRIPTORS = list(itertools.product(range(1, 16), (0, 1), (0, 1)))       # (tiles, small, narrow)


@pytest.fixture(scope="session")
def prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("select_smoke") / "select_smoke"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "select_smoke.cpp"),
                           os.path.join(ROOT, "sqpsolver.jl_amd", "csrc", "mf_select.cpp")])
    return str(exe)


def run(prog, sections, env):
    """the program's lines as lists of fields, under an environment without any SQPHIP_ variable but those of `env`"""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SQPHIP_")}
    r = subprocess.run([prog, sections] + [f"{k}={v}" for k, v in env.items()], capture_output=True, text=True, timeout=60, env=clean)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]            # (a sanitizer report ends the program with one)
    return [ln.split("\t") for ln in r.stdout.splitlines()]


def ids(env):
    return ",".join(f"{k[7:]}={v}" for k, v in env.items()) or "default"


def test_the_census_names_are_the_list_in_its_order(prog):
    got = run(prog, "n", {})
    assert [int(f[1]) for f in got] == list(range(len(REF.KERNEL_NAMES)))
    assert [f[2] for f in got] == REF.KERNEL_NAMES
    assert not [k for k in REF.KERNEL_NAMES if "solve_inst" in k]


@pytest.mark.parametrize("env", SWITCH_SETS, ids=ids)
def test_the_front_kernel_over_the_whole_domain(prog, env):
    sw = REF.switches(env)
    got = run(prog, "f", env)
    assert len(got) == 15 * 8
    choice = {}
    for tag, T, small, narrow, big, name, packed in got:
        key = (int(T), int(small), int(narrow), int(big))
        assert tag == "front" and key not in choice
        choice[key] = (name, bool(int(packed)))
        assert choice[key] == REF.select_front(*key, sw), (key, choice[key])
        assert name in REF.FACTOR_SIDE and name != "k_mf_spine"
    assert sorted(choice) == sorted((T, s, n, b) for (T, s, n) in DESCRIPTORS for b in (0, 1))
    # what the deferral pass relies on: launches that count as the same selection run the same kernel with the same image
    same = run(prog, "p", env)
    assert len(same) == len(DESCRIPTORS) ** 2
    pairs = set()
    for f in same:
        a, b, eq = tuple(map(int, f[1:4])), tuple(map(int, f[4:7])), bool(int(f[7]))
        pairs.add((a, b))
        assert f[0] == "same" and eq == REF.same_selection(a, b), (a, b)
        if eq:
            for big in (0, 1):
                assert choice[a + (big,)] == choice[b + (big,)], (env, a, b, big)
    assert pairs == set(itertools.product(DESCRIPTORS, DESCRIPTORS))


@pytest.mark.parametrize("env", SOLVE_SETS, ids=ids)
def test_the_solve_side_kernels(prog, env):
    sw = REF.switches(env)
    got = run(prog, "s", env)
    want = [["level", str(w), str(h), *REF.select_solve_level(w, h, sw)] for w in (-1, 0, 100) for h in (0, 1)]
    want += [["top", str(n), str(c), REF.select_top(n, c, sw)] for n in (0, 3) for c in (0, 3)]
    want += [["inertia", str(s), str(n), str(int(REF.top_tests_inertia(s, n, sw)))] for s in (0, 1) for n in (0, 3)]
    assert got == want


def _printed(value):
    return -1 if value is None else int(value)


@pytest.mark.parametrize("value", [None, "0", "1", "2", "x"], ids=lambda v: "unset" if v is None else v)
def test_the_reader_parses_every_switch_as_the_expressions_it_replaced(prog, value):
    """one switch at a time: unset, "0", "1", "2" and a string without a number"""
    for field, name in list(SWITCH_ENV.items()) + list(PLAN_ENV.items()):
        env = {} if value is None else {name: value}
        sw, ps = REF.switches(env), REF.plan_switches(env)
        want = [["switch", f, str(_printed(getattr(sw, f)))] for f in SWITCH_ENV] + [["plan", f, str(_printed(getattr(ps, f)))] for f in PLAN_ENV]
        assert run(prog, "w", env) == want, (name, value)
        if value is None:
            break


def test_the_defaults_are_the_member_initialisers(prog):
    got = {(f[0], f[1]): int(f[2]) for f in run(prog, "w", {})}
    assert got == {("switch", "values_serial"): 0, ("switch", "v1"): 0, ("switch", "stat"): 1, ("switch", "f2_packed"): 1,
                   ("switch", "front_packed"): 1, ("switch", "static_min"): -1, ("switch", "static_max"): 12, ("switch", "nw4"): 3,
                   ("switch", "nw8"): 1, ("switch", "big_ldsimg"): 1, ("switch", "generic"): 0, ("switch", "level2"): 1,
                   ("switch", "inertia_kernel"): 0, ("switch", "inertia_serial"): 0, ("plan", "big_solve"): 1, ("plan", "top"): -1,
                   ("plan", "top_narrow"): 0, ("plan", "merge_t"): -1, ("plan", "no_level_merge"): 0, ("plan", "top2"): 1,
                   ("plan", "spine"): 0, ("plan", "defer"): 1, ("plan", "sym_dump"): 0}
