"""CPU tests of the C-ABI boundary: the HIP library loads without a GPU, exports every symbol that
include/sqphip.h declares (and nothing is declared that is not exported), argument validation that
needs no device work behaves, and the product never routes through oracle/."""
import ctypes as C
import os
import re

import numpy as np

import pytest

import sqpsolver_jl_amd as pkg
from sqpsolver_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header="sqphip.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sqphip_[a-z0-9_]+)\s*\(", src)))


def test_library_loads_and_exports_every_declared_symbol():
    _lib.build()
    L = _lib.lib()
    declared, hooks = _declared(), _declared("sqphip_test_hooks.h")
    assert len(declared) >= 25 and not set(declared) & set(hooks)
    missing = [s for s in declared + hooks if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(_lib.EXPORTS) == sorted(declared + hooks)
    # the test hooks stay out of the boundary: the Julia shim binds none of them
    jl = open(os.path.join(ROOT, "julia", "SqpHip.jl")).read()
    assert not [h for h in hooks if h in jl]


def test_options_defaults_mirror_parameters_jl():
    o = pkg.default_options()
    # /root/reference/src/parameters.jl:17-29
    assert (o.tol_direction, o.tol_residual, o.tol_infeas) == (1e-8, 1e-8, 1e-8)
    assert (o.max_iter, o.init_mu, o.max_mu, o.tr_size, o.use_soc) == (3000, 1.0, 1e10, 10.0, 0)
    assert (o.rho, o.eta, o.tau, o.min_alpha) == (0.8, 0.4, 0.9, 1e-6)
    assert o.literal_quirks == 1


def test_tr_update_needs_no_device():
    """sqp_trust_region.jl:529-538, :574-577 -- pure scalar logic of the ABI."""
    L = _lib.lib()
    acc, dn = C.c_int32(), C.c_double()
    assert L.sqphip_tr_update(1.0, 2.0, 10.0, 10.0, 1e8, 1e-8, C.byref(acc), C.byref(dn)) == 0
    assert acc.value == 1 and dn.value == 20.0                # accepted at the boundary: radius doubles
    L.sqphip_tr_update(1.0, 2.0, 10.0, 3.0, 1e8, 1e-8, C.byref(acc), C.byref(dn))
    assert acc.value == 1 and dn.value == 10.0                # interior step: radius kept
    L.sqphip_tr_update(-1.0, 2.0, 10.0, 3.0, 1e8, 1e-8, C.byref(acc), C.byref(dn))
    assert acc.value == 0 and dn.value == 1.5                 # rejected: half of min(delta, |p|)
    L.sqphip_tr_update(1.0, -2.0, 1e-9, 1e-9, 1e8, 1e-8, C.byref(acc), C.byref(dn))
    assert acc.value == 0 and dn.value == 1e-9                # floor 0.1 * tol_direction
    L.sqphip_tr_update(1.0, 2.0, 9e7, 9e7, 1e8, 1e-8, C.byref(acc), C.byref(dn))
    assert dn.value == 1e8                                    # capped at delta_max


def test_create_rejects_bad_arguments_before_touching_the_device():
    L = _lib.lib()
    import numpy as np
    h = C.c_void_p()
    o = pkg.default_options()
    one = np.array([1], dtype=np.int64)
    lp = C.POINTER(C.c_int64)
    dp = C.POINTER(C.c_double)
    z = np.zeros(1)
    inf = np.array([np.inf]); ninf = np.array([-np.inf])
    d = lambda a: a.ctypes.data_as(dp)
    l = lambda a: a.ctypes.data_as(lp)
    # row unbounded on both sides
    rc = L.sqphip_create(C.byref(h), 1, 1, 0, 1, l(one), l(one), 0, l(one), l(one), d(z), d(z), d(ninf), d(inf),
                         C.byref(o), 1)
    assert rc == -1
    bad = np.array([7], dtype=np.int64)                       # index out of range
    rc = L.sqphip_create(C.byref(h), 1, 1, 0, 1, l(bad), l(one), 0, l(one), l(one), d(z), d(z), d(z), d(z),
                         C.byref(o), 1)
    assert rc == -1
    assert L.sqphip_create(C.byref(h), 0, 1, 0, 0, l(one), l(one), 0, l(one), l(one), d(z), d(z), d(z), d(z),
                           C.byref(o), 1) == -1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "libsqphip.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_product_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pkgdir = os.path.join(ROOT, "sqpsolver.jl_amd")
    for dirpath, _, files in os.walk(pkgdir):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".h")):
                text = open(os.path.join(dirpath, fn)).read()
                code = "\n".join(ln for ln in text.splitlines()
                                 if not ln.strip().startswith(("#", "//", "*", '"""', "The oracle")))
                assert "from oracle" not in code and "import oracle" not in code, fn
                assert "liboracle" not in code and "sqp_oracle.h" not in code, fn


def test_armijo_and_mu_rules_host_logic():
    """sqp_line_search.jl:270-334 -- scalar/host logic of the (upstream unreachable) line-search merit path."""
    import ctypes as C
    L = _lib.lib()
    PHI = C.CFUNCTYPE(C.c_double, C.c_double, C.c_void_p)
    L.sqphip_armijo_alpha.argtypes = [C.c_double] * 7 + [PHI, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    calls = []
    # phi(alpha) = (alpha - 0.3)^2 along the step: phi0 = 0.09, D = -0.6; Armijo with eta = 0.4, tau = 0.5
    phi = PHI(lambda a, u: (calls.append(a), (a - 0.3) ** 2)[1])
    al, ok = C.c_double(), C.c_int32()
    assert L.sqphip_armijo_alpha(0.09, -0.6, 0.4, 0.5, 1e-4, 1.0, 1e-8, phi, None, C.byref(al), C.byref(ok)) == 0
    assert calls == [1.0, 0.5, 0.25] and al.value == 0.25 and ok.value == 1      # 0.0025 <= 0.09 - 0.06
    # tiny direction: no evaluation, alpha = 1
    calls.clear()
    assert L.sqphip_armijo_alpha(0.09, -0.6, 0.4, 0.5, 1e-4, 1e-9, 1e-8, phi, None, C.byref(al), C.byref(ok)) == 0
    assert calls == [] and al.value == 1.0 and ok.value == 1
    # never sufficient decrease: alpha falls below min_alpha -> invalid
    up = PHI(lambda a, u: 1.0 + a)
    assert L.sqphip_armijo_alpha(1.0, -1.0, 0.4, 0.5, 0.2, 1.0, 1e-8, up, None, C.byref(al), C.byref(ok)) == 0
    assert ok.value == 0 and al.value == 0.125                                  # 1, .5, .25, .125 (< 0.2: stop)
    dp = C.POINTER(C.c_double)
    L.sqphip_compute_mu_rule.argtypes = [C.c_int32, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, dp, dp]
    lam = np.array([0.5, -3.0, 0.0]); t = (2.0 + 1.0) / max((1 - 0.5) * 4.0, 1e-8)     # = 1.5
    for rule, it, want in ((1, 5, [1.5, 3.0, 1.5]), (2, 1, [1.5, 1.5, 1.5]), (2, 2, [1.0, 3.0, 1.0]), (3, 7, [1.0, 3.0, 1.0])):
        mu = np.ones(3)
        assert L.sqphip_compute_mu_rule(rule, it, 0.5, 4.0, 2.0, 1.0, 3, lam.ctypes.data_as(dp), mu.ctypes.data_as(dp)) == 0
        assert mu.tolist() == want, (rule, it, mu)
    mu = np.ones(3)
    assert L.sqphip_compute_mu_rule(1, 1, 0.5, 0.0, 2.0, -9.0, 3, lam.ctypes.data_as(dp), mu.ctypes.data_as(dp)) == 0
    assert mu[0] == 2.0 / 1e-8                                                   # denominator floor, negative curvature dropped
    assert L.sqphip_compute_mu_rule(4, 1, 0.5, 1.0, 1.0, 1.0, 3, lam.ctypes.data_as(dp), mu.ctypes.data_as(dp)) != 0


def test_plain_c_caller_sees_the_same_abi(tmp_path):
    """tests/c_abi_smoke.c (gcc, dlopen, no Python): struct sizes and option defaults field by field, the host-only
    entry points.  Its GPU part (the toy NLP through sqphip_qp_solve) runs under -m gpu."""
    import subprocess
    from sqpsolver_jl_amd import _lib
    exe = tmp_path / "c_abi_smoke"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi_smoke.c")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Werror", "-o", str(exe), src, "-ldl", "-lm"])
    out = subprocess.run([str(exe), _lib.SO_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and "c_abi_smoke: ok" in out.stdout, out.stderr


def test_julia_shim_mirrors_the_options_struct():
    """julia/SqpHip.jl cannot run here (no Julia); at least its SqpHipOptions must list the fields of sqphip_options in
    order with matching widths, and every symbol it ccalls must be exported."""
    import re
    from sqpsolver_jl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jl = open(os.path.join(root, "julia", "SqpHip.jl")).read()
    body = jl[jl.index("struct SqpHipOptions"):jl.index("end", jl.index("struct SqpHipOptions"))]
    fields = re.findall(r"(\w+)::(Cdouble|Int32)", body)
    want = [(k, "Cdouble" if t is C.c_double else "Int32") for k, t in _lib.Options._fields_]
    assert fields == want
    L = _lib.lib()
    for sym in set(re.findall(r"\(:(sqphip_\w+), LIBSQPHIP\)", jl)):
        assert hasattr(L, sym), sym


def _c_kind(decl: str) -> str:
    """argument class of one C parameter declaration of include/sqphip.h"""
    import re
    d = re.sub(r"/\*.*?\*/", " ", decl, flags=re.S).replace("const", " ").strip()
    stars = d.count("*")
    base = re.sub(r"\b\w+\s*$", "", d.replace("*", " ")).strip() if not d.endswith("*") else d.replace("*", " ").strip()
    base = base.split()[0] if base.split() else d.replace("*", " ").split()[0]
    if "(" in decl:
        return "fnptr"
    table = {"double": "f64", "int32_t": "i32", "int": "i32", "int64_t": "i64", "void": "void", "sqphip_ctx": "ctx",
             "sqphip_options": "opts", "char": "char", "sqphip_counters": "struct", "sqphip_symbolic_stats": "struct",
             "sqphip_mode_counters": "struct"}
    return table.get(base, base) + "*" * stars


def _jl_kind(t: str) -> str:
    t = t.strip()
    table = {"Cdouble": "f64", "Int32": "i32", "Cint": "i32", "Int64": "i64", "Cvoid": "void", "Cstring": "char*",
             "Ptr{Cvoid}": "ctx*", "Ref{Ptr{Cvoid}}": "ctx**", "Ptr{Cdouble}": "f64*", "Ref{Cdouble}": "f64*",
             "Ptr{Int32}": "i32*", "Ref{Int32}": "i32*", "Ref{Cint}": "i32*", "Ptr{Int64}": "i64*", "Ptr{UInt8}": "void*",
             "Ref{SqpHipOptions}": "opts*"}
    return table[t]


def test_julia_ccalls_match_the_header_prototypes():
    """Every `ccall((:sqphip_x, LIBSQPHIP), Ret, (ArgTypes...), ...)` of julia/SqpHip.jl against the prototype of
    sqphip_x in include/sqphip.h: same number of arguments, same C type class per argument, same return class.  (The file
    cannot run here; a wrong width or a missing argument would otherwise only show up as a crash on a maintainer's box.)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "sqphip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"\b(int|void|const char \*)\s*(sqphip_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        parts, depth, cur = [], 0, ""
        for ch in args:
            if ch == "(": depth += 1
            if ch == ")": depth -= 1
            if ch == "," and depth == 0: parts.append(cur); cur = ""
            else: cur += ch
        if cur.strip(): parts.append(cur)
        kinds = [] if [p.strip() for p in parts] == ["void"] else [_c_kind(p) for p in parts]
        protos[name] = ({"int": "i32", "void": "void", "const char *": "char*"}[ret], kinds)
    jl = open(os.path.join(root, "julia", "SqpHip.jl")).read()
    jl = re.sub(r"#[^\n]*", "", jl)
    calls = re.findall(r"ccall\(\(:(sqphip_\w+), LIBSQPHIP\),\s*(\w+),\s*\((.*?)\)\s*(?:,|\))", jl, flags=re.S)
    # the attach wrappers pass their argument-type tuple through a variable `T`
    tvar = re.search(r"\bT = \((Ptr\{Cvoid\}.*?)\)\n", jl, flags=re.S).group(1)
    calls += [(name, ret, tvar) for name, ret in re.findall(r"ccall\(\(:(sqphip_\w+), LIBSQPHIP\),\s*(\w+),\s*T,", jl)]
    assert len(calls) >= 22
    seen = set()
    for name, ret, argt in calls:
        assert name in protos, name
        want_ret, want = protos[name]
        got = [_jl_kind(a) for a in re.findall(r"(?:Ref|Ptr)\{(?:Ptr\{Cvoid\}|\w+)\}|\w+", argt)]
        assert _jl_kind(ret) == want_ret, (name, ret, want_ret)
        norm = lambda k: "ctx*" if k in ("ctx*", "void*") else k          # Ptr{Cvoid} stands for sqphip_ctx* and void*
        assert [norm(k) for k in got] == [norm(k) for k in want], (name, got, want)
        seen.add(name)
    assert {"sqphip_create", "sqphip_qp_solve", "sqphip_gather_status", "sqphip_comm_init", "sqphip_compute_qmodel"} <= seen


def test_julia_soc_call_site_builds_a_fresh_qpdata():
    """QpData(sqp) aliases b === sqp.E (reference sqp.jl:66-79): the SOC call site must not write E_soc through it
    (VERDICT r2 weak #12).  A textual guard, since the file cannot run here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jl = open(os.path.join(root, "julia", "SqpHip.jl")).read()
    body = jl[jl.index("function sub_optimize_soc_hip!"):]
    body = body[:body.index("\nend\n")]
    assert "data.b .=" not in body and "sqp.E_soc, sqp.problem.g_L" in body
    for fn in ("sub_optimize_lp_hip!", "sub_optimize_hip!", "uses_hip"):
        assert f"{fn}(" in jl


def test_no_kernel_takes_its_arguments_through_scratch():
    """Every kernel takes the 1 KB device view `DV` by value.  A kernel whose helpers stop being inlined in one piece gets
    that struct copied to scratch memory for the outlined parts -- 2 KB per lane on the stage kernel when the third
    evaluator went in, -12 % QP/s with identical results.  The build records what the compiler
    reports (sqpsolver.jl_amd/csrc/kernel_resources.json); a few hundred bytes of ordinary spills are tolerated."""
    import json
    if not os.path.exists(_lib.RESOURCES_PATH):
        _lib.build(force=True)
    res = json.load(open(_lib.RESOURCES_PATH))
    assert len(res) >= 40
    worst = {k: v["ScratchSize"] for k, v in res.items() if v.get("ScratchSize", 0) > 256}
    assert not worst, worst
    # the fused vector stages must leave room for one workgroup of 1024 threads per CU
    for k, v in res.items():
        if any(t in k for t in ("k_ipm_head", "k_ipm_mid", "k_ipm_tail", "k_sqp_stage")):
            assert v["VGPRs"] <= 128, (k, v)


def test_bench_starts_its_own_ranks_and_refuses_a_mismatched_launcher():
    """`python bench.py --gpus N` typed without a launcher starts N rank processes itself (the parent touches no GPU) with
    the environment torch.distributed.run would give them; under a launcher whose WORLD_SIZE differs it must not quietly
    measure another rank count and call it N: exit code 2, before anything touches a GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--quick"],
                       env=dict(env, SQPHIP_BENCH_RANK_ECHO="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = sorted((json.loads(ln) for ln in r.stdout.splitlines() if ln.strip()), key=lambda d: d["rank"])
    assert [d["rank"] for d in rows] == [0, 1, 2] and all(d["world"] == 3 and d["local_rank"] == d["rank"] for d in rows)
    assert all(d["master"] == "127.0.0.1" and d["port"] == rows[0]["port"] for d in rows)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="1", RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "torch.distributed.run" in r.stderr and r.stdout.strip() == ""


def test_bench_refuses_zero_steps_and_takes_full_and_dump_outputs():
    """--steps sets the number of timed steps, so 0 (which sqphip_sqp_run reads as "to termination") is refused before
    anything touches a GPU; --full and --dump-outputs are options of every run."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and r.stdout.strip() == ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_acceptable_termination_rules_are_the_same_in_oracle_and_device():
    """The interior-point method ends on `e0 <= tol` or acceptably: 8 iterates within 100 x tol, 15 within 1000 x, 25 within
    10^4 x (the third rule is what lets the 9241-bus line-outage scenarios get past their flat QPs).
    Oracle (oracle/qp_ipm.c, ipm_run) and device (ipm.hip, b_ipm_prepare) must carry the same ladder: the parity tests
    compare their iteration counts."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ora = open(os.path.join(root, "oracle", "qp_ipm.c")).read()
    dev = open(os.path.join(root, "sqpsolver.jl_amd", "csrc", "ipm.hip")).read()
    def ladder(src, tol):
        fac = [float(m) for m in re.findall(r"e0 <= ([0-9.e]+) \* " + re.escape(tol) + r" \? n_acc", src)]
        cnt = [int(m) for m in re.findall(r"n_acc\d? >= (\d+)", src)]
        return fac, sorted(set(cnt))
    fo, co = ladder(ora, "tol")
    fd, cd = ladder(dev, "d.ipm_tol")
    assert fo == fd == [100.0, 1000.0, 1e4], (fo, fd)
    assert co == cd == [8, 15, 25], (co, cd)
