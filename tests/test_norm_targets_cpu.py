"""nlp_block_targets (csrc/model_plans.cpp), the plan builder behind sqphip_nlp_add_norm_block, without a GPU and without the
library: tests/norm_targets_smoke.cpp is compiled together with model_plans.cpp under the address and undefined-behaviour
sanitizers and run as a child process.  The program checks the distinct targets in order of first appearance, the CSR list of
a target's outputs in rising order, the Jacobian slots per (target, column) with a duplicated COO entry, every refusal (row out
of range, linear row, missing Jacobian entry) and R = 5000 outputs on three targets."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_builder_of_the_norm_blocks_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "norm_targets_smoke"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "norm_targets_smoke.cpp"),
                           os.path.join(ROOT, "sqpsolver.jl_amd", "csrc", "model_plans.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "ok\n", (r.stdout[-2000:], r.stderr[-2000:])
