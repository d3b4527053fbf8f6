"""Which kernels a bign batch runs (bee2_amd/csrc/bign_plan.hpp) without a GPU: tests/hostshim/bign_plan_main.cpp is built by g++ from the
header alone -- no HIP, no mock -- and holds verify_plan, finish_plan, onekey_plan, mulbase_plan and sign_wg to the decision table, row by
row, at every switch of the batch size and its two neighbours, on the three curves and under every override the tests force.  Built
twice, each a process of its own: plain, and ASan + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "hostshim")


CXX = ["g++", "-std=c++17", "-O1", "-g", "-Wall"]


def _build(tmp_path, name, flags=()):
    out = tmp_path / name
    subprocess.check_call(CXX + list(flags) + ["-o", str(out), os.path.join(SHIM, "bign_plan_main.cpp")])
    return str(out)


def _run_clean(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bign plan ok" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    for word in ("AddressSanitizer", "runtime error"):
        assert word not in r.stderr, r.stderr[-6000:]


def test_bign_plans_match_the_decision_table(tmp_path):
    _run_clean(_build(tmp_path, "bign_plan_plain"))


def test_bign_plans_under_asan_and_ubsan(tmp_path):
    """a shift or a product that overflows at 2^24 signatures is a runtime error here (no skip where gcc's sanitizer runtimes are
    missing: the build fails there, and so does the test)"""
    _run_clean(_build(tmp_path, "bign_plan_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
