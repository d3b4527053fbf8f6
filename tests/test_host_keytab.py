"""The one-signer key-table cache (bee2_amd/csrc/bign_keytab.hpp) without a GPU: tests/hostshim/keytab_mock_main.cpp drives it
against tests/hostshim/mockhip -- streams are threads, device memory is the heap, the table "kernel" writes a pattern made from the
key -- through every point of its contract: hits, credit and promotion, a miss under capture, slabs, the slot and the byte bound,
the out-of-memory sweep and its retry, pinned tables, a slab with a holder outside the cache, no hipFree under the cache's lock, and
eight threads on a four-slot cache.  Built three ways, each a process of its own: plain, ASan + UBSan (a table freed too early is a
use after free), TSan (three runs: schedules differ)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "hostshim")


def _rt(name):
    p = subprocess.check_output(["gcc", f"-print-file-name={name}"], text=True).strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


ASAN, UBSAN, TSAN = _rt("libasan.so"), _rt("libubsan.so"), _rt("libtsan.so")
CXX = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]


def _build(tmp_path, name, flags=()):
    out = tmp_path / name
    subprocess.check_call(CXX + list(flags) + ["-I", os.path.join(SHIM, "mockhip"), "-x", "c++", "-o", str(out),
                                               os.path.join(SHIM, "keytab_mock_main.cpp")])
    return str(out)


def _run_clean(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "keytab mock ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    for word in ("AddressSanitizer", "runtime error", "ThreadSanitizer"):
        assert word not in r.stderr, r.stderr[-6000:]


def test_key_table_cache_keeps_its_contract(tmp_path):
    _run_clean(_build(tmp_path, "keytab_plain"))


@pytest.mark.skipif(not (ASAN and UBSAN), reason="gcc's libasan / libubsan not installed")
def test_key_table_cache_under_asan_and_ubsan(tmp_path):
    """every table a call returns is read while it is held, and the pinned ones after every kind of eviction: one freed too early
    is a heap-use-after-free here"""
    _run_clean(_build(tmp_path, "keytab_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.mark.skipif(not TSAN, reason="gcc's libtsan not installed")
def test_key_table_cache_is_race_free_under_tsan(tmp_path):
    exe = _build(tmp_path, "keytab_tsan", ["-fsanitize=thread"])
    for _ in range(3):                                   # schedules differ from run to run
        _run_clean(exe)
