"""normalized_*_join_topk, the ratio's similarity_join_topk and jaro's *_join_topk of the header-only C++ facade (include/rapidfuzz_amd.hpp) compile against the C
ABI and behave: tests/cpp/join_topk_f64_test.cpp."""
import os
import shutil
import subprocess

import pytest

from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    N.lib()
    exe = str(tmp_path / "join_topk_f64_test")
    libdir = os.path.dirname(N.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "join_topk_f64_test.cpp"),
           "-o", exe, "-L", libdir, "-lrfgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cpp_join_topk_f64_compiles_and_runs_cpu(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and "join_topk_f64 ok (cpu)" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_join_topk_f64_on_gpu(tmp_path):
    r = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and "join_topk_f64 ok (gpu)" in r.stdout, r.stdout + r.stderr
