"""The C++ facade's Corpus::from_device_ragged overloads (include/rapidfuzz_amd.hpp), compiled and run: tests/cpp/device_ragged_facade_test.cpp.  Without a GPU
the argument errors of rf_corpus_pack_device / rf_corpus_pack_u32_device arrive as rapidfuzz::Error; with one, bytes and code points are packed from device
memory through a window, read back, and scored like the corpus the host constructors build."""
import os
import shutil
import subprocess

import pytest

from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    N.lib()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "device_ragged_facade_test")
    libdir = os.path.dirname(N.LIB_PATH)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "device_ragged_facade_test.cpp"),
                    "-o", exe, "-L", libdir, "-lrfgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    return exe


def test_device_ragged_facade_argument_errors_without_a_device(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and "device ragged facade ok (cpu)" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_device_ragged_facade_on_gpu(tmp_path):
    r = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and "device ragged facade ok (gpu)" in r.stdout, r.stdout + r.stderr
