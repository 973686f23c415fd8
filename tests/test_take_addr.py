"""rf_take_addr.hpp -- where a candidate's symbols sit in a packed corpus -- is shared by the kernels of rf_corpus_take and the host: tests/cpp/take_addr_check.cpp
includes it with the host compiler, packs each shape with rf_corpus_layout_host and rebuilds every candidate from the layout with the header's functions alone, byte
for byte, checking as well that no payload byte is read by two candidates and that every byte nobody reads is padding.  Shapes: one length each of 1, 15, 16, 17,
20 and 64 with n = 64 * 3 - 27; ragged 0..64 with n = 3001, three empty candidates and whole exact tiles of 20 / 33 / 64; lengths 0..300 with n = 200; all 256 byte
values; and the ragged shape again under RF_NO_MIXED_TILES=1 in a child process (partial exact tiles).  Once plainly, once under the host sanitizers."""
import os
import subprocess
import sys

import pytest

from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "take_addr_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def exe(request, tmp_path_factory):
    N.lib()
    out = str(tmp_path_factory.mktemp("take_addr") / f"take_addr_check_{request.param}")
    libdir = os.path.dirname(N.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-Wall", *FLAGS[request.param], "-o", out, SRC, "-L", libdir, "-lrfgpu", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, *args, **env):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env={**os.environ, **env})
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failures 0" in r.stdout
    return r.stdout


def test_every_candidate_is_rebuilt_from_the_layout_with_the_header_alone(exe):
    out = _run(exe)
    for length in (1, 15, 16, 17, 20, 64):
        assert f"single length {length} " in out
    for name in ("lengths 0..300", "five symbols", "ragged 0..64 "):
        assert name in out
    assert out.count(": ok") == 9


def test_the_same_without_mixed_tiles(exe):
    out = _run(exe, "ragged", RF_NO_MIXED_TILES="1")
    assert "mixed blocks   0" in out and out.count(": ok") == 1


def test_the_kernels_and_the_host_compile_the_checked_header():
    csrc = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")
    kernel = open(os.path.join(csrc, "rf_take.hip")).read()
    assert '#include "rf_take_addr.hpp"' in kernel and "take_chunk_at(" in kernel and "take_chunk_fill(" in kernel
    host = open(os.path.join(csrc, "rf_api_take.hip")).read()
    assert '#include "rf_take_addr.hpp"' in host and "take_byte_at(" in host and "take_inverse_sigma(" in host
    assert "__device__" not in open(os.path.join(csrc, "rf_take_addr.hpp")).read().replace("__host__ __device__", "")
