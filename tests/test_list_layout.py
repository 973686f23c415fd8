"""The one description of the tile / lane list buffer (rapidfuzz_rs_amd/csrc/rf_list_layout.hpp) holds no HIP call, so the host compiler can include it:
tests/cpp/list_layout_check.cpp sweeps corpus sizes, grids and both list kinds, checks that the regions are in order, disjoint and inside
words_needed(n_tiles), and that every offset equals the expression the launchers and kernels used to spell by hand -- under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_layout_regions_and_literal_offsets(tmp_path):
    exe = str(tmp_path / "list_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "list_layout_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "list layout ok: 120 shapes" in out, out  # 10 corpus sizes x 4 grids x (band + the head filter's two forms)
