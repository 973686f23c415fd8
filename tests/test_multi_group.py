"""The one grouping rule of the multi-query calls (rapidfuzz_rs_amd/csrc/rf_multi_group.hpp: rf_many_multi_*, rf_topk_multi_*, rf_filter_multi_*) holds no HIP call, so
the host compiler can include it: tests/cpp/multi_group_check.cpp enumerates every assignment of {not fusable, key A, key B} to up to 9 queries, members free and
contiguous, and checks the groups property by property against a restatement of the rule -- sizes 2 and 4 of one key, nobody twice, `taken` the union, 5 of a key -> 4 + one
left, 3 -> 2, neighbours when contiguous, groups in ascending order of their first member -- and norm_key_fits (rf_norm_key.hpp) on each side of 65535, under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_group_rule_and_norm_key_fits(tmp_path):
    exe = str(tmp_path / "multi_group_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "multi_group_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "multi group ok: 59048 assignments" in out, out  # 2 x (3^0 + ... + 3^9)
