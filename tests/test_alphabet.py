"""The alphabet of a `char` corpus is chosen in one header without HIP calls (rapidfuzz_rs_amd/csrc/rf_alphabet.hpp), which the host packer and the device road of
rf_corpus_pack_u32 both call: tests/cpp/alphabet_check.cpp holds it to a naive re-statement of the rule -- rank by count descending then symbol ascending, 254
ids in rank order, the rest overflow, narrow iff nothing at or above 0xFFFF, 0xFFFFFFFF refused -- for 0, 1, 254, 255 and 300 distinct symbols with ties across
ranks 253/254, 0xFFFF / 0xFFFE, symbols above the BMP, the reserved symbol and counts above 2^32, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_alphabet_choice_against_a_naive_restatement(tmp_path):
    exe = str(tmp_path / "alphabet_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I",
                    os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "alphabet_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "alphabet ok: 40 cases" in out, out  # 5 alphabet sizes x 8 variations
