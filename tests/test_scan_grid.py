"""The grid arithmetic of tests/multitile_rowdp_check.py on the host: the claim "every wavefront owns at least 4 tiles" must not rest on the kernels under test.
tests/cpp/scan_grid_check.cpp restates scan_grid() (rf_scan.hip) as literals -- min(ceil(tiles / 4), CUs x per_cu) -- walks the grid-stride deal wavefront by
wavefront for the corpus sizes the checker derives, and asserts 4 or more tiles per wavefront at one workgroup per CU and, at the default of 32, exactly one for
workgroups of 4 wavefronts (the gap the checker closes) and 4 / waves for the LDS-row launches of fewer -- under AddressSanitizer and UndefinedBehaviorSanitizer.  The restated literals are held to the library's source by text."""
import os
import re
import subprocess

import multitile_rowdp_check as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")
CU_COUNTS = (8, 32, 64, 256, 304)  # a CPX partition, a whole MI355X, and counts that are no power of two times anything


def _text(name):
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def test_every_wavefront_owns_four_tiles_at_one_workgroup_per_cu_and_one_at_the_default(tmp_path):
    exe = str(tmp_path / "scan_grid_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "cpp", "scan_grid_check.cpp"), "-o", exe], check=True)
    triples = [t for cus in CU_COUNTS for t in M.derived_sizes(cus)]
    assert {w for _, w, _ in triples} == {1, 2, 4}  # the LDS-row launches of long queries have fewer wavefronts per workgroup: counted with those
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + [str(v) for t in triples for v in t], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert f"scan grid ok: {len(triples)} shapes" in out, out
    # a corpus one workgroup's worth of tiles short of the derived size is refused: the check can fail
    cus, waves, n = 256, 4, M.candidates_for(256, 4)
    r = subprocess.run([exe, str(cus), str(waves), str(n - 64)], capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "owns 3 tiles" in r.stderr, r.stdout + r.stderr
    # the checker's own count agrees with the deal
    for cus, waves, n in triples:
        assert M.tiles_per_wavefront((n + 63) // 64, cus, waves) == M.TILES_PER_WAVE
        assert M.tiles_per_wavefront((n + 63) // 64, cus, waves, per_cu=32) == 4 // waves  # one at 4 wavefronts per workgroup: the gap


def test_restated_grid_and_plan_literals_are_the_sources():
    scan = _text("rf_scan.hip")
    assert 'positive_or(env_int("RF_SCAN_BLOCKS_PER_CU", 0), 32)' in scan  # the default the C++ check calls "32 per CU"
    assert "hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;" in scan  # the CU count is the device's; 256 only when it cannot be read
    assert re.search(r"int scan_grid\(uint32_t n_tiles\)\s*\{\s*return \(int\)std::min<uint32_t>\(\(n_tiles \+ kWavesPerBlock - 1\) / kWavesPerBlock, \(uint32_t\)scan_max_grid\(\)\);", scan)
    assert "return device_cus() * per_cu;" in scan
    assert "constexpr int kWavesPerBlock = 4;" in _text("rf_internal.hpp")
    # plan()'s wavefronts per workgroup of the LDS-row kernels, restated in the checker (dl_waves, wf_waves)
    plan = _text("rf_api_scan.hip")
    assert plan.count("const uint64_t lds_budget = 150u << 10;") == 2 and M.LDS_BUDGET == 150 << 10
    assert "p->wf_waves = (uint32_t)std::min<uint64_t>(kWavesPerBlock, (lds_budget - p->len1 - 16) / row_bytes);" in plan
    assert "p->wf_waves = (uint32_t)std::min<uint64_t>(kWavesPerBlock, (lds_budget - p->len1 - 8) / row_bytes);" in plan
    assert "const uint64_t row_bytes = ((uint64_t)p->len1 + 1) * kWave * sizeof(uint32_t);" in plan
    assert "std::max<uint64_t>(p->len1, 1) * kWave * (p->dl_wide ? sizeof(DlCell16::word) : sizeof(DlCell8::word));" in plan
    cell = _text("rf_dl_cell.hpp")  # 8-bit fields hold strings of up to 2^8 - 2 = 254 symbols: beyond that the 8-byte cells
    assert "kInf = (1u << kBits) - 1u;" in cell and "kMaxLen = kInf - 1u;" in cell and "using DlCell8 = DlCell<uint32_t, 8>;" in cell and "using DlCell16 = DlCell<uint64_t, 16>;" in cell
    # the shapes the checker names reach the plans it names
    assert [M.dl_waves(q, longest) for q, longest, _ in M.DL_SHAPES] == [4, 4, 4, 4, 4, 4, 4, 1, 4]
    assert M.dl_waves(700, 64) == 4 and 700 * 64 * 8 + 700 + 16 > M.LDS_BUDGET  # the global strip
    assert [M.wf_waves(q) for q in M.WF_QUERIES] == [4, 4, 4, 2, 4] and [M.wf_waves(q, reg=False) for q in (16, 32, 64)] == [4, 4, 4]
    assert 701 * 64 * 4 + 700 + 8 > M.LDS_BUDGET
