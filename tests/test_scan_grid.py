"""The grid arithmetic of tests/multitile_rowdp_check.py on the host: the claim "every wavefront owns at least 4 tiles" must not rest on the kernels under test.
tests/cpp/scan_grid_check.cpp restates scan_grid() (rf_scan.hip) as literals -- min(ceil(tiles / 4), CUs x per_cu) -- walks the grid-stride deal wavefront by
wavefront for the corpus sizes the checker derives, and asserts 4 or more tiles per wavefront at one workgroup per CU and, at the default of 32, exactly one for
workgroups of 4 wavefronts (the gap the checker closes) and 4 / waves for the LDS-row launches of fewer -- under AddressSanitizer and UndefinedBehaviorSanitizer.  The restated literals are held to the library's source by text."""
import os
import re
import subprocess

import multitile_lists_check as L
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


def test_list_walking_grids_are_capped_by_the_knob_and_unchanged_without_it():
    """tests/multitile_lists_check.py restates the grids of the launches that walk survivor lists.  Held here to the launchers by text, to the factors they have
    always had when RF_SCAN_BLOCKS_PER_CU is unset (32, 8, 16 and 8 per CU: list_max_grid() returns CUs x min(factor, 32)), and -- with the knob at 1 -- to the
    units per wavefront the checker promises, wavefront by wavefront, for every corpus it sizes from the CU count alone."""
    scan, sparse, band = _text("rf_scan.hip"), _text("rf_sparse.hip"), _text("rf_band.hip")
    assert "int list_max_grid(int per_cu) { return device_cus() * std::min(per_cu, scan_blocks_per_cu()); }" in scan
    assert re.search(r'static int scan_blocks_per_cu\(\)\s*\{\s*static const int per_cu = positive_or\(env_int\("RF_SCAN_BLOCKS_PER_CU", 0\), 32\);\s*return per_cu;\s*\}', scan)
    assert re.search(r"int scan_max_grid\(\)\s*\{\s*const int per_cu = scan_blocks_per_cu\(\);\s*return device_cus\(\) \* per_cu;\s*\}", scan)  # one static for both
    assert "const uint32_t want = (uint32_t)list_max_grid((p.topk_k || p.run_orig) ? 8 : 32), most = (tiles + kWavesPerBlock - 1) / kWavesPerBlock;" in sparse
    assert "const dim3 g(std::max(1u, std::min(want, most))), b(kWave * kWavesPerBlock);" in sparse
    assert "const dim3 g(std::max(1u, std::min((uint32_t)list_max_grid(16), (tiles + kWavesPerBlock - 1) / kWavesPerBlock))), b(kWave * kWavesPerBlock);" in sparse
    assert "const uint32_t pairs = (p.tile_end - p.tile_begin + 1) / 2;" in scan
    assert "std::min<uint32_t>((pairs + kWavesPerBlock - 1) / kWavesPerBlock, std::min<uint32_t>((uint32_t)list_max_grid(16), 4096u));" in scan
    assert "hipLaunchKernelGGL((early_lean_kernel<State, J>), dim3((uint32_t)list_max_grid(8)), b, 0, stream, p2);" in scan
    assert "return std::max(1, std::min(scan_grid(p.tile_end - p.tile_begin), (scan_max_grid() + 1) / 2)); }" in band
    assert "hipLaunchKernelGGL(band_sparse_kernel, dim3(std::max(1, band_grid / 2)), b, lds, stream, p2);" in band
    assert "device_cus() * 8u" not in scan and "device_cus() * 16u" not in scan and "cus * 16u" not in sparse  # no list-walking grid is left beside the helper
    for cus in (32, 256, 304):
        many = 1 << 22  # tiles: a list long enough for every grid to be its cap
        # the knob unset: today's literals
        assert L.list_max_grid(cus, 32) == cus * 32 and L.list_max_grid(cus, 16) == cus * 16 and L.list_max_grid(cus, 8) == cus * 8
        assert L.sparse_lean_grid(many, cus) == cus * 32 and L.sparse_lean_grid(many, cus, small=True) == cus * 8
        assert L.sparse_words_grid(many, cus) == cus * 16 and L.early_list_grid(cus) == cus * 8
        assert L.head_filter_grid(many, cus) == min(cus * 16, 4096)
        assert L.band_grid(many, cus) == cus * 16 and L.band_sparse_grid(many, cus) == cus * 8
        for per_cu in (32, 64, 1000):  # a larger knob leaves them alone too
            assert L.sparse_lean_grid(many, cus, per_cu) == cus * 32 and L.sparse_words_grid(many, cus, per_cu) == cus * 16 and L.early_list_grid(cus, per_cu) == cus * 8
        # a short list: as many workgroups as there are tiles / 4, whatever the knob
        assert L.sparse_lean_grid(5, cus, 1) == L.sparse_lean_grid(5, cus) == 2 and L.sparse_words_grid(0, cus, 1) == 1 and L.head_filter_grid(9, cus, 1) == 2
        # the knob at 1: W wavefronts, and the deal gives every one of them the checker's floor
        W = L.capped_waves(cus)
        for what, units, grid, floor in L.derived_shapes(cus):
            assert grid * L.WAVES == (W if not what.startswith("band") else L.WAVES * max(1, ((cus + 1) // 2) // 2)), (cus, what)
            owned = [len(range(w, units, grid * L.WAVES)) for w in range(grid * L.WAVES)]
            assert min(owned) == L.units_per_wavefront(units, grid) >= floor, (cus, what, min(owned), floor)
            assert L.units_per_wavefront(units - grid * L.WAVES, grid) < L.units_per_wavefront(units, grid)  # (the count can fail)
        # ... while at the default the same corpora leave every wavefront at most one dense tile: the gap
        a = L.tiles_for(10, W)
        assert L.units_per_wavefront(a, L.sparse_lean_grid(a, cus)) <= 1 and L.units_per_wavefront((a + 1) // 2, L.head_filter_grid(a, cus)) <= 1
        for tiles in (L.tiles_for(10, W), L.tiles_for(8, W, 65), L.tiles_for(4, W), L.tiles_for(17, W, 65), L.band_tiles(cus)):
            assert tiles % 2 == 1 and L.candidates_of(tiles) % 64 != 0 and (L.candidates_of(tiles) + 63) // 64 == tiles
        assert L.WAVES * L.head_filter_grid(a, cus, 1) <= 16384  # ListLayout::kMaxSegments
    assert "static constexpr uint32_t kMaxSegments = 16384;" in _text("rf_list_layout.hpp")
