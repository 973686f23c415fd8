"""The four join calls over `char` corpora on the device road (tests/join_wide_check.py holds the inputs and the checks; every check runs in a child process with
RF_TRACE_PLAN=1, because the road a call took is read from its plan line and the library reads that switch once per process).

  every call            join, join_f64, join_topk, join_topk_f64 over two `char` corpora that rank their symbols differently: results equal the CPU oracle's over a
                        byte image of the symbols; only the 65-symbol row goes per query
  self-join             one `char` handle on both sides: `upper`, `no_self`, unordered and repeated rows
  overflow class        rows that hold an overflow-class symbol go per query, the others fuse; two different rare symbols never match each other
  overflow across       the class on the queries' side only, on the scanned side only, on both
  mixed kinds           bytes x `char`, `char` x bytes, and a symbol above 0xFF against a byte corpus: the per-query road's error, outputs untouched
  borders               RF_JOIN_BATCH=8 with 1 .. 17 rows; RF_SCAN_BLOCKS_PER_CU=1; RF_JOIN=0: identical results with every row per query"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "join_wide_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0 and "FAILURES 0" in r.stdout and "FAILED" not in r.stdout, r.stdout[-6000:] + r.stderr[-3000:]
    return r


def test_every_call_fuses_two_char_corpora():
    _child("calls")


def test_self_join_of_a_char_corpus():
    _child("self")


def test_rows_with_overflow_symbols_go_per_query_and_the_rest_fuse():
    _child("overflow")


def test_overflow_class_on_either_side_or_both():
    _child("across")


def test_mixed_corpus_kinds():
    _child("mixed")


def test_batch_borders():
    _child("batch", RF_JOIN_BATCH="8")


def test_one_workgroup_per_cu_over_several_tiles():
    _child("calls", RF_SCAN_BLOCKS_PER_CU="1")


def test_join_off_sends_every_row_per_query_with_identical_results():
    _child("calls", RF_JOIN="0")
