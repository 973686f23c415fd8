"""`rapidfuzz::distance` (src/distance.rs:1-10): the metric modules that have a bit-parallel batch path."""
from .. import _native as _N
from .._comparator import MetricModule as _M

levenshtein = _M("levenshtein", _N.LEVENSHTEIN, False)    # src/distance/levenshtein.rs
indel = _M("indel", _N.INDEL, False)                      # src/distance/indel.rs
lcs_seq = _M("lcs_seq", _N.LCS_SEQ, False)                # src/distance/lcs_seq.rs
osa = _M("osa", _N.OSA, False)                            # src/distance/osa.rs
damerau_levenshtein = _M("damerau_levenshtein", _N.DAMERAU_LEVENSHTEIN, False)  # src/distance/damerau_levenshtein.rs
hamming = _M("hamming", _N.HAMMING, False)                # src/distance/hamming.rs (Args().pad(True): hamming.rs:112-118)
prefix = _M("prefix", _N.PREFIX, False)                   # src/distance/prefix.rs
postfix = _M("postfix", _N.POSTFIX, False)                # src/distance/postfix.rs
jaro = _M("jaro", _N.JARO, True)                          # src/distance/jaro.rs
jaro_winkler = _M("jaro_winkler", _N.JARO_WINKLER, True)  # src/distance/jaro_winkler.rs

__all__ = ["levenshtein", "indel", "lcs_seq", "osa", "damerau_levenshtein", "hamming", "prefix", "postfix", "jaro", "jaro_winkler"]
