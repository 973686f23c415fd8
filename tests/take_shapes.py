"""The corpora the take tests share (tests/test_take_host_layout.py, tests/test_gpu_take.py): lists of `bytes`, made once per process.
Candidates are drawn over all 256 byte values, 0 included and skewed, so the renaming is a full permutation that moves the byte 0 too."""
import functools

import numpy as np

SINGLE_LENGTHS = (1, 15, 16, 17, 20, 64)
N_SINGLE = 64 * 3 - 27
N_RAGGED = 3001


def _draw(rng, lengths):
    total = int(np.sum(lengths))
    skew = (rng.integers(0, 7, total) * 37) % 256
    data = np.where(rng.integers(0, 3, total) > 0, skew, rng.integers(0, 256, total)).astype(np.uint8).tobytes()
    ends = np.cumsum(lengths)
    return [data[int(e) - int(l):int(e)] for l, e in zip(lengths, ends)]


@functools.lru_cache(maxsize=None)
def shape(name):
    """'len<L>': N_SINGLE candidates of one length; 'ragged': 0..64, n = 3001, three empty candidates, whole exact tiles of 20 / 33 / 64 (and
    leftovers of each); 'long': 0..300, n = 200 (19 chunk rows, mixed blocks sized for their longest lane)."""
    rng = np.random.default_rng(sum(name.encode()) + 7)
    if name.startswith("len"):
        return _draw(rng, np.full(N_SINGLE, int(name[3:])))
    if name == "long":
        lengths = rng.integers(0, 301, 200)
        lengths[:2] = (300, 0)
        return _draw(rng, lengths)
    assert name == "ragged"
    lengths = np.concatenate([np.zeros(3, int), np.full(64 + 9, 20), np.full(128 + 1, 33), np.full(64, 64)])
    lengths = np.concatenate([lengths, rng.integers(1, 65, N_RAGGED - len(lengths))])
    rng.shuffle(lengths)
    return _draw(rng, lengths)


NAMES = tuple(f"len{l}" for l in SINGLE_LENGTHS) + ("ragged", "long")
