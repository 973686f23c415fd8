"""What a corpus costs to build: rf_corpus_pack -- ragged HOST bytes + offsets -> a device-resident, scannable corpus -- on the device packer
(rf_pack_ragged.hip, the default from 65536 candidates on) and on the host packer (RF_DEVICE_PACK_MIN=0: round 5's counting sort + byte scatter + one upload), with the
library's own phase timings (RF_PACK_TIMING=1, stderr).  Each packer runs in a process of its own (the switch is read once); the input is generated once and shared.
    python tools/time_pack.py [candidates]          (profiles/pack_r06.txt is this script's output for 100 M)
    python tools/time_pack.py [candidates] --u32 [--device-input]
        `char` corpora (rf_corpus_pack_u32; profiles/pack_u32.txt): candidates of 1..64 symbols over three alphabets -- 62 symbols, 3 000 Zipf-distributed BMP
        symbols, the same plus 1 % symbols above the BMP -- on the device road and on the host road, then the byte rf_corpus_pack of the same shape for scale;
        with --device-input also rf_corpus_pack_u32_device / rf_corpus_pack_device on tensors that already sit in HBM.  Every process makes its own input
        (a Zipf block tiled to size: 13 GB of symbols are cheaper to make than to pass through a file)."""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 100_000_000
ALPHABETS = ("ascii62", "zipf3000", "zipf3000_astral")


def wide_input(alphabet, n):
    """(uint32 symbols, uint64 offsets): n candidates of 1..64 symbols"""
    rng = np.random.default_rng(ALPHABETS.index(alphabet) + 1)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(rng.integers(1, 65, size=n), out=offsets[1:])
    total = int(offsets[-1])
    m = min(total, 1 << 24)
    if alphabet == "ascii62":
        syms = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", dtype=np.uint8).astype(np.uint32)
        block = rng.choice(syms, size=m).astype(np.uint32)
    else:
        syms = rng.permutation(np.arange(0x4E00, 0x9FA0))[:3000].astype(np.uint32)
        w = 1.0 / np.arange(1, 3001) ** 1.1
        block = rng.choice(syms, size=m, p=w / w.sum()).astype(np.uint32)
        if alphabet == "zipf3000_astral":
            hi = rng.random(m) < 0.01
            block[hi] = rng.integers(0x10000, 0x10000 + 5000, size=int(hi.sum())).astype(np.uint32)
    data = np.empty(total, dtype=np.uint32)
    for at in range(0, total, m):
        data[at:at + m] = block[: min(m, total - at)]
    return data, offsets


if "--u32" in sys.argv and "child" in sys.argv:
    import torch

    import rapidfuzz_rs_amd as rf

    alphabet, device_input = sys.argv[sys.argv.index("child") + 1], "--device-input" in sys.argv
    t0 = time.perf_counter()
    data, offsets = wide_input(alphabet, n)
    print(f"{alphabet}: n={n} symbols={len(data) / 1e9:.3f} G ({data.nbytes / 1e9:.2f} GB as u32, made in {time.perf_counter() - t0:.1f} s)", flush=True)
    torch.cuda.synchronize()

    def timed(what, make, nbytes):
        for rep in range(2):  # (call 0 also pays the pinned staging buffers and the first touch of the input's pages)
            print(f"[mark] {what} call {rep}", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            c = make()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"  {what} call {rep}: {dt:.3f} s  ({nbytes / dt / 1e9:.2f} GB/s of input symbols)  device_bytes={c.device_bytes} alphabet={c.alphabet_size()}", flush=True)
            del c

    timed("rf_corpus_pack_u32 (host arrays)", lambda: rf.Corpus.from_ragged_u32(data, offsets), data.nbytes)
    if device_input:
        d, o = torch.from_numpy(data.view(np.int32)).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda()
        timed("rf_corpus_pack_u32_device (tensors in HBM)", lambda: rf.Corpus.from_device_ragged(d, o), data.nbytes)
        del d
    if "--bytes-too" in sys.argv:
        b = data.astype(np.uint8)  # (the low byte: the same shape over u8 elements)
        del data
        timed("rf_corpus_pack (host arrays, u8)", lambda: rf.Corpus.from_ragged(b, offsets), b.nbytes)
        if device_input:
            d = torch.from_numpy(b).cuda()
            timed("rf_corpus_pack_device (tensors in HBM, u8)", lambda: rf.Corpus.from_device_ragged(d, o), b.nbytes)
    sys.exit(0)

if "--u32" in sys.argv:
    extra = [a for a in sys.argv[1:] if a.startswith("--")]
    for alphabet in ALPHABETS:
        for label, env, more in (("device road (default)", {}, ["--bytes-too"] if alphabet == ALPHABETS[0] else []), ("host road (RF_DEVICE_PACK_MIN=0)", {"RF_DEVICE_PACK_MIN": "0"}, [])):
            print(f"==== {alphabet}: {label}", flush=True)
            flags = extra if not env else [a for a in extra if a != "--device-input"]
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n)] + flags + more + ["child", alphabet], env=dict(os.environ, RF_PACK_TIMING="1", **env),
                               capture_output=True, text=True)
            print(r.stdout.rstrip())
            if r.returncode != 0:
                print(f"child exit {r.returncode}\n{r.stderr[-2000:]}", flush=True)
                sys.exit(1)
            print("\n".join(ln for ln in r.stderr.splitlines() if ln.startswith("[rf_corpus_pack]") or ln.startswith("[mark]")), flush=True)
    sys.exit(0)

if len(sys.argv) > 2 and sys.argv[2] == "child":
    import torch  # noqa: F401  (pay the one-off import before anything is timed)

    import rapidfuzz_rs_amd as rf
    from rapidfuzz_rs_amd import _native as N

    for kind in ("ragged", "rows64"):
        data, offsets = np.load(os.path.join(sys.argv[3], kind + "_data.npy")), np.load(os.path.join(sys.argv[3], kind + "_off.npy"))
        torch.cuda.synchronize()
        for rep in range(2):  # (the first call also pays the pinned staging buffers / the page faults of the host image)
            t0 = time.perf_counter()
            c = rf.Corpus.from_ragged(data, offsets)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"{kind:7s} n={len(offsets) - 1} payload={data.nbytes / 1e9:.2f} GB  rf_corpus_pack call {rep}: {dt:.3f} s  ({data.nbytes / dt / 1e9:.2f} GB/s of payload)", flush=True)
            if rep == 0:
                q = bytes(data[:40])
                t0 = time.perf_counter()
                rf.distance.levenshtein.BatchComparator(q).many(N.OP_DISTANCE, c, score_cutoff=3)
                t1 = time.perf_counter()
                rf.distance.levenshtein.BatchComparator(q).many(N.OP_DISTANCE, c, score_cutoff=3)
                t2 = time.perf_counter()
                print(f"        first cutoff-3 scan {1e3 * (t1 - t0):.1f} ms (builds the head plane, tile lists), second {1e3 * (t2 - t1):.1f} ms (host results both times)", flush=True)
            del c
    sys.exit(0)

from rapidfuzz_rs_amd.utils import synth  # noqa: E402

with tempfile.TemporaryDirectory(dir="/tmp") as d:
    data, offsets = synth.ragged_host(n, 64, seed=2, min_len=1)
    np.save(os.path.join(d, "ragged_data.npy"), data)
    np.save(os.path.join(d, "ragged_off.npy"), offsets)
    rows = synth.rows_host(n, 64, seed=1)
    np.save(os.path.join(d, "rows64_data.npy"), rows.reshape(-1))
    np.save(os.path.join(d, "rows64_off.npy"), np.arange(0, n * 64 + 1, 64, dtype=np.uint64))
    del data, offsets, rows
    for label, env in (("device packer (default)", {}), ("host packer (RF_DEVICE_PACK_MIN=0)", {"RF_DEVICE_PACK_MIN": "0"})):
        print(f"==== {label}", flush=True)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), "child", d], env=dict(os.environ, RF_PACK_TIMING="1", **env), capture_output=True, text=True)
        print(r.stdout.rstrip())
        print("\n".join(ln for ln in r.stderr.splitlines() if ln.startswith("[rf_corpus_pack]")), flush=True)
