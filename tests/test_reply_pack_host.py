"""Host pack / unpack of packed replies (pir_amd/csrc/reply_pack.h) and their wire form (wire_codec.cpp) without a GPU:
tests/cpp/reply_pack_test.cpp, a stand-alone program under AddressSanitizer + UBSan, against vectors the model
(tests/reply_pack_model.py) writes here."""
import os
import struct
import subprocess

import numpy as np

import reply_pack_model as rpm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = [2, 30, 36, 37, 43, 49, 60, 61]


def _moduli(w):
    """Moduli of width w (the model and the host code need no primes): the smallest, 2^(w-1) + 1, and the largest, 2^w."""
    return [(1 << (w - 1)) + 1, 1 << w]


def write_vectors(path):
    rng = np.random.default_rng(68)
    cases = []
    for w in WIDTHS:
        for N in (64, 192):
            for q in _moduli(w):
                assert rpm.width(q) == w
                top = q - 1
                for x in (rng.integers(0, top, size=N, dtype=np.uint64, endpoint=True),
                          np.full(N, top, dtype=np.uint64),
                          np.array([0, top] * (N // 2), dtype=np.uint64),
                          np.array([0] * (N - 1) + [1], dtype=np.uint64)):
                    cases.append((w, N, q, x, rpm.pack_poly(x, w)))
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for w, N, q, x, p in cases:
            f.write(struct.pack("<QQQQ", w, N, q, p.shape[0]))
            f.write(x.astype("<u8").tobytes())
            f.write(p.astype("<u8").tobytes())
    return len(cases)


def test_host_pack_and_wire_form_under_sanitizers(tmp_path):
    exe, vec = str(tmp_path / "reply_pack_test"), str(tmp_path / "vectors.bin")
    assert write_vectors(vec) == len(WIDTHS) * 2 * 2 * 4
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-Wextra", os.path.join(ROOT, "tests", "cpp", "reply_pack_test.cpp"),
                    os.path.join(ROOT, "pir_amd", "csrc", "wire_codec.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "reply_pack_test OK" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def test_one_header_serves_codec_client_and_context():
    """Host pack and unpack live in reply_pack.h alone: the codec, the client and the context include it."""
    csrc = os.path.join(ROOT, "pir_amd", "csrc")
    for name in ("wire_codec.h", "ctx.hip"):
        with open(os.path.join(csrc, name)) as f:
            assert '#include "reply_pack.h"' in f.read(), name
    for name in ("client.cpp", "wire_codec.cpp", "wire.cpp", "ctx.hip"):
        with open(os.path.join(csrc, name)) as f:
            src = f.read()
        assert "rpk::" in src and "inline bool unpack_poly" not in src, name
