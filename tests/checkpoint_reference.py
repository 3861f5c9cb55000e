"""Numpy restatement of the checkpoint digest (csrc/hdg_checkpoint.hpp, csrc/hdg_digest.hpp): for the 64-bit patterns b_i of n
doubles, d0 = sum b_i and d1 = sum b_i (2 i + 1), both mod 2^64 (numpy's uint64 arithmetic wraps).  Also the vectors the digest
tests use and the fixed test vector the host program is checked against."""
import numpy as np

# lengths around the wave (64), the workgroup (256) and its pair (512) boundaries, odd and even, and one length beyond what a
# single grid of 4096 workgroups x 256 threads x 2 words covers (the kernel's second trip)
GRID_WORDS = 4096 * 256 * 2
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 255, 256, 257, 2 ** 16 + 3, GRID_WORDS + 5)


def digest(v):
    """(d0, d1) as Python ints of a float64 (or uint64) array"""
    b = np.ascontiguousarray(v).reshape(-1).view(np.uint64)
    w = np.arange(b.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over="ignore"):
        return int(b.sum(dtype=np.uint64)), int((b * w).sum(dtype=np.uint64))


def digest_bytes(data):
    """the digest of host bytes: little-endian words, the last one zero-padded"""
    data = bytes(data) + b"\0" * (-len(data) % 8)
    return digest(np.frombuffer(data, dtype="<u8"))


def digest_of_digests(ds):
    return digest(np.array([x for d in ds for x in d], dtype=np.uint64))


def patterns(kind, n, seed=0):
    """n doubles given by their bit patterns: `random` words, `nan` NaNs with payloads, `zeros` +-0, `denormal` subnormals,
    `ones` all-ones words (every sum wraps)"""
    rng = np.random.default_rng(1234 + seed)
    if kind == "random":
        b = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    elif kind == "nan":
        b = np.uint64(0x7FF0000000000000) | rng.integers(1, 2 ** 52, size=n, dtype=np.uint64) | (rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63))
    elif kind == "zeros":
        b = rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)
    elif kind == "denormal":
        b = rng.integers(1, 2 ** 52, size=n, dtype=np.uint64)
    elif kind == "ones":
        b = np.full(n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    else:
        raise KeyError(kind)
    return b.view(np.float64)


KINDS = ("random", "nan", "zeros", "denormal", "ones")


def fixed_words(n):
    """the words the host program digests too (tests/host/checkpoint_check.cpp: same recurrence)"""
    out = np.empty(n, dtype=np.uint64)
    x = 88172645463325252
    m = 2 ** 64 - 1
    for i in range(n):
        x ^= (x << 13) & m
        x ^= x >> 7
        x ^= (x << 17) & m
        out[i] = x
    return out
