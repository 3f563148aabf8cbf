#!/usr/bin/env python3
"""Pins random_permutation (csrc/index.hip: 64-bit Philox keys, the eight-pass stable radix sort): for a fixed seed, the SHA-256 of
the int64 bytes of random_permutation(n), n = 2048, 2049, 16385, 100000 drawn in that order, from the CPU test double, which runs
the same Philox code and sorts the keys with std::stable_sort; tests/test_index_paths.py replays the draws on both targets.
(A file of its own: further draws in make_rng_golden.py would shift the stream pinned in rng_stream.npz.)
    python tests/golden/make_perm_golden.py        -> tests/golden/rng_permutation.json"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

SEED = 20261018
SIZES = (2048, 2049, 16385, 100000)


def draw(nd):
    """The permutations, one per size, in call order."""
    prev = nd.device_rng(True, seed=SEED)
    try:
        return [nd.random_permutation(n).get() for n in SIZES]
    finally:
        nd.device_rng(prev)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, os.path.dirname(HERE))
    import conftest
    lib, gpu = conftest.bound_library()
    assert not gpu, "generate on the CPU test double"
    from minidiff_amd import ndarray as nd
    digests = {str(n): hashlib.sha256(p.tobytes()).hexdigest() for n, p in zip(SIZES, draw(nd))}
    with open(os.path.join(HERE, "rng_permutation.json"), "w") as f:
        json.dump({"seed": SEED, "sizes": list(SIZES), "sha256": digests}, f, indent=1)
        f.write("\n")
    print("written")
