#!/usr/bin/env python3
"""Generates tests/golden/nanoflann_knn.npz -- what the reference tree's own nanoflann (ScanContext module, L2_Simple_Adaptor<float>)
returns for the k-NN cases of tests/test_oracle.py::test_kdtree_against_the_reference_trees_own_nanoflann, so that the test needs
nothing outside this repository.

Per case (the golden pair and two 8k bench pairs, source transformed under both fp32 orders of T * p, plus the target against itself):
a seeded sample of Q query rows (`<case>__sel`, the queries themselves `<case>__q`), the SHA-256 of the target cloud (`<case>__tgt_sha`)
and nanoflann's indices and fp32 squared distances for k in (1, 20) and leaf sizes (10, 15) (`<case>__idx_k<k>_l<leaf>`,
`<case>__d_k<k>_l<leaf>`).  Needs oracle/_ref/libnanoflann_nn.so (oracle/Makefile, built from the reference tree's header where it
lies).  Run:  python tests/golden/make_nanoflann_golden.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref as R  # noqa: E402
from test_oracle import NANOFLANN_KS, NANOFLANN_LEAVES, NANOFLANN_QUERIES, _nanoflann_cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "nanoflann_knn.npz")


def main():
    if R.nanoflann_lib() is None:
        raise SystemExit("oracle/_ref/libnanoflann_nn.so cannot be built: the reference tree's nanoflann.hpp is not present")
    golden = dict(np.load(os.path.join(ROOT, "tests", "golden", "apdgicp_golden.npz")))
    rng = np.random.default_rng(20261016)
    out = {}
    for name, tgt, q in _nanoflann_cases(golden):
        key = name.replace("/", "_")
        sel = np.sort(rng.choice(len(q), size=min(NANOFLANN_QUERIES, len(q)), replace=False)).astype(np.int32)
        qs = np.ascontiguousarray(q[sel], dtype=np.float32)
        out[f"{key}__sel"] = sel
        out[f"{key}__q"] = qs
        out[f"{key}__tgt_sha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(tgt, dtype=np.float32).tobytes()).digest(), dtype=np.uint8)
        for k in NANOFLANN_KS:
            for leaf in NANOFLANN_LEAVES:
                ni, nd = R.nanoflann_knn(tgt, qs, k, leaf)
                out[f"{key}__idx_k{k}_l{leaf}"] = ni
                out[f"{key}__d_k{k}_l{leaf}"] = nd
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
