#!/usr/bin/env python3
"""Golden vectors of the head-size table, generated FROM THE REFERENCE ITSELF in the build container (needs oracle/_ref/libflref.so: `make -C oracle ref`).

  head_sizes.npz   every case of tests/head_sizes.py (int8 at every table size, int16 at one size per class) through the reference's ParallelTransformer::forward:
                   per case the model shape, a checksum of the weights, the prompt, and per call (the prompt, then five greedy steps) the argmax id, the sha256 digest
                   of the logits and the first 16 logits; and the reference's RoPE of the table's seeded vectors at positions 0, 1, 37 and 255 for every table size.
                   Inputs and recorded results only.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
import head_sizes as HS  # noqa: E402
import oracle_py as O  # noqa: E402
from fast_llama_amd import synth  # noqa: E402
from test_head_sizes_host import sha, weights_checksum  # noqa: E402


def main():
    assert O.have_ref(), "build oracle/_ref first: make -C oracle ref"
    out = {}
    for case in HS.CASES:
        hs, qt = case
        name = HS.case_id(case)
        cfg, tensors = HS.model(hs, qt)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.flm")
            synth.write_synthetic_flm(path, cfg, tensors=tensors)
            lgs = HS.greedy_run(O.RefModel(path, qt, threads=2), HS.SHORT_PROMPT, HS.N_GREEDY_REF)
        assert all(np.isfinite(l).all() for l in lgs), name
        out[f"{name}/shape"] = np.array(HS.SHAPES[hs], np.int32)
        out[f"{name}/weights_checksum"] = np.uint64(weights_checksum(tensors))
        out[f"{name}/prompt"] = HS.SHORT_PROMPT
        out[f"{name}/ids"] = np.array([int(np.argmax(l)) for l in lgs], np.int32)
        out[f"{name}/sha256"] = np.stack([sha(l) for l in lgs])
        out[f"{name}/head"] = np.stack([l[:16] for l in lgs]).astype(np.float32)
        print(name, len(lgs), "calls", flush=True)
    R = O.ref()
    out["rope/positions"] = np.array(HS.ROPE_POSITIONS, np.int32)
    for hs in HS.SIZES:
        xs = [HS.rope_input(hs, pos) for pos in HS.ROPE_POSITIONS]
        out[f"rope/hs{hs}/in"] = np.stack(xs)
        out[f"rope/hs{hs}/out"] = np.stack([O.rope(x, pos, lib=R) for x, pos in zip(xs, HS.ROPE_POSITIONS)])
    path = os.path.join(HERE, "head_sizes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
