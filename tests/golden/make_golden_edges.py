#!/usr/bin/env python3
"""Golden vectors of the value-edge model cases, generated FROM THE REFERENCE ITSELF in the build container (needs oracle/_ref/libflref.so: `make -C oracle ref`).

  value_edges.npz   the tiny and tiny128 model cases of tests/value_edges.py (all families at once, both types; the all-rows-equal classifier) through the
                    reference's ParallelTransformer::forward: per case the tokens fed (all schedules, in order), a checksum of the weights, and per call the argmax
                    id, the sha256 digest of the logits and the first 16 logits.  Recorded results only.
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
import oracle_py as O  # noqa: E402
import value_edges as VE  # noqa: E402
from fast_llama_amd import synth  # noqa: E402
from test_value_edges_host import GOLD_CASES, sha, weights_checksum  # noqa: E402


def main():
    assert O.have_ref(), "build oracle/_ref first: make -C oracle ref"
    out = {}
    for name, shape, qt, fam, layers in GOLD_CASES:
        cfg, tensors = VE.edge_model(shape, qt, fam, layers)
        out[f"{name}/weights_checksum"] = np.uint64(weights_checksum(tensors))
        tokens, lg_all = [], []
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.flm")
            synth.write_synthetic_flm(path, cfg, tensors=tensors)
            m = O.RefModel(path, qt, threads=2, max_batch=512)
            for sname, sch in VE.case_schedules(name, cfg):                  # (every schedule starts at position 0 and reads only the cache rows it wrote)
                lgs = VE.run_schedule(m, sch)
                assert all(np.isfinite(l).all() for l in lgs), (name, sname)
                tokens += [t for t, _ in sch]; lg_all += lgs
        out[f"{name}/tokens"] = np.concatenate(tokens).astype(np.int32)
        out[f"{name}/ids"] = np.array([int(np.argmax(l)) for l in lg_all], np.int32)
        out[f"{name}/sha256"] = np.stack([sha(l) for l in lg_all])
        out[f"{name}/head"] = np.stack([l[:16] for l in lg_all]).astype(np.float32)
        print(name, len(lg_all), "calls", flush=True)
    path = os.path.join(HERE, "value_edges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
