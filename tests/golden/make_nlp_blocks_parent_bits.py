"""Records tests/golden/nlp_{block,rowblock,softmax,cox,lse}_parent_bits.npz: f, grad, g, jval, hval of acopf_eval for every
evaluation of tests/nlp_blocks_parent_cases.py, from whichever library the package loads.  The committed records come from the
library of the commit before the block families were put on shared building blocks (nlp_blocks_dev.hpp), loaded through
SQPHIP_SO; tests/test_gpu_nlp_blocks_parent_bits.py holds every later library to them bit for bit.  Needs a GPU.

Run:  SQPHIP_SO=<the parent's libsqphip.so> python tests/golden/make_nlp_blocks_parent_bits.py [directory to write to]

The script also checks that the call without the Hessian pointer files the same f, grad, g and jval as the full call: the
records stand for both."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
import nlp_blocks_parent_cases as PC                                  # noqa: E402


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for family in PC.FAMILIES:
        rec = {}
        for name, build in PC.case_list(family):
            for b, ev, no in PC.run_case(pkg, build):
                for k in PC.KEYS:
                    rec["%s/%d/%s" % (name, b, k)] = np.asarray(ev[k])
                    assert np.all(np.isfinite(rec["%s/%d/%s" % (name, b, k)])), (family, name, b, k)
                    assert k == "hval" or np.array_equal(np.asarray(no[k]), np.asarray(ev[k])), (family, name, b, k)
        path = os.path.join(out_dir, os.path.basename(PC.golden_path(".", family)))
        np.savez_compressed(path, **rec)
        print(family, len(rec) // len(PC.KEYS), "evaluations,", sum(v.size for v in rec.values()), "doubles,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
