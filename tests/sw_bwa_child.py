"""Child of tests/test_sw_routes_bwa_gpu.py: one bwa-mode launch in a fresh process (switches
the library reads once per process come from the environment), the result arrays to an .npz.
usage: sw_bwa_child.py OUT.npz"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))


def main(out):
    from proovread_amd import _abi, sw
    from test_sw_routes_bwa_gpu import bwa_data
    d = bwa_data(False)
    ctx = _abi.default_context()
    res = sw.run(d.sw_input(), sw.default_opts(False), ctx=ctx)
    rounds, n_ext, n_patch = sw.bwa_stats(ctx)
    np.savez(out, n=res.n, stats=np.array([rounds, n_ext, n_patch]), **{k: res.a[k] for k in res.a})


if __name__ == "__main__":
    main(sys.argv[1])
