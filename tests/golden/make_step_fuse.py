"""tests/golden/step_fuse.npz: the solves of tests/_step_cases.py through the bit-exact host emulation of the device
solver (csrc/htp_emusim.cpp), built from the commit BEFORE the step's vector passes were fused (HTP_STEP_FUSE).
tests/test_gpu_step_fuse.py asserts the device returns these doubles bit for bit, so the file is made once from
that older build and never regenerated from the code under test:

    git worktree add /tmp/before <commit before HTP_STEP_FUSE>     # build its emulation library there, then
    python tests/golden/make_step_fuse.py /tmp/before/build/libhtp_emusim.so
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(lib_path):
    import _step_cases as S
    from headland_trajectory_planning_amd import _native
    L = ctypes.CDLL(lib_path)
    L.htp_emusim_obca_solve.argtypes = [ctypes.POINTER(_native.ObcaBatch), ctypes.POINTER(_native.ObcaResult),
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.htp_emusim_obca_solve.restype = ctypes.c_int
    out = {}
    for name in S.CASES:
        pk = _native.PackedBatch([S.instance(name)])
        res = _native.HostResults(pk.batch, pk.n_var)
        b, r = pk.struct(), res.struct()
        assert L.htp_emusim_obca_solve(ctypes.byref(b), ctypes.byref(r), None, None, 0) == 0
        out.update({f"{name}_x": res.x[0], f"{name}_objective": res.objective[:1], f"{name}_status": res.status[:1],
                    f"{name}_iters": res.iterations[:1], f"{name}_n_factor": res.n_factor[:1],
                    f"{name}_n_resto": res.n_resto[:1]})
        print(name, "status", res.status[0], "iters", res.iterations[0], "n_factor", res.n_factor[0], "n_resto",
              res.n_resto[0], flush=True)
    np.savez(S.FIXTURE, **out)


if __name__ == "__main__":
    main(sys.argv[1])
