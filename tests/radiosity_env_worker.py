"""Worker for tests/test_gpu_radiosity_ragged.py: launch_radiosity_iteration reads PTMI_RADIOSITY_ROWS and
PTMI_RADIOSITY_TILE_ROWS once per process, so the kernels they select run in a fresh process that its parent starts with
the variable set.  Solves ragged_scenes.ENV_CASES on the GPU and writes one .npz per case into the directory given as the
only argument; the parent compares them with the oracle."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "cuda-pathtracer_amd", "python"))
import ptmi  # noqa: E402
import ragged_scenes as rs  # noqa: E402


def main():
    out = sys.argv[1]
    R = ptmi.Renderer(0)
    for case in rs.ENV_CASES:
        R.load_scene_arrays(*rs.case_scene(case))
        st = R.run_radiosity_solver(**rs.case_params(case))
        np.savez(os.path.join(out, case + ".npz"), rays=st.rays, pairs=st.pairs, cdfs=R.precomputed_cdfs(), **R.radiosity_solution())
    R.close()


if __name__ == "__main__":
    main()
