import os
import sys

import pytest
# before anything loads libptmi.so: torch ships its own HIP and HSA runtimes and asks for them by a name that the system's
# libamdhip64.so.7 does not answer to, so a torch imported after libptmi.so (as a test that asks torch for the GPU does)
# would put a second pair into the process, and both would tear down the device at exit.  Imported first, torch's pair is
# the one libptmi.so binds to, as in bench.py.
import torch  # noqa: F401,E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "cuda-pathtracer_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session", autouse=True)
def _built():
    """Build the checker (oracle/) and the product library once per session if missing."""
    import subprocess
    if not os.path.exists(os.path.join(ROOT, "oracle", "libptmi_oracle.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    if not os.path.exists(os.path.join(ROOT, "cuda-pathtracer_amd", "libptmi.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-pathtracer_amd"), "-j4"])   # hipcc cross-compiles gfx950 anywhere
    yield
