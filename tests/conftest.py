import os
import sys

import pytest
# torch before any test loads the product library: torch brings its own HIP runtime (needed as libamdhip64.so, unversioned), so a process
# that loads the library first maps the ROCm installation's runtime as well -- two HIP / HSA runtimes, and the one that initialises
# second finds no device.  Loaded after torch, the library binds to torch's runtime (same SONAME), as in bench.py.
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle_lib():
    import oracle_binding
    return oracle_binding.lib()
