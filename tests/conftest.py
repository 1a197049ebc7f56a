import os
import sys

import pytest

# PyTorch bundles its own HIP runtime: it has to be loaded before libpm_gpu.so pulls in the system one,
# or torch finds no GPU later in the same process (tests that allocate the stream with torch).
try:
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def ref_harness():
    """the reference engines' harness, by its name in oracle/_ref: run where it is built, replayed from the recording
    (tests/refrec.py) where it is not"""
    return "ref_harness"
