import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    from oracle import fixtures

    def load(name):
        return fixtures.load(os.path.join(GOLDEN, name))
    return load


@pytest.fixture(scope="session")
def state_dict0():
    """Seed-0 weights of the build's deterministic generator (shared across tests)."""
    from oracle import weightgen
    return weightgen.gen_state_dict(0)
