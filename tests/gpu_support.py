"""The fixtures of the GPU tests.  A test module imports them by name; each stays module-scoped, so every module still gets an
engine (a context) of its own, closed when the module is done."""
import pytest

from tests.library_support import M  # noqa: F401 (a fixture, imported from here by the GPU tests)


@pytest.fixture(scope="module")
def eng(M):
    e = M.Engine(0)           # raises when the HIP extension or the GPU is missing: no fallback
    yield e
    e.close()


def fresh_engine(M, monkeypatch, chunk):
    with monkeypatch.context() as mp:
        if chunk:
            mp.setenv("BLSBN254_CHUNK_LANES", chunk)
        return M.Engine(0)
