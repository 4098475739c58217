import gzip
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "darwin-gpu_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    import oracle_py
    return oracle_py.Oracle()


REFERENCE_CALLS = os.path.join(ROOT, "tests", "golden", "reference_calls.json.gz")


class ReferenceCalls:
    """The reference's own answers (oracle_py.RefLib) to the calls the tests make, keyed by the call.  With `live` every
    call goes to the library and is kept for save() (tests/golden/make_reference_calls.py); without it the answers come
    from REFERENCE_CALLS, so that the tests stand where oracle/_ref cannot be built."""

    def __init__(self, live=None):
        self.live, self.calls = live, {}
        if live is None:
            with gzip.open(REFERENCE_CALLS, "rt") as f:
                self.calls = json.load(f)

    def _call(self, name, *args, **kwargs):
        key = hashlib.sha256(repr((name, args, sorted(kwargs.items()))).encode()).hexdigest()
        if self.live is not None:
            self.calls[key] = getattr(self.live, name)(*args, **kwargs)
            return self.calls[key]
        if key not in self.calls:
            pytest.skip("oracle/_ref/libdarwin_ref.so not built and this call is not in %s" % os.path.relpath(REFERENCE_CALLS, ROOT))
        res = self.calls[key]
        return [[tuple(c) for c in q] for q in res] if name == "dsoft_candidates" else res

    def dsoft_candidates(self, *args, **kwargs):
        return self._call("dsoft_candidates", *args, **kwargs)

    def align_with_bt(self, *args, **kwargs):
        return self._call("align_with_bt", *args, **kwargs)

    def gact_line(self, *args, **kwargs):
        return self._call("gact_line", *args, **kwargs)

    def save(self):
        with gzip.GzipFile(REFERENCE_CALLS, "wb", mtime=0) as f:
            f.write(json.dumps(self.calls, sort_keys=True, separators=(",", ":")).encode())


@pytest.fixture(scope="session")
def reflib():
    import oracle_py
    if not oracle_py.ref_available():
        yield ReferenceCalls()
    elif os.environ.get("GACT_RECORD_REFERENCE_CALLS"):
        rec = ReferenceCalls(live=oracle_py.RefLib())
        yield rec
        rec.save()
    else:
        yield oracle_py.RefLib()


@pytest.fixture(scope="session")
def hip_lib_path():
    from gact_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build()
    return engine.LIB_PATH


_BLOCKS = {}


def workload_block(name):
    """a named workload's reads and candidates (gact_amd/workload.py), built once per session: simulating the reads and
    running the D-SOFT restatement takes seconds per block, and several files use the same ones"""
    from gact_amd import workload
    if name not in _BLOCKS:
        _BLOCKS[name] = workload.make_block(name, candidates="dsoft")
    return _BLOCKS[name]
