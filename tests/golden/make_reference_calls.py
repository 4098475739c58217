"""Records tests/golden/reference_calls.json.gz: the answers of the reference's own code (oracle/_ref/libdarwin_ref.so)
to every call the CPU tests make of it, so that those tests also run where oracle/_ref cannot be built (the `reflib`
fixture of tests/conftest.py replays them there).  Run where oracle/_ref is built:

    python tests/golden/make_reference_calls.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_py  # noqa: E402

if not oracle_py.ref_available():
    raise SystemExit("oracle/_ref/libdarwin_ref.so is not built: nothing to record from")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_calls.json.gz")


def recorded():
    import gzip
    import json
    if not os.path.exists(GOLDEN):
        return set()
    with gzip.open(GOLDEN, "rt") as f:
        return set(json.load(f))


before = recorded()
rc = subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu", "-k", "reference",
                      "tests/test_dsoft.py", "tests/test_dsoft_model.py", "tests/test_oracle.py", "tests/test_paths_model.py"],
                     cwd=ROOT, env=dict(os.environ, GACT_RECORD_REFERENCE_CALLS="1"))
# the file is rewritten as a whole: a call that was in it and is gone means a test that replays it lost its answer
lost = before - recorded()
if lost:
    print("%d calls recorded before are no longer in %s" % (len(lost), os.path.relpath(GOLDEN, ROOT)))
sys.exit(rc or (1 if lost else 0))
