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
sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu", "-k", "reference",
                          "tests/test_dsoft.py", "tests/test_oracle.py"],
                         cwd=ROOT, env=dict(os.environ, GACT_RECORD_REFERENCE_CALLS="1")))
