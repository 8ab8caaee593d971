"""The refusals of the mesh and TSDF entry points, status and full ``lvdgs_last_error()`` text, against a recording.

The refusal tables of tests/test_mesh_eval.py, test_mesh_cull.py, test_mesh_depth.py, test_tsdf.py and test_tsdf_blocks.py assert a
status and a few words of each message; every case of them also comes here, where the status and the whole text are compared with
``tests/golden/mesh_tsdf_refusals.json``: what is refused, and in which words, is part of the interface.  A parametrised case is
filed under its pytest id, a case of a loop under the test's name and its number in the order of the test's calls (``Numbered``).

``python tests/refusal_recording.py`` records the file anew from the library in place (a build known to be good).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mesh_tsdf_refusals.json")
MODULES = ["test_mesh_eval.py", "test_mesh_cull.py", "test_mesh_depth.py", "test_tsdf.py", "test_tsdf_blocks.py"]

RECORD = None      # a dict while the file is being recorded
_golden = None


def check(key, status, error):
    """A refusal a test has just seen: it is the recorded one (or, while recording, becomes it)."""
    global _golden
    error = error.decode() if isinstance(error, bytes) else error
    assert status != 0 and error, key
    if RECORD is not None:
        assert key not in RECORD, key
        RECORD[key] = {"status": int(status), "error": error}
        return
    if _golden is None:
        _golden = json.load(open(GOLDEN))
    assert (int(status), error) == (_golden[key]["status"], _golden[key]["error"]), key


class Numbered:
    """The refusals of one test's loops, filed in the order of its calls; a call that is not refused takes no number."""

    def __init__(self, name):
        self.name, self.n = name, 0

    def __call__(self, status, error):
        if status != 0:
            check("%s#%d" % (self.name, self.n), status, error)
            self.n += 1


if __name__ == "__main__":
    import pytest
    sys.path.insert(0, HERE)
    import refusal_recording as rr      # (the module the tests import, not __main__)
    rr.RECORD = {}
    status = pytest.main(["-q", "-p", "no:cacheprovider", "-k", "refusals", "-m", "not gpu"] + [os.path.join(HERE, m) for m in MODULES])
    assert status == 0, status
    with open(GOLDEN, "w") as f:
        json.dump(rr.RECORD, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(rr.RECORD), "refusals recorded")
