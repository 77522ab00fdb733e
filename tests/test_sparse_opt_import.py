"""dir_amd.sparse_opt holds the fused sparse optimisers and dir_amd.ops keeps their names: whichever of the two modules a fresh
interpreter imports first, both name the same objects (ops imports sparse_opt at module level; sparse_opt takes what it needs of ops
inside the constructors)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("SparseAdagrad", "SparseAdam", "SparseFtrl", "share_sorted_entries")


@pytest.mark.parametrize("first,second", [("sparse_opt", "ops"), ("ops", "sparse_opt")])
def test_either_module_may_be_imported_first(first, second):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import dir_amd.%s\nimport dir_amd.%s\n"
            "from dir_amd import ops, sparse_opt\n"
            "assert all(getattr(ops, n) is getattr(sparse_opt, n) for n in %r)\n"
            "print('same objects')\n" % (ROOT, first, second, NAMES))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "same objects", r.stderr[-2000:]
