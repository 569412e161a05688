"""Test modules do not import one another: what more than one of them needs lives in a plain module beside them
(tests/cxx_support.py, abi_support.py, gpu_support.py, port_models.py, secp256k1_model.py, merkle_model.py, extremes.py,
redzone.py, oracle_lib.py), so that a test file can be moved or renamed without breaking an unrelated suite, and build() imports
no test.  Reads source text only: the import statements of tests/test_*.py and of __graft_entry__.py.

The exemptions read the engine's TABLE / ALIASING data out of the two large files that define it; nothing else may."""
import ast
import glob
import os
import re

TESTS = os.path.dirname(os.path.abspath(__file__))
EXEMPT = {"test_gpu_aliasing.py": {"test_gpu_redzones"},
          "test_aliasing_model.py": {"test_gpu_aliasing", "test_gpu_redzones", "test_abi"},
          "test_redzone_model.py": {"test_gpu_aliasing", "test_gpu_redzones", "test_abi"}}
SINGLE_COPY = ("settle", "device_entry_points", "declared_symbols", "_newest_header")


def sources():
    return sorted(glob.glob(os.path.join(TESTS, "test_*.py"))) + [os.path.join(os.path.dirname(TESTS), "__graft_entry__.py")]


def imported_modules(path):
    """the top-level name of every module an import statement of the file names, at any depth of the file"""
    with open(path) as fh:
        tree = ast.parse(fh.read(), path)
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            yield from ((a.name.split(".")[0], node.lineno) for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.module:
            yield node.module.split(".")[0], node.lineno


def test_no_test_module_imports_another():
    files = sources()
    assert len(files) > 40 and files[-1].endswith("__graft_entry__.py")
    bad = [f"{os.path.basename(p)}:{line} imports {m}" for p in files for m, line in imported_modules(p)
           if m.startswith("test_") and m not in EXEMPT.get(os.path.basename(p), ())]
    assert not bad, bad


def test_the_shared_helpers_are_defined_once():
    """the helpers that had been copied from file to file stay in the support modules (tests/test_gpu_redzones.py keeps the
    engine's own)"""
    bad = []
    for p in sources()[:-1]:
        if os.path.basename(p) == "test_gpu_redzones.py":
            continue
        with open(p) as fh:
            src = fh.read()
        bad += [f"{os.path.basename(p)} defines {name}" for name in SINGLE_COPY if re.search(r"^\s*def %s\(" % name, src, flags=re.M)]
    assert not bad, bad
