"""The test tree's own layout (CPU, source text only): no file under tests/ or tools/ imports a test module — what
more than one file needs lives in a support module (keyed_cases.py, gpu_cases.py, torsion_model.py, joint_model.py,
abi_model.py, isa_asm.py, reference_checks.py), imported once under one name — and the helpers that used to exist
in several copies are defined in one file each."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) +
               glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True))
PREFIX = "test" + "_"  # (in two pieces: this file's own text must not match)
# `import a, <test module> as b`, `from <test module> import ...`, with or without a package in front; anywhere in
# the text, so the programs that tests hand to child processes as strings count
IMPORTS = re.compile(r"^[ \t]*(?:import\s+(?:[\w.]+(?:\s+as\s+\w+)?\s*,\s*)*(?:\w+\.)*%s\w+|from\s+(?:\w+\.)*%s\w+\s+import\b)"
                     % (PREFIX, PREFIX), re.M)
ONE_HOME = ("_diff", "_poison", "_sign_items", "_dev", "_dev_col", "_mixed_arrays", "_dual", "_pick", "_patterns")


def test_no_file_imports_a_test_module():
    assert len(FILES) > 80
    found = [(os.path.relpath(f, ROOT), m.group(0).strip()) for f in FILES for m in IMPORTS.finditer(open(f).read())]
    assert not found, found


def test_the_pattern_sees_every_form():
    forms = ("import %sx as T", "    import %sx", "from %sx import a, b", "import os, %sx as T", "import a as b, c.%sx",
             "from tests.%sx import y")
    for form in forms:
        assert IMPORTS.search("x = 1\n" + form % PREFIX + "\n"), form
    for text in ("import pytest", "from keyed_cases import _dev", "# import %sx" % PREFIX, "import testing_x"):
        assert not IMPORTS.search(text), text


def test_shared_helpers_have_one_home():
    homes = {name: [] for name in ONE_HOME}
    for f in FILES:
        if os.path.relpath(f, ROOT).startswith("tests"):
            for name in re.findall(r"^[ \t]*def (\w+)\(", open(f).read(), re.M):
                if name in homes:
                    homes[name].append(os.path.relpath(f, ROOT))
    assert all(len(v) == 1 for v in homes.values()), homes
