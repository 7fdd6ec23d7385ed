"""The key census through the C++ host mirror (include/dusk_schnorr.hpp: KeySet*::census): compile
tests/cpp/test_keyed_census.cpp — key objects of a batch against a set of some of the keys: the hits per registered
key, the missed keys with counts and first items, the totals as constructed, and the census again after the busiest
missed key was appended — against libdsv.so and run it on the GPU."""
import os
import subprocess

import pytest

from cpp_build import compile_program


def test_cpp_keyed_census_compiles():
    assert os.path.exists(compile_program("test_keyed_census"))


@pytest.mark.gpu
def test_cpp_keyed_census_matches_the_batch_on_gpu():
    out = subprocess.run([compile_program("test_keyed_census")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
